"""float64 torch-on-CPU restatement of recurrent training with a recurrent critic (include/hk.h "PPO trainer" RECURRENT CRITIC): the value pass
(the critic run sequentially over the rollout, memory carried) and the loss of a minibatch whose value is the critic's own cell over the window,
started from CRITIC_MEMORY[k].  The windows, the zeroing at FIRST and the dead rows are ppo_lstm_restate.forward's, applied to the critic's
parameters (its value head is W_mu / b_mu); the actor side is ppo_lstm_restate.loss's text with the value replaced.  It imports nothing from
the device path.  `mutate` turns it into one of five deliberately WRONG trainers of the critic."""
import numpy as np
import torch

import ppo_restate as PR
import ppo_lstm_restate as LR

MUTATIONS = ("critic_grad_through_first", "critic_grad_into_initial_memory", "critic_initial_memory_zero", "critic_whh_grad_pre_reset",
             "dead_rows_in_mean")
_FORWARD = {"critic_grad_through_first": "grad_through_first", "critic_grad_into_initial_memory": "grad_into_initial_memory",
            "critic_whh_grad_pre_reset": "whh_grad_pre_reset"}


def value_pass(cp, lc, X, boot, first, done_last, mem_in, L):
    """cp: the critic's parameters (torch float64); X [R, E S, in_dim], boot [E S, in_dim]: NORMALISED stacked inputs (torch); first [R, E S];
    done_last [E S]; mem_in [E S, 2 m_v] -> (v [R, E S], v_boot [E S], critic_memory [ceil(R / L), E S, 2 m_v], mem_out [E S, 2 m_v]), numpy"""
    R = X.shape[0]
    m = cp["W_hh"].shape[1]
    mem = torch.tensor(np.asarray(mem_in, np.float64))
    first = np.asarray(first) != 0
    v, cm = [], []
    with torch.no_grad():
        for t in range(R + 1):
            if t < R and t % L == 0:
                cm.append(mem.numpy().copy())
            if t < R:
                mem = torch.where(torch.tensor(first[t])[:, None], torch.zeros_like(mem), mem)
            else:
                out = torch.where(torch.tensor(np.asarray(done_last) != 0)[:, None], torch.zeros_like(mem), mem).numpy().copy()
            h, c = LR.cell(PR.trunk(X[t] if t < R else boot, cp, lc), mem[:, :m], mem[:, m:], cp)
            mem = torch.cat([h, c], 1)
            v.append((h @ cp["W_mu"] + cp["b_mu"][0]).numpy())
    return np.stack(v[:R]), v[R], np.stack(cm), out


def loss(ap, cp, la, lc, X, memory, critic_memory, first, f, adv, v_old, ret, sids, R, L, E, S, eps, beta, mutate=None):
    """The loss of a minibatch, L = L_pi + 0.5 L_v - beta mean H over its valid rows, v from the critic's cell.  memory [R, E S, 2m]: the
    recorder's MEMORY; critic_memory [ceil(R / L), E S, 2 m_v]: CRITIC_MEMORY; the rest as ppo_lstm_restate.loss.
    -> (L, stats dict, dict(mu, v [L, ms], mem, critic_mem [L, ms, 2 m_*], rowid [L, ms]))"""
    assert mutate is None or mutate in MUTATIONS
    H, MEM, rowid = LR.forward(ap, la, X, memory, first, sids, R, L, E, S)
    cmem = np.zeros((R,) + critic_memory.shape[1:])
    if mutate != "critic_initial_memory_zero":
        cmem[::L] = critic_memory          # forward reads row k L of what it is given
    Hc, CMEM, rowid_c = LR.forward(cp, lc, X, cmem, first, sids, R, L, E, S, _FORWARD.get(mutate))
    assert np.array_equal(rowid, rowid_c)
    Lw, ms = rowid.shape
    live = rowid >= 0
    nseq = LR.n_sequences(R, L, E, S)
    rid = torch.tensor(rowid[live])
    lv = torch.tensor(live)
    hl, hcl = H[lv], Hc[lv]
    T = lambda a: torch.tensor(np.asarray(a, np.float64))[rid]
    mu = hl @ ap["W_mu"] + ap["b_mu"][0]
    logits = hl @ ap["W_branch"].T + ap["b_branch"]
    v = hcl @ cp["W_mu"] + cp["b_mu"][0]
    ls = ap["log_sigma"][0]
    z = (T(f["raw"]) - mu) / torch.exp(ls)
    logp_c = -0.5 * z * z - ls - PR.HALF_LOG_2PI
    lsm = torch.log_softmax(logits, dim=-1)
    logp_d = lsm.gather(-1, torch.tensor(np.asarray(f["branch"]).astype(np.int64))[rid][:, None])[:, 0]
    lp = torch.stack([logp_c, logp_d], 1)
    old = torch.stack([T(f["logp_cont"]), T(f["logp_disc"])], 1)
    rho = torch.exp(lp - old)
    denom = float(max(int(live.sum()), 1))
    if mutate == "dead_rows_in_mean":
        denom = float(max(Lw * sum(1 for s in sids if 0 <= s < nseq), 1))
    A = T(adv)[:, None]
    L_pi = -torch.min(rho * A, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * A).sum() / (2.0 * denom)
    vo, rt = T(v_old), T(ret)
    clipped = vo + torch.clamp(v - vo, -eps, eps)
    L_v = torch.max((rt - v) ** 2, (rt - clipped) ** 2).sum() / denom
    Hent = PR._entropy(ls, logits, lsm)
    Lt = L_pi + 0.5 * L_v - beta * Hent.sum() / denom
    stats = {"L_pi": L_pi.item(), "L_v": L_v.item(), "entropy": (Hent.sum() / denom).item(), "approx_kl": ((old - lp).sum() / (2.0 * denom)).item()}
    full = lambda x: torch.zeros((Lw, ms), dtype=torch.float64).masked_scatter(lv, x.detach()).numpy()
    return Lt, stats, dict(mu=full(mu), v=full(v), mem=MEM.detach().numpy(), critic_mem=CMEM.detach().numpy(), rowid=rowid)
