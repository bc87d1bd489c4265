"""float64 torch-on-CPU restatement of recurrent training (include/hk.h "PPO trainer" RECURRENT): the training forward over windows of
sequence_length rows, the loss of ppo_restate.py on h', and torch autograd for the gradients.  It carries the windows, the constant initial
memory MEMORY[k L], the zeroing at FIRST (value and gradient) and the dead rows of the last window.  It builds on ppo_restate.py (trunk, critic,
entropy, normaliser) and is cross-checked against policy_lstm_restate.py's single step; it imports nothing from the device path.
The `mutate` argument turns it into one of five deliberately WRONG trainers, which the tests use to prove that their inputs tell a wrong
backward from rounding."""
import numpy as np
import torch

import ppo_restate as PR

MUTATIONS = ("grad_through_first", "grad_into_initial_memory", "whh_grad_pre_reset", "gate_order_iofg", "dead_rows_in_mean")


def n_sequences(R, L, E, S):
    return -(-R // L) * E * S


def cell(a, h, c, p, mutate=None, extra=None):
    """one LSTM cell on the trunk output a [g, H] and the memory (h, c) [g, m] each: hk.h "RECURRENT ACTORS", gates i f g o -> (h', c');
    extra: a term added to the pre-activations (a mutation's)"""
    m = p["W_hh"].shape[1]
    z = a @ p["W_ih"].T + h @ p["W_hh"].T + p["b_ih"] + p["b_hh"]
    if extra is not None:
        z = z + extra
    zi, zf, zg, zo = (z[:, g * m:(g + 1) * m] for g in range(4))
    if mutate == "gate_order_iofg":
        zi, zo, zf, zg = (z[:, g * m:(g + 1) * m] for g in range(4))
    i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
    c2 = f * c + i * g
    return o * torch.tanh(c2), c2


def forward(ap, la, X, memory, first, sids, R, L, E, S, mutate=None):
    """ap: the actor's parameters (torch float64: W0.., b0.., W_ih, W_hh, b_ih, b_hh, heads); X [R, E S, in_dim]: the rows' NORMALISED stacked
    inputs (torch); memory [R, E S, 2m]: the recorder's MEMORY of the actor's slots; first [R, E S]: FIRST; sids: the minibatch's sequence ids.
    -> (H [L, ms, m] the h' of every row, zeros where the row is dead or its sequence skipped; MEM [L, ms, 2m] = [h' | c'], likewise;
        rowid int64 [L, ms], -1 where dead or skipped) — time-major, as the device lays a minibatch out"""
    assert mutate is None or mutate in MUTATIONS
    ES, ms = E * S, len(sids)
    nseq = n_sequences(R, L, E, S)
    m = ap["W_hh"].shape[1]
    memory = np.asarray(memory, np.float64)
    first = np.asarray(first) != 0
    rowid = np.full((L, ms), -1, np.int64)
    out_h = [[None] * ms for _ in range(L)]
    out_c = [[None] * ms for _ in range(L)]
    groups = {}
    for q, s in enumerate(sids):
        if 0 <= s < nseq:
            groups.setdefault(int(s) // ES, []).append(q)
    last = {}                                    # (k, rem) -> [h' | c'] of the window's last live row
    for k in sorted(groups):
        qs = groups[k]
        rem = [int(sids[q]) % ES for q in qs]
        mem0 = torch.tensor(memory[k * L, rem])                     # a constant of the minibatch: no gradient flows into it
        if mutate == "grad_into_initial_memory":
            rows = []
            for i, r in enumerate(rem):
                prev = last.get((k - 1, r))
                rows.append(mem0[i] if prev is None else mem0[i] + (prev - prev.detach()))
            mem0 = torch.stack(rows)
        h, c = mem0[:, :m], mem0[:, m:]
        for tau in range(min((k + 1) * L, R) - k * L):
            t = k * L + tau
            fr = torch.tensor(first[t, rem])[:, None]
            a = PR.trunk(X[t, rem], ap, la)
            h_pre = h
            if mutate == "grad_through_first":                      # the value is zeroed, the gradient is not
                h, c = torch.where(fr, h - h.detach(), h), torch.where(fr, c - c.detach(), c)
            else:
                h, c = torch.where(fr, torch.zeros_like(h), h), torch.where(fr, torch.zeros_like(c), c)
            extra = None
            if mutate == "whh_grad_pre_reset":                      # the same value, W_hh's gradient taken on h before the reset
                extra = (h_pre - h).detach() @ (ap["W_hh"] - ap["W_hh"].detach()).T
            h, c = cell(a, h, c, ap, mutate, extra)
            for i, q in enumerate(qs):
                out_h[tau][q], out_c[tau][q] = h[i], c[i]
                rowid[tau, q] = t * ES + rem[i]
        for i, r in enumerate(rem):
            last[(k, r)] = torch.cat([h[i], c[i]])
    zero = torch.zeros(m, dtype=torch.float64)
    H = torch.stack([torch.stack([zero if x is None else x for x in row]) for row in out_h])
    Cc = torch.stack([torch.stack([zero if x is None else x for x in row]) for row in out_c])
    return H, torch.cat([H, Cc], dim=2), rowid


def loss(ap, cp, la, lc, X, memory, first, f, adv, v_old, ret, sids, R, L, E, S, eps, beta, mutate=None):
    """The loss of a recurrent minibatch, L = L_pi + 0.5 L_v - beta mean H over its valid rows (ppo_restate.loss on h').
    f: dict of the rows' fields by row id (raw, branch, logp_cont, logp_disc; numpy [n]); adv, v_old, ret: numpy [n].
    -> (L, stats dict, dict(mu [L, ms], logits [L, ms, nb], v [L, ms], mem [L, ms, 2m], rowid [L, ms]))"""
    H, MEM, rowid = forward(ap, la, X, memory, first, sids, R, L, E, S, mutate)
    Lw, ms = rowid.shape
    live = rowid >= 0
    nseq = n_sequences(R, L, E, S)
    rid = torch.tensor(rowid[live])
    hl = H[torch.tensor(live)]
    T = lambda a: torch.tensor(np.asarray(a, np.float64))[rid]
    xr = X.reshape(-1, X.shape[-1])[rid]
    mu = hl @ ap["W_mu"] + ap["b_mu"][0]
    logits = hl @ ap["W_branch"].T + ap["b_branch"]
    v = PR.critic_values(xr, cp, lc)
    ls = ap["log_sigma"][0]
    z = (T(f["raw"]) - mu) / torch.exp(ls)
    logp_c = -0.5 * z * z - ls - PR.HALF_LOG_2PI
    lsm = torch.log_softmax(logits, dim=-1)
    logp_d = lsm.gather(-1, torch.tensor(np.asarray(f["branch"]).astype(np.int64))[rid][:, None])[:, 0]
    lp = torch.stack([logp_c, logp_d], 1)
    old = torch.stack([T(f["logp_cont"]), T(f["logp_disc"])], 1)
    rho = torch.exp(lp - old)
    n_live = int(live.sum())
    denom = float(max(n_live, 1))
    if mutate == "dead_rows_in_mean":
        denom = float(max(Lw * sum(1 for s in sids if 0 <= s < nseq), 1))
    A = T(adv)[:, None]
    L_pi = -torch.min(rho * A, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * A).sum() / (2.0 * denom)
    vo, rt = T(v_old), T(ret)
    clipped = vo + torch.clamp(v - vo, -eps, eps)
    L_v = torch.max((rt - v) ** 2, (rt - clipped) ** 2).sum() / denom
    Hent = PR._entropy(ls, logits, lsm)
    Lt = L_pi + 0.5 * L_v - beta * Hent.sum() / denom
    stats = {"L_pi": L_pi.item(), "L_v": L_v.item(), "entropy": (Hent.sum() / denom).item(), "approx_kl": ((old - lp).sum() / (2.0 * denom)).item(),
             "clip_fraction": (((rho - 1.0).abs() > eps).double().sum() / (2.0 * denom)).item(),
             "skipped": float(sum(1 for s in sids if not 0 <= s < nseq))}
    lv = torch.tensor(live)
    full = lambda x, shape: torch.zeros(shape, dtype=torch.float64).masked_scatter(lv.reshape(lv.shape + (1,) * (len(shape) - 2)).expand(shape), x.detach())
    heads = dict(mu=full(mu, (Lw, ms)).numpy(), logits=full(logits, (Lw, ms, logits.shape[1])).numpy(), v=full(v, (Lw, ms)).numpy(),
                 mem=MEM.detach().numpy(), rowid=rowid)
    return Lt, stats, heads
