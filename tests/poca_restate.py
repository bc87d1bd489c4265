"""float64 torch-on-CPU restatement of the POCA trainer (include/hk.h "POCA"): the attention critic (value and counterfactual baselines), the
team reward, the lambda-returns and the loss with both value terms; torch autograd gives the reference gradients.  The actor side is
ppo_restate's.  Shared by the CPU and GPU tests."""
import math
import numpy as np
import torch

import ppo_restate as PR

HEADS = 4


def swish(z):
    return z * torch.sigmoid(z)


def layer_norm(u):
    """(u - mean) / sqrt(var + 1e-5) over the last axis, population variance, no affine"""
    mu = u.mean(-1, keepdim=True)
    var = ((u - mu) ** 2).mean(-1, keepdim=True)
    return (u - mu) / torch.sqrt(var + 1e-5)


def action_features(raw, branch, n_branch):
    """raw [...], branch int [...] -> [..., 1 + n_branch] = [RAW, onehot(BRANCH)]"""
    raw = torch.as_tensor(np.asarray(raw, np.float64))
    b = torch.as_tensor(np.asarray(branch).astype(np.int64))
    return torch.cat([raw[..., None], torch.nn.functional.one_hot(b, n_branch).double()], -1)


def entities(x, a, cp):
    """x [G, S, in], a [G, S, 1 + nb] -> (obs entities, act entities) [G, S, H]"""
    uo = swish(x @ cp["W_obs"].T + cp["b_obs"])
    ua = swish(torch.cat([x, a], -1) @ cp["W_act"].T + cp["b_act"])
    return uo, ua


def attention(u, cp):
    """one sequence per leading index: u [..., S, H] -> (z [..., H], alpha [..., HEADS, S, S])"""
    S, H = u.shape[-2], u.shape[-1]
    n = layer_norm(u)
    lead = u.shape[:-2]
    split = lambda t: t.reshape(*lead, S, HEADS, H // HEADS).transpose(-2, -3)          # [..., HEADS, S, dw]
    q, k, v = (split(n @ cp["W_" + w].T + cp["b_" + w]) for w in ("q", "k", "v"))
    alpha = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(H), -1)
    c = (alpha @ v).transpose(-2, -3).reshape(*lead, S, H)
    o = layer_norm(c @ cp["W_out"].T + cp["b_out"] + n)
    return o.sum(-2) / S, alpha


def head(z, cp, n_layers):
    y = z
    for l in range(n_layers):
        y = swish(y @ cp["W%d" % l].T + cp["b%d" % l])
    return y @ cp["w_val"] + cp["b_val"][0]


def baseline_sequence(uo, ua, i):
    """agent i's baseline sequence: (uo_i, then ua_k for k != i, k ascending) [G, S, H]"""
    S = uo.shape[1]
    return torch.stack([uo[:, i]] + [ua[:, k] for k in range(S) if k != i], 1)


def critic(x, a, cp, n_layers):
    """x [G, S, in] (normalised), a [G, S, 1 + nb] -> (V [G], B [G, S])"""
    uo, ua = entities(x, a, cp)
    V = head(attention(uo, cp)[0], cp, n_layers)
    B = torch.stack([head(attention(baseline_sequence(uo, ua, i), cp)[0], cp, n_layers) for i in range(uo.shape[1])], 1)
    return V, B


def team_reward(r, g):
    """r, g [R, E, S] (the transition forms) -> rho [R, E, S] = sum_k r_k + g_i, float64"""
    r, g = np.asarray(r, np.float64), np.asarray(g, np.float64)
    return r.sum(-1, keepdims=True) + g


def team_reward_f32(r, g):
    """the device's fp32 sum, operation for operation: ((r_0 + r_1) + ...) + g_i"""
    r, g = np.asarray(r, np.float32), np.asarray(g, np.float32)
    acc = r[..., 0].copy()
    for k in range(1, r.shape[-1]):
        acc = (acc + r[..., k]).astype(np.float32)
    return (acc[..., None] + g).astype(np.float32)


def lambda_returns(rho, d, v, v_boot, gamma, lambd):
    """rho [R, E, S], d [R, E] (DONE != 0 terminal), v [R, E], v_boot [E] -> G [R, E, S]:
    G_R = V_R;  G_t = rho_t + gamma (1 - d_t) ((1 - lambd) V_{t+1} + lambd G_{t+1})"""
    rho, v = np.asarray(rho, np.float64), np.asarray(v, np.float64)
    nd = 1.0 - (np.asarray(d) != 0).astype(np.float64)
    G = np.zeros_like(rho)
    vnext = np.asarray(v_boot, np.float64)
    gnext = np.repeat(vnext[:, None], rho.shape[2], 1)
    for t in range(rho.shape[0] - 1, -1, -1):
        G[t] = rho[t] + gamma * nd[t][:, None] * ((1.0 - lambd) * vnext[:, None] + lambd * gnext)
        vnext, gnext = v[t], G[t]
    return G


def clipped_value_loss(v, old, ret, eps):
    clipped = old + torch.clamp(v - old, -eps, eps)
    return torch.max((ret - v) ** 2, (ret - clipped) ** 2).mean()


def loss(ap, cp, la, lc, x, raw, branch, old_c, old_d, adv, v_old, b_old, ret, eps, beta):
    """The minibatch loss over the groups of x [mg, S, in]; every other argument [mg, S] (v_old: the group's value per agent), torch float64.
    L = L_pi + 0.5 (L_v + 0.5 L_b) - beta mean H -> (L, stats dict, (mu, logits, V [mg], B [mg, S]))"""
    mg, S = x.shape[0], x.shape[1]
    fl = lambda t: t.reshape(mg * S, *t.shape[2:])
    xf = fl(x)
    h = PR.trunk(xf, ap, la)
    mu = h @ ap["W_mu"] + ap["b_mu"][0]
    logits = h @ ap["W_branch"].T + ap["b_branch"]
    ls = ap["log_sigma"][0]
    z = (fl(raw) - mu) / torch.exp(ls)
    logp_c = -0.5 * z * z - ls - PR.HALF_LOG_2PI
    lsm = torch.log_softmax(logits, dim=-1)
    logp_d = lsm.gather(-1, fl(branch)[:, None])[:, 0]
    lp = torch.stack([logp_c, logp_d], 1)
    old = torch.stack([fl(old_c), fl(old_d)], 1)
    rho = torch.exp(lp - old)
    A = fl(adv)[:, None]
    L_pi = -torch.min(rho * A, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * A).mean()
    V, B = critic(x, action_features(raw.detach().numpy(), branch.numpy(), logits.shape[1]), cp, lc)
    L_v = clipped_value_loss(V[:, None].expand(mg, S), v_old, ret, eps)
    L_b = clipped_value_loss(B, b_old, ret, eps)
    H = PR._entropy(ls, logits, lsm)
    L = L_pi + 0.5 * (L_v + 0.5 * L_b) - beta * H.mean()
    stats = {"L_pi": L_pi.item(), "L_v": L_v.item(), "L_b": L_b.item(), "entropy": H.mean().item(), "approx_kl": (old - lp).mean().item(),
             "clip_fraction": ((rho - 1.0).abs() > eps).double().mean().item()}
    return L, stats, (mu, logits, V, B)
