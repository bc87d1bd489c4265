"""float64 torch-on-CPU restatement of the PPO trainer (include/hk.h "PPO trainer"): the critic, GAE and the loss, with torch autograd for the
gradients.  Inputs come from rollout.stacked_inputs; shared by the CPU and GPU tests."""
import math
import numpy as np
import torch

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def normalise(x, mean, std):
    """the actor's normaliser: clip((x - mean) / std, -5, 5) (identity without one)"""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    if mean is None:
        return x
    m = torch.as_tensor(np.asarray(mean, np.float64))
    s = torch.as_tensor(np.asarray(std, np.float64))
    return torch.clamp((x - m) / s, -5.0, 5.0)


def trunk(x, p, n_layers):
    for l in range(n_layers):
        z = x @ p["W%d" % l].T + p["b%d" % l]
        x = z * torch.sigmoid(z)
    return x


def tensors(d, grad=False):
    return {k: torch.tensor(np.asarray(v, np.float64), requires_grad=grad) for k, v in d.items()}


def critic_values(x, cp, n_layers):
    """x: normalised inputs [..., in_dim]; cp: critic params (torch) -> V [...]"""
    return trunk(x, cp, n_layers) @ cp["W_mu"] + cp["b_mu"][0]


def gae(r, d, v, v_boot, gamma, lambd):
    """r, d, v: [R, ...] (d: DONE != 0), v_boot: [...] -> (A, RET) float64, the recurrences of hk.h"""
    r, v = np.asarray(r, np.float64), np.asarray(v, np.float64)
    nd = 1.0 - (np.asarray(d) != 0).astype(np.float64)
    A = np.zeros_like(v)
    vnext, anext = np.asarray(v_boot, np.float64), np.zeros_like(v[0])
    for t in range(v.shape[0] - 1, -1, -1):
        delta = r[t] + gamma * nd[t] * vnext - v[t]
        A[t] = delta + gamma * lambd * nd[t] * anext
        vnext, anext = v[t], A[t]
    return A, A + v


def normalise_adv(A):
    A = np.asarray(A, np.float64)
    return (A - A.mean()) / (A.std() + 1e-10)


def _heads_and_ratios(ap, cp, la, lc, x, raw, branch, old_c, old_d):
    """-> (mu, logits, v, log_sigma, log_softmax(logits), new logp [m, 2], old logp [m, 2], rho [m, 2]) of the rows of x"""
    h = trunk(x, ap, la)
    mu = h @ ap["W_mu"] + ap["b_mu"][0]
    logits = h @ ap["W_branch"].T + ap["b_branch"]
    v = critic_values(x, cp, lc)
    ls = ap["log_sigma"][0]
    z = (raw - mu) / torch.exp(ls)
    logp_c = -0.5 * z * z - ls - HALF_LOG_2PI
    lsm = torch.log_softmax(logits, dim=-1)
    logp_d = lsm.gather(-1, branch[:, None])[:, 0]
    lp = torch.stack([logp_c, logp_d], 1)
    old = torch.stack([old_c, old_d], 1)
    return mu, logits, v, ls, lsm, lp, old, torch.exp(lp - old)


def _entropy(ls, logits, lsm):
    return 0.5 * math.log(2.0 * math.pi * math.e) + ls - (torch.softmax(logits, -1) * lsm).sum(-1)


def entropy(ap, la, x):
    """H [m] of the actor's two distributions at the rows of x: 0.5 log(2 pi e) + log_sigma, plus the categorical's"""
    logits = trunk(x, ap, la) @ ap["W_branch"].T + ap["b_branch"]
    return _entropy(ap["log_sigma"][0], logits, torch.log_softmax(logits, dim=-1))


def loss(ap, cp, la, lc, x, raw, branch, old_c, old_d, adv, v_old, ret, eps, beta):
    """The minibatch loss L = L_pi + 0.5 L_v - beta mean H over the rows of x (torch float64 tensors) -> (L, stats dict, heads)"""
    mu, logits, v, ls, lsm, lp, old, rho = _heads_and_ratios(ap, cp, la, lc, x, raw, branch, old_c, old_d)
    A = adv[:, None]
    L_pi = -torch.min(rho * A, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * A).mean()
    clipped = v_old + torch.clamp(v - v_old, -eps, eps)
    L_v = torch.max((ret - v) ** 2, (ret - clipped) ** 2).mean()
    H = _entropy(ls, logits, lsm)
    L = L_pi + 0.5 * L_v - beta * H.mean()
    stats = {"L_pi": L_pi.item(), "L_v": L_v.item(), "entropy": H.mean().item(), "approx_kl": (old - lp).mean().item(),
             "clip_fraction": ((rho - 1.0).abs() > eps).double().mean().item()}
    return L, stats, (mu, logits, v)


def row_terms(ap, cp, la, lc, x, raw, branch, old_c, old_d, adv, v_old, ret, eps, beta):
    """loss()'s inputs -> float64 numpy per row: "rho" [m, 2] (continuous, discrete), "dv" = v - v_old, "f1" = (ret - v)^2,
    "f2" = (ret - v_old - clip(v - v_old, -eps, eps))^2, and the heads "mu" [m], "logits" [m, nb], "v" [m]"""
    with torch.no_grad():
        mu, logits, v, _, _, _, _, rho = _heads_and_ratios(ap, cp, la, lc, x, raw, branch, old_c, old_d)
        clipped = v_old + torch.clamp(v - v_old, -eps, eps)
        out = dict(rho=rho, dv=v - v_old, f1=(ret - v) ** 2, f2=(ret - clipped) ** 2, mu=mu, logits=logits, v=v)
    return {k: a.numpy() for k, a in out.items()}


# classify(): the policy classes of a (row, column) and the value classes of a row
BELOW_LIVE, BELOW_DEAD, ABOVE_DEAD, ABOVE_LIVE, INSIDE = range(5)      # rho below / above the band, by the sign of A: min picks rho A (live) or the clip
V_INSIDE, V_LIVE, V_DEAD = range(3)                                    # |v - v_old| <= eps; clipped with f1 > f2 (max picks f1); clipped with f2 > f1
POLICY_DEAD = (BELOW_DEAD, ABOVE_DEAD)


def classify(terms, adv, eps, margin):
    """row_terms() and the rows' advantages -> dict: "policy" int [m, 2] (BELOW_LIVE .. INSIDE), "value" int [m] (V_INSIDE, V_LIVE, V_DEAD),
    "decided" bool [m].  A row is undecided — a float32 evaluation may take the other side of one of its branches — when a rho lies within
    margin of 1 - eps or 1 + eps, |v - v_old| within margin of eps, a clipped value's f1 and f2 agree to margin relatively, or |A| < margin."""
    rho, dv, f1, f2 = (np.asarray(terms[k], np.float64) for k in ("rho", "dv", "f1", "f2"))
    A = np.asarray(adv, np.float64)
    lo, hi = 1.0 - eps, 1.0 + eps
    pos = (A > 0)[:, None]
    policy = np.where(rho < lo, np.where(pos, BELOW_LIVE, BELOW_DEAD), np.where(rho > hi, np.where(pos, ABOVE_DEAD, ABOVE_LIVE), INSIDE))
    clipped = np.abs(dv) > eps
    value = np.where(clipped, np.where(f1 > f2, V_LIVE, V_DEAD), V_INSIDE)
    near = (np.abs(rho - lo) < margin).any(1) | (np.abs(rho - hi) < margin).any(1) | (np.abs(np.abs(dv) - eps) < margin)
    near |= clipped & (np.abs(f1 - f2) <= margin * np.maximum(f1, f2))
    near |= np.abs(A) < margin
    return dict(policy=policy, value=value, decided=~near)


def adam_f32(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """float32 numpy restatement of hk.h's Adam, operation for operation -> (p, m, v)"""
    f = np.float32
    b1, b2, eps, lr = f(b1), f(b2), f(eps), f(lr)
    omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
    c1, c2 = f(1.0 - float(b1) ** step), f(1.0 - float(b2) ** step)
    g = g.astype(np.float32)
    m = b1 * m + omb1 * g
    v = b2 * v + (omb2 * g) * g
    mh = m / c1
    vh = v / c2
    p = p - lr * mh / (np.sqrt(vh) + eps)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)
