"""An independent float64 restatement of a recurrent actor, written from the formulas of include/hk.h "RECURRENT ACTORS" alone: it shares no
code with the host twin (tests/policy_lstm_host_check.cpp) or the kernel, takes torch-layout arrays and uses np.float64, np.tanh and
1 / (1 + np.exp(-z)).  The `mutate` argument turns it into one of four deliberately WRONG actors, which the CPU test uses to prove that its
inputs tell a wrong formula from rounding."""
import numpy as np

MUTATIONS = ("gate_order_iofg", "swap_h_c", "drop_b_hh", "heads_on_c")


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def step(a, obs, mem, mutate=None):
    """a: the dict of Policy.arrays() (W0.., b0.., lstm_W_ih, lstm_W_hh, lstm_b_ih, lstm_b_hh, W_mu, b_mu, W_branch, b_branch and,
    optionally, norm_mean / norm_std); obs [rows, in_dim] stacked oldest first; mem [rows, 2m] = [h | c]
    -> (mu [rows], logits [rows, n_branch], mem_out [rows, 2m]), all float64"""
    assert mutate is None or mutate in MUTATIONS
    d = {k: np.asarray(v, np.float64) for k, v in a.items()}
    x = np.asarray(obs, np.float64)
    mem = np.asarray(mem, np.float64)
    if "norm_mean" in d:
        x = np.clip((x - d["norm_mean"]) / d["norm_std"], -5.0, 5.0)
    l = 0
    while "W%d" % l in d:
        s = x @ d["W%d" % l].T + d["b%d" % l]
        x = s * _sig(s)
        l += 1
    m = d["lstm_W_hh"].shape[1]
    h, c = mem[:, :m], mem[:, m:]
    if mutate == "swap_h_c":
        h, c = c, h
    z = x @ d["lstm_W_ih"].T + h @ d["lstm_W_hh"].T + d["lstm_b_ih"]
    if mutate != "drop_b_hh":
        z = z + d["lstm_b_hh"]
    zi, zf, zg, zo = (z[:, g * m:(g + 1) * m] for g in range(4))
    if mutate == "gate_order_iofg":
        zi, zo, zf, zg = (z[:, g * m:(g + 1) * m] for g in range(4))
    i, f, g, o = _sig(zi), _sig(zf), np.tanh(zg), _sig(zo)
    c2 = f * c + i * g
    h2 = o * np.tanh(c2)
    top = c2 if mutate == "heads_on_c" else h2
    mu = top @ d["W_mu"] + d["b_mu"][0]
    logits = top @ d["W_branch"].T + d["b_branch"]
    return mu, logits, np.concatenate([h2, c2], axis=1)
