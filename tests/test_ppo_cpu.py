"""PPO trainer pieces that need no GPU: the float64 restatement's gradients against finite differences, GAE on a hand-worked case, the row
permutation's host twin, and the hk_ppo_config layout (C, ctypes, C#)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ppo_restate as PR
import test_csharp_layout as CSL
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.ppo import param_layout, permutation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_problem(seed=0, m=9, in_dim=6, Ha=8, La=2, nb=3, Hc=4, Lc=1):
    r = np.random.default_rng(seed)
    ap = {}
    for name, shape in param_layout(in_dim, Ha, La, nb):
        ap[name] = r.standard_normal(shape) * 0.5
    cp = {}
    for name, shape in param_layout(in_dim, Hc, Lc, 0):
        cp[name] = r.standard_normal(shape) * 0.5
    rows = dict(x=r.standard_normal((m, in_dim)), raw=r.standard_normal(m), branch=r.integers(0, nb, m),
                old_c=r.standard_normal(m) * 0.3 - 1.0, old_d=-r.random(m) * 1.5, adv=r.standard_normal(m),
                v_old=r.standard_normal(m), ret=r.standard_normal(m))
    return ap, cp, rows, La, Lc


def _L(ap, cp, rows, La, Lc, eps=0.2, beta=5e-3):
    t = {k: torch.tensor(v) for k, v in rows.items()}
    L, st, _ = PR.loss(ap, cp, La, Lc, t["x"], t["raw"], t["branch"].long(), t["old_c"], t["old_d"], t["adv"], t["v_old"], t["ret"], eps, beta)
    return L


def test_restatement_gradients_match_central_differences():
    ap0, cp0, rows, La, Lc = _small_problem()
    ap, cp = PR.tensors(ap0, True), PR.tensors(cp0, True)
    L = _L(ap, cp, rows, La, Lc)
    L.backward()
    h = 1e-6
    checked = 0
    for params, grads in ((ap0, ap), (cp0, cp)):
        for name, arr in params.items():
            g = grads[name].grad.numpy()
            flat = arr.reshape(-1)
            for k in range(0, flat.size, max(1, flat.size // 7)):
                save = flat[k]
                flat[k] = save + h
                lp = _L(PR.tensors(ap0), PR.tensors(cp0), rows, La, Lc).item()
                flat[k] = save - h
                lm = _L(PR.tensors(ap0), PR.tensors(cp0), rows, La, Lc).item()
                flat[k] = save
                fd = (lp - lm) / (2 * h)
                assert abs(fd - g.reshape(-1)[k]) <= 1e-6 + 1e-5 * abs(fd), (name, k, fd, g.reshape(-1)[k])
                checked += 1
    assert checked > 40


def _off_tie_problem(seed=3, m=600, s=0.25, eps=0.2):
    """_small_problem's networks with a rollout recorded at them (RAW, BRANCH sampled from the heads, the old log-probabilities and V_OLD
    theirs), then every parameter perturbed to p (1 + s xi) (+ 0.1 s xi' on the vectors): rho != 1 and v != v_old.
    -> (ap, cp, rows, La, Lc, eps, classes) over the decided rows only"""
    ap, cp, rows, La, Lc = _small_problem(seed, m)
    r = np.random.default_rng(seed + 100)
    t = {k: torch.tensor(v) for k, v in rows.items()}
    with torch.no_grad():
        a0, c0 = PR.tensors(ap), PR.tensors(cp)
        h = PR.trunk(t["x"], a0, La)
        mu = (h @ a0["W_mu"] + a0["b_mu"][0]).numpy()
        p = torch.softmax(h @ a0["W_branch"].T + a0["b_branch"], -1).numpy()
        v0 = PR.critic_values(t["x"], c0, Lc).numpy()
    rows["raw"] = mu + r.standard_normal(m) * np.exp(ap["log_sigma"][0])
    rows["branch"] = np.array([r.choice(p.shape[1], p=q) for q in p])
    rows["old_c"], rows["old_d"] = np.zeros(m), np.zeros(m)
    t0 = _terms(ap, cp, rows, La, Lc, eps)
    rows["old_c"], rows["old_d"] = np.log(t0["rho"][:, 0]), np.log(t0["rho"][:, 1])      # rho == 1 at the recording parameters
    rows["v_old"] = v0
    rows["ret"] = v0 + r.standard_normal(m)
    for d in (ap, cp):
        for name, a in d.items():
            a *= 1.0 + s * r.standard_normal(a.shape)
            if a.ndim == 1:
                a += 0.1 * s * r.standard_normal(a.shape)
    cl = PR.classify(_terms(ap, cp, rows, La, Lc, eps), rows["adv"], eps, 1e-3)
    keep = cl["decided"]
    rows = {k: v[keep] for k, v in rows.items()}
    return ap, cp, rows, La, Lc, eps, {k: v[keep] for k, v in cl.items()}


def _terms(ap, cp, rows, La, Lc, eps):
    t = {k: torch.tensor(v) for k, v in rows.items()}
    return PR.row_terms(PR.tensors(ap), PR.tensors(cp), La, Lc, t["x"], t["raw"], t["branch"].long(), t["old_c"], t["old_d"], t["adv"], t["v_old"],
                        t["ret"], eps, 0.0)


def test_restatement_gradients_match_central_differences_off_the_tie_point():
    """perturbed parameters: rows in each of the 5 classes of both policy columns and in each of the 3 value classes (classify), none of them
    within 1e-3 of a branch boundary, so that a central difference of width 1e-6 never crosses one"""
    ap0, cp0, rows, La, Lc, eps, cl = _off_tie_problem()
    for q in (0, 1):
        assert np.bincount(cl["policy"][:, q], minlength=5).min() >= 5, np.bincount(cl["policy"][:, q], minlength=5)
    assert np.bincount(cl["value"], minlength=3).min() >= 5 and cl["decided"].all()
    ap, cp = PR.tensors(ap0, True), PR.tensors(cp0, True)
    _L(ap, cp, rows, La, Lc, eps).backward()
    h = 1e-6
    checked = 0
    for params, grads in ((ap0, ap), (cp0, cp)):
        for name, arr in params.items():
            g = grads[name].grad.numpy()
            flat = arr.reshape(-1)
            for k in range(0, flat.size, max(1, flat.size // 7)):
                save = flat[k]
                flat[k] = save + h
                lp = _L(PR.tensors(ap0), PR.tensors(cp0), rows, La, Lc, eps).item()
                flat[k] = save - h
                lm = _L(PR.tensors(ap0), PR.tensors(cp0), rows, La, Lc, eps).item()
                flat[k] = save
                fd = (lp - lm) / (2 * h)
                assert abs(fd - g.reshape(-1)[k]) <= 1e-6 + 1e-5 * abs(fd), (name, k, fd, g.reshape(-1)[k])
                checked += 1
    assert checked > 40


def test_dead_rows_hand_worked_case():
    """four rows whose rho and value terms are set by hand (eps 0.2, beta 0): rho_c = rho_d = 0.5 with A = -2 and rho_c = rho_d = 1.5 with
    A = +3 are dead in both columns — min picks clip(rho) A, a constant: L_pi = -(2 * 0.8 * -2 + 2 * 1.2 * 3) / 4 = -1 — and v = v_old + 0.5,
    ret = v + 1 is value-dead: f1 = 1 < f2 = (1 + 0.3)^2 = 1.69, so L_v = 1.69.  autograd gives exact zeros for the actor and for the critic.
    The live twins (A's signs flipped; ret = v - 1: f1 = 1 > f2 = 0.49) do not."""
    ap0, cp0, rows, La, Lc = _small_problem(1, 4)
    eps = 0.2
    rows["old_c"], rows["old_d"] = np.zeros(4), np.zeros(4)
    t0 = _terms(ap0, cp0, rows, La, Lc, eps)
    target = np.array([0.5, 1.5, 0.5, 1.5])
    rows["old_c"], rows["old_d"] = np.log(t0["rho"][:, 0] / target), np.log(t0["rho"][:, 1] / target)
    rows["adv"] = np.array([-2.0, 3.0, -2.0, 3.0])
    rows["v_old"] = t0["v"] - 0.5
    rows["ret"] = t0["v"] + 1.0
    tm = _terms(ap0, cp0, rows, La, Lc, eps)
    assert np.allclose(tm["rho"], target[:, None], rtol=1e-12) and np.allclose(tm["f1"], 1.0) and np.allclose(tm["f2"], 1.69)
    cl = PR.classify(tm, rows["adv"], eps, 1e-3)
    assert cl["decided"].all() and (cl["value"] == PR.V_DEAD).all()
    assert np.array_equal(cl["policy"][:, 0], [PR.BELOW_DEAD, PR.ABOVE_DEAD] * 2) and np.array_equal(cl["policy"], cl["policy"][:, :1].repeat(2, 1))
    ap, cp = PR.tensors(ap0, True), PR.tensors(cp0, True)
    t = {k: torch.tensor(v) for k, v in rows.items()}
    L, st, _ = PR.loss(ap, cp, La, Lc, t["x"], t["raw"], t["branch"].long(), t["old_c"], t["old_d"], t["adv"], t["v_old"], t["ret"], eps, 0.0)
    L.backward()
    assert abs(st["L_pi"] + 1.0) < 1e-12 and abs(st["L_v"] - 1.69) < 1e-12 and st["clip_fraction"] == 1.0
    for d in (ap, cp):
        for name, p in d.items():
            assert not p.grad.numpy().any(), name
    # the live twins
    rows["adv"] = -rows["adv"]
    rows["ret"] = t0["v"] - 1.0
    tm = _terms(ap0, cp0, rows, La, Lc, eps)
    cl = PR.classify(tm, rows["adv"], eps, 1e-3)
    assert np.array_equal(cl["policy"][:, 0], [PR.BELOW_LIVE, PR.ABOVE_LIVE] * 2) and (cl["value"] == PR.V_LIVE).all() and np.allclose(tm["f2"], 0.49)
    ap, cp = PR.tensors(ap0, True), PR.tensors(cp0, True)
    _L(ap, cp, rows, La, Lc, eps, 0.0).backward()
    for d in (ap, cp):
        assert all(p.grad.numpy().any() for p in d.values())


def test_gae_hand_worked_case():
    """one (e, j), R = 4: DONE = 1 at t = 1, DONE = 2 (time-out) at t = 3 -> the bootstrap is unused; and again with no done at the end"""
    g, lam = 0.5, 0.5
    r = np.array([1.0, 2.0, 3.0, 4.0])[:, None]
    v = np.array([0.5, 1.0, 1.5, 2.0])[:, None]
    d = np.array([0, 1, 0, 2])[:, None]
    A, RET = PR.gae(r, d, v, np.array([100.0]), g, lam)
    # t = 3 terminal: delta = 4 - 2 = 2, A3 = 2;  t = 2: delta = 3 + 0.5 * 2 - 1.5 = 2.5, A2 = 2.5 + 0.25 * 2 = 3.0
    # t = 1 terminal: delta = 2 - 1 = 1, A1 = 1;  t = 0: delta = 1 + 0.5 * 1 - 0.5 = 1.0, A0 = 1 + 0.25 * 1 = 1.25
    assert np.allclose(A[:, 0], [1.25, 1.0, 3.0, 2.0]) and np.allclose(RET[:, 0], [1.75, 2.0, 4.5, 4.0])
    d2 = np.array([0, 1, 0, 0])[:, None]
    A2, _ = PR.gae(r, d2, v, np.array([10.0]), g, lam)
    # t = 3: delta = 4 + 0.5 * 10 - 2 = 7 = A3;  t = 2: delta = 3 + 1 - 1.5 = 2.5, A2 = 2.5 + 0.25 * 7 = 4.25
    assert np.allclose(A2[2:, 0], [4.25, 7.0]) and np.allclose(A2[:2, 0], [1.25, 1.0])
    n = PR.normalise_adv(A)
    assert abs(n.mean()) < 1e-12 and abs(n.std() - 1.0) < 1e-9


@pytest.mark.parametrize("n", [1, 7, 512, 10 ** 5 + 3])
def test_row_permutation_is_a_bijection_and_changes_per_epoch(n):
    p0 = permutation(n, 1234, 0)
    assert p0.min() >= 0 and p0.max() < n
    assert np.array_equal(np.sort(p0), np.arange(n))
    if n >= 7:
        p1 = permutation(n, 1234, 1)
        assert np.array_equal(np.sort(p1), np.arange(n)) and not np.array_equal(p0, p1)
        assert not np.array_equal(p0, permutation(n, 99, 0))


def test_adam_restatement_bias_correction():
    p, g = np.float32([1.0, -2.0]), np.float32([0.5, -0.25])
    p1, m1, v1 = PR.adam_f32(p, g, np.zeros(2, np.float32), np.zeros(2, np.float32), 1, 1e-3)
    # first step with bias correction: m / c1 = g, v / c2 = g^2 -> a step of lr * sign(g) (to eps)
    assert np.allclose(p - p1, 1e-3 * np.sign(g), rtol=1e-3)


def test_ppo_config_layout_c_ctypes_csharp(tmp_path):
    ct = _lib.PpoConfig
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "hk.h"), "int main(){",
             'printf("%zu\\n", sizeof(hk_ppo_config));']
    want = [C.sizeof(ct)]
    for fname, _ in ct._fields_:
        lines.append('printf("%%zu\\n", offsetof(hk_ppo_config, %s));' % fname)
        want.append(getattr(ct, fname).offset)
    lines += ['printf("%d\\n", HK_PPO_STATS);', 'printf("%d\\n", HK_PPO_FIELDS);', 'printf("%d\\n", HK_ABI_VERSION);', "return 0;}"]
    want += [_lib.HK_PPO_STATS, _lib.HK_PPO_FIELDS, _lib.HK_ABI_VERSION]
    src = tmp_path / "ppo.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "ppo"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    # C#: the parser and the layout rule of test_csharp_layout, applied to HkPpoConfig
    structs, imports = CSL._parse_cs()
    fields = structs["HkPpoConfig"]
    assert [f[0] for f in fields] == [n for n, _ in ct._fields_]
    off = 0
    for (name, typ, ptr, cnt), (fname, ftype) in zip(fields, ct._fields_):
        kind, esz, n = CSL._flatten(ftype)
        assert not ptr and CSL.CS_TYPES[typ] == (kind, esz) and cnt == n
        off = (off + esz - 1) // esz * esz
        assert off == getattr(ct, fname).offset
        off += esz * n
    assert off == C.sizeof(ct)
    assert {s for s in _lib.SYMBOLS if s.startswith("hk_ppo_")} <= set(imports)
