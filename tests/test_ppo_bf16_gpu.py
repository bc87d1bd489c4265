"""PPO trainer, HK_PPO_PREC_BF16 (include/hk.h "PRECISION"): each product form of ppo_gemm_bf16_kernel against a float64 reference
under a derived bound, the rounding points, a minibatch's gradients and the unchanged-parameter statistics against the fp32 mode, determinism,
that it optimises and publishes, and the refusals.  The env of test_ppo_gpu.py: 24 envs, 2v2 Oval, a 312 -> 256 x 3 and a 128 x 2 actor, R = 90."""
import ctypes as C
import functools

import numpy as np
import pytest

import ppo_bf16_restate as BR
from hierarchicalkarting_amd import _lib, ppo
from hierarchicalkarting_amd.policy import Policy
from parity import assert_bits_equal
from test_ppo_gpu import KW, P, R, _ids, _rows, _torch

pytestmark = pytest.mark.gpu

# Measured on the MI355X over three seeds (_measure(0), _measure(1), _measure(2); the tests print seed 0's): per parameter block the LARGEST
# relative L2 difference of GRAD between the two precisions, and the largest unchanged-parameter statistics in bf16 mode (DESIGN §13 has all
# three seeds).  The tests assert 4 x these; the margin covers the spread over seeds.  a.b_mu and a.log_sigma are one-element sums over all
# rows whose terms cancel under normalised advantages (test_ppo_gpu.py notes the same of b_mu against autograd): their relative difference
# is large on the seed where the sum happens to be small (3.64 and 1.28 were measured) and their cosine is only the sign, so 4 x that says
# little.  They are ALSO held to an absolute bound scaled by the sum of the |terms| they add up (MEASURED_ABS_OVER_TERMS, _one_element_terms).
MEASURED_REL_L2 = {
    "a.W0": 0.0397,
    "a.b0": 0.0427,
    "a.W1": 0.0369,
    "a.b1": 0.0361,
    "a.W2": 0.0347,
    "a.b2": 0.037,
    "a.W_mu": 0.0459,
    "a.b_mu": 3.64,
    "a.log_sigma": 1.28,
    "a.W_branch": 0.0157,
    "a.b_branch": 0.0155,
    "c.W0": 0.0044,
    "c.b0": 0.00427,
    "c.W1": 0.00372,
    "c.b1": 0.00311,
    "c.W2": 0.00398,
    "c.b2": 0.00253,
    "c.W_mu": 0.00331,
    "c.b_mu": 0.000628,
}
MEASURED_UNCHANGED = {'approx_kl': 0.000352, 'clip_fraction': 0.000116, 'max_mu': 0.0598}
MEASURED_ABS_OVER_TERMS = {'a.b_mu': 0.000685, 'a.log_sigma': 0.00155}      # |g_bf16 - g_f32| / sum_i |term_i|, the largest of three seeds
COS_FLOOR = 0.99


def _env(seed=0, record=True):
    """test_ppo_gpu._env for seed 0; other seeds move the actors' weights and the start jitter"""
    import hierarchicalkarting_amd as hk
    _torch()
    g = hk.RacingEnv(hk.make_config(24, 4, **dict(KW, jitter_seed=KW["jitter_seed"] + seed)))
    g.reset()
    D = g.obs_dim
    pols = [(Policy.random(D * 4, 256, 3, seed=1 + 100 * seed), [0, 1]), (Policy.random(D * 4, 128, 2, seed=2 + 100 * seed, deterministic=True), [2, 3])]
    for k, (pol, slots) in enumerate(pols):
        assert g.attach_policy(pol, slots, P) == k
    if record:
        g.rollout_begin(R)
        g.step(R * P)
        g.rollout_close()
    return g, pols


_shared = {}


def _plain_env():
    """one handle for the tests that only need the debug tap"""
    if "g" not in _shared:
        _shared["g"] = _env(record=False)[0]
    return _shared["g"]


# ---- 1. each product form against an exact reference
MS, NS, KS, ROWS = (1, 63, 64, 65, 130), (1, 128, 130), (8, 16, 312, 320), (1, 255, 256, 257, 600)


@pytest.mark.parametrize("epi", [1, 2, 0])
def test_product_form_against_the_float64_reference(epi):
    g = _plain_env()
    rng = np.random.default_rng(100 + epi)
    worst = 0.0
    for M in MS:
        for N in NS:
            for K in (ROWS if epi == 0 else KS):
                A = BR.random_bf16(rng, (K, M) if epi == 0 else (M, K))
                B = BR.random_bf16(rng, (N, K) if epi == 1 else (K, N))
                bias = rng.standard_normal(N).astype(np.float32) if epi == 1 else None
                aux = (2.0 * rng.standard_normal((M, N))).astype(np.float32) if epi == 2 else None
                got = ppo.gemm_bf16(g, epi, A, B, bias, aux).astype(np.float64)
                ref, tol = BR.product(epi, A, B, bias, aux)
                err = np.abs(got - ref)
                ratio = float((err / np.maximum(tol, 1e-300)).max())
                worst = max(worst, ratio)
                assert (err <= tol).all(), (epi, M, N, K, ratio, float(err.max()))
    print("epi %d: worst |C - ref| / bound %.3g" % (epi, worst))


def test_rounding_twin_through_the_entry_point():
    """K = 1 against the all-ones row: the weight-gradient form returns the device's view of each bf16 value, which is the twin's"""
    g = _plain_env()
    rng = np.random.default_rng(7)
    A = BR.random_bf16(rng, (1, 130))
    one = ppo.bf16_round(np.ones((1, 3), np.float32))
    got = ppo.gemm_bf16(g, 0, A, one)
    assert_bits_equal(got, np.repeat(ppo.bf16_value(A).reshape(130, 1), 3, axis=1), "K = 1 products")


# ---- 2. rounding points
def test_shadow_is_the_host_rounding_of_the_masters():
    torch = _torch()
    g, pols = _env(record=False)
    tr = g.ppo_trainer(0)
    assert tr.precision == "f32" and "shadow" not in tr.views()
    special = np.array([1e-40, -1e-40, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)
    v = tr.views()["params"]
    v[5:5 + special.size] = torch.from_numpy(special).to(v.device)
    v[tr.n_actor + 3:tr.n_actor + 3 + special.size] = torch.from_numpy(special).to(v.device)
    torch.cuda.synchronize()
    tr.set_precision("bf16")
    assert tr.precision == "bf16"
    for step in range(2):
        prm = tr.read("params")
        got, want = tr.shadow(), ppo.bf16_round(prm)
        assert got.size == prm.size and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        tr.views()["grad"].normal_()                 # a gradient, so that Adam moves the masters
        torch.cuda.synchronize()
        tr.adam(1e-2)
    assert np.isnan(ppo.bf16_value(tr.shadow()[[11, tr.n_actor + 9]])).all()
    tr2 = g.ppo_trainer(0, precision="bf16")
    assert tr2.precision == "bf16" and np.array_equal(tr2.shadow(), ppo.bf16_round(tr2.read("params")))


# ---- 3. gradients of a whole minibatch against fp32 mode
def _blocks(tr, flat):
    out = {"a." + k: v for k, v in tr.actor_params(flat).items()}
    out.update({"c." + k: v for k, v in tr.critic_params(flat).items()})
    return out


def _one_element_terms(tr, f, n, beta):
    """per-row terms of the actor's b_mu and log_sigma gradients at unchanged parameters in fp32 mode, where rho == 1 exactly and lies inside
    the clip, so the surrogate's slope is ADV (hk.h LOSS): d/dmu = -(ADV / 2n) z / sigma, d/dlog_sigma = -(ADV / 2n) (z^2 - 1) - beta / n,
    z = (RAW - MU) / sigma.  -> dict block -> float64 [n]"""
    adv = tr.read("adv").astype(np.float64)
    sigma = float(np.exp(np.float64(tr.actor_params()["log_sigma"][0])))
    z = (f["raw"].astype(np.float64) - f["mu"].astype(np.float64)) / sigma
    return {"a.b_mu": -0.5 * adv / n * z / sigma, "a.log_sigma": -0.5 * adv / n * (z * z - 1.0) - beta / n}


@functools.lru_cache(maxsize=None)
def _measure(seed):
    """-> (per-block (rel L2, cosine) of GRAD between the precisions on all rows + out-of-range ids, unchanged-parameter figures in bf16 mode)"""
    torch = _torch()
    g, pols = _env(seed)
    X, f, _, _ = _rows(g, pols, 0)
    n = X.shape[0]
    ids = np.concatenate([np.arange(n // 2), [n + 7, -1], np.arange(n // 2, n), [n]]).astype(np.int32)
    grads, stats = {}, {}
    tr = g.ppo_trainer(0)
    for prec in ("f32", "bf16", "f32"):
        tr.set_precision(prec)
        tr.advantages()
        st = tr.minibatch(_ids(torch, ids), 0.2, 5e-3)
        assert st["skipped"] == 3.0, st
        grads[prec] = _blocks(tr, tr.read("grad"))
        if prec == "f32" and "terms" not in stats:
            stats["terms"] = _one_element_terms(tr, f, n, 5e-3)
        st = tr.minibatch(_ids(torch, np.arange(n)), 0.2, 5e-3)
        stats[prec] = dict(st, max_mu=float(np.abs(tr.read("mb_mu") - f["mu"]).max()))
        if prec == "f32":
            # the exact path, before and after the trainer was in bf16 mode
            assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0 and stats[prec]["max_mu"] == 0.0, st
    diff = BR.block_differences(grads["bf16"], grads["f32"])
    for k, term in stats["terms"].items():
        g32, g16, scale = float(grads["f32"][k][0]), float(grads["bf16"][k][0]), float(np.abs(term).sum())
        # the terms are the device's: their sum is its fp32-mode gradient up to the fp32 rounding of each term (u = 2^-24 each, and the fp64 sum)
        assert abs(term.sum() - g32) <= 1e-5 * scale, (k, term.sum(), g32, scale)
        diff[k] = diff[k] + (abs(g16 - g32) / scale,)
    return diff, stats["bf16"]


def test_minibatch_gradients_against_fp32_mode():
    diff, _ = _measure(0)
    for k, d in diff.items():
        print("%-12s rel L2 %.3e  cosine %.6f" % (k, d[0], d[1]) + ("  |diff| / sum |terms| %.3e" % d[2] if len(d) > 2 else ""))
    for k, d in diff.items():
        assert d[1] >= COS_FLOOR, (k, d[1])
    assert set(MEASURED_REL_L2) == set(diff), "MEASURED_REL_L2 has not been measured for %s" % sorted(set(diff) - set(MEASURED_REL_L2))
    for k, d in diff.items():
        assert d[0] <= 4.0 * MEASURED_REL_L2[k], (k, d[0], MEASURED_REL_L2[k])
    assert set(MEASURED_ABS_OVER_TERMS) == {"a.b_mu", "a.log_sigma"}, "MEASURED_ABS_OVER_TERMS has not been measured"
    for k, bound in MEASURED_ABS_OVER_TERMS.items():
        assert diff[k][2] <= 4.0 * bound, (k, diff[k][2], bound)


# ---- 4. unchanged parameters
def test_unchanged_parameters_in_bf16_mode_and_back():
    """(that fp32 mode is exact again after the switch back is asserted inside _measure)"""
    _, st = _measure(0)
    print("unchanged parameters, bf16: approx_kl %.3e  clip_fraction %.3e  max |mb_mu - MU| %.3e" % (st["approx_kl"], st["clip_fraction"], st["max_mu"]))
    assert st["skipped"] == 0.0
    assert st["max_mu"] > 0.0            # the bf16 trunk is not the inference chain
    assert set(MEASURED_UNCHANGED) == {"approx_kl", "clip_fraction", "max_mu"}, "MEASURED_UNCHANGED has not been measured"
    for k in ("approx_kl", "clip_fraction", "max_mu"):
        assert abs(st[k]) <= 4.0 * MEASURED_UNCHANGED[k], (k, st[k])


# ---- 5. determinism
def test_bf16_update_is_deterministic():
    g, pols = _env()
    t1, t2 = g.ppo_trainer(0, seed=7, precision="bf16"), g.ppo_trainer(0, seed=7, precision="bf16")
    for t in (t1, t2):
        t.advantages()
    s1, s2 = t1.update(2, 512, 3e-4, 0.2, 5e-3), t2.update(2, 512, 3e-4, 0.2, 5e-3)
    for name in ("params", "adam_m", "adam_v", "perm"):
        assert_bits_equal(t1.read(name), t2.read(name), name + " of two identical bf16 updates")
    assert s1 == s2 and np.isfinite(list(s1.values())).all()
    assert np.array_equal(t1.shadow(), ppo.bf16_round(t1.read("params")))


def test_update_reads_parameters_written_after_advantages():
    """PARAMS written through views() between advantages() and update() (a checkpoint restore): hk_ppo_update rounds them into the shadow at its
    entry, so one bf16 update gives the bits of a trainer whose parameters were written before advantages() (V_OLD / ADV / RET made equal)"""
    torch = _torch()
    g, pols = _env()
    t1, t2 = g.ppo_trainer(0, seed=5, precision="bf16"), g.ppo_trainer(0, seed=5, precision="bf16")
    new = (t1.read("params") * np.float32(1.03)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    t1.views()["params"].copy_(dev(new))
    torch.cuda.synchronize()
    t1.advantages()                                   # the shadow follows the new parameters here
    t2.advantages()                                   # ... and here it is still the old parameters'
    g.synchronize()                                   # (hk_stream is not torch's stream: its writes of V_OLD / ADV / RET come first)
    v1, v2 = t1.views(), t2.views()
    v2["params"].copy_(dev(new))
    for k in ("v_old", "adv", "ret"):
        v2[k].copy_(v1[k])
    torch.cuda.synchronize()
    n = t1.read("adv").size
    s1, s2 = t1.update(1, n, 3e-4, 0.2, 5e-3), t2.update(1, n, 3e-4, 0.2, 5e-3)
    for name in ("grad", "params", "adam_m", "adam_v"):
        assert_bits_equal(t1.read(name), t2.read(name), name + " after parameters written before / after advantages()")
    assert s1 == s2


# ---- 6. it optimises, and publish closes the loop
def test_bf16_update_optimises_and_publishes():
    import hierarchicalkarting_amd as hk
    g, pols = _env()
    tv = g.ppo_trainer(0, seed=3, precision="bf16")
    tv.advantages()
    hist = [tv.update(1, 256, 3e-3, 1e3, 5e-3) for _ in range(10)]
    assert hist[-1]["L_v"] < 0.5 * hist[0]["L_v"], [h["L_v"] for h in hist]
    tp = g.ppo_trainer(1, seed=4, precision="bf16")
    tp.advantages()
    hist = [tp.update(1, 256, 3e-4, 0.2, 5e-3) for _ in range(10)]
    assert hist[-1]["L_pi"] < hist[0]["L_pi"], [h["L_pi"] for h in hist]
    assert hist[-1]["approx_kl"] != 0.0
    # the next step() acts with the published fp32 masters: the recorded heads are actor()'s on the recorded stacked inputs
    a0, a1 = tv.actor(), tp.actor()
    assert not np.array_equal(a0.W[0], pols[0][0].W[0]) and not np.array_equal(a1.W[0], pols[1][0].W[0])
    h = hk.RacingEnv(hk.make_config(24, 4, **KW))
    h.reset()
    h.attach_policy(a0, [0, 1], P)
    h.attach_policy(a1, [2, 3], P)
    g.rollout_begin(8); g.step(8 * P); g.rollout_close()
    for p in (0, 1):
        X, f, _, _ = _rows(g, pols, p)
        mu, lg = h.policy_forward(p, X.astype(np.float32))
        assert_bits_equal(mu, f["mu"], "next rollout MU %d" % p)
        assert_bits_equal(lg, f["logits"], "next rollout LOGITS %d" % p)


# ---- 7. refusals
def test_refusals():
    torch = _torch()
    g = _plain_env()
    L, h = g.L, g.h
    tr = g.ppo_trainer(0)
    INV = _lib.HK_ERR_INVALID
    assert L.hk_ppo_set_precision(h, tr.t, 2) == INV and L.hk_ppo_set_precision(h, tr.t, -1) == INV
    assert L.hk_ppo_set_precision(h, 9, _lib.HK_PPO_PREC_BF16) == INV and L.hk_ppo_set_precision(h, -1, 0) == INV
    assert L.hk_ppo_get_precision(h, 9) == INV and L.hk_ppo_get_precision(h, tr.t) == _lib.HK_PPO_PREC_F32
    with pytest.raises(ValueError):
        tr.set_precision("fp16")
    with pytest.raises(ValueError):
        g.ppo_trainer(0, precision="half")
    assert L.hk_ppo_ptr(h, tr.t, _lib.PPO_FIELDS["shadow"]) is None and L.hk_ppo_count(h, tr.t, _lib.PPO_FIELDS["shadow"]) == 0
    a = torch.zeros(64, dtype=torch.int16, device="cuda:0")
    c = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pa, pc = C.c_void_p(a.data_ptr()), C.c_void_p(c.data_ptr())
    assert L.hk_ppo_gemm_bf16(h, 1, 8, 8, 8, pa, pa, None, None, pc) == 0
    for epi, M, N, K, A, B, aux, out in ((3, 8, 8, 8, pa, pa, pc, pc), (-1, 8, 8, 8, pa, pa, pc, pc), (1, 0, 8, 8, pa, pa, None, pc),
                                         (1, 8, -1, 8, pa, pa, None, pc), (0, 8, 8, 0, pa, pa, None, pc), (1, 8, 8, 8, None, pa, None, pc),
                                         (1, 8, 8, 8, pa, None, None, pc), (1, 8, 8, 8, pa, pa, None, None), (2, 8, 8, 8, pa, pa, None, pc)):
        assert L.hk_ppo_gemm_bf16(h, epi, M, N, K, A, B, None, aux, out) == INV, (epi, M, N, K)
    g.synchronize()
