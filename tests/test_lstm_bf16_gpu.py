"""Recurrent actors in bf16 on the device (include/hk.h "RECURRENT ACTORS IN BF16"): hk_policy_lstm_set_precision,
hk_ppo_recurrent_set_precision and the tap hk_ppo_lstm_gates_bf16.

Fields.  Two 2v2 Oval fields (4 karts, every kart RL, DecisionPeriod 2; the trained recurrent actor drives karts 0 and 1, a second recurrent
actor of the same shape karts 2 and 3): 5 envs and 70 envs (10 and 140 sequences per window: below and above the 64-row tile of the step
kernels), the envs with env % 4 == k restarted at tick k and max_episode_steps = 100 as in tests/test_ppo_lstm_gpu.py, so that FIRST falls
strictly inside a window.  R = 10 rows in windows of L = 4: the last window is short (2 live
rows, 2 dead ones).

Bounds.  The gate product is held to 2 gamma_K sum |a| |b| + the seed's ulp (lstm_bf16_restate.gates_ref, §13's bound).  Everything said to be
"bit for bit" is compared as bits.  The gradients and one inference step of the bf16 mode against the fp32 mode follow §13's scheme: cosine at
least 0.99 and the relative L2 at most 4 x the largest of three seeds measured on the MI355X (MEASURED_* below; the one-element blocks b_mu and
log_sigma also in §13's absolute form, |difference| over the sum of the |terms| they add up)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lstm_bf16_restate as LB
import policy_lstm_twin as TW
import ppo_bf16_restate as BR
from hierarchicalkarting_amd import _lib, ppo
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.ppo import bf16_round, bf16_value
from hierarchicalkarting_amd.selfplay import SnapshotPool
from parity import assert_bits_equal

pytestmark = pytest.mark.gpu
P, R, L, S = 2, 10, 4, 2
SHAPES = [(32, 32), (96, 96), (128, 128), (256, 64)]          # (H, m)
EPS, BETA = 0.2, 5e-3
COS_FLOOR = 0.99
SEEDS = (4, 5, 6)
# GRAD of the bf16 mode against the fp32 mode on the same state, E = 5, 312 -> 128 x 2 -> m = 128, every sequence in one minibatch: the largest
# relative L2 per block over SEEDS as measured on the MI355X (test_gradients_against_fp32_mode prints the table; DESIGN §20 has it).
MEASURED_REL_L2 = {
    "trunk": 8.19e-3, "W_ih": 7.92e-3, "W_hh": 7.24e-3, "b_ih": 7.01e-3, "b_hh": 7.01e-3, "heads": 4.56e-3, "critic": 8.06e-3,
    "b_mu": 1.05e-2, "log_sigma": 2.83e-1,
}
# b_mu and log_sigma are one-element sums over all rows whose terms nearly cancel (log_sigma's was small on the first seed, hence 0.283 above),
# so they are also held to §13's absolute form: |g_bf16 - g_f32| / sum_i |term_i|, the largest of SEEDS
MEASURED_ABS_OVER_TERMS = {"b_mu": 9.60e-4, "log_sigma": 3.85e-3}
# one decision of the bf16 policy against the fp32 policy, same weights, 130 rows and memory: relative L2 over all rows, the largest of SEEDS
MEASURED_STEP_REL_L2 = {"mu": 5.76e-3, "logits": 5.33e-3, "h": 5.01e-3, "c": 4.35e-3}


def _torch():
    import torch
    torch.cuda.init()
    return torch


def _ids(a):
    return _torch().as_tensor(np.asarray(a, np.int32), device="cuda:0")


def _field(E, H, m, seed=4, layers=2):
    _torch()
    g = TW.rl_env(E, 4, rewards=1, max_episode_steps=100, jitter_seed=9)
    assert g.obs_dim * 4 == 312
    pol = Policy.random(g.obs_dim * 4, H, layers, 3, seed=seed, memory_size=2 * m)
    assert g.attach_policy(pol, [0, 1], P) == 0
    assert g.attach_policy(Policy.random(g.obs_dim * 4, H, layers, 3, seed=seed + 100, memory_size=2 * m), [2, 3], P) == 1
    for k in (1, 2, 3):                            # the envs with env % 4 == k restart their episode after k ticks
        g.step(1)
        ids = np.array([e for e in range(E) if e % 4 == k], np.int32)
        if ids.size:
            g.reset(ids)
    g.step(89)                                     # tick 92
    return g, pol


def _rollout(g, again=False):
    """records R rows from tick 92 on (again: from tick 190 on, after a first rollout that ended at tick 112: the next round of time-outs)"""
    if again:
        g.step(78)
    g.rollout_begin(R)
    g.step(R * P)
    g.rollout_close()
    ro = g.rollout()
    first = ro["first"][:, :, 0]
    assert g.rollout_rows() == R
    assert any(first[t].any() for t in (1, 2, 3, 5, 6, 7, 9)), "no FIRST strictly inside a window"
    return ro


def _fields_of(ro, pol):
    E, mm = ro["obs"].shape[1], pol.memory_size
    f = {k: ro[k][:, :, [0, 1]].reshape(-1) for k in ("raw", "mu")}
    f["logits"] = ro["logits"][:, :, [0, 1], :pol.n_branch].reshape(-1, pol.n_branch)
    return dict(f=f, memory=ro["memory"][:, :, [0, 1], :mm].reshape(R, E * S, mm), first=ro["first"][:, :, [0, 1]].reshape(R, E * S),
                next_memory=ro["next_memory"][:, [0, 1], :mm].reshape(E * S, mm), done=np.repeat(ro["done"][:, :, None] != 0, S, axis=2).reshape(R, E * S))


def _rowids(sids, E):
    out = np.full((L, len(sids)), -1, np.int64)
    for q, s in enumerate(sids):
        for tau, rid in enumerate(ppo.sequence_rows(int(s), R, L, E, S)):
            out[tau, q] = rid
    return out


def _mb_against_recorder(tr, g, pol, hst, sids):
    """one minibatch -> (stats, max |MB_MU - MU| over the live rows, did MB_MU / MB_LOGITS / MB_MEMORY equal the recorder's rows bit for bit)"""
    E, mm, nb = g.E, pol.memory_size, pol.n_branch
    st = tr.minibatch(_ids(sids), EPS, BETA)
    rid = _rowids(sids, E)
    live = rid >= 0
    ms = len(sids)
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    mu = tr.read("mb_mu").reshape(L, ms)[live]
    same = np.array_equal(bits(mu), bits(hst["f"]["mu"][rid[live]]))
    same &= np.array_equal(bits(tr.read("mb_logits").reshape(L, ms, nb)[live]), bits(hst["f"]["logits"][rid[live]]))
    mem = tr.read("mb_memory").reshape(L, ms, mm)
    t, p = rid // (E * S), rid % (E * S)
    chained = 0
    for tau in range(L):
        for q in range(ms):
            if rid[tau, q] < 0:
                continue
            tt, pp = t[tau, q], p[tau, q]
            if tt + 1 < R and not hst["first"][tt + 1, pp]:
                same &= np.array_equal(bits(mem[tau, q]), bits(hst["memory"][tt + 1, pp])); chained += 1
            elif tt == R - 1 and not hst["done"][tt, pp]:
                same &= np.array_equal(bits(mem[tau, q]), bits(hst["next_memory"][pp])); chained += 1
    assert chained > 0
    return st, float(np.abs(mu - hst["f"]["mu"][rid[live]]).max()), bool(same)


@pytest.fixture(scope="module")
def tap_env():
    _torch()
    return TW.rl_env(1, 2)


# ---- 1. the gate product against float64
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_gate_product_against_float64(tap_env, rows, shape):
    H, m = shape
    rng = np.random.default_rng(1000 * rows + H + m)
    a, h = BR.random_bf16(rng, (rows, H)), BR.random_bf16(rng, (rows, m))
    W_ih, W_hh = BR.random_bf16(rng, (4 * m, H)), BR.random_bf16(rng, (4 * m, m))
    bs = rng.standard_normal(4 * m).astype(np.float32)
    z = ppo.lstm_gates_bf16(tap_env, a, h, W_ih, W_hh, bs)
    ref, tol = LB.gates_ref(a, h, W_ih, W_hh, bs)
    err = np.abs(z.astype(np.float64) - ref)
    print("rows %d H %d m %d: max err / tol %.3f" % (rows, H, m, (err / tol).max()))
    assert z.shape == (rows, 4 * m) and (err <= tol).all()
    # the same call gives the same bits
    assert_bits_equal(ppo.lstm_gates_bf16(tap_env, a, h, W_ih, W_hh, bs), z, "tap twice")


@pytest.mark.parametrize("shape", SHAPES)
def test_gate_product_minus_zero_seed(tap_env, shape):
    """an accumulator seeded -0.0 and stepped with all-zero operands ends +0.0: the padding steps are issued"""
    H, m = shape
    zero = lambda *s: np.zeros(s, np.uint16)
    z = ppo.lstm_gates_bf16(tap_env, zero(65, H), zero(65, m), zero(4 * m, H), zero(4 * m, m), np.full(4 * m, -0.0, np.float32))
    assert not z.view(np.uint32).any()


def test_tap_refusals(tap_env):
    g = tap_env
    torch = _torch()
    buf = torch.zeros(4 * 32 * 32, dtype=torch.float32, device="cuda:0")
    p = C.c_void_p(buf.data_ptr())
    ok = lambda rows=1, H=32, m=32, ptrs=(p,) * 6: g.L.hk_ppo_lstm_gates_bf16(g.h, rows, H, m, *ptrs)
    assert ok() == _lib.HK_OK
    for kw in (dict(rows=0), dict(H=0), dict(m=0), dict(H=48), dict(m=16), dict(m=40)):
        assert ok(**kw) == _lib.HK_ERR_INVALID, kw
    for i in range(6):
        assert ok(ptrs=tuple(None if j == i else p for j in range(6))) == _lib.HK_ERR_INVALID and "NULL" in g.L.hk_last_error(g.h).decode()
    # hk_ppo_gemm_bf16 keeps refusing other epi values
    assert g.L.hk_ppo_gemm_bf16(g.h, 3, 1, 1, 1, p, p, p, p, p) == _lib.HK_ERR_INVALID and "epi" in g.L.hk_last_error(g.h).decode()
    g.synchronize()


# ---- 2. inference against the composed chain, bit for bit
#        (karts, stack) -> in_dim 54 / 312 / 624; layers 1 - 3; the (H, m) of case 1; every pairing of in_dim and shape, every layer count
FORWARD = [(2, 1, 1, 32, 32), (2, 1, 3, 256, 64), (2, 1, 2, 96, 96), (2, 1, 2, 128, 128), (4, 4, 3, 128, 128), (4, 4, 1, 32, 32), (4, 4, 2, 256, 64),
           (4, 4, 2, 96, 96), (4, 8, 2, 96, 96), (4, 8, 1, 128, 128), (4, 8, 3, 32, 32), (4, 8, 2, 256, 64)]


@pytest.mark.parametrize("karts,stack,layers,H,m", FORWARD)
def test_inference_is_the_composed_chain(karts, stack, layers, H, m):
    _torch()
    g = TW.rl_env(2, karts)
    in_dim = g.obs_dim * stack
    assert in_dim == {(2, 1): 54, (4, 4): 312, (4, 8): 624}[(karts, stack)]
    pol = Policy.random(in_dim, H, layers, 3, stack=stack, seed=H + m + layers, memory_size=2 * m)
    assert g.attach_policy(pol, [0], P) == 0
    g.policy_lstm_set_precision(0, "bf16")
    assert g.policy_precision(0) == "bf16"
    rng = np.random.default_rng(in_dim + H)
    for rows in (1, 64, 65, 130):
        obs = (rng.standard_normal((rows, in_dim)) * 2).astype(np.float32)
        for mem in (None, rng.standard_normal((rows, 2 * m)).astype(np.float32)):
            mu, lg, out = g.policy_forward(0, obs, mem)
            rmu, rlg, rout = LB.compose(g, pol, obs, mem)
            tag = (in_dim, layers, H, m, rows, mem is not None)
            assert_bits_equal(mu, rmu, (tag, "mu"))
            assert_bits_equal(lg, rlg, (tag, "logits"))
            assert_bits_equal(out[:, :m], rout[:, :m], (tag, "h'"))
            assert_bits_equal(out[:, m:], rout[:, m:], (tag, "c'"))
    # ... and it is not the fp32 chain
    g.policy_lstm_set_precision(0, "f32")
    mu32, _, _ = g.policy_forward(0, obs, mem)
    assert not np.array_equal(mu32, mu)
    t_mu, t_lg, t_out = TW.step(pol, obs, mem)
    assert_bits_equal(mu32, t_mu, "fp32 again: the host twin")


# ---- 3. rho == 1 with policy and trainer both in bf16; the mixed settings differ
@pytest.mark.parametrize("E,shape", [(5, (32, 32)), (5, (128, 128)), (70, (96, 96)), (70, (128, 128))])
def test_unchanged_parameters_reproduce_the_recorder_in_bf16(E, shape):
    g, pol = _field(E, *shape)
    g.policy_lstm_set_precision(0, "bf16")
    hst = _fields_of(_rollout(g), pol)
    tr = g.ppo_trainer(0, sequence_length=L)
    tr.set_recurrent_precision("bf16")
    assert tr.precision == "bf16"
    tr.advantages()
    nseq = ppo.sequence_count(R, L, E, S)
    assert nseq == 3 * E * S
    rng = np.random.default_rng(E)
    for sids in (np.arange(nseq), np.concatenate([rng.permutation(nseq), [nseq + 3, -1]])):
        st, dmu, same = _mb_against_recorder(tr, g, pol, hst, sids)
        assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0, st
        assert dmu == 0.0 and same
    # control: the fp32 trainer on the rows of the bf16 policy is NOT that chain
    tr.set_recurrent_precision("f32")
    tr.advantages()
    st, dmu, same = _mb_against_recorder(tr, g, pol, hst, np.arange(nseq))
    assert dmu > 0.0 and not same
    # control: the bf16 trainer on rows of the fp32 policy
    g.policy_lstm_set_precision(0, "f32")
    hst32 = _fields_of(_rollout(g, again=True), pol)
    tr.advantages()
    st, dmu, same = _mb_against_recorder(tr, g, pol, hst32, np.arange(nseq))
    assert dmu == 0.0 and same and st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0          # fp32 on fp32: exact, as ever
    tr.set_recurrent_precision("bf16")
    tr.advantages()
    st, dmu, same = _mb_against_recorder(tr, g, pol, hst32, np.arange(nseq))
    assert dmu > 0.0 and not same


# ---- 4. back to fp32: the bits of a handle that never switched, also after a publish
def test_back_to_fp32_is_the_untouched_handle():
    E, shape = 5, (96, 96)
    ga, pa = _field(E, *shape)
    gb, _ = _field(E, *shape)
    ta = ga.ppo_trainer(0, sequence_length=L, seed=3)
    tb = gb.ppo_trainer(0, sequence_length=L, seed=3)
    # handle b goes to bf16 and back, with a forward and a publish (which rebuilds the bf16 copies) in between; handle a never switches
    gb.policy_lstm_set_precision(0, "bf16")
    tb.set_recurrent_precision("bf16")
    gb.policy_forward(0, np.ones((3, pa.in_dim), np.float32))
    tb.publish()
    gb.policy_lstm_set_precision(0, "f32")
    tb.set_recurrent_precision("f32")
    assert gb.policy_precision(0) == "f32" and tb.precision == "f32"
    rng = np.random.default_rng(2)
    obs = rng.standard_normal((65, pa.in_dim)).astype(np.float32)
    mem = rng.standard_normal((65, pa.memory_size)).astype(np.float32)
    for x, y in zip(ga.policy_forward(0, obs, mem), gb.policy_forward(0, obs, mem)):
        assert_bits_equal(x, y, "forward after the switch back")
    roa, rob = _rollout(ga), _rollout(gb)
    for k in ("mu", "logits", "memory", "next_memory", "raw"):
        assert_bits_equal(roa[k], rob[k], ("rollout after the switch back", k))
    nseq = ppo.sequence_count(R, L, E, S)
    for t in (ta, tb):
        t.advantages()
        t.minibatch(_ids(np.arange(nseq)), EPS, BETA)
    assert_bits_equal(ta.read("grad"), tb.read("grad"), "GRAD after the switch back")
    assert_bits_equal(ta.read("mb_memory"), tb.read("mb_memory"), "MB_MEMORY after the switch back")
    for t in (ta, tb):
        t.update(1, 8, 3e-4, EPS, BETA)
    assert_bits_equal(ta.read("params"), tb.read("params"), "PARAMS after an update and publish")
    for x, y in zip(ga.policy_forward(0, obs, mem), gb.policy_forward(0, obs, mem)):
        assert_bits_equal(x, y, "forward after the publish")


# ---- 5. publish and pools rebuild the bf16 copies
def test_publish_and_pool_rebuild_the_bf16_copies():
    E, (H, m) = 5, (96, 96)
    g, pol = _field(E, H, m)
    g.policy_lstm_set_precision(0, "bf16")
    tr = g.ppo_trainer(0, sequence_length=L)
    tr.set_recurrent_precision("bf16")
    _rollout(g)
    tr.advantages()
    tr.update(1, 8, 3e-3, EPS, BETA)                         # ... ends with a publish
    assert not np.array_equal(tr.actor_params()["W_hh"], pol.lstm["W_hh"])
    # every bf16 inference weight is the HK_PPO_SHADOW element: the forward equals the chain composed from the shadow's bit patterns
    sh = ppo.split_params(tr.shadow()[:tr.n_actor], tr.actor_layout)
    new = tr.actor()
    for k in ["W%d" % l for l in range(2)] + ["W_ih", "W_hh"]:
        assert np.array_equal(sh[k], bf16_round(tr.actor_params()[k])), k
    rng = np.random.default_rng(3)
    obs = rng.standard_normal((65, pol.in_dim)).astype(np.float32)
    mem = rng.standard_normal((65, 2 * m)).astype(np.float32)
    got = g.policy_forward(0, obs, mem)
    want = LB.compose(g, new, obs, mem)                      # (rounds the published masters once: the shadow's elements, checked above)
    for x, y, k in zip(got, want, ("mu", "logits", "memory")):
        assert_bits_equal(x, y, ("published weights play", k))
    stale = LB.compose(g, pol, obs, mem)
    assert not np.array_equal(stale[0], got[0])
    # a recurrent pool: save / load into a bf16 policy plays the loaded weights — bit-equal to a fresh attach of those weights switched to bf16
    g2 = TW.rl_env(2, 4)
    a, b = Policy.random(pol.in_dim, H, 2, 3, seed=11, memory_size=2 * m), Policy.random(pol.in_dim, H, 2, 3, seed=12, memory_size=2 * m)
    assert g2.attach_policy(a, [0], P) == 0 and g2.attach_policy(b, [1], P) == 1
    g2.policy_lstm_set_precision(1, "bf16")
    before = g2.policy_forward(1, obs, mem)
    pool = SnapshotPool(g2, 0, 2)
    pool.save(0)                                             # policy 0's weights (fp32 policy) -> slot 0
    pool.load(0, 1)                                          # -> the bf16 policy 1
    after = g2.policy_forward(1, obs, mem)
    g3 = TW.rl_env(2, 4)
    assert g3.attach_policy(a, [0], P) == 0
    g3.policy_lstm_set_precision(0, "bf16")
    fresh = g3.policy_forward(0, obs, mem)
    for x, y, z, k in zip(after, fresh, before, ("mu", "logits", "memory")):
        assert_bits_equal(x, y, ("pool load into a bf16 policy", k))
        assert not np.array_equal(x, z)
    pool.put(1, b)
    pool.load(1, 1)
    for x, z, k in zip(g2.policy_forward(1, obs, mem), before, ("mu", "logits", "memory")):
        assert_bits_equal(x, z, ("put + load", k))


# ---- 6. gradients and one decision against the fp32 mode
def _blocks(tr, flat):
    a, c = tr.actor_params(flat), tr.critic_params(flat)
    cat = lambda d, keys: np.concatenate([d[k].reshape(-1) for k in keys])
    trunk = [k for k in a if k[0] in "Wb" and k[1:].isdigit()]
    return {"trunk": cat(a, trunk), "W_ih": a["W_ih"], "W_hh": a["W_hh"], "b_ih": a["b_ih"], "b_hh": a["b_hh"],
            "heads": cat(a, ["W_mu", "W_branch", "b_branch"]), "critic": cat(c, list(c)), "b_mu": a["b_mu"], "log_sigma": a["log_sigma"]}


@functools.lru_cache(maxsize=None)
def _measure(seed):
    E, (H, m) = 5, (128, 128)
    g, pol = _field(E, H, m, seed=seed)
    ro = _rollout(g)
    f = _fields_of(ro, pol)["f"]
    nseq = ppo.sequence_count(R, L, E, S)
    tr = g.ppo_trainer(0, sequence_length=L)
    grads = {}
    for prec in ("f32", "bf16"):
        tr.set_recurrent_precision(prec)
        tr.advantages()
        tr.minibatch(_ids(np.arange(nseq)), EPS, BETA)
        grads[prec] = _blocks(tr, tr.read("grad"))
        if prec == "f32":
            n = R * E * S
            adv = tr.read("adv").astype(np.float64)
            sigma = float(np.exp(np.float64(tr.actor_params()["log_sigma"][0])))
            z = (f["raw"].astype(np.float64) - f["mu"].astype(np.float64)) / sigma
            terms = {"b_mu": -0.5 * adv / n * z / sigma, "log_sigma": -0.5 * adv / n * (z * z - 1.0) - BETA / n}
    diff = BR.block_differences(grads["bf16"], grads["f32"])
    for k, term in terms.items():
        g32, g16, scale = float(grads["f32"][k][0]), float(grads["bf16"][k][0]), float(np.abs(term).sum())
        assert abs(term.sum() - g32) <= 1e-5 * scale, (k, term.sum(), g32, scale)          # the terms are the device's
        diff[k] = diff[k] + (abs(g16 - g32) / scale,)
    # one decision in both precisions on the same rows and memory
    rng = np.random.default_rng(seed)
    obs = (rng.standard_normal((130, pol.in_dim)) * 2).astype(np.float32)
    mem = rng.standard_normal((130, 2 * m)).astype(np.float32) * 0.5
    g.policy_lstm_set_precision(0, "f32")
    x32 = g.policy_forward(0, obs, mem)
    g.policy_lstm_set_precision(0, "bf16")
    x16 = g.policy_forward(0, obs, mem)
    split = lambda x: {"mu": x[0], "logits": x[1], "h": x[2][:, :m], "c": x[2][:, m:]}
    return diff, BR.block_differences(split(x16), split(x32))


def test_gradients_against_fp32_mode():
    table = [_measure(s)[0] for s in SEEDS]
    for k in table[0]:
        print("%-10s rel L2 %s  cosine %s%s" % (k, " ".join("%.3e" % t[k][0] for t in table), " ".join("%.6f" % t[k][1] for t in table),
                                               "  |diff| / sum |terms| " + " ".join("%.3e" % t[k][2] for t in table) if len(table[0][k]) > 2 else ""))
    assert set(MEASURED_REL_L2) == set(table[0])
    for t in table:
        for k, d in t.items():
            if k not in MEASURED_ABS_OVER_TERMS:          # (a one-element block's cosine is only its sign: §13)
                assert d[1] >= COS_FLOOR, (k, d)
            assert d[0] <= 4.0 * MEASURED_REL_L2[k], (k, d[0], MEASURED_REL_L2[k])
        for k, bound in MEASURED_ABS_OVER_TERMS.items():
            assert t[k][2] <= 4.0 * bound, (k, t[k][2], bound)


def test_one_decision_against_fp32_mode():
    table = [_measure(s)[1] for s in SEEDS]
    for k in table[0]:
        print("%-8s rel L2 %s  cosine %s" % (k, " ".join("%.3e" % t[k][0] for t in table), " ".join("%.6f" % t[k][1] for t in table)))
    for t in table:
        for k, d in t.items():
            assert d[1] >= COS_FLOOR and 0.0 < d[0] <= 4.0 * MEASURED_STEP_REL_L2[k], (k, d)


# ---- 7. determinism
def test_two_handles_record_and_train_the_same_bits():
    E, shape = 70, (96, 96)
    outs = []
    for _ in range(2):
        g, pol = _field(E, *shape)
        g.policy_lstm_set_precision(0, "bf16")
        ro = _rollout(g)
        tr = g.ppo_trainer(0, sequence_length=L, seed=7)
        tr.set_recurrent_precision("bf16")
        tr.advantages()
        state = {k: tr.read(k) for k in ("params", "adam_m", "adam_v")}
        counters = tr.counters()
        tr.update(2, 64, 3e-4, EPS, BETA)
        p1 = tr.read("params")
        # update twice from the same state: the same PARAMS
        for k, v in state.items():
            tr.write(k, v)
        tr.set_counters(*counters)
        tr.update(2, 64, 3e-4, EPS, BETA)
        assert_bits_equal(tr.read("params"), p1, "update twice from the same state")
        assert not np.array_equal(p1, state["params"])
        outs.append((ro, p1, tr.read("grad"), g.policy_forward(0, np.ones((3, pol.in_dim), np.float32))))
    for k in ("mu", "logits", "memory", "next_memory", "raw", "logp_cont", "logp_disc"):
        assert_bits_equal(outs[0][0][k], outs[1][0][k], ("two handles", k))
    assert_bits_equal(outs[0][1], outs[1][1], "two handles: PARAMS")
    assert_bits_equal(outs[0][2], outs[1][2], "two handles: GRAD")
    for x, y in zip(outs[0][3], outs[1][3]):
        assert_bits_equal(x, y, "two handles: the published policy")


# ---- 8. refusals, each with the state as it was; resume
def _refused(call, code, word):
    with pytest.raises(_lib.HkError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals_and_resume(tmp_path):
    g, pol = _field(5, 32, 32)
    plain = Policy.random(g.obs_dim * 4, 32, 2, 3, seed=9)
    g2 = TW.rl_env(2, 4)
    assert g2.attach_policy(plain, [0], P) == 0
    # the new entry points on the wrong kind of policy / trainer
    _refused(lambda: g2.policy_lstm_set_precision(0, "bf16"), _lib.HK_ERR_INVALID, "hk_policy_set_precision")
    assert g2.policy_precision(0) == "f32"
    tp = g2.ppo_trainer(0)
    _refused(lambda: tp.set_recurrent_precision("bf16"), _lib.HK_ERR_INVALID, "hk_ppo_set_precision")
    assert tp.precision == "f32"
    tp.set_precision("bf16")                                 # the plain trainer's own switch works as before
    assert tp.precision == "bf16"
    # the recurrent-critic trainer
    gc, polc = _field(5, 32, 32)
    tc = gc.ppo_trainer(0, sequence_length=L, critic_memory_size=64)
    _refused(lambda: tc.set_recurrent_precision("bf16"), _lib.HK_ERR_UNSUPPORTED, "recurrent critic")
    assert tc.precision == "f32"
    # a bad precision or index
    assert g.L.hk_policy_lstm_set_precision(g.h, 0, 7) == _lib.HK_ERR_INVALID and "precision" in g.L.hk_last_error(g.h).decode()
    assert g.L.hk_policy_lstm_set_precision(g.h, 2, 1) == _lib.HK_ERR_INVALID and "index" in g.L.hk_last_error(g.h).decode()
    tr = g.ppo_trainer(0, sequence_length=L, seed=2)
    assert g.L.hk_ppo_recurrent_set_precision(g.h, tr.t, 7) == _lib.HK_ERR_INVALID and "precision" in g.L.hk_last_error(g.h).decode()
    assert g.L.hk_ppo_recurrent_set_precision(g.h, 5, 1) == _lib.HK_ERR_INVALID
    with pytest.raises(ValueError):
        g.policy_lstm_set_precision(0, "fp8")
    with pytest.raises(ValueError):
        tr.set_recurrent_precision("fp8")
    assert g.policy_precision(0) == "f32" and tr.precision == "f32"
    # the old entry points refuse exactly as before
    _refused(lambda: g.policy_set_precision(0, "bf16"), _lib.HK_ERR_UNSUPPORTED, "policy with memory")
    _refused(lambda: tr.set_precision("bf16"), _lib.HK_ERR_UNSUPPORTED, "precision")
    assert g.policy_precision(0) == "f32" and tr.precision == "f32"
    # an open rollout
    g.rollout_begin(R)
    _refused(lambda: g.policy_lstm_set_precision(0, "bf16"), _lib.HK_ERR_INVALID, "rollout is open")
    assert g.policy_precision(0) == "f32"
    g.step(R * P)
    g.rollout_close()
    # resume through a checkpoint keeps precision and bits
    g.policy_lstm_set_precision(0, "bf16")
    tr.set_recurrent_precision("bf16")
    tr.advantages()
    tr.update(1, 8, 3e-4, EPS, BETA)
    path = str(tmp_path / "ck.npz")
    tr.save(path)
    assert ppo.checkpoint_read(path)["precision"] == "bf16"
    gb, _ = _field(5, 32, 32)
    gb.policy_lstm_set_precision(0, "bf16")
    tb = gb.ppo_trainer(0, sequence_length=L, seed=2)
    tb.load(path)
    assert tb.precision == "bf16" and tb.counters() == tr.counters()
    for k in ("params", "adam_m", "adam_v", "shadow"):
        assert_bits_equal(tb.read(k), tr.read(k), ("resume", k))
    obs = np.ones((3, pol.in_dim), np.float32)
    for x, y in zip(g.policy_forward(0, obs), gb.policy_forward(0, obs)):
        assert_bits_equal(x, y, "resume: the published policy")
