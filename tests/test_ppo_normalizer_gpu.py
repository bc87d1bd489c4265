"""The running observation normaliser on the device (include/hk.h "PPO trainer" NORMALISER) against float64 numpy on
rollout.stacked_inputs of the downloaded rollout (normalizer_restate.py): one update on the base shape and on the odd ones, accumulation over
rollouts and the get -> set round trip, every consumer of the published statistics, the two call orders, no change without opt-in, refusals.
The bounds are those of an fp64 accumulation (normalizer_restate.reference); published values and repeated calls are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import normalizer_restate as NR
import oracle_lib as O
import policy_bf16_restate as PB
import ppo_restate as PR
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.ppo import normalizer_merge
from hierarchicalkarting_amd.rollout import stacked_inputs
from parity import assert_bits_equal
from test_ppo_branches_gpu import PRE_TICKS, RESET_ENVS, R_SHAPES
from test_ppo_gpu import KW, P, R, _env, _ids, _rows, _torch

pytestmark = pytest.mark.gpu
RL, INVALID = _lib.HK_LOW_RL, _lib.HK_ERR_INVALID


def _X(g, pols, p, rows=None):
    """the un-normalised stacked inputs of policy p's rows [n, in_dim] (the completed rows, or the first `rows`) and the rollout"""
    ro = g.rollout()
    pol, slots = pols[p]
    rows = g.rollout_rows() if rows is None else rows
    return stacked_inputs(ro, slots, pol.stack)[:rows].reshape(-1, pol.in_dim), ro


def _snapshot(tr):
    steps, mean, m2 = tr.normalizer_state()
    return steps, mean, m2, tr.read("norm_mean"), tr.read("norm_std")


def _assert_same(a, b, what):
    assert a[0] == b[0], what
    for x, y, name in zip(a[1:], b[1:], ("mean", "m2", "published mean", "published std")):
        assert np.array_equal(NR.bits(x), NR.bits(y)), "%s: %s" % (what, name)


def _update_and_check(g, pols, p, tr, what, rows=None):
    """init(1) on the attached statistics, one update against the reference, then the same update from the same state: the same bits"""
    pol = pols[p][0]
    tr.normalizer_init(1)
    before = tr.normalizer_state()
    assert before[0] == 1 and np.array_equal(before[1], pol.norm_mean.astype(np.float64))
    assert np.array_equal(before[2], pol.norm_std.astype(np.float64) ** 2)
    assert_bits_equal(tr.read("norm_mean"), pol.norm_mean, what + ": init publishes nothing (mean)")
    assert_bits_equal(tr.read("norm_std"), pol.norm_std, what + ": init publishes nothing (std)")
    X, ro = _X(g, pols, p, rows)
    tr.normalizer_update()
    NR.assert_update(tr, before, X, what)
    first = _snapshot(tr)
    tr.normalizer_load(*before)
    assert_bits_equal(tr.read("norm_mean"), np.float32(before[1]), what + ": load publishes (mean)")
    tr.normalizer_update()
    _assert_same(_snapshot(tr), first, what + ": the same update twice")
    return X, ro


# ---- 1. the base shape
@pytest.mark.parametrize("p", [0, 1], ids=["sampled_312_256x3", "deterministic_312_128x2"])
def test_base_shape(p):
    g, pols = _env()
    X, ro = _update_and_check(g, pols, p, g.ppo_trainer(p), "base shape, policy %d" % p)
    assert X.shape == (R * 24 * 2, 312)
    assert ro["first"][1:][:, :, pols[p][1]].any(), "no FIRST mid-rollout"


# ---- 2. odd shapes
def _odd_env(actors):
    """test_ppo_branches_gpu's 8-env set-up: a rollout that begins mid-episode after a partial reset (live RING0, FIRST on inner rows)"""
    import hierarchicalkarting_amd as hk
    _torch()
    g = hk.RacingEnv(hk.make_config(8, 4, low_mode=[RL] * 4, rewards=1, max_episode_steps=100, jitter_seed=4))
    g.reset()
    pols = []
    for k, (stack, hidden, layers) in enumerate(actors):
        pol = Policy.random(g.obs_dim * stack, hidden, layers, stack=stack, seed=21 + k, normalize=True)
        slots = [2 * k, 2 * k + 1]
        assert g.attach_policy(pol, slots, P) == k
        pols.append((pol, slots))
    g.step(PRE_TICKS)
    g.reset(RESET_ENVS)
    g.step(37 + 1)
    g.rollout_begin(R_SHAPES)
    g.step(R_SHAPES * P)
    g.rollout_close()
    return g, pols


@pytest.mark.parametrize("actors,p", [(((8, 32, 4), (2, 96, 2)), 0), (((8, 32, 4), (2, 96, 2)), 1), (((1, 32, 1), (4, 256, 3)), 0)],
                         ids=["stack8", "stack2_under_smax8", "stack1_under_smax4"])
def test_odd_stacks_on_a_rollout_that_begins_mid_episode(actors, p):
    g, pols = _odd_env(actors)
    pol, slots = pols[p]
    X, ro = _update_and_check(g, pols, p, g.ppo_trainer(p), "stack %d" % pol.stack)
    smax = max(q.stack for q, _ in pols)
    first = ro["first"][:, :, slots]
    assert ro["ring0"].shape[2] == smax - 1 and first[1:].any()
    if pol.stack > 1:
        assert all(ro["ring0"][:, a, smax - pol.stack:].any() for a in slots), "RING0 of the driven slots"
        assert (X.reshape(R_SHAPES, 8, 2, pol.stack, -1)[:, :, :, 0] == 0.0).all(axis=-1).any(), "no absent entry"
    if pol.stack > 2:
        assert first[1:pol.stack - 1].any(), "no clear that hides live RING0 entries"


def test_rollout_closed_early_counts_its_completed_rows_only():
    g, pols = _env(record=False)
    g.rollout_begin(R)
    g.step((R - 17) * P)
    g.rollout_close()
    assert g.rollout_rows() == R - 17
    tr = g.ppo_trainer(0)
    X, ro = _update_and_check(g, pols, 0, tr, "short rollout")
    assert ro["obs"].shape[0] == R and X.shape[0] == (R - 17) * 24 * 2
    assert tr.normalizer_state()[0] == 1 + (R - 17) * 24 * 2


# ---- 3. accumulation and the checkpoint
def test_three_rollouts_accumulate_and_the_state_round_trips():
    g, pols = _env(record=False)
    pol = pols[0][0]
    tr = g.ppo_trainer(0)
    tr.normalizer_init(1)
    start = tr.normalizer_state()
    Xs = []
    for r in (20, 7, 33):
        g.rollout_begin(r); g.step(r * P); g.rollout_close()
        before = tr.normalizer_state()
        X, _ = _X(g, pols, 0)
        tr.normalizer_update()
        NR.assert_update(tr, before, X, "rollout of %d rows" % r)
        Xs.append(X)
    Xall = np.concatenate(Xs)
    steps, mean, m2 = NR.assert_update(tr, start, Xall, "three rollouts against one merge of their %d rows" % Xall.shape[0])
    N, m, M = normalizer_merge(*start, Xall)                  # (the host twin is the reference's formulas: the same bits)
    ref = NR.reference(*start, Xall)
    assert N == steps == ref[0] and np.array_equal(NR.bits(m), NR.bits(ref[1])) and np.array_equal(NR.bits(M), NR.bits(ref[2]))
    # get -> set into a second trainer: state and published values bit for bit
    a = _snapshot(tr)
    t2 = g.ppo_trainer(0)
    with pytest.raises(_lib.HkError):
        t2.normalizer_state()                        # (no state yet)
    t2.normalizer_load(*a[:3])
    _assert_same(_snapshot(t2), a, "get -> set round trip")
    assert not np.array_equal(a[3], pol.norm_mean) and not np.array_equal(a[4], pol.norm_std)


# ---- 5. every consumer follows
def _edge_obs(in_dim, rows, seed):
    obs = (np.random.default_rng(seed).standard_normal((rows, in_dim)) * 4).astype(np.float32)
    obs[0, :7] = [0.0, -0.0, 1e-30, -1e30, 5.0, -5.0, 1e30]
    return obs


def test_inference_follows_in_both_precisions():
    import hierarchicalkarting_amd as hk
    g, pols = _env()
    tr = g.ppo_trainer(0)
    obs = _edge_obs(pols[0][0].in_dim, 300, 5)
    mu0, lg0 = g.policy_forward(0, obs)
    tr.normalizer_init(1)
    tr.normalizer_update()
    a = tr.actor()
    assert_bits_equal(a.norm_mean, tr.read("norm_mean"), "actor() hands back the published mean")
    assert_bits_equal(a.norm_std, tr.read("norm_std"), "actor() hands back the published std")
    assert not np.array_equal(a.norm_mean, pols[0][0].norm_mean) and np.array_equal(a.W[0], pols[0][0].W[0])
    o = O.OracleEnv(hk.make_config(24, 4, **KW))
    o.reset()
    o.attach_policy(a, [0, 1], P)
    want = o.policy_forward(0, obs)
    mu, lg = g.policy_forward(0, obs)
    assert_bits_equal(mu, want[0], "mu on the new statistics")
    assert_bits_equal(lg, want[1], "logits on the new statistics")
    assert not np.array_equal(mu, mu0)
    # bf16 and back
    g.policy_set_precision(0, "bf16")
    bm, bl = g.policy_forward(0, obs)
    wm, wl = PB.policy_bf16_of(g, a, obs)
    assert_bits_equal(bm, wm, "bf16 mu on the new statistics")
    assert_bits_equal(bl, wl, "bf16 logits on the new statistics")
    g.policy_set_precision(0, "f32")
    mu2, lg2 = g.policy_forward(0, obs)
    assert_bits_equal(mu2, want[0], "mu after switching back")
    assert_bits_equal(lg2, want[1], "logits after switching back")
    # the other policy is untouched
    assert_bits_equal(g.ppo_trainer(1).read("norm_mean"), pols[1][0].norm_mean, "the other policy's mean")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_exact_order_keeps_rho_at_one(prec):
    """advantages -> update -> normalizer_update: the new statistics act from the next rollout on, whose training forward is its recorded one"""
    torch = _torch()
    g, pols = _env(record=False)
    for k in (0, 1):
        g.policy_set_precision(k, prec)
    tr = g.ppo_trainer(0, precision=prec)
    tr.normalizer_init(1)
    g.rollout_begin(12); g.step(12 * P); g.rollout_close()
    tr.advantages()
    tr.normalizer_update()
    mean1 = tr.read("norm_mean")
    assert not np.array_equal(mean1, pols[0][0].norm_mean)
    g.rollout_begin(16); g.step(16 * P); g.rollout_close()
    tr.advantages()
    X, f, _, _ = _rows(g, pols, 0)
    n = X.shape[0]
    st = tr.minibatch(_ids(torch, np.arange(n)), 0.2, 5e-3)
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0, st
    assert_bits_equal(tr.read("mb_mu"), f["mu"], prec + " MB_MU against the recorded MU")
    assert_bits_equal(tr.read("mb_logits").reshape(n, -1), f["logits"], prec + " MB_LOGITS against the recorded LOGITS")
    assert_bits_equal(tr.read("norm_mean"), mean1, "the statistics the rollout ran under")


def test_ml_agents_order_makes_the_advantages_stale():
    """normalizer_update -> advantages -> update, on the same rollout: a minibatch is refused until advantages has run again, for every trainer
    of the policy; V_OLD is then the critic on inputs normalised with the NEW statistics"""
    torch = _torch()
    g, pols = _env()
    pol = pols[0][0]
    tr, other, t1 = g.ppo_trainer(0), g.ppo_trainer(0), g.ppo_trainer(1)
    for t in (tr, other, t1):
        t.advantages()
    ids = _ids(torch, np.arange(64))
    L, h = g.L, g.h
    assert L.hk_ppo_minibatch(h, tr.t, ids.data_ptr(), 64, 0.2, 0.0, None) == 0
    tr.normalizer_init(1)
    assert L.hk_ppo_minibatch(h, tr.t, ids.data_ptr(), 64, 0.2, 0.0, None) == 0          # init publishes nothing: nothing is stale
    v_before = tr.read("v_old")
    tr.normalizer_update()
    for t in (tr, other):
        assert L.hk_ppo_minibatch(h, t.t, ids.data_ptr(), 64, 0.2, 0.0, None) == INVALID
        assert L.hk_ppo_update(h, t.t, 1, 64, 1e-4, 0.2, 0.0, None) == INVALID
    assert b"normaliser" in L.hk_last_error(h)
    assert L.hk_ppo_minibatch(h, t1.t, ids.data_ptr(), 64, 0.2, 0.0, None) == 0          # the other policy's trainer is not concerned
    tr.advantages()
    st = tr.minibatch(_ids(torch, np.arange(tr.read("adv").size)), 0.2, 5e-3)
    assert st["approx_kl"] != 0.0                                                        # LOGP_* were recorded under the old statistics
    assert L.hk_ppo_minibatch(h, other.t, ids.data_ptr(), 64, 0.2, 0.0, None) == INVALID  # (its own advantages are still the old ones)
    X, _ = _X(g, pols, 0)
    a = tr.actor()
    cp = PR.tensors(tr.critic_params())
    v_ref = PR.critic_values(PR.normalise(X, a.norm_mean, a.norm_std), cp, len(tr.critic_policy.W)).numpy()
    v_dev = tr.read("v_old")
    err, bound = np.abs(v_dev - v_ref).max(), 1e-5 * max(1.0, np.abs(v_ref).max())
    print("V_OLD on the new statistics: max error %.3g (bound %.3g); moved by %.3g" % (err, bound, np.abs(v_dev - v_before).max()))
    assert err <= bound
    assert np.abs(v_dev - v_before).max() > bound           # (the old statistics would not pass)


# ---- 6. unchanged without opt-in
def test_a_trainer_that_never_opts_in_is_unchanged():
    outs = []
    for opt_in_elsewhere in (False, True):
        g, pols = _env()
        tr = g.ppo_trainer(0, seed=7)
        if opt_in_elsewhere:
            t1 = g.ppo_trainer(1)
            t1.normalizer_init(1)
            t1.normalizer_update()
            assert not np.array_equal(t1.read("norm_mean"), pols[1][0].norm_mean)
        tr.advantages()
        st = tr.update(2, 256, 3e-4, 0.2, 5e-3)
        outs.append((tr.read("params"), tr.read("adam_m"), tr.read("adam_v"), st, tr.read("norm_mean"), tr.read("norm_std")))
        assert_bits_equal(outs[-1][4], pols[0][0].norm_mean, "the statistics stay as attached")
        assert_bits_equal(outs[-1][5], pols[0][0].norm_std, "the statistics stay as attached")
    for k, name in enumerate(("params", "adam_m", "adam_v")):
        assert_bits_equal(outs[0][k], outs[1][k], name + " with and without a running normaliser on the other policy")
    assert outs[0][3] == outs[1][3]


# ---- 7. refusals
def test_refusals_leave_state_and_published_values():
    import hierarchicalkarting_amd as hk
    torch = _torch()
    g = hk.RacingEnv(hk.make_config(8, 4, low_mode=[RL] * 4, rewards=1, max_episode_steps=100, jitter_seed=4))
    g.reset()
    D = g.obs_dim
    pol = Policy.random(D * 2, 32, 1, stack=2, seed=3, normalize=True)
    raw = Policy.random(D * 2, 32, 1, stack=2, seed=4, normalize=False)
    g.attach_policy(pol, [0, 1], P)
    g.attach_policy(raw, [2, 3], P)
    L, h = g.L, g.h
    tr, tn = g.ppo_trainer(0), g.ppo_trainer(1)
    K = pol.in_dim
    steps = C.c_int64(0)
    mean, m2 = np.zeros(K), np.ones(K)
    pm, pp = lambda a: C.c_void_p(a.ctypes.data), lambda: (tr.read("norm_mean"), tr.read("norm_std"))
    get = lambda t: L.hk_ppo_normalizer_get(h, t, C.byref(steps), pm(mean), pm(m2))
    # a policy attached with normalize == 0 has no buffers
    assert L.hk_ppo_normalizer_init(h, tn.t, 1) == INVALID and L.hk_ppo_normalizer_update(h, tn.t) == INVALID
    assert get(tn.t) == INVALID and L.hk_ppo_normalizer_set(h, tn.t, 1, pm(mean), pm(m2)) == INVALID
    assert L.hk_ppo_count(h, tn.t, _lib.PPO_FIELDS["norm_mean"]) == 0 and L.hk_ppo_ptr(h, tn.t, _lib.PPO_FIELDS["norm_std"]) is None
    # a bad trainer; before init
    assert L.hk_ppo_normalizer_init(h, 9, 1) == INVALID and L.hk_ppo_normalizer_update(h, -1) == INVALID
    assert L.hk_ppo_normalizer_update(h, tr.t) == INVALID and get(tr.t) == INVALID
    # init's own rules
    assert L.hk_ppo_normalizer_init(h, tr.t, 0) == INVALID and L.hk_ppo_normalizer_init(h, tr.t, -5) == INVALID
    assert get(tr.t) == INVALID
    tr.normalizer_init(3)
    ref = _snapshot(tr)
    assert ref[0] == 3 and np.array_equal(ref[2], pol.norm_std.astype(np.float64) ** 2 * 3)

    def unchanged(what):
        _assert_same(_snapshot(tr), ref, what)
    assert L.hk_ppo_normalizer_update(h, tr.t) == INVALID; unchanged("update before any rollout")
    for bad_steps, bad_mean, bad_m2, what in ((0, mean, m2, "steps 0"), (1, np.where(np.arange(K) == 3, np.nan, 0.0), m2, "NaN mean"),
                                              (1, np.where(np.arange(K) == 3, np.inf, 0.0), m2, "Inf mean"),
                                              (1, mean, np.where(np.arange(K) == 5, 0.0, 1.0), "m2 0"), (1, mean, np.where(np.arange(K) == 5, -1.0, 1.0), "m2 < 0"),
                                              (1, mean, np.where(np.arange(K) == 5, np.inf, 1.0), "m2 Inf"), (1, mean, np.where(np.arange(K) == 5, np.nan, 1.0), "m2 NaN")):
        bm, b2 = np.ascontiguousarray(bad_mean, np.float64), np.ascontiguousarray(bad_m2, np.float64)
        assert L.hk_ppo_normalizer_set(h, tr.t, bad_steps, pm(bm), pm(b2)) == INVALID, what
        unchanged("set: " + what)
    assert L.hk_ppo_normalizer_set(h, tr.t, 1, None, pm(m2)) == INVALID; unchanged("set: NULL mean")
    # an open rollout refuses all four
    g.rollout_begin(4)
    assert L.hk_ppo_normalizer_init(h, tr.t, 1) == INVALID and L.hk_ppo_normalizer_update(h, tr.t) == INVALID
    assert get(tr.t) == INVALID and L.hk_ppo_normalizer_set(h, tr.t, 1, pm(mean), pm(m2)) == INVALID
    g.rollout_close()
    unchanged("an open rollout")
    assert g.rollout_rows() == 0
    assert L.hk_ppo_normalizer_update(h, tr.t) == INVALID; unchanged("a rollout with no completed row")
    # init on published values that are not a normaliser: a std of 0, a NaN mean (written through the published buffers, then restored)
    v = tr.views()
    keep_m, keep_s = v["norm_mean"].clone(), v["norm_std"].clone()
    g.synchronize()
    v["norm_std"][2] = 0.0
    torch.cuda.synchronize()
    assert L.hk_ppo_normalizer_init(h, tr.t, 1) == INVALID
    v["norm_std"].copy_(keep_s); v["norm_mean"][4] = float("nan"); torch.cuda.synchronize()
    assert L.hk_ppo_normalizer_init(h, tr.t, 1) == INVALID
    v["norm_mean"].copy_(keep_m); torch.cuda.synchronize()
    unchanged("init on a bad published value")
    # and what is allowed still works
    g.rollout_begin(3); g.step(3 * P); g.rollout_close()
    tr.normalizer_update()
    assert tr.normalizer_state()[0] == 3 + 3 * 8 * 2
