"""HK_POLICY_PREC_BF16 (include/hk.h beside hk_policy_attach): the actor's trunk on the bf16 matrix cores is the bf16 trainer's
forward bit for bit — composed on the host from the trainer's product kernel (policy_bf16_restate.py) and through a recorded rollout, where
rho == 1 returns exactly — switching back is the oracle's chain, publish reaches the bf16 copies, the recorder's identities and determinism
hold, and every refusal of the contract.  The field of test_ppo_gpu.py (24 envs, 2v2 Oval, DecisionPeriod 2) with R = 12 decisions."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import policy_bf16_restate as PB
from hierarchicalkarting_amd import _lib, ppo
from hierarchicalkarting_amd.policy import Policy
from parity import assert_bits_equal
from rollout_restate import logp_cont, logp_disc
from test_ppo_branches_gpu import PRE_TICKS, RESET_ENVS, SHAPES
from test_ppo_gpu import KW, P, _actors, _ids, _rows, _torch

pytestmark = pytest.mark.gpu
RL, R = _lib.HK_LOW_RL, 12


def _field(prec, record=True):
    """test_ppo_gpu._env with both actors in `prec` and a rollout of R decisions"""
    import hierarchicalkarting_amd as hk
    _torch()
    g = hk.RacingEnv(hk.make_config(24, 4, **KW))
    g.reset()
    pols = _actors(g.obs_dim)
    for k, (pol, slots) in enumerate(pols):
        assert g.attach_policy(pol, slots, P, precision=prec) == k
        assert g.policy_precision(k) == prec
    if record:
        g.rollout_begin(R)
        g.step(R * P)
        g.rollout_close()
    return g, pols


@functools.lru_cache(maxsize=None)
def _recorded(prec):
    """one recorded field per precision for the tests that leave its parameters alone"""
    return _field(prec)


# ---- 1. the trunk against the trainer's product kernel, bit for bit
# (agents, stack) -> K: (2, 1) 54, (4, 1) 78, (2, 2) 108, (4, 4) 312, (4, 8) 624 — K tails 6, 14, 12, 8, 0 mod 16, one K above a chunk of 320.
# hidden 32 .. 128: one block per wave; 160 .. 256: two; 32 / 96 / 160 / 224 leave half a 64-wide chunk of padding in the later layers.
CASES = [
    dict(agents=4, stack=4, hidden=256, layers=3, rows=63, normalize=True),       # the reference's shape
    dict(agents=4, stack=4, hidden=256, layers=2, rows=130, normalize=True),
    dict(agents=4, stack=4, hidden=160, layers=4, rows=65, normalize=True),
    dict(agents=4, stack=4, hidden=224, layers=1, rows=64, normalize=False),
    dict(agents=4, stack=8, hidden=32, layers=4, rows=65, normalize=True),
    dict(agents=4, stack=8, hidden=256, layers=1, rows=1, normalize=False),
    dict(agents=4, stack=8, hidden=96, layers=2, rows=130, normalize=True),
    dict(agents=4, stack=1, hidden=128, layers=2, rows=64, normalize=True),
    dict(agents=4, stack=1, hidden=32, layers=1, rows=63, normalize=False),
    dict(agents=2, stack=1, hidden=96, layers=4, rows=1, normalize=True),
    dict(agents=2, stack=1, hidden=160, layers=2, rows=130, normalize=False),
    dict(agents=2, stack=2, hidden=128, layers=1, rows=65, normalize=True),
    dict(agents=2, stack=2, hidden=224, layers=2, rows=64, normalize=True),
]


def _case_id(c):
    return "a%d_s%d_h%dx%d_r%d_%s" % (c["agents"], c["stack"], c["hidden"], c["layers"], c["rows"], "norm" if c["normalize"] else "raw")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_trunk_is_the_trainers_product_kernel(case):
    import hierarchicalkarting_amd as hk
    _torch()
    A = case["agents"]
    g = hk.RacingEnv(hk.make_config(8, A, low_mode=[RL] * A))
    g.reset()
    K = g.obs_dim * case["stack"]
    assert K == {(2, 1): 54, (4, 1): 78, (2, 2): 108, (4, 4): 312, (4, 8): 624}[(A, case["stack"])]
    pol = Policy.random(K, case["hidden"], case["layers"], stack=case["stack"], seed=31, normalize=case["normalize"])
    assert g.attach_policy(pol, [0], P) == 0
    g.policy_set_precision(0, "bf16")
    rng = np.random.default_rng(K + case["hidden"] + case["rows"])
    obs = (3.0 * rng.standard_normal((case["rows"], K))).astype(np.float32)       # (some inputs land on the +-5 clip)
    mu, lg = g.policy_forward(0, obs)
    want_mu, want_lg = PB.policy_bf16_of(g, pol, obs)
    assert_bits_equal(mu, want_mu, "mu")
    assert_bits_equal(lg, want_lg, "logits")
    assert np.isfinite(mu).all() and np.abs(mu).max() > 0.0


# ---- 2. back to fp32
def test_switching_back_is_the_oracles_chain():
    import hierarchicalkarting_amd as hk
    _torch()
    cfg = hk.make_config(8, 4, low_mode=[RL] * 4)
    g, o = hk.RacingEnv(cfg), O.OracleEnv(cfg)
    g.reset()
    pol = Policy.random(g.obs_dim * 4, 256, 3, seed=1)
    for e in (g, o):
        assert e.attach_policy(pol, [0, 1], P) == 0
    obs = (3.0 * np.random.default_rng(2).standard_normal((130, pol.in_dim))).astype(np.float32)
    want = o.policy_forward(0, obs)
    assert g.policy_precision(0) == "f32"
    first = g.policy_forward(0, obs)
    g.policy_set_precision(0, "bf16")
    second = g.policy_forward(0, obs)
    g.policy_set_precision(0, "f32")
    third = g.policy_forward(0, obs)
    for got, tag in ((first, "before the switch"), (third, "after switching back")):
        assert_bits_equal(got[0], want[0], "mu " + tag)
        assert_bits_equal(got[1], want[1], "logits " + tag)
    assert not np.array_equal(second[0], want[0]) and not np.array_equal(second[1], want[1])


# ---- 3. rho == 1 is back
def _unchanged(g, pols, p, critic=None):
    """one minibatch of all rows at unchanged parameters, trainer in bf16 -> (stats, max |MB_MU - MU|, MB_MU, MB_LOGITS, recorded fields)"""
    torch = _torch()
    tr = g.ppo_trainer(p, critic=critic, precision="bf16")
    tr.advantages()
    X, f, _, _ = _rows(g, pols, p)
    n = X.shape[0]
    st = tr.minibatch(_ids(torch, np.arange(n)), 0.2, 5e-3)
    return st, float(np.abs(tr.read("mb_mu") - f["mu"]).max()), tr.read("mb_mu"), tr.read("mb_logits").reshape(n, -1), f


def _assert_rho_one(g, pols, p, what, critic=None):
    st, _, mb_mu, mb_lg, f = _unchanged(g, pols, p, critic)
    assert_bits_equal(mb_mu, f["mu"], what + " MB_MU against the recorded MU")
    assert_bits_equal(mb_lg, f["logits"], what + " MB_LOGITS against the recorded LOGITS")
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0, (what, st)


@pytest.mark.parametrize("p", [0, 1], ids=["sampled_312_256x3", "deterministic_312_128x2"])
def test_rho_is_one_with_policy_and_trainer_in_bf16(p):
    g, pols = _recorded("bf16")
    _assert_rho_one(g, pols, p, "policy %d" % p)
    # the control: the same trainer on a policy left in fp32 sees the bf16 rounding of the trunk (today's behaviour)
    g32, pols32 = _recorded("f32")
    st, max_mu, _, _, _ = _unchanged(g32, pols32, p)
    assert max_mu > 0.0 and st["skipped"] == 0.0, (max_mu, st)


def test_rho_is_one_on_a_short_stack_under_a_larger_one():
    """test_ppo_branches_gpu's "stack2_of_8_h96x2": K = 156, 96 x 2, stack 2 beside a stack of 8 on the handle, a rollout that begins
    mid-episode with live RING0 and clears inside it"""
    import hierarchicalkarting_amd as hk
    _torch()
    c = SHAPES["stack2_of_8_h96x2"]
    g = hk.RacingEnv(hk.make_config(8, 4, low_mode=[RL] * 4, rewards=1, max_episode_steps=100, jitter_seed=4))
    g.reset()
    pols = []
    for k, (stack, hidden, layers, norm) in enumerate(c["actors"]):
        pol = Policy.random(g.obs_dim * stack, hidden, layers, stack=stack, seed=21 + k, normalize=norm)
        slots = [2 * k, 2 * k + 1]
        assert g.attach_policy(pol, slots, P, precision="bf16") == k
        pols.append((pol, slots))
    g.step(PRE_TICKS)
    g.reset(RESET_ENVS)
    g.step(37 + 1)
    g.rollout_begin(R)
    g.step(R * P)
    g.rollout_close()
    p = c["train"]
    pol = pols[p][0]
    assert pol.in_dim == 156 and pol.hidden == 96 and len(pol.W) == 2
    ro = g.rollout()
    assert ro["ring0"].any() and ro["first"][:, :, pols[p][1]].any()
    critic = Policy.random(pol.in_dim, c["critic"][0], c["critic"][1], n_branch=1, stack=pol.stack, seed=77, normalize=False)
    _assert_rho_one(g, pols, p, "stack 2 of 8", critic)


# ---- 4. publish reaches the bf16 copies
def test_publish_reaches_the_bf16_copies():
    import hierarchicalkarting_amd as hk
    torch = _torch()
    g, pols = _field("bf16")
    pol = pols[0][0]
    tr = g.ppo_trainer(0, seed=3, precision="bf16")
    tr.advantages()
    st = tr.update(epochs=1, minibatch=256, lr=3e-3, eps=0.2, beta=5e-3)
    assert np.isfinite(list(st.values())).all()
    ap = tr.actor_params()
    assert not np.array_equal(ap["W0"], pol.W[0])
    # the policy's bf16 weights are the trainer's shadow: the forward is the host composition on the shadow's bits
    sh = ppo.split_params(tr.shadow()[:tr.n_actor], tr.actor_layout)
    L = len(pol.W)
    assert all(np.array_equal(sh["W%d" % l], ppo.bf16_round(ap["W%d" % l])) for l in range(L))
    obs = (3.0 * np.random.default_rng(5).standard_normal((65, pol.in_dim))).astype(np.float32)
    mu, lg = g.policy_forward(0, obs)
    want_mu, want_lg = PB.policy_bf16(g, obs, pol.norm_mean, pol.norm_std, [sh["W%d" % l] for l in range(L)], [ap["b%d" % l] for l in range(L)],
                                      ap["W_mu"], ap["b_mu"], ap["W_branch"], ap["b_branch"])
    assert_bits_equal(mu, want_mu, "mu after publish")
    assert_bits_equal(lg, want_lg, "logits after publish")
    # a second rollout, recorded with the published weights: rho == 1 again
    g.rollout_begin(R)
    g.step(R * P)
    g.rollout_close()
    tr.advantages()
    X, f, _, _ = _rows(g, pols, 0)
    n = X.shape[0]
    st = tr.minibatch(_ids(torch, np.arange(n)), 0.2, 5e-3)
    assert_bits_equal(tr.read("mb_mu"), f["mu"], "MB_MU on the second rollout")
    assert_bits_equal(tr.read("mb_logits").reshape(n, -1), f["logits"], "MB_LOGITS on the second rollout")
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0, st
    # back in fp32 the policy is the oracle's chain on the published fp32 masters
    g.policy_set_precision(0, "f32")
    o = O.OracleEnv(hk.make_config(24, 4, **KW))
    assert o.attach_policy(tr.actor(), [0, 1], P) == 0
    got, want = g.policy_forward(0, obs), o.policy_forward(0, obs)
    assert_bits_equal(got[0], want[0], "fp32 mu on the published masters")
    assert_bits_equal(got[1], want[1], "fp32 logits on the published masters")


# ---- 5. the recorder's identities
def test_recorder_identities_in_bf16_mode():
    g, pols = _recorded("bf16")
    ro = g.rollout()
    for k, (pol, slots) in enumerate(pols):
        raw, mu = ro["raw"][:, :, slots], ro["mu"][:, :, slots]
        lg, br = ro["logits"][:, :, slots, :pol.n_branch], ro["branch"][:, :, slots]
        assert_bits_equal(ro["steer"][:, :, slots], np.clip(raw, np.float32(-3), np.float32(3)) / np.float32(3), "STEER %d" % k)
        assert np.allclose(ro["logp_cont"][:, :, slots], logp_cont(raw, mu, pol.log_sigma[0]), rtol=1e-6, atol=2e-6), k
        assert np.allclose(ro["logp_disc"][:, :, slots], logp_disc(lg, br), rtol=1e-6, atol=2e-6), k
        if pol.deterministic:
            assert_bits_equal(raw, mu, "RAW == MU %d" % k)
            assert np.array_equal(br, lg.argmax(axis=-1)), k
        else:
            assert (raw != mu).mean() > 0.9 and len(np.unique(br)) == pol.n_branch, k
    # ... and the rows are the bf16 chain's, not the fp32 one's: the first decision sees the same observations in both fields
    ro32 = _recorded("f32")[0].rollout()
    assert np.array_equal(ro["obs"][0], ro32["obs"][0]) and not np.array_equal(ro["mu"][0], ro32["mu"][0])


# ---- 6. determinism
def test_two_handles_record_the_same_bits():
    ro1, ro2 = _recorded("bf16")[0].rollout(), _field("bf16")[0].rollout()
    assert set(ro1) == set(ro2)
    for name in sorted(ro1):
        assert_bits_equal(ro1[name], ro2[name], "rollout field " + name)


# ---- 7. refusals
def test_refusals():
    g, pols = _field("f32", record=False)
    Lb, h = g.L, g.h
    INV, F32, BF16 = _lib.HK_ERR_INVALID, _lib.HK_POLICY_PREC_F32, _lib.HK_POLICY_PREC_BF16
    msg = lambda: Lb.hk_last_error(h).decode()
    for pol_index in (-1, 2, 9):
        assert Lb.hk_policy_set_precision(h, pol_index, BF16) == INV and "bad policy index" in msg()
        assert Lb.hk_policy_get_precision(h, pol_index) == INV and "bad policy index" in msg()
    for prec in (-1, 2, 7):
        assert Lb.hk_policy_set_precision(h, 0, prec) == INV and "unknown precision" in msg()
    assert Lb.hk_policy_get_precision(h, 0) == F32 and Lb.hk_policy_get_precision(h, 1) == F32
    with pytest.raises(ValueError):
        g.policy_set_precision(0, "fp16")
    with pytest.raises(ValueError):
        g.attach_policy(pols[0][0], [0], P, precision="half")
    g.policy_set_precision(1, "bf16")                     # per policy
    assert g.policy_precision(0) == "f32" and g.policy_precision(1) == "bf16"
    g.rollout_begin(4)
    g.step(P)
    for k, prec in ((0, BF16), (1, F32), (1, BF16)):      # any switch while a rollout is open, one to the current precision included
        assert Lb.hk_policy_set_precision(h, k, prec) == INV and "rollout is open" in msg()
    assert g.policy_precision(0) == "f32" and g.policy_precision(1) == "bf16"
    g.rollout_close()
    g.policy_set_precision(0, "bf16")
    g.policy_set_precision(1, "f32")
    assert g.policy_precision(0) == "bf16" and g.policy_precision(1) == "f32"
    g.synchronize()
