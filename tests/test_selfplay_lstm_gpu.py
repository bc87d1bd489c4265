"""Self-play for recurrent actors on the device (include/hk.h "SELF-PLAY" RECURRENT POOLS): hk_policy_pool_create_recurrent,
save / load / put / get of a slot that carries the LSTM cell, hk_policy_memory_clear, every refusal, and the SelfPlay driver around a recurrent
trainer with and without a recurrent critic, run twice and resumed through a file.

The field is test_ppo_lstm_gpu.py's: a 2-kart Oval, both karts RL, DecisionPeriod 2, rewards on, max_episode_steps 100 (auto-reset), the envs with
env % 4 == k restarted at tick k.  Here kart 0 is the learner's and kart 1 the opponent's, two attached policies of one shape.  Every compare is
assert_bits_equal: nothing on these paths rounds but the one documented sum fp32(b_ih + b_hh), which the inference outputs see on both sides."""
import ctypes as C

import numpy as np
import pytest

import policy_lstm_twin as TW
from hierarchicalkarting_amd import _lib, ppo
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.selfplay import SelfPlay, SnapshotPool, flat_to_policy, policy_to_flat
from parity import assert_bits_equal

pytestmark = pytest.mark.gpu
P, R, L = 2, 11, 4
SHAPES = [(32, 32, 2), (96, 96, 2), (128, 128, 3)]          # (H, m, trunk layers): the cell's smallest width, an odd multiple of 32, the largest
SHAPE_IDS = ["h%d_m%d_x%d" % s for s in SHAPES]
ENVS = [1, 5]
EPS, BETA, LR_ = 0.2, 5e-3, 3e-4
VECTORS = ("params", "adam_m", "adam_v")
FP = C.POINTER(C.c_float)
OBS = 54                                           # hk_obs_dim of the 2-kart field (216 = 4 x 54 in test_ppo_lstm_gpu.py); _field asserts it


def _torch():
    import torch
    torch.cuda.init()
    return torch


def _actor(D, shape, seed, stack=4, **kw):
    H, m, layers = shape
    return Policy.random(D * stack, H, layers, 3, stack=stack, seed=seed, memory_size=2 * m, **kw)


def _stagger(g):
    for k in (1, 2, 3):                            # the envs with env % 4 == k restart their episode after k ticks
        g.step(1)
        ids = np.array([e for e in range(g.E) if e % 4 == k], np.int32)
        if ids.size:
            g.reset(ids)


def _field(E, pols, ticks=92):
    """the field with pols[k] attached to kart k, staggered and stepped to `ticks` (0: left at the reset)"""
    _torch()
    g = TW.rl_env(E, 2, rewards=1, max_episode_steps=100, jitter_seed=9)
    assert g.obs_dim == OBS
    for k, pol in enumerate(pols):
        assert g.attach_policy(pol, [k], P) == k
    if ticks:
        _stagger(g)
        g.step(ticks - 3)
    return g


def _pair(E, shape, ticks=92, seeds=(4, 14), **kw):
    pols = [_actor(OBS, shape, s, **kw) for s in seeds]
    return _field(E, pols, ticks), pols


def _inputs(pol, rows=130, seed=0):
    r = np.random.default_rng(seed + pol.in_dim)
    return (2.0 * r.standard_normal((rows, pol.in_dim))).astype(np.float32), r.uniform(-1, 1, (rows, pol.memory_size)).astype(np.float32)


def _forward(g, index, pol, seed=0):
    return g.policy_forward(index, *_inputs(pol, seed=seed))


def _same_outputs(got, want, tag):
    for a, b, name in zip(got, want, ("mu", "logits", "mem_out")):
        assert_bits_equal(a, b, "%s: %s" % (tag, name))


def _record(g, rows):
    g.rollout_begin(rows); g.step(rows * P); g.rollout_close()
    return g.rollout()


def _same_rollouts(a, b, tag):
    assert sorted(a) == sorted(b)
    for k in a:
        assert_bits_equal(a[k], b[k], "%s: %s" % (tag, k))


def _ids(a):
    return _torch().as_tensor(np.asarray(a, np.int32), device="cuda:0")


# ---- 1. save -> get
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_save_then_get_is_the_attached_policy(shape):
    g, pols = _pair(1, shape, ticks=0)
    for p, pol in enumerate(pols):
        pool = SnapshotPool(g, p, 2)
        assert pool.pool == p and pool.count == sum(v.size for v in pol.arrays().values()) == g.L.hk_policy_pool_count(g.h, pool.pool)
        pool.save(1)
        flat = pool.get_flat(1)
        assert_bits_equal(flat, policy_to_flat(pol), "policy %d: the slot" % p)
        # the two biases as attached, each in its place, not their sum
        lay = ppo.split_params(flat, ppo.param_layout(pol.in_dim, pol.hidden, len(pol.W), pol.n_branch, pol.memory_size))
        assert_bits_equal(lay["b_ih"], pol.lstm["b_ih"], "b_ih")
        assert_bits_equal(lay["b_hh"], pol.lstm["b_hh"], "b_hh")
        assert not np.array_equal(lay["b_ih"], pol.lstm["b_ih"] + pol.lstm["b_hh"])
        got = pool.get(1)
        assert got.memory_size == pol.memory_size and (got.stack, got.seed, got.deterministic) == (pol.stack, pol.seed, pol.deterministic)
        for k, v in pol.arrays().items():
            assert_bits_equal(got.arrays()[k], v, "policy %d: %s" % (p, k))


# ---- 2. save after an update
def test_save_after_update_is_the_masters_and_the_published_statistics():
    g, pols = _pair(5, SHAPES[1])
    _record(g, R)
    tr = g.ppo_trainer(0, sequence_length=L, seed=3)
    tr.normalizer_init(1)
    tr.advantages()
    tr.update(1, 4, 3e-3, EPS, BETA)
    tr.normalizer_update()
    pool = SnapshotPool(g, 0, 1)
    pool.save(0)
    mean, std = tr.read("norm_mean"), tr.read("norm_std")
    assert_bits_equal(pool.get_flat(0), np.concatenate([tr.read("params")[:tr.n_actor], mean, std]), "the slot after update and publish")
    p = tr.actor_params()
    assert not np.array_equal(p["W_hh"], pols[0].lstm["W_hh"]) and not np.array_equal(p["b_hh"], pols[0].lstm["b_hh"])
    assert not np.array_equal(mean, pols[0].norm_mean)
    got = pool.get(0)
    for k in Policy.LSTM_KEYS:
        assert_bits_equal(got.lstm[k], p[k], k)


# ---- 3. put -> load against attaching on a fresh handle
@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_put_then_load_equals_attaching_on_a_fresh_handle(E, shape):
    g, pols = _pair(E, shape, ticks=0)
    D = g.obs_dim
    b = _actor(D, shape, 33)
    pool = SnapshotPool(g, 0, 3)
    pool.put(2, b)
    assert_bits_equal(pool.get_flat(2), policy_to_flat(b), "put -> get")
    before = _forward(g, 1, b)
    pool.load(2, 1)
    # the seed, the mode and the stack are the attached policy's: the fresh handle attaches B's arrays under them
    b_as_opponent = flat_to_policy(policy_to_flat(b), pols[1])
    assert b_as_opponent.seed == pols[1].seed
    fresh = _field(E, [pols[0], b_as_opponent], ticks=0)
    got, want = _forward(g, 1, b), _forward(fresh, 1, b)
    _same_outputs(got, want, "hk_policy_forward_mem")
    assert not np.array_equal(got[0], before[0]) and not np.array_equal(got[2], before[2])
    for h in (g, fresh):
        _stagger(h)
        h.step(1)
    ra, rb = _record(g, 20), _record(fresh, 20)               # 40 ticks of hk_step
    _same_rollouts(ra, rb, "40 ticks")
    assert ra["memory"][-1][:, 1].any() and (ra["raw"][:, :, 1] != ra["mu"][:, :, 1]).any()
    assert_bits_equal(g.agent_state(), fresh.agent_state(), "every agent record")
    for p in (0, 1):
        assert_bits_equal(g.policy_memory(p), fresh.policy_memory(p), "hk_policy_memory_get of policy %d" % p)


# ---- 4. what a load leaves alone
@pytest.mark.parametrize("E", ENVS)
def test_load_keeps_the_memory_the_ring_and_the_learner(E):
    shape = SHAPES[1]
    g, pols = _pair(E, shape)
    twin, _ = _pair(E, shape)                                  # the same race with no pool and no load
    pool = SnapshotPool(g, 1, 2)
    pool.put(0, _actor(g.obs_dim, shape, 33))
    mem0, learner0 = g.policy_memory(1), g.policy_memory(0)
    assert mem0.any(axis=-1).all()
    out0 = _forward(g, 0, pols[0])
    pool.load(0, 1)
    assert_bits_equal(g.policy_memory(1), mem0, "the opponent's memory after the load")
    assert_bits_equal(g.policy_memory(0), learner0, "the learner's memory after the load")
    _same_outputs(_forward(g, 0, pols[0]), out0, "the learner's forward after the load")
    ra, rb = _record(g, 2), _record(twin, 2)
    # the next decision: no FIRST, the memory it read, the ring it stacked (RING0 and OBS), and everything the learner did in that row
    assert not ra["first"][0].any()
    assert_bits_equal(ra["memory"][0][:, 1, :pols[1].memory_size], mem0[:, 0], "MEMORY of the decision after the load")
    assert_bits_equal(ra["ring0"], rb["ring0"], "RING0 after the load")
    for k in ("obs", "first", "memory"):
        assert_bits_equal(ra[k][0], rb[k][0], "the decision after the load: %s" % k)
    for k in ("mu", "raw", "logits", "steer", "branch", "logp_cont", "logp_disc"):
        assert_bits_equal(ra[k][0][:, 0], rb[k][0][:, 0], "the learner's row after the load: %s" % k)
    assert not np.array_equal(ra["mu"][0][:, 1], rb["mu"][0][:, 1])          # the opponent does play other weights


# ---- 5. save, load, save
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_save_load_save_gives_equal_slots(shape):
    g, pols = _pair(1, shape, ticks=0)
    pool = SnapshotPool(g, 0, 3)
    pool.save(0, 0)
    pool.save(2, 1)
    pool.load(0, 1)
    pool.save(1, 1)
    assert_bits_equal(pool.get_flat(1), pool.get_flat(0), "A -> slot -> C -> slot")
    assert not np.array_equal(pool.get_flat(2), pool.get_flat(0))
    _same_outputs(_forward(g, 1, pols[0]), _forward(g, 0, pols[0]), "C plays A's weights")


# ---- 6. a swap does not touch the learner
@pytest.mark.parametrize("E", ENVS)
def test_rho_is_one_after_a_swap(E):
    shape = SHAPES[2]
    g, pols = _pair(E, shape)
    tr = g.ppo_trainer(0, sequence_length=L)
    pool = SnapshotPool(g, 0, 2)
    pool.put(1, _actor(g.obs_dim, shape, 33))
    pool.load(1, 1)
    ro = _record(g, R)
    tr.advantages()
    nseq = ppo.sequence_count(R, L, E, 1)
    st = tr.minibatch(_ids(np.arange(nseq)), EPS, BETA)
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0, st
    rid = np.full((L, nseq), -1, np.int64)
    for q in range(nseq):
        for tau, r in enumerate(ppo.sequence_rows(q, R, L, E, 1)):
            rid[tau, q] = r
    live = rid >= 0
    assert_bits_equal(tr.read("mb_mu").reshape(L, nseq)[live], ro["mu"][:, :, 0].reshape(-1)[rid[live]], "MB_MU against the recorder")
    assert_bits_equal(tr.read("mb_logits").reshape(L, nseq, 3)[live], ro["logits"][:, :, 0, :3].reshape(-1, 3)[rid[live]], "MB_LOGITS against the recorder")


# ---- 7. hk_policy_memory_clear
@pytest.mark.parametrize("E", ENVS)
def test_memory_clear_is_memory_set_of_zeros(E):
    shape = SHAPES[1]
    a, pols = _pair(E, shape)
    b, _ = _pair(E, shape)
    assert a.policy_memory(1).any()
    a.policy_memory_clear(1)
    b.set_policy_memory(1, np.zeros_like(b.policy_memory(1)))
    ma = a.policy_memory(1)
    assert not ma.view(np.int32).any()                         # exactly +0.0
    assert_bits_equal(ma, b.policy_memory(1), "the memory after the clear")
    assert_bits_equal(a.policy_memory(0), b.policy_memory(0), "the other policy's memory")
    ra, rb = _record(a, 10), _record(b, 10)                    # 20 further ticks
    _same_rollouts(ra, rb, "after the clear")
    assert not ra["first"][0].any() and not ra["memory"][0][:, 1].any() and ra["memory"][0][:, 0].any() and ra["memory"][1][:, 1].any()
    assert_bits_equal(a.agent_state(), b.agent_state(), "agent records after the clear")
    assert_bits_equal(a.policy_memory(1), b.policy_memory(1), "the memory 20 ticks on")


def test_memory_clear_refusals():
    D = OBS
    rec, plain = _actor(D, SHAPES[0], 4), Policy.random(D * 4, 32, 2, 3, seed=8)
    g = _field(5, [rec, plain])
    mem0 = g.policy_memory(0)

    def refused(rc, word):
        msg = g.L.hk_last_error(g.h).decode()
        assert rc == _lib.HK_ERR_INVALID and "hk_policy_memory_clear" in msg and word in msg, (rc, msg)
        assert_bits_equal(g.policy_memory(0), mem0, "memory after a refused clear (%s)" % word)
    refused(g.L.hk_policy_memory_clear(g.h, 1), "no memory")
    refused(g.L.hk_policy_memory_clear(g.h, 2), "bad policy index")
    refused(g.L.hk_policy_memory_clear(g.h, -1), "bad policy index")
    g.rollout_begin(2)
    refused(g.L.hk_policy_memory_clear(g.h, 0), "rollout")
    g.rollout_close()
    assert g.L.hk_policy_memory_clear(None, 0) == _lib.HK_ERR_INVALID
    g.policy_memory_clear(0)
    assert not g.policy_memory(0).any()


# ---- 8. refusals
def _refusal_handle(other):
    """policy 0: the pool's recurrent actor (32, 32, 2) on kart 0; policy 1 on kart 1: `other`"""
    D = OBS
    own = _actor(D, SHAPES[0], 4)
    second = {"same": lambda: _actor(D, SHAPES[0], 14), "memory_size": lambda: _actor(D, (32, 64, 2), 14), "hidden": lambda: _actor(D, (64, 32, 2), 14),
              "layers": lambda: _actor(D, (32, 32, 3), 14), "normalize": lambda: _actor(D, SHAPES[0], 14, normalize=False),
              "stack": lambda: _actor(D, SHAPES[0], 14, stack=2), "plain": lambda: Policy.random(D * 4, 32, 2, 3, seed=14)}[other]()
    return _field(2, [own, second]), own, second


class _Watch:
    """what a refusal must leave as it was: slot 0 of the pool, the forward outputs of both policies and the memory of the recurrent ones"""

    def __init__(self, g, pool, pols):
        self.g, self.pool, self.pols = g, pool, pols
        self.was = self.now()

    def now(self):
        g = self.g
        out = [self.pool.get_flat(0)]
        for k, pol in enumerate(self.pols):
            if pol.memory_size:
                out += list(_forward(g, k, pol)) + [g.policy_memory(k)]
            else:
                out += list(g.policy_forward(k, _inputs(self.pols[0])[0][:, :pol.in_dim]))
        return out

    def refused(self, rc, code, word, tag):
        msg = self.g.L.hk_last_error(self.g.h).decode()
        assert rc == code and word in msg, (tag, rc, msg)
        for a, b in zip(self.now(), self.was):
            assert_bits_equal(a, b, "state after the refusal: " + tag)


def test_refusals_of_indices_slots_and_pointers():
    g, own, second = _refusal_handle("same")
    L_, h = g.L, g.h
    INV, UNS = _lib.HK_ERR_INVALID, _lib.HK_ERR_UNSUPPORTED
    # the entry point the old tests pin still refuses a policy with memory, and makes no pool
    rc = L_.hk_policy_pool_create(h, 0, 2)
    assert rc == UNS and "out of scope" in L_.hk_last_error(h).decode()
    for args, word in (((2, 2), "bad policy index"), ((-1, 2), "bad policy index"), ((0, 0), "slots"), ((0, 65), "slots")):
        rc = L_.hk_policy_pool_create_recurrent(h, *args)
        assert rc == INV and "hk_policy_pool_create_recurrent" in L_.hk_last_error(h).decode() and word in L_.hk_last_error(h).decode(), (args, rc)
    assert L_.hk_policy_pool_count(h, 0) == INV              # none of them made a pool
    pool = SnapshotPool(g, 0, 3)
    assert pool.pool == 0
    pool.save(0)
    w = _Watch(g, pool, [own, second])
    flat = np.zeros(pool.count, np.float32)
    fp = flat.ctypes.data_as(FP)
    calls = [("bad pool (save)", lambda: L_.hk_policy_pool_save(h, 7, 0, 1), "bad pool"), ("bad pool (load)", lambda: L_.hk_policy_pool_load(h, -1, 0, 1), "bad pool"),
             ("bad pool (count)", lambda: L_.hk_policy_pool_count(h, 1), "bad pool"), ("bad pool (put)", lambda: L_.hk_policy_pool_put(h, 1, 0, fp), "bad pool"),
             ("bad slot (save)", lambda: L_.hk_policy_pool_save(h, 0, 3, 1), "bad slot"), ("bad slot (load)", lambda: L_.hk_policy_pool_load(h, 0, -1, 1), "bad slot"),
             ("bad slot (put)", lambda: L_.hk_policy_pool_put(h, 0, 3, fp), "bad slot"), ("bad slot (get)", lambda: L_.hk_policy_pool_get(h, 0, 64, fp), "bad slot"),
             ("bad policy (save)", lambda: L_.hk_policy_pool_save(h, 0, 1, 2), "bad policy"), ("bad policy (load)", lambda: L_.hk_policy_pool_load(h, 0, 0, -1), "bad policy"),
             ("never written (load)", lambda: L_.hk_policy_pool_load(h, 0, 1, 1), "never been written"),
             ("never written (get)", lambda: L_.hk_policy_pool_get(h, 0, 1, fp), "never been written"),
             ("NULL (put)", lambda: L_.hk_policy_pool_put(h, 0, 1, None), "NULL"), ("NULL (get)", lambda: L_.hk_policy_pool_get(h, 0, 0, None), "NULL")]
    for tag, f, word in calls:
        w.refused(f(), INV, word, tag)
    # a load while a rollout is open; the rollout then goes on
    g.rollout_begin(2)
    rc = L_.hk_policy_pool_load(h, 0, 0, 1)
    assert rc == INV and "rollout" in L_.hk_last_error(h).decode()
    g.step(2 * P); g.rollout_close()
    assert g.rollout_rows() == 2
    # a load into a policy that has a trainer
    tr = g.ppo_trainer(1, sequence_length=L)
    rc = L_.hk_policy_pool_load(h, 0, 0, 1)
    assert rc == INV and "trainer" in L_.hk_last_error(h).decode()
    pool.save(1, 1)                                            # (saving a trained policy is what the driver does)
    # HK_MAX_POOLS is shared by both entry points
    for k in range(1, _lib.HK_MAX_POOLS):
        assert L_.hk_policy_pool_create_recurrent(h, 0, 1) == k
    rc = L_.hk_policy_pool_create_recurrent(h, 0, 1)
    assert rc == INV and "HK_MAX_POOLS" in L_.hk_last_error(h).decode()


@pytest.mark.parametrize("other,word", [("memory_size", "memory_size"), ("hidden", "shape"), ("layers", "shape"), ("normalize", "shape"), ("stack", "shape")])
def test_refusals_of_another_shape(other, word):
    g, own, second = _refusal_handle(other)
    pool = SnapshotPool(g, 0, 2)
    pool.save(0)
    w = _Watch(g, pool, [own, second])
    w.refused(g.L.hk_policy_pool_save(g.h, 0, 1, 1), _lib.HK_ERR_INVALID, word, "save of another " + other)
    w.refused(g.L.hk_policy_pool_load(g.h, 0, 0, 1), _lib.HK_ERR_INVALID, word, "load into another " + other)
    with pytest.raises(ValueError, match="parameters"):
        pool.put(1, second)
    w.refused(g.L.hk_policy_pool_get(g.h, 0, 1, np.zeros(pool.count, np.float32).ctypes.data_as(FP)), _lib.HK_ERR_INVALID, "never been written", "the refused put wrote nothing")


def test_refusals_between_the_two_kinds_of_pool():
    g, own, plain = _refusal_handle("plain")
    L_, h = g.L, g.h
    INV, UNS = _lib.HK_ERR_INVALID, _lib.HK_ERR_UNSUPPORTED
    rc = L_.hk_policy_pool_create_recurrent(h, 1, 2)
    assert rc == INV and "without memory" in L_.hk_last_error(h).decode() and "hk_policy_pool_create" in L_.hk_last_error(h).decode()
    rc = L_.hk_policy_pool_create(h, 0, 2)
    assert rc == UNS and "hk_policy_pool_create: policy: a recurrent actor (snapshot pools of recurrent actors are out of scope)" == L_.hk_last_error(h).decode()
    rpool, fpool = SnapshotPool(g, 0, 2), SnapshotPool(g, 1, 2)
    assert (rpool.pool, fpool.pool) == (0, 1) and rpool.count != fpool.count          # one table
    rpool.save(0); fpool.save(0)
    w = _Watch(g, rpool, [own, plain])
    f0 = fpool.get_flat(0)
    w.refused(L_.hk_policy_pool_save(h, 0, 1, 1), INV, "without memory", "recurrent pool, save of a policy without memory")
    w.refused(L_.hk_policy_pool_load(h, 0, 0, 1), INV, "without memory", "recurrent pool, load into a policy without memory")
    w.refused(L_.hk_policy_pool_save(h, 1, 1, 0), UNS, "hk_policy_pool_save: policy: a recurrent actor (snapshot pools of recurrent actors are out of scope)",
              "feed-forward pool, save of a recurrent policy")
    w.refused(L_.hk_policy_pool_load(h, 1, 0, 0), UNS, "hk_policy_pool_load: policy: a recurrent actor (snapshot pools of recurrent actors are out of scope)",
              "feed-forward pool, load into a recurrent policy")
    assert_bits_equal(fpool.get_flat(0), f0, "the feed-forward pool's slot")
    # the feed-forward pool beside a recurrent one works as before
    assert_bits_equal(f0, policy_to_flat(plain), "the feed-forward slot")
    fpool.load(0, 1)
    for a, b in zip(w.now(), w.was):
        assert_bits_equal(a, b, "after a feed-forward load of its own weights")


# ---- 9. the driver
ROWS, DRIVE_E, PRE_ROWS = 12, 5, 78
N = ROWS * DRIVE_E                                             # learner rows per rollout


def _drive_field(shape):
    """stack-1 actors (what the next decision needs of the observation ring is then the observation itself, so a race can be carried to a fresh
    handle: tests/test_policy_lstm_gpu.py test_race_resumes_on_a_second_handle), staggered, then one rollout of PRE_ROWS rows whose statistics
    are taken: it holds every env's first time-out, so the episodes that end in the driver's rollouts are whole and move the ratings"""
    D = OBS
    pols = [_actor(D, shape, s, stack=1) for s in (4, 14)]
    g = _field(DRIVE_E, pols, ticks=4)
    ro = _record(g, PRE_ROWS)
    assert (ro["done"] != 0).any(axis=0).all()
    g.episode_stats(0)
    return g, pols


def _trainer(g, shape, critic):
    if not critic:
        return g.ppo_trainer(0, sequence_length=L, seed=5)
    c = Policy.random(g.obs_dim, shape[0], 2, 1, stack=1, seed=21, normalize=False, memory_size=2 * shape[1])
    return g.ppo_trainer(0, critic=c, sequence_length=L, critic_memory_size=2 * shape[1], seed=5)


def _selfplay(g, tr, seed=3, **kw):
    return SelfPlay(g, tr, 1, window=2, save_steps=N, swap_steps=N, initial_elo=400.0, max_steps=10 * N, seed=seed, **kw)


def _iterate(sp, n):
    return [sp.iteration(ROWS, epochs=2, minibatch=4, lr=LR_, eps=EPS, beta=BETA) for _ in range(n)]


def _slots(sp):
    return sp.state_dict()["pool"]


def _outcome(g, tr, sp, critic):
    out = {k: tr.read(k) for k in VECTORS}
    if critic:
        out["critic_mem_out"] = tr.read("critic_mem_out")
    out.update({"pool " + k: v for k, v in _slots(sp).items()})
    out["ratings"] = np.asarray([sp.elo, sp.attached_elo] + sp.ratings, np.float64)
    for p in (0, 1):
        out["memory %d" % p] = g.policy_memory(p)
    return out


def _run(shape, critic, cut=None, tmp=None):
    """4 iterations -> (outcome, history, per-iteration stats); cut: the state after that many iterations goes to a file under tmp"""
    g, pols = _drive_field(shape)
    tr = _trainer(g, shape, critic)
    sp = _selfplay(g, tr)
    outs = _iterate(sp, cut or 4)
    if cut:
        ppo.checkpoint_write(str(tmp / "run.ckpt"), dict(selfplay=sp.state_dict(), trainer=tr.state_dict(), agents=g.agent_state().view(np.uint8),
                                                         envs=g.env_state().view(np.uint8), memory0=g.policy_memory(0), memory1=g.policy_memory(1)))
        outs += _iterate(sp, 4 - cut)
    return g, _outcome(g, tr, sp, critic), sp, outs


@pytest.mark.parametrize("critic", [False, True], ids=["recurrent", "recurrent_critic"])
def test_driver_twice_and_resumed_through_a_file(critic, tmp_path):
    shape = SHAPES[1]
    ga, a, spa, outs = _run(shape, critic, cut=2, tmp=tmp_path)
    _, b, spb, outs_b = _run(shape, critic)
    # the schedule: a save and a swap after every rollout; steps in learner rows; minibatches of 4 sequences out of 3 E
    assert [o["steps"] for o in outs] == [N, 2 * N, 3 * N, 4 * N] and [o["saved"] for o in outs] == [1, 0, 1, 0]
    assert all(o["swapped"] is not None for o in outs) and len(spa.history) == 4
    assert spa.elo != 400.0, [o["stats"] for o in outs]          # whole episodes ended inside the driver's rollouts
    # twice from the same seeds
    assert spa.history == spb.history and [o["stats"] for o in outs] == [o["stats"] for o in outs_b]
    assert sorted(a) == sorted(b)
    for k in a:
        assert_bits_equal(a[k], b[k], "two runs from the same seeds: %s" % k)
    # resumed on a fresh handle, which has stepped as many ticks (the sampling counter is the decision count) with the attached weights
    ck = ppo.checkpoint_read(str(tmp_path / "run.ckpt"))
    gc, pols = _drive_field(shape)
    gc.step(2 * ROWS * P)
    gc.set_agent_state(ck["agents"].view(ga.agent_state().dtype).reshape(ga.agent_state().shape))
    gc.set_env_state(ck["envs"].view(ga.env_state().dtype).reshape(ga.env_state().shape))
    trc = _trainer(gc, shape, critic)
    trc.load_state_dict(ck["trainer"])
    spc = _selfplay(gc, trc, seed=999)                         # (the generator comes from the state)
    spc.load_state_dict(ck["selfplay"])
    for p in (0, 1):
        gc.set_policy_memory(p, ck["memory%d" % p])
    assert spc.history == spa.history[:2] and spc.opponent == spa.history[1]
    outs_c = _iterate(spc, 2)
    c = _outcome(gc, trc, spc, critic)
    assert spc.history == spa.history
    assert [o["stats"]["len_sum"] for o in outs_c] == [o["stats"]["len_sum"] for o in outs[2:]]
    for k in a:
        assert_bits_equal(c[k], a[k], "resumed after 2 of 4 iterations: %s" % k)


def test_driver_reset_opponent_memory_on_the_device():
    shape = SHAPES[0]
    g, pols = _drive_field(shape)
    tr = _trainer(g, shape, False)
    sp = _selfplay(g, tr, reset_opponent_memory=True)
    assert g.policy_memory(1).any()
    o = sp.iteration(ROWS, epochs=1, minibatch=4, lr=LR_, eps=EPS, beta=BETA)
    assert o["swapped"] is not None
    assert not g.policy_memory(1).view(np.int32).any() and g.policy_memory(0).any()
    ro = _record(g, 1)
    assert not ro["first"].any() and not ro["memory"][0][:, 1].any() and ro["memory"][0][:, 0].any()


# ---- 10. side by side
def test_a_handle_with_a_recurrent_pool_computes_what_one_without_does():
    E, shape = 5, SHAPES[2]
    got = []
    for with_pool in (True, False):
        g, pols = _pair(E, shape)
        tr = g.ppo_trainer(0, sequence_length=L, seed=2)
        if with_pool:
            pool = SnapshotPool(g, 0, 3)
            pool.save(0)
            pool.save(1, 1)
            pool.load(1, 1)                                    # the opponent's own weights through a slot: what attach wrote, written again
        ro = _record(g, R)
        tr.advantages()
        tr.minibatch(_ids(np.arange(ppo.sequence_count(R, L, E, 1))), EPS, BETA, stats=False)
        got.append((ro, tr.read("grad"), tr.read("adv"), g.agent_state()))
    _same_rollouts(got[0][0], got[1][0], "with and without a recurrent pool")
    assert_bits_equal(got[0][1], got[1][1], "GRAD")
    assert_bits_equal(got[0][2], got[1][2], "ADV")
    assert_bits_equal(got[0][3], got[1][3], "agent records")
    assert got[0][1].any()
