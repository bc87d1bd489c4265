"""Self-play for recurrent actors on the host (hierarchicalkarting_amd/selfplay.py, include/hk.h "SELF-PLAY" RECURRENT POOLS), no GPU:
the flat slot vector of a Policy with memory against ppo.param_layout, SelfPlay's bookkeeping around a fake recurrent trainer on a fake pool and
a fake env (the schedule, reset_opponent_memory, the state round trip, the ValueErrors), and the two new prototypes' three declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.ppo import checkpoint_read, checkpoint_write, param_layout, split_params
from hierarchicalkarting_amd.selfplay import SelfPlay, SnapshotPool, flat_to_policy, policy_to_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(54, 32, 2, 32), (216, 96, 2, 96), (216, 128, 3, 128)]          # (in_dim, H, layers, m)


# ---- the flat vector
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_round_trip_of_a_policy_with_memory(shape, norm):
    K, H, Ln, m = shape
    pol = Policy.random(K, H, Ln, 3, stack=1, seed=5, normalize=norm, deterministic=True, memory_size=2 * m)
    flat = policy_to_flat(pol)
    trunk = K * H + H + (Ln - 1) * (H * H + H)
    assert flat.dtype == np.float32 and flat.size == trunk + 4 * m * H + 4 * m * m + 8 * m + m + 1 + 1 + 3 * m + 3 + (2 * K if norm else 0)
    back = flat_to_policy(flat, pol)
    assert back.memory_size == 2 * m and set(back.arrays()) == set(pol.arrays()) and "lstm_b_hh" in back.arrays()
    for k, v in pol.arrays().items():
        assert np.array_equal(back.arrays()[k].view(np.int32), v.view(np.int32)), k
    assert (back.stack, back.deterministic, back.seed) == (1, True, 5)


def test_flat_order_is_param_layout_with_memory():
    K, H, Ln, nb, m = 24, 32, 2, 3, 32
    layout = param_layout(K, H, Ln, nb, 2 * m)
    assert [n for n, _ in layout] == ["W0", "b0", "W1", "b1", "W_ih", "W_hh", "b_ih", "b_hh", "W_mu", "b_mu", "log_sigma", "W_branch", "b_branch"]
    const = {n: np.full(s, 1.0 + i, np.float32) for i, (n, s) in enumerate(layout)}          # a distinct constant per tensor
    pol = Policy([const["W0"], const["W1"]], [const["b0"], const["b1"]], const["W_mu"], const["b_mu"], const["log_sigma"], const["W_branch"],
                 const["b_branch"], np.full(K, 101.0, np.float32), np.full(K, 102.0, np.float32), 1, False, 0,
                 {k: const[k] for k in Policy.LSTM_KEYS})
    flat = policy_to_flat(pol)
    n = sum(int(np.prod(s)) for _, s in layout)
    assert flat.size == n + 2 * K
    for i, (name, v) in enumerate(split_params(flat[:n], layout).items()):
        assert v.shape == dict(layout)[name] and (v == 1.0 + i).all(), name
    assert (flat[n:n + K] == 101.0).all() and (flat[n + K:] == 102.0).all()
    # b_ih and b_hh lie apart, each with its own value: nothing is summed on the host
    p = split_params(flat[:n], layout)
    assert (p["b_ih"] == 7.0).all() and (p["b_hh"] == 8.0).all()


def test_a_feed_forward_policy_flattens_as_before():
    for norm in (True, False):
        pol = Policy.random(78, 32, 2, seed=5, stack=1, normalize=norm)
        parts = []
        for l in range(2):
            parts += [pol.W[l].reshape(-1), pol.b[l]]
        parts += [pol.W_mu, pol.b_mu, pol.log_sigma, pol.W_branch.reshape(-1), pol.b_branch] + ([pol.norm_mean, pol.norm_std] if norm else [])
        want = np.concatenate(parts).astype(np.float32)
        got = policy_to_flat(pol)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        back = flat_to_policy(got, pol)
        assert back.memory_size == 0 and back.lstm is None and set(back.arrays()) == set(pol.arrays())


# ---- SelfPlay around a fake recurrent trainer
class _FakeLib:
    def __init__(self, count):
        self.count, self.created = count, []

    def hk_policy_pool_create(self, h, policy, slots):
        self.created.append(("plain", policy, slots))
        return 0

    def hk_policy_pool_create_recurrent(self, h, policy, slots):
        self.created.append(("recurrent", policy, slots))
        return 0

    def hk_policy_pool_count(self, h, pool):
        return self.count

    def hk_policy_pool_put(self, h, pool, slot, flat):
        raise AssertionError("put reached the library")


class _FakeEnv:
    """what SelfPlay.iteration and SnapshotPool touch of a RacingEnv"""
    E, h, _decision_period = 5, None, 2

    def __init__(self, policies=None):
        self.calls, self.cleared = [], []
        self._policies = policies or []
        self._policy_slots = [[0], [1]]
        self.rows = 0

    def policy_memory_clear(self, index):
        self.cleared.append(index)
        self.calls.append(("clear", index))

    def rollout_begin(self, rows):
        self.rows = rows

    def step(self, n):
        self.calls.append(("step", n))

    def rollout_close(self):
        pass

    def rollout_rows(self):
        return self.rows

    def episode_stats(self, index):
        return dict(wins=3, draws=1, losses=2)


class _FakePool:
    count = 7

    def __init__(self, env):
        self.env, self.slot, self.version = env, {}, 0.0

    def save(self, slot, policy_index=None):
        self.env.calls.append(("save", slot))
        self.slot[slot] = np.full(self.count, self.version, np.float32)

    def load(self, slot, policy_index):
        self.env.calls.append(("load", slot, policy_index))

    def get_flat(self, slot):
        return self.slot[slot].copy()

    def put_flat(self, slot, flat):
        self.env.calls.append(("put", slot))
        self.slot[slot] = np.array(flat, np.float32)


class _FakeRecurrentTrainer:
    index, sequence_length, critic_memory_size = 0, 4, 0

    def __init__(self):
        self.updates = []

    def advantages(self):
        pass

    def update(self, epochs, minibatch, lr, eps, beta, **opts):
        self.updates.append((epochs, minibatch))
        return dict(L_pi=0.0)


def _sp(**kw):
    env = _FakeEnv()
    pool = _FakePool(env)
    return SelfPlay(env, _FakeRecurrentTrainer(), 1, pool=pool, **kw), pool, env


def test_schedule_around_a_recurrent_trainer_counts_rows_and_passes_sequences_through():
    sp, pool, env = _sp(window=2, save_steps=2 * 12 * 5, swap_steps=12 * 5, play_against_latest_model_ratio=0.0, seed=1)
    assert env.calls == [("save", 0)] and not sp.reset_opponent_memory
    outs = [sp.iteration(12, epochs=2, minibatch=6) for _ in range(4)]
    # steps are learner rows (rows x E x the learner's one slot); the minibatch reaches the trainer as given: it counts sequences there
    assert [o["steps"] for o in outs] == [60, 120, 180, 240] and sp.trainer.updates == [(2, 6)] * 4
    assert [o["saved"] for o in outs] == [None, 1, None, 0] and all(o["swapped"] is not None for o in outs)
    assert [c for c in env.calls if c[0] == "step"] == [("step", 24)] * 4
    assert env.cleared == [] and sum(1 for c in env.calls if c[0] == "load") == 4          # the default keeps the memory, as ML-Agents does


@pytest.mark.parametrize("ratio", [0.0, 0.5, 1.0])
def test_reset_opponent_memory_clears_once_after_every_load(ratio):
    sp, pool, env = _sp(window=3, save_steps=5, swap_steps=3, play_against_latest_model_ratio=ratio, seed=7, reset_opponent_memory=True)
    for _ in range(20):
        sp.advance(3)
    loads = [i for i, c in enumerate(env.calls) if c[0] == "load"]
    assert len(loads) == 20 and env.cleared == [1] * 20
    for i in loads:                                     # the clear follows its load, of the opponent's index, with nothing between
        assert env.calls[i][2] == 1 and env.calls[i + 1] == ("clear", 1)
    off, _, env_off = _sp(window=3, save_steps=5, swap_steps=3, play_against_latest_model_ratio=ratio, seed=7)
    for _ in range(20):
        off.advance(3)
    assert env_off.cleared == [] and off.history == sp.history


def test_state_round_trip_through_a_file(tmp_path):
    kw = dict(window=3, save_steps=5, swap_steps=3, play_against_latest_model_ratio=0.5, seed=7)
    a, pa, ea = _sp(reset_opponent_memory=True, **kw)
    for i in range(9):
        pa.version = float(i + 1)
        a.record_results(3 + i % 4, i % 3, 2 + (i * 5) % 7)
        a.advance(3)
    sd = a.state_dict()
    assert sd["reset_opponent_memory"] == 1 and all(v.shape == (7,) and v.dtype == np.float32 for v in sd["pool"].values())
    path = str(tmp_path / "sp.ckpt")
    checkpoint_write(path, sd)
    b, pb, eb = _sp(**dict(kw, seed=99))
    assert not b.reset_opponent_memory
    b.load_state_dict(checkpoint_read(path))
    assert b.reset_opponent_memory                     # the flag is part of the state
    # the restoring load does not clear: the caller restores the opponent's memory of the episode in progress
    assert eb.cleared == [] and eb.calls[-1][0] == "load" and b.opponent == a.opponent
    for i in range(9, 25):
        for sp, pool in ((a, pa), (b, pb)):
            pool.version = float(i + 1)
            sp.record_results(3 + i % 4, i % 3, 2 + (i * 5) % 7)
            sp.advance(3)
    assert b.history == a.history and b.ratings == a.ratings and b.elo == a.elo and (b.steps, b.cursor) == (a.steps, a.cursor)
    assert set(pb.slot) == set(pa.slot) and all(np.array_equal(pb.slot[s], pa.slot[s]) for s in pa.slot)
    assert len(eb.cleared) == 16
    # a state without the key (written before the flag existed) leaves the object's own setting
    c, _, _ = _sp(reset_opponent_memory=True, **kw)
    old = {k: v for k, v in sd.items() if k != "reset_opponent_memory"}
    c.load_state_dict(old)
    assert c.reset_opponent_memory


def test_value_errors():
    kw = dict(window=2, save_steps=5, swap_steps=3, seed=1)
    a, pa, _ = _sp(**kw)
    for _ in range(4):
        a.advance(3)
    sd = a.state_dict()
    # slots of another length than the pool's (a pool of another shape or memory size): refused before anything is put
    b, pb, eb = _sp(**kw)
    pb.count = 9
    was = {k: v.copy() for k, v in pb.slot.items()}
    with pytest.raises(ValueError, match="slot"):
        b.load_state_dict(sd)
    assert not [c for c in eb.calls if c[0] in ("put", "load")] and all(np.array_equal(pb.slot[k], was[k]) for k in was) and b.history == []
    # SnapshotPool: the recurrent create for a policy with memory, the plain one otherwise; put refuses another memory size
    rec, rec64, plain = (Policy.random(24, 32, 1, 3, stack=1, seed=1, memory_size=ms) for ms in (64, 128, 0))
    lib = _FakeLib(policy_to_flat(rec).size)
    env = _FakeEnv([rec, plain])
    env.L = lib
    env._ck = lambda rc: None
    pool = SnapshotPool(env, 0, 3)
    SnapshotPool(env, 1, 2)
    assert lib.created == [("recurrent", 0, 3), ("plain", 1, 2)]
    for other in (rec64, plain):
        with pytest.raises(ValueError, match="parameters"):
            pool.put(0, other)
    with pytest.raises(ValueError, match="float32"):
        pool.put_flat(0, np.zeros(pool.count + 1, np.float32))
    with pytest.raises(ValueError):
        SelfPlay(env, _FakeRecurrentTrainer(), 1, window=0, pool=_FakePool(env))


# ---- hk.h, _lib.py and HkNative.cs
def test_the_three_declarations_agree():
    hdr = open(os.path.join(ROOT, "include", "hk.h")).read()
    cs = open(os.path.join(ROOT, "host", "HkNative.cs")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+hk_policy_pool_create_recurrent\s*\(\s*hk_handle\s+h\s*,\s*int\s+policy\s*,\s*int\s+slots\s*\)\s*;", code)
    assert re.search(r"\bint\s+hk_policy_memory_clear\s*\(\s*hk_handle\s+h\s*,\s*int\s+policy\s*\)\s*;", code)
    assert _lib.SYMBOLS["hk_policy_pool_create_recurrent"] == _lib.SYMBOLS["hk_policy_pool_create"]
    res, args = _lib.SYMBOLS["hk_policy_pool_create_recurrent"]
    assert res is C.c_int and args[1:] == [C.c_int, C.c_int] and len(args) == 3
    res, args = _lib.SYMBOLS["hk_policy_memory_clear"]
    assert res is C.c_int and args[1:] == [C.c_int] and args[0] is _lib.SYMBOLS["hk_policy_memory_size"][1][0]
    assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern int hk_policy_pool_create_recurrent\(IntPtr h, int policy, int slots\);", cs)
    assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern int hk_policy_memory_clear\(IntPtr h, int policy\);", cs)
    # the contract's words: the recurrent pools are in, and out of scope is only what remains
    sp = hdr[hdr.index("---- SELF-PLAY"):hdr.index("#define HK_MAX_POOLS")]
    assert "RECURRENT POOLS" in sp and "hk_policy_pool_create_recurrent" in sp
    out = sp[sp.rindex("Out of scope"):]
    assert "team_change" in out and "per-env opponents" in out and "bf16 POCA" in out and "recurrent" not in out
