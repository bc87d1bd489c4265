"""Recurrent actors (policy_lstm_kernel and its memory kernels) on the fields tests/test_policy_lstm_gpu.py does not reach, bit for
bit against the same host twin: layer 0 in two and three chunks (the `kb > 0` leg of the kernel's own copy of the trunk), 4- and 8-kart fields
whose lane groups a regroup has permuted (slot_of is not the identity from A = 3 on), slot lists that are descending and scattered, two memory
widths on one handle, episodes that end on the first tick of a decision interval, and shards with env_id_base != 0.

Ticks.  An env that began its episode at tick k (hk_reset after k ticks of the handle) counts episode_steps 1 .. 100 in the ticks k .. k + 99,
so with max_episode_steps = 100 its time-outs fall in the ticks 100 n + 99 + k.  `_stagger` starts the envs with env % 4 == k at tick k: four
classes with four regroup keys, (episode_steps + left) & 3, whose time-outs lie one tick apart — 299, 300, 301, 302 — where the decision
intervals are [298, 300), [300, 302), [302, 304): the classes 1 and 3 end their episode on an interval's FIRST tick and run the second tick of
it in the next episode.  The rollouts below end with the interval [302, 304): class 0 is done in the third row from the end, 1 and 2 in the
one before the last, 3 in the last.  The periodic regroup runs every 48 rounds and a round is at most one decision interval here."""
import numpy as np
import pytest
import policy_lstm_twin as TW
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.rollout import stacked_inputs
from parity import assert_bits_equal
from rollout_restate import logp_cont, logp_disc

pytestmark = pytest.mark.gpu
P = 2
PM_KC_MAX = 256


def _chunks(in_dim, H):
    """layer 0's chunks as policy_upload cuts them: equal chunks of at most PM_KC_MAX inputs, whole groups of 8, never below the hidden size"""
    nch = -(-in_dim // PM_KC_MAX)
    kc = (-(-in_dim // nch) + 7) & ~7
    kc = max(min(kc, PM_KC_MAX), H)
    return [min(kc, in_dim - kb) for kb in range(0, in_dim, kc)]


# (karts, stack, H, layers, m, normalise, layer-0 chunks).  At H = 256 the chunk is raised to the hidden size (policy_upload: "later layers run as
# one chunk of `hidden`"), so 312 inputs go as 256 + 56 and 624 as 256 + 256 + 112; three chunks of 208 need H <= 208, hence the H = 192 row.
FORWARD = [
    (4, 4, 128, 3, 128, True, [160, 152]),          # the timed shape (DESIGN §16 "Measured")
    (4, 4, 128, 3, 128, False, [160, 152]),         # ... without the normaliser
    (4, 4, 256, 2, 64, True, [256, 56]),            # a last chunk of 7 groups of 8
    (4, 7, 96, 2, 96, True, [184, 184, 178]),       # remainder 2 modulo 8 in the last chunk; an odd block count, two unit-block waves idle
    (4, 8, 256, 2, 128, True, [256, 256, 112]),     # the largest LDS footprint, 101 888 bytes
    (4, 8, 192, 2, 64, True, [208, 208, 208]),      # three equal chunks
    (4, 1, 160, 1, 32, True, [78]),                 # one chunk: 9 groups of 8 plus 6; kc raised to H
    (8, None, 128, 2, 128, True, [256, 248]),       # an 8-kart observation: stack = min(4, HK_POLICY_MAX_IN // obs_dim)
]


@pytest.mark.parametrize("A,stack,H,layers,m,norm,chunks", FORWARD)
def test_forward_chunked_layer0_against_the_twin(A, stack, H, layers, m, norm, chunks):
    g = TW.rl_env(2, A)
    D = g.obs_dim
    assert D == {4: 78, 8: 126}[A]
    if stack is None:
        stack = min(4, _lib.HK_POLICY_MAX_IN // D)
        assert stack == 4
    pol = Policy.random(D * stack, H, layers, 3, stack=stack, seed=H + m + stack, memory_size=2 * m, normalize=norm)
    assert pol.in_dim == sum(chunks) and _chunks(pol.in_dim, H) == chunks, (pol.in_dim, _chunks(pol.in_dim, H))
    assert (pol.norm_mean is not None) == norm
    assert g.attach_policy(pol, [A - 1], P) == 0 and g.L.hk_policy_memory_size(g.h, 0) == 2 * m
    r = np.random.default_rng(7 * H + m + stack)
    names = ("mu", "logits", "mem_out")
    for rows in (1, 65, 130):                       # one row, a last tile of one row, more than two tiles
        obs = (r.standard_normal((rows, pol.in_dim)) * 4).astype(np.float32)
        mem = r.uniform(-1.0, 1.0, (rows, 2 * m)).astype(np.float32)
        got = g.policy_forward(0, obs, mem)
        want = TW.step(pol, obs, mem)
        for x, y, n in zip(got, want, names):
            assert_bits_equal(x, y, (A, stack, H, m, rows, n))
        assert np.abs(got[2]).max() > 1e-3 and np.isfinite(got[0]).all() and np.abs(got[0]).max() > 1e-3
        if rows in (1, 65):
            null = g.policy_forward(0, obs, None)
            for x, y, z, n in zip(null, g.policy_forward(0, obs, np.zeros_like(mem)), TW.step(pol, obs, None), names):
                assert_bits_equal(x, y, (A, stack, H, m, rows, n, "NULL == zeros"))
                assert_bits_equal(x, z, (A, stack, H, m, rows, n, "NULL vs twin"))
            obs2 = (r.standard_normal((rows, pol.in_dim)) * 4).astype(np.float32)        # two chained calls == two twin steps
            for x, y, n in zip(g.policy_forward(0, obs2, got[2]), TW.step(pol, obs2, want[2]), names):
                assert_bits_equal(x, y, (A, stack, H, m, rows, n, "chained"))
    assert not g.policy_memory(0).any()             # the tap leaves the policy's own memory alone


# ---- closed loops on regrouped fields
def _stagger(g, upto, base=0):
    """the envs whose global id % 4 == k restart their episode after k ticks, k = 1, 2, 3; then on to tick `upto` of the handle"""
    for k in (1, 2, 3):
        g.step(1)
        g.reset(np.array([e for e in range(g.E) if (base + e) % 4 == k], np.int32))
    g.step(upto - 3)


def _field(E, A, rec_slots, plain_slots, base=0, det=False, stack=4):
    """every kart RL; a recurrent actor (obs_dim * stack -> 128 x 3 -> m = 128) and a plain one beside it"""
    g = TW.rl_env(E, A, rewards=1, max_episode_steps=100, jitter_seed=9, env_id_base=base)
    D = g.obs_dim
    rec = Policy.random(D * stack, 128, 3, 3, stack=stack, seed=4, memory_size=256, deterministic=det)
    plain = Policy.random(D * stack, 128, 3, 3, stack=stack, seed=5, deterministic=det)
    assert g.attach_policy(rec, rec_slots, P) == 0 and g.attach_policy(plain, plain_slots, P) == 1
    return g, rec, plain


def _done_rows(ro):
    """-> per class env % 4: the rows in which its envs are done (every env of a class alike)"""
    done = ro["done"] != 0
    out = []
    for k in range(4):
        d = done[:, k::4]
        assert (d == d[:, :1]).all(), k
        out.append(np.flatnonzero(d[:, 0]).tolist())
    return out


def _check_recorded(g, ro, live, rec, rs, plain, ps, tag):
    """what a closed rollout of _field must satisfy: the recurrent actor replays through the twin from MEMORY / FIRST / OBS alone, the live
    memory and NEXT_MEMORY follow, the plain actor's rows equal its forward tap and hold no memory"""
    R, A = ro["obs"].shape[0], g.A
    assert ro["memory"].shape == (R, g.E, A, 256) and ro["next_memory"].shape == (g.E, A, 256)
    done = ro["done"] != 0
    assert sorted(rs + ps) == list(range(A))
    assert np.array_equal(ro["first"][1:] == 1, np.broadcast_to(done[:-1, :, None], (R - 1, g.E, A))), tag      # every slot is driven
    assert done[:R - 1].any() and done[R - 1].any() and (~done[R - 1]).any()       # NEXT_MEMORY: both sides of its rule
    # the time-outs of the four classes, one tick apart: 0 on an interval's second tick, 1 on the first tick of the next interval, 2 on its second, 3 on
    # the last interval's first
    assert _done_rows(ro) == [[R - 3], [R - 2], [R - 2], [R - 1]], _done_rows(ro)
    last = TW.replay(ro, rec, rs, tag)
    assert_bits_equal(live, last, (tag, "hk_policy_memory_get after the last row"))
    want = np.where(done[R - 1][:, None, None], np.float32(0), last)
    assert_bits_equal(ro["next_memory"][:, rs], want, (tag, "NEXT_MEMORY"))
    assert not ro["memory"][:, :, ps].any() and not ro["next_memory"][:, ps].any()
    x = stacked_inputs(ro, ps, plain.stack)
    mu, lg = g.policy_forward(1, x.reshape(-1, plain.in_dim))
    assert_bits_equal(mu, ro["mu"][:, :, ps].reshape(-1), (tag, "plain mu"))
    assert_bits_equal(lg, ro["logits"][:, :, ps, :3].reshape(-1, 3), (tag, "plain logits"))
    raw, mu, lg, br = ro["raw"], ro["mu"], ro["logits"], ro["branch"]
    assert np.allclose(ro["logp_cont"][:, :, rs], logp_cont(raw, mu, rec.log_sigma[0])[:, :, rs], rtol=1e-6, atol=2e-6)
    assert np.allclose(ro["logp_disc"], logp_disc(lg, br), rtol=1e-6, atol=2e-6)
    assert_bits_equal(ro["steer"], np.clip(raw, np.float32(-3), np.float32(3)) / np.float32(3), (tag, "steer"))
    assert (raw != mu).mean() > 0.9


def _record(g, upto, R, calls):
    _stagger(g, upto)
    g.rollout_begin(R)
    for n in calls:
        g.step(n)
    assert g.rollout_rows() == R
    live = g.policy_memory(0)
    g.rollout_close()
    return g.rollout(), live


def test_closed_loop_on_a_regrouped_2v2_field():
    g, rec, plain = _field(70, 4, [3, 0], [1, 2])             # 140 rows a decision; the recurrent actor's slots descending and not adjacent
    ro, live = _record(g, 280, 12, (1, 3, 2, 7, 11))
    _check_recorded(g, ro, live, rec, [3, 0], plain, [1, 2], "2v2")


def test_call_patterns_on_a_regrouped_2v2_field():
    """hk_step(2) x 12, hk_step(24) and a mixed split on equal seeds: every recorder field, the final memory and agent_state, bit for bit"""
    outs = []
    for calls in ((2,) * 12, (24,), (1, 3, 2, 7, 11)):
        g, _, _ = _field(70, 4, [3, 0], [1, 2])
        ro, live = _record(g, 280, 12, calls)
        outs.append((ro, live, g.policy_memory(0), g.agent_state()))
    assert (outs[0][0]["done"] != 0).any()
    for ro, live, mem, st in outs[1:]:
        assert sorted(ro) == sorted(outs[0][0])
        for name in ro:
            assert_bits_equal(ro[name], outs[0][0][name], name)
        assert_bits_equal(live, outs[0][1], "memory before the close")
        assert_bits_equal(mem, outs[0][2], "memory")
        assert_bits_equal(st, outs[0][3], "agent_state")


def test_memory_set_through_a_permuted_slot_of():
    """at tick 300 class 0 has just ended its third episode and the others are in theirs: the episode words differ from class to class, and the
    lane groups are ordered by class.  hk_policy_memory_set makes the recurrent actor's epoch words current, so the next decision keeps what was
    set — also where the plain actor beside it sees FIRST"""
    g, rec, plain = _field(70, 4, [3, 0], [1, 2], det=True, stack=1)
    _stagger(g, 300)
    words = g.env_state()["episodes_done"]
    assert len(np.unique(words)) == 2 and (words[0::4] == words[0]).all() and (words[1::4] != words[0]).all()
    mem = np.random.default_rng(2).uniform(-1, 1, (70, 2, 256)).astype(np.float32)
    g.set_policy_memory(0, mem)
    assert_bits_equal(g.policy_memory(0), mem, "set / get")
    g.rollout_begin(1)
    g.step(2)
    g.rollout_close()
    ro = g.rollout()
    assert not ro["first"][:, :, [3, 0]].any()
    cls0 = np.arange(70) % 4 == 0
    assert (ro["first"][0][cls0][:, [1, 2]] == 1).all() and not ro["first"][0][~cls0].any()    # (the plain actor: class 0 has started an episode)
    assert_bits_equal(ro["memory"][0][:, [3, 0]], mem, "the decision after hk_policy_memory_set reads what was set")
    TW.replay(ro, rec, [3, 0], "after hk_policy_memory_set")


def test_race_resumes_on_a_fresh_handle_at_4_karts():
    """agent and env state and the memory carried from a handle whose lane groups are permuted to a fresh one, where slot_of is the identity: the
    race continues bit for bit across every env's next time-out (deterministic actors on a stack of one observation, as the 2-kart test's: the
    observation stack and the sampling counter are not part of what the getters carry).

    The carry is taken at tick 300, where class 0 has ended an episode since its last decision.  hk_policy_memory_get returns the memory as the
    last decision left it, and what hk_policy_memory_set writes belongs to the episode an env is in NOW (hk.h): the memory of an env whose
    episode ended since its last decision is the caller's to clear, as the decision on the first handle will — carried as it is, the race of
    exactly those envs (and of no other) leaves the first handle's at the next decision, which the test shows on a third handle."""
    a, _, _ = _field(70, 4, [3, 0], [1, 2], det=True, stack=1)
    b, _, _ = _field(70, 4, [3, 0], [1, 2], det=True, stack=1)
    c, _, _ = _field(70, 4, [3, 0], [1, 2], det=True, stack=1)
    _stagger(a, 298)
    before = a.env_state()["episodes_done"].copy()
    a.step(2)
    ended = a.env_state()["episodes_done"] != before
    assert np.array_equal(ended, np.arange(70) % 4 == 0)
    mem = a.policy_memory(0)
    assert mem.any(axis=-1).all()
    for h, m in ((b, np.where(ended[:, None, None], np.float32(0), mem)), (c, mem)):
        h.set_agent_state(a.agent_state()); h.set_env_state(a.env_state())
        h.set_policy_memory(0, m)
    c.step(2)
    done0 = a.env_state()["episodes_done"].copy()
    for n in (2, 5, 9, 101):
        a.step(n); b.step(n)
        assert_bits_equal(a.agent_state(), b.agent_state(), ("agent_state", n))
        assert_bits_equal(a.env_state()["episodes_done"], b.env_state()["episodes_done"], ("episodes_done", n))
        assert_bits_equal(a.get_actions()[0], b.get_actions()[0], ("steer", n))
        assert_bits_equal(a.policy_memory(0), b.policy_memory(0), ("memory", n))
        if n == 2:          # the memory carried uncleared: the envs that ended an episode, on the recurrent actor's slots, and nothing else
            diff = a.get_actions()[0] != c.get_actions()[0]
            assert np.array_equal(diff[:, [3, 0]], np.broadcast_to(ended[:, None], (70, 2))) and not diff[:, [1, 2]].any()
    assert (a.env_state()["episodes_done"] > done0).all()
    assert len(np.unique(a.get_actions()[0])) > 8 and a.policy_memory(0).any(axis=-1).all()


def test_two_memory_widths_on_one_handle():
    g = TW.rl_env(70, 4, rewards=1, max_episode_steps=100, jitter_seed=9)
    D = g.obs_dim
    pols = [Policy.random(D, 64, 2, 3, stack=1, seed=6, memory_size=64), Policy.random(D * 4, 128, 3, 3, stack=4, seed=7, memory_size=256)]
    slots = [[2, 0], [1, 3]]
    for k in (0, 1):
        assert g.attach_policy(pols[k], slots[k], P) == k
    assert g.L.hk_policy_memory_size(g.h, 0) == 64 and g.L.hk_policy_memory_size(g.h, 1) == 256
    R = 8
    _stagger(g, 288)
    g.rollout_begin(R)
    g.step(2 * R)
    live = [g.policy_memory(k) for k in (0, 1)]
    g.rollout_close()
    ro = g.rollout()
    assert ro["memory"].shape[-1] == 256 and ro["next_memory"].shape[-1] == 256
    done = ro["done"] != 0
    assert _done_rows(ro) == [[R - 3], [R - 2], [R - 2], [R - 1]], _done_rows(ro)
    for k in (0, 1):
        last = TW.replay(ro, pols[k], slots[k], ("widths", k))
        assert_bits_equal(live[k], last, ("widths", k, "hk_policy_memory_get after the last row"))
        mm = pols[k].memory_size
        want = np.where(done[R - 1][:, None, None], np.float32(0), last)
        assert_bits_equal(ro["next_memory"][:, slots[k], :mm], want, ("widths", k, "NEXT_MEMORY"))
        assert ro["memory"][:, :, slots[k], :mm].any(axis=-1).mean() > 0.5
    assert not ro["memory"][:, :, slots[0], 64:].any() and not ro["next_memory"][:, slots[0], 64:].any()


def test_closed_loop_on_eight_karts():
    g, rec, plain = _field(17, 8, [0, 1, 2, 3], [4, 5, 6, 7])      # 68 rows a decision: a second tile of 4
    assert rec.in_dim == 504
    ro, live = _record(g, 284, 10, (20,))
    _check_recorded(g, ro, live, rec, [0, 1, 2, 3], plain, [4, 5, 6, 7], "eight karts")


def test_two_shards_equal_one_handle_with_a_recurrent_actor():
    """E = 12 on one handle against 6 + 6 on two, the second with env_id_base = 6: the stochastic recurrent actor's sampling key and the start
    jitter follow the global env id, and so does the stagger here; a second rollout crosses the classes' time-outs"""
    def run(E, base):
        g, _, _ = _field(E, 4, [3, 0], [1, 2], base=base)
        _stagger(g, 130, base)
        out = []
        for gap in (0, 34):
            g.step(gap)
            g.rollout_begin(10)
            g.step(20)
            g.rollout_close()
            out.append(g.rollout())
        return out, g.policy_memory(0), g.agent_state()

    whole, lo, hi = run(12, 0), run(6, 0), run(6, 6)
    for i in (0, 1):
        for name, w in whole[0][i].items():
            ax = 0 if name in ("ring0", "next_obs", "next_memory") else 1
            assert_bits_equal(w, np.concatenate([lo[0][i][name], hi[0][i][name]], axis=ax), ("rollout", i, name))
    assert (whole[0][1]["done"] != 0).any(axis=0).all() and not (whole[0][0]["done"] != 0).any()
    assert (whole[0][0]["raw"] != whole[0][0]["mu"]).mean() > 0.9
    assert_bits_equal(whole[1], np.concatenate([lo[1], hi[1]], axis=0), "policy_memory")
    assert_bits_equal(whole[2], np.concatenate([lo[2], hi[2]], axis=0), "agent_state")
