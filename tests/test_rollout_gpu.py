"""Rollout recorder (hk_rollout_begin / hk_step / hk_rollout_close, include/hk.h hk_rollout_field) against the CPU oracle stepped one
decision interval at a time: recording changes no result bit, every row holds what the actors did and what the interval paid."""
import numpy as np
import pytest
import oracle_lib as O
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.rollout import stacked_inputs, transition_rewards
from parity import assert_bits_equal, assert_child, assert_same_state
from rollout_restate import logp_cont, logp_disc

pytestmark = pytest.mark.gpu
RL, P = _lib.HK_LOW_RL, 2


def _make(E, A=4, policies=None, **kw):
    """-> (libhk handle, oracle, policies) with the same config and actors"""
    import hierarchicalkarting_amd as hk
    b = hk.make_config(E, A, **kw)
    g, o = hk.RacingEnv(b), O.OracleEnv(b)
    g.reset(); o.reset()
    pols = policies(g.obs_dim) if policies else _team_actors(g.obs_dim)
    for e in (g, o):
        for k, (pol, slots) in enumerate(pols):
            assert e.attach_policy(pol, slots, P) == k
    return g, o, pols


def _team_actors(D, stack2=4):
    """one stochastic and one deterministic team actor (the reference's Team 1 / Team 2 models are 312 -> 256 x 3)"""
    return [(Policy.random(D * 4, 256, 3, seed=1), [0, 1]),
            (Policy.random(D * stack2, 128, 2, stack=stack2, seed=2, deterministic=True), [2, 3])]


def _same_state(x, y, what, skip_acc=False):
    """skip_acc: not the reward accumulators, and not hk_episode_result.group_reward, which is the group accumulator as the episode's end found
    it — since the last read (Agent.SendInfo), and recording reads it at every decision, as a trainer does"""
    skip = np.full((x.E, x.A), skip_acc)
    assert_same_state(x, y, what, results=True, exclude=dict.fromkeys(("agent_state.step_reward", "agent_state.group_reward", "episode_results.group_reward"), skip))


def test_recording_changes_no_result_bit():
    kw = dict(low_mode=[RL] * 4, rewards=1, max_episode_steps=150, jitter_seed=4)
    g, o, pols = _make(24, **kw)
    import hierarchicalkarting_amd as hk
    h = hk.RacingEnv(hk.make_config(24, 4, **kw)); h.reset()
    for k, (pol, slots) in enumerate(pols):
        h.attach_policy(pol, slots, P)
    g.rollout_begin(120)
    t = 0
    for n in (1, 3, 7, 2, 50, 101, 33, 23):
        g.step(n); h.step(n); o.step(n); t += n
        _same_state(g, h, t, skip_acc=True)
        _same_state(g, o, t, skip_acc=True)
        assert_bits_equal(g.get_actions()[0], h.get_actions()[0], t)
    assert g.rollout_rows() == t // P
    g.rollout_close()
    assert (g.env_state()["episodes_done"] >= 1).all()


def _rows_vs_oracle(g, o, pols, R, chunks):
    """g records R rows over hk_step calls of `chunks` (cycled); the oracle steps interval by interval.  -> (ro, done rows)"""
    A = g.A
    m = np.zeros(A, bool)
    for _, slots in pols:
        m[slots] = True
    g.rollout_begin(R)
    left, k = R * P, 0
    while left > 0:
        n = min(chunks[k % len(chunks)], left); k += 1
        g.step(n); left -= n
    assert g.rollout_rows() == R
    g.rollout_close()
    ro = g.rollout()
    n_done = 0
    for t in range(R):
        cum0 = o.agent_state()["cum_reward"].copy()
        ep0 = o.env_state()["episodes_done"].copy()
        o.step(P)
        s, b = o.get_actions()
        assert_bits_equal(ro["steer"][t][:, m], s[:, m], t)
        assert np.array_equal(ro["branch"][t][:, m], b[:, m]), t
        r, gr = o.rewards()
        assert_bits_equal(ro["reward"][t][:, m], r[:, m], t)
        assert_bits_equal(ro["group_reward"][t][:, m], gr[:, m], t)
        es = o.env_state()
        d = np.where(es["episodes_done"] > ep0, np.where(es["status"] & 2, 2, 1), 0)
        assert np.array_equal(ro["done"][t], d), t
        assert (es["episodes_done"] - ep0 <= 1).all()
        ended = d != 0
        if ended.any():
            n_done += int(ended.sum())
            res = o.episode_results()
            assert_bits_equal(ro["term_group_reward"][t][ended][:, m], res["group_reward"][ended][:, m], t)
            if A >= 2:
                want = (res["reward"] - cum0)[ended][:, m]
                assert np.allclose(ro["term_reward"][t][ended][:, m], want, rtol=1e-4, atol=2e-4), t
        assert not ro["term_reward"][t][~ended].any() and not ro["term_group_reward"][t][~ended].any(), t
        assert not ro["steer"][t][:, ~m].any() and not ro["obs"][t][:, ~m].any(), t
    return ro, n_done


def test_rows_against_the_oracle():
    g, o, pols = _make(64, low_mode=[RL] * 4, rewards=1, max_episode_steps=100, jitter_seed=7)
    ro, n_done = _rows_vs_oracle(g, o, pols, 200, (1, 3, 7, 50, 2, 64, 11))
    assert n_done >= 200, n_done
    assert (ro["done"] == 2).any()
    # the terminal step pays what the interval paid before the reset: DONE ? TERM : REWARD is the transition reward
    tr = transition_rewards(ro)
    assert np.array_equal(tr[ro["done"] == 0], ro["reward"][ro["done"] == 0])
    # log-probabilities: a float64 restatement from the recorded heads and samples
    for k, (pol, slots) in enumerate(pols):
        raw, mu = ro["raw"][:, :, slots], ro["mu"][:, :, slots]
        lg, br = ro["logits"][:, :, slots, :pol.n_branch], ro["branch"][:, :, slots]
        assert np.allclose(ro["logp_cont"][:, :, slots], logp_cont(raw, mu, pol.log_sigma[0]), rtol=1e-6, atol=2e-6), k
        assert np.allclose(ro["logp_disc"][:, :, slots], logp_disc(lg, br), rtol=1e-6, atol=2e-6), k
        assert_bits_equal(ro["steer"][:, :, slots], np.clip(raw, np.float32(-3), np.float32(3)) / np.float32(3), k)
        if pol.deterministic:
            assert_bits_equal(raw, mu, k)
            assert np.array_equal(br, lg.argmax(axis=-1)), k
        else:
            assert (raw != mu).mean() > 0.9 and len(np.unique(br)) == pol.n_branch, k


def test_observations_and_stacks():
    g, o, pols = _make(16, policies=lambda D: _team_actors(D, stack2=2), low_mode=[RL] * 4, rewards=1, max_episode_steps=100, jitter_seed=3)
    g.step(5); o.step(5)                   # (a rollout may begin on any decision: RING0 then holds a live stack)
    g.step(1); o.step(1)
    o.rewards(); g.rewards()               # both accumulators start the rollout empty
    R = 60
    g.rollout_begin(R)
    for n in (2, 5, 1, 40, 72):
        g.step(n)
    g.rollout_close()
    o.step(R * P)
    o.rewards()
    ro = g.rollout()
    assert ro["ring0"].shape[2] == 3 and ro["ring0"].any() and ro["first"].any()
    for k, (pol, slots) in enumerate(pols):
        x = stacked_inputs(ro, slots, pol.stack)
        mu, lg = g.policy_forward(k, x.reshape(-1, pol.in_dim))
        assert_bits_equal(mu, ro["mu"][:, :, slots].reshape(-1), k)
        assert_bits_equal(lg, ro["logits"][:, :, slots, :pol.n_branch].reshape(-1, pol.n_branch), k)
    next_obs = ro["next_obs"].copy()
    assert next_obs.any()
    # the next rollout's first decision observes exactly what close() wrote, and close() raised no reward events
    g.rollout_begin(3)
    g.step(2); o.step(2)
    g.rollout_close()
    ro2 = g.rollout()
    assert_bits_equal(ro2["obs"][0], next_obs, "next_obs")
    r, gr = o.rewards()
    assert_bits_equal(ro2["reward"][0], r, "reward")
    assert_bits_equal(ro2["group_reward"][0], gr, "group_reward")
    assert_bits_equal(g.observations(), o.observations(), "observations")


def test_rules():
    import hierarchicalkarting_amd as hk
    kw = dict(low_mode=[RL] * 4, rewards=1, max_episode_steps=150, jitter_seed=5)
    g, o, pols = _make(8, **kw)
    twin = hk.RacingEnv(hk.make_config(8, 4, **kw)); twin.reset()
    for k, (pol, slots) in enumerate(pols):
        twin.attach_policy(pol, slots, P)
    bare = hk.RacingEnv(hk.make_config(2, 4, **kw)); bare.reset()

    def refused(fn, *a):
        with pytest.raises(_lib.HkError) as e:
            fn(*a)
        return e.value.code

    assert refused(bare.rollout_begin, 4) == _lib.HK_ERR_INVALID                # no actor attached
    assert bare.L.hk_rollout_ptr(bare.h, _lib.RO_FIELDS["obs"][0]) is None        # no rollout yet
    assert refused(g.rollout_begin, 0) == _lib.HK_ERR_INVALID
    g.step(1); twin.step(1)
    assert refused(g.rollout_begin, 4) == _lib.HK_ERR_INVALID                   # mid-interval
    g.step(1); twin.step(1)
    g.rollout_begin(3)
    assert refused(g.rollout_begin, 3) == _lib.HK_ERR_INVALID                   # already open
    assert g.L.hk_rollout_ptr(g.h, _lib.HK_RO_FIELDS) is None and g.L.hk_rollout_ptr(g.h, -1) is None
    assert refused(g.step, 7) == _lib.HK_ERR_INVALID                            # 4 decisions, 3 rows
    _same_state(g, twin, "refused step")
    st, es = g.agent_state(), g.env_state()
    for fn, a in ((g.reset, ()), (g.set_agent_state, (st,)), (g.set_env_state, (es,)), (g.rewards, ()), (g.rewards_device, ()),
                  (g.attach_policy, (pols[0][0], [0], P))):
        assert refused(fn, *a) == _lib.HK_ERR_INVALID, fn
    g.step(5); twin.step(5)
    assert g.rollout_rows() == 2
    assert refused(g.rollout_close) == _lib.HK_ERR_INVALID                      # mid-interval
    g.step(1); twin.step(1)
    g.rollout_close()
    # begin / close / begin: the stacks continue across rollouts
    for n in (2, 6):
        g.rollout_begin(4)
        g.step(n); twin.step(n)
        g.rollout_close()
        _same_state(g, twin, n, skip_acc=True)
        assert_bits_equal(g.get_actions()[0], twin.get_actions()[0], n)
    g.rewards()                                                                # closed: reading the accumulators is allowed again
    # destroy with an open rollout
    g.rollout_begin(2); g.step(2)
    g.close()
    # an env that ends two episodes inside one interval (a decision period of 250 ticks, time-outs every 100) cannot be expressed:
    # close fails loudly
    one = hk.RacingEnv(hk.make_config(2, 4, **{**kw, "max_episode_steps": 100})); one.reset()
    one.attach_policy(pols[0][0], [0, 1], 250)
    one.rollout_begin(1)
    one.step(250)
    assert refused(one.rollout_close) == _lib.HK_ERR_INVALID
    one.rollout_begin(1)                                                       # the failed close closed the rollout
    one.close(); twin.close(); bare.close()


def _duo_actors(D):
    return [(Policy.random(D * 4, 256, 3, seed=11), [0, 1]), (Policy.random(D * 4, 256, 3, seed=12), [2, 3])]


@pytest.mark.parametrize("case", ["training2", "fused2", "mcts_rl_duos"])
def test_instantiations_against_the_oracle(case):
    if case == "training2":        # the fused Training-mode kernel (2-agent Training fields)
        g, o, pols = _make(24, A=2, policies=lambda D: [(Policy.random(D * 4, 128, 3, seed=3), [0, 1])], low_mode=[RL, RL],
                           env_mode=_lib.HK_MODE_TRAINING, training_agents=[1, 1], rewards=1, laps=1, max_episode_steps=120, jitter_seed=1)
        R, chunks = 150, (3, 20, 1, 50)
    elif case == "fused2":         # 2 agents, rewards, an RL agent beside an LQ one: the fused reward kernel
        g, o, pols = _make(24, A=2, policies=lambda D: [(Policy.random(D * 4, 64, 2, seed=5), [0])], low_mode=[RL, _lib.HK_LOW_LQR],
                           rewards=1, max_episode_steps=110, jitter_seed=2)
        R, chunks = 150, (7, 2, 33)
    else:                          # the reference's MCTS-RL team agents, 2v2 (OvalDuos): planner hooks + rewards
        g, o, pols = _make(4, policies=_duo_actors, low_mode=[RL] * 4, high_mode=_lib.HK_HIGH_MCTS, tree_search_depth=4,
                           mcts_iterations=10, rewards=1, max_episode_steps=120, jitter_seed=6)
        R, chunks = 80, (5, 1, 40)
    ro, n_done = _rows_vs_oracle(g, o, pols, R, chunks)
    assert n_done > 0


def _child_rollout_views():
    import torch
    torch.cuda.init()                      # torch's HIP runtime first (see RacingEnv.torch_views)
    import numpy as np
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    g = hk.RacingEnv(hk.make_config(32, 4, low_mode=[_lib.HK_LOW_RL] * 4, rewards=1, max_episode_steps=100, jitter_seed=2))
    g.reset()
    g.attach_policy(Policy.random(g.obs_dim * 4, 128, 2, seed=1), [0, 1, 2, 3], 2)
    g.rollout_begin(60)
    g.step(120)
    g.rollout_close()
    v = g.rollout_views()
    ro = g.rollout()
    D = g.obs_dim
    want = {"obs": (60, 32, 4, D), "logits": (60, 32, 4, 3), "done": (60, 32), "ring0": (32, 4, 3, D), "next_obs": (32, 4, D), "reward": (60, 32, 4)}
    for k, t in v.items():
        assert t.is_cuda, k
        assert t.dtype == (torch.int32 if k in ("first", "branch", "done") else torch.float32), k
        assert tuple(t.shape) == ro[k].shape, k
        if k in want:
            assert tuple(t.shape) == want[k], k
        assert_bits_equal(t.cpu().numpy(), ro[k], k)
    assert (ro["done"] != 0).any() and ro["obs"].any()


def test_torch_views():
    assert_child(_child_rollout_views, timeout=600)
