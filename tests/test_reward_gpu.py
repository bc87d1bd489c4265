"""Reward shaping inside the fused tick kernel vs the CPU oracle: cumulative / per-decision / group accumulators of every
agent bit-identical tick by tick (float adds replayed in the same order), terminal group rewards in the episode results,
hk_get_rewards read-and-reset semantics."""
import functools
import numpy as np
import pytest
from hierarchicalkarting_amd import _lib
from parity import assert_bits_equal, assert_same_state, step_both, twin

pytestmark = pytest.mark.gpu


def _pair(E, A, **kw):
    import hierarchicalkarting_amd as hk
    return twin(hk.make_config(E, A, rewards=1, **kw))


def test_two_agents_tick_by_tick():
    g, o = _pair(6, 2, jitter_seed=4)
    step_both(g, o, [1] * 400)
    a = g.agent_state()
    assert (a["cum_reward"] > 20).all() and (a["group_reward"] > 20).all()


def test_four_agents_2v2_with_read_and_reset():
    g, o = _pair(32, 4, jitter_seed=9, training_agents=[1, 1, 1, 1])
    t = 0
    for n in (75, 3, 100, 57, 200, 65, 300):
        g.step(n); o.step(n); t += n
        assert_same_state(g, o, t)
        gr, gg = g.rewards(); orr, og = o.rewards()
        assert_bits_equal(gr, orr, (t, "reward")); assert_bits_equal(gg, og, (t, "group_reward"))
        a = g.agent_state()
        assert (a["step_reward"] == 0).all() and (a["group_reward"] == 0).all()      # Agent.SendInfo zeroes them


def test_episode_end_goal_timing_and_resets():
    """1-lap races with a tight time-out: finishes, time-outs, goal-timing rewards (disableOnEnd off so they reach the
    groups), table resets, next episode"""
    g, o = _pair(24, 4, jitter_seed=2, laps=1, max_episode_steps=1200, training_agents=[1, 0, 1, 1], disable_on_end=0)
    step_both(g, o, (400, 400, 200, 150, 100, 250, 500), check=functools.partial(assert_same_state, results=True))
    gr = g.episode_results()
    assert (gr["episode"] >= 0).all() and (gr["group_reward"] != 0).any() and (gr["reward"] != 0).all()


def test_rl_and_mcts_agents_with_rewards():
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd.policy import Policy
    g, o = twin(hk.make_config(8, 4, rewards=1, jitter_seed=6, low_mode=[_lib.HK_LOW_RL, _lib.HK_LOW_LQR, _lib.HK_LOW_LQR, _lib.HK_LOW_LQR],
                               high_mode=[_lib.HK_HIGH_FIXED, _lib.HK_HIGH_MCTS, _lib.HK_HIGH_FIXED, _lib.HK_HIGH_MCTS],
                               tree_search_depth=[5, 8, 5, 8], mcts_iterations=12))
    pol = Policy.random(g.obs_dim * 4, 64, 2, seed=3)
    g.attach_policy(pol, [0], 2); o.attach_policy(pol, [0], 2)
    step_both(g, o, (80, 45, 100, 75))


def test_hit_penalties_from_observations():
    """HKA:580-598: karts parked against a wall and behind each other; hk_get_observations raises the events"""
    g, o = _pair(3, 4, jitter_seed=0, jitter_pos=0.0, jitter_yaw=0.0)
    for e in (g, o):
        e.step(80); e.rewards()
        st = e.agent_state()
        for k in range(3):
            st["px"][k] = [19.6 - 0.05 * k, 15.0, 15.0, 15.9]; st["pz"][k] = [2.0, 30.0, 31.3, 30.6]
            st["yaw"][k] = [np.pi / 2, 0.0, 0.0, 3.3]
        st["vx"][:] = 0; st["vz"][:] = 0
        e.set_agent_state(st)
    assert_bits_equal(g.observations(), o.observations(), "observations")      # (first: observing raises the events)
    assert_same_state(g, o, 80)
    gr, gg = g.rewards(); orr, og = o.rewards()
    assert_bits_equal(gr, orr, "reward")
    assert (gr < -0.04).any()
    # and through the decision loop of an attached policy
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd.policy import Policy
    g, o = _pair(16, 2, jitter_seed=3, low_mode=[_lib.HK_LOW_RL, _lib.HK_LOW_RL])
    pol = Policy.random(g.obs_dim * 4, 64, 2, seed=8)
    g.attach_policy(pol, [0, 1], 2); o.attach_policy(pol, [0, 1], 2)
    step_both(g, o, (150, 151, 200, 97))
