"""Training mode on device (random scatter resets inside the tick kernel and in hk_reset, planRandomly) vs the CPU oracle."""
import pytest
from hierarchicalkarting_amd import _lib
from parity import assert_same_state, step_both, twin

pytestmark = pytest.mark.gpu
TR = _lib.HK_MODE_TRAINING


def _pair(E, A, **kw):
    import hierarchicalkarting_amd as hk
    return twin(hk.make_config(E, A, env_mode=TR, **kw))


def test_scatter_and_random_plans_match():
    g, o = _pair(300, 4, training_agents=[1, 1, 1, 1], laps=2, jitter_seed=0)
    assert_same_state(g, o, 0)
    g.reset([5, 17, 100], 3); o.reset([5, 17, 100], 3)
    assert_same_state(g, o, "partial reset")


def test_training_episodes_with_timeouts_rewards_and_complex_track():
    g, o = _pair(24, 4, training_agents=[1, 1, 0, 0], laps=1, max_episode_steps=300, rewards=1, jitter_seed=0, track="complex")
    step_both(g, o, (100, 1, 199, 57, 243, 300))
    assert (g.env_state()["episodes_done"] >= 2).all()


def test_training_with_mcts_and_policy():
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd.policy import Policy
    b = hk.make_config(12, 2, env_mode=TR, training_agents=[1, 0], rewards=1, high_mode=[_lib.HK_HIGH_MCTS, _lib.HK_HIGH_MCTS],
                       low_mode=[_lib.HK_LOW_RL, _lib.HK_LOW_LQR], tree_search_depth=8, mcts_iterations=10, laps=1,
                       max_episode_steps=350, jitter_seed=0)
    step_both(*twin(b, attach=lambda D: (Policy.random(D * 4, 64, 2, seed=4), [0], 2)), (120, 130, 101, 99, 250))
