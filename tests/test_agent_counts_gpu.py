"""Agent counts other than the 2 / 4 of the reference scenes: 1 kart alone (time-trial style) and 3 karts (2 v 1) must
still match the oracle field for field — with the planner, the actor and rewards switched on."""
import functools
import pytest
from hierarchicalkarting_amd import _lib
from parity import assert_same_state, step_both, twin

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("A,wiring", [(1, ([0], [[]], [[]])), (3, ([0, 0, 1], [[1], [0], []], [[2], [2], [0, 1]]))])
def test_odd_agent_counts(A, wiring):
    import hierarchicalkarting_amd as hk
    high = [_lib.HK_HIGH_MCTS] + [_lib.HK_HIGH_FIXED] * (A - 1)
    b = hk.make_config(10, A, wiring=wiring, jitter_seed=5, rewards=1, high_mode=high, tree_search_depth=[8] + [5] * (A - 1),
                       mcts_iterations=12, training_agents=[1] * A)
    step_both(*twin(b), (80, 41, 100, 79, 300), check=functools.partial(assert_same_state, obs=True))
