"""The games meter and the lazily joined parts of a split batch across a race start stepped tick by tick (round 6).

Default: every call of a plain handle of >= 8 192 envs runs as two halves on two streams whose parts stay open from call to call (hk_api.hip split_join) —
a host that steps tick by tick keeps both halves' meter words current, reaches the sparse (in-wave) schedule once the field has spread, and sees the same
state, bit for bit, as a host that steps in long calls, whatever schedule each was given; a getter in between joins the parts."""
import pytest
from parity import assert_child, assert_same_state

pytestmark = pytest.mark.gpu


def _child_tick_by_tick():
    import numpy as np
    import hierarchicalkarting_amd as hk
    b = hk.make_config(8192, 4, jitter_seed=5, laps=3, max_episode_steps=4000)
    g = hk.RacingEnv(b); ref = hk.RacingEnv(b)
    g.reset(); ref.reset()
    g.step(1)
    first = g.schedule_info()
    assert first["streams"] == 2, first                 # the close field of a race start: two halves
    for k in range(899):
        g.step(1)
        if k == 300:                                    # a look in the middle of the run joins the open parts and must show the long-call host's state
            ref.step(302)
            assert_same_state(g, ref, k)
    last = g.schedule_info()
    assert last["call_ticks"] == 1 and last["streams"] == 2, last
    assert last["games_meter"] == "sparse", last
    assert "in-wave" in last["multi_player_games"], last
    ref.step(598)
    assert_same_state(g, ref, 900)
    # and on: a long call after the tick-by-tick stretch
    g.step(64); ref.step(64)
    again = g.schedule_info()
    assert again["streams"] == 2 and again["games_meter"] in ("sparse", "medium"), again
    assert_same_state(g, ref, 964)
    # short calls of mixed sizes with results read through the device-pointer path in between (settle_for_pointer joins too)
    for n in (1, 3, 1, 7, 2, 1, 1, 20, 1):
        g.step(n); ref.step(n)
    assert g.device_results_ptr() != 0
    assert np.array_equal(g.episode_results().view(np.uint8), ref.episode_results().view(np.uint8))
    assert_same_state(g, ref, 1001)
    g.close(); ref.close()


@pytest.mark.parametrize("mode", ["default"])
def test_tick_by_tick_host_after_a_split_start(mode):
    assert_child(_child_tick_by_tick, timeout=900)
