"""Settling the handle (hk_api.hip settle): an hk_step may leave work open — the laggards of a lazily completed call, the unverified guard of an
optimistic plan, the parts of a split call on their own streams, a search launch on the planner's side stream — and whichever entry point
touches the handle next has to bring that in before it reads or writes.  For each such pending state a fresh handle is put into it, ONE
entry point is the first thing that touches it, and what that returns is the oracle's, bit for bit."""
import numpy as np
import pytest
import hierarchicalkarting_amd as hk
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.env import AGENT_DT, RESULT_DT
from hierarchicalkarting_amd.policy import Policy
from parity import ENV_FIELDS, assert_bits_equal, twin

pytestmark = pytest.mark.gpu

MCTS, FIXED, RL, LQR = _lib.HK_HIGH_MCTS, _lib.HK_HIGH_FIXED, _lib.HK_LOW_RL, _lib.HK_LOW_LQR


def _planner_actor():
    """the planner + actor handle of smoke()"""
    cfg = hk.make_config(8, 4, jitter_seed=7, rewards=1, mcts_iterations=16, tree_search_depth=[8, 8, 5, 5],
                         high_mode=[MCTS, MCTS, FIXED, FIXED], low_mode=[RL, LQR, LQR, LQR])
    return cfg, lambda obs_dim: (Policy.random(obs_dim * 4, 128, 3, seed=1), [0], 2)


# state -> (config and actor, the HK_* switches of the handle, the calls that leave the state, what hk_schedule_info must say of the last one)
STATES = {
    # past the start hold (75 ticks) the field stands close and every ego holds a multi-player game: the 80-tick call from tick 100 is
    # completed lazily and has laggards
    "lazy": (lambda: (hk.make_config(64, 4, jitter_seed=0x5EED0000), None), {}, [100, 80], {"rounds": "lazy"}),
    # the belief is off by 2 (tests/test_optimistic_plan_gpu.py): the one-tick call from step 103 is planned without its solve tick 104,
    # so the guard of the short calls reports envs that kept ticks
    "optimistic": (lambda: (hk.make_config(64, 4, jitter_seed=0x5EED0000, laps=1), None), {"HK_OPTIMISTIC_SKEW": "2"}, [60, 20, 20, 3, 1, 2, 7],
                   {"rounds": "fixed", "optimistic_plan": True}),
    # plan_call splits from 8 192 envs on; short folded calls leave their parts open
    "split": (lambda: (hk.make_config(8192 + 64, 4, jitter_seed=0x5EED0000), None), {}, [1, 1, 1], {"streams": 2, "armed_in_first_launch": True}),
    # decision chunks across the replan step 100: its searches run on the side stream until step 145
    "search": (_planner_actor, {}, [104], {"planner": True, "actors": 1}),
}


def _read(g, ptr, dtype, shape):
    """a device pointer's buffer after hk_synchronize"""
    assert ptr, g.L.hk_last_error(g.h)
    g.synchronize()
    a = np.zeros(shape, dtype)
    _lib.copy_device_to_host(a.ctypes.data, ptr, a.nbytes)
    return a


def _observed(g):
    p = g.L.hk_device_obs_ptr(g.h)
    g.observe()
    return _read(g, p, np.float32, (g.E, g.A, g.obs_dim))


def _then(first, getter):
    def probe(g):
        first(g)
        return getter(g)
    return probe


# entry point -> (what it returns on the fresh handle, the oracle's word for it)
PROBES = {
    "hk_get_agent_state": (lambda g: g.agent_state(), "agent_state"),
    "hk_get_env_state": (lambda g: g.env_state(), "env_state"),
    "hk_get_observations": (lambda g: g.observations(), "observations"),
    "hk_get_rewards": (lambda g: np.stack(g.rewards()), "rewards"),
    "hk_get_episode_results": (lambda g: g.episode_results(), "episode_results"),
    "hk_get_mcts_state": (lambda g: g.mcts_state(), "mcts_state"),
    "hk_device_agents_ptr": (lambda g: _read(g, g.L.hk_device_agents_ptr(g.h), AGENT_DT, (g.E, g.A)), "agent_state"),
    "hk_device_results_ptr": (lambda g: _read(g, g.L.hk_device_results_ptr(g.h), RESULT_DT, (g.E, g.A)), "episode_results"),
    "hk_device_obs_ptr": (_observed, "observations"),
    "hk_synchronize": (_then(lambda g: g.synchronize(), lambda g: g.agent_state()), "agent_state"),
    "hk_reset": (_then(lambda g: g.reset(), lambda g: g.agent_state()), "agent_state after a reset"),
}
APPLIES = {
    "lazy": [p for p in PROBES if p not in ("hk_get_rewards", "hk_get_mcts_state")],          # (a handle without rewards and planner)
    "optimistic": [p for p in PROBES if p not in ("hk_get_rewards", "hk_get_mcts_state")],
    "split": ["hk_get_agent_state", "hk_device_agents_ptr", "hk_synchronize"],
    "search": list(PROBES),
}
_oracle = {}


def _pending(state, monkeypatch):
    """-> (a fresh handle in the state, the oracle's words after the same calls; computed once per state)"""
    make, switches, calls, says = STATES[state]
    for k, v in switches.items():
        monkeypatch.setenv(k, v)          # (read by hk_create)
    cfg, attach = make()
    if state in _oracle:
        g = hk.RacingEnv(cfg)
        if attach:
            g.attach_policy(*attach(g.obs_dim))
        g.reset()
    else:
        g, o = twin(cfg, attach)
        for n in calls:
            o.step(n)
        # the observations last: CollectObservations raises reward events
        ref = {"agent_state": o.agent_state(), "env_state": o.env_state(), "episode_results": o.episode_results(), "mcts_state": o.mcts_state(),
               "rewards": np.stack(o.rewards()), "observations": o.observations()}
        o.reset()
        ref["agent_state after a reset"] = o.agent_state()
        o.close()
        _oracle[state] = ref
    for n in calls:
        g.step(n)
    info = g.schedule_info()
    assert {k: info[k] for k in says} == says, "the calls did not run the schedule that leaves the state: %r" % info
    return g, _oracle[state]


@pytest.mark.parametrize("state,entry", [(s, p) for s in STATES for p in APPLIES[s]])
def test_first_touch_settles(state, entry, monkeypatch):
    g, ref = _pending(state, monkeypatch)
    probe, word = PROBES[entry]
    got = probe(g)
    if word == "env_state":
        for n in ENV_FIELDS:
            assert_bits_equal(got[n], ref[word][n], (state, entry), path="env_state." + n)
    else:
        assert_bits_equal(got, ref[word], (state, entry), path=word)
    g.close()
