"""Parity of every instantiation of the tick kernel under every scheduling mode (a kernel whose results once depended
on its loop form deserves a test per instantiated <HAS_MCTS, HAS_RW, HAS_TRAIN, TAB_LDS> x {eager assembly on / off, planner pause on / off,
split batch, fused / fission}) and of the 8-lane groups' instantiations (hk::g8).  The switches are read once per process (hk_create), so every combination runs in a child process; each child steps a
small batch through resets, short and long calls against the CPU oracle, every field of every agent record bit for bit."""
import pytest
from parity import assert_child, assert_same_state, step_both, twin

pytestmark = pytest.mark.gpu


def _child_matrix(kind):
    import os
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    MC, FX, LQ, RL = _lib.HK_HIGH_MCTS, _lib.HK_HIGH_FIXED, _lib.HK_LOW_LQR, _lib.HK_LOW_RL
    kw = dict(jitter_seed=0x5EED0000, laps=1, max_episode_steps=260)
    E = 8192 + 64 if os.environ.get("HK_SPLIT") == "1" else 160
    E8 = 40
    cfg = {
        "plain": lambda: hk.make_config(E, 4, **kw),                                                                        # <false, false, false>
        "rewards": lambda: hk.make_config(E, 4, rewards=1, **kw),                                                           # <false, true, false>
        "planner": lambda: hk.make_config(E, 4, high_mode=[MC, MC, FX, FX], tree_search_depth=[8, 8, 5, 5], mcts_iterations=12, **kw),   # <true, false, false>
        "planner_rw": lambda: hk.make_config(E, 4, high_mode=[MC, FX, MC, FX], tree_search_depth=[8, 5, 8, 5], mcts_iterations=12, rewards=1, **kw),   # <true, true, false>
        "training": lambda: hk.make_config(E, 4, env_mode=_lib.HK_MODE_TRAINING, training_agents=[1, 1, 0, 0], rewards=1, jitter_seed=0, laps=1,
                                           max_episode_steps=260),                                                          # <true, true, true>
        # round 4: handles with attached actors — with and without LQ agents beside them (decision chunks on the fission schedule / the tick kernel alone)
        "actor_lq": lambda: hk.make_config(E, 4, low_mode=[RL, RL, LQ, LQ], **kw),
        "actor_only": lambda: hk.make_config(E, 4, low_mode=[RL] * 4, **kw),
        "planner_actor_lq": lambda: hk.make_config(E, 4, high_mode=[MC, MC, FX, FX], low_mode=[RL, RL, LQ, LQ], tree_search_depth=[8, 8, 5, 5],
                                                   mcts_iterations=12, **kw),
        # the 8-lane groups (hk::g8, BASELINE configs[4]): plain LQNG, planner + on-device actor for one team, Training mode
        "g8_plain": lambda: hk.make_config(E8, 8, **kw),
        "g8_planner_actor": lambda: hk.make_config(E8, 8, high_mode=[MC] * 8, low_mode=[RL] * 4 + [LQ] * 4, tree_search_depth=8, mcts_iterations=8, **kw),
        "g8_training": lambda: hk.make_config(E8, 8, env_mode=_lib.HK_MODE_TRAINING, training_agents=[1] * 4 + [0] * 4, rewards=1, jitter_seed=0, laps=1,
                                              max_episode_steps=260),
    }[kind]()
    attach = None
    if kind in ("actor_lq", "actor_only", "planner_actor_lq"):
        attach = lambda D: (Policy.random(D * 4, 64, 2, seed=78), [0, 1] if kind != "actor_only" else [0, 1, 2, 3], 2)
    if kind == "g8_planner_actor":
        attach = lambda D: (Policy.random(D * 4, 64, 2, seed=77), [0, 1, 2, 3], 2)
    g, o = twin(cfg, attach)
    # start hold, race start, short calls, long calls (lazy / pause), a time-out reset inside
    calls = (90, 70, 1, 2, 3, 20, 7, 107, 300) if not kind.startswith("g8") else (90, 40, 1, 2, 3, 20, 7, 127)
    step_both(g, o, calls, check=lambda g, o, t: assert_same_state(g, o, (kind, t)))
    assert (g.env_state()["episodes_done"] >= 1).all() or kind.startswith("g8") or "actor" in kind
    print("matrix ok", kind)


MODES = {"default": {}, "tab_global": {"HK_TAB_GLOBAL": "1"}, "fixed_rounds": {"HK_FIXED_ROUNDS": "1"}}
CASES = [(k, m) for k in ("plain", "rewards", "planner", "planner_rw", "training") for m in MODES]
CASES += [("plain", "split"), ("rewards", "split"), ("planner", "no_pause"), ("planner_rw", "no_pause"), ("training", "no_pause")]
# the fused tick kernel of plain handles (the default since round 4 is the tick kernel without phase B1 + env_b1_kernel: hk_env_run.h FISSION)
CASES += [("plain", "fused"), ("plain", "fused_split"), ("plain", "fused_tab_global")]
# the 8-lane groups under the scheduling modes
CASES += [(k, m) for k in ("g8_plain", "g8_planner_actor", "g8_training") for m in ("default", "fixed_rounds", "tab_global")]
# the fission schedule of planner / actor handles against its fused alternatives (round 4)
CASES += [(k, m) for k in ("actor_lq", "actor_only", "planner_actor_lq") for m in ("default", "fused", "tab_global")]
CASES += [("planner", "fused")]
# round 5: the planner's long calls with the searches beside the ticks (the default) against the schedule that stops an env at its request
CASES += [("planner", "no_overlap"), ("planner_rw", "no_overlap")]
# reward-shaped / Training handles: the fission schedule is their default since round 5; their fused kernel stays reachable (HK_FISSION=0: every handle fused)
CASES += [("rewards", "fused"), ("planner_rw", "fused"), ("training", "fused")]
MODES.update({"no_overlap": {"HK_MCTS_NO_OVERLAP": "1"}})
# the searches beside the ticks in 8-wave workgroups on half the CUs (the default is 4 waves on every CU wherever a tick block fits beside one, with phase B1 on
# its global-table instantiation and lqn_round_small_kernel for those rounds): both forms of the side launch stay reachable
CASES += [("planner", "side8"), ("planner_rw", "side8")]
MODES.update({"side8": {"HK_MCTS_SIDE_WAVES": "8"}})
# round 6: where the multi-player games of the fission schedule are solved — by the B1 waves that assembled them (in every round, the race start too; the
# default does so only once the field has spread), through the queues by the spread solver's launch, through the queues by the pair / matrix-core kernel
CASES += [(k, m) for k in ("plain", "rewards", "planner", "planner_rw", "training", "actor_lq", "planner_actor_lq") for m in ("inwave_all", "queues", "queues_pair")]
CASES += [("plain", "inwave_all_split"), ("plain", "inwave_all_tab_global")]
MODES.update({"inwave_all": {"HK_INWAVE": "1"}, "queues": {"HK_INWAVE": "0"}, "queues_pair": {"HK_INWAVE": "0", "HK_LQN": "pair"},
              "inwave_all_split": {"HK_INWAVE": "1", "HK_SPLIT": "1"}, "inwave_all_tab_global": {"HK_INWAVE": "1", "HK_TAB_GLOBAL": "1"}})
MODES.update({"split": {"HK_SPLIT": "1"}, "no_pause": {"HK_MCTS_NO_PAUSE": "1"}, "fused": {"HK_FISSION": "0"}, "fused_split": {"HK_FISSION": "0", "HK_SPLIT": "1"},
              "fused_tab_global": {"HK_FISSION": "0", "HK_TAB_GLOBAL": "1"}})


@pytest.mark.parametrize("kind,mode", CASES)
def test_every_instantiation_under_every_mode(kind, mode):
    assert "matrix ok " + kind in assert_child(_child_matrix, kind, switches=MODES[mode], timeout=900).output
