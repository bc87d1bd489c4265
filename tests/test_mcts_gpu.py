"""MCTS planner on device (mcts_search_kernel + the request / consume hooks of the fused tick kernel, through the C ABI)
vs the CPU oracle: planner state (pending / visible plans, beliefs, section times) and every agent field bit-identical,
tick by tick, including time-out resets that re-plan."""
import functools
import pytest
from hierarchicalkarting_amd import _lib
from parity import assert_bits_equal, assert_same_state, step_both, twin

pytestmark = pytest.mark.gpu
MC, FX = _lib.HK_HIGH_MCTS, _lib.HK_HIGH_FIXED


def _pair(E, A, high, **kw):
    import hierarchicalkarting_amd as hk
    kw.setdefault("tree_search_depth", [8 if h == MC else 5 for h in high])
    return twin(hk.make_config(E, A, high_mode=high, **kw))


_check = functools.partial(assert_same_state, mcts=True)


def test_first_plan_matches():
    g, o = _pair(16, 2, [MC, FX], jitter_seed=3, mcts_iterations=48)
    _check(g, o, 0)
    assert (g.mcts_state()["pend"]["n_states"][:, 0] == 8).all()


def test_two_agent_mcts_vs_fixed_tick_by_tick():
    g, o = _pair(6, 2, [MC, FX], jitter_seed=5, mcts_iterations=32)
    for t in range(1, 331):
        g.step(1); o.step(1)
        if t % 10 == 0 or 70 < t < 80 or 140 < t < 150:
            _check(g, o, t)
        else:
            assert_bits_equal(g.mcts_state(), o.mcts_state(), (t, "mcts_state"))


@pytest.mark.parametrize("persist_gb", ["64", "0"])
def test_four_agents_all_mcts_odd_steps_and_timeout_resets(persist_gb, monkeypatch):
    monkeypatch.setenv("HK_MCTS_PERSIST_GB", persist_gb)
    g, o = _pair(12, 4, [MC, MC, MC, MC], jitter_seed=7, mcts_iterations=16, max_episode_steps=260)
    step_both(g, o, (3, 97, 1, 45, 60, 54, 7, 100, 133, 29, 71), check=_check)
    assert (g.env_state()["episodes_done"] >= 2).all()


def test_long_calls_without_the_pause_schedule(monkeypatch):
    """HK_MCTS_NO_PAUSE=1: long calls keep the fully asynchronous deadline schedule (searches launched every few rounds, envs never
    wait) — the schedule must not show in the results"""
    monkeypatch.setenv("HK_MCTS_NO_PAUSE", "1")
    g, o = _pair(10, 4, [MC, MC, MC, MC], jitter_seed=19, mcts_iterations=16)
    step_both(g, o, (150, 90, 260), check=_check)


def test_mixed_team_complex_track():
    g, o = _pair(8, 4, [MC, FX, MC, FX], track="complex", jitter_seed=2, mcts_iterations=20)
    step_both(g, o, (100, 50, 150, 200), check=_check)


def test_create_rejects_bad_planner_budgets():
    import hierarchicalkarting_amd as hk
    for kw in (dict(mcts_latency_ticks=4), dict(mcts_latency_ticks=120), dict(mcts_iterations=0), dict(tree_search_depth=[9, 5])):
        with pytest.raises(hk.HkError):
            hk.RacingEnv(hk.make_config(2, 2, high_mode=[MC, FX], **{**dict(tree_search_depth=[8, 5]), **kw}))
    # a tree pool beyond 65 535 nodes per search (1 + (initial + 2 x replan iterations) x (depth x agents + 1): a root can be
    # searched three times) is refused, not truncated
    with pytest.raises(hk.HkError) as e:
        hk.RacingEnv(hk.make_config(2, 2, high_mode=[MC, FX], tree_search_depth=[8, 5], mcts_iterations=2000))
    assert e.value.code == _lib.HK_ERR_UNSUPPORTED
    hk.RacingEnv(hk.make_config(2, 2, high_mode=[MC, FX], tree_search_depth=[8, 5], mcts_iterations=1000)).close()   # 1 + 3667 x 17 nodes fits
    with pytest.raises(hk.HkError):
        hk.RacingEnv(hk.make_config(2, 2, high_mode=[MC, FX], tree_search_depth=[8, 5], section_window=5))   # sectionTimes ring: window <= 4


@pytest.mark.parametrize("persist_gb", ["64", "0"])
def test_root_reuse_matches_the_oracles_persistent_trees(persist_gb, monkeypatch):
    """HKA:265-283, both homes of the trees: one arena slice per agent (the tree survives between searches, as in the oracle) and,
    when that does not fit the memory budget (forced here with HK_MCTS_PERSIST_GB=0), one per resident lane with the re-searched
    tree rebuilt by replaying the searches it received.  Kart 0 is pinned to its grid slot (never enters a section): searched at
    reset, at tick 100 and 200 on the same root, then not at all; the other karts race on and drop their roots at every section
    they enter."""
    monkeypatch.setenv("HK_MCTS_PERSIST_GB", persist_gb)
    g, o = _pair(6, 4, [MC, MC, MC, FX], jitter_seed=13, mcts_iterations=20)
    st = o.agent_state()
    t = 0
    for k in range(18):
        g.step(25); o.step(25); t += 25
        _check(g, o, t)
        a = o.agent_state()
        a[:, 0] = st[:, 0]
        o.set_agent_state(a); g.set_agent_state(a)
    m = g.mcts_state()
    assert (m["searches"][:, 0] == 3).all() and (m["root_cycles"][:, 0] == 3).all() and (m["root_phases"][:, 0] == 3).all()
    assert (m["searches"][:, 1:3] == 5).all()
    assert (m["root_phases"][:, 1:3].max() >= 1)


def test_section_window_three_reads_section_times_two_rows_back():
    g, o = _pair(8, 4, [MC, MC, MC, MC], jitter_seed=17, mcts_iterations=16, section_window=3, mcts_seed=5)
    _check(g, o, 0)
    row2 = g.agent_state()["section_index"] == 1
    assert row2.sum() == 16 and (g.mcts_state()["sec_time"][:, :, 0][row2] < 0).all()     # the second grid row got a made-up time for section 0 (REC:690)
    step_both(g, o, (100, 45, 55, 100), check=_check)


def test_tick_by_tick_stepping_defers_but_never_misses_a_plan():
    """A host that steps one tick per call (Unity's FixedUpdate) or in small uneven chunks: the searches are batched over up to
    32 armed ticks, yet every plan is there when it is due — records, plans and beliefs equal the oracle's all the way."""
    import hierarchicalkarting_amd as hk
    g, o = twin(hk.make_config(6, 4, track="complex", jitter_seed=21, high_mode=_lib.HK_HIGH_MCTS, tree_search_depth=4, mcts_iterations=10,
                               mcts_latency_ticks=41, mcts_initial_latency_ticks=41))
    t = 0
    chunks = [1] * 130 + [3, 7, 31, 2, 32, 33, 1, 1, 30, 5, 64, 1] + [1] * 60
    for k, n in enumerate(chunks):
        g.step(n); o.step(n); t += n
        if k % 9 == 0 or n > 1:
            assert_same_state(g, o, t)
    assert_bits_equal(g.mcts_state(), o.mcts_state(), (t, "mcts_state"))
    assert g.mcts_state()["searches"].min() >= 4
