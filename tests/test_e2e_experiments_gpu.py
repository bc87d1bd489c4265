"""The reference's 16 EndToEndKartAgent ("E2E") set-ups of the *All scenes, raced on libhk with the scenes' own actors (tests/e2e_setups.py).

(a) every set-up runs its TotalExperiments races (48 / 50 envs, MCTS opponents at the mcts_iterations of tests/test_experiments_gpu.py) and
    every agent row of a set-up with a log of its own name falls in the bands of tests/test_reference_logs.py, or is listed in
    E2E_RESIDUALS with its measured ratios and a cause;
(b) for one 1v1 and one 2v2 set-up per track, the first 1 500 ticks tick by tick against the CPU oracle fed libhk's actions, the E2E slot
    run there as Fixed-RL (the mechanism and exemptions of tests/test_e2e_gpu.py); then the same race in 20-tick calls and in one call;
(c) every set-up reproduces the hashes of tests/golden/e2e_experiment_gpu.json (tools/compare_experiment_logs.py --e2e --update)."""
import functools
import json
import os
import sys
import numpy as np
import pytest
import e2e_setups as E2E
import oracle_lib as O
from test_e2e_gpu import _check        # every field bit for bit but the E2E slots' exempt ones
from test_reference_logs import BANDS, LANE_DIFF_BAND

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")
GPU = json.load(open(os.path.join(GOLD, "e2e_experiment_gpu.json")))
REF = json.load(open(os.path.join(GOLD, "reference_e2e_log_stats.json")))
ALL = sorted(E2E.experiments())
# set-ups raced and hashed but not banded: no log of their own name.  Only ...Duos.txt exists, and no controller of any scene is called
# that, so the scenes do not show which controller wrote it (it is older than the *All scenes' "...2" controllers)
NO_LOG = ("E2E_vs_Fixed_RL_ComplexDuos2", "E2E_vs_Fixed_RL_OvalDuos2")
# (set-up, agent type) -> {statistic: libhk / reference as measured on the MI355X}, "cause": why it is outside the bands.  Filled from
# tools/compare_experiment_logs.py --e2e; the bands themselves are test_reference_logs.py's and are not widened here.
E2E_RESIDUALS = {
    # the reference's E2E team is stopped in 21 of 96 races (DNF) and its finishers lose time to the same contacts; ours finish all 96.
    # 0.9699 is 0.01 % under the pace band; the same set-up's best lap (0.981) and the E2E team against MCTS-LQR (0.974) are inside
    ("E2E_vs_Fixed_LQR_ComplexDuos2", "E2E"): {"mean_total_time": 0.9699,
                                               "cause": "reference E2E team: 21 / 96 DNFs and slowed finishers; ours: 0 DNFs"},
    # our Fixed-RL actor keeps its lane more tightly than the reference's in every 1v1 Oval set-up (0.78 - 0.91 x in the 22 hierarchical
    # set-ups); against the E2E kart the reference's metric is its widest (0.58 m against 0.46 - 0.60 there), ours stays at 0.41 m
    ("E2E_vs_Fixed_RL_Oval2", "Fixed-RL"): {"mean_lane_difference": 0.6999,
                                            "cause": "Fixed-RL lane tracking tighter than the reference's, as in the hierarchical set-ups"},
    # the reference's MCTS_RL_vs_E2E_ComplexDuos.txt is byte for byte MCTS_RL_vs_E2E_OvalDuos.txt: Oval lap times (19.4 s best lap)
    # against a 33 - 35 s Complex lap.  Not a Complex race; our Complex races are in the bands of the other Complex 2v2 set-ups
    ("MCTS_RL_vs_E2E_ComplexDuos", "E2E"): {"median_best_lap": 1.7318, "mean_total_time": 1.2938,
                                            "cause": "the reference's log of this name is a copy of the OvalDuos log"},
    ("MCTS_RL_vs_E2E_ComplexDuos", "MCTS-RL"): {"median_best_lap": 1.7452, "mean_total_time": 1.3008,
                                                "cause": "the reference's log of this name is a copy of the OvalDuos log"},
}


@functools.lru_cache(maxsize=None)
def _race(name):
    import compare_experiment_logs as CE
    res, stats = CE.run_e2e(name, GPU[name]["mcts_iterations"])
    return CE.results_hash(res), stats


def _outside(o, r):
    """{statistic: ratio} of the band checks test_reference_logs.py applies to an agent row that fail here"""
    bad = {}
    if o["dnfs"] > max(r["dnfs"], 2):
        bad["dnfs"] = (o["dnfs"], r["dnfs"])
    for k, (lo, hi) in BANDS.items():
        if o[k] is None or r[k] is None or not lo <= o[k] / r[k] <= hi:
            bad[k] = None if o[k] is None or r[k] is None else round(o[k] / r[k], 4)
    if o["mean_lane_difference"] is not None and r["mean_lane_difference"]:
        ratio = o["mean_lane_difference"] / r["mean_lane_difference"]
        if not LANE_DIFF_BAND[0] <= ratio <= LANE_DIFF_BAND[1]:
            bad["mean_lane_difference"] = round(ratio, 4)
    return bad


def test_the_16_setups_are_raced_and_the_logs_accounted_for():
    assert len(ALL) == 16 and set(GPU) == set(ALL)
    assert set(REF) | set(NO_LOG) == set(ALL) and not set(REF) & set(NO_LOG)
    for key, row in E2E_RESIDUALS.items():
        assert key[0] in REF and row.get("cause"), key


@pytest.mark.parametrize("name", ALL)
def test_e2e_setups_fall_in_the_reference_bands(name):
    """(a): every agent row of a set-up with a log, inside the bands of test_reference_logs.py or an entry of E2E_RESIDUALS"""
    _, ours = _race(name)
    e = E2E.experiments()[name]
    for typ, o in ours.items():                                 # every race of the set-up, for each kart of that type
        assert o["races"] == e["TotalExperiments"] * sum(a["name"].split("(")[0] == typ for a in e["agents"]), (name, typ)
    if name in NO_LOG:
        return
    ref = REF[name]["stats"]
    assert set(ours) == set(ref), name
    for typ, o in ours.items():
        r = ref[typ]
        assert o["races"] == r["races"], (name, typ)
        bad = _outside(o, r)
        if (name, typ) in E2E_RESIDUALS:
            want = {k: v for k, v in E2E_RESIDUALS[(name, typ)].items() if k != "cause"}
            assert bad == want, (name, typ, bad, want)
        else:
            assert not bad, (name, typ, bad)


@pytest.mark.parametrize("name", ALL)
def test_e2e_setups_reproduce_the_stored_races(name):
    """(c)"""
    h, stats = _race(name)
    assert stats == GPU[name]["stats"], name
    assert h == GPU[name]["results_sha256"], name


TWINS = ["E2E_vs_MCTS_LQR_Oval2", "E2E_vs_Fixed_RL_OvalDuos2", "MCTS_RL_vs_E2E_Complex2", "E2E_vs_Fixed_LQR_ComplexDuos2"]
TWIN_TICKS, TWIN_ENVS = 1500, 8


def _handle(s):
    import hierarchicalkarting_amd as hk
    return s.start(hk.RacingEnv)


@pytest.mark.parametrize("name", TWINS)
def test_e2e_setup_twin_against_the_oracle(name):
    """(b): the race start (75 held ticks), the first quasi-MCTS requests (episode steps 100, 200 ...) and the first Trigger entries, tick
    by tick against the oracle; then 20-tick calls and one 1 500-tick call on fresh handles reach the same states and results"""
    s = E2E.Setup(name, n_exp=TWIN_ENVS, mcts_iterations=GPU[name]["mcts_iterations"])
    e2e = [i for i, l in enumerate(s.low) if l == E2E._lib.HK_LOW_E2E]
    g = _handle(s)
    o = O.OracleEnv(s.twin_config())
    for pol, slots, period in s.policies[:s.n_rl_policies()]:     # the RL actors, at the indices they hold on libhk (the index keys the
        o.attach_policy(pol, slots, period)                         # sampling stream); the E2E slots take libhk's actions
    o.reset()
    for t in range(1, TWIN_TICKS + 1):
        g.step(1)
        st, br = g.get_actions()
        o.set_actions(st, br)
        o.step(1)
        gs = _check(g, o, e2e, t)
    assert (gs["section_index"][:, e2e] > 2).all()             # every E2E kart has passed Triggers
    m = g.mcts_state()
    assert all((m["searches"][:, i] >= 1).all() for i in e2e if s.high[i] == E2E._lib.HK_HIGH_MCTS)
    want = (g.agent_state(), g.env_state(), g.episode_results())
    g.close()
    for calls in ([20] * (TWIN_TICKS // 20), [TWIN_TICKS]):
        h = _handle(s)
        for n in calls:
            h.step(n)
        got = (h.agent_state(), h.env_state(), h.episode_results())
        h.close()
        for a, b in zip(got, want):
            for f in a.dtype.names:
                assert np.array_equal(a[f], b[f]), (name, calls[0], f)
