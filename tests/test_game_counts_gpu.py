"""hk_prof_games against the oracle's tally (oracle hko_game_counts, itself checked by hand and against the Python restatement in
tests/test_game_tally_oracle.py): the multi-player games the kernels solved, by player count, must EQUAL the games the reference solves — one per ego per
solve tick that holds one — wherever they are solved (the pair / matrix-core launch, lqn_spread_kernel, in-wave in env_b1_kernel, lqn_big_kernel for 5 .. 8
players, the fused kernel's launches) and whatever the call sizes, the optimistic plan and its recovery, the split into parts and the restart bursts —
less, by the documented rule (hk.h hk_prof_games), the start-hold solves the kernels skip because they would repeat the one before bit for bit.
bench.py's fp64 roofline of the dense regimes is built from these counts.  Words [0] / [1] (in-wave passes, waves that ran any) are held to their rules.
The switches are read in hk_create: one child process per setting, each under a time limit."""
import pytest
from parity import assert_child, assert_same_state, twin

pytestmark = pytest.mark.gpu


def _child_counts(case):
    import os
    import numpy as np
    import hierarchicalkarting_amd as hk
    # The kernels skip the solves of the start hold after its first cadence (hk_env_run.h P.hold_dedupe; hk.h hk_prof_games): the karts cannot move, each
    # solve would decode the controls of the one before bit for bit.  Those games are in the oracle's tally and not in hk_prof_games.  The rule is active
    # while no planner runs, HK_NO_HOLD_DEDUPE is unset and the host has not written kart or env states (hk_set_agent_state turns it off for good).
    hold_dedupe = os.environ.get("HK_NO_HOLD_DEDUPE") != "1"
    skipped = np.zeros(9, np.int64)

    def ostep(o, b, n, dedupe):
        # the oracle, one tick at a time: the games of solve ticks inside the hold (cadence < episode step < hold) go to `skipped` while the rule is on
        cad = 4 if b.cfg.num_agents > 2 else 1
        for _ in range(n):
            c0 = o.game_counts()
            o.step(1)
            if dedupe:
                s = o.env_state()["episode_steps"]
                assert (s == s[0]).all(), "the field left lock-step"
                if cad < s[0] < b.cfg.start_hold_ticks:
                    skipped[:] += o.game_counts() - c0

    def counts(g, o, t):
        got, want = g.prof_games(), o.game_counts() - skipped
        for n in range(2, 9):
            assert got[n] == want[n], (case, t, n, got, want.tolist())
        passes, waves = g.prof_games_words()
        assert waves <= passes <= sum(got.values()), (case, t, passes, waves, got)
        if os.environ.get("HK_INWAVE") == "0":
            assert passes == 0 and waves == 0, (case, t, passes, waves)
        if os.environ.get("HK_INWAVE") == "1" and got[2] + got[3] + got[4] > 0 and case.startswith("race"):
            assert waves > 0, (case, t, got)
        return got

    def run(g, o, b, calls, dedupe=hold_dedupe):
        t = 0
        for n in calls:
            g.step(n); ostep(o, b, n, dedupe); t += n
            assert_same_state(g, o, (case, t))
            last = counts(g, o, t)
        return last

    def counted(b):
        g, o = twin(b)
        g.prof_enable(True); g.prof_reset()
        return g, o

    MIXED = [1, 3, 2, 7, 5, 20, 1, 64, 9, 4, 1, 2, 33, 1]
    if case.startswith("race"):
        # a natural 4-agent Oval race start on a batch that splits, the call patterns of the hosts (one-tick Unity steps, the driver's 20-tick window,
        # lazily completed long calls) one after another on the same field; the counts since prof_reset after every call
        b = hk.make_config(8192 + 192, 4, jitter_seed=5, laps=3, max_episode_steps=4000)
        g, o = counted(b)
        if case == "race":
            calls = [1] * 200 + [2] * 40 + [4] * 20 + [20] * 6 + [64] * 2 + [512] + MIXED
        else:           # the recovery path (HK_OPTIMISTIC_SKEW) / the worst-case round counts (HK_NO_OPTIMISTIC): shorter
            calls = [1] * 40 + [2] * 10 + [4] * 10 + [20] * 4 + [64] + MIXED
        got = run(g, o, b, calls)
        if hold_dedupe:
            assert skipped[2] > 0, skipped     # (the rule was met)
        assert got[2] > 0 and got[3] > 0 and got[4] > 0, got
    elif case == "restart":
        # short episodes with auto-reset: every env restarts at the same tick, the restart burst (a game for every ego on the grid) is counted too
        b = hk.make_config(2048, 4, jitter_seed=9, laps=3, max_episode_steps=120)
        g, o = counted(b)
        got = run(g, o, b, [20] * 8 + [1] * 12 + [64] + [4] * 10 + [100])
        assert (o.env_state()["episodes_done"] >= 2).all()
    elif case == "two_agents":
        # the fused kernel (2-agent handles): a 2-player game for every ego on every tick
        b = hk.make_config(1024, 2, jitter_seed=7, laps=2, max_episode_steps=3000)
        g, o = counted(b)
        got = run(g, o, b, [1] * 20 + [3, 20, 20, 64, 128])
        assert got[2] > 0 and sum(got.values()) == got[2]
    elif case == "eight_agents":
        # the synthetic 8-agent Complex configuration: a natural start, then the whole field packed within 8 m (games of 5 .. 8 players: lqn_big_kernel)
        b = hk.make_config(64, 8, track="complex", jitter_seed=0x5EED0000, laps=1, max_episode_steps=1500)
        g, o = counted(b)
        run(g, o, b, [1] * 8 + [20, 64, 100])
        g.reset(); o.reset()
        st = o.agent_state().copy()
        s0 = b.track["sections"][0]
        for j in range(8):
            lane = j % 4 + 1
            st["px"][:, j] = s0["Lane%d" % lane]["x"]
            st["pz"][:, j] = s0["Lane%d" % lane]["z"] + 2.0 + 2.6 * (j // 4)
            st["lane"][:, j] = lane
            st["section_index"][:, j] = 0
            st["init_checkpoint_index"][:, j] = 0
        g.set_agent_state(st); o.set_agent_state(st)
        g.prof_reset(); o.game_counts_reset(); skipped[:] = 0
        got = run(g, o, b, [76, 4, 1, 3, 20, 64], dedupe=False)      # (written kart states: every solve of the hold runs)
        assert sum(got[n] for n in range(5, 9)) > 0, got
    else:
        raise AssertionError("unknown case " + case)
    g.close(); o.close()
    print("counts ok", case, got)


CASES = {"race": {}, "race_no_optimistic": {"HK_NO_OPTIMISTIC": "1"}, "race_skew": {"HK_OPTIMISTIC_SKEW": "1"},
         "race_inwave": {"HK_INWAVE": "1"}, "race_queues": {"HK_INWAVE": "0"},
         "race_no_hold_dedupe": {"HK_NO_HOLD_DEDUPE": "1"},
         "restart": {}, "two_agents": {}, "eight_agents": {}}


@pytest.mark.parametrize("case", sorted(CASES))
def test_game_counts_equal_the_oracle_tally(case):
    assert_child(_child_counts, case, switches=CASES[case], timeout=1200)
