"""The games-per-launch meter (hk_prof_meter; env_b1_kernel writes it, hk_api.hip meter_look / apply_meter pick the schedule from it) against the
oracle's per-launch totals, for every call size.

On a field in lock-step (no resets inside the window) a part's B1 launches are its solve ticks, in order, followed by the launches of rounds that found
no env at a solve tick (the worst-case round counts, a lazily completed call's tail) — which hold no game.  The B1 launches of each call are counted by
hk_prof_read; the oracle, stepped one tick at a time, gives the games (egos that hold a multi-player game) of each solve tick.  Then, after a
synchronising getter:
  unsplit handle   the slot of the part's last launch (launch k counts into slot k % 3) equals the reference total of that launch, and word [3] equals
                   m <- max(total of the launch before, m - (m >> 2)) applied to the reference sequence (hk_env_device.h GAME_METER);
  split handle     the slots of the parts' last launches, summed over the parts, equal the reference total (the sum does not depend on the regroup).
And the schedule follows the meter: on a dense aligned field stepped 2, 4 or 20 ticks at a time the label leaves "sparse", and it is always meter_look's
classification of the value hk_schedule_info reports.  Every call also keeps the agent records bit-identical to the oracle."""
import pytest
from parity import assert_child, assert_same_state, twin

pytestmark = pytest.mark.gpu


def _decayed(seq):
    m = 0
    for k in range(len(seq)):
        prev = seq[k - 1] if k > 0 else 0
        m = max(prev, m - (m >> 2))
    return m


def _child_meter(case):
    import hierarchicalkarting_amd as hk
    split = case.startswith("split")
    E = 8192 + 192 if split else 2048
    b = hk.make_config(E, 4, jitter_seed=5, laps=3, max_episode_steps=4000)
    g, o = twin(b)
    g.prof_enable(True); g.prof_reset()
    seq = []                 # reference total of every B1 launch of a part (split: of both parts together, launch by launch)
    launched = 0
    t = 0

    def oracle_call(n):
        # the games of each solve tick of an n-tick call of a field in lock-step (0 for the solve ticks of the start hold the kernels skip: hk.h hk_prof_games)
        tot = []
        c = int(o.game_counts()[2:].sum())
        for _ in range(n):
            o.step(1)
            steps = o.env_state()["episode_steps"]
            assert (steps == steps[0]).all(), "the field left lock-step"
            c1 = int(o.game_counts()[2:].sum())
            if steps[0] % 4 == 0:
                tot.append(0 if 4 < steps[0] < b.cfg.start_hold_ticks else c1 - c)
            else:
                assert c1 == c
            c = c1
        return tot

    def call(n):
        nonlocal launched, t
        before = g.prof_read()["env_b1_kernel"][1]
        g.step(n)
        tot = oracle_call(n)
        t += n
        L = g.prof_read()["env_b1_kernel"][1] - before
        parts = 2 if split else 1
        assert L % parts == 0, (case, t, L)
        L //= parts
        assert L >= len(tot), (case, t, n, L, tot)
        seq.extend(tot + [0] * (L - len(tot)))
        launched += L
        w = g.prof_meter()
        if launched:
            last = (launched - 1) % 3
            got = sum(w[p][last] for p in range(parts))
            assert got == seq[-1], (case, t, n, "last launch", launched, w[:parts], seq[-4:])
            if not split:
                assert w[0][3] == _decayed(seq), (case, t, n, "decaying maximum", w[0], _decayed(seq), seq[-4:])

    SIZES = [1] * 6 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [20] * 2 + [1, 2, 3, 4, 5, 20, 1, 7, 2]
    if not split:
        SIZES = SIZES + [64, 512]
    for n in SIZES:                         # the race start: dense
        call(n)
    assert_same_state(g, o, (case, t))
    dense_m = max(seq)
    assert dense_m > E // 8, (case, dense_m)
    while t < 600:                          # on to a spread field (fixed-round calls: every launch of a split handle stays split)
        call(min(20, 600 - t) if split else min(128, 600 - t))
    assert_same_state(g, o, (case, t))
    for n in SIZES:                         # a spread field
        call(n)
    assert_same_state(g, o, (case, t))
    print("meter ok", case, t, launched, dense_m, seq[-6:])


def _child_label(N):
    import hierarchicalkarting_amd as hk
    E = 2048
    g, o = twin(hk.make_config(E, 4, jitter_seed=5, laps=3, max_episode_steps=4000))
    prev_sparse = None
    labels = []
    for k in range(max(160 // N, 8)):           # the close field of the race start, stepped N ticks at a time from an aligned start
        g.step(N); o.step(N)
        s = g.schedule_info()
        v, lab = s["games_meter_value"], s["games_meter"]
        epl = E / s["streams"]
        # meter_look (hk_api.hip): sparse up to 1 per 40 envs of a launch, or 1 per 28 if it was sparse at the last look; dense beyond 1 per 8
        sparse = v <= epl / 40.0 or (bool(prev_sparse) and v <= epl / 28.0)
        want = "sparse" if sparse else ("dense" if v > epl / 8.0 else "medium")
        assert lab == want, (N, k, s)
        prev_sparse = lab == "sparse"
        labels.append(lab)
    assert_same_state(g, o, N)
    assert labels[-1] != "sparse", (N, labels, g.prof_meter()[0], s)
    print("label ok", N, labels[-1], s["games_meter_value"])


CASES = {"unsplit": {}, "unsplit_no_optimistic": {"HK_NO_OPTIMISTIC": "1"}, "split": {}, "split_no_optimistic": {"HK_NO_OPTIMISTIC": "1"}}


@pytest.mark.parametrize("case", sorted(CASES))
def test_meter_equals_the_reference_per_launch_totals(case):
    assert_child(_child_meter, case, switches=CASES[case], timeout=1200)


@pytest.mark.parametrize("n", [2, 4, 20])
def test_schedule_follows_the_meter_on_a_dense_field(n):
    assert_child(_child_label, n, timeout=600)
