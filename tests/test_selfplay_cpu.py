"""Self-play on the host (hierarchicalkarting_amd/selfplay.py, include/hk.h "SELF-PLAY"): ELO, the linear schedules, the numpy restatement of the
episode statistics on hand-made rows, SelfPlay's bookkeeping against a fake pool, and the new struct's three layouts.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import selfplay_restate as SR
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.selfplay import (SCHEDULE_MINIMA, SelfPlay, elo_apply, elo_expected, flat_to_policy, linear_schedule,
                                              policy_to_flat)
from test_csharp_layout import _parse_cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ELO
def test_elo_expected_of_equals_is_a_half():
    for r in (0.0, 400.0, 1234.5):
        assert elo_expected(r, r) == 0.5
    assert elo_expected(800.0, 400.0) == 1.0 / 1.1 and elo_expected(400.0, 800.0) == 1.0 / 11.0


def test_elo_apply_is_zero_sum_and_order_free():
    rl, ro = elo_apply(400.0, 520.0, 30, 5, 12)
    assert abs((rl + ro) - 920.0) < 1e-9
    assert rl > 400.0 and ro < 520.0
    assert elo_apply(400.0, 520.0, 0, 0, 0) == (400.0, 520.0)
    assert elo_apply(400.0, 520.0, 3, 0, 0, k=2.0)[0] > elo_apply(400.0, 520.0, 3, 0, 0)[0]


def test_elo_apply_rests_where_the_mean_result_is_the_expectation():
    # equal ratings expect 0.5: all draws, or as many wins as losses
    assert elo_apply(400.0, 400.0, 0, 7, 0) == (400.0, 400.0)
    assert elo_apply(400.0, 400.0, 5, 2, 5) == (400.0, 400.0)
    # a 400-point favourite expects 10 / 11
    rl, ro = elo_apply(800.0, 400.0, 10, 0, 1)
    assert abs(rl - 800.0) < 1e-9 and abs(ro - 400.0) < 1e-9


def test_elo_apply_equals_mlagents_steps_when_all_results_agree():
    def mlagents_step(rating, opp, result):          # GhostController.compute_elo_rating_changes, K = 1
        r1, r2 = 10.0 ** (rating / 400.0), 10.0 ** (opp / 400.0)
        return result - r1 / (r1 + r2)
    for result, (w, d, l) in ((1.0, (9, 0, 0)), (0.5, (0, 9, 0)), (0.0, (0, 0, 9))):
        rl, ro = 400.0, 430.0
        for _ in range(9):
            ch = mlagents_step(rl, ro, result)
            rl, ro = rl + ch, ro - ch
        got = elo_apply(400.0, 430.0, w, d, l)
        assert abs(got[0] - rl) < 1e-9 and abs(got[1] - ro) < 1e-9
        # and, stated with this module's own expectation, bit for bit
        a, b = 400.0, 430.0
        for _ in range(9):
            ch = result - elo_expected(a, b)
            a, b = a + ch, b - ch
        assert got == (a, b)


def test_elo_apply_is_self_limiting():
    rl, ro = elo_apply(400.0, 400.0, 30000, 0, 0)         # a one-shot n (s - e) would be + 15 000
    assert rl - 400.0 < 2000.0 and abs((rl + ro) - 800.0) < 1e-6


# ---- schedules
def test_linear_schedule_end_points_and_clamp():
    assert linear_schedule(3e-4, 1e-10, 0, 1000) == 3e-4
    assert linear_schedule(3e-4, 1e-10, 1000, 1000) == 1e-10
    assert linear_schedule(3e-4, 1e-10, 5000, 1000) == 1e-10
    assert linear_schedule(0.2, 0.1, 500, 1000) == (0.2 - 0.1) * 0.5 + 0.1
    assert SCHEDULE_MINIMA == dict(lr=1e-10, eps=0.1, beta=1e-5)
    vals = [linear_schedule(5e-3, 1e-5, s, 100) for s in range(0, 130, 10)]
    assert all(a >= b for a, b in zip(vals, vals[1:])) and vals[-1] == 1e-5


# ---- the restatement on hand-made rows
def _rows(R, E=1, A=2):
    z = lambda: np.zeros((R, E, A), np.float32)
    return dict(reward=z(), group_reward=z(), term_reward=z(), term_group_reward=z(), done=np.zeros((R, E), np.int32))


def test_restatement_carry_in_completes_an_episode():
    ro = _rows(3)
    ro["reward"][:, 0, 0] = [0.5, 0.25, 7.0]
    ro["group_reward"][:, 0, 0] = [1.0, 0.0, 3.0]
    ro["done"][1, 0] = 1
    ro["term_reward"][1, 0, 0], ro["term_group_reward"][1, 0, 0] = 2.0, -0.5
    carry = SR.empty_carry(1, 2)
    carry["ret"][0, 0], carry["gret"][0, 0], carry["len"][0, 0], carry["whole"][0, 0] = 10.0, 20.0, 4, 1
    st, cout, eps = SR.episode_stats(ro, [0], carry=carry)
    assert (st["episodes"], st["partial"], st["wins"], st["len_sum"]) == (1, 0, 1, 6)
    assert eps == [(np.float32(12.5), np.float32(20.5), 6, 1, np.float32(1.5))]
    assert st["ret_sum"] == 12.5 and st["ret_sumsq"] == 156.25 and st["gret_sum"] == 20.5 and st["ret_min"] == st["ret_max"] == 12.5
    # REWARD on the DONE row opens the next episode, whose length restarts at 0; the row after it adds
    assert (cout["ret"][0, 0], cout["gret"][0, 0], cout["len"][0, 0], cout["whole"][0, 0]) == (7.25, 3.0, 1, 1)
    # slot 1 was not asked for: its carry is what came in
    assert cout["whole"][0, 1] == 0 and cout["len"][0, 1] == 0


def test_restatement_without_a_carry_counts_partial_and_nowhere_else():
    ro = _rows(4)
    ro["reward"][:, 0, 1] = 1.0
    ro["done"][2, 0] = 2
    ro["term_reward"][2, 0, 1] = 5.0
    st, cout, eps = SR.episode_stats(ro, [1])
    assert st["partial"] == 1 and eps == []
    assert all(st[k] == 0 for k in SR.INT_FIELDS if k != "partial")
    assert st["ret_sum"] == 0.0 and st["ret_min"] == np.inf and st["ret_max"] == -np.inf
    assert (cout["ret"][0, 1], cout["len"][0, 1], cout["whole"][0, 1]) == (2.0, 1, 1)
    # a carry that itself began before the chain (whole == 0) is no valid carry either
    st2, _, _ = SR.episode_stats(ro, [1], carry=SR.empty_carry(1, 2))
    assert st2 == st


def test_restatement_two_ends_of_one_lane():
    ro = _rows(6)
    ro["reward"][:, 0, 0] = [1, 2, 4, 8, 16, 32]
    ro["done"][[1, 4], 0] = [1, 2]
    ro["term_reward"][1, 0, 0], ro["term_reward"][4, 0, 0] = 100.0, -3.0
    st, cout, eps = SR.episode_stats(ro, [0])
    # the first end is partial (no carry); the second episode is rows 1 (its REWARD after the reset) .. 4 (its TERM_REWARD): 2 + 4 + 8 - 3
    assert (st["partial"], st["episodes"], st["losses"], st["timeouts"], st["len_sum"]) == (1, 1, 1, 1, 3)
    assert eps[0][:3] == (np.float32(11.0), np.float32(0.0), 3)
    assert (cout["ret"][0, 0], cout["len"][0, 0]) == (48.0, 1)


def test_restatement_outcome_classes():
    # one lane per class, each with a whole carry so that its end counts: +0, -0, an exact cancellation, a NaN, DONE == 2 with f > 0, f < 0
    cases = [(0.0, 0.0, 1, "draws"), (-0.0, -0.0, 1, "draws"), (1.5, -1.5, 1, "draws"), (np.nan, 1.0, 1, "draws"), (0.25, 0.5, 2, "wins"),
             (0.25, -0.5, 1, "losses")]
    E = len(cases)
    ro = _rows(1, E, 1)
    carry = SR.empty_carry(E, 1)
    carry["whole"][:] = 1
    for e, (tr, tg, d, _) in enumerate(cases):
        ro["term_reward"][0, e, 0], ro["term_group_reward"][0, e, 0], ro["done"][0, e] = tr, tg, d
    st, _, eps = SR.episode_stats(ro, [0], carry=carry)
    assert (st["episodes"], st["wins"], st["draws"], st["losses"], st["timeouts"], st["partial"], st["len_sum"]) == (6, 1, 4, 1, 1, 0, 6)
    for e, (_, _, _, kind) in enumerate(cases):
        one = {k: v[:, e:e + 1] for k, v in ro.items()}
        s1, _, _ = SR.episode_stats(one, [0], carry={k: v[e:e + 1] for k, v in carry.items()})
        assert s1[kind] == 1 and s1["wins"] + s1["draws"] + s1["losses"] == 1, (e, kind)


def test_restatement_rows_argument_and_fp32_rounding():
    ro = _rows(3)
    ro["reward"][:, 0, 0] = [1e8, 1.0, -1e8]           # fp32: 1e8 + 1 == 1e8
    ro["done"][2, 0] = 1
    carry = SR.empty_carry(1, 2)
    carry["whole"][:] = 1
    st, _, eps = SR.episode_stats(ro, [0], carry=carry)
    assert eps[0][0] == np.float32(1e8) and st["ret_sum"] == 1e8       # (TERM_REWARD 0 is what the DONE row adds)
    st2, cout2, _ = SR.episode_stats(ro, [0], rows=2, carry=carry)
    assert st2["episodes"] == 0 and cout2["len"][0, 0] == 2


# ---- SelfPlay's bookkeeping against a fake pool
class _FakePool:
    def __init__(self):
        self.calls = []

    def save(self, slot, policy_index=None):
        self.calls.append(("save", slot))

    def load(self, slot, policy_index):
        self.calls.append(("load", slot, policy_index))


class _FakeTrainer:
    index = 0


def _sp(**kw):
    pool = _FakePool()
    return SelfPlay(None, _FakeTrainer(), 1, pool=pool, **kw), pool


def test_selfplay_window_wraps_and_slots_keep_the_rating_at_save_time():
    sp, pool = _sp(window=3, save_steps=10, swap_steps=10 ** 9, initial_elo=400.0)
    assert pool.calls == [("save", 0)] and sp.cursor == 1 and sp.ratings == [400.0] * 3
    slots, want = [], {0: 400.0}
    for i in range(7):
        sp.record_results(3 + i, 1, 2)                 # the learner's rating moves before every save
        saved, swapped = sp.advance(10)
        assert swapped is None and saved == (i + 1) % 3
        slots.append(saved)
        want[saved] = sp.elo
        assert sp.ratings[saved] == sp.elo
    assert slots == [1, 2, 0, 1, 2, 0, 1]
    assert sp.ratings == [want[0], want[1], want[2]]
    assert [c for c in pool.calls if c[0] == "save"] == [("save", 0)] + [("save", s) for s in slots]
    # not due: nothing happens
    assert sp.advance(9) == (None, None) and sp.advance(1)[0] == 2


def test_selfplay_same_seed_same_opponents_and_the_two_ratios():
    def run(seed, ratio):
        sp, pool = _sp(window=4, save_steps=5, swap_steps=3, play_against_latest_model_ratio=ratio, seed=seed)
        for _ in range(40):
            sp.advance(3)
        return sp, pool
    a, pa = run(7, 0.5)
    b, _ = run(7, 0.5)
    c, _ = run(8, 0.5)
    assert a.history == b.history and len(a.history) == 40 and a.history != c.history
    assert "latest" in a.history and any(isinstance(x, int) for x in a.history)
    never, pn = run(7, 0.0)
    assert "latest" not in never.history and all(0 <= x < 4 for x in never.history)
    always, pl = run(7, 1.0)
    assert set(always.history) == {"latest"}
    # latest: the learner is saved into the last slot (index window), then loaded into the opponent; a window pick is loaded as it is
    assert ("save", 4) in pl.calls and ("load", 4, 1) in pl.calls and ("save", 4) not in pn.calls
    # a pick is always a filled slot: the first swap happens with one save so far
    first, _ = _sp(window=4, save_steps=10 ** 9, swap_steps=1, play_against_latest_model_ratio=0.0, seed=3)
    for _ in range(10):
        first.advance(1)
    assert set(first.history) == {0}


def test_selfplay_ratings_follow_elo_apply():
    sp, _ = _sp(window=2, save_steps=10 ** 9, swap_steps=4, play_against_latest_model_ratio=0.0, initial_elo=400.0, seed=1)
    # before the first swap the opponent plays its attached weights
    sp.record_results(6, 0, 2)
    l1, o1 = elo_apply(400.0, 400.0, 6, 0, 2)
    assert (sp.elo, sp.attached_elo, sp.opponent) == (l1, o1, None) and sp.ratings == [400.0, 400.0]
    assert sp.advance(4) == (None, 0) and sp.opponent == 0 and sp.opponent_elo() == 400.0
    sp.record_results(1, 1, 5)
    l2, o2 = elo_apply(l1, 400.0, 1, 1, 5)
    assert (sp.elo, sp.ratings[0], sp.attached_elo) == (l2, o2, o1)
    # latest: the learner's own rating, not decremented
    sp.opponent = "latest"
    sp.record_results(4, 0, 0)
    assert sp.ratings[0] == o2 and sp.elo == elo_apply(l2, l2, 4, 0, 0)[0] and sp.opponent_elo() == sp.elo


def test_selfplay_schedules():
    sp, _ = _sp(window=2, max_steps=1000)
    assert sp.scheduled(3e-4, 0.2, 5e-3) == (3e-4, 0.2, 5e-3)
    sp.steps = 500
    assert sp.scheduled(3e-4, 0.2, 5e-3) == (linear_schedule(3e-4, 1e-10, 500, 1000), linear_schedule(0.2, 0.1, 500, 1000),
                                             linear_schedule(5e-3, 1e-5, 500, 1000))
    assert sp.scheduled(3e-4, 0.2, 5e-3, {"lr": "constant"}, {"eps": 0.05})[:2] == (3e-4, linear_schedule(0.2, 0.05, 500, 1000))
    sp.steps = 99999
    assert sp.scheduled(3e-4, 0.2, 5e-3) == (1e-10, 0.1, 1e-5)
    flat, _ = _sp(window=2)
    flat.steps = 500
    assert flat.scheduled(3e-4, 0.2, 5e-3) == (3e-4, 0.2, 5e-3)
    with pytest.raises(ValueError):
        flat.scheduled(3e-4, 0.2, 5e-3, {"lr": "linear"})


def test_flat_vector_round_trip():
    for norm in (True, False):
        pol = Policy.random(78, 32, 2, seed=5, stack=1, normalize=norm, deterministic=True)
        flat = policy_to_flat(pol)
        assert flat.size == 78 * 32 + 32 + 32 * 32 + 32 + 32 + 1 + 1 + 3 * 32 + 3 + (2 * 78 if norm else 0)
        back = flat_to_policy(flat, pol)
        for k, v in pol.arrays().items():
            assert np.array_equal(back.arrays()[k], v), k
        assert (back.stack, back.deterministic, back.seed) == (1, True, 5)


# ---- hk_episode_stats: C, ctypes and C#
def test_episode_stats_layouts(tmp_path):
    names = [n for n, _ in _lib.EpisodeStats._fields_]
    src = tmp_path / "es.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu\\n", sizeof(hk_episode_stats));\n%s\nreturn 0;}\n'
                   % (os.path.join(ROOT, "include", "hk.h"), "\n".join('printf("%%zu\\n", offsetof(hk_episode_stats, %s));' % n for n in names)))
    exe = tmp_path / "es"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.EpisodeStats)] + [getattr(_lib.EpisodeStats, n).offset for n in names] == [104] + list(range(0, 104, 8))
    structs, imports = _parse_cs()
    assert structs["HkEpisodeStats"] == [(n, "long" if i < 7 else "double", False, 1) for i, n in enumerate(names)]
    assert {"hk_policy_pool_create", "hk_policy_pool_save", "hk_policy_pool_load", "hk_policy_pool_put", "hk_policy_pool_get", "hk_policy_pool_count",
            "hk_rollout_episode_stats"} <= set(imports)
