"""The oracle's game tally (hko_game_counts: the multi-player games every env solved, by player count) — the reference hk_prof_games is held to
on the GPU (tests/test_game_counts_gpu.py) — checked here against counts derived WITHOUT the C oracle: by hand from the geometry of a cluster field,
and from the independent Python restatement of SolveLQR (oracle/step_numpy.py Mirror.game_of) on the ticks of a natural race start.
One game per ego per solve tick; a solve with one player is not a game (hk.h hk_prof_games)."""
import numpy as np
import oracle_lib as O
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.config import make_config
from oracle import step_numpy as SN

NG = _lib.HK_MAX_AGENTS + 1


def cluster_field(b, o, whole=True):
    """the cluster field of tests/test_inwave_gpu.py: env mod 4 — 0: all four karts in one cluster, 1: three + one 30 m ahead, 2: two pairs 30 m
    apart, 3: the grid as reset left it.  whole: every moved kart starts from the record of a kart the grid placed in section 0, so that its
    checkpoint state matches where it now stands (test_inwave_gpu.py moves the grid's records as they are: a kart the jittered grid had put in
    section 1 is then behind its checkpoint and retired on the first tick — DroveReverseLimit, REC:475 — and the cluster holds fewer egos)"""
    st = o.agent_state().copy()
    s0 = b.track["sections"][0]
    for env in range(b.cfg.num_envs):
        kind = env % 4
        if kind == 3:
            continue
        if whole:
            first = [j for j in range(4) if st["section_index"][env, j] == 0]
            assert first, env
            st[env, :] = st[env, first[0]]
        for j in range(4):
            lane = j % 4 + 1
            far = (kind == 1 and j == 3) or (kind == 2 and j >= 2)
            st["px"][env, j] = s0["Lane%d" % lane]["x"]
            st["pz"][env, j] = s0["Lane%d" % lane]["z"] + 2.0 + (30.0 if far else 0.0) + 0.01 * (env % 7)
            st["lane"][env, j] = lane
    return st


def mirror_games(M, ags_env):
    """games[N] of one env's solve tick by the Python restatement: every active, enabled ego solves one game of len(players) players"""
    out = np.zeros(NG, np.int64)
    for ego in range(len(ags_env)):
        fl = int(ags_env[ego]["flags"])
        if (fl & _lib.HK_F_ACTIVE) and (fl & _lib.HK_F_ENABLED):
            n = len(M.game_of(ags_env, ego)["players"])
            if n >= 2:
                out[n] += 1
    return out


def test_tally_of_the_cluster_field_by_hand():
    E = 16
    b = make_config(E, 4, jitter_seed=21, laps=1, max_episode_steps=1200)
    o = O.OracleEnv(b)
    o.reset()
    o.set_agent_state(cluster_field(b, o))
    assert (o.game_counts() == 0).all()
    # step to the first solve tick that solves any game (the karts stand still through the start hold, so the geometry is the one set above)
    t = 0
    while o.game_counts().sum() == 0:
        before = o.agent_state().copy()
        o.step(1); t += 1
        assert t <= 8, "no multi-player game in the first two solve cadences"
    assert (o.env_state()["episode_steps"] % 4 == 0).all()
    want = {0: {4: 4}, 1: {3: 3}, 2: {2: 4}}       # kind -> {players: games}: four in one cluster, three + one alone (not a game), two pairs
    M = SN.Mirror(b)
    total = np.zeros(NG, np.int64)
    for env in range(E):
        got = o.game_counts(env, env + 1)
        assert got[0] == 0 and got[1] == 0, (env, got)
        kind = env % 4
        if kind == 3:
            exp = mirror_games(M, before[env])
            assert exp.sum() > 0, "the reset grid holds multi-player games"
        else:
            exp = np.zeros(NG, np.int64)
            for n, c in want[kind].items():
                exp[n] = c
            assert np.array_equal(exp, mirror_games(M, before[env])), (env, exp, mirror_games(M, before[env]))
        assert np.array_equal(got, exp), (env, kind, got.tolist(), exp.tolist())
        total += got
    # the range form sums the per-env rows; reset clears them; ticks off the cadence add nothing
    assert np.array_equal(o.game_counts(), total) and np.array_equal(o.game_counts(0, E), total)
    assert np.array_equal(o.game_counts(4, 8), o.game_counts(4, 5) + o.game_counts(5, 6) + o.game_counts(6, 7) + o.game_counts(7, 8))
    assert (o.game_counts(3, 3) == 0).all()
    o.step(3)
    assert np.array_equal(o.game_counts(), total)
    o.game_counts_reset()
    assert (o.game_counts() == 0).all()
    o.close()


def test_tally_of_natural_race_start_ticks_against_the_mirror():
    """a natural 4-agent Oval start (start hold, then the first corners): on each solve tick the tally's increase equals the mirror's players count
    of every ego, env by env; off-cadence ticks add nothing"""
    E = 8
    b = make_config(E, 4, jitter_seed=1592590336)
    o = O.OracleEnv(b)
    o.reset()
    M = SN.Mirror(b)
    checked, sizes = 0, set()
    for t in range(1, 321):
        before = o.agent_state().copy()
        c0 = np.stack([o.game_counts(env, env + 1) for env in range(E)])
        o.step(1)
        c1 = np.stack([o.game_counts(env, env + 1) for env in range(E)])
        steps = o.env_state()["episode_steps"]
        if t % 4 != 0:
            assert np.array_equal(c0, c1), t
            continue
        assert (steps == t).all()
        if t % 16 != 0 and t > 8:       # (the mirror is slow: every fourth solve tick past the first two)
            continue
        for env in range(E):
            exp = mirror_games(M, before[env])
            assert np.array_equal(c1[env] - c0[env], exp), (t, env, (c1[env] - c0[env]).tolist(), exp.tolist())
            sizes.update(int(n) for n in np.nonzero(exp)[0])
            checked += 1
    assert checked >= 8 * 20 and {2, 3} <= sizes, (checked, sizes)
    o.close()


def test_two_agent_tally_is_one_two_player_game_per_ego_per_tick():
    """2-agent handles solve every tick (cadence 1) and both egos hold the 2-player game whatever the distance (HKA:723)"""
    E = 4
    b = make_config(E, 2, jitter_seed=3)
    o = O.OracleEnv(b)
    o.reset()
    o.step(10)
    act = 2 * E * 10
    got = o.game_counts()
    assert got[2] == act and got.sum() == act, got
    o.close()
