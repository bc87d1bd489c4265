"""The running normaliser's host twin (hierarchicalkarting_amd.ppo.normalizer_merge; include/hk.h "PPO trainer" NORMALISER): one batch
against ML-Agents' sequential form, against the direct moments, with zero-padded columns, and the host-side validation of a state."""
import numpy as np
import pytest

import normalizer_restate as NR
from hierarchicalkarting_amd.ppo import PPOTrainer, normalizer_merge, normalizer_published


def _rows(n=1001, k=37, seed=3):
    r = np.random.default_rng(seed)
    scale = 10.0 ** r.uniform(-1.0, 1.0, k)              # scales two orders of magnitude apart, as the observation's are
    X = (r.standard_normal((n, k)) * scale + r.uniform(-3.0, 3.0, k) * scale).astype(np.float32)
    X[:, 5] = 0.0                                          # a column that is zero padding in every row
    X[: n // 3, 11] = 0.0                                  # ... in a third of them
    return X


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("start", ["fresh", "running"])
def test_one_batch_equals_the_sequential_form(start):
    X = _rows()
    n, k = X.shape
    if start == "fresh":
        st = (1, np.zeros(k), np.ones(k))
    else:
        r = np.random.default_rng(9)
        st = (4321, r.standard_normal(k), r.uniform(0.5, 2.0, k) * 4321)
    N1, m1, M1 = normalizer_merge(*st, X)
    assert N1 == st[0] + n
    for nb in (1, 7, n):
        N, m, M = NR.sequential(*st, X, nb)
        assert N == N1
        print("%s, %d batches: relative difference mean %.3g m2 %.3g" % (start, nb, _rel(m1, m), _rel(M1, M)))
        assert _rel(m1, m) <= 1e-12 and _rel(M1, M) <= 1e-12, nb
    # ... and fed through the twin itself in 7 pieces
    s = st
    for B in np.array_split(X, 7):
        s = normalizer_merge(*s, B)
    assert s[0] == N1 and _rel(s[1], m1) <= 1e-12 and _rel(s[2], M1) <= 1e-12


def test_fresh_state_gives_the_moments_of_the_rows_plus_one_zero_sample():
    X = _rows()
    n, k = X.shape
    N1, m1, M1 = normalizer_merge(1, np.zeros(k), np.ones(k), X)
    Z = np.concatenate([np.zeros((1, k)), X.astype(np.float64)])
    mean = Z.mean(axis=0)
    ss = ((Z - mean) ** 2).sum(axis=0) + 1.0              # the population sum of squares about the mean, on top of the initial M2 = 1
    assert N1 == n + 1
    assert np.abs(m1 - mean).max() <= 1e-12 * np.abs(mean).max()
    assert np.abs(M1 - ss).max() <= 1e-12 * ss.max()
    # a zero-padded column: mean 0, M2 at its initial value, and its published std shrinks as 1 / sqrt(N)
    assert m1[5] == 0.0 and M1[5] == 1.0
    pm, ps = normalizer_published(N1, m1, M1)
    assert pm.dtype == np.float32 and ps.dtype == np.float32 and ps[5] == np.float32(np.sqrt(1.0 / N1))
    # a partly padded column counts its zeros
    assert abs(m1[11] - Z[:, 11].mean()) <= 1e-12 * abs(Z[:, 11].mean())


def test_no_rows_and_bad_rows():
    st = (3, np.arange(4.0), np.ones(4))
    N, m, M = normalizer_merge(*st, np.zeros((0, 4)))
    assert N == 3 and np.array_equal(m, st[1]) and np.array_equal(M, st[2])
    with pytest.raises(ValueError):
        normalizer_merge(*st, np.zeros((5, 3)))


class _Refuses:
    """the library must not be reached: normalizer_load validates on the host first"""
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def _trainer(in_dim):
    tr = PPOTrainer.__new__(PPOTrainer)
    tr.env = type("E", (), {"L": _Refuses(), "h": None})()
    tr.t = 0
    tr.actor_policy = type("P", (), {"in_dim": in_dim})()
    return tr


@pytest.mark.parametrize("steps,mean,m2", [
    (0, [0.0, 0.0], [1.0, 1.0]),                  # steps < 1
    (-3, [0.0, 0.0], [1.0, 1.0]),
    (1.5, [0.0, 0.0], [1.0, 1.0]),                # not an integer
    (1, [0.0, np.nan], [1.0, 1.0]),               # a non-finite mean
    (1, [np.inf, 0.0], [1.0, 1.0]),
    (1, [0.0, 0.0], [1.0, 0.0]),                  # m2 must be > 0
    (1, [0.0, 0.0], [-1.0, 1.0]),
    (1, [0.0, 0.0], [np.inf, 1.0]),
    (1, [0.0, 0.0], [np.nan, 1.0]),
    (1, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]),        # not [in_dim]
    (1, [0.0, 0.0], [1.0]),
])
def test_load_refuses_on_the_host(steps, mean, m2):
    with pytest.raises(ValueError):
        _trainer(2).normalizer_load(steps, mean, m2)
    if len(mean) != 3:                                # (the twin takes its in_dim from the state: three columns are a valid one)
        with pytest.raises(ValueError):
            normalizer_merge(steps, mean, m2, np.zeros((1, len(mean))))
