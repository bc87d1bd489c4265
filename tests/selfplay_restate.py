"""Host twin of hk_rollout_episode_stats (include/hk.h "SELF-PLAY"): the per-(e, j) scan in numpy fp32, one rounding per operation, and the
cross-episode sums in float64.  Also returns the emitted episodes themselves, so that a test can bound the device's fp64 sums by their own
rounding."""
import math
import numpy as np

INT_FIELDS = ("episodes", "partial", "wins", "draws", "losses", "timeouts", "len_sum")
F32 = np.float32


def empty_carry(E, A):
    """the carry of [E][A]: ret, gret (fp32), len, whole (int32; whole 0: the episode in progress began before the chain)"""
    return dict(ret=np.zeros((E, A), F32), gret=np.zeros((E, A), F32), len=np.zeros((E, A), np.int32), whole=np.zeros((E, A), np.int32))


def episode_stats(ro, slots, rows=None, carry=None):
    """ro: dict of the rollout's fields (reward, group_reward, term_reward, term_group_reward [R, E, A]; done [R, E]); slots: the policy's agent
    slots; rows: completed rows (None: all); carry: the carry-in (None: no valid carry).
    -> (stats dict, carry-out, episodes): episodes = list of (ret fp32, gret fp32, len, done, f fp32) of the emitted, non-partial episodes in
    (e, j, t) order"""
    R = ro["done"].shape[0] if rows is None else int(rows)
    E, A = ro["reward"].shape[1:3]
    cout = empty_carry(E, A) if carry is None else {k: v.copy() for k, v in carry.items()}
    st = dict.fromkeys(INT_FIELDS, 0)
    eps = []
    for e in range(E):
        for a in slots:
            whole = int(carry["whole"][e, a]) if carry is not None else 0
            acc = F32(carry["ret"][e, a]) if whole else F32(0)
            gacc = F32(carry["gret"][e, a]) if whole else F32(0)
            ln = int(carry["len"][e, a]) if whole else 0
            for t in range(R):
                d = int(ro["done"][t, e])
                rw, gr = F32(ro["reward"][t, e, a]), F32(ro["group_reward"][t, e, a])
                if d == 0:
                    acc = F32(acc + rw); gacc = F32(gacc + gr); ln += 1
                    continue
                tr, tg = F32(ro["term_reward"][t, e, a]), F32(ro["term_group_reward"][t, e, a])
                acc = F32(acc + tr); gacc = F32(gacc + tg); ln += 1
                if not whole:
                    st["partial"] += 1
                else:
                    f = F32(tr + tg)
                    st["episodes"] += 1
                    st["len_sum"] += ln
                    st["wins" if f > 0 else ("losses" if f < 0 else "draws")] += 1
                    st["timeouts"] += int(d == 2)
                    eps.append((acc, gacc, ln, d, f))
                acc, gacc, ln, whole = rw, gr, 0, 1
            cout["ret"][e, a], cout["gret"][e, a], cout["len"][e, a], cout["whole"][e, a] = acc, gacc, ln, whole
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.array([x[0] for x in eps], np.float64)
        g = np.array([x[1] for x in eps], np.float64)
        # the correctly rounded float64 sums (math.fsum) where every value is finite: any n-term fp64 summation lies within (n - 1) 2^-53 sum |x|
        # of the exact sum, so within n 2^-53 sum |x| of these
        tot = (lambda v: math.fsum(v)) if np.isfinite(r).all() and np.isfinite(g).all() else (lambda v: float(np.sum(v)))
        st.update(ret_sum=tot(r), ret_sumsq=tot(r * r), gret_sum=tot(g), gret_sumsq=tot(g * g))
        mn, mx = np.inf, -np.inf
        for v in r:             # the device's comparisons: a NaN never replaces the running value
            mn = v if v < mn else mn
            mx = v if v > mx else mx
        st.update(ret_min=float(mn), ret_max=float(mx))
    return st, cout, eps


def sum_bounds(eps):
    """-> dict: the bound n 2^-53 sum |x| on each of the four fp64 sums (any summation order of n terms is within it of any other)"""
    r = np.array([x[0] for x in eps], np.float64)
    g = np.array([x[1] for x in eps], np.float64)
    n, u = len(eps), 2.0 ** -53
    return dict(ret_sum=n * u * np.abs(r).sum(), ret_sumsq=n * u * (r * r).sum(), gret_sum=n * u * np.abs(g).sum(), gret_sumsq=n * u * (g * g).sum())
