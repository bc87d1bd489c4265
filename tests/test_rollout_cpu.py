"""Host helpers of the rollout recorder (hierarchicalkarting_amd/rollout.py) and the log-probability restatement the GPU tests use,
against direct simulations and closed forms.  No GPU."""
import numpy as np
import pytest
from hierarchicalkarting_amd.rollout import stacked_inputs, transition_rewards
from rollout_restate import logp_cont, logp_disc, HALF_LOG_2PI


def _ring_sim(rng, E, A, slots, stack, smax, R, D, pre):
    """policy_stack_kernel's ring (slot w = decision % stack gets the newest slice, cleared when stale) run over `pre` decisions, then
    RING0 as rollout_ring0_kernel snapshots it, then R recorded decisions: -> (ro, the inputs the actor saw [R][E][S][stack * D])"""
    ring = np.zeros((E, len(slots), stack, D), np.float32)
    ro = {"obs": np.zeros((R, E, A, D), np.float32), "first": np.zeros((R, E, A), np.int32),
          "ring0": np.zeros((E, A, smax - 1, D), np.float32)}
    want = np.zeros((R, E, len(slots), stack * D), np.float32)
    for d in range(pre + R):
        w = d % stack
        if d == pre:
            for i in range(stack - 1):
                ro["ring0"][:, slots, smax - stack + i] = ring[:, :, (w + 1 + i) % stack]
        stale = rng.random((E, len(slots))) < 0.2
        ring[stale] = 0.0
        o = rng.standard_normal((E, len(slots), D)).astype(np.float32)
        ring[:, :, w] = o
        if d >= pre:
            t = d - pre
            ro["obs"][t][:, slots] = o
            ro["first"][t][:, slots] = stale
            order = [(w + 1 + i) % stack for i in range(stack)]
            want[t] = ring[:, :, order].reshape(E, len(slots), stack * D)
    return ro, want


@pytest.mark.parametrize("stack,smax,pre", [(4, 4, 0), (4, 4, 9), (2, 4, 5), (1, 3, 3), (7, 8, 13), (3, 3, 2)])
def test_stacked_inputs_rebuild_the_ring(stack, smax, pre):
    rng = np.random.default_rng(stack * 100 + smax * 10 + pre)
    E, A, D, R = 5, 4, 6, 23
    slots = [1, 3]
    ro, want = _ring_sim(rng, E, A, slots, stack, smax, R, D, pre)
    got = stacked_inputs(ro, slots, stack)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


def test_stacked_inputs_rejects_a_stack_ring0_cannot_hold():
    ro = {"obs": np.zeros((2, 1, 1, 3), np.float32), "first": np.zeros((2, 1, 1), np.int32), "ring0": np.zeros((1, 1, 1, 3), np.float32)}
    with pytest.raises(ValueError):
        stacked_inputs(ro, [0], 3)


def test_transition_rewards_and_the_accounting_identity():
    rng = np.random.default_rng(1)
    R, E, A = 40, 7, 4
    done = (rng.random((R, E)) < 0.2).astype(np.int32) * rng.integers(1, 3, (R, E)).astype(np.int32)
    term = rng.standard_normal((R, E, A)).astype(np.float32) * (done[:, :, None] != 0)
    reward = rng.standard_normal((R, E, A)).astype(np.float32)
    ro = {"done": done, "term_reward": term, "reward": reward}
    tr = transition_rewards(ro)
    assert np.array_equal(tr[done != 0], term[done != 0])
    assert np.array_equal(tr[done == 0], reward[done == 0])
    # every AddReward of the interval: the terminal part and what followed the reset
    assert np.allclose((tr + reward * (done[:, :, None] != 0)).sum(), (term + reward).sum(), rtol=1e-5)


def test_logp_restatement_against_closed_forms():
    # the density at the mean, and one sigma out
    for ls in (-2.0, -0.5, 0.0, 0.7):
        s = np.exp(ls)
        assert np.isclose(logp_cont(1.25, 1.25, ls), -ls - HALF_LOG_2PI, rtol=1e-15)
        assert np.isclose(logp_cont(1.25 + s, 1.25, ls), -0.5 - ls - HALF_LOG_2PI, rtol=1e-14)
        # it is a density: integrates to 1
        x = np.linspace(-12 * s, 12 * s, 200001)
        y = np.exp(logp_cont(x, 0.0, ls))
        assert np.isclose(((y[1:] + y[:-1]) * np.diff(x)).sum() / 2, 1.0, rtol=1e-8)
    # categorical: uniform logits, a probability vector, shift invariance
    assert np.allclose(logp_disc(np.zeros((4, 3)), np.array([0, 1, 2, 1])), -np.log(3.0))
    lg = np.random.default_rng(2).standard_normal((50, 3)) * 4
    lp = np.stack([logp_disc(lg, np.full(50, b)) for b in range(3)], axis=1)
    assert np.allclose(np.exp(lp).sum(axis=1), 1.0, rtol=1e-13)
    assert np.allclose(logp_disc(lg + 100.0, np.zeros(50, int)), lp[:, 0], rtol=1e-12)
    p = np.exp(lg[:, 1]) / np.exp(lg).sum(axis=1)
    assert np.allclose(lp[:, 1], np.log(p), rtol=1e-12)
