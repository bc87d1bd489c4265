"""float64 restatement of the rollout recorder's log-probabilities (include/hk.h hk_rollout_field), shared by the CPU and GPU tests."""
import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def logp_cont(raw, mu, log_sigma):
    """log N(raw; mu, exp(log_sigma)) of the UNCLIPPED sample (ML-Agents GaussianDistInstance.log_prob without its epsilon)"""
    raw, mu = np.asarray(raw, np.float64), np.asarray(mu, np.float64)
    z = (raw - mu) / np.exp(np.float64(log_sigma))
    return -0.5 * z * z - np.float64(log_sigma) - HALF_LOG_2PI


def logp_disc(logits, branch):
    """log_softmax(logits)[branch] over the last axis"""
    lg = np.asarray(logits, np.float64)
    m = lg.max(axis=-1, keepdims=True)
    ls = lg - m - np.log(np.exp(lg - m).sum(axis=-1, keepdims=True))
    return np.take_along_axis(ls, np.asarray(branch)[..., None].astype(np.int64), axis=-1)[..., 0]
