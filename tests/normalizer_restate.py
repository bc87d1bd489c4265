"""Float64 restatement of the running normaliser (include/hk.h "PPO trainer" NORMALISER) for the tests: ML-Agents' update in its sequential,
batch-by-batch form, the reference of one device update with the bounds the accumulation allows, and the comparison itself."""
import numpy as np

U = 2.0 ** -53          # unit roundoff of fp64


def sequential(steps, mean, m2, X, n_batches):
    """ML-Agents' normaliser fed the rows X [n, in_dim] in n_batches successive batches (float64), written batch by batch:
        steps' = steps + b;  mean' = mean + sum(x - mean) / steps';  m2' = m2 + sum((x - mean') (x - mean))"""
    steps, mean, m2 = int(steps), np.array(mean, np.float64), np.array(m2, np.float64)
    for B in np.array_split(np.asarray(X, np.float64), n_batches):
        if B.shape[0] == 0:
            continue
        new_steps = steps + B.shape[0]
        delta = B - mean
        new_mean = mean + delta.sum(axis=0) / new_steps
        m2 = m2 + ((B - new_mean) * delta).sum(axis=0)
        mean, steps = new_mean, new_steps
    return steps, mean, m2


def reference(steps, mean, m2, X):
    """one update of the state by the rows X in float64 numpy -> (steps', mean', m2', bound on |mean' error|, bound on |m2' error|).
    The bounds are those of an fp64 accumulation over n terms plus the final operations, u = 2^-53, with c = x - mean:
        |m' error|  <= 4 n u sum|c| / N' + 2 u |m'|
        |M2' error| <= 4 n u (sum c^2 + delta^2 / N') + 2 u M2'"""
    mean, m2, X = np.asarray(mean, np.float64), np.asarray(m2, np.float64), np.asarray(X, np.float64)
    n = X.shape[0]
    N1 = int(steps) + n
    c = X - mean
    delta = c.sum(axis=0)
    mean1 = mean + delta / N1
    m21 = m2 + ((X - mean1) * c).sum(axis=0)
    b_mean = 4.0 * n * U * np.abs(c).sum(axis=0) / N1 + 2.0 * U * np.abs(mean1)
    b_m2 = 4.0 * n * U * ((c * c).sum(axis=0) + delta * delta / N1) + 2.0 * U * m21
    return N1, mean1, m21, b_mean, b_m2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_published(tr, what=""):
    """the policy's fp32 statistics are the trainer's fp64 state rounded as hk.h states, bit for bit -> (steps, mean, m2, norm_mean, norm_std)"""
    steps, mean, m2 = tr.normalizer_state()
    pm, ps = tr.read("norm_mean"), tr.read("norm_std")
    assert np.array_equal(bits(pm), bits(np.float32(mean))), what + ": published mean"
    assert np.array_equal(bits(ps), bits(np.float32(np.sqrt(m2 / np.float64(steps))))), what + ": published std"
    return steps, mean, m2, pm, ps


def assert_update(tr, before, X, what=""):
    """the trainer's state after ONE update from `before` = (steps, mean, m2) by the rows X, against reference(); prints the figures first"""
    N1, mean1, m21, b_mean, b_m2 = reference(*before, X)
    steps, mean, m2, pm, ps = assert_published(tr, what)
    e_mean, e_m2 = np.abs(mean - mean1), np.abs(m2 - m21)
    print("%s: n %d, steps %d -> %d; worst |mean error| / bound %.3g, worst |m2 error| / bound %.3g" % (
        what, X.shape[0], before[0], steps, (e_mean / b_mean).max(), (e_m2 / b_m2).max()))
    assert steps == N1, (what, steps, N1)
    assert (e_mean <= b_mean).all(), (what, "mean", int(np.argmax(e_mean / b_mean)), (e_mean / b_mean).max())
    assert (e_m2 <= b_m2).all(), (what, "m2", int(np.argmax(e_m2 / b_m2)), (e_m2 / b_m2).max())
    return steps, mean, m2
