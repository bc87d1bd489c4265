"""Float64 restatement of the three product forms of the PPO trainer's bf16 mode (include/hk.h "PRECISION", hk_ppo_gemm_bf16) with the
error bound they are held to, and the per-block gradient comparison of the two precisions.

The bound: a bf16 x bf16 product is exact in fp32 (8 + 8 significand bits), so only the K additions of the fp32 accumulation round, and
|C - ref| <= gamma_K sum |a| |b| with gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability, section 3.1), for any order of the
additions — the split into chunks and their combine included, since no term passes through more than K additions.  The tests assert twice that.
A Swish epilogue is applied to the accumulated value: its Lipschitz constant is at most 1.1 (max |swish'| = 1.0998), and its own fp32
evaluation is allowed one fp32 ulp of the result."""
import numpy as np

from hierarchicalkarting_amd.ppo import bf16_round, bf16_value

U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def swish(x):
    return x / (1.0 + np.exp(-x))


def dswish(x):
    sg = 1.0 / (1.0 + np.exp(-x))
    return sg + x * sg * (1.0 - sg)


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def random_bf16(rng, shape):
    """random fp32 values rounded to bf16 on the host -> uint16 bit patterns"""
    return bf16_round(rng.standard_normal(shape).astype(np.float32))


def product(epi, A, B, bias=None, aux=None):
    """-> (reference, tolerance), float64 [M, N], of hk_ppo_gemm_bf16's epi on the bf16 bit patterns A, B"""
    a, b = bf16_value(A).astype(np.float64), bf16_value(B).astype(np.float64)
    if epi == 0:                      # weight gradient: A [K, M], B [K, N]
        K = a.shape[0]
        return a.T @ b, 2.0 * gamma(K) * (np.abs(a).T @ np.abs(b))
    if epi == 1:                      # forward: A [M, K], B [N, K]
        K = a.shape[1]
        acc = a @ b.T + (0.0 if bias is None else np.asarray(bias, np.float64)[None, :])
        ref = swish(acc)
        return ref, 1.1 * 2.0 * gamma(K) * (np.abs(a) @ np.abs(b).T) + ulp32(ref)
    K = a.shape[1]                    # backward delta: A [M, K], B [K, N]
    ref = (a @ b) * dswish(np.asarray(aux, np.float64))
    return ref, 1.1 * 2.0 * gamma(K) * (np.abs(a) @ np.abs(b)) + ulp32(ref)


def block_differences(got, want):
    """per parameter block: (relative L2 difference, cosine) of two dicts name -> array"""
    out = {}
    for k in want:
        g, w = got[k].astype(np.float64).ravel(), want[k].astype(np.float64).ravel()
        nw, ng = np.linalg.norm(w), np.linalg.norm(g)
        out[k] = (np.linalg.norm(g - w) / max(nw, 1e-300), float(g @ w) / max(ng * nw, 1e-300))
    return out
