// hk_policy_lstm.h — recurrent actors: the ML-Agents NetworkBody with `memory` (contract in include/hk.h "RECURRENT ACTORS").
//   normalise -> n x (Linear + Swish) = a[H] -> one LSTM cell on (a, h, c) -> heads on h' (width m = memory_size / 2)
// Two parts.  The first is plain C (HK_HD): the sigmoid, the tanh and the cell, ONE definition each, shared by policy_lstm_kernel and by
// the host build of tests/policy_lstm_host_check.cpp, which is the bit reference of the GPU tests.  The second (hipcc only) is the kernel
// and the kernel that clears / records the memory.
//
// policy_lstm_kernel is policy_mlp_kernel's trunk (same tile of 64 rows, 8 waves, At transposed in LDS, pm_gemm, its MODE 2 form for every
// hidden size) followed by the cell.  A wave takes one (row block of 32, block of 32 hidden units) and holds FOUR accumulators, the
// i / f / g / o columns of those units: 2 x m / 32 <= 8 tasks, one per wave at m = 128.  The accumulators are seeded with b_ih + b_hh
// (summed once at attach) and stepped over a[0 .. H) from At and then over h[0 .. m) from Ht, the row's hidden state staged transposed
// beside At — one k-ascending fmaf chain per gate pre-activation, as the trunk's.  The four gates of a unit meet in one lane's registers,
// so the cell is an epilogue on the C/D layout: c is read and c' written straight from / to the memory buffer (32 consecutive units per
// half-wave: 128-byte rows), h' goes to the memory buffer and over Ht for the heads (pm_tail with width m).  The memory [rows][2m] =
// [h | c] is updated in place: a row reads its own entry (h by the loader, c by the epilogue) and then writes it; no other row touches it.
// LDS: (max(kc, H) + m) x 65 floats + the heads' 2 KB — 91 488 bytes at 216 -> 128 x 3 -> m = 128, 101 888 at H = 256: one workgroup per CU,
// hence __launch_bounds__(512, 2) and the 256-register budget (resource row: DESIGN §16).
#pragma once
#include "../../include/hk_detmath.h"

/* 1 / (1 + exp(-z)) on hk_expf_fast_core, as hk_swishf's factor.  The exp argument -z is held inside the core's range [-87, 88]; from
 * z <= -88 on (true value < 6.1e-39) the result is exactly 0, so -Inf gives 0 and +Inf gives 1 / (1 + 1.6e-38) == 1; a NaN stays a NaN. */
HK_HD float hk_sigmoidf(float z)
{
    const float x0 = -z;
    const float x = x0 < -87.0f ? -87.0f : (x0 < 88.0f ? x0 : 88.0f);      /* (a NaN lands on 88: the core's int cast needs a finite value) */
    float r = 1.0f / (1.0f + hk_expf_fast_core(x));
    r = x0 < 88.0f ? r : 0.0f;
    return z == z ? r : z;
}

/* tanh(z) = sign(z) (1 - t) / (1 + t), t = exp(-2 |z|) on hk_expf_fast_core; t = 1.6e-38 from |z| >= 43.5 on, so the result is exactly
 * +-1 there and at +-Inf; a NaN stays a NaN.  (1 - t is exact near 0 — Sterbenz — so the absolute error near 0 is t's, ~6e-8.) */
HK_HD float hk_tanhf_fast(float z)
{
    const float a = z < 0.0f ? -z : z;
    const float x0 = -2.0f * a;
    const float x = x0 > -87.0f ? x0 : -87.0f;                              /* (a NaN lands on -87) */
    const float t = hk_expf_fast_core(x);
    const float r = (1.0f - t) / (1.0f + t);
    return z == z ? (z < 0.0f ? -r : r) : z;
}

/* The cell on the four gate pre-activations of one unit (torch's order i, f, g, o) and its cell state c:
 * c' = fmaf(f, c, i g~), h' = o tanh(c').  Every fused step is written as one: contraction can add none and take none away. */
HK_HD void hk_lstm_cell(float zi, float zf, float zg, float zo, float c, float* h_new, float* c_new)
{
    const float i = hk_sigmoidf(zi), f = hk_sigmoidf(zf), g = hk_tanhf_fast(zg), o = hk_sigmoidf(zo);
    const float ig = i * g;
    const float cn = __builtin_fmaf(f, c, ig);
    *c_new = cn;
    *h_new = o * hk_tanhf_fast(cn);
}

#if defined(__HIPCC__)
#include "hk_policy.h"

namespace hk {

inline size_t policy_lstm_lds_bytes(const PolicyParams& q, const PolicyLstm& l)
{
    const int kmax = q.kc > q.hidden ? q.kc : q.hidden;
    return ((size_t)(kmax + l.m) * PM_LD + (size_t)PM_MAX_OUT * PM_TILE) * sizeof(float);
}

// The first decision of an episode starts from zero memory: the `stale` test of policy_stack_kernel (pm_episode_word) on the epoch word that
// kernel rewrites — so this one is issued BEFORE it, and FIRST == 1 if and only if the memory read is zero.  One wave per (env, slot).
// rec_mem (an open rollout's MEMORY row, [E][A][mem_max]; nullptr: not recording): the memory the decision reads, after the clear.
#ifdef HK_POLICY_KERNELS      // (hk_policy.h: the kernels, in the one unit that defines them)
__global__ __launch_bounds__(256) void policy_memory_kernel(PolicyParams Q, PolicyLstm L, int E, int A, const hk_env_state* envs_by_slot, const int* slot_of,
                                                            float* rec_mem, int mem_max)
{
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = threadIdx.x & 63;
    if (pair >= E * Q.n_slots) return;                         // (wave-uniform)
    const int env = pair / Q.n_slots, j = pair % Q.n_slots;
    const hk_env_state* es = &envs_by_slot[slot_of[env]];
    const bool stale = Q.epoch[pair] != pm_episode_word(*es);
    float* mem = L.mem + (size_t)pair * 2 * L.m;
    float* rec = rec_mem ? rec_mem + ((size_t)env * A + Q.slots[j]) * mem_max : nullptr;
    for (int k = t; k < 2 * L.m; k += 64) {
        float v = 0.0f;
        if (stale) mem[k] = 0.0f; else v = mem[k];
        if (rec) rec[k] = v;
    }
}

// hk_policy_memory_set: the memory just written belongs to the episode each env is in NOW — the epoch word is made current, so the next decision
// keeps it (and the observation stack) unless the episode changes first
__global__ __launch_bounds__(256) void policy_epoch_current_kernel(PolicyParams Q, int E, const hk_env_state* envs_by_slot, const int* slot_of)
{
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= E * Q.n_slots) return;
    const hk_env_state* es = &envs_by_slot[slot_of[pair / Q.n_slots]];
    Q.epoch[pair] = pm_episode_word(*es);
}

// hk_rollout_close: NEXT_MEMORY [E][A][mem_max] = the memory after the last completed row, zero where that row's interval ended an episode
// (done_last: DONE of that row, [E]; nullptr: no row completed)
__global__ __launch_bounds__(256) void rollout_next_memory_kernel(PolicyParams Q, PolicyLstm L, int E, int A, const int* done_last, float* next_mem, int mem_max)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)2 * L.m;
    if (idx >= (size_t)E * Q.n_slots * per) return;
    const size_t pair = idx / per;
    const int k = (int)(idx % per), env = (int)(pair / Q.n_slots), j = (int)(pair % Q.n_slots);
    const bool ended = done_last && done_last[env] != 0;
    next_mem[((size_t)env * A + Q.slots[j]) * mem_max + k] = ended ? 0.0f : L.mem[idx];
}

// One wave's share of the gate products over K inputs (a multiple of 32): z[g] += A[32 rows][K] * B_g[K][32 units], g = i, f, g, o, as MFMA
// 32x32x2 f32 steps in ascending k.  ap: this lane's first element of A (LDS, row stride PM_LD per k); qp: this lane's float4 of gate i in the
// group-major weight copy (PolicyLstm::Wq_*: 2 * 4m float4 per group of 8 inputs), gate g another g * m float4 on.  The B loads run three
// groups ahead (four register sets), the A reads one group ahead, as in pm_gemm; a group is 16 MFMAs on four independent accumulators.
__device__ __forceinline__ void pl_gemm4(f32x16 (&z)[4], const float* ap, const float4* __restrict__ qp, int m, int K)
{
    const int ng = K >> 3;                               // a multiple of 4
    const size_t qs = (size_t)8 * m;                     // float4 per group
    auto ldB = [&](int g, float4 (&x)[4]) {
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] = qp[(size_t)g * qs + (size_t)q * m];
    };
    auto ldA = [&](int g, float (&x)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = ap[(size_t)(8 * g + 2 * j) * PM_LD];
    };
    auto mm = [&](const float4 (&y)[4], const float (&x)[4]) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            z[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[0], y[q].x, z[q], 0, 0, 0);
            z[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[1], y[q].y, z[q], 0, 0, 0);
            z[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[2], y[q].z, z[q], 0, 0, 0);
            z[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[3], y[q].w, z[q], 0, 0, 0);
        }
    };
    float4 Ba[4], Bb[4], Bc[4], Bd[4];
    float Ap[4], Aq[4];
    ldB(0, Ba); ldB(1, Bb); ldB(2, Bc);
    ldA(0, Ap);
    for (int g = 0; g < ng; g += 4) {
        ldB(g + 3, Bd);
        ldA(g + 1, Aq);
        mm(Ba, Ap);
        if (g + 4 < ng) ldB(g + 4, Ba);
        ldA(g + 2, Ap);
        mm(Bb, Aq);
        if (g + 5 < ng) ldB(g + 5, Bb);
        ldA(g + 3, Aq);
        mm(Bc, Ap);
        if (g + 6 < ng) ldB(g + 6, Bc);
        if (g + 4 < ng) ldA(g + 4, Ap);
        mm(Bd, Aq);
    }
}

// Arguments as policy_mlp_kernel's, plus L (the cell's weights) and mem [rows][2m], read and rewritten in place (the policy's own buffer in
// hk_step, a staging copy in hk_policy_forward_mem).  The trunk below is policy_mlp_kernel<2>'s text (the per-wave mixed form serves every
// hidden size here: at one workgroup per CU the register budget that made MODE 0 / 1 worth having is not binding).  A trunk function shared
// with that kernel was measured: this kernel came out 1.3 - 1.7 % slower per launch, so it keeps its copy; change both together.
__global__ __launch_bounds__(PM_THREADS, 2) void policy_lstm_kernel(PolicyParams Q, PolicyLstm L, float* mem, int rows, const float* src, int w,
                                                                     unsigned long long decision, int env_id_base, int A,
                                                                     float* mu_out, float* logit_out, float* act_steer, int* act_branch, PolicyRec rec)
{
    extern __shared__ __align__(16) float At[];        // [max(kc, hidden)][PM_LD], Ht[m][PM_LD], head[PM_MAX_OUT][PM_TILE]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PM_TILE;
    const int K0 = Q.in_dim, H = Q.hidden, KC = Q.kc, m = L.m;
    float* Ht = At + (size_t)(KC > H ? KC : H) * PM_LD;
    float* head = Ht + (size_t)m * PM_LD;

    // ---- h of the tile's rows, transposed: lanes over units (coalesced reads, conflict-free column writes), waves over rows
    for (int r = wave; r < PM_TILE; r += PM_THREADS / 64) {
        const bool rowok = row0 + r < rows;
        const float* mrow = mem + (size_t)(row0 + r) * 2 * m;
        for (int k = lane; k < m; k += 64) Ht[(size_t)k * PM_LD + r] = rowok ? mrow[k] : 0.0f;
    }

    const int ncb = H >> 5;
    const int nunits = ncb * 2;
    const int half = lane >> 5, c = lane & 31;
    const int u0 = wave, u1 = wave + 8;
    const bool has0 = u0 < nunits, has1 = u1 < nunits;
    const int cb0 = u0 % ncb, rb0 = u0 / ncb;
    const int cb1 = has1 ? u1 % ncb : cb0, rb1 = has1 ? u1 / ncb : rb0;
    const float* a0p = At + (size_t)half * PM_LD + rb0 * 32 + c;
    const float* a1p = At + (size_t)half * PM_LD + rb1 * 32 + c;

    for (int l = 0; l < Q.n_layers; l++) {
        const int K = l == 0 ? K0 : H;
        f32x16 acc0, acc1;
        {
            const float bias0 = has0 ? Q.b[l][cb0 * 32 + c] : 0.0f;
            const float bias1 = has1 ? Q.b[l][cb1 * 32 + c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) { acc0[r] = bias0; acc1[r] = bias1; }
        }
        for (int kb = 0; kb < K; kb += KC) {
            const int kc = (K - kb) < KC ? (K - kb) : KC;
            if (l == 0) {
                if (kb > 0) __syncthreads();                      // the previous chunk has been consumed
                constexpr int MMAX = (PM_KC_MAX + 63) / 64;
                int soff[MMAX];
                float mean[MMAX], sdev[MMAX];
#pragma unroll
                for (int mm = 0; mm < MMAX; mm++) {
                    const int kl = lane + 64 * mm, k = kb + kl;
                    soff[mm] = -1; mean[mm] = 0.0f; sdev[mm] = 1.0f;
                    if (kl < kc) {
                        soff[mm] = pm_ring_offset(Q, w, k);
                        if (Q.normalize) { mean[mm] = Q.mean[k]; sdev[mm] = Q.std[k]; }
                    }
                }
                for (int r = wave; r < PM_TILE; r += PM_THREADS / 64) {
                    const bool rowok = row0 + r < rows;
                    const float* srow = src + (size_t)(row0 + r) * K0;
                    float v[MMAX];
#pragma unroll
                    for (int mm = 0; mm < MMAX; mm++) v[mm] = (rowok && soff[mm] >= 0) ? srow[soff[mm]] : 0.0f;
#pragma unroll
                    for (int mm = 0; mm < MMAX; mm++) {
                        if (soff[mm] < 0) continue;
                        float x = v[mm];
                        if (Q.normalize && rowok) x = pm_normalise(x, mean[mm], sdev[mm]);
                        At[(size_t)(lane + 64 * mm) * PM_LD + r] = x;
                    }
                }
                __syncthreads();
            }
            if (has0) {
                const float* __restrict__ Wt = Q.Wt[l] + (size_t)kb * H;
                const float* b0p = Wt + (size_t)half * H + cb0 * 32 + c;
                const float* b1p = Wt + (size_t)half * H + cb1 * 32 + c;
                const float4* __restrict__ Wq = Q.Wq[l] + (size_t)(kb >> 3) * 2 * H;
                const float4* q0p = Wq + (size_t)half * H + cb0 * 32 + c;
                const float4* q1p = Wq + (size_t)half * H + cb1 * 32 + c;
                if (!has1) pm_gemm<false, false>(acc0, acc1, a0p, a1p, b0p, b1p, q0p, q1p, kc, H);
                else if (cb1 == cb0) pm_gemm<true, true>(acc0, acc1, a0p, a1p, b0p, b1p, q0p, q1p, kc, H);
                else pm_gemm<true, false>(acc0, acc1, a0p, a1p, b0p, b1p, q0p, q1p, kc, H);
            }
        }
        if (has0) {
#pragma unroll
            for (int r = 0; r < 16; r++) { acc0[r] = swish(acc0[r]); if (has1) acc1[r] = swish(acc1[r]); }
        }
        __syncthreads();            // every wave has finished reading this layer's input
        if (has0) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = (r & 3) + 8 * (r >> 2) + 4 * half;
                At[(size_t)(cb0 * 32 + c) * PM_LD + rb0 * 32 + rr] = acc0[r];
                if (has1) At[(size_t)(cb1 * 32 + c) * PM_LD + rb1 * 32 + rr] = acc1[r];
            }
        }
        __syncthreads();
    }

    // ---- the cell: wave -> (row block rbc, unit block ub); the gate columns of unit u are g * m + u of the 4m
    const int nub = m >> 5;
    const bool hasc = wave < 2 * nub;
    const int ub = hasc ? wave % nub : 0, rbc = hasc ? wave / nub : 0;
    const int unit = ub * 32 + c;
    f32x16 z[4];
    if (hasc) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float bias = L.b[q * m + unit];
#pragma unroll
            for (int r = 0; r < 16; r++) z[q][r] = bias;
        }
        pl_gemm4(z, At + (size_t)half * PM_LD + rbc * 32 + c, L.Wq_ih + (size_t)half * 4 * m + unit, m, H);
        pl_gemm4(z, Ht + (size_t)half * PM_LD + rbc * 32 + c, L.Wq_hh + (size_t)half * 4 * m + unit, m, m);
    }
    __syncthreads();                // every wave has finished reading h
    if (hasc) {
        // C/D layout: col (unit) = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        float cc[16];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = rbc * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            cc[r] = row0 + row < rows ? mem[(size_t)(row0 + row) * 2 * m + m + unit] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = rbc * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float hn, cn;
            hk_lstm_cell(z[0][r], z[1][r], z[2][r], z[3][r], cc[r], &hn, &cn);
            Ht[(size_t)unit * PM_LD + row] = hn;
            if (row0 + row < rows) {
                float* mrow = mem + (size_t)(row0 + row) * 2 * m;
                mrow[unit] = hn;
                mrow[m + unit] = cn;
            }
        }
    }
    __syncthreads();
    pm_tail(Q, Ht, head, rows, row0, decision, env_id_base, A, mu_out, logit_out, act_steer, act_branch, rec, tid, m);
}
#endif  /* HK_POLICY_KERNELS */

// ---------------------------------------------------------------------------------------------------------------------
inline int policy_lstm_validate(const hk_policy_lstm_desc* l, std::string& err)
{
    if (l->reserved != 0) { err = "hk_policy_attach_lstm: reserved != 0"; return HK_ERR_INVALID; }
    if (l->memory_size & 1) { err = "hk_policy_attach_lstm: memory_size is odd (it holds h and c, m = memory_size / 2 each)"; return HK_ERR_INVALID; }
    const int m = l->memory_size / 2;
    if (m < 32 || m > HK_POLICY_MAX_MEMORY / 2 || m % 32) { err = "hk_policy_attach_lstm: memory_size: m = memory_size / 2 must be a multiple of 32 in [32, 128]"; return HK_ERR_INVALID; }
    if (!l->W_ih || !l->W_hh || !l->b_ih || !l->b_hh) { err = "hk_policy_attach_lstm: NULL W_ih / W_hh / b_ih / b_hh"; return HK_ERR_INVALID; }
    return HK_OK;
}

// the cell's weights re-laid for pl_gemm4 (torch layout in: W [4m][K], gates i f g o), the summed bias, and the zeroed memory [E][n_slots][2m]
// (E == 0: none); pd.q is already uploaded (policy_upload with head_width = m)
inline int policy_lstm_upload(PolicyDevice& pd, const hk_policy_lstm_desc* l, int E, hipStream_t stream, std::string& err)
{
    const int m = l->memory_size / 2, N = 4 * m, H = pd.q.hidden;
    std::vector<float> host;
    auto lay = [&](const float* W, int K) {              // -> offset of W [N][K] in the group-major form (pm_wq_fill)
        const size_t off = host.size();
        host.resize(off + (size_t)K * N);
        pm_wq_fill(host.data() + off, W, N, K);
        return off;
    };
    const size_t o_ih = lay(l->W_ih, H), o_hh = lay(l->W_hh, m), o_b = host.size();
    for (int k = 0; k < N; k++) host.push_back(l->b_ih[k] + l->b_hh[k]);
    const size_t o_raw = host.size();                    // the two biases themselves, for hk_ppo_create_recurrent's master copy
    host.insert(host.end(), l->b_ih, l->b_ih + N);
    host.insert(host.end(), l->b_hh, l->b_hh + N);
    hipError_t e;
    if ((e = hipMalloc(&pd.wlstm, host.size() * sizeof(float))) != hipSuccess ||
        (e = hipMemcpyAsync(pd.wlstm, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess) {
        err = std::string("hk_policy_attach_lstm: ") + hipGetErrorString(e);
        return HK_ERR_HIP;
    }
    PolicyLstm& q = pd.lq;
    q.m = m;
    q.Wq_ih = reinterpret_cast<const float4*>(pd.wlstm + o_ih);      // (hipMalloc's base and K * N floats: 16-byte aligned)
    q.Wq_hh = reinterpret_cast<const float4*>(pd.wlstm + o_hh);
    q.b = pd.wlstm + o_b;
    pd.braw = pd.wlstm + o_raw;
    q.mem = nullptr;
    if (E > 0) {
        const size_t bytes = (size_t)E * pd.q.n_slots * 2 * m * sizeof(float);
        if ((e = hipMalloc(&q.mem, bytes)) != hipSuccess || (e = hipMemsetAsync(q.mem, 0, bytes, stream)) != hipSuccess) {
            err = std::string("hk_policy_attach_lstm: ") + hipGetErrorString(e);
            return HK_ERR_HIP;
        }
    }
    return HK_OK;
}

}  // namespace hk
#endif  /* __HIPCC__ */
