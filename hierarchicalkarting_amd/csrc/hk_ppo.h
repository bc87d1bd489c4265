// hk_ppo.h — device side of the PPO trainer (contract in include/hk.h "PPO trainer", host side in hk_train.hip).
// Per minibatch of m rows (ids into the rollout's n = R * E * S rows):
//   ppo_gather_kernel       the stacked input of every row rebuilt from OBS / FIRST / RING0 (NEXT_OBS for the bootstrap rows), normalised
//                           and clipped exactly as policy_mlp_kernel's loader does: X0 [m][in_dim] (a workspace sized by the minibatch)
//   ppo_gemm_kernel<EPI>    every matrix product, on v_mfma_f32_32x32x2_f32: the trunk forward (seeded with the bias, k ascending: the
//                           bits of policy_mlp_kernel), the backward delta (delta W) * swish', and the weight gradients (delta^T a, K = rows,
//                           split into fixed chunks of PPO_KCH rows whose partial tiles ppo_combine_kernel sums in chunk order)
//   ppo_loss_kernel         the heads as fmaf chains (the bits of policy_mlp_kernel's heads), the log-probabilities as the recorder writes
//                           them, the clipped losses and their per-row gradients; one thread per row
//   ppo_colsum_kernel       bias / log_sigma gradients and the stats: fixed-order column sums (no float atomics anywhere)
//   ppo_gae_kernel          one lane per (env, slot): the reverse GAE scan;  ppo_adv_norm_kernel: fp64 mean / std in one block
//   ppo_adam_kernel, ppo_publish_kernel<TO_POLICY>              elementwise
//   ppo_gradnorm_partial_kernel, ppo_adam_clip_kernel           the clip-aware Adam step (hk.h "LONG RUNS"): fp64 partials of |GRAD|^2 over fixed
//                           runs, then norm, coef and ppo_adam_kernel's step on g coef in one launch
//   ppo_norm_partial / combine / finalise / publish_kernel      the running normaliser (hk.h "NORMALISER"): fp64 sums over OBS / FIRST / RING0 read
//                           once, per-workgroup partials combined in partition order, the new state and the policy's fp32 mean / std
// HK_PPO_PREC_BF16 (hk.h "PRECISION"): the trunk products run on ppo_gemm_bf16_kernel<EPI> (v_mfma_f32_32x32x16_bf16, fp32 accumulation) over
// operands their producers rounded once — ppo_shadow_kernel (the weights, after Adam), ppo_gather_kernel<uint16_t>, ppo_head_back_bf16_kernel and
// the product's own epilogues; everything else above is shared with the fp32 mode.
#pragma once
#include "hk_policy.h"

namespace hk {

constexpr int PPO_KCH = 256;          // rows per split-K chunk of a weight gradient
constexpr int PPO_TM = 64, PPO_TN = 64, PPO_TK = 32, PPO_LD = 65;

// flat parameter layout of one network (torch order: W[l] [out][in], b[l], then the heads)
struct PpoNet {
    int in_dim = 0, hidden = 0, n_layers = 0, n_branch = 0;     // n_branch 0: the critic (one linear output)
    size_t oW[HK_POLICY_MAX_LAYERS] = {}, ob[HK_POLICY_MAX_LAYERS] = {};
    size_t oWmu = 0, obmu = 0, ols = 0, oWbr = 0, obbr = 0;      // critic: oWmu / obmu are the value head, ols / oWbr / obbr unused
    size_t count = 0;
    void layout(int in, int H, int L, int nb, size_t base)
    {
        in_dim = in; hidden = H; n_layers = L; n_branch = nb;
        size_t o = base;
        for (int l = 0; l < L; l++) {
            oW[l] = o; o += (size_t)H * (l == 0 ? in : H);
            ob[l] = o; o += H;
        }
        oWmu = o; o += H;
        obmu = o; o += 1;
        if (nb > 0) {
            ols = o; o += 1;
            oWbr = o; o += (size_t)nb * H;
            obbr = o; o += nb;
        }
        count = o - base;
    }
};

// the rollout rows a trainer reads (hk_rollout_field buffers) and its actor's input rule
struct PpoRows {
    const float *obs, *ring0, *next_obs, *raw, *reward, *term_reward, *logp_c, *logp_d;
    const int *first, *branch, *done;
    const float *mean, *std;            // the actor's normaliser, read in place (hk_ppo_normalizer_* publish into it); nullptr: none
    int R, E, A, S, D, stack, smax, in_dim, normalize;
    int slots[HK_MAX_AGENTS];
};

// (ppo_bf16_rne / ppo_bf16_f32, the fp32 <-> bf16 conversions: hk_bf16.h, shared with the bf16 inference chain)
struct ppo_bf16 { uint16_t v; __device__ operator double() const { return (double)ppo_bf16_f32(v); } };      // an element type for ppo_colsum_kernel
// a producer's store: as it is, or rounded once to bf16
__device__ __forceinline__ void ppo_put(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void ppo_put(uint16_t* p, size_t i, float v) { p[i] = ppo_bf16_rne(v); }

// ---------------------------------------------------------------------------------------------------------------------
// Row ids -> X0.  id in [0, n): row (t, e, j), t = id / (E S), e = id / S % E, j = id % S.  boot && id in [n, n + E S): the bootstrap input of
// (e, j) = id - n: the last row's stack shifted by one with NEXT_OBS pushed.  Any other id: a zero row, valid[i] = 0.
// The stack rule of rollout.stacked_inputs: entry q (oldest first) of row t is decision u = t - (stack - 1 - q); it is present when no
// decision in (u, t] cleared the stack (FIRST; the bootstrap's own push clears nothing) — OBS[u] for u >= 0, RING0 for u < 0 — else 0.
// T: float, or uint16_t (HK_PPO_PREC_BF16: rounded once to bf16 as it is written, ppo_put)
template <typename T>
__global__ __launch_bounds__(256) void ppo_gather_kernel(PpoRows P, const int* ids, int m, int boot, T* X0, int* valid)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)m * P.in_dim) return;
    const int i = (int)(idx / P.in_dim), k = (int)(idx % P.in_dim);
    const int n = P.R * P.E * P.S;
    const int id = ids[i];
    const bool is_row = id >= 0 && id < n;
    const bool is_boot = boot && id >= n && id < n + P.E * P.S;
    if (k == 0) valid[i] = is_row || is_boot;
    if (!is_row && !is_boot) { ppo_put(X0, idx, 0.0f); return; }
    int t, e, j;
    if (is_row) { t = id / (P.E * P.S); e = (id / P.S) % P.E; j = id % P.S; }
    else { t = P.R; e = (id - n) / P.S; j = (id - n) % P.S; }
    const int a = P.slots[j];
    const size_t ea = (size_t)e * P.A + a, EA = (size_t)P.E * P.A;
    const int q = k / P.D, d = k % P.D;
    const int u = t - (P.stack - 1 - q);
    const int last = t < P.R ? t : P.R - 1;          // the decisions whose FIRST can clear this entry: (u, last]
    bool present = true;
    for (int v = (u < 0 ? 0 : u + 1); v <= last; v++) if (P.first[(size_t)v * EA + ea]) { present = false; break; }
    float x = 0.0f;
    if (present) {
        if (u >= P.R) x = P.next_obs[ea * P.D + d];
        else if (u >= 0) x = P.obs[((size_t)u * EA + ea) * P.D + d];
        else x = P.ring0[(ea * (P.smax - 1) + (P.smax - 1 + u)) * P.D + d];
    }
    if (P.normalize) x = pm_normalise(x, P.mean[k], P.std[k]);      // policy_mlp_kernel's loader (hk_policy.h)
    ppo_put(X0, idx, x);
}

__global__ __launch_bounds__(256) void ppo_iota_kernel(int* ids, int base, int m)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) ids[i] = base + i;
}

// ---------------------------------------------------------------------------------------------------------------------
// C = seed + A B, A(i, k) = A[i sai + k sak] (M x K), B(k, j) = B[k sbk + j sbj] (K x N).  A workgroup of 4 waves owns a 64 x 64 tile of C,
// one 32 x 32 block per wave; K runs through LDS in chunks of 32 (tiles stored k-major, row stride 65: the MFMA operand reads of 32
// consecutive rows / columns are conflict-free), each chunk as MFMA 32x32x2 steps in ascending k — lane half h supplies k0 + h, the
// pairing pm_gemm uses — so a product with K even and no split is the k-ascending fmaf chain policy_mlp_kernel computes.
// blockIdx.z = split-K chunk of kch rows of K; chunk z writes C + z M N (row stride N) when nz > 1.
// EPI 0: C = acc (seeded with bias[j] when bias != nullptr).  EPI 1 (trunk forward): Z = acc, C = swish(acc).  EPI 2 (backward): C = acc * swish'(Z).
template <int EPI>
__global__ __launch_bounds__(256) void ppo_gemm_kernel(int M, int N, int K, const float* __restrict__ A, int sai, int sak, const float* __restrict__ B,
                                                       int sbk, int sbj, const float* __restrict__ bias, float* C, int ldc, float* Z, int kch)
{
    __shared__ float As[PPO_TK * PPO_LD], Bs[PPO_TK * PPO_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * PPO_TM, j0 = blockIdx.x * PPO_TN;
    const int kbeg = blockIdx.z * kch, kend = (kbeg + kch < K) ? kbeg + kch : K;
    const int wr = wave >> 1, wc = wave & 1, half = lane >> 5, c = lane & 31;
    const int jcol = j0 + wc * 32 + c;
    f32x16 acc;
    {
        const float s = (bias && jcol < N) ? bias[jcol] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = s;
    }
    for (int kb = kbeg; kb < kend; kb += PPO_TK) {
        const int kc = (kend - kb) < PPO_TK ? (kend - kb) : PPO_TK;
        // A tile [kk][ii]: threads along whichever dimension is contiguous in memory
        for (int x = tid; x < PPO_TK * PPO_TM; x += 256) {
            int ii, kk;
            if (sak == 1) { kk = x & 31; ii = x >> 5; } else { ii = x & 63; kk = x >> 6; }
            const int gi = i0 + ii, gk = kb + kk;
            As[kk * PPO_LD + ii] = (gi < M && kk < kc) ? A[(size_t)gi * sai + (size_t)gk * sak] : 0.0f;
        }
        for (int x = tid; x < PPO_TK * PPO_TN; x += 256) {
            int jj, kk;
            if (sbj == 1) { jj = x & 63; kk = x >> 6; } else { kk = x & 31; jj = x >> 5; }
            const int gj = j0 + jj, gk = kb + kk;
            Bs[kk * PPO_LD + jj] = (gj < N && kk < kc) ? B[(size_t)gk * sbk + (size_t)gj * sbj] : 0.0f;
        }
        __syncthreads();
        const float* ap = As + half * PPO_LD + wr * 32 + c;
        const float* bp = Bs + half * PPO_LD + wc * 32 + c;
        const int steps = (kc + 1) >> 1;
        for (int s = 0; s < steps; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[(size_t)2 * s * PPO_LD], bp[(size_t)2 * s * PPO_LD], acc, 0, 0, 0);
        __syncthreads();
    }
    if (jcol >= N) return;
    float* Cz = C + (gridDim.z > 1 ? (size_t)blockIdx.z * M * N : 0);
    // C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = i0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row >= M) continue;
        const size_t o = (size_t)row * ldc + jcol;
        if (EPI == 0) Cz[o] = acc[r];
        else if (EPI == 1) { Z[o] = acc[r]; Cz[o] = swish(acc[r]); }
        else {
            const float s = Z[o];
            const float sg = 1.0f / (1.0f + expf(-s));
            Cz[o] = acc[r] * (sg + s * sg * (1.0f - sg));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// HK_PPO_PREC_BF16: C = seed + A B over bf16 operands (raw bits) on v_mfma_f32_32x32x16_bf16, fp32 accumulation.  The tile, the wave blocks, the
// split-K rule and the three epilogues are ppo_gemm_kernel's.  An operand is stored either with k contiguous (a_kc: A is [M][K], b_kc: B is
// [N][K]; leading dimension lda / ldb) or with k as its row index ([K][M], [K][N]: the weight-gradient operands and W of the backward delta).
// K runs through LDS in chunks of 64 (4 MFMAs per wave), every tile kept [row][k] with a row stride of 72 elements (144 B: the 16-byte
// operand reads of 16 consecutive rows cover the 64 banks once), so an MFMA operand is one ds_read_b128.  The loader moves 8 elements
// (16 bytes) per load along whichever dimension is contiguous — element by element where the leading dimension or the base is not a
// multiple of 16 bytes, or the piece crosses an edge — holds the next chunk in registers while the MFMAs of the current one run, and stores
// it into the other LDS buffer: one barrier per chunk.  A k-as-row operand is transposed by that store (eight 2-byte stores per piece,
// consecutive lanes on consecutive k: conflict-free); there is no transposed copy in memory and no transposing LDS read.  Whatever lies
// past M, N or the chunk's K is staged as +0.0, which changes no fp32 sum.
// EPI 0: C = acc (fp32; the split-K partial tile of chunk blockIdx.z).  EPI 1: Z = acc (when Z), swish(acc) to C (fp32) and / or Cb (rounded to
// bf16).  EPI 2: acc * swish'(Z) to C and / or Cb.
constexpr int PB_TM = 64, PB_TN = 64, PB_TK = 64, PB_LD = 72;
typedef __bf16 ppo_bf16x8 __attribute__((ext_vector_type(8)));

// this thread's two pieces of the 64 x 64 tile (rows r0 .. of the operand, limit rlim; k from kb, limit kend), zero outside
__device__ __forceinline__ void pb_fetch(uint4 (&v)[2], const uint16_t* __restrict__ P, int ld, bool kc, bool vec, int r0, int rlim, int kb, int kend, int tid)
{
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int x = tid + 256 * q;
        int f, flim, c, clim;                      // f: the index on the strided dimension, c: the first of 8 on the contiguous one
        if (kc) { f = r0 + (x >> 3); flim = rlim; c = kb + (x & 7) * 8; clim = kend; }
        else { f = kb + (x & 63); flim = kend; c = r0 + (x >> 6) * 8; clim = rlim; }
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (f < flim && c < clim) {
            const uint16_t* p = P + (size_t)f * ld + c;
            if (vec && c + 8 <= clim) w = *reinterpret_cast<const uint4*>(p);
            else {
                uint32_t e[8];
#pragma unroll
                for (int j = 0; j < 8; j++) e[j] = (c + j < clim) ? (uint32_t)p[j] : 0u;
                w = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
            }
        }
        v[q] = w;
    }
}
// ... into the LDS tile T [64][PB_LD] (k contiguous)
__device__ __forceinline__ void pb_stage(uint16_t* T, const uint4 (&v)[2], bool kc, int tid)
{
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int x = tid + 256 * q;
        if (kc) *reinterpret_cast<uint4*>(T + (x >> 3) * PB_LD + (x & 7) * 8) = v[q];
        else {
            uint16_t* t = T + ((x >> 6) * 8) * PB_LD + (x & 63);
            const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
            for (int j = 0; j < 8; j++) t[j * PB_LD] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
    }
}

template <int EPI>
__global__ __launch_bounds__(256) void ppo_gemm_bf16_kernel(int M, int N, int K, const uint16_t* __restrict__ A, int lda, int a_kc,
                                                            const uint16_t* __restrict__ B, int ldb, int b_kc, const float* __restrict__ bias, float* C,
                                                            uint16_t* Cb, int ldc, float* Z, int kch)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][PB_TM * PB_LD], Bs[2][PB_TN * PB_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * PB_TM, j0 = blockIdx.x * PB_TN;
    const int kbeg = blockIdx.z * kch, kend = (kbeg + kch < K) ? kbeg + kch : K;
    const int wr = wave >> 1, wc = wave & 1, half = lane >> 5, c = lane & 31;
    const int jcol = j0 + wc * 32 + c;
    const bool avec = (lda & 7) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
    const bool bvec = (ldb & 7) == 0 && (reinterpret_cast<uintptr_t>(B) & 15) == 0;
    f32x16 acc;
    {
        const float s = (bias && jcol < N) ? bias[jcol] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = s;
    }
    const int nch = (kend - kbeg + PB_TK - 1) / PB_TK;
    uint4 va[2], vb[2];
    pb_fetch(va, A, lda, a_kc != 0, avec, i0, M, kbeg, kend, tid);
    pb_fetch(vb, B, ldb, b_kc != 0, bvec, j0, N, kbeg, kend, tid);
    pb_stage(As[0], va, a_kc != 0, tid);
    pb_stage(Bs[0], vb, b_kc != 0, tid);
    __syncthreads();
    for (int n = 0; n < nch; n++) {
        const int cur = n & 1;
        const bool more = n + 1 < nch;
        if (more) {                              // the next chunk's loads are in flight while this one's MFMAs run
            pb_fetch(va, A, lda, a_kc != 0, avec, i0, M, kbeg + (n + 1) * PB_TK, kend, tid);
            pb_fetch(vb, B, ldb, b_kc != 0, bvec, j0, N, kbeg + (n + 1) * PB_TK, kend, tid);
        }
        // operand maps of 32x32x16: lane (r = lane & 31, h = lane >> 5) holds A[r][8 h + j] and B[8 h + j][r], j = 0 .. 7
        const uint16_t* ap = As[cur] + (wr * 32 + c) * PB_LD + half * 8;
        const uint16_t* bp = Bs[cur] + (wc * 32 + c) * PB_LD + half * 8;
#pragma unroll
        for (int s = 0; s < PB_TK / 16; s++) {
            const ppo_bf16x8 a = *reinterpret_cast<const ppo_bf16x8*>(ap + s * 16);
            const ppo_bf16x8 b = *reinterpret_cast<const ppo_bf16x8*>(bp + s * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        }
        if (more) {                              // the other buffer: every wave finished reading it before the last barrier
            pb_stage(As[cur ^ 1], va, a_kc != 0, tid);
            pb_stage(Bs[cur ^ 1], vb, b_kc != 0, tid);
        }
        __syncthreads();
    }
    if (jcol >= N) return;
    const size_t zo = gridDim.z > 1 ? (size_t)blockIdx.z * M * N : 0;
    // C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = i0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row >= M) continue;
        const size_t o = (size_t)row * ldc + jcol;
        float v;
        if (EPI == 0) v = acc[r];
        else if (EPI == 1) { if (Z) Z[o] = acc[r]; v = swish(acc[r]); }
        else {
            const float s = Z[o];
            const float sg = 1.0f / (1.0f + expf(-s));
            v = acc[r] * (sg + s * sg * (1.0f - sg));
        }
        if (C) C[zo + o] = v;
        if (Cb) Cb[o] = ppo_bf16_rne(v);
    }
}

// the bf16 shadow of PARAMS: element i of the actor at i, of the critic at i + pad (the critic's matrices then start on 16 bytes as the actor's do)
__global__ __launch_bounds__(256) void ppo_shadow_kernel(const float* p, uint16_t* shadow, size_t n, size_t n_actor, size_t pad)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) shadow[i + (i >= n_actor ? pad : 0)] = ppo_bf16_rne(p[i]);
}

// out[r][c] (row stride N; rows >= 1 go to out1 + (r - 1) N when out1) = sum over the nz chunks' partial tiles, in chunk order
__global__ __launch_bounds__(256) void ppo_combine_kernel(const float* part, int nz, int M, int N, float* out0, float* out1)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, MN = (size_t)M * N;
    if (idx >= MN) return;
    float s = 0.0f;
    for (int z = 0; z < nz; z++) s += part[(size_t)z * MN + idx];
    const int r = (int)(idx / N);
    if (out1 && r >= 1) out1[idx - N] = s;
    else out0[idx] = s;
}

// out[c] = sum_i X[i ld + c] for c < ncol, one workgroup per column: fixed strided partial sums, then a fixed tree (deterministic)
template <typename T>
__global__ __launch_bounds__(256) void ppo_colsum_kernel(const T* X, int m, int ld, float* out)
{
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < m; i += 256) s += (double)X[(size_t)i * ld + c];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[c] = (float)red[0];
}

// the minibatch's valid rows (one workgroup)
__global__ __launch_bounds__(256) void ppo_count_kernel(const int* valid, int m, int* out)
{
    __shared__ int red[256];
    const int tid = threadIdx.x;
    int s = 0;
    for (int i = tid; i < m; i += 256) s += valid[i] != 0;
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    if (tid == 0) out[0] = red[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// One thread per minibatch row: heads, log-probabilities, the losses and dL / d(head) (HK_PPO_* row stats: [0] the two clipped surrogate
// terms summed, [1] the value term, [2] H, [3] old - new logp summed over c, d, [4] clipped columns, [5] skipped).
struct PpoLossArgs {
    const float *Aa, *Ac;            // the last hidden activations [m][Ha], [m][Hc]
    const float *W_mu, *b_mu, *log_sigma, *W_br, *b_br, *W_v, *b_v;
    const float *v_old, *adv, *ret;
    const int* ids;
    const int* valid;
    const int* n_valid;              // the minibatch's valid rows (ppo_count_kernel)
    int m, n, Ha, Hc, nb;
    float eps, beta;
    float *dhead;                    // [m][PM_MAX_OUT]: dmu, dlogits
    float *dls, *dv;                 // [m]
    double* rowstat;                 // [m][6]
    float *mu_out, *logit_out, *v_out;   // debug taps [m], [m][nb], [m]
};

__global__ __launch_bounds__(256) void ppo_loss_kernel(PpoRows P, PpoLossArgs L)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.m) return;
    double* st = L.rowstat + (size_t)i * 6;
    float* dh = L.dhead + (size_t)i * PM_MAX_OUT;
    const int id = L.ids[i];
    if (!L.valid[i] || id < 0 || id >= L.n) {
        for (int o = 0; o < PM_MAX_OUT; o++) dh[o] = 0.0f;
        L.dls[i] = 0.0f; L.dv[i] = 0.0f;
        for (int o = 0; o < 5; o++) st[o] = 0.0;
        st[5] = 1.0;
        return;
    }
    const float inv = 1.0f / (float)L.n_valid[0];
    // ---- heads: policy_mlp_kernel's fmaf chains (pm_head, hk_policy.h)
    const float* aa = L.Aa + (size_t)i * L.Ha;
    const float mu = pm_head(aa, 1, L.W_mu, L.b_mu[0], L.Ha);
    float lg[PM_MAX_OUT];
    for (int b = 0; b < L.nb; b++) lg[b] = pm_head(aa, 1, L.W_br + (size_t)b * L.Ha, L.b_br[b], L.Ha);
    const float v = pm_head(L.Ac + (size_t)i * L.Hc, 1, L.W_v, L.b_v[0], L.Hc);
    if (L.mu_out) {
        L.mu_out[i] = mu; L.v_out[i] = v;
        for (int b = 0; b < L.nb; b++) L.logit_out[(size_t)i * L.nb + b] = lg[b];
    }
    // ---- the row
    const int t = id / (P.E * P.S), e = (id / P.S) % P.E, j = id % P.S;
    const size_t ea = ((size_t)t * P.E + e) * P.A + P.slots[j];
    const float raw = P.raw[ea], old_c = P.logp_c[ea], old_d = P.logp_d[ea];
    const int pick = P.branch[ea];
    const float A = L.adv[id], vo = L.v_old[id], R = L.ret[id];
    // ---- log-probabilities: the recorder's own helpers (hk_policy.h), so that unchanged parameters give rho == 1 exactly
    const float ls = L.log_sigma[0];
    const float sigma = hk_expf(ls);
    const float z = (raw - mu) / sigma;
    const float logp_c = pm_logp_cont(raw, mu, sigma, ls);
    const int best = pm_argmax(lg, L.nb);
    const float logp_d = pm_logp_disc(lg, L.nb, best, pick);
    float ex[PM_MAX_OUT], tot = 0.0f;
    for (int b = 0; b < L.nb; b++) { ex[b] = hk_expf(lg[b] - lg[best]); tot += ex[b]; }
    const float ltot = hk_logf(tot);
    // ---- clipped surrogate, per column (torch.min / torch.clamp gradients: a tie splits, the clamp passes inside [lo, hi])
    const float lo = 1.0f - L.eps, hi = 1.0f + L.eps;
    float surr = 0.0f, clipped = 0.0f, dlogp[2];
    const float lp[2] = {logp_c, logp_d}, old[2] = {old_c, old_d};
    for (int q = 0; q < 2; q++) {
        const float rho = hk_expf(lp[q] - old[q]);
        const float rc = rho < lo ? lo : (rho > hi ? hi : rho);
        const float u = rho * A, w = rc * A;
        const float gu = A, gw = (rho >= lo && rho <= hi) ? A : 0.0f;
        const float g = u < w ? gu : (u > w ? gw : 0.5f * (gu + gw));
        surr += u < w ? u : w;
        clipped += (rho < lo || rho > hi) ? 1.0f : 0.0f;
        dlogp[q] = -0.5f * inv * g * rho;
    }
    // ---- entropy
    float Hd = 0.0f, logp_b[PM_MAX_OUT], p_b[PM_MAX_OUT];
    for (int b = 0; b < L.nb; b++) {
        p_b[b] = ex[b] / tot;
        logp_b[b] = (lg[b] - lg[best]) - ltot;
        Hd -= p_b[b] * logp_b[b];
    }
    const float H = 1.418938533204672742f + ls + Hd;           // 0.5 log(2 pi e) + log_sigma + categorical
    // ---- gradients of L = L_pi + 0.5 L_v - beta mean H with respect to the heads
    dh[0] = dlogp[0] * (z / sigma);
    for (int b = 0; b < L.nb; b++)
        dh[1 + b] = dlogp[1] * ((b == pick ? 1.0f : 0.0f) - p_b[b]) + L.beta * inv * p_b[b] * (logp_b[b] + Hd);
    for (int b = 1 + L.nb; b < PM_MAX_OUT; b++) dh[b] = 0.0f;
    L.dls[i] = dlogp[0] * (z * z - 1.0f) - L.beta * inv;
    // ---- clipped value loss (torch.max: a tie splits)
    const float dvv = v - vo;
    const float dc = dvv < -L.eps ? -L.eps : (dvv > L.eps ? L.eps : dvv);
    const float a1 = R - v, b1 = R - vo - dc;
    const float f1 = a1 * a1, f2 = b1 * b1;
    const float g1 = -2.0f * a1, g2 = (dvv >= -L.eps && dvv <= L.eps) ? -2.0f * b1 : 0.0f;
    const float gv = f1 > f2 ? g1 : (f1 < f2 ? g2 : 0.5f * (g1 + g2));
    L.dv[i] = 0.5f * inv * gv;
    st[0] = surr; st[1] = f1 > f2 ? f1 : f2; st[2] = H; st[3] = (double)(old_c - logp_c) + (double)(old_d - logp_d); st[4] = clipped; st[5] = 0.0;
}

// the six stats of a minibatch from the row stats (one workgroup, fixed order); acc != nullptr: also added into acc[0..5], acc[6] += 1
__global__ __launch_bounds__(256) void ppo_stats_kernel(const double* rowstat, int m, float* stats, double* acc)
{
    __shared__ double red[6][256];
    const int tid = threadIdx.x;
    double s[6] = {};
    for (int i = tid; i < m; i += 256)
        for (int q = 0; q < 6; q++) s[q] += rowstat[(size_t)i * 6 + q];
    for (int q = 0; q < 6; q++) red[q][tid] = s[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) for (int q = 0; q < 6; q++) red[q][tid] += red[q][tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double skipped = red[5][0], mv = (double)m - skipped;
        const double d = mv > 0 ? mv : 1.0;
        double o[6] = {-red[0][0] / (2.0 * d), red[1][0] / d, red[2][0] / d, red[3][0] / (2.0 * d), red[4][0] / (2.0 * d), skipped};
        for (int q = 0; q < 6; q++) stats[q] = (float)o[q];
        if (acc) { for (int q = 0; q < 6; q++) acc[q] += o[q]; acc[6] += 1.0; }
    }
}

// delta_L of a trunk: dA[i][h] = (sum_o dhead[i][o] W_head[o][h]) * swish'(Z[i][h])  (vector ALU; n_out <= PM_MAX_OUT)
template <typename T>
__device__ __forceinline__ void ppo_head_back_row(int m, int H, int n_out, const float* dhead, int ldd, const float* W0, const float* W1, const float* Z, T* dA)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)m * H) return;
    const int i = (int)(idx / H), h = (int)(idx % H);
    float s = dhead[(size_t)i * ldd] * W0[h];
    for (int o = 1; o < n_out; o++) s += dhead[(size_t)i * ldd + o] * W1[(size_t)(o - 1) * H + h];
    const float zz = Z[idx];
    const float sg = 1.0f / (1.0f + expf(-zz));
    ppo_put(dA, idx, s * (sg + zz * sg * (1.0f - sg)));
}
__global__ __launch_bounds__(256) void ppo_head_back_kernel(int m, int H, int n_out, const float* dhead, int ldd, const float* W0, const float* W1,
                                                            const float* Z, float* dA)
{
    ppo_head_back_row(m, H, n_out, dhead, ldd, W0, W1, Z, dA);
}
__global__ __launch_bounds__(256) void ppo_head_back_bf16_kernel(int m, int H, int n_out, const float* dhead, int ldd, const float* W0, const float* W1,
                                                                 const float* Z, uint16_t* dA)
{
    ppo_head_back_row(m, H, n_out, dhead, ldd, W0, W1, Z, dA);
}

// hk_ppo_advantages: the critic's value head over rows ids[0 .. m) (row ids and bootstrap ids, ppo_gather_kernel) -> v_old[id] / vb[id - n]
__global__ __launch_bounds__(256) void ppo_value_kernel(const float* Ac, int m, int Hc, const float* W_v, const float* b_v, const int* ids, int n, int nb_boot,
                                                        float* v_old, float* vb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int id = ids[i];
    const float v = pm_head(Ac + (size_t)i * Hc, 1, W_v, b_v[0], Hc);          // the minibatch's value head, bit for bit
    if (id >= 0 && id < n) v_old[id] = v;
    else if (id >= n && id < n + nb_boot) vb[id - n] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// GAE, one lane per (e, j), t from R - 1 down (hk.h); V of row R is the bootstrap value vb[e][j]
__global__ __launch_bounds__(256) void ppo_gae_kernel(PpoRows P, const float* v_old, const float* vb, float gamma, float lambd, float* adv, float* ret)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.E * P.S) return;
    const int e = p / P.S, j = p % P.S;
    float vnext = vb[p], anext = 0.0f;
    for (int t = P.R - 1; t >= 0; t--) {
        const size_t r = ((size_t)t * P.E + e) * P.S + j;
        const size_t ea = ((size_t)t * P.E + e) * P.A + P.slots[j];
        const int d = P.done[(size_t)t * P.E + e] != 0;
        const float rw = d ? P.term_reward[ea] : P.reward[ea];
        const float nd = d ? 0.0f : 1.0f;
        const float v = v_old[r];
        const float delta = rw + gamma * nd * vnext - v;
        const float a = delta + gamma * lambd * nd * anext;
        adv[r] = a;
        ret[r] = a + v;
        vnext = v; anext = a;
    }
}

// ADV <- (ADV - mean) / (std + 1e-10), population std, both in fp64 (one workgroup: fixed strided sums, fixed tree)
__global__ __launch_bounds__(1024) void ppo_adv_norm_kernel(float* adv, int n)
{
    __shared__ double red[1024];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n; i += 1024) s += (double)adv[i];
    red[tid] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    const double mean = red[0] / n;
    __syncthreads();
    s = 0.0;
    for (int i = tid; i < n; i += 1024) { const double d = (double)adv[i] - mean; s += d * d; }
    red[tid] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    const double sd = sqrt(red[0] / n) + 1e-10;
    for (int i = tid; i < n; i += 1024) adv[i] = (float)(((double)adv[i] - mean) / sd);
}

// ---------------------------------------------------------------------------------------------------------------------
// The row permutation of an update's epoch: a 4-round Feistel network on 2 hb bits (2^(2 hb) >= n) keyed by (seed, count), cycle-walked
// into [0, n).  The host twin is hierarchicalkarting_amd/ppo.py permutation().
__host__ __device__ inline uint32_t ppo_hash(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t ppo_perm(uint32_t i, uint32_t n, uint32_t seed, uint32_t count)
{
    int bits = 2;
    while (bits < 32 && (1u << bits) < n) bits++;
    const int hb = (bits + 1) >> 1;
    const uint32_t mask = (1u << hb) - 1u;
    uint32_t key[4];
    for (int r = 0; r < 4; r++) key[r] = ppo_hash(seed ^ ppo_hash(count * 0x9E3779B9u + (uint32_t)r * 0x85EBCA6Bu + 1u));
    uint32_t x = i;
    do {
        uint32_t lft = x >> hb, rgt = x & mask;
        for (int r = 0; r < 4; r++) {
            const uint32_t f = ppo_hash(rgt ^ key[r]) & mask;
            const uint32_t nr = lft ^ f;
            lft = rgt; rgt = nr;
        }
        x = (lft << hb) | rgt;
    } while (x >= n);
    return x;
}
__global__ __launch_bounds__(256) void ppo_perm_kernel(int* perm, int n, uint32_t seed, uint32_t count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (int)ppo_perm((uint32_t)i, (uint32_t)n, seed, count);
}

// Adam, in the order hk.h states: m = b1 m + (1 - b1) g; v = b2 v + ((1 - b2) g) g; p = p - lr (m / c1) / (sqrt(v / c2) + eps)
__global__ __launch_bounds__(256) void ppo_adam_kernel(float* p, const float* g, float* mm, float* vv, size_t n, float b1, float omb1, float b2, float omb2,
                                                       float c1, float c2, float eps, float lr)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float m1 = b1 * mm[i] + omb1 * gi;
    const float v1 = b2 * vv[i] + (omb2 * gi) * gi;
    mm[i] = m1; vv[i] = v1;
    const float mh = m1 / c1;
    const float vh = v1 / c2;
    p[i] = p[i] - lr * mh / (sqrtf(vh) + eps);
}

// ---------------------------------------------------------------------------------------------------------------------
// Clip by the global L2 norm (hk.h "LONG RUNS"): two launches per step.
//   ppo_gradnorm_partial_kernel   workgroup x owns the run [x PPO_GN_RUN, (x + 1) PPO_GN_RUN) of GRAD and writes part[x] = sum (double)g (double)g
//                                 (a square of an fp32 value is exact in fp64).  GRAD starts P floats into the allocation, so its runs are
//                                 16-byte aligned only when P % 4 == 0: the run is peeled to alignment (head < 4 elements, lanes 0 .. head - 1),
//                                 read as float4 v = tid, tid + 256, ... (coalesced), and closed by a tail of < 4 elements.  A lane adds its
//                                 elements in ascending index order, then a fixed LDS tree: the partition and the order depend on P alone.
//   ppo_adam_clip_kernel          every workgroup sums the partials in index order (lane 0; <= a few hundred cached loads), derives the same
//                                 norm and coef, and does ppo_adam_kernel's step, operation for operation, on g' = g coef.  A norm2 that is not
//                                 finite: nothing is written.  Workgroup 0 keeps the HK_PPO_CLIP words.
constexpr int PPO_GN_RUN = 4096;

__global__ __launch_bounds__(256) void ppo_gradnorm_partial_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const size_t lo = (size_t)blockIdx.x * PPO_GN_RUN;
    const int len = (int)((n - lo < (size_t)PPO_GN_RUN) ? n - lo : (size_t)PPO_GN_RUN);
    const float* run = g + lo;
    int head = (int)((4u - (unsigned)(((uintptr_t)run >> 2) & 3u)) & 3u);
    if (head > len) head = len;
    const int nv = (len - head) >> 2, tail0 = head + 4 * nv;
    const float4* body = reinterpret_cast<const float4*>(run + head);
    double s = 0.0;
    if (tid < head) { const double x = (double)run[tid]; s += x * x; }
    float4 x[PPO_GN_RUN / 1024];
#pragma unroll
    for (int j = 0; j < PPO_GN_RUN / 1024; j++) {
        const int v = tid + 256 * j;
        x[j] = v < nv ? body[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int j = 0; j < PPO_GN_RUN / 1024; j++) {
        if (tid + 256 * j < nv) {
            const double a = (double)x[j].x, b = (double)x[j].y, c = (double)x[j].z, d = (double)x[j].w;
            s += a * a; s += b * b; s += c * c; s += d * d;
        }
    }
    if (tail0 + tid < len) { const double y = (double)run[tail0 + tid]; s += y * y; }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

// words: HK_PPO_CLIP [8] — norm, coef, steps, steps with coef < 1, non-finite steps, sum and max of norm over the finite steps, 0
__global__ __launch_bounds__(256) void ppo_adam_clip_kernel(float* p, const float* g, float* mm, float* vv, size_t n, float b1, float omb1, float b2, float omb2,
                                                            float c1, float c2, float eps, float lr, const double* __restrict__ part, int npart,
                                                            float max_norm, double* words)
{
    __shared__ float s_coef;
    __shared__ int s_finite;
    if (threadIdx.x == 0) {
        double norm2 = 0.0;
        for (int x = 0; x < npart; x++) norm2 += part[x];
        const bool finite = isfinite(norm2);
        const double norm = sqrt(norm2);
        const double r = (double)max_norm / (norm + 1e-6);
        const float coef = finite ? (float)(r < 1.0 ? r : 1.0) : 0.0f;
        s_coef = coef; s_finite = finite ? 1 : 0;
        if (blockIdx.x == 0) {
            words[0] = norm; words[1] = (double)coef; words[2] += 1.0; words[7] = 0.0;
            if (finite) {
                if (coef < 1.0f) words[3] += 1.0;
                words[5] += norm;
                if (norm > words[6]) words[6] = norm;
            } else {
                words[4] += 1.0;
            }
        }
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !s_finite) return;
    const float gi = g[i] * s_coef;
    const float m1 = b1 * mm[i] + omb1 * gi;
    const float v1 = b2 * vv[i] + (omb2 * gi) * gi;
    mm[i] = m1; vv[i] = v1;
    const float mh = m1 / c1;
    const float vh = v1 / c2;
    p[i] = p[i] - lr * mh / (sqrtf(vh) + eps);
}

// ---------------------------------------------------------------------------------------------------------------------
// master actor parameters (PpoNet layout) <-> the inference copies of policy_upload: Wt[k][j] = W[j][k], the group-major Wq, biases, heads.
// One thread per element of the flat actor vector.  TO_POLICY: publish; else the master copy is read back from the attached policy.
template <bool TO_POLICY>
__global__ __launch_bounds__(256) void ppo_publish_kernel(PolicyParams Q, PpoNet net, float* flat)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= net.count) return;
    const int H = Q.hidden;
    auto mv = [&](const float* dst_c, size_t di) {
        float* dst = const_cast<float*>(dst_c);
        if (TO_POLICY) dst[di] = flat[idx]; else flat[idx] = dst[di];
    };
    for (int l = 0; l < net.n_layers; l++) {
        const int K = l == 0 ? Q.in_dim : H;
        if (idx >= net.oW[l] && idx < net.oW[l] + (size_t)H * K) {
            const size_t w = idx - net.oW[l];
            const int jj = (int)(w / K), k = (int)(w % K);
            mv(Q.Wt[l], (size_t)k * H + jj);
            if (TO_POLICY && k < (K / 8) * 8)        // the group-major copy: k = 8 g + 2 j + half
                const_cast<float*>(reinterpret_cast<const float*>(Q.Wq[l]))[pm_wq_index(k >> 3, k & 1, jj, (k & 7) >> 1, H)] = flat[idx];
            return;
        }
        if (idx >= net.ob[l] && idx < net.ob[l] + H) { mv(Q.b[l], idx - net.ob[l]); return; }
    }
    if (idx >= net.oWmu && idx < net.oWmu + H) mv(Q.W_mu, idx - net.oWmu);
    else if (idx == net.obmu) mv(Q.b_mu, 0);
    else if (idx == net.ols) mv(Q.log_sigma, 0);
    else if (idx >= net.oWbr && idx < net.oWbr + (size_t)net.n_branch * H) mv(Q.W_branch, idx - net.oWbr);
    else if (idx >= net.obbr && idx < net.obbr + net.n_branch) mv(Q.b_branch, idx - net.obbr);
}

// ---------------------------------------------------------------------------------------------------------------------
// Running normaliser (hk.h "PPO trainer" NORMALISER): sum_i c_ik and sum_i c_ik^2, c_ik = x_ik - m_k, over the n rows' stacked inputs, which
// are never built.  An ITEM is one recorded observation (u, e, j), u in [-(stack - 1), R): OBS[u] for u >= 0, the RING0 entry for u < 0.  It is
// entry q = stack - 1 - s of row t = u + s for every s in [0, stack) with 0 <= t < R and no FIRST in (u, t] (ppo_gather_kernel's rule, read
// from the entry's side), so one read of the item feeds every stack position: s ascending, the FIRST words of (e, j) ORed as it goes.  What
// is absent is not visited: the finalise kernel adds (n - present_q) (-m_k) and (n - present_q) m_k^2 from the counts.
// Threads: lane d of a group of DL = min(D, 256) lanes owns observation column d (coalesced along the observation; blockIdx.z: further
// blocks of 256 columns), the 256 / DL groups of a workgroup take consecutive items, PPO_NORM_U of them per trip with their loads issued
// together.  blockIdx.y: PPO_NORM_Q stack positions per pass (one pass up to stack 8; a taller stack reads its items once per 8 positions).
// Workgroup x owns the items [x ipw, (x + 1) ipw) — a partition fixed by the shapes — and writes its fp64 partials to part[x][W],
// W = 2 in_dim + stack: sum c [in_dim], sum c^2 [in_dim], present [stack]; every sum in a fixed order, no atomics.
constexpr int PPO_NORM_Q = 8, PPO_NORM_U = 4, PPO_NORM_MAXWG = 2048, PPO_NORM_SEG = 16;

__global__ __launch_bounds__(256) void ppo_norm_partial_kernel(PpoRows P, const double* __restrict__ state, int ipw, double* __restrict__ part)
{
    __shared__ double red[PPO_NORM_Q][256];
    const int tid = threadIdx.x;
    const int D = P.D, stack = P.stack, R = P.R, ES = P.E * P.S;
    const int DL = D < 256 ? D : 256, G = 256 / DL;
    const int g = tid / DL, d = blockIdx.z * 256 + tid % DL;
    const bool lane_ok = g < G && d < D;
    const int q_hi = stack - blockIdx.y * PPO_NORM_Q;                 // this pass: positions [q_hi - nq, q_hi), acc[r] <-> q = q_hi - 1 - r, s = s0 + r
    const int nq = q_hi < PPO_NORM_Q ? q_hi : PPO_NORM_Q;
    const int s0 = stack - q_hi;
    const int items = (R + stack - 1) * ES;
    const int lo = blockIdx.x * ipw, hi = (lo + ipw < items) ? lo + ipw : items;
    const size_t EA = (size_t)P.E * P.A;
    double m[PPO_NORM_Q], s1[PPO_NORM_Q], s2[PPO_NORM_Q];
    unsigned cnt[PPO_NORM_Q];
#pragma unroll
    for (int r = 0; r < PPO_NORM_Q; r++) {
        m[r] = (lane_ok && r < nq) ? state[(size_t)(q_hi - 1 - r) * D + d] : 0.0;
        s1[r] = 0.0; s2[r] = 0.0; cnt[r] = 0u;
    }
    for (int base = lo; base < hi; base += G * PPO_NORM_U) {
        float x[PPO_NORM_U];
        int uu[PPO_NORM_U];
        size_t eaa[PPO_NORM_U];
        bool ok[PPO_NORM_U];
#pragma unroll
        for (int v = 0; v < PPO_NORM_U; v++) {
            const int it = base + v * G + g;
            ok[v] = lane_ok && it < hi;
            const int itc = ok[v] ? it : lo;
            const int ue = itc / ES, rem = itc - ue * ES, e = rem / P.S;
            const int u = ue - (stack - 1), a = P.slots[rem - e * P.S];
            const size_t ea = (size_t)e * P.A + a;
            uu[v] = u; eaa[v] = ea;
            x[v] = 0.0f;
            if (ok[v]) x[v] = u >= 0 ? P.obs[((size_t)u * EA + ea) * D + d] : P.ring0[(ea * (P.smax - 1) + (P.smax - 1 + u)) * D + d];
        }
#pragma unroll
        for (int v = 0; v < PPO_NORM_U; v++) {
            const int u = uu[v];
            const int* fr = P.first + eaa[v];
            bool dead = !ok[v];
            for (int s = 1; s < s0; s++) {                            // (a stack above PPO_NORM_Q: the positions of the passes before this one)
                const int t = u + s;
                if (t >= 0 && t < R && fr[(size_t)t * EA]) dead = true;
            }
            const double xd = (double)x[v];
#pragma unroll
            for (int r = 0; r < PPO_NORM_Q; r++) {
                const int s = s0 + r, t = u + s;
                const bool row = r < nq && t >= 0 && t < R;
                if (row && s >= 1 && fr[(size_t)t * EA]) dead = true;
                if (row && !dead) {
                    const double c = xd - m[r];
                    s1[r] += c; s2[r] += c * c; cnt[r] += 1u;
                }
            }
        }
    }
    // the groups' sums, group 0 first (fixed order); one LDS buffer, used for sum c, then sum c^2, then the counts
    const int in_dim = P.in_dim;
    double* out = part + (size_t)blockIdx.x * (2 * in_dim + stack);
    const bool writer = lane_ok && g == 0;
    for (int pass = 0; pass < 3; pass++) {
#pragma unroll
        for (int r = 0; r < PPO_NORM_Q; r++) red[r][tid] = pass == 0 ? s1[r] : (pass == 1 ? s2[r] : (double)cnt[r]);
        __syncthreads();
        if (writer && (pass < 2 || d == 0)) {
#pragma unroll
            for (int r = 0; r < PPO_NORM_Q; r++) {
                if (r >= nq) continue;
                double a = red[r][tid];
                for (int gg = 1; gg < G; gg++) a += red[r][gg * DL + tid];
                const int q = q_hi - 1 - r;
                if (pass < 2) out[(size_t)pass * in_dim + (size_t)q * D + d] = a;
                else out[2 * in_dim + q] = a;
            }
        }
        __syncthreads();
    }
}

// sums[c] = the nwg partials of column c in partition order: PPO_NORM_SEG consecutive runs summed side by side, then the runs in order
__global__ __launch_bounds__(256) void ppo_norm_combine_kernel(const double* __restrict__ part, int nwg, int W, double* __restrict__ sums)
{
    __shared__ double red[PPO_NORM_SEG][256 / PPO_NORM_SEG];
    constexpr int NC = 256 / PPO_NORM_SEG;
    const int tid = threadIdx.x, cl = tid % NC, seg = tid / NC;
    const int c = blockIdx.x * NC + cl;
    const int per = (nwg + PPO_NORM_SEG - 1) / PPO_NORM_SEG;
    const int x0 = seg * per, x1 = (x0 + per < nwg) ? x0 + per : nwg;
    double s = 0.0;
    if (c < W) for (int x = x0; x < x1; x++) s += part[(size_t)x * W + c];
    red[seg][cl] = s;
    __syncthreads();
    if (seg != 0 || c >= W) return;
    for (int k = 1; k < PPO_NORM_SEG; k++) s += red[k][cl];
    sums[c] = s;
}

// the published form of a state: mean = fp32(m), std = fp32(sqrt(M2 / N)), division and square root in fp64 (IEEE: no fast-math in this build)
__device__ __forceinline__ void ppo_norm_put(double m, double M2, double N, float* mean, float* sdev, int k)
{
    mean[k] = (float)m;
    sdev[k] = (float)sqrt(M2 / N);
}

// one thread per stacked input k: the batch update of hk.h from the combined sums (n rows, N1 = N + n), the new state and its published form
__global__ __launch_bounds__(256) void ppo_norm_finalise_kernel(const double* __restrict__ sums, double* state, float* mean, float* sdev, int in_dim, int D,
                                                                double n, double N1)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= in_dim) return;
    const double absent = n - sums[2 * in_dim + k / D];
    const double m = state[k];
    const double delta = sums[k] - absent * m;
    const double c2 = sums[in_dim + k] + absent * (m * m);
    const double m1 = m + delta / N1;
    const double M2 = state[in_dim + k] + (c2 - (delta * delta) / N1);
    state[k] = m1; state[in_dim + k] = M2;
    ppo_norm_put(m1, M2, N1, mean, sdev, k);
}

__global__ __launch_bounds__(256) void ppo_norm_publish_kernel(const double* __restrict__ state, float* mean, float* sdev, int in_dim, double N)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < in_dim) ppo_norm_put(state[k], state[in_dim + k], N, mean, sdev, k);
}

}  // namespace hk
