// hk_policy_lstm_bf16.h — HK_POLICY_PREC_BF16 for a policy with memory (hk_policy_lstm_set_precision): the decision of policy_lstm_kernel
// with the trunk AND the four gate chains on v_mfma_f32_32x32x16_bf16 (contract in include/hk.h "RECURRENT ACTORS IN BF16").
// Included by hk_policy.h after hk_policy_bf16.h and hk_policy_lstm.h, whose pieces it is made of.
//
// The arithmetic is, operand for operand, the bf16 recurrent trainer's forward (hk_train.hip: ppo_trunk_forward, ppo_cell_project,
// hk_ppo_lstm_bf16.h ppo_lstm_step_bf16_kernel):
//   trunk   policy_mlp_bf16_kernel's, with one difference: the LAST layer's post-activation a is rounded to bf16 too and stays in X, padded
//           with +0.0 to a whole 64-wide chunk — here it is an operand of the cell's product and no head reads it.
//   gates   one fp32 accumulator per (row, unit, gate), seeded with fp32 b_ih + b_hh (PolicyLstm::b), stepped in ascending k over a[0 .. Hp),
//           Hp = H padded to 64 (the all-zero steps are NOT skipped: they are the product kernel's), then over h[0 .. m) in m / 16 whole steps;
//           W_ih / W_hh rounded once from the fp32 inference copies, h rounded once where it is staged.
//   cell    hk_lstm_cell, fp32 and unchanged: c read from and c' written to the fp32 memory, h' fp32 to the memory and to Ht for the heads.
//   heads   pm_tail with width m on the fp32 h'.
//
// One workgroup (8 waves) per tile of 64 rows, one launch per decision; activations never leave LDS:
//   X   bf16 [row][k], stride kmax + 8 (hk_policy_bf16.h: PB_LD's rule), the trunk's tile;
//   Hb  bf16 [row][k], stride m + 8 (m / 8 is a multiple of 4, so the stride is an odd multiple of four dwords too), h of the tile's rows;
//   Ht  fp32 [unit][PM_LD], h' as pm_tail reads it, written over X / Hb after the gates' barrier.
//   LDS = max(64 (kmax + 8) 2 + 64 (m + 8) 2, m x 65 x 4) + the heads' 2 KB: 61 440 B at 312 -> 128 x 3 -> m = 128 (the fp32 kernel: 101 888 B),
//   under the 64 KB default limit at every supported shape.
// Weights: policy_lstm_bf16_build_kernel lays W_ih / W_hh out fragment-major, [unit block][gate][k step][lane][8]: one MFMA's B operand is 1 KB,
// one coalesced 16-byte load per lane, +0.0 where k >= K.  A wave holds the four gate accumulators of its (row block, unit block), as in
// policy_lstm_kernel, and keeps the next step's four B operands in flight (plb_gemm4).
#pragma once

namespace hk {

// elements of the fragment-major copies of W_ih (K = hidden, padded to 64) and W_hh (K = m)
inline size_t policy_lstm_bf16_ih_elems(const PolicyParams& q, const PolicyLstm& l) { return (size_t)4 * l.m * pmb_pad64(q.hidden); }
inline size_t policy_lstm_bf16_hh_elems(const PolicyLstm& l) { return (size_t)4 * l.m * l.m; }

inline size_t policy_lstm_bf16_lds_bytes(const PolicyParams& q, const PolicyLstm& l)
{
    const size_t xb = (size_t)PM_TILE * (pmb_kmax(q) + 8) * sizeof(uint16_t), hb = (size_t)PM_TILE * (l.m + 8) * sizeof(uint16_t);
    const size_t fb = (size_t)l.m * PM_LD * sizeof(float);
    return (xb + hb > fb ? xb + hb : fb) + (size_t)PM_MAX_OUT * PM_TILE * sizeof(float);
}

#ifdef HK_POLICY_KERNELS
// Wf_ih (hh == 0) or Wf_hh from the CURRENT fp32 group-major inference copy, each weight rounded once: element
// (((ub * 4 + g) * nsteps + s) * 64 + lane) * 8 + j = W[gate column g m + 32 ub + (lane & 31)][k = 16 s + 8 (lane >> 5) + j], +0.0 where k >= K
__global__ __launch_bounds__(256) void policy_lstm_bf16_build_kernel(PolicyLstm L, PolicyLstmBf16 B, int H, int hh)
{
    const int m = L.m, N = 4 * m, K = hh ? m : H;
    const int nsteps = ((K + 63) & ~63) >> 4;
    const int nsk = hh ? m >> 4 : nsteps;                     // W_hh: m / 16 whole steps, no padding
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * nsk * 16) return;
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    const int s = (int)((idx >> 9) % nsk), ug = (int)((idx >> 9) / nsk);
    const int g = ug & 3, ub = ug >> 2;
    const int k = 16 * s + 8 * (lane >> 5) + j, col = g * m + 32 * ub + (lane & 31);
    const float* wq = reinterpret_cast<const float*>(hh ? L.Wq_hh : L.Wq_ih);
    const_cast<uint16_t*>(hh ? B.Wf_hh : B.Wf_ih)[idx] = k < K ? ppo_bf16_rne(wq[pm_wq_index(k >> 3, k & 1, col, (k & 7) >> 1, N)]) : (uint16_t)0;
}

// (re)build both copies on `stream` — the first switch to HK_POLICY_PREC_BF16, hk_ppo_publish and hk_policy_pool_load, after the fp32 copies
// are written (out of line, in the unit that has the kernel; hk_train.hip sees the declaration alone)
__attribute__((visibility("hidden"))) hipError_t policy_lstm_bf16_refresh(const PolicyParams& q, const PolicyLstm& l, const PolicyLstmBf16& b, hipStream_t stream)
{
    const size_t n_ih = policy_lstm_bf16_ih_elems(q, l), n_hh = policy_lstm_bf16_hh_elems(l);
    hipLaunchKernelGGL(policy_lstm_bf16_build_kernel, dim3((unsigned)((n_ih + 255) / 256)), dim3(256), 0, stream, l, b, q.hidden, 0);
    hipLaunchKernelGGL(policy_lstm_bf16_build_kernel, dim3((unsigned)((n_hh + 255) / 256)), dim3(256), 0, stream, l, b, q.hidden, 1);
    return hipGetLastError();
}

// One wave's share of the gate products over ns k-steps: z[g] += A[32 rows][16 ns] * B_g[16 ns][32 units], g = i, f, g, o.  ap: this lane's first
// 8 elements of its row (LDS); bp: this lane's 16 bytes of gate i's first step (64 x 16 bytes per step), gate g another g * ns steps on.  The
// four B operands of step s + 1 are in flight while step s multiplies: four MFMAs of 32 cycles on four independent accumulators.
__device__ __forceinline__ void plb_gemm4(f32x16 (&z)[4], const uint16_t* ap, const pm_bf16x8* __restrict__ bp, int ns)
{
    pm_bf16x8 Ba[4], Bb[4];
    auto ldB = [&](int s, pm_bf16x8 (&x)[4]) {
#pragma unroll
        for (int g = 0; g < 4; g++) x[g] = bp[((size_t)g * ns + s) * 64];
    };
    auto mm = [&](int s, const pm_bf16x8 (&y)[4]) {
        const pm_bf16x8 a = *reinterpret_cast<const pm_bf16x8*>(ap + s * 16);
#pragma unroll
        for (int g = 0; g < 4; g++) z[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, y[g], z[g], 0, 0, 0);
    };
    ldB(0, Ba);
    for (int s = 0; s < ns; s += 2) {                     // ns is even (K a multiple of 32)
        ldB(s + 1, Bb);
        mm(s, Ba);
        if (s + 2 < ns) ldB(s + 2, Ba);
        mm(s + 1, Bb);
    }
}

// Arguments as policy_lstm_kernel's, and the bf16 weight copies of the trunk (B) and of the cell (LB).  TWO: hidden > 128, as policy_mlp_bf16_kernel;
// its two trunk accumulators beside the ring of B operands do not fit 128 registers without a spill, so that form is built for two waves per SIMD
// (one workgroup per CU, as policy_lstm_kernel), the hidden <= 128 form — the reference's 128 x 3 — for four (two workgroups per CU).
template <bool TWO>
__global__ __launch_bounds__(PM_THREADS, TWO ? 2 : 4) void policy_lstm_bf16_kernel(PolicyParams Q, PolicyBf16 B, PolicyLstm L, PolicyLstmBf16 LB, float* mem, int rows,
                                                                         const float* src, int w, unsigned long long decision, int env_id_base, int A,
                                                                         float* mu_out, float* logit_out, float* act_steer, int* act_branch, PolicyRec rec)
{
    extern __shared__ __align__(16) float At[];        // X (bf16 [PM_TILE][LD]), Hb (bf16 [PM_TILE][LDH]) / Ht (fp32 [m][PM_LD]), then head[PM_MAX_OUT][PM_TILE]
    uint16_t* X = reinterpret_cast<uint16_t*>(At);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PM_TILE;
    const int K0 = Q.in_dim, H = Q.hidden, m = L.m;
    const int K0p = (K0 + 63) & ~63, Hp = (H + 63) & ~63;
    const int kc0 = K0p < PMB_KC ? K0p : PMB_KC;
    const int kmax = kc0 > Hp ? kc0 : Hp;
    const int LD = kmax + 8, LDH = m + 8;
    const size_t xb = (size_t)PM_TILE * LD * sizeof(uint16_t), hb = (size_t)PM_TILE * LDH * sizeof(uint16_t), fb = (size_t)m * PM_LD * sizeof(float);
    uint16_t* Hb = X + (size_t)PM_TILE * LD;
    float* Ht = At;
    float* head = At + (xb + hb > fb ? xb + hb : fb) / sizeof(float);

    // ---- h of the tile's rows, rounded once: a lane owns two consecutive units (one packed dword), waves run over rows
    for (int r = wave; r < PM_TILE; r += PM_THREADS / 64) {
        const bool rowok = row0 + r < rows;
        const float* mrow = mem + (size_t)(row0 + r) * 2 * m;
        for (int k = 2 * lane; k < m; k += 128) {
            const float2 v = rowok ? *reinterpret_cast<const float2*>(mrow + k) : make_float2(0.0f, 0.0f);
            *reinterpret_cast<uint32_t*>(Hb + (size_t)r * LDH + k) = (uint32_t)ppo_bf16_rne(v.x) | ((uint32_t)ppo_bf16_rne(v.y) << 16);
        }
    }

    const int ncb = H >> 5;
    const int half = lane >> 5, c = lane & 31;
    const bool has = TWO ? wave < ncb : wave < 2 * ncb;
    const int cb = TWO ? wave : wave % ncb;
    const int rb0 = TWO ? 0 : wave / ncb;
    const uint16_t* a0p = X + (size_t)(rb0 * 32 + c) * LD + half * 8;
    const uint16_t* a1p = X + (size_t)(32 + c) * LD + half * 8;

    // ---- the trunk: policy_mlp_bf16_kernel's text, every layer's post-activation rounded into X
    for (int l = 0; l < Q.n_layers; l++) {
        const int Kp = l == 0 ? K0p : Hp;
        f32x16 acc0, acc1;
        {
            const float bias = has ? Q.b[l][cb * 32 + c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) { acc0[r] = bias; acc1[r] = bias; }
        }
        const pm_bf16x8* wf = reinterpret_cast<const pm_bf16x8*>(B.Wf[l]) + (size_t)cb * (Kp >> 4) * 64 + lane;
        for (int kb = 0; kb < Kp; kb += PMB_KC) {
            const int kc = (Kp - kb) < PMB_KC ? (Kp - kb) : PMB_KC;      // a multiple of 64
            if (l == 0) {
                if (kb > 0) __syncthreads();                      // the previous chunk has been consumed
                constexpr int MMAX = (PMB_KC / 2 + 63) / 64;
                int soff[MMAX][2];
                float mean[MMAX][2], sdev[MMAX][2];
#pragma unroll
                for (int mm = 0; mm < MMAX; mm++)
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const int kl = 2 * (lane + 64 * mm) + e, k = kb + kl;
                        soff[mm][e] = -1; mean[mm][e] = 0.0f; sdev[mm][e] = 1.0f;
                        if (kl < kc && k < K0) {
                            soff[mm][e] = pm_ring_offset(Q, w, k);
                            if (Q.normalize) { mean[mm][e] = Q.mean[k]; sdev[mm][e] = Q.std[k]; }
                        }
                    }
                for (int r = wave; r < PM_TILE; r += PM_THREADS / 64) {
                    const bool rowok = row0 + r < rows;
                    const float* srow = src + (size_t)(row0 + r) * K0;
                    float v[MMAX][2];
#pragma unroll
                    for (int mm = 0; mm < MMAX; mm++)
#pragma unroll
                        for (int e = 0; e < 2; e++) v[mm][e] = (rowok && soff[mm][e] >= 0) ? srow[soff[mm][e]] : 0.0f;
#pragma unroll
                    for (int mm = 0; mm < MMAX; mm++) {
                        const int kl = 2 * (lane + 64 * mm);
                        if (kl >= kc) continue;
                        uint32_t pk = 0u;
#pragma unroll
                        for (int e = 0; e < 2; e++) {
                            float x = v[mm][e];
                            if (Q.normalize && rowok && soff[mm][e] >= 0) x = pm_normalise(x, mean[mm][e], sdev[mm][e]);
                            pk |= (uint32_t)ppo_bf16_rne(x) << (16 * e);
                        }
                        *reinterpret_cast<uint32_t*>(X + (size_t)r * LD + kl) = pk;
                    }
                }
                __syncthreads();
            }
            if (has) {
                const pm_bf16x8* bp = wf + (size_t)(kb >> 4) * 64;
                pmb_gemm<TWO>(acc0, acc1, a0p, a1p, bp, kc >> 4);      // (a chunk sits at the start of X)
            }
        }
        if (has) {
#pragma unroll
            for (int r = 0; r < 16; r++) { acc0[r] = swish(acc0[r]); if (TWO) acc1[r] = swish(acc1[r]); }
        }
        __syncthreads();            // every wave has finished reading this layer's input
        // C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        if (has) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = (r & 3) + 8 * (r >> 2) + 4 * half;
                X[(size_t)(rb0 * 32 + rr) * LD + cb * 32 + c] = ppo_bf16_rne(acc0[r]);
                if (TWO) X[(size_t)(32 + rr) * LD + cb * 32 + c] = ppo_bf16_rne(acc1[r]);
            }
        }
        // hidden = 32 (mod 64): the next product's chunk is padded to 64 with +0.0, as the product kernel stages it
        if (H & 32)
            for (int x = tid; x < PM_TILE * 32; x += PM_THREADS) X[(size_t)(x >> 5) * LD + H + (x & 31)] = (uint16_t)0;
        __syncthreads();
    }

    // ---- the cell: wave -> (row block rbc, unit block ub), as policy_lstm_kernel
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
        const int ns_ih = Hp >> 4, ns_hh = m >> 4;
        plb_gemm4(z, X + (size_t)(rbc * 32 + c) * LD + half * 8, reinterpret_cast<const pm_bf16x8*>(LB.Wf_ih) + (size_t)ub * 4 * ns_ih * 64 + lane, ns_ih);
        plb_gemm4(z, Hb + (size_t)(rbc * 32 + c) * LDH + half * 8, reinterpret_cast<const pm_bf16x8*>(LB.Wf_hh) + (size_t)ub * 4 * ns_hh * 64 + lane, ns_hh);
    }
    __syncthreads();                // every wave has finished reading a and h: Ht goes over them
    if (hasc) {
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
#else
__attribute__((visibility("hidden"))) hipError_t policy_lstm_bf16_refresh(const PolicyParams& q, const PolicyLstm& l, const PolicyLstmBf16& b, hipStream_t stream);
#endif  /* HK_POLICY_KERNELS */

}  // namespace hk
