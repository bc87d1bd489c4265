// hk_policy_bf16.h — HK_POLICY_PREC_BF16: the decision of policy_mlp_kernel with the trunk on v_mfma_f32_32x32x16_bf16 (contract in
// include/hk.h beside hk_policy_attach).  Included by hk_policy.h, whose loader rule, normaliser and tail it uses.
//
// The arithmetic is, operand for operand, the bf16 trainer's forward (hk_ppo.h: ppo_gather_kernel<uint16_t>, ppo_gemm_bf16_kernel<1>): the
// input normalised in fp32 (pm_normalise) and rounded once (ppo_bf16_rne), the weights rounded once, every layer an fp32 accumulator seeded
// with the fp32 bias and stepped in ascending k, lane half h of a step holding k = 16 s + 8 h + j, K padded with +0.0 to whole chunks of
// 64 — NO step is skipped, the all-zero ones of the padding included, so the sequence of matrix instructions an output element sees is the
// product kernel's, and since an MFMA's result in one element depends only on that element's row of A, column of B and accumulator input, the
// pre-activations are the product kernel's bits whatever the tiling.  Post-activations below the last layer are rounded once to bf16; the
// last layer's stays fp32 and feeds pm_tail, the fp32 kernel's own tail.
//
// One workgroup (8 waves) per tile of 64 rows, one launch per decision; activations never leave LDS:
//   X  bf16 [row][k], k contiguous, row stride LD = kmax + 8 elements (kmax = the widest padded operand, a multiple of 64): 2 kmax + 16
//      bytes = 4 (kmax / 8 + 1) dwords, an odd multiple of four, so the 16-byte operand reads (ds_read_b128) of 16 consecutive rows cover the
//      64 banks once — PB_LD's rule (144 B at K = 64; 528 B at 256, 656 B at 320).
//   The epilogue holds a column per lane and rows in its registers (C/D layout), so register r of a wave is 32 consecutive k (16 dwords,
//      two lanes to a dword) at one row for each lane half; the halves are 4 rows = 8 kmax + 64 bytes apart, i.e. 16 banks modulo 64: the
//      64 lanes of one store touch 32 different banks, none twice except the two halves of a dword.
//   F  the last layer's fp32 post-activations, [k][PM_LD] as the fp32 kernel keeps them (pm_tail reads that), written over X after the
//      layer's barrier.  LDS = max(hidden x 65 x 4, 64 x LD x 2) + the heads' 2 KB: 68 608 B at hidden = 256, the fp32 kernel's figure.
// Weights: a B operand is 8 consecutive k of one output column per lane.  policy_bf16_build_kernel lays each layer out fragment-major,
// [column block][k step][lane][8] (PolicyBf16::Wf): one MFMA's B operand is 1 KB, one coalesced 16-byte load per lane, zero where k >= K.
// A wave owns one column block (hidden > 128: both row blocks of it, sharing the B operand; else one of the two) and keeps the B operands of
// the next eight steps in flight (pmb_gemm).
#pragma once

namespace hk {

constexpr int PMB_KC = 320;                 // layer-0 inputs staged per chunk (whole 64-wide chunks of the product kernel)
typedef __bf16 pm_bf16x8 __attribute__((ext_vector_type(8)));

inline int pmb_pad64(int k) { return (k + 63) & ~63; }
inline int pmb_kmax(const PolicyParams& q)
{
    const int k0 = pmb_pad64(q.in_dim) < PMB_KC ? pmb_pad64(q.in_dim) : PMB_KC, hp = pmb_pad64(q.hidden);
    return k0 > hp ? k0 : hp;
}
inline size_t policy_bf16_lds_bytes(const PolicyParams& q)
{
    const size_t xb = (size_t)PM_TILE * (pmb_kmax(q) + 8) * sizeof(uint16_t), fb = (size_t)q.hidden * PM_LD * sizeof(float);
    return (xb > fb ? xb : fb) + (size_t)PM_MAX_OUT * PM_TILE * sizeof(float);
}
// elements of layer l's fragment-major copy
inline size_t policy_bf16_layer_elems(const PolicyParams& q, int l) { return (size_t)q.hidden * pmb_pad64(l == 0 ? q.in_dim : q.hidden); }

// Wf[l] from the CURRENT fp32 inference copy Wt[l] ([k][hidden]), each weight rounded once: element ((cb * nsteps + s) * 64 + lane) * 8 + j
// = W[k = 16 s + 8 (lane >> 5) + j][col = 32 cb + (lane & 31)], +0.0 where k >= K.  One thread per element.
#ifdef HK_POLICY_KERNELS
__global__ __launch_bounds__(256) void policy_bf16_build_kernel(PolicyParams Q, PolicyBf16 B, int l)
{
    const int H = Q.hidden, K = l == 0 ? Q.in_dim : H;
    const int nsteps = ((K + 63) & ~63) >> 4;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)H * nsteps * 16) return;
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    const int s = (int)((idx >> 9) % nsteps), cb = (int)((idx >> 9) / nsteps);
    const int k = 16 * s + 8 * (lane >> 5) + j, col = 32 * cb + (lane & 31);
    const_cast<uint16_t*>(B.Wf[l])[idx] = k < K ? ppo_bf16_rne(Q.Wt[l][(size_t)k * H + col]) : (uint16_t)0;
}

// (re)build every layer's copy on `stream` — the switch to HK_POLICY_PREC_BF16 and hk_ppo_publish, after the fp32 copies are written
// (out of line, in the unit that has the kernel; hk_train.hip sees the declaration alone)
__attribute__((visibility("hidden"))) hipError_t policy_bf16_refresh(const PolicyParams& q, const PolicyBf16& bq, hipStream_t stream)
{
    for (int l = 0; l < q.n_layers; l++) {
        const size_t n = policy_bf16_layer_elems(q, l);
        hipLaunchKernelGGL(policy_bf16_build_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, q, bq, l);
    }
    return hipGetLastError();
}
#else
__attribute__((visibility("hidden"))) hipError_t policy_bf16_refresh(const PolicyParams& q, const PolicyBf16& bq, hipStream_t stream);
#endif  /* HK_POLICY_KERNELS */

// One wave's share of a layer over ns k-steps (a multiple of 4): acc0 (+ acc1 when TWO) += A[32 rows][16 ns] * B[16 ns][32 cols].  a?p: this
// lane's first 8 elements of its row of X; bp: this lane's 16 bytes of the first step's B operand (64 x 16 bytes per step).  The B loads run
// through a ring of eight operands: step s multiplies B[s % 8] and then refills it with step s + 8, so a load has seven steps of lead, 7 or
// 14 MFMAs of 32 cycles.  (pm_gemm's lead for fp32 is three groups of 8 MFMAs x 64 cycles; the same distance in time here would take a
// ring of 24 or 48 operands, which four waves per SIMD have no registers for: what the ring does not cover is the other three waves' of
// the SIMD to hide, and all layers' copies together are <= 0.3 MB of L2.)  The A operands are LDS reads the compiler schedules within a step.
template <bool TWO>
__device__ __forceinline__ void pmb_gemm(f32x16& acc0, f32x16& acc1, const uint16_t* a0p, const uint16_t* a1p, const pm_bf16x8* __restrict__ bp, int ns)
{
    pm_bf16x8 B[8];
#pragma unroll
    for (int j = 0; j < 8; j++) if (j < ns) B[j] = bp[(size_t)j * 64];
    for (int s0 = 0; s0 < ns; s0 += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (j == 4 && s0 + 4 >= ns) break;
            const int s = s0 + j;
            const pm_bf16x8 a0 = *reinterpret_cast<const pm_bf16x8*>(a0p + s * 16);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, B[j], acc0, 0, 0, 0);
            if (TWO) {
                const pm_bf16x8 a1 = *reinterpret_cast<const pm_bf16x8*>(a1p + s * 16);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, B[j], acc1, 0, 0, 0);
            }
            if (s + 8 < ns) B[j] = bp[(size_t)(s + 8) * 64];
        }
    }
}

// Arguments: policy_mlp_kernel's, and the bf16 weight copies.  TWO: hidden > 128 — wave = column block, both row blocks; else unit = wave -> (column block = unit %
// ncb, row block = unit / ncb), units >= 2 ncb idle.
template <bool TWO>
__global__ __launch_bounds__(PM_THREADS, 4) void policy_mlp_bf16_kernel(PolicyParams Q, PolicyBf16 B, int rows, const float* src, int w, unsigned long long decision,
                                                                        int env_id_base, int A, float* mu_out, float* logit_out, float* act_steer,
                                                                        int* act_branch, PolicyRec rec)
{
    extern __shared__ __align__(16) float At[];        // X (bf16 [PM_TILE][LD]) / F (fp32 [hidden][PM_LD]), then head[PM_MAX_OUT][PM_TILE]
    uint16_t* X = reinterpret_cast<uint16_t*>(At);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * PM_TILE;
    const int K0 = Q.in_dim, H = Q.hidden;
    const int K0p = (K0 + 63) & ~63, Hp = (H + 63) & ~63;
    const int kc0 = K0p < PMB_KC ? K0p : PMB_KC;
    const int kmax = kc0 > Hp ? kc0 : Hp;
    const int LD = kmax + 8;
    const size_t xb = (size_t)PM_TILE * LD * sizeof(uint16_t), fb = (size_t)H * PM_LD * sizeof(float);
    float* head = At + (xb > fb ? xb : fb) / sizeof(float);

    const int ncb = H >> 5;
    const int half = lane >> 5, c = lane & 31;
    const bool has = TWO ? wave < ncb : wave < 2 * ncb;
    const int cb = TWO ? wave : wave % ncb;
    const int rb0 = TWO ? 0 : wave / ncb;
    const uint16_t* a0p = X + (size_t)(rb0 * 32 + c) * LD + half * 8;
    const uint16_t* a1p = X + (size_t)(32 + c) * LD + half * 8;

    for (int l = 0; l < Q.n_layers; l++) {
        const int Kp = l == 0 ? K0p : Hp;
        const bool last = l == Q.n_layers - 1;
        f32x16 acc0, acc1;
        {
            const float bias = has ? Q.b[l][cb * 32 + c] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) { acc0[r] = bias; acc1[r] = bias; }
        }
        const pm_bf16x8* wf = reinterpret_cast<const pm_bf16x8*>(B.Wf[l]) + (size_t)cb * (Kp >> 4) * 64 + lane;
        // layer 0 streams its inputs through X in chunks of PMB_KC (the accumulators carry the chain across chunks); the later layers read
        // what the previous epilogue left in X
        for (int kb = 0; kb < Kp; kb += PMB_KC) {
            const int kc = (Kp - kb) < PMB_KC ? (Kp - kb) : PMB_KC;      // a multiple of 64
            if (l == 0) {
                if (kb > 0) __syncthreads();                      // the previous chunk has been consumed
                // ---- load + normalise + round the tile chunk.  A lane owns two consecutive k (one packed dword: consecutive lanes on consecutive
                // banks), waves run over rows; the per-k constants (ring offset, mean, std) are set up once.  k in [K0, K0p) is the +0.0 padding.
                constexpr int MMAX = (PMB_KC / 2 + 63) / 64;
                int soff[MMAX][2];
                float mean[MMAX][2], sdev[MMAX][2];
#pragma unroll
                for (int m = 0; m < MMAX; m++)
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const int kl = 2 * (lane + 64 * m) + e, k = kb + kl;
                        soff[m][e] = -1; mean[m][e] = 0.0f; sdev[m][e] = 1.0f;
                        if (kl < kc && k < K0) {
                            soff[m][e] = pm_ring_offset(Q, w, k);
                            if (Q.normalize) { mean[m][e] = Q.mean[k]; sdev[m][e] = Q.std[k]; }
                        }
                    }
                for (int r = wave; r < PM_TILE; r += PM_THREADS / 64) {
                    const bool rowok = row0 + r < rows;
                    const float* srow = src + (size_t)(row0 + r) * K0;
                    float v[MMAX][2];
#pragma unroll
                    for (int m = 0; m < MMAX; m++)
#pragma unroll
                        for (int e = 0; e < 2; e++) v[m][e] = (rowok && soff[m][e] >= 0) ? srow[soff[m][e]] : 0.0f;
#pragma unroll
                    for (int m = 0; m < MMAX; m++) {
                        const int kl = 2 * (lane + 64 * m);
                        if (kl >= kc) continue;
                        uint32_t pk = 0u;
#pragma unroll
                        for (int e = 0; e < 2; e++) {
                            float x = v[m][e];
                            if (Q.normalize && rowok && soff[m][e] >= 0) x = pm_normalise(x, mean[m][e], sdev[m][e]);
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
        if (!last) {
            if (has) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int rr = (r & 3) + 8 * (r >> 2) + 4 * half;
                    X[(size_t)(rb0 * 32 + rr) * LD + cb * 32 + c] = ppo_bf16_rne(acc0[r]);
                    if (TWO) X[(size_t)(32 + rr) * LD + cb * 32 + c] = ppo_bf16_rne(acc1[r]);
                }
            }
            // hidden = 32 (mod 64): the next layer's chunk is padded to 64 with +0.0, as the product kernel stages it
            if (H & 32)
                for (int x = tid; x < PM_TILE * 32; x += PM_THREADS) X[(size_t)(x >> 5) * LD + H + (x & 31)] = (uint16_t)0;
        } else if (has) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = (r & 3) + 8 * (r >> 2) + 4 * half;
                At[(size_t)(cb * 32 + c) * PM_LD + rb0 * 32 + rr] = acc0[r];
                if (TWO) At[(size_t)(cb * 32 + c) * PM_LD + 32 + rr] = acc1[r];
            }
        }
        __syncthreads();
    }
    pm_tail(Q, At, head, rows, row0, decision, env_id_base, A, mu_out, logit_out, act_steer, act_branch, rec, tid, H);
}

}  // namespace hk
