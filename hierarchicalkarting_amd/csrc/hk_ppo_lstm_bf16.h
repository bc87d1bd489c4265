// hk_ppo_lstm_bf16.h — device side of recurrent training in HK_PPO_PREC_BF16 (hk_ppo_recurrent_set_precision; contract in include/hk.h
// "RECURRENT ACTORS IN BF16", host side in hk_train.hip).  The host path is hk_ppo_lstm.h's: the trunk's last post-activation a, the
// bf16 h_prev and the gate deltas are PpoMat operands of the bf16 kind, so Zx = bsum + a W_ih^T, the recurrent delta dG_tau W_hh, da = dG W_ih and
// the two weight gradients all run on ppo_gemm_bf16_kernel through ppo_product / ppo_wgrad.  New here are the two kernels the step loop launches:
//   ppo_lstm_step_bf16_kernel   ppo_lstm_step_kernel with the gate chains continued from Zx over bf16 h on v_mfma_f32_32x32x16_bf16, m / 16 whole
//                               steps in ascending k — policy_lstm_bf16_kernel's chain, bit for bit; h is rounded once as it is staged, and the
//                               rounded h_prev is stored beside the fp32 one: it is the operand of dW_hh.  The cell is hk_lstm_cell, fp32.
//   ppo_lstm_back_bf16_kernel   ppo_lstm_back_kernel with the gate deltas rounded once into a bf16 buffer as they are made (the cell backward
//                               itself, dc and dh' stay fp32)
#pragma once
#include "hk_ppo_lstm.h"

namespace hk {

// Step tau.  A workgroup of 4 waves owns 64 sequences x 64 units; a wave one 32 x 32 block with the four gate accumulators of its units, seeded
// from Zx.  h goes through LDS in chunks of 64 k (the last one 32 when m = 32 mod 64: only its whole steps are issued), W_hh's four gate tiles
// beside it, both [row][k] with ppo_gemm_bf16_kernel's stride PB_LD, staged by its pb_fetch / pb_stage.
// Whh: bf16 [4m][m], torch layout (the HK_PPO_SHADOW elements).  htap == nullptr (the trainer): h comes from mem0 (tau == 0) or the previous step's
// hnew, zero where FIRST; the arguments are ppo_lstm_step_kernel's, and hprevb [M][m] receives the rounded h.  htap != nullptr (hk_ppo_lstm_gates_bf16):
// h is htap [ms][m] as given, the cell is left out and GZ returns the pre-activations.
__global__ __launch_bounds__(256) void ppo_lstm_step_bf16_kernel(int tau, int ms, int mc, const uint16_t* __restrict__ Whh, const float* __restrict__ mem0,
                                                                 const int* __restrict__ first, const uint16_t* __restrict__ htap, float* GZ, float* hnew,
                                                                 float* mbmem, float* hprev, uint16_t* hprevb, float* cprev)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[PB_TM * PB_LD], Bs[4][PB_TN * PB_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * PB_TM, u0 = blockIdx.x * PB_TN;
    const int wr = wave >> 1, wc = wave & 1, half = lane >> 5, c = lane & 31;
    const int unit = u0 + wc * 32 + c;
    const size_t rbase = (size_t)tau * ms;
    const int N = 4 * mc;
    const bool wvec = (reinterpret_cast<uintptr_t>(Whh) & 15) == 0;          // (m is a multiple of 32: every row of W_hh starts on 16 bytes when the matrix does)
    const bool hvec = htap && (reinterpret_cast<uintptr_t>(htap) & 15) == 0;
    f32x16 z[4];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int q = i0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool ok = q < ms && unit < mc;
        const float* zx = GZ + (rbase + (ok ? q : 0)) * N + (ok ? unit : 0);
#pragma unroll
        for (int g = 0; g < 4; g++) z[g][r] = ok ? zx[(size_t)g * mc] : 0.0f;
    }
    for (int kb = 0; kb < mc; kb += PB_TK) {
        const int kw = mc - kb < PB_TK ? mc - kb : PB_TK;          // 64, or 32 in the last chunk
        uint4 v[2];
        if (htap) pb_fetch(v, htap, mc, true, hvec, i0, ms, kb, mc, tid);
        else {
            // this thread's two pieces of 8 consecutive k of one sequence: read in fp32, rounded once, stored as the row's h_prev in both kinds
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const int x = tid + 256 * p;
                const int q = i0 + (x >> 3), k = kb + (x & 7) * 8;
                uint4 pk = make_uint4(0u, 0u, 0u, 0u);
                if (q < ms && k < mc) {
                    const size_t row = rbase + q;
                    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
                    if (!first[row]) {
                        const float* hp = tau == 0 ? mem0 + (size_t)q * 2 * mc + k : hnew + (row - ms) * mc + k;
                        lo = *reinterpret_cast<const float4*>(hp);
                        hi = *reinterpret_cast<const float4*>(hp + 4);
                    }
                    pk = make_uint4((uint32_t)ppo_bf16_rne(lo.x) | ((uint32_t)ppo_bf16_rne(lo.y) << 16), (uint32_t)ppo_bf16_rne(lo.z) | ((uint32_t)ppo_bf16_rne(lo.w) << 16),
                                    (uint32_t)ppo_bf16_rne(hi.x) | ((uint32_t)ppo_bf16_rne(hi.y) << 16), (uint32_t)ppo_bf16_rne(hi.z) | ((uint32_t)ppo_bf16_rne(hi.w) << 16));
                    if (blockIdx.x == 0) {
                        *reinterpret_cast<float4*>(hprev + row * mc + k) = lo;
                        *reinterpret_cast<float4*>(hprev + row * mc + k + 4) = hi;
                        *reinterpret_cast<uint4*>(hprevb + row * mc + k) = pk;
                    }
                }
                v[p] = pk;
            }
        }
        pb_stage(As, v, true, tid);
#pragma unroll
        for (int g = 0; g < 4; g++) {
            pb_fetch(v, Whh + (size_t)g * mc * mc, mc, true, wvec, u0, mc, kb, mc, tid);
            pb_stage(Bs[g], v, true, tid);
        }
        __syncthreads();
        // operand maps of 32x32x16: lane (r = lane & 31, h = lane >> 5) holds A[r][8 h + j] and B[8 h + j][r], j = 0 .. 7
        const uint16_t* ap = As + (wr * 32 + c) * PB_LD + half * 8;
        const int bo = (wc * 32 + c) * PB_LD + half * 8;
        for (int s = 0; s < (kw >> 4); s++) {
            const ppo_bf16x8 a = *reinterpret_cast<const ppo_bf16x8*>(ap + s * 16);
#pragma unroll
            for (int g = 0; g < 4; g++)
                z[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, *reinterpret_cast<const ppo_bf16x8*>(Bs[g] + bo + s * 16), z[g], 0, 0, 0);
        }
        __syncthreads();
    }
    if (unit >= mc) return;
    // C/D layout: col (unit) = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int q = i0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (q >= ms) continue;
        const size_t row = rbase + q;
        float* gz = GZ + row * N + unit;
        if (htap) {
#pragma unroll
            for (int g = 0; g < 4; g++) gz[(size_t)g * mc] = z[g][r];
            continue;
        }
        float c0 = 0.0f;
        if (!first[row]) c0 = tau == 0 ? mem0[(size_t)q * 2 * mc + mc + unit] : mbmem[(row - ms) * 2 * mc + mc + unit];
        float hn, cn;
        hk_lstm_cell(z[0][r], z[1][r], z[2][r], z[3][r], c0, &hn, &cn);
        gz[0] = hk_sigmoidf(z[0][r]);
        gz[(size_t)mc] = hk_sigmoidf(z[1][r]);
        gz[(size_t)2 * mc] = hk_tanhf_fast(z[2][r]);
        gz[(size_t)3 * mc] = hk_sigmoidf(z[3][r]);
        hnew[row * mc + unit] = hn;
        mbmem[row * 2 * mc + unit] = hn;
        mbmem[row * 2 * mc + mc + unit] = cn;
        cprev[row * mc + unit] = c0;
    }
}

// Step tau of the backward: ppo_lstm_back_kernel's text, the gate deltas rounded once into GZb [M][4m] (bf16) as they are made.  GZ keeps the gate
// outputs; the products and the bias gradient read GZb.
__global__ __launch_bounds__(256) void ppo_lstm_back_bf16_kernel(int tau, int ms, int mc, int last, const int* __restrict__ first, const float* __restrict__ dH,
                                                                 const float* __restrict__ drec, const float* __restrict__ mbmem, const float* __restrict__ cprev,
                                                                 const float* __restrict__ GZ, uint16_t* GZb, float* dcar)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)ms * mc) return;
    const int q = (int)(idx / mc), u = (int)(idx % mc);
    const size_t row = (size_t)tau * ms + q;
    const bool carry = !last && !first[row + ms];
    const float dh = dH[row * mc + u] + (carry ? drec[idx] : 0.0f);
    const float* gz = GZ + row * 4 * mc + u;
    uint16_t* gb = GZb + row * 4 * mc + u;
    float dz[4], dcp;
    hk_lstm_cell_back(dh, carry ? dcar[idx] : 0.0f, gz[0], gz[(size_t)mc], gz[(size_t)2 * mc], gz[(size_t)3 * mc], mbmem[row * 2 * mc + mc + u],
                      cprev[row * mc + u], dz, &dcp);          // (hk_lstm_train.h)
    gb[0] = ppo_bf16_rne(dz[0]);
    gb[(size_t)mc] = ppo_bf16_rne(dz[1]);
    gb[(size_t)2 * mc] = ppo_bf16_rne(dz[2]);
    gb[(size_t)3 * mc] = ppo_bf16_rne(dz[3]);
    dcar[idx] = dcp;
}

}  // namespace hk
