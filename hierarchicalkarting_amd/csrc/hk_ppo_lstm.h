// hk_ppo_lstm.h — device side of recurrent training: PPO with truncated BPTT through the actor's LSTM cell (contract in include/hk.h
// "PPO trainer" RECURRENT, host side in hk_train.hip).  A minibatch is ms sequences of L = sequence_length rows, gathered
// TIME-MAJOR: row = tau ms + q, so the rows of one time step are a contiguous block and everything that is not recurrent — the gather, the
// trunk, the critic, the loss, the weight gradients — runs once over all M = L ms rows on hk_ppo.h's kernels.  New here:
//   ppo_lstm_expand_kernel      sequence ids -> per-row ids (-1: a dead row or a skipped sequence), the rows' FIRST words and the windows'
//                               initial memory MEMORY[k L] (a constant of the minibatch)
//   ppo_lstm_bsum_kernel        the gate bias the forward uses, fp32 b_ih + b_hh as policy_lstm_upload forms it
//   (Zx = bsum + a W_ih^T is ppo_gemm_kernel<0> seeded with bsum: the first part of the inference chain, stored to fp32 memory, which is lossless)
//   ppo_lstm_step_kernel        launched L times in stream order: the four gate chains of the step's ms rows continued from Zx over h on
//                               v_mfma_f32_32x32x2_f32 in ascending k — policy_lstm_kernel's chain, bit for bit — and hk_lstm_cell as an
//                               epilogue on the C/D layout.  h / c come from the previous step's output, from MEMORY[k L] at tau = 0, and are
//                               exactly zero where FIRST.  Stores the gate outputs (over Zx), h', c', and the h / c it read.
//   ppo_lstm_head_back_kernel   dh' = dhead [W_mu; W_branch] (the heads read h', so there is no swish')
//   ppo_lstm_back_kernel        launched L times in reverse: the cell backward of the step's rows from the stored gate outputs; the gate deltas
//                               replace the gate outputs, dc is carried in place.  The recurrent delta dG_tau W_hh is ppo_gemm_kernel<0> on
//                               them (a second launch per step); both carried deltas are dropped where FIRST of the row they come from is set.
//   ppo_lstm_stats_kernel       ppo_stats_kernel with stats[5] counting skipped SEQUENCES (the means stay over the valid rows)
//   ppo_lstm_publish_kernel     master cell parameters and the m-wide heads <-> the policy's group-major Wq_ih / Wq_hh, summed bias and heads
// No float atomics, every sum in a fixed order: the same call on the same state gives the same bits.
#pragma once
#include "hk_ppo.h"
#include "hk_policy_lstm.h"
#include "hk_lstm_train.h"

namespace hk {

// where the cell and the m-wide heads sit in the flat actor vector (PARAMS offsets), behind the trunk (PpoNet's oW / ob)
struct PpoLstmNet {
    int m = 0, hidden = 0, n_branch = 0;
    size_t oWih = 0, oWhh = 0, obih = 0, obhh = 0;      // W_ih [4m][H], W_hh [4m][m], b_ih [4m], b_hh [4m]: torch layout, gates i f g o
    size_t oWmu = 0, obmu = 0, ols = 0, oWbr = 0, obbr = 0, end = 0;
    void layout(int H, int mc, int nb, size_t base)
    {
        m = mc; hidden = H; n_branch = nb;
        size_t o = base;
        oWih = o; o += (size_t)4 * mc * H;
        oWhh = o; o += (size_t)4 * mc * mc;
        obih = o; o += (size_t)4 * mc;
        obhh = o; o += (size_t)4 * mc;
        oWmu = o; o += mc;
        obmu = o; o += 1;
        ols = o; o += 1;
        oWbr = o; o += (size_t)nb * mc;
        obbr = o; o += nb;
        end = o;
    }
};

// One thread per row (tau, q) of the minibatch, then one per element of the windows' initial memory [ms][2m].
// Sequence id s = (k E + e) S + j: window k of agent (e, j), rows t = k L + tau < R; a row with t >= R is dead, an id outside [0, n_seq) skips
// its whole sequence: row id -1, FIRST 0, initial memory 0.
__global__ __launch_bounds__(256) void ppo_lstm_expand_kernel(PpoRows P, const float* __restrict__ memory, int mem_max, const int* __restrict__ sids, int ms,
                                                              int L, int n_seq, int mc, int* rowids, int* first, float* mem0)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t M = (size_t)L * ms;
    const int ES = P.E * P.S;
    if (idx < M) {
        const int tau = (int)(idx / ms), q = (int)(idx % ms);
        const int sid = sids[q];
        int t = 0, fr = 0;
        const int rid = hk_seq_row(sid, tau, L, P.R, ES, n_seq, &t);          // (hk_lstm_train.h)
        if (rid >= 0) {
            const int rem = rid - t * ES, e = rem / P.S, j = rem - e * P.S;
            fr = P.first[((size_t)t * P.E + e) * P.A + P.slots[j]] != 0;
        }
        rowids[idx] = rid; first[idx] = fr;
        return;
    }
    const size_t y = idx - M;
    if (y >= (size_t)ms * 2 * mc) return;
    const int q = (int)(y / (2 * mc)), x = (int)(y % (2 * mc));
    const int sid = sids[q];
    float v = 0.0f;
    if (sid >= 0 && sid < n_seq) {
        const int k = sid / ES, rem = sid - k * ES, e = rem / P.S, j = rem - e * P.S;
        v = memory[(((size_t)k * L * P.E + e) * P.A + P.slots[j]) * mem_max + x];       // (k L < R for every k < ceil(R / L))
    }
    mem0[y] = v;
}

__global__ __launch_bounds__(256) void ppo_lstm_bsum_kernel(const float* b_ih, const float* b_hh, int n, float* bsum)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) bsum[k] = b_ih[k] + b_hh[k];
}

// Step tau.  A workgroup of 4 waves owns 64 sequences x 64 units; a wave one 32 x 32 block with FOUR accumulators, the i / f / g / o columns of
// its units (policy_lstm_kernel's arrangement), seeded from Zx.  h runs through LDS in chunks of 32 as ppo_gemm_kernel's operands do (tiles
// k-major, row stride 65), each chunk as MFMA 32x32x2 steps in ascending k, lane half h supplying k0 + h.  m is a multiple of 32: every chunk is whole.
// GZ [M][4m]: Zx of the step's rows on entry, their gate outputs i f g~ o on return (each element is read and written by the one lane that owns it).
// hnew [M][m], mbmem [M][2m] = [h' | c'], hprev / cprev [M][m]: the h / c the row read, after the reset.
__global__ __launch_bounds__(256) void ppo_lstm_step_kernel(int tau, int ms, int mc, const float* __restrict__ Whh, const float* __restrict__ mem0,
                                                            const int* __restrict__ first, float* GZ, float* hnew, float* mbmem, float* hprev, float* cprev)
{
    __shared__ float As[PPO_TK * PPO_LD], Bs[4][PPO_TK * PPO_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * PPO_TM, u0 = blockIdx.x * PPO_TN;
    const int wr = wave >> 1, wc = wave & 1, half = lane >> 5, c = lane & 31;
    const int unit = u0 + wc * 32 + c;
    const size_t rbase = (size_t)tau * ms;
    const int N = 4 * mc;
    f32x16 z[4];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int q = i0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool ok = q < ms && unit < mc;
        const float* zx = GZ + (rbase + (ok ? q : 0)) * N + (ok ? unit : 0);
#pragma unroll
        for (int g = 0; g < 4; g++) z[g][r] = ok ? zx[(size_t)g * mc] : 0.0f;
    }
    for (int kb = 0; kb < mc; kb += PPO_TK) {
        for (int x = tid; x < PPO_TK * PPO_TM; x += 256) {
            const int kk = x & 31, ii = x >> 5;
            const int q = i0 + ii, k = kb + kk;
            float v = 0.0f;
            if (q < ms) {
                const size_t row = rbase + q;
                if (!first[row]) v = tau == 0 ? mem0[(size_t)q * 2 * mc + k] : hnew[(row - ms) * mc + k];
                if (blockIdx.x == 0) hprev[row * mc + k] = v;
            }
            As[kk * PPO_LD + ii] = v;
        }
#pragma unroll
        for (int g = 0; g < 4; g++)
            for (int x = tid; x < PPO_TK * PPO_TN; x += 256) {
                const int kk = x & 31, jj = x >> 5;
                const int u = u0 + jj;
                Bs[g][kk * PPO_LD + jj] = u < mc ? Whh[((size_t)g * mc + u) * mc + kb + kk] : 0.0f;
            }
        __syncthreads();
        const float* ap = As + half * PPO_LD + wr * 32 + c;
        const int bo = half * PPO_LD + wc * 32 + c;
        for (int s = 0; s < PPO_TK / 2; s++) {
            const float a = ap[2 * s * PPO_LD];
#pragma unroll
            for (int g = 0; g < 4; g++) z[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[g][bo + 2 * s * PPO_LD], z[g], 0, 0, 0);
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
        float c0 = 0.0f;
        if (!first[row]) c0 = tau == 0 ? mem0[(size_t)q * 2 * mc + mc + unit] : mbmem[(row - ms) * 2 * mc + mc + unit];
        float hn, cn;
        hk_lstm_cell(z[0][r], z[1][r], z[2][r], z[3][r], c0, &hn, &cn);
        float* gz = GZ + row * N + unit;
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

// dh'[i][u] = sum_o dhead[i][o] W_head[o][u] over all M rows (vector ALU; n_out <= PM_MAX_OUT), ppo_head_back_row without the swish'
__global__ __launch_bounds__(256) void ppo_lstm_head_back_kernel(int M, int mc, int n_out, const float* dhead, int ldd, const float* W0, const float* W1, float* dH)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)M * mc) return;
    const size_t i = idx / mc;
    const int u = (int)(idx % mc);
    float s = dhead[i * ldd] * W0[u];
    for (int o = 1; o < n_out; o++) s += dhead[i * ldd + o] * W1[(size_t)(o - 1) * mc + u];
    dH[idx] = s;
}

// Step tau of the backward, one thread per (q, unit).  dh = the heads' delta of the row + the recurrent delta drec from tau + 1; dc = the carried
// dc from tau + 1 + dh o tanh'(c'); both carried parts are dropped where FIRST of row tau + 1 is set (that row read zeros, not this row's output)
// and at the last step (last != 0).  sigma' = s (1 - s) and tanh' = 1 - t^2 from the stored gate outputs; tanh(c') from the stored c'.
// GZ: the gate outputs on entry, the gate pre-activations' deltas on return.  dcar [ms][m]: dc f, what step tau - 1 adds to its dc.
// A dead row has dH == 0 and nothing carried into it, so every delta it writes is a zero.
__global__ __launch_bounds__(256) void ppo_lstm_back_kernel(int tau, int ms, int mc, int last, const int* __restrict__ first, const float* __restrict__ dH,
                                                            const float* __restrict__ drec, const float* __restrict__ mbmem, const float* __restrict__ cprev,
                                                            float* GZ, float* dcar)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)ms * mc) return;
    const int q = (int)(idx / mc), u = (int)(idx % mc);
    const size_t row = (size_t)tau * ms + q;
    const bool carry = !last && !first[row + ms];
    const float dh = dH[row * mc + u] + (carry ? drec[idx] : 0.0f);
    float* gz = GZ + row * 4 * mc + u;
    float dz[4], dcp;
    hk_lstm_cell_back(dh, carry ? dcar[idx] : 0.0f, gz[0], gz[(size_t)mc], gz[(size_t)2 * mc], gz[(size_t)3 * mc], mbmem[row * 2 * mc + mc + u],
                      cprev[row * mc + u], dz, &dcp);          // (hk_lstm_train.h)
    gz[0] = dz[0];
    gz[(size_t)mc] = dz[1];
    gz[(size_t)2 * mc] = dz[2];
    gz[(size_t)3 * mc] = dz[3];
    dcar[idx] = dcp;
}

// ppo_stats_kernel for a recurrent minibatch of M rows in ms sequences: the same means over the valid rows (rowstat[.][5] marks the others, dead
// rows included); stats[5] = the sequences whose id lies outside [0, n_seq)
__global__ __launch_bounds__(256) void ppo_lstm_stats_kernel(const double* rowstat, int M, const int* sids, int ms, int n_seq, float* stats, double* acc)
{
    __shared__ double red[6][256];
    const int tid = threadIdx.x;
    double s[6] = {};
    for (int i = tid; i < M; i += 256)
        for (int q = 0; q < 6; q++) s[q] += rowstat[(size_t)i * 6 + q];
    double sk = 0.0;
    for (int i = tid; i < ms; i += 256) sk += (sids[i] < 0 || sids[i] >= n_seq) ? 1.0 : 0.0;
    for (int q = 0; q < 6; q++) red[q][tid] = s[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) for (int q = 0; q < 6; q++) red[q][tid] += red[q][tid + w];
        __syncthreads();
    }
    const double invalid = red[5][0];
    __syncthreads();
    red[5][tid] = sk;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[5][tid] += red[5][tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double mv = (double)M - invalid;
        const double d = mv > 0 ? mv : 1.0;
        double o[6] = {-red[0][0] / (2.0 * d), red[1][0] / d, red[2][0] / d, red[3][0] / (2.0 * d), red[4][0] / (2.0 * d), red[5][0]};
        for (int q = 0; q < 6; q++) stats[q] = (float)o[q];
        if (acc) { for (int q = 0; q < 6; q++) acc[q] += o[q]; acc[6] += 1.0; }
    }
}

// master cell parameters and heads (PpoLstmNet offsets into flat) <-> the inference copies of policy_lstm_upload / policy_upload: the group-major
// Wq_ih / Wq_hh (pm_wq_index over 4m columns), the summed bias L.b, the two biases as attached (braw [8m] = b_ih | b_hh) and the m-wide heads.
// One thread per element of flat in [net.oWih, net.end).  TO_POLICY: publish; else the master copy is read back from the attached policy.
template <bool TO_POLICY>
__global__ __launch_bounds__(256) void ppo_lstm_publish_kernel(PolicyParams Q, PolicyLstm L, float* braw, PpoLstmNet net, float* flat)
{
    const size_t idx = net.oWih + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= net.end) return;
    const int mc = net.m, N = 4 * mc, H = net.hidden;
    auto mv = [&](const float* dst_c, size_t di) {
        float* dst = const_cast<float*>(dst_c);
        if (TO_POLICY) dst[di] = flat[idx]; else flat[idx] = dst[di];
    };
    if (idx < net.oWhh) {
        const size_t w = idx - net.oWih;
        const int col = (int)(w / H), k = (int)(w % H);
        mv(reinterpret_cast<const float*>(L.Wq_ih), pm_wq_index(k >> 3, k & 1, col, (k & 7) >> 1, N));
    } else if (idx < net.obih) {
        const size_t w = idx - net.oWhh;
        const int col = (int)(w / mc), k = (int)(w % mc);
        mv(reinterpret_cast<const float*>(L.Wq_hh), pm_wq_index(k >> 3, k & 1, col, (k & 7) >> 1, N));
    } else if (idx < net.obhh) {
        const size_t j = idx - net.obih;
        mv(braw, j);
        if (TO_POLICY) const_cast<float*>(L.b)[j] = flat[idx] + flat[net.obhh + j];      // fp32 b_ih + b_hh, as policy_lstm_upload forms it
    } else if (idx < net.oWmu) mv(braw, (size_t)N + (idx - net.obhh));
    else if (idx < net.obmu) mv(Q.W_mu, idx - net.oWmu);
    else if (idx == net.obmu) mv(Q.b_mu, 0);
    else if (idx == net.ols) mv(Q.log_sigma, 0);
    else if (idx < net.obbr) mv(Q.W_branch, idx - net.oWbr);
    else mv(Q.b_branch, idx - net.obbr);
}

}  // namespace hk
