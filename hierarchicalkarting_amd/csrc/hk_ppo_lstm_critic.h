// hk_ppo_lstm_critic.h — device side of the recurrent critic of recurrent PPO (contract in include/hk.h "PPO trainer" RECURRENT CRITIC, host
// side in hk_train.hip).  The critic is the actor's normalised input -> n x (Linear + Swish) of width Hc -> ONE LSTM cell of m_v units
// -> v = b_v + sum_k W_v[k] h'[k], in the arithmetic of a recurrent actor (hk_policy_lstm.h): its training forward and backward over a window
// are hk_ppo_lstm.h's kernels on a second workspace.  New here:
//   ppo_lstm_value_ids_kernel     the row ids of a chunk of the value pass, time-major: (t0 + tl) E S + p0 + q; t == R gives the bootstrap ids;
//                                 and the rows' flag words: FIRST of row t, at the bootstrap step DONE of row R - 1
//   ppo_lstm_value_kernel         hk_ppo_advantages: the cell and the value head over `T` consecutive time steps of a tile of sequences in ONE
//                                 launch.  A workgroup owns 32 sequences and ALL m_v units of them, so a step needs nothing from another
//                                 workgroup: h' stays in LDS, c in the registers of the lane that owns (sequence, unit).  Per step the four
//                                 gate chains are seeded from Zx (bsum + a W_ih^T, ppo_gemm_kernel<0>, stored to fp32) and continued over h
//                                 in ascending k on v_mfma_f32_32x32x2_f32 — ppo_lstm_step_kernel's order, bit for bit — hk_lstm_cell is the
//                                 epilogue on the C/D layout, the value head one lane per sequence on the LDS copy of h' (pm_head).
//                                 It writes V_OLD / the bootstrap value, the memory at window starts and the carry at the end of the launch,
//                                 and none of what only a backward pass reads (gate outputs, hprev, cprev, per-row h').
//   ppo_lstm_critic_mem0_kernel   a minibatch's windows' initial critic memory from CRITIC_MEMORY (ppo_lstm_expand_kernel's second half)
#pragma once
#include "hk_ppo_lstm.h"

namespace hk {

// where the critic's cell and value head sit in the flat vector (PARAMS offsets), behind the critic's trunk (PpoNet's oW / ob)
struct PpoLstmCriticNet {
    int m = 0, hidden = 0;
    size_t oWih = 0, oWhh = 0, obih = 0, obhh = 0, oWv = 0, obv = 0, end = 0;      // W_ih [4m][Hc], W_hh [4m][m], b_ih, b_hh [4m], W_v [m], b_v
    void layout(int Hc, int mv, size_t base)
    {
        m = mv; hidden = Hc;
        size_t o = base;
        oWih = o; o += (size_t)4 * mv * Hc;
        oWhh = o; o += (size_t)4 * mv * mv;
        obih = o; o += (size_t)4 * mv;
        obhh = o; o += (size_t)4 * mv;
        oWv = o; o += mv;
        obv = o; o += 1;
        end = o;
    }
};

constexpr int PLV_TS = 32;          // sequences per workgroup (one MFMA row block)
constexpr int PLV_LDH = 33;         // row stride of the h tile, k-major: the 32 lanes of a half read / write 32 distinct banks

inline size_t ppo_lstm_value_lds_bytes(int mv) { return ((size_t)mv * PLV_LDH + (size_t)4 * PPO_TK * (mv + 1)) * sizeof(float); }

__global__ __launch_bounds__(256) void ppo_lstm_value_ids_kernel(PpoRows P, int* ids, int* flags, int t0, int T, int p0, int sq)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * sq) return;
    const int t = t0 + idx / sq, p = p0 + idx % sq, e = p / P.S, j = p - e * P.S;
    ids[idx] = t <= P.R ? t * P.E * P.S + p : -1;          // (row R: the bootstrap ids n + p of ppo_gather_kernel)
    flags[idx] = t < P.R ? P.first[((size_t)t * P.E + e) * P.A + P.slots[j]] != 0 : (t == P.R && P.done[(size_t)(P.R - 1) * P.E + e] != 0);
}

// Time steps t0 .. t0 + T - 1 (<= R; t == R is the bootstrap step) of the sequences p0 .. p0 + sq - 1, p = e S + j.  blockDim = 64 (m_v / 32): wave
// w owns the units [32 w, 32 w + 32) of the workgroup's 32 sequences, with FOUR accumulators, the i / f / g / o columns of its units.
// Zx [T][sq][4 m_v], flags [T][sq] (ppo_lstm_value_ids_kernel): the chunk's rows time-major.  carry [E S][2 m_v]: the memory [h | c] entering step t0, replaced by the one leaving step
// t0 + T - 1.  Before a step's FIRST rule the memory it was handed is recorded: into cmem[t / L] [E S][2 m_v] at a window start t = k L < R, and
// into mem_out at t == R, zero where DONE[R - 1].  LDS: Hs [m_v][33] (h of the tile, k-major), Bs [4][32][m_v + 1] (a k-chunk of W_hh, all units).
__global__ __launch_bounds__(256) void ppo_lstm_value_kernel(int R, int ES, int t0, int T, int p0, int sq, int mv, int L, const float* __restrict__ Zx,
                                                             const int* __restrict__ flags, const float* __restrict__ Whh, const float* __restrict__ W_v, const float* __restrict__ b_v,
                                                             float* carry, float* cmem, float* mem_out, float* v_old, float* v_boot)
{
    extern __shared__ __align__(16) float plv_lds[];
    float* Hs = plv_lds;
    float* Bs = plv_lds + (size_t)mv * PLV_LDH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x;
    const int half = lane >> 5, c = lane & 31;
    const int unit = wave * 32 + c, ldb = mv + 1, N = 4 * mv;
    const int q0 = blockIdx.x * PLV_TS;
    // the tile's sequences: a row of the block past them is a twin of the last one — the same loads, the same arithmetic and the same stores of
    // the same bits to the same addresses — so that no lane needs a mask per accumulator register
    const int nq = sq - q0 < PLV_TS ? sq - q0 : PLV_TS;
    // C/D layout: col (unit) = lane & 31, row (sequence of the tile) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float cc[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int ql = (r & 3) + 8 * (r >> 2) + 4 * half, qc = ql < nq ? ql : nq - 1;
        const float* mrow = carry + (size_t)(p0 + q0 + qc) * 2 * mv;
        Hs[unit * PLV_LDH + ql] = mrow[unit];
        cc[r] = mrow[mv + unit];
    }
    for (int tl = 0; tl < T; tl++) {
        const int t = t0 + tl;
        const bool boot = t >= R;
        const bool rec = boot || t % L == 0;
        float* recp = boot ? mem_out : cmem + (size_t)(t / L) * ES * 2 * mv;
        f32x16 z[4];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int ql = (r & 3) + 8 * (r >> 2) + 4 * half, qc = ql < nq ? ql : nq - 1;
            const size_t row = (size_t)tl * sq + q0 + qc;
            // the flag word (0 / 1: FIRST of the row; at the bootstrap step DONE[R - 1]) as a bit mask: all ones keeps, zero gives exactly +0.0f
            const unsigned keep = (unsigned)flags[row] - 1u;
            // (each (sequence, unit) of Hs and cc is touched by the one lane that owns it)
            float hq = Hs[unit * PLV_LDH + ql];
            if (rec) {
                float* mrow = recp + (size_t)(p0 + q0 + qc) * 2 * mv;
                mrow[unit] = boot ? __uint_as_float(__float_as_uint(hq) & keep) : hq;
                mrow[mv + unit] = boot ? __uint_as_float(__float_as_uint(cc[r]) & keep) : cc[r];
            }
            if (!boot) {
                Hs[unit * PLV_LDH + ql] = __uint_as_float(__float_as_uint(hq) & keep);
                cc[r] = __uint_as_float(__float_as_uint(cc[r]) & keep);
            }
            const float* zx = Zx + row * N + unit;
#pragma unroll
            for (int g = 0; g < 4; g++) z[g][r] = zx[(size_t)g * mv];
        }
        for (int kb = 0; kb < mv; kb += PPO_TK) {
            for (int x = tid; x < PPO_TK * N; x += nthr) {
                const int kk = x & 31, gu = x >> 5, g = gu / mv, u = gu - g * mv;
                Bs[(g * PPO_TK + kk) * ldb + u] = Whh[(size_t)gu * mv + kb + kk];
            }
            __syncthreads();          // (also: every h of this step is in place)
            const float* ap = Hs + (kb + half) * PLV_LDH + c;
            const float* bp = Bs + half * ldb + unit;
            for (int s = 0; s < PPO_TK / 2; s++) {
                const float a = ap[2 * s * PLV_LDH];
#pragma unroll
                for (int g = 0; g < 4; g++) z[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[(g * PPO_TK + 2 * s) * ldb], z[g], 0, 0, 0);
            }
            __syncthreads();
        }
        // every wave has finished reading h: the cell, h' over h
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int ql = (r & 3) + 8 * (r >> 2) + 4 * half;
            float hn, cn;
            hk_lstm_cell(z[0][r], z[1][r], z[2][r], z[3][r], cc[r], &hn, &cn);
            Hs[unit * PLV_LDH + ql] = hn;
            cc[r] = cn;
        }
        __syncthreads();
        if (tid < nq) {
            const float v = pm_head(Hs + tid, PLV_LDH, W_v, b_v[0], mv);          // the actor's mu chain on h'
            const int p = p0 + q0 + tid;
            if (boot) v_boot[p] = v; else v_old[(size_t)t * ES + p] = v;
        }
        __syncthreads();          // the head has read h' before the next step's FIRST rule may clear it
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int ql = (r & 3) + 8 * (r >> 2) + 4 * half, qc = ql < nq ? ql : nq - 1;
        float* mrow = carry + (size_t)(p0 + q0 + qc) * 2 * mv;
        mrow[unit] = Hs[unit * PLV_LDH + ql];
        mrow[mv + unit] = cc[r];
    }
}

// mem0 [ms][2 m_v] of a minibatch: CRITIC_MEMORY of sequence sid = (k E + e) S + j is its row sid; an id outside [0, n_seq): zeros
__global__ __launch_bounds__(256) void ppo_lstm_critic_mem0_kernel(const float* __restrict__ cmem, const int* __restrict__ sids, int ms, int n_seq, int mv,
                                                                   float* mem0)
{
    const size_t y = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= (size_t)ms * 2 * mv) return;
    const int q = (int)(y / (2 * mv)), x = (int)(y % (2 * mv));
    const int sid = sids[q];
    mem0[y] = (sid >= 0 && sid < n_seq) ? cmem[(size_t)sid * 2 * mv + x] : 0.0f;
}

}  // namespace hk
