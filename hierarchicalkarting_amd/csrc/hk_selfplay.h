// hk_selfplay.h — device side of hk_rollout_episode_stats (contract in include/hk.h "SELF-PLAY", host side in hk_api.hip).
//   episode_scan_kernel      one lane per (env, slot) of the policy, t ascending over the completed rows: the running fp32 return, group
//                            return and length of the episode in progress; every DONE row emits an episode into the lane's own partial
//                            record (integers, fp64 sums, min / max) and the carry of the part after the last row goes to the carry-out
//   episode_combine_kernel   one workgroup: the lanes' records summed in (env, slot) order (fixed strided sums, fixed tree, as
//                            ppo_adv_norm_kernel does) into one hk_episode_stats.  No float atomics: the same call gives the same bits.
// The snapshot pool needs no kernel of its own: it launches ppo_publish_kernel<false / true> and policy_bf16_build_kernel as they are.
#pragma once
#include "hk_handle.h"      // EpisodeCarry, which the handle holds two of

namespace hk {

// the rollout fields the scan reads ([R][E][A], DONE [R][E]) and the policy's agent slots
struct EpisodeRows {
    const float *reward, *group_reward, *term_reward, *term_group;
    const int* done;
    int R, E, A, S;
    int slots[HK_MAX_AGENTS];
};

__device__ __forceinline__ void episode_stats_zero(hk_episode_stats& s)
{
    s.episodes = s.partial = s.wins = s.draws = s.losses = s.timeouts = s.len_sum = 0;
    s.ret_sum = s.ret_sumsq = s.gret_sum = s.gret_sumsq = 0.0;
    s.ret_min = __builtin_huge_val(); s.ret_max = -__builtin_huge_val();
}

__device__ __forceinline__ void episode_stats_add(hk_episode_stats& s, const hk_episode_stats& o)
{
    s.episodes += o.episodes; s.partial += o.partial; s.wins += o.wins; s.draws += o.draws; s.losses += o.losses; s.timeouts += o.timeouts;
    s.len_sum += o.len_sum;
    s.ret_sum += o.ret_sum; s.ret_sumsq += o.ret_sumsq; s.gret_sum += o.gret_sum; s.gret_sumsq += o.gret_sumsq;
    s.ret_min = o.ret_min < s.ret_min ? o.ret_min : s.ret_min;
    s.ret_max = o.ret_max > s.ret_max ? o.ret_max : s.ret_max;
}

constexpr int EPISODE_SCAN_U = 8;      // rows whose loads are in flight together

// The scan of hk.h, one lane per (e, j).  Every per-lane operation is one fp32 add (the unit is built with -ffp-contract=off).  use_carry 0:
// the carry-in is not read (nothing to adopt: every lane starts at 0 inside an episode of unknown beginning).
__global__ __launch_bounds__(256) void episode_scan_kernel(EpisodeRows P, EpisodeCarry cin, int use_carry, EpisodeCarry cout, hk_episode_stats* part)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.E * P.S) return;
    const int e = p / P.S, j = p % P.S;
    const size_t ca = (size_t)e * P.A + P.slots[j];
    int whole = use_carry ? cin.whole[ca] : 0;
    float acc = whole ? cin.ret[ca] : 0.0f, gacc = whole ? cin.gret[ca] : 0.0f;
    int len = whole ? cin.len[ca] : 0;
    hk_episode_stats s;
    episode_stats_zero(s);
    for (int t0 = 0; t0 < P.R; t0 += EPISODE_SCAN_U) {
        // the loads of EPISODE_SCAN_U rows first (none depends on the scan; the TERM_* words are read on every row so that no load waits for a
        // branch), then the rows in order.  A row past the last is read at the last row's address and not used.
        int d[EPISODE_SCAN_U];
        float rw[EPISODE_SCAN_U], gr[EPISODE_SCAN_U], tr[EPISODE_SCAN_U], tg[EPISODE_SCAN_U];
#pragma unroll
        for (int u = 0; u < EPISODE_SCAN_U; u++) {
            const int t = t0 + u < P.R ? t0 + u : P.R - 1;
            const size_t ea = ((size_t)t * P.E + e) * P.A + P.slots[j];
            d[u] = P.done[(size_t)t * P.E + e];
            rw[u] = P.reward[ea]; gr[u] = P.group_reward[ea]; tr[u] = P.term_reward[ea]; tg[u] = P.term_group[ea];
        }
#pragma unroll
        for (int u = 0; u < EPISODE_SCAN_U; u++) {
            if (t0 + u >= P.R) break;
            if (d[u] == 0) {
                acc += rw[u]; gacc += gr[u]; len += 1;
                continue;
            }
            acc += tr[u]; gacc += tg[u]; len += 1;
            if (!whole) s.partial += 1;
            else {
                const float f = tr[u] + tg[u];
                s.episodes += 1; s.len_sum += len;
                if (f > 0.0f) s.wins += 1; else if (f < 0.0f) s.losses += 1; else s.draws += 1;
                if (d[u] == 2) s.timeouts += 1;
                const double r = (double)acc, g = (double)gacc;
                s.ret_sum += r; s.ret_sumsq += r * r; s.gret_sum += g; s.gret_sumsq += g * g;
                s.ret_min = r < s.ret_min ? r : s.ret_min;
                s.ret_max = r > s.ret_max ? r : s.ret_max;
            }
            acc = rw[u]; gacc = gr[u]; len = 0; whole = 1;
        }
    }
    cout.ret[ca] = acc; cout.gret[ca] = gacc; cout.len[ca] = len; cout.whole[ca] = whole;
    part[p] = s;
}

// part [n] -> out [1], one workgroup of EPISODE_COMBINE_THREADS: thread i sums records i, i + 256, ... in that order, then the fixed tree
constexpr int EPISODE_COMBINE_THREADS = 256;      // 256 records of 104 bytes in LDS
__global__ __launch_bounds__(EPISODE_COMBINE_THREADS) void episode_combine_kernel(const hk_episode_stats* part, int n, hk_episode_stats* out)
{
    __shared__ hk_episode_stats red[EPISODE_COMBINE_THREADS];
    const int tid = threadIdx.x;
    hk_episode_stats s;
    episode_stats_zero(s);
    for (int i = tid; i < n; i += EPISODE_COMBINE_THREADS) episode_stats_add(s, part[i]);
    red[tid] = s;
    __syncthreads();
    for (int w = EPISODE_COMBINE_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) episode_stats_add(red[tid], red[tid + w]);
        __syncthreads();
    }
    if (tid == 0) *out = red[0];
}

}  // namespace hk
