// hk_rollout.h — device side of the rollout recorder (contract in include/hk.h, host side in hk_api.hip).  What a decision writes comes
// from policy_stack_kernel (OBS, FIRST) and the epilogue of policy_mlp_kernel (actions, RAW, heads, log-probabilities); the tick kernel
// stores TERM_* at ResetGame (hk_env_step.h phase_begin, reward instantiations only).  Here: the two snapshots of hk_rollout_begin and the
// kernel that closes an interval.  (MEMORY / NEXT_MEMORY of recurrent actors: policy_memory_kernel / rollout_next_memory_kernel, hk_policy_lstm.h.)
#pragma once
#include "hk_policy.h"

namespace hk {

// RING0: the stack entries that precede decision 0 of the rollout, oldest first, right-aligned in [E][A][smax - 1][obs_dim] (an actor of
// stack s fills the last s - 1 entries).  w0 = the ring slot decision 0 will write; the entries before it are w0 + 1 .. w0 + s - 1 (mod s).
__global__ __launch_bounds__(256) void rollout_ring0_kernel(PolicyParams Q, int E, int A, int w0, int smax, float* ring0)
{
    const size_t per = (size_t)(Q.stack - 1) * Q.obs_dim;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)E * Q.n_slots * per) return;
    const size_t pair = idx / per, r = idx % per;
    const int env = (int)(pair / Q.n_slots), j = (int)(pair % Q.n_slots);
    // (entry i = r / obs_dim of the s - 1 lands on entry smax - s + i of the row's smax - 1)
    const size_t dst = (((size_t)env * A + Q.slots[j]) * (smax - 1) + (smax - Q.stack)) * Q.obs_dim + r;
    ring0[dst] = Q.ring[pair * Q.in_dim + pm_ring_offset(Q, w0, (int)r)];
}

// the episode counters an interval's DONE is measured against (env words by lane-group slot, as policy_stack_kernel reads them)
__global__ __launch_bounds__(256) void rollout_epoch_kernel(const hk_env_state* envs_by_slot, const int* slot_of, int E, int* ep_prev)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env < E) ep_prev[env] = envs_by_slot[slot_of[env]].episodes_done;
}

// The end of interval t, one thread per (env, agent): the accumulators of the agents an actor drives move into REWARD / GROUP_REWARD [E][A]
// and are zeroed (Agent.SendInfo, as rewards_read_kernel does); DONE [E] from the rise of episodes_done since the interval before (2 when
// the time-out ended the episode: status bit 1).  More than one episode inside one interval raises *bad (hk_rollout_close reports it).
__global__ __launch_bounds__(256) void rollout_close_kernel(hk_agent_state* agents, const hk_env_state* envs_by_slot, const int* slot_of, int E, int A,
                                                            uint32_t driven, float* reward, float* group_reward, int* done, int* ep_prev, int* bad)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= E * A) return;
    const int env = idx / A, a = idx % A;
    if ((driven >> a) & 1u) {
        reward[idx] = agents[idx].step_reward; group_reward[idx] = agents[idx].group_reward;
        agents[idx].step_reward = 0.0f; agents[idx].group_reward = 0.0f;
    }
    if (a == 0) {
        const hk_env_state es = envs_by_slot[slot_of[env]];
        const int n = es.episodes_done - ep_prev[env];
        if (n > 0) {
            done[env] = (es.status & 2u) ? 2 : 1;
            ep_prev[env] = es.episodes_done;
            if (n > 1) atomicOr(bad, 1);
        }
    }
}

}  // namespace hk
