"""Host helpers over a recorded rollout (RacingEnv.rollout() / rollout_views(); row contract in include/hk.h, hk_rollout_field).
Both work on numpy arrays and on torch tensors alike (indexing and arithmetic only)."""
import numpy as np


def stacked_inputs(ro, slots, stack):
    """-> [R, E, len(slots), stack * obs_dim]: the stacked observation the actor of `stack` saw at every row, oldest first —
    the StackingSensor rule of policy_stack_kernel: the stack starts from RING0 (its last stack - 1 entries), is zeroed where FIRST
    is set, and every decision pushes OBS[t].  Fed to the actor (hk_policy_forward) it gives MU / LOGITS of the rows."""
    obs, first, ring0 = ro["obs"], ro["first"], ro["ring0"]
    R, E = obs.shape[0], obs.shape[1]
    D = obs.shape[3]
    slots = list(slots)
    if stack < 1 or stack - 1 > ring0.shape[2]:
        raise ValueError("stack %d: RING0 holds %d entries" % (stack, ring0.shape[2]))
    to_np = not isinstance(obs, np.ndarray)
    if to_np:           # (torch tensors: the rebuild runs on the host)
        obs, first, ring0 = obs.cpu().numpy(), first.cpu().numpy(), ring0.cpu().numpy()
    hist = np.array(ring0[:, slots, ring0.shape[2] - (stack - 1):, :], np.float32)       # [E, S, stack - 1, D]
    out = np.zeros((R, E, len(slots), stack * D), np.float32)
    for t in range(R):
        clear = first[t][:, slots].astype(bool)
        hist[clear] = 0.0
        cur = np.concatenate([hist, obs[t][:, slots, None, :]], axis=2)                    # [E, S, stack, D]
        out[t] = cur.reshape(E, len(slots), stack * D)
        hist = cur[:, :, 1:, :]
    return out


def transition_rewards(ro):
    """-> [R, E, A]: the reward of every row's transition, DONE ? TERM_REWARD : REWARD (a row whose interval held an episode end
    rewards the terminal step; what followed the reset belongs to the next episode's first transition)"""
    done = ro["done"][:, :, None] != 0
    if isinstance(done, np.ndarray):
        return np.where(done, ro["term_reward"], ro["reward"])
    import torch
    return torch.where(done, ro["term_reward"], ro["reward"])
