#!/usr/bin/env python3
"""What a host-side refactor of hk_api.hip (the environment's unit) or of hk_handle.h must leave as it is: one fixed course through the entry
points outside the trainers — the snapshot pools, which live in hk_train.hip, are on it too — (LQ batch, reset / actions / step, policy attach / forward / memory, the rollout recorder, snapshot pools, episode statistics, the
state getters and setters, the RCCL gather, the device-pointer getters, the profiler), printed as one JSON document.  Run it once per
library, each in a fresh process, and compare the two outputs byte for byte:

    HK_LIB_PATH=build/libhk_parent.so python tools/api_identity.py --out a.json
    python tools/api_identity.py --out b.json && cmp a.json b.json

The course runs on handles of 8 envs x 4 karts: "pa", the planner + actor handle of smoke(); "rc", four RL karts under a recurrent and a
plain actor; "pl", a plain LQ handle; "ne", a handle without an environment (hk_create(NULL)); and the NULL handle.  Every entry point gets
one good call, recorded as a SHA-256 of what it returned, and every refusal it can give, recorded as the return code and the texts of
hk_last_error(h) and hk_last_error(NULL).  Under `rocprofv3 --hip-trace --stats` the same course gives the HIP call counts to compare.
tests/test_api_refusals_gpu.py runs refusals() against a literal table; tools/trainer_identity.py and tools/actor_identity.py are the
siblings for the trainers and the actor kernels."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hierarchicalkarting_amd as hk
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy

RL, LQR, MCTS, FIXED = _lib.HK_LOW_RL, _lib.HK_LOW_LQR, _lib.HK_HIGH_MCTS, _lib.HK_HIGH_FIXED
E, A, P = 8, 4, 2
fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def sha(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def f32(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(fp)


def i32(a):
    return np.ascontiguousarray(a, np.int32).ctypes.data_as(ip)


class Course:
    """the handles of the course; `h` maps their names to the raw handles the entry points take (None: the NULL handle)"""

    def __init__(self):
        self.L = _lib.load()
        pa = hk.RacingEnv(hk.make_config(E, A, jitter_seed=7, rewards=1, mcts_iterations=16, tree_search_depth=[8, 8, 5, 5],
                                         high_mode=[MCTS, MCTS, FIXED, FIXED], low_mode=[RL, LQR, LQR, LQR]))
        pa.attach_policy(Policy.random(pa.obs_dim * 4, 128, 3, seed=1), [0], P)
        pa.reset()
        rc = hk.RacingEnv(hk.make_config(E, A, low_mode=[RL] * A, rewards=1, max_episode_steps=150, jitter_seed=4))
        self.rec_pol = Policy.random(rc.obs_dim * 4, 64, 2, stack=4, seed=2, memory_size=64)
        self.plain_pol = Policy.random(rc.obs_dim * 4, 64, 2, stack=4, seed=3)
        rc.attach_policy(self.rec_pol, [0, 1], P)
        rc.attach_policy(self.plain_pol, [2], P)
        rc.reset()
        pl = hk.RacingEnv(hk.make_config(E, A, jitter_seed=3))
        pl.reset()
        ne = C.c_void_p()
        _lib.check(self.L.hk_create(None, C.byref(ne)), None)
        self.pa, self.rc, self.pl, self.ne = pa, rc, pl, ne
        self.h = {"pa": pa.h, "rc": rc.h, "pl": pl.h, "ne": ne, "null": None}

    def close(self):
        for g in (self.pa, self.rc, self.pl):
            g.close()
        self.L.hk_destroy(self.ne)


def entry_points(L):
    """every entry point of the course as name -> call(h) with arguments that are otherwise fine: what the NULL handle and the handle
    without an environment are refused with"""
    buf = np.zeros(1 << 16, np.float32)            # room for any getter of an 8 x 4 handle but hk_get_agent_state / hk_get_mcts_state, which get their own
    big = np.zeros(1 << 20, np.uint8)
    i64 = (C.c_int64 * 64)()
    desc, _keep = Policy.random(8, 32, 1, stack=1, seed=0).desc()
    ids = (C.c_char * _lib.HK_COMM_ID_BYTES)()
    st = _lib.EpisodeStats()
    dbg = _lib.LqDebug()
    as_ = lambda t: big.ctypes.data_as(C.POINTER(t))
    calls = {
        "hk_reset": lambda h: L.hk_reset(h, None, 0, -1),
        "hk_set_actions": lambda h: L.hk_set_actions(h, f32(buf), i32(buf.view(np.int32))),
        "hk_step": lambda h: L.hk_step(h, 1),
        "hk_policy_attach": lambda h: L.hk_policy_attach(h, C.byref(desc), i32([0]), 1, P),
        "hk_policy_attach_lstm": lambda h: L.hk_policy_attach_lstm(h, C.byref(desc), None, i32([0]), 1, P),
        "hk_policy_forward": lambda h: L.hk_policy_forward(h, 0, 1, f32(buf), f32(buf), f32(buf)),
        "hk_policy_forward_mem": lambda h: L.hk_policy_forward_mem(h, 0, 1, f32(buf), None, f32(buf), f32(buf), None),
        "hk_policy_memory_size": lambda h: L.hk_policy_memory_size(h, 0),
        "hk_policy_memory_get": lambda h: L.hk_policy_memory_get(h, 0, f32(buf)),
        "hk_policy_memory_set": lambda h: L.hk_policy_memory_set(h, 0, f32(buf)),
        "hk_policy_set_precision": lambda h: L.hk_policy_set_precision(h, 0, _lib.HK_POLICY_PREC_F32),
        "hk_policy_get_precision": lambda h: L.hk_policy_get_precision(h, 0),
        "hk_get_actions": lambda h: L.hk_get_actions(h, f32(buf), i32(buf.view(np.int32))),
        "hk_rollout_begin": lambda h: L.hk_rollout_begin(h, 4),
        "hk_rollout_rows": lambda h: L.hk_rollout_rows(h),
        "hk_rollout_close": lambda h: L.hk_rollout_close(h),
        "hk_rollout_ptr": lambda h: L.hk_rollout_ptr(h, 0),
        "hk_policy_pool_create": lambda h: L.hk_policy_pool_create(h, 0, 2),
        "hk_policy_pool_count": lambda h: L.hk_policy_pool_count(h, 0),
        "hk_policy_pool_save": lambda h: L.hk_policy_pool_save(h, 0, 0, 0),
        "hk_policy_pool_load": lambda h: L.hk_policy_pool_load(h, 0, 0, 0),
        "hk_policy_pool_put": lambda h: L.hk_policy_pool_put(h, 0, 0, f32(buf)),
        "hk_policy_pool_get": lambda h: L.hk_policy_pool_get(h, 0, 0, f32(buf)),
        "hk_rollout_episode_stats": lambda h: L.hk_rollout_episode_stats(h, 0, C.byref(st)),
        "hk_obs_dim": lambda h: L.hk_obs_dim(h),
        "hk_get_observations": lambda h: L.hk_get_observations(h, f32(buf)),
        "hk_get_agent_state": lambda h: L.hk_get_agent_state(h, as_(_lib.AgentState)),
        "hk_set_agent_state": lambda h: L.hk_set_agent_state(h, as_(_lib.AgentState)),
        "hk_get_env_state": lambda h: L.hk_get_env_state(h, as_(_lib.EnvState)),
        "hk_set_env_state": lambda h: L.hk_set_env_state(h, as_(_lib.EnvState)),
        "hk_get_episode_results": lambda h: L.hk_get_episode_results(h, as_(_lib.EpisodeResult)),
        "hk_comm_init": lambda h: L.hk_comm_init(h, 1, 0, ids),
        "hk_gather_results": lambda h: L.hk_gather_results(h, as_(_lib.EpisodeResult)),
        "hk_gather_count": lambda h: L.hk_gather_count(h, i64),
        "hk_comm_destroy": lambda h: L.hk_comm_destroy(h),
        "hk_get_rewards": lambda h: L.hk_get_rewards(h, f32(buf), f32(buf[4096:])),
        "hk_get_mcts_state": lambda h: L.hk_get_mcts_state(h, as_(_lib.MctsState)),
        "hk_get_lq_debug": lambda h: L.hk_get_lq_debug(h, 0, 0, C.byref(dbg)),
        "hk_device_results_ptr": lambda h: L.hk_device_results_ptr(h),
        "hk_device_agents_ptr": lambda h: L.hk_device_agents_ptr(h),
        "hk_device_obs_ptr": lambda h: L.hk_device_obs_ptr(h),
        "hk_device_act_steer_ptr": lambda h: L.hk_device_act_steer_ptr(h),
        "hk_device_act_branch_ptr": lambda h: L.hk_device_act_branch_ptr(h),
        "hk_device_reward_ptr": lambda h: L.hk_device_reward_ptr(h),
        "hk_device_group_reward_ptr": lambda h: L.hk_device_group_reward_ptr(h),
        "hk_observe": lambda h: L.hk_observe(h),
        "hk_rewards_device": lambda h: L.hk_rewards_device(h),
        "hk_prof_enable": lambda h: L.hk_prof_enable(h, 0),
        "hk_prof_reset": lambda h: L.hk_prof_reset(h),
        "hk_prof_games": lambda h: L.hk_prof_games(h, i64),
        "hk_prof_meter": lambda h: L.hk_prof_meter(h, i64),
        "hk_prof_read": lambda h: L.hk_prof_read(h, None, None),
        "hk_synchronize": lambda h: L.hk_synchronize(h),
        "hk_stream": lambda h: L.hk_stream(h),
        "hk_lq_solve_batch_device": lambda h: L.hk_lq_solve_batch_device(h, 1, 2, None, None, None, None, None, None, 3, None, None),
    }
    calls["_keep"] = (buf, big, i64, desc, _keep, ids, st, dbg)
    return calls


POINTERS = ("hk_rollout_ptr", "hk_stream", "hk_device_results_ptr", "hk_device_agents_ptr", "hk_device_obs_ptr", "hk_device_act_steer_ptr",
            "hk_device_act_branch_ptr", "hk_device_reward_ptr", "hk_device_group_reward_ptr")
# a NULL handle: these three said HK_ERR_INVALID without a message before settle(); they may now also set "NULL handle"
NULL_MESSAGE_MAY_DIFFER = ("null hk_synchronize", "null hk_prof_reset", "null hk_prof_read")


def refusals(c):
    """the refusal half of the course, in its fixed order: yields (label, handle name, call); call() returns the entry point's code (a
    pointer getter: 0 for a pointer, "NULL" for none).  Steps that only move a handle into the state the next refusals need are yielded
    with the label None and must succeed."""
    L, h = c.L, c.h
    ep = entry_points(L)
    keep = ep.pop("_keep")

    def ptr(f):
        return lambda: 0 if f() else "NULL"

    # the NULL handle and the handle without an environment, every entry point; after each of the three calls whose NULL-handle message
    # may differ comes one that sets it, so the difference stays in those three lines
    for who in ("null", "ne"):
        for name, call in ep.items():
            if who == "ne" and name == "hk_lq_solve_batch_device":          # (needs no environment: it would launch on the NULL arrays)
                continue
            f = (lambda call=call, who=who: call(h[who]))
            yield "%s %s" % (who, name), who, ptr(f) if name in POINTERS else f
            if who == "null" and "null " + name in NULL_MESSAGE_MAY_DIFFER:
                yield "null hk_rollout_rows (after %s)" % name, who, lambda: L.hk_rollout_rows(None)
    buf = np.zeros(1 << 16, np.float32)
    i64 = (C.c_int64 * 64)()
    st = _lib.EpisodeStats()
    dbg = _lib.LqDebug()
    pa, rc, pl = h["pa"], h["rc"], h["pl"]
    # ---- arguments, no rollout yet
    yield "hk_reset n < 0", "pa", lambda: L.hk_reset(pa, i32([0]), -1, -1)
    yield "hk_reset env id out of range", "pa", lambda: L.hk_reset(pa, i32([0, E]), 2, -1)
    yield "hk_set_actions NULL", "pa", lambda: L.hk_set_actions(pa, None, None)
    yield "hk_get_actions NULL", "pa", lambda: L.hk_get_actions(pa, None, None)
    yield "hk_step n_ticks < 0", "pa", lambda: L.hk_step(pa, -1)
    yield "hk_policy_forward bad policy", "pa", lambda: L.hk_policy_forward(pa, 5, 1, f32(buf), f32(buf), f32(buf))
    yield "hk_policy_forward rows < 0", "pa", lambda: L.hk_policy_forward(pa, 0, -1, f32(buf), f32(buf), f32(buf))
    yield "hk_policy_forward NULL", "pa", lambda: L.hk_policy_forward(pa, 0, 1, None, f32(buf), f32(buf))
    yield "hk_policy_forward on a recurrent actor", "rc", lambda: L.hk_policy_forward(rc, 0, 1, f32(buf), f32(buf), f32(buf))
    yield "hk_policy_forward_mem without memory", "pa", lambda: L.hk_policy_forward_mem(pa, 0, 1, f32(buf), None, f32(buf), f32(buf), None)
    yield "hk_policy_forward_mem NULL", "rc", lambda: L.hk_policy_forward_mem(rc, 0, 1, f32(buf), None, None, f32(buf), None)
    yield "hk_policy_memory_size bad policy", "pa", lambda: L.hk_policy_memory_size(pa, 1)
    yield "hk_policy_memory_get bad policy", "rc", lambda: L.hk_policy_memory_get(rc, -1, f32(buf))
    yield "hk_policy_memory_get without memory", "pa", lambda: L.hk_policy_memory_get(pa, 0, f32(buf))
    yield "hk_policy_memory_get NULL", "rc", lambda: L.hk_policy_memory_get(rc, 0, None)
    yield "hk_policy_memory_set without memory", "rc", lambda: L.hk_policy_memory_set(rc, 1, f32(buf))
    yield "hk_policy_memory_set NULL", "rc", lambda: L.hk_policy_memory_set(rc, 0, None)
    yield "hk_policy_set_precision bad policy", "pa", lambda: L.hk_policy_set_precision(pa, 3, 0)
    yield "hk_policy_set_precision unknown", "pa", lambda: L.hk_policy_set_precision(pa, 0, 7)
    yield "hk_policy_set_precision bf16 with memory", "rc", lambda: L.hk_policy_set_precision(rc, 0, _lib.HK_POLICY_PREC_BF16)
    yield "hk_policy_get_precision bad policy", "pa", lambda: L.hk_policy_get_precision(pa, -1)
    # hk_policy_attach: what hk::policy_validate and the entry point itself refuse
    good, keep1 = c.plain_pol.desc()
    bad_in = _lib.PolicyDesc.from_buffer_copy(good); bad_in.stack = 2
    odd = _lib.PolicyDesc.from_buffer_copy(good); odd.in_dim = 7
    wide = _lib.PolicyDesc.from_buffer_copy(good); wide.hidden = 48
    lstm_ok = c.rec_pol.lstm_desc()
    lstm_res = _lib.PolicyLstmDesc.from_buffer_copy(lstm_ok); lstm_res.reserved = 1
    lstm_odd = _lib.PolicyLstmDesc.from_buffer_copy(lstm_ok); lstm_odd.memory_size = 65
    keep += (good, keep1, bad_in, odd, wide, lstm_ok, lstm_res, lstm_odd)
    att = lambda hh, d, slots, n, period: (lambda: L.hk_policy_attach(hh, C.byref(d) if d is not None else None, i32(slots), n, period))
    yield "hk_policy_attach NULL desc", "rc", att(rc, None, [3], 1, P)
    yield "hk_policy_attach odd in_dim", "rc", att(rc, odd, [3], 1, P)
    yield "hk_policy_attach hidden 48", "rc", att(rc, wide, [3], 1, P)
    yield "hk_policy_attach_lstm reserved", "rc", lambda: L.hk_policy_attach_lstm(rc, C.byref(good), C.byref(lstm_res), i32([3]), 1, P)
    yield "hk_policy_attach_lstm odd memory_size", "rc", lambda: L.hk_policy_attach_lstm(rc, C.byref(good), C.byref(lstm_odd), i32([3]), 1, P)
    yield "hk_policy_attach no slots", "rc", att(rc, good, [3], 0, P)
    yield "hk_policy_attach NULL slots", "rc", lambda: L.hk_policy_attach(rc, C.byref(good), None, 1, P)
    yield "hk_policy_attach decision_period 0", "rc", att(rc, good, [3], 1, 0)
    yield "hk_policy_attach in_dim of another stack", "rc", att(rc, bad_in, [3], 1, P)
    yield "hk_policy_attach slot out of range", "rc", att(rc, good, [4], 1, P)
    yield "hk_policy_attach slot not RL", "pa", att(pa, good, [1], 1, P)
    yield "hk_policy_attach slot taken", "rc", att(rc, good, [2], 1, P)
    yield "hk_policy_attach duplicate slot", "rc", att(rc, good, [3, 3], 2, P)
    yield "hk_policy_attach other decision_period", "rc", att(rc, good, [3], 1, 3)
    # recorder, before any rollout
    yield "hk_rollout_begin no actor", "pl", lambda: L.hk_rollout_begin(pl, 4)
    yield "hk_rollout_begin rows < 1", "pa", lambda: L.hk_rollout_begin(pa, 0)
    yield "hk_rollout_close none open", "pa", lambda: L.hk_rollout_close(pa)
    yield "hk_rollout_ptr bad field", "pa", ptr(lambda: L.hk_rollout_ptr(pa, _lib.HK_RO_FIELDS))
    yield "hk_rollout_ptr no rollout yet", "pa", ptr(lambda: L.hk_rollout_ptr(pa, 0))
    yield "hk_rollout_episode_stats NULL", "pa", lambda: L.hk_rollout_episode_stats(pa, 0, None)
    yield "hk_rollout_episode_stats bad policy", "pa", lambda: L.hk_rollout_episode_stats(pa, 2, C.byref(st))
    yield "hk_rollout_episode_stats no rollout yet", "pa", lambda: L.hk_rollout_episode_stats(pa, 0, C.byref(st))
    yield None, "pa", lambda: L.hk_step(pa, 1)
    yield "hk_rollout_begin mid-interval", "pa", lambda: L.hk_rollout_begin(pa, 4)
    yield None, "pa", lambda: L.hk_step(pa, 1)
    # snapshot pools
    yield "hk_policy_pool_create bad policy", "rc", lambda: L.hk_policy_pool_create(rc, 9, 2)
    yield "hk_policy_pool_create no slots", "rc", lambda: L.hk_policy_pool_create(rc, 1, 0)
    yield "hk_policy_pool_create too many slots", "rc", lambda: L.hk_policy_pool_create(rc, 1, _lib.HK_POOL_MAX_SLOTS + 1)
    yield "hk_policy_pool_create recurrent", "rc", lambda: L.hk_policy_pool_create(rc, 0, 2)
    yield "hk_policy_pool_count bad pool", "rc", lambda: L.hk_policy_pool_count(rc, 0)
    yield "hk_policy_pool_save bad pool", "rc", lambda: L.hk_policy_pool_save(rc, 0, 0, 1)
    yield None, "rc", lambda: L.hk_policy_pool_create(rc, 1, 2)
    yield "hk_policy_pool_save bad slot", "rc", lambda: L.hk_policy_pool_save(rc, 0, 2, 1)
    yield "hk_policy_pool_save bad policy", "rc", lambda: L.hk_policy_pool_save(rc, 0, 0, -1)
    yield "hk_policy_pool_save recurrent", "rc", lambda: L.hk_policy_pool_save(rc, 0, 0, 0)
    yield "hk_policy_pool_load never written", "rc", lambda: L.hk_policy_pool_load(rc, 0, 1, 1)
    yield "hk_policy_pool_put NULL", "rc", lambda: L.hk_policy_pool_put(rc, 0, 0, None)
    yield "hk_policy_pool_get NULL", "rc", lambda: L.hk_policy_pool_get(rc, 0, 0, None)
    yield "hk_policy_pool_get never written", "rc", lambda: L.hk_policy_pool_get(rc, 0, 1, f32(buf))
    # getters and setters
    yield "hk_get_observations NULL", "pa", lambda: L.hk_get_observations(pa, None)
    yield "hk_get_agent_state NULL", "pa", lambda: L.hk_get_agent_state(pa, None)
    yield "hk_set_agent_state NULL", "pa", lambda: L.hk_set_agent_state(pa, None)
    far = c.pa.agent_state(); far["section_index"][3, 2] = -1
    keep += (far,)
    yield "hk_set_agent_state section_index < 0", "pa", lambda: L.hk_set_agent_state(pa, far.ctypes.data_as(C.POINTER(_lib.AgentState)))
    yield "hk_get_env_state NULL", "pa", lambda: L.hk_get_env_state(pa, None)
    yield "hk_set_env_state NULL", "pa", lambda: L.hk_set_env_state(pa, None)
    yield "hk_get_episode_results NULL", "pa", lambda: L.hk_get_episode_results(pa, None)
    yield "hk_get_rewards NULL", "pa", lambda: L.hk_get_rewards(pa, None, f32(buf))
    yield "hk_get_mcts_state NULL", "pa", lambda: L.hk_get_mcts_state(pa, None)
    yield "hk_get_lq_debug bad env", "pl", lambda: L.hk_get_lq_debug(pl, E, 0, C.byref(dbg))
    yield "hk_get_lq_debug NULL", "pl", lambda: L.hk_get_lq_debug(pl, 0, 0, None)
    # ("debug taps are off" cannot be reached: env_create allocates the taps for every handle)
    yield "hk_prof_games NULL", "pl", lambda: L.hk_prof_games(pl, None)
    yield "hk_prof_meter NULL", "pl", lambda: L.hk_prof_meter(pl, None)
    # the gather
    yield "hk_comm_init NULL id", "pl", lambda: L.hk_comm_init(pl, 1, 0, None)
    yield "hk_comm_init bad rank", "pl", lambda: L.hk_comm_init(pl, 1, 1, (C.c_char * _lib.HK_COMM_ID_BYTES)())
    yield "hk_gather_results NULL", "pl", lambda: L.hk_gather_results(pl, None)
    yield "hk_gather_results no communicator", "pl", lambda: L.hk_gather_results(pl, buf.ctypes.data_as(C.POINTER(_lib.EpisodeResult)))
    yield "hk_gather_count NULL", "pl", lambda: L.hk_gather_count(pl, None)
    yield "hk_gather_count no communicator", "pl", lambda: L.hk_gather_count(pl, i64)
    cid = (C.c_char * _lib.HK_COMM_ID_BYTES)()
    yield None, "null", lambda: L.hk_comm_unique_id(cid)
    yield None, "pl", lambda: L.hk_comm_init(pl, 1, 0, cid)
    yield "hk_comm_init twice", "pl", lambda: L.hk_comm_init(pl, 1, 0, cid)
    yield "hk_comm_unique_id NULL", "null", lambda: L.hk_comm_unique_id(None)
    # the LQ batch
    yield "hk_lq_solve_batch bad batch", "pl", lambda: L.hk_lq_solve_batch(pl, -1, 2, None, None, None, None, None, None, 3, None)
    yield "hk_lq_solve_batch N > 8", "pl", lambda: L.hk_lq_solve_batch(pl, 1, 9, None, None, None, None, None, None, 3, None)
    yield "hk_lq_solve_batch NULL", "pl", lambda: L.hk_lq_solve_batch(pl, 1, 2, None, None, None, None, None, None, 3, None)
    yield "hk_lq_solve_batch_device bad horizon", "pl", lambda: L.hk_lq_solve_batch_device(pl, 1, 2, None, None, None, None, None, None, -1, None, None)
    yield "hk_lq_solve_batch_device N > 8", "pl", lambda: L.hk_lq_solve_batch_device(pl, 1, 9, None, None, None, None, None, None, 3, None, None)
    # ---- while a rollout is open
    for name, hh in (("pa", pa), ("rc", rc)):
        yield None, name, (lambda hh=hh: L.hk_rollout_begin(hh, 4))
    yield "hk_rollout_begin already open", "pa", lambda: L.hk_rollout_begin(pa, 4)
    yield "hk_reset while open", "pa", lambda: L.hk_reset(pa, None, 0, -1)
    yield "hk_policy_attach while open", "rc", att(rc, good, [3], 1, P)
    yield "hk_policy_set_precision while open", "pa", lambda: L.hk_policy_set_precision(pa, 0, _lib.HK_POLICY_PREC_BF16)
    yield "hk_policy_memory_set while open", "rc", lambda: L.hk_policy_memory_set(rc, 0, f32(buf))
    yield "hk_set_agent_state while open", "pa", lambda: L.hk_set_agent_state(pa, far.ctypes.data_as(C.POINTER(_lib.AgentState)))
    yield "hk_set_env_state while open", "pa", lambda: L.hk_set_env_state(pa, buf.ctypes.data_as(C.POINTER(_lib.EnvState)))
    yield "hk_get_rewards while open", "pa", lambda: L.hk_get_rewards(pa, f32(buf), f32(buf[4096:]))
    yield "hk_rewards_device while open", "pa", lambda: L.hk_rewards_device(pa)
    yield "hk_rollout_episode_stats while open", "pa", lambda: L.hk_rollout_episode_stats(pa, 0, C.byref(st))
    yield None, "rc", lambda: L.hk_policy_pool_save(rc, 0, 0, 1)
    yield "hk_policy_pool_load while open", "rc", lambda: L.hk_policy_pool_load(rc, 0, 0, 1)
    yield "hk_step more decisions than rows", "pa", lambda: L.hk_step(pa, 5 * P)
    yield None, "pa", lambda: L.hk_step(pa, 1)
    yield "hk_rollout_close mid-interval", "pa", lambda: L.hk_rollout_close(pa)
    yield None, "pa", lambda: L.hk_step(pa, 1)
    yield None, "pa", lambda: L.hk_rollout_close(pa)
    yield None, "rc", lambda: L.hk_rollout_close(rc)
    # ---- after a rollout
    yield "hk_rollout_ptr MEMORY without a recurrent actor", "pa", ptr(lambda: L.hk_rollout_ptr(pa, _lib.RO_FIELDS["memory"][0]))
    yield "hk_rollout_episode_stats no completed row", "rc", lambda: L.hk_rollout_episode_stats(rc, 1, C.byref(st))
    c.keep = keep + (buf, i64, st, dbg, cid)          # (what the calls above point into, alive until the course ends)


def run_refusals(c):
    """-> [{label, code, handle, thread}]: the code, hk_last_error(h) (None for the NULL handle) and hk_last_error(NULL) after each refusal"""
    L, out = c.L, []
    for label, who, call in refusals(c):
        rc = call()
        if label is None:
            assert rc is not None and (rc == "NULL" or rc >= 0), "a set-up step of the course failed: %r %s" % (rc, L.hk_last_error(c.h[who]))
            continue
        hm = L.hk_last_error(c.h[who]).decode() if c.h[who] else None
        out.append({"label": label, "code": rc, "handle": hm, "thread": L.hk_last_error(None).decode()})
    return out


def good_calls(c):
    """one good call of every entry point, after the refusals (the handles hold a closed rollout and a pool) -> {entry point: SHA-256}"""
    L, out = c.L, {}
    pa, rc, pl = c.pa, c.rc, c.pl
    ck = _lib.check

    def ptr_read(g, p, nbytes):
        if not p:
            return np.frombuffer(b"NULL", np.uint8)
        g.synchronize()
        a = np.zeros(nbytes, np.uint8)
        _lib.copy_device_to_host(a.ctypes.data, p, nbytes)
        return a
    for name, g in (("pa", pa), ("rc", rc), ("pl", pl)):
        g.reset()
        g.step(24)
        out["hk_reset + hk_step(24) " + name] = sha(g.agent_state(), g.env_state(), g.observations(), g.episode_results())
    out["hk_get_mcts_state"] = sha(pa.mcts_state(), pl.mcts_state())
    out["hk_get_actions"] = sha(*rc.get_actions())
    steer = np.linspace(-1, 1, E * A).astype(np.float32); branch = (np.arange(E * A) % 3).astype(np.int32)
    pl.set_actions(steer, branch)
    out["hk_set_actions"] = sha(*pl.get_actions())
    out["hk_obs_dim"] = [g.obs_dim for g in (pa, rc, pl)] + [L.hk_obs_dim(c.ne)]
    obs = (np.random.default_rng(1).standard_normal((5, c.plain_pol.in_dim)) * 2).astype(np.float32)
    out["hk_policy_forward"] = sha(*rc.policy_forward(1, obs)) + " " + sha(*rc.policy_forward(1, obs[:0]))
    mem = np.random.default_rng(2).uniform(-1, 1, (5, 64)).astype(np.float32)
    out["hk_policy_forward_mem"] = sha(*rc.policy_forward(0, obs, mem)) + " " + sha(*rc.policy_forward(0, obs))
    out["hk_policy_memory_size"] = [L.hk_policy_memory_size(rc.h, 0), L.hk_policy_memory_size(rc.h, 1)]
    m = rc.policy_memory(0)
    out["hk_policy_memory_get"] = sha(m)
    rc.set_policy_memory(0, m[::-1] * 0.5)
    out["hk_policy_memory_set"] = sha(rc.policy_memory(0))
    pa.policy_set_precision(0, "bf16")
    out["hk_policy_set_precision"] = pa.policy_precision(0) + " " + sha(*pa.policy_forward(0, obs))
    pa.policy_set_precision(0, "f32")
    out["hk_policy_attach_lstm"] = rc.attach_policy(Policy.random(rc.obs_dim * 4, 32, 1, stack=4, seed=9, memory_size=64), [3], P)
    for name, g in (("pa", pa), ("rc", rc)):
        g.rollout_begin(6)
        g.step(3 * P)
        rows_open = g.rollout_rows()
        g.step(3 * P)
        g.rollout_close()
        ro = g.rollout()
        out["hk_rollout_* " + name] = [rows_open, g.rollout_rows(), sha(*[ro[k] for k in sorted(ro)])]
        out["hk_rollout_episode_stats " + name] = json.dumps(g.episode_stats(0), sort_keys=True)
    rc.rollout_begin(2)          # a smaller one in the buffer the first one grew, closed after one of its two rows
    rc.step(P)
    rc.rollout_close()
    out["hk_rollout_* rc again"] = [rc.rollout_rows(), sha(*[v for _, v in sorted(rc.rollout().items())])]
    # the pool made by the refusals: slot 0 holds policy 1
    n = L.hk_policy_pool_count(rc.h, 0)
    flat = np.zeros(n, np.float32)
    ck(L.hk_policy_pool_get(rc.h, 0, 0, f32(flat)), rc.h)
    out["hk_policy_pool_count / get"] = [n, sha(flat)]
    put = (flat * 0.5).astype(np.float32)
    ck(L.hk_policy_pool_put(rc.h, 0, 1, put.ctypes.data_as(fp)), rc.h)
    ck(L.hk_policy_pool_load(rc.h, 0, 1, 1), rc.h)
    ck(L.hk_policy_pool_save(rc.h, 0, 0, 1), rc.h)
    ck(L.hk_policy_pool_get(rc.h, 0, 0, f32(flat)), rc.h)
    out["hk_policy_pool_put / load / save"] = sha(flat) + " " + sha(*rc.policy_forward(1, obs))
    # setters: a state written back one env rotated
    st, es = pl.agent_state(), pl.env_state()
    pl.set_agent_state(np.roll(st, 1, axis=0)); pl.set_env_state(np.roll(es, 1))
    pl.step(7)
    out["hk_set_agent_state / hk_set_env_state"] = sha(pl.agent_state(), pl.env_state())
    out["hk_get_rewards"] = sha(*pa.rewards()) + " " + sha(*rc.rewards())
    for name, g in (("pa", pa), ("pl", pl)):
        g.step(3)
        g.observe(); g.rewards_device()
        ptrs = [(L.hk_device_obs_ptr(g.h), E * A * g.obs_dim * 4), (L.hk_device_reward_ptr(g.h), E * A * 4), (L.hk_device_group_reward_ptr(g.h), E * A * 4),
                (L.hk_device_act_steer_ptr(g.h), E * A * 4), (L.hk_device_act_branch_ptr(g.h), E * A * 4),
                (L.hk_device_agents_ptr(g.h), E * A * C.sizeof(_lib.AgentState)), (L.hk_device_results_ptr(g.h), E * A * C.sizeof(_lib.EpisodeResult))]
        out["hk_observe / hk_rewards_device / hk_device_*_ptr " + name] = sha(*[ptr_read(g, p, nb) for p, nb in ptrs])
        out["hk_stream " + name] = bool(L.hk_stream(g.h))
    # the communicator of the refusals (world size 1)
    out["hk_gather_count / hk_gather_results"] = sha(pl.gather_results())
    pl.comm_destroy()
    out["hk_comm_destroy"] = L.hk_comm_destroy(c.ne)
    # the LQ batch: twice, the second batch larger (its scratch grows)
    from oracle import lq_numpy as LQ
    rng = np.random.default_rng(0)
    lq = []
    for batch in (3, 9):
        games = [LQ.random_game(rng, 4) for _ in range(batch)]
        lq.append(hk.solve_feedback_lqr_batch(*[np.array([gm[k] for gm in games]) for k in range(6)], 3))
    out["hk_lq_solve_batch"] = sha(*lq)
    # the profiler: counts only (times differ run by run)
    pl.prof_enable(True); pl.prof_reset()
    pl.step(8)
    out["hk_prof_*"] = [{k: v[1] for k, v in pl.prof_read().items()}, pl.prof_games(), pl.prof_meter()]
    pl.prof_enable(False)
    out["hk_prof_reset / hk_prof_read / hk_synchronize without an environment"] = [L.hk_prof_reset(c.ne), L.hk_prof_read(c.ne, None, None), L.hk_synchronize(c.ne),
                                                                                   bool(L.hk_stream(c.ne))]
    sched = ("call_ticks", "rounds", "rounds_issued", "kernel", "streams", "ticks_per_launch", "optimistic_plan", "armed_in_first_launch", "planner", "actors")
    out["hk_schedule_info"] = [{k: g.schedule_info()[k] for k in sched} for g in (pa, rc, pl)]          # (not the meter's words: they arrive when they arrive)
    out["hk_get_lq_debug"] = sha(np.frombuffer(bytes(pl.lq_debug(2, 1)), np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the JSON here (default: stdout)")
    a = ap.parse_args()
    c = Course()
    out = {"refusals": run_refusals(c), "good calls": good_calls(c)}
    c.close()
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
