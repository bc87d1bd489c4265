"""Host mirror of the reference's environment surface for the hot path, on top of libhk.so.

RacingEnv  <->  RacingEnvController (+ its KartAgents / ArcadeKarts), E independent instances on one GPU:
    reset(env_ids, experiment_num)   REC.ResetGame            (RacingEnvController.cs:499-719)
    step(n)                          n Unity FixedUpdate ticks
    observations()                   HierarchicalKartAgent.CollectObservations (HKA:485-604)
    set_actions(steer, branch)       KartAgent.OnActionReceived (KA:440-478) for LowMode == RL agents
    attach_policy(policy, slots)     BehaviorParameters.Model: the ML-Agents actor runs on device every DecisionPeriod ticks
    rollout_begin / rollout_close    record what the attached actors did (obs, actions, log-probs, rewards) on the device
    episode_stats(policy)            returns, lengths, wins / draws / losses of the closed rollout's episodes, reduced on the device
    snapshot_pool(policy, slots)     device slots of saved actors; load one into an attached policy (self-play opponent swaps)
    ppo_trainer(policy)              PPO on the recorded rows, on the device (ppo.PPOTrainer)
    poca_trainer(policy)             MA-POCA for a team's policy: attention critic, counterfactual baseline, team reward (poca.POCATrainer)
    agent_state() / set_agent_state  snapshot / restore of every KartAgent + ArcadeKart + Rigidbody field
    episode_results()                TelemetryViewer quantities of the last finished episode
All arrays are numpy views of the ABI structs; all compute happens in the HIP kernels."""
import ctypes as C
import numpy as np
from . import _lib
from .config import make_config, BuiltConfig

AGENT_DT = np.dtype(_lib.AgentState)
ENV_DT = np.dtype(_lib.EnvState)
RESULT_DT = np.dtype(_lib.EpisodeResult)


class RacingEnv:
    def __init__(self, built=None, **kw):
        self.built = built if isinstance(built, BuiltConfig) else make_config(**kw)
        self.L = _lib.load()
        self.h = C.c_void_p()
        rc = self.L.hk_create(C.byref(self.built.cfg), C.byref(self.h))
        _lib.check(rc, None)
        self.E, self.A = self.built.cfg.num_envs, self.built.cfg.num_agents
        self.obs_dim = self.L.hk_obs_dim(self.h)

    def schedule_info(self):
        """-> dict: the schedule the last hk_step of this handle ran (hk_schedule_info)"""
        import json
        txt = self.L.hk_schedule_info(self.h)
        return json.loads(txt.decode()) if txt else {}

    def close(self):
        if getattr(self, "h", None):
            self.L.hk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        return _lib.check(rc, self.h)

    def reset(self, env_ids=None, experiment_num=-1):
        if env_ids is None:
            self._ck(self.L.hk_reset(self.h, None, 0, int(experiment_num)))
        else:
            ids = np.ascontiguousarray(env_ids, np.int32)
            self._ck(self.L.hk_reset(self.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), int(experiment_num)))

    def step(self, n=1):
        self._ck(self.L.hk_step(self.h, int(n)))

    def synchronize(self):
        self._ck(self.L.hk_synchronize(self.h))

    def agent_state(self):
        out = np.zeros((self.E, self.A), AGENT_DT)
        self._ck(self.L.hk_get_agent_state(self.h, out.ctypes.data_as(C.POINTER(_lib.AgentState))))
        return out

    def set_agent_state(self, st):
        st = np.ascontiguousarray(st, AGENT_DT)
        assert st.shape == (self.E, self.A)
        self._ck(self.L.hk_set_agent_state(self.h, st.ctypes.data_as(C.POINTER(_lib.AgentState))))

    def env_state(self):
        out = np.zeros(self.E, ENV_DT)
        self._ck(self.L.hk_get_env_state(self.h, out.ctypes.data_as(C.POINTER(_lib.EnvState))))
        return out

    def set_env_state(self, st):
        st = np.ascontiguousarray(st, ENV_DT)
        assert st.shape == (self.E,)
        self._ck(self.L.hk_set_env_state(self.h, st.ctypes.data_as(C.POINTER(_lib.EnvState))))

    def episode_results(self):
        out = np.zeros((self.E, self.A), RESULT_DT)
        self._ck(self.L.hk_get_episode_results(self.h, out.ctypes.data_as(C.POINTER(_lib.EpisodeResult))))
        return out

    def rewards(self):
        """Agent.SendInfo: (m_Reward, m_GroupReward) collected since the last call, [E, A] each; both reset to 0"""
        r = np.zeros((self.E, self.A), np.float32)
        g = np.zeros((self.E, self.A), np.float32)
        self._ck(self.L.hk_get_rewards(self.h, r.ctypes.data_as(C.POINTER(C.c_float)), g.ctypes.data_as(C.POINTER(C.c_float))))
        return r, g

    def mcts_state(self):
        out = np.zeros((self.E, self.A), np.dtype(_lib.MctsState))
        self._ck(self.L.hk_get_mcts_state(self.h, out.ctypes.data_as(C.POINTER(_lib.MctsState))))
        return out

    def observations(self):
        out = np.zeros((self.E, self.A, self.obs_dim), np.float32)
        self._ck(self.L.hk_get_observations(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def set_actions(self, steer, branch):
        s = np.ascontiguousarray(steer, np.float32).reshape(self.E, self.A)
        b = np.ascontiguousarray(branch, np.int32).reshape(self.E, self.A)
        self._ck(self.L.hk_set_actions(self.h, s.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_int32))))

    def get_actions(self):
        s = np.zeros((self.E, self.A), np.float32)
        b = np.zeros((self.E, self.A), np.int32)
        self._ck(self.L.hk_get_actions(self.h, s.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_int32))))
        return s, b

    # ---- RL low-level policy on device
    POLICY_PRECISIONS = {"f32": _lib.HK_POLICY_PREC_F32, "bf16": _lib.HK_POLICY_PREC_BF16}

    def attach_policy(self, policy, agent_slots, decision_period=2, precision="f32"):
        """policy: hierarchicalkarting_amd.policy.Policy (e.g. Policy.from_onnx(path)); agent_slots: LowMode RL or E2E
        agents it drives; decision_period: DecisionRequester.DecisionPeriod (2 in the reference scenes); precision: policy_set_precision
        of the new policy.  -> policy index"""
        if precision not in self.POLICY_PRECISIONS:
            raise ValueError("precision: one of %s" % sorted(self.POLICY_PRECISIONS))
        d, _keep = policy.desc()
        slots = np.ascontiguousarray(agent_slots, np.int32)
        ld = policy.lstm_desc()
        if ld is None:
            rc = self.L.hk_policy_attach(self.h, C.byref(d), slots.ctypes.data_as(C.POINTER(C.c_int32)), len(slots), int(decision_period))
        else:           # a recurrent actor (hk.h "RECURRENT ACTORS")
            rc = self.L.hk_policy_attach_lstm(self.h, C.byref(d), C.byref(ld), slots.ctypes.data_as(C.POINTER(C.c_int32)), len(slots), int(decision_period))
        if rc < 0:
            self._ck(rc)
        self._policies = getattr(self, "_policies", []) + [policy]
        self._policy_slots = getattr(self, "_policy_slots", []) + [[int(a) for a in slots]]
        self._decision_period = int(decision_period)
        if precision != "f32":
            self.policy_set_precision(rc, precision)
        return rc

    def policy_set_precision(self, index, precision):
        """ "f32" (the default: the oracle's chain, bit for bit) or "bf16" (the trunk on the bf16 matrix cores, the bf16 trainer's forward bit
        for bit; hk.h beside hk_policy_attach); per policy, between calls, never while a rollout is open"""
        if precision not in self.POLICY_PRECISIONS:
            raise ValueError("precision: one of %s" % sorted(self.POLICY_PRECISIONS))
        self._ck(self.L.hk_policy_set_precision(self.h, int(index), self.POLICY_PRECISIONS[precision]))

    def policy_lstm_set_precision(self, index, precision):
        """policy_set_precision for a recurrent actor (hk_policy_lstm_set_precision; hk.h "RECURRENT ACTORS IN BF16"): "bf16" runs the trunk and the
        cell's gate products on the bf16 matrix cores, the recurrent bf16 trainer's forward bit for bit; the cell, the memory and the heads stay fp32"""
        if precision not in self.POLICY_PRECISIONS:
            raise ValueError("precision: one of %s" % sorted(self.POLICY_PRECISIONS))
        self._ck(self.L.hk_policy_lstm_set_precision(self.h, int(index), self.POLICY_PRECISIONS[precision]))

    def policy_precision(self, index):
        rc = self.L.hk_policy_get_precision(self.h, int(index))
        if rc < 0:
            self._ck(rc)
        return {v: k for k, v in self.POLICY_PRECISIONS.items()}[rc]

    def policy_forward(self, index, obs, memory=None):
        """the actor alone on stacked observations [rows, in_dim] -> (mu [rows], logits [rows, n_branch]); a recurrent actor takes
        memory [rows, memory_size] (None: zeros) and returns (mu, logits, memory_out [rows, memory_size]); its own memory is not touched"""
        pol = self._policies[index]
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, pol.in_dim)
        mu = np.zeros(obs.shape[0], np.float32)
        lg = np.zeros((obs.shape[0], pol.n_branch), np.float32)
        fp = C.POINTER(C.c_float)
        if not pol.memory_size:
            if memory is not None:
                raise ValueError("policy %d has no memory" % index)
            self._ck(self.L.hk_policy_forward(self.h, int(index), obs.shape[0], obs.ctypes.data_as(fp), mu.ctypes.data_as(fp), lg.ctypes.data_as(fp)))
            return mu, lg
        mem_in = None
        if memory is not None:
            mem_in = np.ascontiguousarray(memory, np.float32).reshape(obs.shape[0], pol.memory_size)
        out = np.zeros((obs.shape[0], pol.memory_size), np.float32)
        self._ck(self.L.hk_policy_forward_mem(self.h, int(index), obs.shape[0], obs.ctypes.data_as(fp), None if mem_in is None else mem_in.ctypes.data_as(fp),
                                              mu.ctypes.data_as(fp), lg.ctypes.data_as(fp), out.ctypes.data_as(fp)))
        return mu, lg, out

    def policy_memory(self, index):
        """-> [E, n_slots, memory_size]: the memory [h | c] of a recurrent actor's agents (synchronises)"""
        pol = self._policies[index]
        a = np.zeros((self.E, len(self._policy_slots[index]), pol.memory_size), np.float32)
        self._ck(self.L.hk_policy_memory_get(self.h, int(index), a.ctypes.data_as(C.POINTER(C.c_float))))
        return a

    def set_policy_memory(self, index, array):
        """write the memory of a recurrent actor's agents ([E, n_slots, memory_size]); it belongs to the episodes the envs are in now
        (hk.h hk_policy_memory_set); refused while a rollout is open"""
        pol = self._policies[index]
        a = np.ascontiguousarray(array, np.float32)
        if a.shape != (self.E, len(self._policy_slots[index]), pol.memory_size):
            raise ValueError("memory: expected shape %s" % ((self.E, len(self._policy_slots[index]), pol.memory_size),))
        self._ck(self.L.hk_policy_memory_set(self.h, int(index), a.ctypes.data_as(C.POINTER(C.c_float))))

    def policy_memory_clear(self, index):
        """zero the memory of a recurrent actor's agents on the device: set_policy_memory of zeros without the host array, asynchronous on the
        handle's stream (hk.h hk_policy_memory_clear); refused while a rollout is open"""
        self._ck(self.L.hk_policy_memory_clear(self.h, int(index)))

    def lq_debug(self, env, ego):
        d = _lib.LqDebug()
        self._ck(self.L.hk_get_lq_debug(self.h, env, ego, C.byref(d)))
        return d

    # ---- profiling taps used by bench.py
    def prof_enable(self, on=True):
        self._ck(self.L.hk_prof_enable(self.h, 1 if on else 0))

    def prof_reset(self):
        self._ck(self.L.hk_prof_reset(self.h))

    def prof_read(self):
        """-> {stage name: (total ms, launches)} since the last prof_reset (HIP events on the handle's stream)"""
        ms = (C.c_double * _lib.HK_PROF_STAGES)()
        n = (C.c_int64 * _lib.HK_PROF_STAGES)()
        self._ck(self.L.hk_prof_read(self.h, ms, n))
        return {name: (ms[i], n[i]) for i, name in enumerate(_lib.PROF_STAGE_NAMES)}

    def prof_games(self):
        """-> {N: multi-player LQ games of N players the solver kernels ran since the last prof_reset} (N = 2 .. 8)"""
        g = (C.c_int64 * (_lib.HK_MAX_AGENTS + 1))()
        self._ck(self.L.hk_prof_games(self.h, g))
        return {n: int(g[n]) for n in range(2, _lib.HK_MAX_AGENTS + 1)}

    def prof_games_words(self):
        """-> (in-wave solver passes, waves that ran any): hk_prof_games words [0], [1] since the last prof_reset"""
        g = (C.c_int64 * (_lib.HK_MAX_AGENTS + 1))()
        self._ck(self.L.hk_prof_games(self.h, g))
        return int(g[0]), int(g[1])

    def prof_meter(self):
        """-> int64[HK_METER_PARTS, 4]: the games-per-launch meter, per part: slots 0 .. 2 (B1 launch j of the part counts into j % 3), the decaying maximum"""
        w = (C.c_int64 * (4 * _lib.HK_METER_PARTS))()
        self._ck(self.L.hk_prof_meter(self.h, w))
        return [[int(w[4 * p + k]) for k in range(4)] for p in range(_lib.HK_METER_PARTS)]

    # ---- the path's one exchange step, natively over RCCL (hk_comm_* / hk_gather_results)
    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * _lib.HK_COMM_ID_BYTES)()
        _lib.check(_lib.load().hk_comm_unique_id(buf), None)
        return bytes(buf.raw)

    def comm_init(self, world_size, rank, comm_id):
        assert len(comm_id) == _lib.HK_COMM_ID_BYTES
        buf = (C.c_char * _lib.HK_COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._ck(self.L.hk_comm_init(self.h, int(world_size), int(rank), buf))
        self._comm_world = int(world_size)

    def comm_destroy(self):
        self._ck(self.L.hk_comm_destroy(self.h))
        self._comm_world = 0

    def gather_results(self):
        """-> hk_episode_result[E_total][A] on every rank, rank order (one RCCL all-gather; ranks may hold different E)"""
        tot = C.c_int64(0)
        self._ck(self.L.hk_gather_count(self.h, C.byref(tot)))
        out = np.zeros((int(tot.value), self.A), RESULT_DT)
        self._ck(self.L.hk_gather_results(self.h, out.ctypes.data_as(C.POINTER(_lib.EpisodeResult))))
        return out

    # ---- device-resident RL loop: zero-copy torch views of the library's buffers (PyTorch as plumbing, not as compute)
    def torch_views(self):
        """-> dict of torch CUDA tensors ALIASING libhk's device buffers: obs [E, A, obs_dim] f32, reward / group_reward [E, A] f32,
        act_steer [E, A] f32, act_branch [E, A] i32.  Fill them with observe() / rewards_device(), write actions in place,
        then step().  The handle's stream is not torch's current stream: call synchronize() (or use the stream pointer from
        hk_stream) before reading on another stream.  Import torch and touch the GPU (torch.cuda.init())
        BEFORE the first RacingEnv of the process: torch ships its own libamdhip64, and whichever HIP runtime is loaded first
        serves both libraries (the other order leaves torch without a device)."""
        import torch

        class _Ext:
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 3, "strides": None}

        dev = "cuda:%d" % self.built.cfg.device_id
        mk = lambda ptr, shape, ts: torch.as_tensor(_Ext(ptr, shape, ts), device=dev)
        E, A = self.E, self.A
        return {"obs": mk(self.L.hk_device_obs_ptr(self.h), (E, A, self.obs_dim), "<f4"),
                "reward": mk(self.L.hk_device_reward_ptr(self.h), (E, A), "<f4"),
                "group_reward": mk(self.L.hk_device_group_reward_ptr(self.h), (E, A), "<f4"),
                "act_steer": mk(self.L.hk_device_act_steer_ptr(self.h), (E, A), "<f4"),
                "act_branch": mk(self.L.hk_device_act_branch_ptr(self.h), (E, A), "<i4")}

    # ---- rollout recorder (hk.h hk_rollout_*): every decision of the attached actors writes a row of device buffers
    def rollout_begin(self, rows):
        self._ck(self.L.hk_rollout_begin(self.h, int(rows)))
        self._ro_rows = int(rows)

    def rollout_close(self):
        self._ck(self.L.hk_rollout_close(self.h))

    def rollout_rows(self):
        """completed rows: decisions whose interval has run"""
        n = self.L.hk_rollout_rows(self.h)
        if n < 0:
            self._ck(n)
        return n

    def _rollout_shapes(self):
        R, E, A, D = self._ro_rows, self.E, self.A, self.obs_dim
        pols = getattr(self, "_policies", [])
        nbm = max([p.n_branch for p in pols] + [1])
        smax = max([p.stack for p in pols] + [1])
        mem_max = max([p.memory_size for p in pols] + [0])
        sh = {n: (R, E, A) for n in _lib.RO_FIELDS}
        sh.update(obs=(R, E, A, D), logits=(R, E, A, nbm), done=(R, E), ring0=(E, A, smax - 1, D), next_obs=(E, A, D),
                  memory=(R, E, A, mem_max), next_memory=(E, A, mem_max))
        if mem_max == 0:          # no recurrent actor: the two fields have no elements and no pointer
            del sh["memory"], sh["next_memory"]
        return sh

    def rollout_views(self):
        """-> dict field -> torch CUDA tensor ALIASING the recorder's buffer (shapes: hk.h hk_rollout_field; all rows R of the last
        rollout_begin, of which rollout_rows() are complete).  The same caveats as torch_views: synchronize() before reading, and torch
        must have touched the GPU before the first RacingEnv of the process.  Valid until the next rollout_begin or close()."""
        import torch

        class _Ext:
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 3, "strides": None}

        dev = "cuda:%d" % self.built.cfg.device_id
        out = {}
        for name, shape in self._rollout_shapes().items():
            idx, ts = _lib.RO_FIELDS[name]
            ptr = self.L.hk_rollout_ptr(self.h, idx)
            if not ptr:
                self._ck(_lib.HK_ERR_INVALID)
            out[name] = torch.as_tensor(_Ext(ptr, shape, ts), device=dev)
        return out

    def rollout(self):
        """-> dict field -> numpy copy of the recorder's buffers (the handle's stream is synchronised first)"""
        self.synchronize()
        out = {}
        for name, shape in self._rollout_shapes().items():
            idx, ts = _lib.RO_FIELDS[name]
            ptr = self.L.hk_rollout_ptr(self.h, idx)
            if not ptr:
                self._ck(_lib.HK_ERR_INVALID)
            a = np.zeros(shape, np.dtype(ts))
            if a.size:
                _lib.copy_device_to_host(a.ctypes.data, ptr, a.nbytes)
            out[name] = a
        return out

    def episode_stats(self, policy_index):
        """-> dict of hk_episode_stats: episodes, partial, wins, draws, losses, timeouts, len_sum (ints), ret_sum, ret_sumsq, ret_min, ret_max,
        gret_sum, gret_sumsq (floats) of the closed rollout's completed rows, over the agent slots of the policy (hk.h "SELF-PLAY")"""
        st = _lib.EpisodeStats()
        self._ck(self.L.hk_rollout_episode_stats(self.h, int(policy_index), C.byref(st)))
        return {n: getattr(st, n) for n, _ in _lib.EpisodeStats._fields_}

    def snapshot_pool(self, policy_index, slots):
        """-> selfplay.SnapshotPool of the policy's shape (hk_policy_pool_create; hk_policy_pool_create_recurrent for a policy with memory)"""
        from .selfplay import SnapshotPool
        return SnapshotPool(self, policy_index, slots)

    def ppo_trainer(self, policy_index, critic=None, **cfg):
        """-> ppo.PPOTrainer of an attached policy (hk_ppo_create): it trains on this handle's closed rollouts and publishes into the policy.
        sequence_length=64 (PPOTrainer's named argument, passed through): a recurrent actor's trainer (hk_ppo_create_recurrent), truncated BPTT over windows of that many rows;
        critic_memory_size=256 with it (passed through too): the critic gets an LSTM cell of its own (hk_ppo_create_recurrent_critic)"""
        from .ppo import PPOTrainer
        return PPOTrainer(self, policy_index, critic, **cfg)

    def poca_trainer(self, policy_index, critic=None, **cfg):
        """-> poca.POCATrainer of an attached policy whose slots are one whole team (hk_ppo_create_poca); critic: a poca.PocaCritic or None (seeded random)"""
        from .poca import POCATrainer
        return POCATrainer(self, policy_index, critic, **cfg)

    def observe(self):
        self._ck(self.L.hk_observe(self.h))

    def rewards_device(self):
        self._ck(self.L.hk_rewards_device(self.h))

    def results_tensor(self):
        """-> torch CUDA uint8 tensor [E * A * 32] ALIASING the library's hk_episode_result[E][A] buffer (the payload of the result gather); the handle is
        settled and its stream synchronised first, so the view is complete"""
        import torch

        class _Ext:
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 3, "strides": None}
        ptr = self.L.hk_device_results_ptr(self.h)
        if not ptr:
            raise RuntimeError("hk_device_results_ptr: " + (self.L.hk_last_error(self.h) or b"").decode())
        self.synchronize()
        return torch.as_tensor(_Ext(ptr, self.E * self.A * RESULT_DT.itemsize), device="cuda:%d" % self.built.cfg.device_id)

    def device_results_ptr(self):
        return self.L.hk_device_results_ptr(self.h)
