"""POCA trainer of an attached team policy, on the device (hk.h "POCA"): MA-POCA as ML-Agents 2.0 defines it — a centralised
critic with self-attention over the team's agents, a counterfactual baseline per agent, lambda-returns of the team reward — on the
rollout the recorder already produces.  A POCATrainer is a PPOTrainer whose critic is a PocaCritic and whose minibatch ids are GROUP ids:

    tr = env.poca_trainer(0)                     # policy 0's slots are one whole team; critic=None: PocaCritic.random
    env.rollout_begin(R); env.step(R * P); env.rollout_close()
    tr.advantages()                              # V, B over every row, team reward, lambda-returns
    stats = tr.update(epochs=3, minibatch=512, lr=3e-4)      # minibatch counts groups; stats has "L_b" beside PPO's six

Nothing is computed here: the arrays below only describe the flat parameter layout the library uses."""
import ctypes as C
import numpy as np
from . import _lib
from .ppo import PPOTrainer, param_layout, split_params, DEFAULTS

_DESC_ARRAYS = ("W_obs", "b_obs", "W_act", "b_act", "W_q", "b_q", "W_k", "b_k", "W_v", "b_v", "W_out", "b_out")


def critic_layout(in_dim, n_branch, hidden, n_layers):
    """-> [(name, shape)] of the POCA critic in the flat vector's order (the twin of ppo.param_layout; torch layout, W [out][in])"""
    H = hidden
    out = [("W_obs", (H, in_dim)), ("b_obs", (H,)), ("W_act", (H, in_dim + 1 + n_branch)), ("b_act", (H,))]
    for n in ("q", "k", "v", "out"):
        out += [("W_" + n, (H, H)), ("b_" + n, (H,))]
    for l in range(n_layers):
        out += [("W%d" % l, (H, H)), ("b%d" % l, (H,))]
    return out + [("w_val", (H,)), ("b_val", (1,))]


def critic_count(in_dim, n_branch, hidden, n_layers):
    """the number of critic parameters, in closed form"""
    H = hidden
    return H * in_dim + H + H * (in_dim + 1 + n_branch) + H + 4 * (H * H + H) + n_layers * (H * H + H) + H + 1


class PocaCritic:
    """The arrays of hk_poca_critic_desc (float32, torch layout): a dict name -> array in critic_layout's names"""

    def __init__(self, in_dim, n_branch, hidden, n_layers, arrays):
        self.in_dim, self.n_branch, self.hidden, self.n_layers = int(in_dim), int(n_branch), int(hidden), int(n_layers)
        self.arrays = {}
        for name, shape in critic_layout(self.in_dim, self.n_branch, self.hidden, self.n_layers):
            a = np.ascontiguousarray(arrays[name], np.float32)
            if a.shape != shape:
                raise ValueError("PocaCritic: %s is %s, not %s" % (name, a.shape, shape))
            self.arrays[name] = a

    @classmethod
    def random(cls, in_dim, n_branch, hidden, n_layers, seed=0):
        """numpy, seeded: normal with std sqrt(0.125 / H) for the two embeddings and the four attention maps, He-normal for the encoder and the
        head, zero biases"""
        rng = np.random.default_rng(int(seed))
        H = int(hidden)
        arrays = {}
        for name, shape in critic_layout(in_dim, n_branch, H, n_layers):
            if name.startswith("b"):
                arrays[name] = np.zeros(shape, np.float32)
            elif name in ("W_obs", "W_act", "W_q", "W_k", "W_v", "W_out"):
                arrays[name] = (rng.standard_normal(shape) * np.sqrt(0.125 / H)).astype(np.float32)
            else:
                arrays[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / H)).astype(np.float32)
        return cls(in_dim, n_branch, H, n_layers, arrays)

    def flat(self):
        """-> the critic part of PARAMS, float32"""
        return np.concatenate([self.arrays[n].reshape(-1) for n, _ in critic_layout(self.in_dim, self.n_branch, self.hidden, self.n_layers)])

    def desc(self):
        """-> (PocaCriticDesc, keep-alive list)"""
        d = _lib.PocaCriticDesc()
        d.hidden, d.n_layers, d.reserved0, d.reserved1 = self.hidden, self.n_layers, 0, 0
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        for n in _DESC_ARRAYS + ("w_val", "b_val"):
            setattr(d, n, fp(self.arrays[n]))
        for l in range(self.n_layers):
            d.W[l] = fp(self.arrays["W%d" % l])
            d.b[l] = fp(self.arrays["b%d" % l])
        return d, list(self.arrays.values())


class POCATrainer(PPOTrainer):
    """One POCA trainer of RacingEnv `env`'s attached policy `policy_index` (hk_ppo_create_poca): the policy's slots are one whole team of
    2 .. 4 agents.  critic: a PocaCritic or None (PocaCritic.random of H = 256, 2 layers); cfg: ppo.DEFAULTS' keys.  fp32 only."""
    KIND = "poca"

    def __init__(self, env, policy_index, critic=None, precision="f32", **cfg):
        if precision != "f32":
            raise ValueError("precision: a POCA trainer is fp32 only (hk.h \"POCA\")")
        bad = set(cfg) - set(DEFAULTS)
        if bad:
            raise TypeError("unknown PPO config keys: %s" % sorted(bad))
        self.env, self.index = env, int(policy_index)
        self.actor_policy = env._policies[self.index]
        a = self.actor_policy
        if critic is None:
            critic = PocaCritic.random(a.in_dim, a.n_branch, 256, 2, seed=0xC0CA + self.index)
        if (critic.in_dim, critic.n_branch) != (a.in_dim, a.n_branch):
            raise ValueError("critic: in_dim / n_branch differ from the actor's")
        self.critic_policy = critic
        c = dict(DEFAULTS, **cfg)
        self.cfg = c
        pc = _lib.PpoConfig(c["gamma"], c["lambd"], int(bool(c["normalize_advantages"])), c["adam_beta1"], c["adam_beta2"], c["adam_eps"],
                            int(c["seed"]) & 0xFFFFFFFF)
        d, _keep = critic.desc()
        rc = env.L.hk_ppo_create_poca(env.h, self.index, C.byref(d), C.byref(pc))
        if rc < 0:
            env._ck(rc)
        self.t = rc
        self.actor_layout = param_layout(a.in_dim, a.hidden, len(a.W), a.n_branch)
        self.critic_layout = critic_layout(a.in_dim, a.n_branch, critic.hidden, critic.n_layers)
        self.n_actor = sum(int(np.prod(s)) for _, s in self.actor_layout)
        self.last_report = None

    def set_precision(self, precision):
        if precision == "bf16":
            raise ValueError("precision: a POCA trainer is fp32 only (hk.h \"POCA\")")
        super().set_precision(precision)

    def poca_stats(self):
        """-> {"L_b": ...} belonging to the stats the last minibatch() / update() returned (synchronises)"""
        st = (C.c_float * _lib.HK_POCA_STATS)()
        self._ck(self.env.L.hk_poca_stats(self.env.h, self.t, st))
        return {"L_b": float(st[0])}

    def minibatch(self, ids, eps=0.2, beta=5e-3, stats=True):
        """ids: a torch int32 CUDA tensor of GROUP ids g = t E + e (out-of-range ids are skipped and counted).  -> PPO's stats and "L_b" """
        out = super().minibatch(ids, eps, beta, stats)
        if out is not None:
            out.update(self.poca_stats())
        return out

    def update(self, epochs=3, minibatch=512, lr=3e-4, eps=0.2, beta=5e-3, *, max_grad_norm=None, target_kl=None):
        """PPOTrainer.update with `minibatch` counting groups; -> PPO's stats and "L_b" """
        out = super().update(epochs, minibatch, lr, eps, beta, max_grad_norm=max_grad_norm, target_kl=target_kl)
        out.update(self.poca_stats())
        return out

    # ---- buffers: the HK_POCA_* fields beside the HK_PPO_* ones
    def _field(self, name):
        if name not in _lib.POCA_FIELDS:
            return super()._field(name)
        idx = _lib.POCA_FIELDS[name]
        n = self.env.L.hk_poca_count(self.env.h, self.t, idx)
        if n < 0:
            self._ck(n)
        ptr = self.env.L.hk_poca_ptr(self.env.h, self.t, idx)
        if not ptr:
            self._ck(_lib.HK_ERR_INVALID)
        return ptr, n

    def views(self):
        import torch
        out = super().views()

        class _Ext:
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (int(ptr), False), "version": 3, "strides": None}
        for name, idx in _lib.POCA_FIELDS.items():
            n = self.env.L.hk_poca_count(self.env.h, self.t, idx)
            ptr = self.env.L.hk_poca_ptr(self.env.h, self.t, idx) if n > 0 else None
            if ptr:
                out[name] = torch.as_tensor(_Ext(ptr, n), device="cuda:%d" % self.env.built.cfg.device_id)
        return out

    def critic_params(self, flat=None):
        flat = self.read("params") if flat is None else flat
        return split_params(flat[self.n_actor:], self.critic_layout)

    # ---- exact resume
    def _shapes(self):
        a, c = self.actor_policy, self.critic_policy
        return (np.array([a.in_dim, a.hidden, len(a.W), a.n_branch], np.int64), np.array([a.in_dim, c.hidden, c.n_layers, a.n_branch], np.int64))

    def state_dict(self):
        d = super().state_dict()
        d["kind"] = self.KIND
        return d
