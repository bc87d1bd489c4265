"""PPO trainer of an attached actor, on the device (hk.h "PPO trainer"): consumes a closed rollout of RacingEnv's recorder
and leaves updated weights in the attached policy, so that the next step() acts with them.

    tr = PPOTrainer(env, 0)                      # policy 0; critic=None: a seeded random critic of the actor's shape
    env.rollout_begin(R); env.step(R * P); env.rollout_close()
    tr.advantages()                              # critic over every row + the bootstrap inputs, GAE
    stats = tr.update(epochs=3, minibatch=512, lr=3e-4, eps=0.2, beta=5e-3)     # shuffle, minibatches, Adam; then publish
    tr.set_precision("bf16")                     # trunk products on the bf16 matrix cores, fp32 master weights (hk.h "PRECISION")
    tr.normalizer_init(); ...; tr.normalizer_update()     # the running input normaliser, folded from the closed rollout (hk.h "NORMALISER")
    tr.update(3, 512, 3e-4, max_grad_norm=0.5, target_kl=0.02); tr.last_report      # clip by the global norm, KL stop (hk.h "LONG RUNS")
    tr.save(path); ...; tr2.load(path)           # exact resume: masters, Adam moments, the two counters, precision, normaliser
    tr = PPOTrainer(env, 0, sequence_length=64)  # a recurrent actor: truncated BPTT over windows of 64 rows; ids and `minibatch` count sequences
    tr = PPOTrainer(env, 0, sequence_length=64, critic_memory_size=256)     # ... with a recurrent critic: an LSTM cell of its own (hk.h RECURRENT CRITIC)

Nothing is computed here: the arrays below only describe the flat parameter layout the library uses."""
import ctypes as C
import math
import numpy as np
from . import _lib
from .policy import Policy

DEFAULTS = dict(gamma=0.99, lambd=0.95, normalize_advantages=True, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, seed=0)
PRECISIONS = {"f32": _lib.HK_PPO_PREC_F32, "bf16": _lib.HK_PPO_PREC_BF16}
_DTYPES = {"perm": np.int32, "shadow": np.uint16, "clip": np.float64}       # every other HK_PPO_* field is float32
CHECKPOINT_FORMAT = 1


def bf16_round(x):
    """host twin of the device's fp32 -> bf16 rounding (hk_ppo.h ppo_bf16_rne): to nearest even, Inf kept, every NaN -> 0x7FC0.  -> uint16 bits"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), r)


def bf16_value(bits):
    """bf16 bit patterns (uint16) -> the float32 values they stand for"""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def gemm_bf16(env, epi, A, B, bias=None, aux=None):
    """One product of the trainer's bf16 kernel (hk_ppo_gemm_bf16, a debug tap) on uint16 bf16 bit patterns -> float32 [M, N].
    epi 1: swish(bias + A B^T), A [M, K], B [N, K];  epi 2: (A B) * swish'(aux), A [M, K], B [K, N], aux [M, N];  epi 0: A^T B, A [K, M], B [K, N]"""
    import torch
    A, B = np.ascontiguousarray(A, np.uint16), np.ascontiguousarray(B, np.uint16)
    if epi == 0:
        (K, M), N = A.shape, B.shape[1]
    else:
        (M, K), N = A.shape, (B.shape[0] if epi == 1 else B.shape[1])
    if B.shape != ((N, K) if epi == 1 else (K, N)):
        raise ValueError("gemm_bf16: the operands' shapes do not fit epi %d" % epi)
    dev = "cuda:%d" % env.built.cfg.device_id
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt).view(np.int16 if dt == np.uint16 else dt)).to(dev)
    a, b, bi, ax = up(A, np.uint16), up(B, np.uint16), up(bias, np.float32), up(aux, np.float32)
    if (bi is not None and bi.numel() != N) or (ax is not None and tuple(ax.shape) != (M, N)):
        raise ValueError("gemm_bf16: bias is [N], aux is [M, N]")
    c = torch.empty((M, N), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    env._ck(env.L.hk_ppo_gemm_bf16(env.h, int(epi), M, N, K, ptr(a), ptr(b), ptr(bi), ptr(ax), ptr(c)))
    env.synchronize()
    return c.cpu().numpy()


def lstm_gates_bf16(env, a, h, W_ih, W_hh, bsum):
    """The gate pre-activations of the recurrent bf16 chain (hk_ppo_lstm_gates_bf16, a debug tap: the trainer's Zx product, then one step kernel's
    gate chains without the cell) on uint16 bf16 bit patterns -> float32 z [rows, 4m].  a [rows, H], h [rows, m], W_ih [4m, H], W_hh [4m, m]
    (torch layout, gates i f g o), bsum [4m] float32"""
    import torch
    a, h, W_ih, W_hh = (np.ascontiguousarray(x, np.uint16) for x in (a, h, W_ih, W_hh))
    bsum = np.ascontiguousarray(bsum, np.float32)
    (rows, H), m = a.shape, h.shape[1]
    if h.shape != (rows, m) or W_ih.shape != (4 * m, H) or W_hh.shape != (4 * m, m) or bsum.shape != (4 * m,):
        raise ValueError("lstm_gates_bf16: a [rows, H], h [rows, m], W_ih [4m, H], W_hh [4m, m], bsum [4m]")
    dev = "cuda:%d" % env.built.cfg.device_id
    up = lambda x: torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to(dev)
    ta, th, tw, tu, tb = up(a), up(h), up(W_ih), up(W_hh), up(bsum)
    z = torch.empty((rows, 4 * m), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    env._ck(env.L.hk_ppo_lstm_gates_bf16(env.h, rows, H, m, ptr(ta), ptr(th), ptr(tw), ptr(tu), ptr(tb), ptr(z)))
    env.synchronize()
    return z.cpu().numpy()


def param_layout(in_dim, hidden, n_layers, n_branch, memory_size=0):
    """-> [(name, shape)] of one network in the flat vector's order (torch layout; n_branch 0: the critic, whose value head is W_mu / b_mu).
    memory_size > 0: a recurrent actor — the cell (W_ih, W_hh, b_ih, b_hh; gates i f g o) follows the trunk and the heads are m = memory_size / 2 wide;
    with n_branch 0: a recurrent critic — trunk, cell, then the value head W_mu [m], b_mu"""
    out = []
    for l in range(n_layers):
        out += [("W%d" % l, (hidden, in_dim if l == 0 else hidden)), ("b%d" % l, (hidden,))]
    head = hidden
    if memory_size:
        if memory_size < 2 or memory_size % 2:
            raise ValueError("memory_size: an even number >= 2 (it holds h and c)")
        head = memory_size // 2
        out += [("W_ih", (4 * head, hidden)), ("W_hh", (4 * head, head)), ("b_ih", (4 * head,)), ("b_hh", (4 * head,))]
    out += [("W_mu", (head,)), ("b_mu", (1,))]
    if n_branch:
        out += [("log_sigma", (1,)), ("W_branch", (n_branch, head)), ("b_branch", (n_branch,))]
    return out


def sequence_count(rows, sequence_length, n_envs, n_slots):
    """n_seq = ceil(R / L) E S of a recurrent trainer (hk.h "PPO trainer" RECURRENT)"""
    return -(-int(rows) // int(sequence_length)) * int(n_envs) * int(n_slots)


def sequence_rows(sid, rows, sequence_length, n_envs, n_slots):
    """sequence id s = (k E + e) S + j -> the row ids (t E + e) S + j of its window, t in [k L, min((k + 1) L, R)), time ascending; an id
    outside [0, n_seq) -> []"""
    R, L, ES = int(rows), int(sequence_length), int(n_envs) * int(n_slots)
    if not 0 <= sid < sequence_count(R, L, n_envs, n_slots):
        return []
    k, rem = divmod(int(sid), ES)
    return [t * ES + rem for t in range(k * L, min((k + 1) * L, R))]


def split_params(flat, layout):
    """flat vector (numpy or torch) -> dict name -> view of the given layout"""
    out, o = {}, 0
    for name, shape in layout:
        k = int(np.prod(shape))
        out[name] = flat[o:o + k].reshape(shape)
        o += k
    return out


def _hash(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def permutation(n, seed, count):
    """host twin of the device's row permutation (hk_ppo.h ppo_perm): a 4-round Feistel network keyed by (seed, count), cycle-walked into [0, n)"""
    bits = 2
    while bits < 32 and (1 << bits) < n:
        bits += 1
    hb = (bits + 1) >> 1
    mask = (1 << hb) - 1
    key = [_hash((seed & 0xFFFFFFFF) ^ _hash(count * 0x9E3779B9 + r * 0x85EBCA6B + 1)) for r in range(4)]
    i = np.arange(n, dtype=np.uint64)
    x = i.copy()
    todo = np.ones(n, bool)
    m64 = np.uint64(0xFFFFFFFF)

    def h(v):
        v = v & m64
        v ^= v >> np.uint64(16); v = (v * np.uint64(0x7FEB352D)) & m64
        v ^= v >> np.uint64(15); v = (v * np.uint64(0x846CA68B)) & m64
        v ^= v >> np.uint64(16)
        return v
    while todo.any():
        y = x[todo]
        lft, rgt = y >> np.uint64(hb), y & np.uint64(mask)
        for r in range(4):
            f = h(rgt ^ np.uint64(key[r])) & np.uint64(mask)
            lft, rgt = rgt, lft ^ f
        y = (lft << np.uint64(hb)) | rgt
        x[todo] = y
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def _normalizer_check(steps, mean, m2, in_dim=None):
    """the validity rules of hk_ppo_normalizer_set on the host -> (int steps, float64 mean, float64 m2); ValueError names the offender"""
    mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
    if int(steps) != steps or int(steps) < 1:
        raise ValueError("normaliser: steps must be an integer >= 1")
    if mean.ndim != 1 or mean.shape != m2.shape or (in_dim is not None and mean.size != in_dim):
        raise ValueError("normaliser: mean and m2 are [in_dim]%s" % ("" if in_dim is None else " = [%d]" % in_dim))
    if not np.isfinite(mean).all():
        raise ValueError("normaliser: a mean is not finite")
    if not (np.isfinite(m2) & (m2 > 0.0)).all():
        raise ValueError("normaliser: an m2 is not finite and > 0")
    return int(steps), np.ascontiguousarray(mean), np.ascontiguousarray(m2)


def normalizer_merge(steps, mean, m2, X):
    """host twin of hk_ppo_normalizer_update in float64 (ML-Agents' batch update; hk.h "NORMALISER"): folds the rows X [n, in_dim] — the
    UN-normalised stacked inputs, zero padding included — into the state.  -> (steps', mean', m2').  With c = x - mean:
        N' = N + n;  delta = sum c;  mean' = mean + delta / N';  m2' = m2 + sum (x - mean')(x - mean)
    The result does not depend, algebraically, on how the rows are split into successive calls."""
    steps, mean, m2 = _normalizer_check(steps, mean, m2)
    X = np.asarray(X, np.float64)
    if X.ndim != 2 or X.shape[1] != mean.size:
        raise ValueError("normalizer_merge: X is [n, %d]" % mean.size)
    n = X.shape[0]
    if n == 0:
        return steps, mean.copy(), m2.copy()
    N1 = steps + n
    c = X - mean
    mean1 = mean + c.sum(axis=0) / N1
    return N1, mean1, m2 + ((X - mean1) * c).sum(axis=0)


def normalizer_published(steps, mean, m2):
    """-> (norm_mean, norm_std) float32: the published form of a state, as the device rounds it"""
    return np.float32(np.asarray(mean, np.float64)), np.float32(np.sqrt(np.asarray(m2, np.float64) / np.float64(steps)))


def grad_norm(g):
    """host twin of the device's global gradient norm (hk.h "LONG RUNS"): sqrt of the exactly rounded sum (math.fsum) of the squares, which are
    exact in float64 for a float32 g.  -> float64; not finite when g holds a NaN or an Inf"""
    x = np.asarray(g, np.float64).reshape(-1)
    sq = x * x
    if not np.isfinite(sq).all():
        return np.float64(np.nan if np.isnan(sq).any() else np.inf)
    return np.float64(math.sqrt(math.fsum(sq.tolist())))


def clip_coefficient(norm, max_norm, dtype=np.float32):
    """host twin of the clip-aware step's coefficient: (float) min(1.0, (double)max_norm / (norm + 1e-6)) — torch's clip_coef, clamped — with
    max_norm taken as the float32 the C ABI receives.  -> np.float32, the device's value; dtype=np.float64: the expression before that one rounding"""
    return dtype(min(1.0, float(np.float32(max_norm)) / (float(norm) + 1e-6)))


def _flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        if "/" in str(k):
            raise ValueError("checkpoint: a key may not contain '/': %r" % (k,))
        if isinstance(v, dict):
            out.update(_flatten(v, prefix + str(k) + "/"))
        else:
            a = np.asarray(v)
            if a.dtype == object:
                raise ValueError("checkpoint: %s%s is not an array, a number or a string" % (prefix, k))
            out[prefix + str(k)] = a
    return out


def checkpoint_write(path, d):
    """one .npz of a (nested) dict of numpy arrays, numbers and strings; nested dicts are flattened with '/'.  No pickle.  "format" is added when absent"""
    flat = _flatten(dict({"format": CHECKPOINT_FORMAT}, **d))
    with open(path, "wb") as f:
        np.savez(f, **flat)


def checkpoint_read(path):
    """-> the dict checkpoint_write was given: arrays bit for bit with their dtypes, 0-d entries as Python scalars.  ValueError: no or an unknown "format" """
    out = {}
    with np.load(path, allow_pickle=False) as z:
        for key in z.files:
            a = z[key]
            node = out
            parts = key.split("/")
            for part in parts[:-1]:
                node = node.setdefault(part, {})
            node[parts[-1]] = a.item() if a.ndim == 0 else a
    if "format" not in out:
        raise ValueError("checkpoint: no 'format' entry")
    if out["format"] != CHECKPOINT_FORMAT:
        raise ValueError("checkpoint: format %r is not the format %d this version reads" % (out["format"], CHECKPOINT_FORMAT))
    return out


def _need(d, key, what="state"):
    if key not in d:
        raise ValueError("%s: missing key %r" % (what, key))
    return d[key]


def check_state(d, kind, actor_shape, critic_shape, sequence_length=0):
    """the host-only head of load_state_dict: a checkpoint's format, trainer kind (absent: "ppo"), the two network shapes (a recurrent critic's
    carries its memory size as a fifth entry) and the sequence length (absent: 0, not recurrent) against the loading trainer's; a recurrent
    critic's state must carry critic_mem_in / critic_mem_out; ValueError names the field"""
    if _need(d, "format") != CHECKPOINT_FORMAT:
        raise ValueError("state: format %r is not %d" % (d["format"], CHECKPOINT_FORMAT))
    if str(d.get("kind", "ppo")) != kind:
        raise ValueError("state: kind %r is not this trainer's %r" % (str(d.get("kind", "ppo")), kind))
    for key, want in (("actor_shape", actor_shape), ("critic_shape", critic_shape)):
        if not np.array_equal(np.asarray(_need(d, key)), np.asarray(want)):
            raise ValueError("state: %s %s differs from the trainer's %s" % (key, list(np.asarray(d[key])), list(np.asarray(want))))
    if int(d.get("sequence_length", 0)) != int(sequence_length):
        raise ValueError("state: sequence_length %d differs from the trainer's %d" % (int(d.get("sequence_length", 0)), int(sequence_length)))
    if len(np.asarray(critic_shape)) > 4:
        for key in ("critic_mem_in", "critic_mem_out"):
            a = np.asarray(_need(d, key))
            if a.dtype != np.float32 or a.ndim != 1 or a.size % int(np.asarray(critic_shape)[4]):
                raise ValueError("state: %s is float32 [E S %d]" % (key, int(np.asarray(critic_shape)[4])))


def _option(name, v, inf_ok):
    """an update option as hk_ppo_update_opts takes it: None -> 0 (off); negative, NaN (or infinite) -> ValueError"""
    if v is None:
        return 0.0
    v = float(v)
    if not v >= 0.0 or (math.isinf(v) and not inf_ok):
        raise ValueError("%s: >= 0%s (0 or None: off)" % (name, ", +inf allowed" if inf_ok else " and finite"))
    return v


class PPOTrainer:
    """One trainer of RacingEnv `env`'s attached policy `policy_index` (hk_ppo_create).  critic: a Policy with n_branch 0 semantics (its trunk and
    W_mu / b_mu are used) or None for Policy.random-style weights of the actor's shape; precision: "f32" | "bf16" (set_precision); cfg: DEFAULTS' keys.
    sequence_length: given for a recurrent actor (hk_ppo_create_recurrent): ids and `minibatch` then count sequences of that many rows.
    critic_memory_size (with sequence_length): the critic gets an LSTM cell of m_v = critic_memory_size / 2 units of its own
    (hk_ppo_create_recurrent_critic); critic: then a recurrent Policy of that memory size (trunk, cell, W_mu [m_v] / b_mu) or None for a seeded
    random one.  value_chunk_steps: time steps per value-pass launch (0: the default; the result does not depend on it)."""
    KIND = "ppo"          # a checkpoint's "kind" entry (absent in a PPO checkpoint: it reads as "ppo"); poca.POCATrainer: "poca"
    sequence_length = 0   # > 0: a recurrent trainer (set by __init__ when sequence_length is given)

    critic_memory_size = 0   # > 0: a recurrent critic

    def __init__(self, env, policy_index, critic=None, precision="f32", sequence_length=None, critic_memory_size=None, value_chunk_steps=0, **cfg):
        if precision not in PRECISIONS:
            raise ValueError("precision: one of %s" % sorted(PRECISIONS))
        bad = set(cfg) - set(DEFAULTS)
        if bad:
            raise TypeError("unknown PPO config keys: %s" % sorted(bad))
        self.env, self.index = env, int(policy_index)
        self.actor_policy = env._policies[self.index]
        a = self.actor_policy
        if critic_memory_size is not None and sequence_length is None:
            raise ValueError("critic_memory_size: a recurrent critic needs sequence_length (a recurrent actor's trainer)")
        self.critic_memory_size = 0 if critic_memory_size is None else int(critic_memory_size)
        if critic is None:
            critic = Policy.random(a.in_dim, a.hidden, len(a.W), n_branch=1, stack=a.stack, seed=0xC417 + self.index, normalize=False,
                                   memory_size=self.critic_memory_size)
        if critic_memory_size is not None and critic.memory_size != self.critic_memory_size:
            raise ValueError("critic: a recurrent Policy with memory_size %d (it has %d)" % (self.critic_memory_size, critic.memory_size))
        self.critic_policy = critic
        c = dict(DEFAULTS, **cfg)
        self.cfg = c
        pc = _lib.PpoConfig(c["gamma"], c["lambd"], int(bool(c["normalize_advantages"])), c["adam_beta1"], c["adam_beta2"], c["adam_eps"],
                            int(c["seed"]) & 0xFFFFFFFF)
        d, _keep = critic.desc()
        d.n_branch = 0
        d.W_branch = d.b_branch = None
        self.sequence_length = 0 if sequence_length is None else int(sequence_length)
        if sequence_length is None:
            rc = env.L.hk_ppo_create(env.h, self.index, C.byref(d), C.byref(pc))
        elif critic_memory_size is not None:
            rd = _lib.PpoRecurrentCriticDesc(self.sequence_length, int(value_chunk_steps), (C.c_int32 * 2)(0, 0))
            cell = critic.lstm_desc()
            rc = env.L.hk_ppo_create_recurrent_critic(env.h, self.index, C.byref(d), C.byref(cell) if cell is not None else None, C.byref(pc), C.byref(rd))
        else:
            rd = _lib.PpoRecurrentDesc(self.sequence_length, 0)
            rc = env.L.hk_ppo_create_recurrent(env.h, self.index, C.byref(d), C.byref(pc), C.byref(rd))
        if rc < 0:
            env._ck(rc)
        self.t = rc
        self.actor_layout = param_layout(a.in_dim, a.hidden, len(a.W), a.n_branch, a.memory_size if self.sequence_length else 0)
        self.critic_layout = param_layout(a.in_dim, critic.hidden, len(critic.W), 0, self.critic_memory_size)
        self.n_actor = sum(int(np.prod(s)) for _, s in self.actor_layout)
        self.last_report = None           # of the last update(): a dict when it was given an option, else None
        self.set_precision(precision)

    def _ck(self, rc):
        self.env._ck(rc)

    # ---- the entry points
    def set_precision(self, precision):
        """ "f32" (the default: exact) or "bf16" (trunk products on the bf16 matrix cores, fp32 masters); between calls, never inside one"""
        if precision not in PRECISIONS:
            raise ValueError("precision: one of %s" % sorted(PRECISIONS))
        self._ck(self.env.L.hk_ppo_set_precision(self.env.h, self.t, PRECISIONS[precision]))

    def set_recurrent_precision(self, precision):
        """set_precision for a recurrent actor's trainer (hk_ppo_recurrent_set_precision; hk.h "RECURRENT ACTORS IN BF16"): "bf16" puts the trunk, the
        gate products and the products of the cell's backward on the bf16 matrix cores — with env.policy_lstm_set_precision(index, "bf16") the
        training forward is the inference chain bit for bit; refused for a trainer with a recurrent critic"""
        if precision not in PRECISIONS:
            raise ValueError("precision: one of %s" % sorted(PRECISIONS))
        self._ck(self.env.L.hk_ppo_recurrent_set_precision(self.env.h, self.t, PRECISIONS[precision]))

    @property
    def precision(self):
        rc = self.env.L.hk_ppo_get_precision(self.env.h, self.t)
        if rc < 0:
            self._ck(rc)
        return {v: k for k, v in PRECISIONS.items()}[rc]

    def shadow(self):
        """-> the bf16 shadow of PARAMS as uint16 bit patterns in PARAMS' order (the critic's alignment gap removed)"""
        s = self.read("shadow")
        pad = s.size - self.read("params").size
        return np.concatenate([s[:self.n_actor], s[self.n_actor + pad:]])

    def advantages(self):
        self._ck(self.env.L.hk_ppo_advantages(self.env.h, self.t))

    def _on_handle_stream(self, t):
        """order the handle's stream after torch's current stream (t may still be being written there), and keep t's memory out of torch's
        caching allocator until the handle's stream has read it"""
        import torch
        hs = torch.cuda.ExternalStream(self.env.L.hk_stream(self.env.h), device=t.device)
        hs.wait_stream(torch.cuda.current_stream(t.device))
        t.record_stream(hs)

    def minibatch(self, ids, eps=0.2, beta=5e-3, stats=True):
        """ids: a torch int32 CUDA tensor of row ids (out-of-range ids are skipped), read on the handle's stream after whatever torch's current
        stream has queued.  -> dict of the stats (None: stats=False; the call then returns before the device has run it)"""
        if ids.dtype.itemsize != 4 or not ids.is_cuda or not ids.is_contiguous():
            raise TypeError("minibatch ids: a contiguous int32 CUDA tensor")
        self._on_handle_stream(ids)
        st = (C.c_float * _lib.HK_PPO_STATS)()
        self._ck(self.env.L.hk_ppo_minibatch(self.env.h, self.t, C.c_void_p(ids.data_ptr()), int(ids.numel()), float(eps), float(beta),
                                             st if stats else None))
        return dict(zip(_lib.PPO_STAT_NAMES, list(st))) if stats else None

    def adam(self, lr, max_grad_norm=None):
        """one Adam step from GRAD; max_grad_norm (> 0, inf: measure only): the clip-aware step of hk.h "LONG RUNS", see clip_words()"""
        if max_grad_norm is None:
            self._ck(self.env.L.hk_ppo_adam(self.env.h, self.t, float(lr)))
            return
        if not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm: > 0 (+inf measures only)")
        self._ck(self.env.L.hk_ppo_adam_clipped(self.env.h, self.t, float(lr), float(max_grad_norm)))

    def update(self, epochs=3, minibatch=512, lr=3e-4, eps=0.2, beta=5e-3, *, max_grad_norm=None, target_kl=None):
        """epochs x (device shuffle, minibatches, Adam), then publish.  -> stats (mean over the last epoch's minibatches).
        max_grad_norm: clip every step by the global L2 norm (inf: measure only); target_kl: no further epoch after one whose mean approx-KL
        exceeds it.  With either given, last_report is hk_ppo_update_report as a dict (else None)."""
        st = (C.c_float * _lib.HK_PPO_STATS)()
        if max_grad_norm is None and target_kl is None:
            self._ck(self.env.L.hk_ppo_update(self.env.h, self.t, int(epochs), int(minibatch), float(lr), float(eps), float(beta), st))
            self.last_report = None
            return dict(zip(_lib.PPO_STAT_NAMES, list(st)))
        o = _lib.PpoUpdateOpts(int(epochs), int(minibatch), float(lr), float(eps), float(beta), _option("max_grad_norm", max_grad_norm, True),
                               _option("target_kl", target_kl, False), 0)
        rep = _lib.PpoUpdateReport()
        self._ck(self.env.L.hk_ppo_update_opt(self.env.h, self.t, C.byref(o), st, C.byref(rep)))
        self.last_report = {n: getattr(rep, n) for n, _ in _lib.PpoUpdateReport._fields_ if n != "reserved"}
        return dict(zip(_lib.PPO_STAT_NAMES, list(st)))

    def clip_words(self):
        """-> dict of the HK_PPO_CLIP words (norm, coef of the last clip-aware step; steps, clipped, nonfinite, norm_sum, norm_max since create or
        the last update with an option); all 0 before the first clip-aware step"""
        n = self.env.L.hk_ppo_count(self.env.h, self.t, _lib.PPO_FIELDS["clip"])
        if n < 0:
            self._ck(n)
        return dict(zip(_lib.PPO_CLIP_NAMES, [float(x) for x in (self.read("clip") if n else np.zeros(8))]))

    def counters(self):
        """-> (adam_steps, epochs_done): the Adam step count of the bias corrections and the epoch count that keys the shuffle"""
        a, e = C.c_int64(0), C.c_int64(0)
        self._ck(self.env.L.hk_ppo_get_counters(self.env.h, self.t, C.byref(a), C.byref(e)))
        return int(a.value), int(e.value)

    def set_counters(self, adam_steps, epochs_done):
        self._ck(self.env.L.hk_ppo_set_counters(self.env.h, self.t, int(adam_steps), int(epochs_done)))

    def publish(self):
        self._ck(self.env.L.hk_ppo_publish(self.env.h, self.t))

    # ---- buffers
    def _field(self, name):
        idx = next(f[name] for f in (_lib.PPO_FIELDS, _lib.PPO_RECURRENT_FIELDS, _lib.PPO_RECURRENT_CRITIC_FIELDS) if name in f)
        n = self.env.L.hk_ppo_count(self.env.h, self.t, idx)
        if n < 0:
            self._ck(n)
        ptr = self.env.L.hk_ppo_ptr(self.env.h, self.t, idx)
        if not ptr:
            self._ck(_lib.HK_ERR_INVALID)
        return ptr, n

    def read(self, name):
        """-> numpy copy of an HK_PPO_* field, float32 (int32 for perm, uint16 for shadow, float64 for clip); the handle's stream is synchronised first"""
        self.env.synchronize()
        ptr, n = self._field(name)
        a = np.zeros(n, _DTYPES.get(name, np.float32))
        if n:
            _lib.copy_device_to_host(a.ctypes.data, ptr, a.nbytes)
        return a

    def views(self):
        """-> dict field -> torch CUDA tensor ALIASING the trainer's buffer, float32 (int32 for perm, int16 bits for shadow, float64 for clip); rollout_views' caveats apply"""
        import torch

        class _Ext:
            def __init__(self, ptr, n, ts):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": ts, "data": (int(ptr), False), "version": 3, "strides": None}
        out = {}
        for name, idx in (list(_lib.PPO_FIELDS.items()) + (list(_lib.PPO_RECURRENT_FIELDS.items()) if self.sequence_length else []) +
                          (list(_lib.PPO_RECURRENT_CRITIC_FIELDS.items()) if self.critic_memory_size else [])):
            n = self.env.L.hk_ppo_count(self.env.h, self.t, idx)
            ptr = self.env.L.hk_ppo_ptr(self.env.h, self.t, idx) if n > 0 else None
            if ptr:
                out[name] = torch.as_tensor(_Ext(ptr, n, {"perm": "<i4", "shadow": "<i2", "clip": "<f8"}.get(name, "<f4")), device="cuda:%d" % self.env.built.cfg.device_id)
        return out

    def write(self, name, a):
        """host array -> an HK_PPO_* field the contract calls writable (params, adam_m, adam_v, critic_mem_in, critic_mem_out); the size must fit"""
        self.env.synchronize()
        ptr, n = self._field(name)
        a = np.ascontiguousarray(a, _DTYPES.get(name, np.float32)).reshape(-1)
        if a.size != n:
            raise ValueError("%s: %d elements (given %d)" % (name, n, a.size))
        _lib.copy_host_to_device(ptr, a.ctypes.data, a.nbytes)

    def reset_critic_memory(self):
        """a recurrent critic: zero the carried critic memory — MEM_IN, which the next advantages() on the current rollout reads, and MEM_OUT,
        which the first advantages() on the next rollout starts from"""
        if not self.critic_memory_size:
            raise ValueError("reset_critic_memory: the trainer has no recurrent critic")
        for name in ("critic_mem_in", "critic_mem_out"):
            self.write(name, np.zeros(self._field(name)[1], np.float32))

    def actor_params(self, flat=None):
        flat = self.read("params") if flat is None else flat
        return split_params(flat[:self.n_actor], self.actor_layout)

    def critic_params(self, flat=None):
        flat = self.read("params") if flat is None else flat
        return split_params(flat[self.n_actor:], self.critic_layout)

    # ---- the running normaliser (hk.h "NORMALISER")
    def normalizer_init(self, steps=1):
        """state from the policy's current published statistics: N = steps, m = mean, M2 = std^2 steps (steps = 1 on mean 0, std 1: ML-Agents' start)"""
        self._ck(self.env.L.hk_ppo_normalizer_init(self.env.h, self.t, int(steps)))

    def normalizer_update(self):
        """fold the closed rollout's rows of this trainer into the state and publish; advantages() must run (again) before minibatch() / update()"""
        self._ck(self.env.L.hk_ppo_normalizer_update(self.env.h, self.t))

    def normalizer_state(self):
        """-> (steps, mean float64 [in_dim], m2 float64 [in_dim]); with normalizer_load, the normaliser's checkpoint"""
        k = self.actor_policy.in_dim
        steps, mean, m2 = C.c_int64(0), np.zeros(k, np.float64), np.zeros(k, np.float64)
        self._ck(self.env.L.hk_ppo_normalizer_get(self.env.h, self.t, C.byref(steps), C.c_void_p(mean.ctypes.data), C.c_void_p(m2.ctypes.data)))
        return int(steps.value), mean, m2

    def normalizer_load(self, steps, mean, m2):
        """load a state and publish it (validated here first: ValueError; the library applies the same rules)"""
        steps, mean, m2 = _normalizer_check(steps, mean, m2, self.actor_policy.in_dim)
        self._ck(self.env.L.hk_ppo_normalizer_set(self.env.h, self.t, steps, C.c_void_p(mean.ctypes.data), C.c_void_p(m2.ctypes.data)))

    def actor(self):
        """-> host Policy of the current master actor parameters (stack, seed and mode of the attached actor) with the policy's CURRENT published
        normaliser, read from the device: the attached actor's arrays bit for bit until a normalizer_update / normalizer_load publishes others"""
        a, p = self.actor_policy, self.actor_params()
        L = len(a.W)
        mean, std = a.norm_mean, a.norm_std
        if mean is not None:
            mean, std = self.read("norm_mean"), self.read("norm_std")
        lstm = {k: p[k] for k in Policy.LSTM_KEYS} if self.sequence_length else None          # a recurrent trainer: a recurrent Policy
        return Policy([p["W%d" % l] for l in range(L)], [p["b%d" % l] for l in range(L)], p["W_mu"], p["b_mu"], p["log_sigma"], p["W_branch"],
                      p["b_branch"], mean, std, a.stack, a.deterministic, a.seed, lstm)

    # ---- exact resume (hk.h "LONG RUNS"): a restored trainer fed the same rollout continues bit for bit
    def _shapes(self):
        a, c = self.actor_policy, self.critic_policy
        sa = [a.in_dim, a.hidden, len(a.W), a.n_branch] + ([a.memory_size] if self.sequence_length else [])
        return (np.array(sa, np.int64), np.array([a.in_dim, c.hidden, len(c.W), 0] + ([self.critic_memory_size] if self.critic_memory_size else []), np.int64))

    def state_dict(self):
        """-> dict of numpy arrays and scalars: format, the two network shapes, params / adam_m / adam_v, adam_steps, epochs_done, precision, cfg
        (for checking only) and, when one was initialised, the normaliser state"""
        sa, sc = self._shapes()
        steps, epochs = self.counters()
        d = dict(format=CHECKPOINT_FORMAT, actor_shape=sa, critic_shape=sc, params=self.read("params"), adam_m=self.read("adam_m"),
                 adam_v=self.read("adam_v"), adam_steps=steps, epochs_done=epochs, precision=self.precision,
                 cfg={k: (int(self.cfg[k]) & 0xFFFFFFFF if k == "seed" else int(bool(self.cfg[k])) if k == "normalize_advantages" else float(self.cfg[k]))
                      for k in DEFAULTS})
        if self.sequence_length:
            d["sequence_length"] = self.sequence_length
        if self.critic_memory_size:
            d["critic_mem_in"], d["critic_mem_out"] = self.read("critic_mem_in"), self.read("critic_mem_out")
        if self.actor_policy.norm_mean is not None:
            try:
                n, mean, m2 = self.normalizer_state()
                d["normalizer"] = dict(steps=n, mean=mean, m2=m2)
            except _lib.HkError:          # no normaliser state: the statistics are the frozen ones of the attached policy
                pass
        return d

    def load_state_dict(self, d):
        """validate (ValueError names the field: shapes, cfg — a differing shuffle seed would not continue the permutations), then restore the
        counters, the three vectors, the precision and the normaliser if present, and publish; the library refuses it while a rollout is open"""
        check_state(d, self.KIND, *self._shapes(), sequence_length=self.sequence_length)
        cfg = _need(d, "cfg")
        for k in DEFAULTS:
            mine = int(self.cfg[k]) & 0xFFFFFFFF if k == "seed" else int(bool(self.cfg[k])) if k == "normalize_advantages" else float(self.cfg[k])
            if _need(cfg, k, "state cfg") != mine:
                raise ValueError("state: cfg %s = %r differs from the trainer's %r" % (k, cfg[k], mine))
        if _need(d, "precision") not in PRECISIONS:
            raise ValueError("state: precision %r" % (d["precision"],))
        P = self.env.L.hk_ppo_count(self.env.h, self.t, _lib.PPO_FIELDS["params"])
        vec = {}
        for name in ("params", "adam_m", "adam_v"):
            a = np.asarray(_need(d, name))
            if a.dtype != np.float32 or a.shape != (P,):
                raise ValueError("state: %s is float32 [%d]" % (name, P))
            vec[name] = np.ascontiguousarray(a)
        norm = d.get("normalizer")
        if norm is not None:
            norm = _normalizer_check(_need(norm, "steps", "state normalizer"), _need(norm, "mean", "state normalizer"),
                                     _need(norm, "m2", "state normalizer"), self.actor_policy.in_dim)
            if self.actor_policy.norm_mean is None:
                raise ValueError("state: normalizer given, but the policy was attached without statistics")
        cmem = {}
        if self.critic_memory_size:
            for name in ("critic_mem_in", "critic_mem_out"):
                n = self.env.L.hk_ppo_count(self.env.h, self.t, _lib.PPO_RECURRENT_CRITIC_FIELDS[name])
                if np.asarray(d[name]).shape != (n,):
                    raise ValueError("state: %s is float32 [%d]" % (name, n))
                cmem[name] = np.ascontiguousarray(d[name])
        self.set_counters(_need(d, "adam_steps"), _need(d, "epochs_done"))          # (the library's refusals come first: nothing is written after one)
        self.env.synchronize()
        for name, a in vec.items():
            ptr, _ = self._field(name)
            _lib.copy_host_to_device(ptr, a.ctypes.data, a.nbytes)
        for name, a in cmem.items():
            self.write(name, a)
        if self.sequence_length and not self.critic_memory_size:
            self.set_recurrent_precision(d["precision"])
        else:
            self.set_precision(d["precision"])
        if norm is not None:
            self.normalizer_load(*norm)
        self.publish()

    def save(self, path):
        checkpoint_write(path, self.state_dict())

    def load(self, path):
        self.load_state_dict(checkpoint_read(path))
