"""Self-play for the PPO trainer (hk.h "SELF-PLAY"): what ML-Agents' `self_play:` block and its linear schedules do, as host
bookkeeping on top of three device facilities — the snapshot pool (hk_policy_pool_*), the episode statistics of a closed rollout
(hk_rollout_episode_stats) and the trainer (ppo.PPOTrainer).

    learner, opponent = env.attach_policy(pol, [0, 1]), env.attach_policy(pol, [2, 3])
    tr = env.ppo_trainer(learner)
    sp = SelfPlay(env, tr, opponent, window=10, save_steps=20000, swap_steps=10000, max_steps=5_000_000)
    for _ in range(iterations):
        out = sp.iteration(rows=64, epochs=3, minibatch=512, lr=3e-4, eps=0.2, beta=5e-3)      # out["elo"], out["stats"], out["update"]
    ppo.checkpoint_write(path, sp.state_dict()); ...; sp2.load_state_dict(ppo.checkpoint_read(path))     # ratings, cursor, generator, pool slots

Nothing is computed on the host but ratings, schedules and which slot plays next.  Out of scope: team_change (a trainer is bound to one
policy), per-env opponents, bf16 POCA.  The trainer may be a poca.POCATrainer: nothing here is bound to the critic's kind.  It may be a
recurrent PPOTrainer (sequence_length, with or without critic_memory_size): the pool is then a recurrent one (hk_policy_pool_create_recurrent,
DESIGN §19), whose slots carry the LSTM cell; a swap keeps the opponent's memory unless reset_opponent_memory is set."""
import ctypes as C
import json
import numpy as np
from .policy import Policy
from .ppo import CHECKPOINT_FORMAT, param_layout, split_params

SCHEDULE_MINIMA = dict(lr=1e-10, eps=0.1, beta=1e-5)       # ML-Agents' floors of the three linear decays


def elo_expected(r1, r2):
    """the expected result of a player rated r1 against one rated r2"""
    return 1.0 / (1.0 + 10.0 ** ((float(r2) - float(r1)) / 400.0))


def elo_apply(r_learner, r_opp, wins, draws, losses, k=1.0):
    """-> (r_learner', r_opp') in float64 after a rollout's wins, draws and losses of the learner: n = W + D + L sequential steps of
    change = k (s - elo_expected(r_learner, r_opp)), r_learner += change, r_opp -= change, with the MEAN result s = (W + D / 2) / n.
    ML-Agents applies each episode's own result in arrival order; the episodes of a rollout end together and have no order.  The mean-result
    form is order-free, equals ML-Agents' sequence when all results agree, and is self-limiting (every step moves towards the rating
    difference at which s is the expectation), where a one-shot change of n (s - e) would move ratings by thousands of points."""
    rl, ro = float(r_learner), float(r_opp)
    n = int(wins) + int(draws) + int(losses)
    if n <= 0:
        return rl, ro
    s = (int(wins) + 0.5 * int(draws)) / n
    for _ in range(n):
        change = float(k) * (s - elo_expected(rl, ro))
        rl += change
        ro -= change
    return rl, ro


def linear_schedule(initial, minimum, step, max_steps):
    """ML-Agents' linear decay: (initial - minimum) (1 - min(step, max_steps) / max_steps) + minimum"""
    frac = min(float(step), float(max_steps)) / float(max_steps)
    return (float(initial) - float(minimum)) * (1.0 - frac) + float(minimum)


def policy_to_flat(pol):
    """Policy -> the flat float32 vector of a pool slot: the actor in the trainer's torch layout, then norm_mean, norm_std when it normalises.
    A Policy with memory: the cell (W_ih, W_hh, b_ih, b_hh) between the trunk and the heads, as param_layout(..., memory_size) orders it"""
    parts = []
    for l in range(len(pol.W)):
        parts += [pol.W[l].reshape(-1), pol.b[l]]
    if pol.lstm:
        parts += [pol.lstm[k].reshape(-1) for k in Policy.LSTM_KEYS]
    parts += [pol.W_mu, pol.b_mu, pol.log_sigma, pol.W_branch.reshape(-1), pol.b_branch]
    if pol.norm_mean is not None:
        parts += [pol.norm_mean, pol.norm_std]
    return np.ascontiguousarray(np.concatenate(parts), np.float32)


def flat_to_policy(flat, like):
    """a slot's flat vector -> Policy with the stack, seed and mode of `like` (whose shape, memory size included, it must have)"""
    layout = param_layout(like.in_dim, like.hidden, len(like.W), like.n_branch, like.memory_size)
    n = sum(int(np.prod(s)) for _, s in layout)
    p = split_params(flat[:n], layout)
    mean = std = None
    if like.norm_mean is not None:
        mean, std = flat[n:n + like.in_dim], flat[n + like.in_dim:n + 2 * like.in_dim]
    L = len(like.W)
    lstm = {k: p[k] for k in Policy.LSTM_KEYS} if like.memory_size else None
    return Policy([p["W%d" % l] for l in range(L)], [p["b%d" % l] for l in range(L)], p["W_mu"], p["b_mu"], p["log_sigma"], p["W_branch"],
                  p["b_branch"], mean, std, like.stack, like.deterministic, like.seed, lstm)


class SnapshotPool:
    """`slots` device slots of attached policy `policy_index`'s shape (hk_policy_pool_create; hk_policy_pool_create_recurrent when that policy
    has memory, whose size is then part of the shape).  save / load move a slot from / into an attached policy of that shape on the device;
    put / get exchange it with a host Policy.  A load never touches the policy's memory (env.policy_memory_clear does)."""

    def __init__(self, env, policy_index, slots):
        self.env, self.index, self.slots = env, int(policy_index), int(slots)
        self.like = env._policies[self.index]
        create = env.L.hk_policy_pool_create_recurrent if self.like.memory_size else env.L.hk_policy_pool_create
        rc = create(env.h, self.index, self.slots)
        if rc < 0:
            env._ck(rc)
        self.pool = rc
        self.count = env.L.hk_policy_pool_count(env.h, self.pool)
        if self.count < 0:
            env._ck(self.count)

    def save(self, slot, policy_index=None):
        """the policy's current inference weights and published statistics -> slot (asynchronous); policy_index None: the pool's policy"""
        self.env._ck(self.env.L.hk_policy_pool_save(self.env.h, self.pool, int(slot), self.index if policy_index is None else int(policy_index)))

    def load(self, slot, policy_index):
        """slot -> the attached policy (refused for a policy that has a trainer, and while a rollout is open)"""
        self.env._ck(self.env.L.hk_policy_pool_load(self.env.h, self.pool, int(slot), int(policy_index)))

    def put(self, slot, policy):
        flat = policy_to_flat(policy)
        if flat.size != self.count or policy.memory_size != self.like.memory_size:
            raise ValueError("SnapshotPool.put: the Policy has %d parameters, a slot of this pool %d" % (flat.size, self.count))
        self.env._ck(self.env.L.hk_policy_pool_put(self.env.h, self.pool, int(slot), flat.ctypes.data_as(C.POINTER(C.c_float))))

    def get(self, slot):
        """-> host Policy of the slot, with the stack, seed and mode of the pool's policy (as PPOTrainer.actor())"""
        flat = np.zeros(self.count, np.float32)
        self.env._ck(self.env.L.hk_policy_pool_get(self.env.h, self.pool, int(slot), flat.ctypes.data_as(C.POINTER(C.c_float))))
        return flat_to_policy(flat, self.like)

    def get_flat(self, slot):
        """-> the slot's flat float32 vector as it lies on the device (hk_policy_pool_get)"""
        flat = np.zeros(self.count, np.float32)
        self.env._ck(self.env.L.hk_policy_pool_get(self.env.h, self.pool, int(slot), flat.ctypes.data_as(C.POINTER(C.c_float))))
        return flat

    def put_flat(self, slot, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        if flat.shape != (self.count,):
            raise ValueError("SnapshotPool.put_flat: a slot of this pool is float32 [%d]" % self.count)
        self.env._ck(self.env.L.hk_policy_pool_put(self.env.h, self.pool, int(slot), flat.ctypes.data_as(C.POINTER(C.c_float))))


class SelfPlay:
    """ML-Agents' self-play loop around one trainer (the learner) and one attached opponent policy of the same shape.
    The pool has window + 1 slots: slots 0 .. window - 1 are the snapshot window, the last holds "latest" (the learner as of the swap that
    picked it).  Steps are counted in learner rows (rows x E x the learner's agent slots per rollout).  Every save_steps the learner is saved
    into slot cursor % window with its rating; every swap_steps the opponent is redrawn from numpy.random.default_rng(seed): with
    probability play_against_latest_model_ratio the latest learner (whose rating is the learner's own and is not decremented), otherwise
    uniformly one of the filled window slots.  Until the first swap the opponent plays the weights it was attached with, rated initial_elo.
    pool: a SnapshotPool-like object (save(slot), load(slot, policy_index)); None: a SnapshotPool of the learner's shape.
    The trainer may be recurrent (sequence_length, with or without critic_memory_size): the pool is then a recurrent one, `minibatch` of
    iteration() counts sequences as PPOTrainer.update defines, and steps are still learner rows.  A swap keeps the opponent's memory, as
    ML-Agents' ghost swap does; reset_opponent_memory=True clears it on the device after every load (env.policy_memory_clear)."""

    def __init__(self, env, trainer, opponent_index, window=10, play_against_latest_model_ratio=0.5, save_steps=20000, swap_steps=10000,
                 initial_elo=400.0, max_steps=None, seed=0, pool=None, reset_opponent_memory=False):
        if window < 1 or save_steps < 1 or swap_steps < 1 or not 0.0 <= play_against_latest_model_ratio <= 1.0:
            raise ValueError("SelfPlay: window, save_steps, swap_steps >= 1 and 0 <= play_against_latest_model_ratio <= 1")
        self.env, self.trainer, self.opponent_index = env, trainer, int(opponent_index)
        self.reset_opponent_memory = bool(reset_opponent_memory)
        self.window, self.ratio = int(window), float(play_against_latest_model_ratio)
        self.save_steps, self.swap_steps, self.max_steps = int(save_steps), int(swap_steps), max_steps
        self.pool = SnapshotPool(env, trainer.index, self.window + 1) if pool is None else pool
        self.rng = np.random.default_rng(seed)
        self.elo = float(initial_elo)                       # the learner's rating
        self.ratings = [float(initial_elo)] * self.window   # of the window slots, as of their save (then moved by the games played against them)
        self.attached_elo = float(initial_elo)              # of the weights the opponent was attached with
        self.cursor = 0                                     # saves so far; the next goes to slot cursor % window
        self.opponent = None                                # None: as attached; "latest"; or a window slot
        self.steps = self.last_save = self.last_swap = 0
        self.history = []                                   # the opponents drawn, in order
        self._save()

    # ---- bookkeeping (no device work but pool.save / pool.load)
    def _save(self):
        slot = self.cursor % self.window
        self.pool.save(slot)
        self.ratings[slot] = self.elo
        self.cursor += 1
        return slot

    def _load(self, slot):
        self.pool.load(slot, self.opponent_index)
        if self.reset_opponent_memory:
            self.env.policy_memory_clear(self.opponent_index)

    def _swap(self):
        filled = min(self.cursor, self.window)
        if self.rng.random() < self.ratio:
            pick = "latest"
            self.pool.save(self.window)
            self._load(self.window)
        else:
            pick = int(self.rng.integers(filled))
            self._load(pick)
        self.opponent = pick
        self.history.append(pick)
        return pick

    def opponent_elo(self):
        if self.opponent is None:
            return self.attached_elo
        return self.elo if self.opponent == "latest" else self.ratings[self.opponent]

    def record_results(self, wins, draws, losses):
        """elo_apply of a rollout's results against the current opponent; the latest learner's rating is the learner's own and is not decremented"""
        new_l, new_o = elo_apply(self.elo, self.opponent_elo(), wins, draws, losses)
        if self.opponent is None:
            self.attached_elo = new_o
        elif self.opponent != "latest":
            self.ratings[self.opponent] = new_o
        self.elo = new_l

    def advance(self, n_rows):
        """count a rollout's learner rows; save and swap when due -> (saved slot or None, new opponent or None)"""
        self.steps += int(n_rows)
        saved = swapped = None
        if self.steps - self.last_save >= self.save_steps:
            saved, self.last_save = self._save(), self.steps
        if self.steps - self.last_swap >= self.swap_steps:
            swapped, self.last_swap = self._swap(), self.steps
        return saved, swapped

    def scheduled(self, lr, eps, beta, schedules=None, minima=None):
        """-> (lr, eps, beta) at the current step count; schedules: name -> "linear" | "constant" (default: all linear when max_steps is set)"""
        vals = dict(lr=float(lr), eps=float(eps), beta=float(beta))
        sch = dict.fromkeys(vals, "linear" if self.max_steps else "constant")
        sch.update(schedules or {})
        mins = dict(SCHEDULE_MINIMA, **(minima or {}))
        for k, kind in sch.items():
            if kind not in ("linear", "constant") or k not in vals:
                raise ValueError("schedules: lr / eps / beta -> 'linear' | 'constant'")
            if kind == "linear":
                if not self.max_steps:
                    raise ValueError("a linear schedule needs max_steps")
                vals[k] = linear_schedule(vals[k], mins[k], self.steps, self.max_steps)
        return vals["lr"], vals["eps"], vals["beta"]

    # ---- checkpoint of the bookkeeping and the pool (the trainer has its own: PPOTrainer.state_dict)
    _PICK = {None: -2, "latest": -1}          # an opponent as an integer: as attached, latest, or the window slot itself

    def state_dict(self, include_pool=True):
        """-> dict of numpy arrays and scalars (ppo.checkpoint_write takes it): elo, ratings, attached_elo, cursor, opponent, steps, last_save,
        last_swap, history (None -2, "latest" -1, else the slot), the generator's bit_generator.state as a JSON string and, with include_pool,
        the flat vectors of the filled slots.  Env state and the policies' decision counters are not part of it (env_state / set_env_state)."""
        code = lambda x: self._PICK.get(x, x)
        d = dict(format=CHECKPOINT_FORMAT, window=self.window, elo=self.elo, ratings=np.asarray(self.ratings, np.float64), attached_elo=self.attached_elo,
                 cursor=self.cursor, opponent=int(code(self.opponent)), steps=self.steps, last_save=self.last_save, last_swap=self.last_swap,
                 history=np.asarray([code(x) for x in self.history], np.int64), rng=json.dumps(self.rng.bit_generator.state),
                 reset_opponent_memory=int(self.reset_opponent_memory))
        if include_pool:
            slots = list(range(min(self.cursor, self.window))) + ([self.window] if "latest" in self.history else [])
            d["pool"] = {"slot%d" % s: self.pool.get_flat(s) for s in slots}
        return d

    def load_state_dict(self, d):
        """restore what state_dict stored; the slots are put back, and an opponent that is not None is loaded into the opponent policy (None, "as
        attached", is the caller's to restore, as it is at construction; so is the opponent's memory, which this load does not clear whatever
        the flag says: a resume continues the episode in progress).  reset_opponent_memory is taken from the state when it has the key.
        ValueError: a missing key, another format or window, a slot of another length than the pool's (nothing is put then)"""
        for k in ("format", "window", "elo", "ratings", "attached_elo", "cursor", "opponent", "steps", "last_save", "last_swap", "history", "rng"):
            if k not in d:
                raise ValueError("SelfPlay state: missing key %r" % k)
        if d["format"] != CHECKPOINT_FORMAT:
            raise ValueError("SelfPlay state: format %r is not %d" % (d["format"], CHECKPOINT_FORMAT))
        if int(d["window"]) != self.window or len(d["ratings"]) != self.window:
            raise ValueError("SelfPlay state: window %r differs from this object's %d" % (d["window"], self.window))
        pick = lambda c: {v: k for k, v in self._PICK.items()}.get(int(c), int(c))
        rng_state = json.loads(str(d["rng"]))
        if rng_state.get("bit_generator") != type(self.rng.bit_generator).__name__:
            raise ValueError("SelfPlay state: rng is a %r state" % rng_state.get("bit_generator"))
        count = getattr(self.pool, "count", None)
        for name, flat in sorted(d.get("pool", {}).items()):
            if count is not None and np.asarray(flat).size != count:
                raise ValueError("SelfPlay state: %s has %d floats, a slot of this pool %d (another shape or memory size)" % (name, np.asarray(flat).size, count))
        for name, flat in sorted(d.get("pool", {}).items()):
            self.pool.put_flat(int(name[4:]), flat)
        if "reset_opponent_memory" in d:
            self.reset_opponent_memory = bool(int(d["reset_opponent_memory"]))
        self.elo, self.attached_elo = float(d["elo"]), float(d["attached_elo"])
        self.ratings = [float(x) for x in d["ratings"]]
        self.cursor, self.steps, self.last_save, self.last_swap = int(d["cursor"]), int(d["steps"]), int(d["last_save"]), int(d["last_swap"])
        self.history = [pick(c) for c in np.asarray(d["history"]).reshape(-1)]
        self.opponent = pick(d["opponent"])
        self.rng.bit_generator.state = rng_state
        if self.opponent is not None:
            self.pool.load(self.window if self.opponent == "latest" else self.opponent, self.opponent_index)

    # ---- one rollout + update
    def iteration(self, rows, epochs=3, minibatch=512, lr=3e-4, eps=0.2, beta=5e-3, schedules=None, minima=None, **update_opts):
        """rollout begin, step, close; episode_stats of the learner; elo_apply against the current opponent; advantages; update with the
        scheduled values (update_opts: max_grad_norm / target_kl, passed through; the result then has "report"); then save / swap when due.  -> dict"""
        env, tr = self.env, self.trainer
        env.rollout_begin(rows)
        env.step(int(rows) * env._decision_period)
        env.rollout_close()
        stats = env.episode_stats(tr.index)
        played = self.opponent
        self.record_results(stats["wins"], stats["draws"], stats["losses"])
        lr_t, eps_t, beta_t = self.scheduled(lr, eps, beta, schedules, minima)
        tr.advantages()
        bad = set(update_opts) - {"max_grad_norm", "target_kl"}
        if bad:
            raise TypeError("iteration: unknown update options %s" % sorted(bad))
        upd = tr.update(epochs, minibatch, lr_t, eps_t, beta_t, **update_opts)
        n = env.rollout_rows() * env.E * len(env._policy_slots[tr.index])
        saved, swapped = self.advance(n)
        out = dict(stats=stats, update=upd, elo=self.elo, played=played, lr=lr_t, eps=eps_t, beta=beta_t, steps=self.steps, saved=saved,
                   swapped=swapped, opponent=self.opponent, opponent_elo=self.opponent_elo())
        if update_opts:
            out["report"] = tr.last_report
        return out
