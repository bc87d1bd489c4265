"""The recurrent critic of recurrent PPO on the device (include/hk.h "PPO trainer" RECURRENT CRITIC), on test_ppo_lstm_gpu.py's 2-kart
Oval field, rows and staggered resets (R = 11, L = 4, S = 2, max_episode_steps = 100; `_rollout` asserts its preconditions of every rollout
used): the value pass is the inference chain of a recurrent policy built from the critic's weights, bit for bit, whatever the chunking; GAE
is the plain trainer's; at unchanged parameters the training forward reproduces the value pass; the gradients agree with the float64
restatement (ppo_lstm_critic_restate.py) and five mutated restatements do not; the memory is carried from rollout to rollout; an update is
its sequence minibatches issued by hand and resumes through a file; the other trainer kinds are untouched; every refusal holds."""
import ctypes as C

import numpy as np
import pytest

import ppo_restate as PR
import ppo_lstm_critic_restate as CR
import policy_lstm_twin as TW
import test_ppo_lstm_gpu as RT
from test_ppo_lstm_gpu import P, R, L, S, EPS, BETA, LR_, VECTORS, _field, _rollout, _host, _ids
from hierarchicalkarting_amd import _lib, ppo
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.rollout import stacked_inputs, transition_rewards
from parity import assert_bits_equal

pytestmark = pytest.mark.gpu
SHAPES = [(32, 32), (96, 96), (128, 128)]          # (Hc, m_v); the actor is (H, m) = the same pair
ENVS = [1, 5, 70]                                  # 2, 10 and 140 sequences: under one 32-sequence tile, not a multiple of it, several tiles
K = -(-R // L)
# Against the restatement at perturbed parameters, measured on the MI355X over CASES, both trainer configurations below and the fixed seeds; every
# bound is 10 x the largest deviation measured, rounded up (the project's margin).
#   gradients, relative L2 per parameter tensor (actor and critic): 1.045e-5 (per configuration 1.045e-5 and 7.86e-6)
#   L_v, relative: 1.47e-5 (1.47e-5 and 4.5e-6);  MB_VALUE, relative to max(1, |v|): 1.21e-6 (both)
GRAD_TOL = 1.1e-4
LV_TOL = 1.5e-4
VALUE_TOL = 1.3e-5
# The two trainers of the gradient test; each case runs both.  The critic is random, so its values are far from the returns, and the
# configuration decides which rows carry the value loss's deltas RET - V.  With the defaults (gamma 0.99, lambda 0.95) an episode's end
# dominates every row before it: at E = 1 the mean |RET - V_OLD| falls from 0.6 in row 3 (the episode's last) to 0.007 in the rows 8 .. 10,
# whose deltas are all that crosses a live window edge there (window 1 starts with FIRST), so a wrong gradient into the initial memory moves
# the critic's gradients by 0.4 % only; what crosses a FIRST inside a window is well visible (0.014 .. 0.25).  With gamma 0.5, lambda 0 the
# delta is a one-step TD error of the same order in every row (0.05 .. 0.6 at E = 1): every window edge carries its share (0.06 .. 0.17), and
# the rows behind a FIRST weigh less (0.0055 at E = 5, (128, 128)).  A mutation counts as found by a case when it measures 100 x GRAD_TOL away
# under one of the two; measured per case as the larger of the two, the five mutations lie 0.018 .. 10 away against 100 x GRAD_TOL = 0.011.
GRAD_CFGS = (dict(), dict(gamma=0.5, lambd=0.0))
CASES = [(1, (32, 32)), (5, (96, 96)), (70, (128, 128)), (70, (32, 32)), (5, (128, 128))]
# One case in which the actor's (H, m) and the critic's (Hc, m_v) are four different widths: the host runs both cells through one function, and
# a width or an offset of one leg handed to the other passes every case above.  E = 5: 10 sequences, not a multiple of a tile.
DISTINCT = (5, ((96, 32), (64, 128)))
FIGURES = {}               # the largest deviation per checked quantity over the cases run in this process (nothing asserts on it)


def _pairs(shape):
    """a case's shape -> the actor's (H, m) and the critic's (Hc, m_v): one pair serves both, a pair of pairs is told apart"""
    return shape if isinstance(shape[0], tuple) else (shape, shape)


def _note(name, value):
    FIGURES[name] = max(FIGURES.get(name, 0.0), float(value))


def _critic(D, Hc, mv, seed=21):
    return Policy.random(D * 4, Hc, 2, 1, seed=seed, normalize=False, memory_size=2 * mv)


def _trainer(g, Hc, mv, **kw):
    c = _critic(g.obs_dim, Hc, mv)
    return g.ppo_trainer(0, critic=c, sequence_length=L, critic_memory_size=2 * mv, **kw), c


def _twin(pol, critic):
    """a second handle with a recurrent POLICY whose trunk, cell and W_mu / b_mu are the critic's and whose normaliser is the actor's"""
    h2 = TW.rl_env(1, 2, rewards=1)
    tw = Policy(critic.W, critic.b, critic.W_mu, critic.b_mu, critic.log_sigma, critic.W_branch, critic.b_branch, pol.norm_mean, pol.norm_std,
                pol.stack, False, 0, critic.lstm)
    assert h2.attach_policy(tw, [0, 1], P) == 0
    return h2


def _inputs(pol, ro):
    """-> the rows' UN-normalised stacked inputs [R, E S, in] and the bootstrap inputs [E S, in] (the last row's stack with NEXT_OBS pushed)"""
    X = stacked_inputs(ro, [0, 1], pol.stack)
    D = ro["obs"].shape[3]
    boot = np.concatenate([X[-1][:, :, D:], ro["next_obs"][:, [0, 1], :]], axis=2)
    return X.reshape(R, -1, X.shape[-1]), boot.reshape(-1, boot.shape[-1])


def _chain(h2, X, boot, first, done_last, mem_in):
    """hk_policy_forward_mem stepped through the rollout on the host side -> (v [R, E S], v_boot [E S], critic_memory [K, E S, 2 m_v], mem_out)"""
    mem, v, cm = mem_in.copy(), [], []
    for t in range(R):
        if t % L == 0:
            cm.append(mem.copy())
        mem = mem.copy()
        mem[first[t] != 0] = 0.0
        mu, _, mem = h2.policy_forward(0, X[t], mem)
        v.append(mu)
    out = mem.copy()
    out[done_last] = 0.0
    return np.stack(v), h2.policy_forward(0, boot, mem)[0], np.stack(cm), out


def _last_row_adv(ro, v_last, vb, gamma=0.99):
    """ppo_gae_kernel's last row in its own fp32 arithmetic (lambda's term is + 0): delta = rw + gamma nd vb - v"""
    d = np.repeat(ro["done"][R - 1][:, None] != 0, S, axis=1).reshape(-1)
    rw = transition_rewards(ro)[R - 1][:, [0, 1]].reshape(-1).astype(np.float32)
    nd = np.where(d, np.float32(0.0), np.float32(1.0))
    with np.errstate(invalid="ignore"):
        return ((rw + (np.float32(gamma) * nd) * vb).astype(np.float32) - v_last).astype(np.float32) + np.float32(0.0)


def _check_value_pass(tr, chain, ro, tag):
    v, vb, cm, out = chain
    assert_bits_equal(tr.read("v_old").reshape(R, -1), v, (tag, "V_OLD"))
    assert_bits_equal(tr.read("critic_memory").reshape(cm.shape), cm, (tag, "CRITIC_MEMORY"))
    assert_bits_equal(tr.read("critic_mem_out").reshape(out.shape), out, (tag, "MEM_OUT"))
    assert_bits_equal(tr.read("adv").reshape(R, -1)[R - 1], _last_row_adv(ro, v[R - 1], vb), (tag, "the bootstrap value through ADV of the last row"))


# ---- 1. the value pass against the inference chain, exact
@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("shape", SHAPES)
def test_value_pass_is_the_inference_chain(E, shape):
    g, pol = _field(E, *shape)
    ro = _rollout(g, pol)
    hst = _host(g, pol, ro)
    tr, critic = _trainer(g, *shape, normalize_advantages=False)
    h2 = _twin(pol, critic)
    X, boot = _inputs(pol, ro)
    done_last = hst["done"][R - 1]
    mm = critic.memory_size
    assert not tr.read("critic_mem_in").any() and tr.read("critic_mem_in").size == E * S * mm
    tr.advantages()
    _check_value_pass(tr, _chain(h2, X, boot, hst["first"], done_last, np.zeros((E * S, mm), np.float32)), ro, "from zero memory")
    assert not tr.read("critic_mem_in").any()
    # MEM_IN written through hk_ppo_ptr is honoured by a repeated call on the same rollout, and stays as written
    mem_in = np.random.default_rng(E).uniform(-1, 1, (E * S, mm)).astype(np.float32)
    tr.write("critic_mem_in", mem_in)
    tr.advantages()
    ch = _chain(h2, X, boot, hst["first"], done_last, mem_in)
    _check_value_pass(tr, ch, ro, "from a written MEM_IN")
    assert_bits_equal(tr.read("critic_mem_in").reshape(mem_in.shape), mem_in, "MEM_IN after the call")
    assert ch[2][1:].any() and ch[3].any() and not ch[3][done_last].any()
    # window 0 starts from MEM_IN as written, before the FIRST rule
    assert_bits_equal(ch[2][0], mem_in, "CRITIC_MEMORY[0]")


# ---- 2. chunk and tile independence
@pytest.mark.parametrize("E,shape", [(70, (128, 128)), (5, (32, 32)), (70, (96, 96))])
def test_value_pass_does_not_depend_on_the_chunking(E, shape):
    mem_in = np.random.default_rng(2).uniform(-1, 1, E * S * 2 * shape[1]).astype(np.float32)
    got, ro0 = {}, None
    # 3 and 4 put a chunk edge inside a window and on a window edge, 16 covers the R + 1 steps in one launch; 256 and 512 make the sequence tile
    # 64 and 32 (16 384 rows / value_chunk_steps), so E = 70 runs in 3 and 5 tiles with a ragged last one.  A handle takes four trainers, so
    # the seven go on two handles with the same rollout
    for chunks in ((1, 3, 4, 16), (0, 256, 512)):
        g, pol = _field(E, *shape)
        ro = _rollout(g, pol)
        ro0 = ro0 or ro
        for k in ro:
            assert_bits_equal(ro[k], ro0[k], "the two handles' rollouts: %s" % k)
        for chunk in chunks:
            tr, _ = _trainer(g, *shape, value_chunk_steps=chunk)
            tr.advantages()
            tr.write("critic_mem_in", mem_in)
            tr.advantages()
            got[chunk] = {k: tr.read(k) for k in ("v_old", "adv", "ret", "critic_memory", "critic_mem_out")}
            for k, a in got[chunk].items():
                assert_bits_equal(a, got[1][k], "value_chunk_steps %d against 1: %s" % (chunk, k))
    assert got[0]["v_old"].any() and got[0]["critic_mem_out"].any()


# ---- 3. GAE: the plain trainer's rule and tolerance (tests/test_ppo_gpu.py test_critic_and_gae_against_the_restatement)
def test_gae_of_the_recurrent_values():
    E, shape = 5, (96, 96)
    g, pol = _field(E, *shape)
    ro = _rollout(g, pol)
    hst = _host(g, pol, ro)
    X, boot = _inputs(pol, ro)
    r = transition_rewards(ro)[:, :, [0, 1]]
    d = np.repeat(ro["done"][:, :, None], S, axis=2)
    assert (ro["done"] != 0).any()
    for norm in (False, True):
        tr, critic = _trainer(g, *shape, normalize_advantages=norm, gamma=0.99, lambd=0.95)
        tr.advantages()
        v_dev = tr.read("v_old")
        cp = PR.tensors(tr.critic_params())
        T = lambda a: PR.normalise(a, pol.norm_mean, pol.norm_std)
        v_ref, vb, _, _ = CR.value_pass(cp, len(critic.W), T(X), T(boot), hst["first"], hst["done"][R - 1], np.zeros((E * S, critic.memory_size)), L)
        assert np.abs(v_dev - v_ref.reshape(-1)).max() <= 1e-5 * max(1.0, np.abs(v_ref).max())
        A, RET = PR.gae(r, d, v_dev.reshape(R, E, S), vb.reshape(E, S), 0.99, 0.95)
        if norm:
            A = PR.normalise_adv(A)
        for name, ref in (("adv", A), ("ret", RET)):
            dev = tr.read(name).reshape(ref.shape)
            assert np.abs(dev - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), name


# ---- 4. unchanged parameters
def _check_critic_exact(tr, E, mm, hst, sids, tag):
    """after a minibatch at unchanged parameters: MB_VALUE and MB_CRITIC_MEMORY against the value pass, bit for bit -> chained rows checked"""
    rid = RT._rowids(sids, E)
    live = rid >= 0
    ms = len(sids)
    assert_bits_equal(tr.read("mb_value").reshape(L, ms)[live], tr.read("v_old")[rid[live]], (tag, "MB_VALUE"))
    mem = tr.read("mb_critic_memory").reshape(L, ms, mm)
    cm = tr.read("critic_memory").reshape(K, E * S, mm)
    out = tr.read("critic_mem_out").reshape(E * S, mm)
    t, p = rid // (E * S), rid % (E * S)
    chained = 0
    for tau in range(L):
        for q in range(ms):
            if rid[tau, q] < 0:
                continue
            tt, pp = t[tau, q], p[tau, q]
            if tt + 1 < R and (tt + 1) % L == 0:
                assert_bits_equal(mem[tau, q], cm[(tt + 1) // L, pp], (tag, "MB_CRITIC_MEMORY against CRITIC_MEMORY", tt, pp))
                chained += 1
            elif tt == R - 1 and not hst["done"][tt, pp]:
                assert_bits_equal(mem[tau, q], out[pp], (tag, "MB_CRITIC_MEMORY against MEM_OUT", pp))
                chained += 1
    return chained


@pytest.mark.parametrize("shape,E", [pytest.param(s, E, id="shape%d-%d" % (i, E)) for i, s in enumerate(SHAPES) for E in ENVS] +
                         [pytest.param(DISTINCT[1], DISTINCT[0], id="distinct-%d" % DISTINCT[0])])
def test_unchanged_parameters_reproduce_the_value_pass(E, shape):
    actor, crit = _pairs(shape)
    g, pol = _field(E, *actor)
    hst = _host(g, pol, _rollout(g, pol))
    tr, critic = _trainer(g, *crit)
    tr.advantages()
    tr.write("critic_mem_in", np.random.default_rng(7).uniform(-1, 1, E * S * critic.memory_size).astype(np.float32))
    tr.advantages()
    nseq = ppo.sequence_count(R, L, E, S)
    # the actor side of §17 on this trainer: rho == 1, MB_MU / MB_LOGITS / MB_MEMORY are the recorder's
    _, chained = RT._check_exact(tr, g, pol, hst, np.arange(nseq), "in order")
    assert chained > 0
    assert _check_critic_exact(tr, E, critic.memory_size, hst, np.arange(nseq), "in order") >= 2 * E * S
    sids = np.random.default_rng(E).permutation(nseq)
    sids = np.concatenate([sids[:nseq // 2], [nseq + 3], sids[nseq // 2:], [-1]])
    RT._check_exact(tr, g, pol, hst, sids, "shuffled")
    _check_critic_exact(tr, E, critic.memory_size, hst, sids, "shuffled")
    assert tr.read("mb_critic_memory").size == L * sids.size * critic.memory_size
    # at V == V_OLD the value loss is (RET - V)^2 on both sides of the max: its gradient reaches the critic's cell and trunk
    gc = tr.critic_params(tr.read("grad"))
    for k in ("W0", "W_ih", "W_hh", "b_ih", "W_mu", "b_mu"):
        assert gc[k].any(), k
    assert_bits_equal(gc["b_ih"], gc["b_hh"], "GRAD b_ih against b_hh of the critic")


# ---- 5. gradients against the float64 restatement
def _restate(tr, pol, critic, hst, cm, flat, adv, v_old, ret, sids, E, mutate=None):
    ap, cp = PR.tensors(tr.actor_params(flat), True), PR.tensors(tr.critic_params(flat), True)
    Lt, st, hd = CR.loss(ap, cp, len(pol.W), len(critic.W), hst["X"], hst["memory"], cm, hst["first"], hst["f"], adv, v_old, ret,
                         [int(s) for s in sids], R, L, E, S, EPS, BETA, mutate)
    Lt.backward()
    return {k: v.grad.numpy() for k, v in ap.items()}, {k: v.grad.numpy() for k, v in cp.items()}, st, hd


@pytest.mark.parametrize("E,shape", CASES + [DISTINCT])
def test_gradients_against_the_restatement(E, shape):
    """Measured on the MI355X over CASES and GRAD_CFGS (fixed seeds), largest deviation from the restatement: gradients 1.045e-5 relative L2 per
    tensor (bound 1.1e-4), L_v 1.47e-5 relative (bound 1.5e-4), MB_VALUE 1.21e-6 of max(1, |v|) (bound 1.3e-5); the mutated restatements, per
    case the larger of the two configurations: 0.018 .. 10 away (asked: 100 x 1.1e-4 = 0.011)."""
    actor, crit = _pairs(shape)
    g, pol = _field(E, *actor)
    ro = _rollout(g, pol)
    hst = _host(g, pol, ro)
    nseq = ppo.sequence_count(R, L, E, S)
    away = {}          # mutation -> the largest distance measured under either configuration
    bad = []           # every violated bound of the case: one failure names them all
    prints = []
    for ci, cfg in enumerate(GRAD_CFGS):
        tr, critic = _trainer(g, *crit, **cfg)
        tr.advantages()
        tr.write("critic_mem_in", np.random.default_rng(11).uniform(-1, 1, E * S * critic.memory_size).astype(np.float32))
        tr.advantages()
        adv, v_old, ret = tr.read("adv"), tr.read("v_old"), tr.read("ret")
        cm = tr.read("critic_memory").reshape(K, E * S, critic.memory_size).astype(np.float64)
        flat = RT._perturb(tr, 17 + E)
        rng = np.random.default_rng(5)
        for ms in sorted({1, min(33, nseq), nseq}) if ci == 0 else [nseq]:
            sids = rng.permutation(nseq)[:ms]
            if ms == 1:
                sids = np.array([nseq - 1])                   # a last-window sequence: its dead row is a quarter of the rows
            dev = np.concatenate([sids[:ms // 2], [nseq + 7], sids[ms // 2:]])        # one out of range, skipped
            st = tr.minibatch(_ids(dev), EPS, BETA)
            case = "E=%d (Hc, m_v)=%s cfg=%s ms=%d" % (E, shape, cfg, ms)
            n_bad = len(bad)
            if st["skipped"] != 1.0:
                bad.append("%s skipped %r != 1" % (case, st["skipped"]))
            ga, gc, ref, hd = _restate(tr, pol, critic, hst, cm, flat, adv, v_old, ret, dev, E)
            gd = tr.read("grad")
            da, dc = tr.actor_params(gd), tr.critic_params(gd)
            if not np.array_equal(dc["b_ih"].view(np.int32), dc["b_hh"].view(np.int32)):
                bad.append("%s critic GRAD b_ih != GRAD b_hh" % case)
            for name, e in list(RT._deviation(da, ga).items()) + [("critic " + k, e) for k, e in RT._deviation(dc, gc).items()]:
                _note("grad", e)
                if not e <= GRAD_TOL:
                    bad.append("%s GRAD %s relative L2 %.6g > %.3g" % (case, name, e, GRAD_TOL))
            lv = abs(st["L_v"] - ref["L_v"]) / max(abs(ref["L_v"]), 1e-300)
            _note("L_v", lv)
            if not lv <= LV_TOL:
                bad.append("%s stat L_v device %.9g restatement %.9g" % (case, st["L_v"], ref["L_v"]))
            live = hd["rowid"] >= 0
            val = tr.read("mb_value").reshape(L, dev.size)
            vd = np.abs(val[live] - hd["v"][live]).max() / max(1.0, np.abs(hd["v"][live]).max())
            _note("mb_value", vd)
            if not vd <= VALUE_TOL:
                bad.append("%s MB_VALUE deviation %.6g > %.3g" % (case, vd, VALUE_TOL))
            if ms == nseq:          # the five mutated restatements on the full minibatch
                for mut in CR.MUTATIONS:
                    ma, mc_, _, _ = _restate(tr, pol, critic, hst, cm, flat, adv, v_old, ret, dev, E, mut)
                    d = max(list(RT._deviation(da, ma).values()) + list(RT._deviation(dc, mc_).values()))
                    away[mut] = max(away.get(mut, 0.0), d)
                    prints.append("%s mutation %s %.6g away" % (case, mut, d))
            prints.append("%s so far: grad %.4g L_v %.4g mb_value %.4g" % (case, FIGURES["grad"], FIGURES["L_v"], FIGURES["mb_value"]))
            if len(bad) > n_bad:
                # what tells a device that differs from run to run from inputs that differ: fingerprints, and the same minibatch issued once more
                tr.minibatch(_ids(dev), EPS, BETA, stats=False)
                again = tr.read("grad")
                bad.append("fingerprints (%s): rollout obs %s first %s memory %s | adv %s v_old %s critic_memory %s | PARAMS on device %s, as perturbed %s | "
                           "ids %s | GRAD %s, the same minibatch again %s (%s)"
                           % (case, RT._sha(ro["obs"]), RT._sha(ro["first"]), RT._sha(ro["memory"]), RT._sha(adv), RT._sha(v_old), RT._sha(cm),
                              RT._sha(tr.read("params")), RT._sha(flat), RT._sha(np.asarray(dev, np.int32)), RT._sha(gd), RT._sha(again),
                              "same bits" if np.array_equal(gd.view(np.int32), again.view(np.int32)) else "DIFFERENT bits"))
    print("\n".join(prints))
    # each mutation at least 100 x the bound away in some tensor, under one of the two configurations.  With E = 1 the rollout has no FIRST
    # strictly inside a window, so the two mutations that act only there do not count (§17)
    inert = ("critic_grad_through_first", "critic_whh_grad_pre_reset") if E < 4 else ()
    for mut in CR.MUTATIONS:
        if mut not in inert and not away[mut] >= 100 * GRAD_TOL:
            bad.append("E=%d (Hc, m_v)=%s mutation %s only %.6g away" % (E, shape, mut, away[mut]))
    if bad:
        raise AssertionError("\n".join(bad))


# ---- 6. the memory carried from rollout to rollout
def test_critic_memory_is_carried_between_rollouts():
    E, shape = 5, (96, 96)
    g, pol = _field(E, *shape)
    tr, critic = _trainer(g, *shape, normalize_advantages=False)
    h2 = _twin(pol, critic)
    mm = critic.memory_size
    _rollout(g, pol)
    tr.advantages()
    out1 = tr.read("critic_mem_out").reshape(E * S, mm)
    assert out1.any()
    ro = _rollout(g, pol, again=True)
    hst = _host(g, pol, ro)
    X, boot = _inputs(pol, ro)
    tr.advantages()
    _check_value_pass(tr, _chain(h2, X, boot, hst["first"], hst["done"][R - 1], out1), ro, "the second rollout from the first's MEM_OUT")
    assert_bits_equal(tr.read("critic_mem_in").reshape(out1.shape), out1, "MEM_IN := MEM_OUT of the previous call")
    was = {k: tr.read(k) for k in ("v_old", "adv", "ret", "critic_memory", "critic_mem_in", "critic_mem_out")}
    tr.advantages()
    for k, a in was.items():
        assert_bits_equal(tr.read(k), a, "a repeated call on the same rollout: %s" % k)
    tr.reset_critic_memory()
    assert not tr.read("critic_mem_in").any() and not tr.read("critic_mem_out").any()
    tr.advantages()
    _check_value_pass(tr, _chain(h2, X, boot, hst["first"], hst["done"][R - 1], np.zeros_like(out1)), ro, "after reset_critic_memory")
    assert not np.array_equal(was["v_old"], tr.read("v_old"))


# ---- 7. update
@pytest.mark.parametrize("E,shape,mb", [(5, (96, 96), 7), (70, (128, 128), 65)])
def test_update_is_its_sequence_minibatches_issued_by_hand(E, shape, mb):
    g, pol = _field(E, *shape)
    _rollout(g, pol)
    nseq = ppo.sequence_count(R, L, E, S)
    t1, t2, t3 = (_trainer(g, *shape, seed=7)[0] for _ in range(3))
    for t in (t1, t2, t3):
        t.advantages()
    s1 = t1.update(2, mb, LR_, EPS, BETA)
    s3 = t3.update(2, mb, LR_, EPS, BETA)
    assert s1 == s3
    for ep in range(2):
        pm = ppo.permutation(nseq, 7, ep)
        for b in range(nseq // mb):
            t2.minibatch(_ids(pm[b * mb:(b + 1) * mb]), EPS, BETA, stats=False)
            t2.adam(LR_)
    for k in VECTORS:
        assert_bits_equal(t1.read(k), t2.read(k), "update against its minibatches by hand: %s" % k)
        assert_bits_equal(t1.read(k), t3.read(k), "two identical updates: %s" % k)
    assert t1.counters() == (2 * (nseq // mb), 2)
    c0, c1 = _critic(g.obs_dim, *shape), t1.critic_params()
    assert not np.array_equal(c1["W_hh"], c0.lstm["W_hh"]) and not np.array_equal(c1["W_mu"], c0.W_mu) and not np.array_equal(c1["W0"], c0.W[0])
    ids = _ids(ppo.permutation(nseq, 3, 0)[:mb])
    t1.minibatch(ids, EPS, BETA, stats=False)
    a = t1.read("grad")
    t1.minibatch(ids, EPS, BETA, stats=False)
    assert_bits_equal(a, t1.read("grad"), "GRAD of the same minibatch twice")


def test_clip_and_kl_stop():
    E, shape = 5, (96, 96)
    g, pol = _field(E, *shape)
    _rollout(g, pol)
    nseq = ppo.sequence_count(R, L, E, S)
    tr, _ = _trainer(g, *shape, seed=1)
    tr.advantages()
    RT._perturb(tr, 3)
    tr.minibatch(_ids(np.arange(nseq)), EPS, BETA, stats=False)
    grad = tr.read("grad")
    norm = ppo.grad_norm(grad)
    cell = tr.critic_params(grad)
    without = ppo.grad_norm(np.concatenate([grad[:tr.n_actor]] + [v.reshape(-1) for k, v in cell.items() if k not in Policy.LSTM_KEYS]))
    assert without < norm * (1 - 1e-9)                       # the critic cell's gradients are part of the one norm
    tr.adam(LR_, max_grad_norm=0.5 * norm)
    w = tr.clip_words()
    assert abs(w["norm"] - norm) <= 1e-12 * norm and np.float32(w["coef"]) == ppo.clip_coefficient(w["norm"], 0.5 * norm)
    tr.advantages()
    tr.update(3, 10, 3e-3, EPS, BETA, max_grad_norm=0.5, target_kl=1e-12)
    rep = tr.last_report
    assert rep["epochs_run"] == 1 and rep["stopped_by_kl"] == 1 and rep["minibatches_run"] == nseq // 10 and rep["last_epoch_kl"] > 1e-12
    assert rep["grad_norm_max"] > 0 and rep["nonfinite_steps"] == 0


def test_resume_through_a_file_on_a_fresh_handle(tmp_path):
    E, shape, mb = 5, (96, 96), 6
    ga, pol = _field(E, *shape)
    ra = _rollout(ga, pol)
    a, _ = _trainer(ga, *shape, seed=5)
    a.advantages()
    a.update(2, mb, LR_, EPS, BETA)
    path = str(tmp_path / "recurrent_critic.ckpt")
    a.save(path)
    sd = a.state_dict()
    assert sd["critic_shape"].tolist() == [216, 96, 2, 0, 192] and sd["critic_mem_out"].any() and not sd["critic_mem_in"].any()
    ra2 = _rollout(ga, a.actor(), again=True)               # recorded with the published actor; the value pass starts from MEM_OUT
    a.advantages()
    a.update(2, mb, LR_, EPS, BETA)
    gb, _ = _field(E, *shape)
    rb = _rollout(gb, pol)
    for k in ra:
        assert_bits_equal(ra[k], rb[k], "the two handles' first rollouts: %s" % k)
    b, _ = _trainer(gb, *shape, seed=5)
    b.load(path)
    assert b.counters() == (2 * (30 // mb), 2)
    rb2 = _rollout(gb, b.actor(), again=True)
    for k in ra2:
        assert_bits_equal(ra2[k], rb2[k], "the two handles' second rollouts: %s" % k)
    b.advantages()
    assert_bits_equal(b.read("critic_mem_in"), sd["critic_mem_out"], "the resumed value pass starts from the saved MEM_OUT")
    b.update(2, mb, LR_, EPS, BETA)
    for k in VECTORS + ("v_old", "critic_mem_in", "critic_mem_out"):
        assert_bits_equal(a.read(k), b.read(k), "resumed: %s" % k)
    # another critic memory size, or a feed-forward critic's trainer, refuses the state by name before anything is written
    c = gb.ppo_trainer(0, sequence_length=L, seed=5)
    was = {k: c.read(k) for k in VECTORS}
    with pytest.raises(ValueError, match="critic_shape"):
        c.load_state_dict(sd)
    for k in VECTORS:
        assert_bits_equal(was[k], c.read(k), "a refused load: %s" % k)


# ---- 8. side by side with the other kinds
def _three(with_third):
    RT._torch()
    g = TW.rl_env(5, 2, rewards=1, max_episode_steps=100, jitter_seed=9)
    D = g.obs_dim
    rec, plain = RT._actor(D, 96, 96), Policy.random(D * 4, 64, 2, 3, seed=8)
    assert g.attach_policy(rec, [1], P) == 0 and g.attach_policy(plain, [0], P) == 1
    g.rollout_begin(R); g.step(R * P); g.rollout_close()
    tp, tr = g.ppo_trainer(1), g.ppo_trainer(0, sequence_length=L)
    tc = None
    if with_third:
        tc = g.ppo_trainer(0, critic=_critic(D, 96, 64), sequence_length=L, critic_memory_size=128)
        assert (tp.t, tr.t, tc.t) == (0, 1, 2)
    for t in (tc, tp, tr):
        if t is not None:
            t.advantages()
    if tc is not None:
        st = tc.minibatch(_ids(np.arange(3 * 5)), EPS, BETA)
        assert st["approx_kl"] == 0.0 and st["skipped"] == 0.0
        tc.update(1, 4, LR_, EPS, BETA)
        tc.advantages()
    tp.minibatch(_ids(np.arange(R * 5)), EPS, BETA, stats=False)
    tr.minibatch(_ids(np.arange(3 * 5)), EPS, BETA, stats=False)
    return g, tp, tr, tc


def test_side_by_side_with_a_plain_and_a_recurrent_trainer():
    g, tp, tr, tc = _three(True)
    got = {(n, k): t.read(k) for n, t in (("plain", tp), ("recurrent", tr)) for k in ("grad", "v_old", "adv", "ret", "params")}
    for t in (tp, tr):          # the new fields on other trainer kinds: no elements, and hk_ppo_ptr refuses
        for name, f in _lib.PPO_RECURRENT_CRITIC_FIELDS.items():
            assert g.L.hk_ppo_count(g.h, t.t, f) == 0, name
            assert not g.L.hk_ppo_ptr(g.h, t.t, f) and "recurrent critic" in g.L.hk_last_error(g.h).decode(), name
        assert set(t.views()) & set(_lib.PPO_RECURRENT_CRITIC_FIELDS) == set()
    assert set(_lib.PPO_RECURRENT_CRITIC_FIELDS) <= set(tc.views())
    assert tc.read("mb_critic_memory").size == 0 or tc.read("mb_critic_memory").size % 128 == 0
    del g, tp, tr, tc
    g2, tp2, tr2, _ = _three(False)
    for (n, k), a in got.items():
        assert_bits_equal(a, (tp2 if n == "plain" else tr2).read(k), "%s trainer beside a recurrent-critic trainer: %s" % (n, k))


# ---- 9. refusals
def test_refusals():
    g, pol = _field(5, 32, 32)
    D = g.obs_dim
    h2 = TW.rl_env(2, 2, rewards=1)
    assert h2.attach_policy(Policy.random(D * 4, 64, 2, 3, seed=8), [0, 1], P) == 0
    critic = _critic(D, 32, 32)
    d, _keep = critic.desc()
    d.n_branch = 0
    d.W_branch = d.b_branch = None
    pc = _lib.PpoConfig(0.99, 0.95, 1, 0.9, 0.999, 1e-8, 0)
    rd = lambda Ls=4, chunk=0, r0=0, r1=0: C.byref(_lib.PpoRecurrentCriticDesc(Ls, chunk, (C.c_int32 * 2)(r0, r1)))

    def cell(**kw):
        c = critic.lstm_desc()
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    def refused(env, code, word, *args):
        rc = env.L.hk_ppo_create_recurrent_critic(env.h, *args)
        assert rc == code, (word, rc)
        assert word in env.L.hk_last_error(env.h).decode(), (word, env.L.hk_last_error(env.h))
    I = _lib.HK_ERR_INVALID
    refused(g, I, "NULL r", 0, C.byref(d), cell(), C.byref(pc), None)
    refused(g, I, "NULL critic_cell", 0, C.byref(d), None, C.byref(pc), rd())
    refused(g, I, "sequence_length", 0, C.byref(d), cell(), C.byref(pc), rd(0))
    refused(g, I, "value_chunk_steps", 0, C.byref(d), cell(), C.byref(pc), rd(4, -1))
    refused(g, I, "reserved", 0, C.byref(d), cell(), C.byref(pc), rd(4, 0, 1))
    refused(g, I, "reserved", 0, C.byref(d), cell(), C.byref(pc), rd(4, 0, 0, 1))
    refused(g, I, "critic_cell: reserved", 0, C.byref(d), cell(reserved=1), C.byref(pc), rd())
    refused(g, I, "memory_size is odd", 0, C.byref(d), cell(memory_size=65), C.byref(pc), rd())
    for ms in (0, 32, 96, 320):          # m_v = 0, 16, 48, 160
        refused(g, I, "multiple of 32 in [32, 128]", 0, C.byref(d), cell(memory_size=ms), C.byref(pc), rd())
    for k in Policy.LSTM_KEYS:
        refused(g, I, "critic_cell: NULL", 0, C.byref(d), cell(**{k: None}), C.byref(pc), rd())
    refused(h2, I, "without memory", 0, C.byref(d), cell(), C.byref(pc), rd())
    refused(g, I, "policy", 3, C.byref(d), cell(), C.byref(pc), rd())                   # whatever hk_ppo_create_recurrent refuses ...
    refused(g, I, "critic", 0, None, cell(), C.byref(pc), rd())
    refused(g, I, "Adam", 0, C.byref(d), cell(), C.byref(_lib.PpoConfig(0.99, 0.95, 1, 1.5, 0.999, 1e-8, 0)), rd())
    d.in_dim += 1
    refused(g, I, "in_dim", 0, C.byref(d), cell(), C.byref(pc), rd())
    d.in_dim -= 1
    w_mu = d.W_mu
    d.W_mu = None
    refused(g, I, "value head", 0, C.byref(d), cell(), C.byref(pc), rd())
    d.W_mu = w_mu
    assert g.L.hk_ppo_count(g.h, 0, 0) == I                                             # nothing was created
    with pytest.raises(ValueError, match="sequence_length"):
        g.ppo_trainer(0, critic_memory_size=64)
    with pytest.raises(ValueError, match="memory_size"):
        g.ppo_trainer(0, critic=_critic(D, 32, 64), sequence_length=L, critic_memory_size=64)
    tr, _ = _trainer(g, 32, 32)
    assert tr.t == 0
    with pytest.raises(_lib.HkError) as e:
        tr.set_precision("bf16")
    assert e.value.code == _lib.HK_ERR_UNSUPPORTED and "precision" in str(e.value)
    assert tr.precision == "f32"
    assert g.L.hk_ppo_count(g.h, tr.t, _lib.PPO_RECURRENT_CRITIC_FIELDS["critic_memory"]) == 0          # before hk_ppo_advantages
    assert not g.L.hk_ppo_ptr(g.h, tr.t, _lib.PPO_RECURRENT_CRITIC_FIELDS["critic_memory"])
    with pytest.raises(_lib.HkError):
        tr.read("mb_critic_memory")                                                                     # no minibatch yet
    assert g.L.hk_ppo_count(g.h, tr.t, 37) == I and not g.L.hk_ppo_ptr(g.h, tr.t, 37)
    _rollout(g, pol)
    tr.advantages()
    assert tr.minibatch(_ids([0, 1]), EPS, BETA)["skipped"] == 0.0
    assert tr.read("critic_memory").size == K * 5 * S * 64 and tr.read("mb_critic_memory").size == L * 2 * 64
