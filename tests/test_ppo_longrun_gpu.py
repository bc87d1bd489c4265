"""PPO trainer for long runs on the device (include/hk.h "LONG RUNS"): the global gradient norm and the clip coefficient against
their host twins, the clip-aware step against the float32 Adam restatement, measure-only against the plain update, a clipped update against
its steps issued by hand, the KL stop against single-epoch updates, a non-finite gradient, exact resume through a checkpoint file, and every
refusal.  The base shape of test_ppo_gpu.py: 24 envs x 4 agents, 90 rows, n = 4320; team 0 is 312 -> 256 x 3, team 1 128 x 2."""
import ctypes as C
import math

import numpy as np
import pytest

import ppo_restate as PR
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.ppo import bf16_round, clip_coefficient, grad_norm, permutation
from parity import assert_bits_equal
from test_ppo_gpu import P as PERIOD, _env, _ids, _torch

pytestmark = pytest.mark.gpu
EPS, BETA, LR, MB = 0.2, 5e-3, 3e-4, 512
VECTORS = ("params", "adam_m", "adam_v")


def _state(tr):
    return {k: tr.read(k) for k in VECTORS}


def _same(a, b, what):
    for k in a:
        assert_bits_equal(a[k], b[k], "%s: %s" % (what, k))


def _f32_bits(x):
    return np.float32(x).view(np.uint32)


# ---- 1. norm and coefficient
@pytest.mark.parametrize("p", [0, 1])
def test_norm_and_coefficient_against_the_host_twins(p):
    torch = _torch()
    g, _ = _env()
    tr = g.ppo_trainer(p)
    tr.advantages()
    n = tr.read("adv").size
    Pn = tr.read("params").size
    assert Pn % 4096 != 0 and Pn % 4 != 0 and Pn > 4096          # a tail run, a GRAD base off 16 bytes, more than one workgroup
    assert tr.clip_words() == dict.fromkeys(_lib.PPO_CLIP_NAMES, 0.0) and g.L.hk_ppo_count(g.h, tr.t, _lib.PPO_FIELDS["clip"]) == 0
    steps = 0
    for m in (65, n):
        tr.minibatch(_ids(torch, np.arange(m)), EPS, BETA)
        grad = tr.read("grad")
        ref = grad_norm(grad)
        assert np.isfinite(ref) and ref > 0
        half = None
        for c in (math.inf, "half", 1e-3):
            c = half if c == "half" else c
            tr.adam(LR, max_grad_norm=c)
            steps += 1
            w = tr.clip_words()
            err = abs(w["norm"] - ref) / ref
            print("policy %d, %d rows, bound %g: norm %.17g against %.17g (relative %.3g, bound %.3g), coef %.9g" % (p, m, c, w["norm"], ref, err, Pn * 2.0 ** -53, w["coef"]))
            assert err <= Pn * 2.0 ** -53
            assert _f32_bits(w["coef"]) == _f32_bits(clip_coefficient(w["norm"], c)) and float(np.float32(w["coef"])) == w["coef"]
            assert (w["coef"] == 1.0) == (c == math.inf)
            assert_bits_equal(tr.read("grad"), grad, "GRAD after a clip-aware step")
            assert w["steps"] == steps and w["nonfinite"] == 0 and w["reserved"] == 0
            half = 0.5 * w["norm"]
    w = tr.clip_words()
    assert w["clipped"] == 4 and w["norm_max"] >= w["norm_sum"] / steps > 0
    assert tr.counters() == (steps, 0)


# ---- 2. the step's bits
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_clipped_step_is_the_adam_restatement_on_the_scaled_gradient(prec):
    torch = _torch()
    g, _ = _env()
    tr = g.ppo_trainer(0, precision=prec, seed=3)
    tr.advantages()
    n = tr.read("adv").size
    tr.minibatch(_ids(torch, permutation(n, 3, 0)[:MB]), EPS, BETA)
    tr.adam(LR, max_grad_norm=math.inf)
    bound = 0.5 * tr.clip_words()["norm"]
    for c in (bound, 1e-3):
        before, grad = _state(tr), tr.read("grad")
        step = tr.counters()[0] + 1
        tr.adam(LR, max_grad_norm=c)
        coef = np.float32(tr.clip_words()["coef"])
        assert coef < 1.0
        scaled = grad * coef
        assert scaled.dtype == np.float32
        p1, m1, v1 = PR.adam_f32(before["params"], scaled, before["adam_m"], before["adam_v"], step, LR)
        _same(dict(params=p1, adam_m=m1, adam_v=v1), _state(tr), "clip-aware step, bound %g, %s" % (c, prec))
        assert not np.array_equal(p1, before["params"])
        if prec == "bf16":
            assert np.array_equal(tr.shadow(), bf16_round(tr.read("params")))


# ---- 3. measure-only is the plain path
def test_measure_only_update_is_the_plain_update():
    g, _ = _env()
    t1, t2 = g.ppo_trainer(0, seed=13), g.ppo_trainer(0, seed=13)
    for t in (t1, t2):
        t.advantages()
    s1 = t1.update(2, MB, LR, EPS, BETA)
    assert t1.last_report is None
    s2 = t2.update(2, MB, LR, EPS, BETA, max_grad_norm=math.inf)
    _same(_state(t1), _state(t2), "max_grad_norm = inf against the plain update")
    assert np.array_equal(t1.read("perm"), t2.read("perm"))
    assert s1 == s2
    r = t2.last_report
    print("measure-only report:", r)
    assert (r["epochs_run"], r["minibatches_run"], r["stopped_by_kl"], r["clipped_steps"], r["nonfinite_steps"]) == (2, 16, 0, 0, 0)
    assert r["grad_norm_max"] >= r["grad_norm_mean"] > 0
    assert r["last_epoch_kl"] != 0 and np.float32(r["last_epoch_kl"]) == np.float32(s2["approx_kl"])
    assert t2.clip_words()["steps"] == 16 and t1.counters() == t2.counters() == (16, 2)
    # an update with the options given as 0 is the plain one as well, and zeroes the accumulating words at its entry
    t1.update(1, MB, LR, EPS, BETA)
    t2.update(1, MB, LR, EPS, BETA, max_grad_norm=0.0, target_kl=0.0)
    _same(_state(t1), _state(t2), "options 0 against the plain update")
    assert t2.last_report["grad_norm_max"] == 0.0 and t2.last_report["minibatches_run"] == 8 and t2.clip_words()["steps"] == 0


# ---- 4. a clipped update is its steps by hand
def test_clipped_update_is_its_steps_issued_by_hand():
    torch = _torch()
    g, _ = _env()
    seed = 13
    t0, t1, t2 = (g.ppo_trainer(0, seed=seed) for _ in range(3))
    for t in (t0, t1, t2):
        t.advantages()
    n = t1.read("adv").size
    nmb = n // MB
    t0.minibatch(_ids(torch, permutation(n, seed, 0)[:MB]), EPS, BETA)
    t0.adam(LR, max_grad_norm=math.inf)
    c = 0.5 * t0.clip_words()["norm"]
    s1 = t1.update(2, MB, LR, EPS, BETA, max_grad_norm=c)
    norms, coefs = [], []
    for k in (0, 1):
        perm = permutation(n, seed, k)
        for b in range(nmb):
            t2.minibatch(_ids(torch, perm[MB * b: MB * (b + 1)]), EPS, BETA, stats=False)
            t2.adam(LR, c)
            w = t2.clip_words()
            norms.append(w["norm"])
            coefs.append(w["coef"])
    t2.publish()
    _same(_state(t1), _state(t2), "clipped update against its steps by hand")
    r = t1.last_report
    clipped = sum(1 for x in coefs if x < 1.0)
    print("clipped update: bound %.9g, norms %s, report %s" % (c, ["%.6g" % x for x in norms], r))
    assert r["clipped_steps"] == clipped >= 1 and r["nonfinite_steps"] == 0 and r["minibatches_run"] == 2 * nmb == len(norms)
    assert r["grad_norm_max"] == max(norms)
    mean = 0.0
    for x in norms:
        mean += x
    mean /= len(norms)
    assert abs(r["grad_norm_mean"] - mean) <= np.spacing(mean)
    assert np.isfinite(list(s1.values())).all()


# ---- 5. KL stop
def test_kl_stop_against_single_epoch_updates():
    g, _ = _env()
    seed, lr = 21, 3e-3
    tc, ta, tb = (g.ppo_trainer(0, seed=seed) for _ in range(3))
    for t in (tc, ta, tb):
        t.advantages()
    n = tc.read("adv").size
    kl, after = [], []
    for _ in range(3):
        kl.append(float(tc.update(1, MB, lr, EPS, BETA)["approx_kl"]))
        after.append(_state(tc))
    k0, k1, k2 = kl
    print("KL stop: lr %g, the three epochs' mean approx-KL %.9g %.9g %.9g" % (lr, k0, k1, k2))
    target = 0.5 * (k0 + k1)
    assert k0 < k1 and target > 0, "the premise of the test: the first two epochs' approx-KL at lr = %g are %.9g, %.9g (need k0 < k1, mean > 0)" % (lr, k0, k1)
    sa = ta.update(3, MB, lr, EPS, BETA, target_kl=target)
    ra = ta.last_report
    assert (ra["epochs_run"], ra["stopped_by_kl"], ra["minibatches_run"]) == (2, 1, 2 * (n // MB)), ra
    assert np.array_equal(ta.read("perm"), permutation(n, seed, 1)) and ta.counters()[1] == 2
    _same(after[1], _state(ta), "stopped after two epochs against the control's second call")
    assert np.float32(sa["approx_kl"]) == np.float32(k1) and np.float32(ra["last_epoch_kl"]) == np.float32(k1)
    assert ra["grad_norm_max"] == 0.0 and ra["clipped_steps"] == 0
    # a target above every epoch's KL: all three epochs, the control after its third call
    tb.update(3, MB, lr, EPS, BETA, target_kl=2.0 * max(kl) + 1.0)
    rb = tb.last_report
    assert (rb["epochs_run"], rb["stopped_by_kl"]) == (3, 0) and tb.counters()[1] == 3
    assert np.array_equal(tb.read("perm"), permutation(n, seed, 2))
    _same(after[2], _state(tb), "not stopped against the control's third call")
    assert np.float32(rb["last_epoch_kl"]) == np.float32(k2)


# ---- 6. a non-finite gradient
@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_non_finite_gradient_writes_nothing(bad):
    torch = _torch()
    g, _ = _env()
    tr = g.ppo_trainer(0)
    tr.advantages()
    tr.minibatch(_ids(torch, np.arange(65)), EPS, BETA)
    tr.adam(LR, max_grad_norm=1.0)
    before, steps = _state(tr), tr.counters()[0]          # (read() has synchronised the handle's stream: GRAD is at rest)
    grad = tr.views()["grad"]
    at = grad.numel() - 3
    good = float(grad[at])
    grad[at] = bad
    torch.cuda.synchronize()
    tr.adam(LR, max_grad_norm=1.0)
    _same(before, _state(tr), "a step on a gradient with %r" % bad)
    w = tr.clip_words()
    assert w["nonfinite"] == 1 and w["steps"] == 2 and not np.isfinite(w["norm"]) and w["coef"] == 0.0
    assert tr.counters()[0] == steps + 1
    # the moments are not poisoned: with the element put back the next step is an ordinary one
    grad[at] = good
    torch.cuda.synchronize()
    tr.adam(LR, max_grad_norm=1.0)
    now = _state(tr)
    assert all(np.isfinite(now[k]).all() for k in now) and not np.array_equal(now["params"], before["params"])
    assert tr.clip_words()["nonfinite"] == 1 and tr.clip_words()["steps"] == 3


# ---- 7. resume
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_resume_through_a_file_continues_bit_for_bit(prec, tmp_path):
    torch = _torch()
    seed = 5
    ga, pols = _env()
    a = ga.ppo_trainer(0, seed=seed, precision=prec)
    a.normalizer_init()
    a.advantages()
    a.update(2, MB, LR, EPS, BETA)
    a.normalizer_update()
    path = str(tmp_path / "trainer.ckpt")
    a.save(path)
    sd = a.state_dict()
    assert sd["adam_steps"] == 16 and sd["epochs_done"] == 2 and sd["precision"] == prec and sd["normalizer"]["steps"] == 1 + 4320
    a.advantages()
    a.update(2, MB, LR, EPS, BETA)
    # B: a fresh handle whose recorded rollout is A's, bit for bit
    gb, _ = _env()
    ra, rb = ga.rollout(), gb.rollout()
    for k in ra:
        assert_bits_equal(ra[k], rb[k], "the two handles' rollouts: %s" % k)
    b = gb.ppo_trainer(0, seed=seed)
    b.load(path)
    assert b.precision == prec and b.counters() == (16, 2)
    for k in ("norm_mean", "norm_std"):
        assert_bits_equal(b.read(k), sd_pub(sd)[k], "published %s after load" % k)
    b.advantages()
    b.update(2, MB, LR, EPS, BETA)
    _same(_state(a), _state(b), "resumed (%s)" % prec)
    assert np.array_equal(a.read("perm"), b.read("perm")) and a.counters() == b.counters() == (32, 4)
    for k in ("norm_mean", "norm_std"):
        assert_bits_equal(a.read(k), b.read(k), "published %s" % k)
    x = np.random.default_rng(3).standard_normal((300, pols[0][0].in_dim)).astype(np.float32) * 2
    for got, want, name in zip(gb.policy_forward(0, x), ga.policy_forward(0, x), ("mu", "logits")):
        assert_bits_equal(got, want, "policy_forward %s of the resumed handle" % name)
    # control: the three vectors (and the normaliser) without the two counters is NOT a resume
    gc, _ = _env()
    c = gc.ppo_trainer(0, seed=seed, precision=prec)
    gc.synchronize()
    views = c.views()
    for k in VECTORS:
        views[k].copy_(torch.from_numpy(sd[k]))
    torch.cuda.synchronize()
    c.normalizer_load(sd["normalizer"]["steps"], sd["normalizer"]["mean"], sd["normalizer"]["m2"])
    c.publish()
    c.advantages()
    c.update(2, MB, LR, EPS, BETA)
    assert not np.array_equal(c.read("params"), a.read("params")) and not np.array_equal(c.read("perm"), a.read("perm"))
    # a state of another shuffle seed or another shape is refused by name, before anything is written
    d = gc.ppo_trainer(0, seed=seed + 1)
    was = _state(d)
    with pytest.raises(ValueError, match="seed"):
        d.load_state_dict(sd)
    with pytest.raises(ValueError, match="actor_shape"):
        gc.ppo_trainer(1, seed=seed).load_state_dict(sd)
    with pytest.raises(ValueError, match="adam_v"):
        c.load_state_dict({k: v for k, v in sd.items() if k != "adam_v"})
    _same(was, _state(d), "a refused load")


def sd_pub(sd):
    from hierarchicalkarting_amd.ppo import normalizer_published
    nm = sd["normalizer"]
    mean, std = normalizer_published(nm["steps"], nm["mean"], nm["m2"])
    return dict(norm_mean=mean, norm_std=std)


# ---- 8. refusals
def test_refusals_leave_the_state_as_it_was():
    torch = _torch()
    g, _ = _env()
    L, h = g.L, g.h
    tr = g.ppo_trainer(0)
    tr.advantages()
    tr.minibatch(_ids(torch, np.arange(65)), EPS, BETA)
    tr.adam(LR, max_grad_norm=1.0)
    fresh = g.ppo_trainer(1)                      # no advantages yet
    before, counters, words = _state(tr), tr.counters(), tr.clip_words()

    def opts(**kw):
        d = dict(epochs=1, minibatch=MB, lr=LR, eps=EPS, beta=BETA, max_grad_norm=0.0, target_kl=0.0, reserved=0)
        d.update(kw)
        return C.byref(_lib.PpoUpdateOpts(*[d[n] for n, _ in _lib.PpoUpdateOpts._fields_]))
    rep = _lib.PpoUpdateReport()
    big = 2 ** 31
    cases = [
        (lambda: L.hk_ppo_update_opt(h, tr.t, None, None, None), "NULL opts"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(epochs=0), None, C.byref(rep)), "epochs"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(minibatch=0), None, None), "minibatch"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(max_grad_norm=-1.0), None, None), "max_grad_norm"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(max_grad_norm=math.nan), None, None), "max_grad_norm"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(target_kl=-1e-3), None, None), "target_kl"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(target_kl=math.nan), None, None), "target_kl"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(target_kl=math.inf), None, None), "target_kl"),
        (lambda: L.hk_ppo_update_opt(h, tr.t, opts(reserved=1), None, None), "reserved"),
        (lambda: L.hk_ppo_update_opt(h, 9, opts(), None, None), "trainer"),
        (lambda: L.hk_ppo_update_opt(h, fresh.t, opts(), None, None), "hk_ppo_advantages"),
        (lambda: L.hk_ppo_adam_clipped(h, tr.t, LR, 0.0), "max_grad_norm"),
        (lambda: L.hk_ppo_adam_clipped(h, tr.t, LR, -2.0), "max_grad_norm"),
        (lambda: L.hk_ppo_adam_clipped(h, tr.t, LR, math.nan), "max_grad_norm"),
        (lambda: L.hk_ppo_adam_clipped(h, -1, LR, 1.0), "trainer"),
        (lambda: L.hk_ppo_set_counters(h, tr.t, -1, 0), "adam_steps"),
        (lambda: L.hk_ppo_set_counters(h, tr.t, big, 0), "adam_steps"),
        (lambda: L.hk_ppo_set_counters(h, tr.t, 0, -1), "epochs_done"),
        (lambda: L.hk_ppo_set_counters(h, tr.t, 0, big), "epochs_done"),
        (lambda: L.hk_ppo_set_counters(h, 4, 0, 0), "trainer"),
        (lambda: L.hk_ppo_get_counters(h, 4, None, None), "trainer"),
    ]
    for call, word in cases:
        assert call() == _lib.HK_ERR_INVALID, word
        msg = L.hk_last_error(h).decode()
        assert word in msg, (word, msg)
    assert tr.counters() == counters and tr.clip_words() == words
    _same(before, _state(tr), "after the refusals")
    # the largest counters are taken, and read back
    assert L.hk_ppo_set_counters(h, tr.t, big - 1, big - 1) == 0 and tr.counters() == (big - 1, big - 1)
    tr.set_counters(*counters)
    # ppo.py validates what it can first (ValueError); the rest arrives through _ck as a RuntimeError
    for call in (lambda: tr.update(1, MB, LR, EPS, BETA, max_grad_norm=-1.0), lambda: tr.update(1, MB, LR, EPS, BETA, target_kl=math.nan),
                 lambda: tr.update(1, MB, LR, EPS, BETA, target_kl=math.inf), lambda: tr.adam(LR, 0.0), lambda: tr.adam(LR, math.nan)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        tr.update(1, MB, LR, EPS, BETA, 1.0)           # the options are keyword-only
    with pytest.raises(RuntimeError, match="adam_steps"):
        tr.set_counters(-1, 0)
    with pytest.raises(RuntimeError, match="hk_ppo_advantages"):
        fresh.update(1, MB, LR, EPS, BETA, max_grad_norm=1.0)
    # while a rollout is open: set_counters, and with it load_state_dict, is refused before anything is written
    sd = tr.state_dict()
    sd["params"] = sd["params"] + np.float32(1.0)
    g.rollout_begin(2)
    assert L.hk_ppo_set_counters(h, tr.t, 1, 1) == _lib.HK_ERR_INVALID and "rollout is open" in L.hk_last_error(h).decode()
    with pytest.raises(RuntimeError, match="rollout is open"):
        tr.load_state_dict(sd)
    g.step(2 * PERIOD)
    g.rollout_close()
    assert tr.counters() == counters
    _same(before, _state(tr), "after the refusals while a rollout was open")
