"""PPO trainer on the device (include/hk.h "PPO trainer") against the float64 torch restatement (ppo_restate.py): the training forward is the
inference chain bit for bit, the critic / GAE / gradients / Adam agree with the restatement, updates are deterministic, publish closes the loop,
the update optimises, and every refusal of the contract holds.  24 envs, 2v2 Oval, a stochastic 312 -> 256 x 3 and a deterministic 128 x 2 actor."""
import numpy as np
import pytest

import ppo_restate as PR
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.rollout import stacked_inputs, transition_rewards
from hierarchicalkarting_amd.ppo import permutation
from parity import assert_bits_equal
from test_rollout_gpu import _rows_vs_oracle, _same_state

pytestmark = pytest.mark.gpu
RL, P, R = _lib.HK_LOW_RL, 2, 90
KW = dict(low_mode=[RL] * 4, rewards=1, max_episode_steps=150, jitter_seed=4)


def _torch():
    import torch
    torch.cuda.init()                      # torch's HIP runtime first (see RacingEnv.torch_views)
    return torch


def _actors(D):
    return [(Policy.random(D * 4, 256, 3, seed=1), [0, 1]), (Policy.random(D * 4, 128, 2, seed=2, deterministic=True), [2, 3])]


def _env(record=True):
    import hierarchicalkarting_amd as hk
    _torch()
    g = hk.RacingEnv(hk.make_config(24, 4, **KW))
    g.reset()
    pols = _actors(g.obs_dim)
    for k, (pol, slots) in enumerate(pols):
        assert g.attach_policy(pol, slots, P) == k
    if record:
        g.rollout_begin(R)
        g.step(R * P)
        g.rollout_close()
    return g, pols


def _rows(g, pols, p, rows=None):
    """host view of the first `rows` rows (all: None) of policy p: (stacked inputs [n, in], per-row fields flattened in (t, e, j) order,
    bootstrap inputs [E S, in])"""
    ro = g.rollout()
    pol, slots = pols[p]
    rows = ro["obs"].shape[0] if rows is None else rows
    X = stacked_inputs(ro, slots, pol.stack)[:rows]                # [rows, E, S, in]
    boot = np.concatenate([X[-1][:, :, ro["obs"].shape[3]:], ro["next_obs"][:, slots, :]], axis=2)
    f = {k: ro[k][:rows, :, slots].reshape(-1) for k in ("raw", "mu", "logp_cont", "logp_disc", "branch")}
    f["logits"] = ro["logits"][:rows, :, slots, :pol.n_branch].reshape(-1, pol.n_branch)
    f["r"] = transition_rewards(ro)[:rows, :, slots]
    f["done"] = np.repeat(ro["done"][:rows, :, None], len(slots), axis=2)
    return X.reshape(-1, X.shape[-1]), f, boot.reshape(-1, boot.shape[-1]), ro


def _ids(torch, a):
    return torch.as_tensor(np.asarray(a, np.int32), device="cuda:0")


def _restate_grad(tr, pol, Xn, f, adv, v_old, ret, ids, eps, beta, flat):
    torch = _torch()
    ap = PR.tensors(tr.actor_params(flat), True)
    cp = PR.tensors(tr.critic_params(flat), True)
    T = lambda a: torch.tensor(np.asarray(a, np.float64)[ids])
    L, st, heads = PR.loss(ap, cp, len(pol.W), len(tr.critic_policy.W), Xn[ids], T(f["raw"]), torch.tensor(f["branch"][ids].astype(np.int64)),
                           T(f["logp_cont"]), T(f["logp_disc"]), T(adv), T(v_old), T(ret), eps, beta)
    L.backward()
    return ap, cp, st


def test_unchanged_parameters_reproduce_the_recorded_heads():
    torch = _torch()
    g, pols = _env()
    for p in (0, 1):
        tr = g.ppo_trainer(p)
        tr.advantages()
        X, f, _, _ = _rows(g, pols, p)
        n = X.shape[0]
        st = tr.minibatch(_ids(torch, np.arange(n)), 0.2, 5e-3)
        assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0, st
        assert_bits_equal(tr.read("mb_mu"), f["mu"], "policy %d mu" % p)
        assert_bits_equal(tr.read("mb_logits").reshape(n, -1), f["logits"], "policy %d logits" % p)


def test_critic_and_gae_against_the_restatement():
    g, pols = _env()
    pol = pols[0][0]
    X, f, boot, ro = _rows(g, pols, 0)
    for norm in (False, True):
        tr = g.ppo_trainer(0, normalize_advantages=norm, gamma=0.99, lambd=0.95)
        tr.advantages()
        cp = PR.tensors(tr.critic_params())
        Xn = PR.normalise(X, pol.norm_mean, pol.norm_std)
        v_ref = PR.critic_values(Xn, cp, len(tr.critic_policy.W)).numpy()
        v_dev = tr.read("v_old")
        assert np.abs(v_dev - v_ref).max() <= 1e-5 * max(1.0, np.abs(v_ref).max())
        vb = PR.critic_values(PR.normalise(boot, pol.norm_mean, pol.norm_std), cp, len(tr.critic_policy.W)).numpy()
        E, S = 24, 2
        A, RET = PR.gae(f["r"], f["done"], v_dev.reshape(R, E, S), vb.reshape(E, S), 0.99, 0.95)
        if norm:
            A = PR.normalise_adv(A)
        for name, ref in (("adv", A), ("ret", RET)):
            dev = tr.read(name).reshape(ref.shape)
            assert np.abs(dev - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), name
    assert (ro["done"] != 0).any()


def test_gradients_against_autograd():
    torch = _torch()
    g, pols = _env()
    pol = pols[0][0]
    tr = g.ppo_trainer(0)
    tr.advantages()
    X, f, _, _ = _rows(g, pols, 0)
    n = X.shape[0]
    Xn = PR.normalise(X, pol.norm_mean, pol.norm_std)
    adv, v_old, ret = tr.read("adv"), tr.read("v_old"), tr.read("ret")
    flat = tr.read("params")
    rng = np.random.default_rng(5)
    worst = 0.0
    for m in (1, 63, 64, 65, n):
        ids = rng.permutation(n)[:m]
        dev_ids = np.concatenate([ids[: m // 2], [n + 7], ids[m // 2:]]).astype(np.int32)     # one out of range, skipped
        st = tr.minibatch(_ids(torch, dev_ids), 0.2, 5e-3)
        assert st["skipped"] == 1.0
        ap, cp, ref = _restate_grad(tr, pol, Xn, f, adv, v_old, ret, ids, 0.2, 5e-3, flat)
        gd = tr.read("grad")
        ga, gc = tr.actor_params(gd), tr.critic_params(gd)
        for got, want in ((ga, ap), (gc, cp)):
            dif = sum(np.sum((got[k].astype(np.float64) - want[k].grad.numpy()) ** 2) for k in want) ** 0.5
            ref_n = sum(np.sum(want[k].grad.numpy() ** 2) for k in want) ** 0.5
            assert dif <= 1e-4 * ref_n, (m, dif / ref_n)          # observed <= 1e-5: a 10x margin
            for name in want:
                gr = want[name].grad.numpy()
                err = np.linalg.norm(got[name].astype(np.float64) - gr) / max(np.linalg.norm(gr), 1e-30)
                worst = max(worst, err)
                # per tensor: a sum over rows whose terms cancel keeps the fp32 rounding of its terms — b_mu over all rows under normalised
                # advantages is 7e-5 against 10 for 65 rows and agrees to 1.2e-3 (bound 5e-3: a 4x margin); every other tensor agrees to
                # <= 1e-5 (bound 1e-4: a 10x margin)
                assert err <= (5e-3 if name == "b_mu" else 1e-4), (m, name, err)
        for k in ("L_pi", "L_v", "entropy", "clip_fraction"):
            assert abs(st[k] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-6, (m, k, st[k], ref[k])
        # approx-KL at unchanged parameters: the device's is 0 exactly (the recorder's chain); the restatement's is the fp32 rounding of LOGP_*
        assert st["approx_kl"] == 0.0 and abs(ref["approx_kl"]) <= 2e-5, (m, ref["approx_kl"])
    print("worst relative gradient error %.3g" % worst)


def test_adam_matches_the_float32_restatement():
    torch = _torch()
    g, pols = _env()
    tr = g.ppo_trainer(0, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8)
    tr.advantages()
    n = tr.read("adv").size
    for step in (1, 2):
        tr.minibatch(_ids(torch, np.arange(0, n, 3)), 0.2, 5e-3, stats=False)
        p0, gr, m, v = tr.read("params"), tr.read("grad"), tr.read("adam_m"), tr.read("adam_v")
        tr.adam(3e-4)
        pr, m, v = PR.adam_f32(p0, gr, m, v, step, 3e-4)
        for name, ref in (("params", pr), ("adam_m", m), ("adam_v", v)):
            got = tr.read(name)
            ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
            assert ulp.max() <= 1, (step, name, ulp.max())


def test_update_is_deterministic_and_publish_closes_the_loop():
    import hierarchicalkarting_amd as hk
    g, pols = _env()
    t1, t2 = g.ppo_trainer(0, seed=7), g.ppo_trainer(0, seed=7)
    for t in (t1, t2):
        t.advantages()
    s1 = t1.update(2, 256, 3e-4, 0.2, 5e-3)
    s2 = t2.update(2, 256, 3e-4, 0.2, 5e-3)
    assert_bits_equal(t1.read("params"), t2.read("params"), "PARAMS of two identical updates")
    assert s1 == s2
    # the device's row permutation of the second epoch (count 1) is the host twin's, a bijection of [0, n)
    n = t1.read("adv").size
    perm = t1.read("perm")
    assert np.array_equal(perm, permutation(n, 7, 1)) and np.array_equal(np.sort(perm), np.arange(n))
    assert not np.array_equal(perm, permutation(n, 7, 0))
    a = t2.actor()
    assert not np.array_equal(a.W[0], pols[0][0].W[0])
    # the attached actor now computes exactly what a fresh handle with actor() attached computes; the other actor is untouched
    h = hk.RacingEnv(hk.make_config(24, 4, **KW))
    h.reset()
    h.attach_policy(a, [0, 1], P)
    h.attach_policy(pols[1][0], [2, 3], P)
    x = np.random.default_rng(3).standard_normal((300, a.in_dim)).astype(np.float32) * 2
    for p in (0, 1):
        mu_g, lg_g = g.policy_forward(p, x)
        mu_h, lg_h = h.policy_forward(p, x)
        assert_bits_equal(mu_g, mu_h, "mu %d" % p)
        assert_bits_equal(lg_g, lg_h, "logits %d" % p)
    # the next hk_step acts with the published weights: the recorded heads are actor()'s on the recorded stacked inputs
    g.rollout_begin(8); g.step(8 * P); g.rollout_close()
    X, f, _, _ = _rows(g, pols, 0)
    mu, lg = h.policy_forward(0, X.astype(np.float32))
    assert_bits_equal(mu, f["mu"], "next rollout MU")
    assert_bits_equal(lg, f["logits"], "next rollout LOGITS")


def test_published_actor_records_what_the_oracle_twin_records():
    """weights trained on one handle, written into a fresh handle's trainer and published there (hk_ppo_publish re-lays Wt / Wq / heads),
    record a rollout bit-identical, state and rows, to the CPU oracle twin with actor() attached the host way"""
    import hierarchicalkarting_amd as hk
    import oracle_lib as O
    torch = _torch()
    g, pols = _env()
    tr = g.ppo_trainer(0, seed=11)
    tr.advantages()
    tr.update(1, 512, 3e-4, 0.2, 5e-3)
    a = tr.actor()
    assert not np.array_equal(a.W[1], pols[0][0].W[1])
    cfg = hk.make_config(24, 4, **KW)
    g2, o2 = hk.RacingEnv(cfg), O.OracleEnv(cfg)
    g2.reset(); o2.reset()
    for pol, slots in pols:
        g2.attach_policy(pol, slots, P)
    pols2 = [(a, [0, 1]), pols[1]]
    for pol, slots in pols2:
        o2.attach_policy(pol, slots, P)
    t2 = g2.ppo_trainer(0)
    t2.views()["params"][:tr.n_actor].copy_(torch.from_numpy(tr.read("params")[:tr.n_actor]).to("cuda:0"))
    torch.cuda.synchronize()
    t2.publish()
    ro, n_done = _rows_vs_oracle(g2, o2, pols2, R, (1, 7, 50, 2, 64))
    _same_state(g2, o2, "after the rollout", skip_acc=True)
    assert n_done > 0
    X = stacked_inputs(ro, [0, 1], a.stack).reshape(-1, a.in_dim)
    mu_o, lg_o = o2.policy_forward(0, X)
    assert_bits_equal(ro["mu"][:, :, [0, 1]].reshape(-1), mu_o, "MU against the oracle's forward")
    assert_bits_equal(ro["logits"][:, :, [0, 1], :a.n_branch].reshape(-1, a.n_branch), lg_o, "LOGITS against the oracle's forward")


def test_short_rollout_trains_on_its_completed_rows():
    """a rollout closed before all its rows: the trainer reads the completed rows only, bootstraps after the last of them, and a rollout
    with none is refused"""
    torch = _torch()
    g, pols = _env(record=False)
    pol = pols[0][0]
    g.rollout_begin(R)
    g.step((R - 17) * P)
    g.rollout_close()
    rows = g.rollout_rows()
    assert rows == R - 17
    tr = g.ppo_trainer(0, normalize_advantages=False)
    tr.advantages()
    E, S = 24, 2
    n = rows * E * S
    X, f, boot, ro = _rows(g, pols, 0, rows)
    v_dev = tr.read("v_old")
    assert v_dev.size == n
    cp = PR.tensors(tr.critic_params())
    v_ref = PR.critic_values(PR.normalise(X, pol.norm_mean, pol.norm_std), cp, len(tr.critic_policy.W)).numpy()
    assert np.abs(v_dev - v_ref).max() <= 1e-5 * max(1.0, np.abs(v_ref).max())
    vb = PR.critic_values(PR.normalise(boot, pol.norm_mean, pol.norm_std), cp, len(tr.critic_policy.W)).numpy()
    A, RET = PR.gae(f["r"], f["done"], v_dev.reshape(rows, E, S), vb.reshape(E, S), 0.99, 0.95)
    for name, ref in (("adv", A), ("ret", RET)):
        assert np.abs(tr.read(name).reshape(ref.shape) - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), name
    # ids past the completed rows are out of range: skipped, never read
    st = tr.minibatch(_ids(torch, np.arange(n + 5)), 0.2, 5e-3)
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 5.0, st
    assert_bits_equal(tr.read("mb_mu")[:n], f["mu"], "short rollout mu")
    st = tr.update(1, 256, 3e-4, 0.2, 5e-3)
    assert st["skipped"] == 0.0 and np.isfinite(list(st.values())).all()
    g.rollout_begin(4)
    g.rollout_close()
    assert g.rollout_rows() == 0
    assert g.L.hk_ppo_advantages(g.h, tr.t) == _lib.HK_ERR_INVALID


def test_critic_chunks_do_not_change_the_advantages():
    """hk_ppo_advantages runs the critic in chunks of max(cap, min(n + E S, 16 384)) rows.  96 envs: n = 17 280, n + E S = 17 472 — two chunks
    (16 384 + 1 088) on a dropped workspace, one chunk once a minibatch of 17 472 ids has raised cap.  Bit equality, in both precisions: an output
    row of either product kernel is a fixed-order chain over k whatever tile or chunk the row falls in, the value head is per row, and GAE and
    the normalisation are fixed-order functions of V_OLD."""
    import hierarchicalkarting_amd as hk
    torch = _torch()
    E, S = 96, 2
    g = hk.RacingEnv(hk.make_config(E, 4, **KW))
    g.reset()
    for pol, slots in _actors(g.obs_dim):
        g.attach_policy(pol, slots, P)
    g.rollout_begin(R); g.step(R * P); g.rollout_close()
    n = R * E * S
    assert n == 17280 and 16384 < n + E * S < 2 * 16384
    ids = _ids(torch, np.concatenate([np.arange(n), np.full(E * S, n)]))
    tr = g.ppo_trainer(0)
    for prec in ("f32", "bf16"):
        tr.set_precision(prec)                  # (drops the workspace: cap 0)
        tr.advantages()
        two = {k: tr.read(k) for k in ("v_old", "adv", "ret")}
        assert two["v_old"].size == n
        st = tr.minibatch(ids, 0.2, 5e-3)       # the ids equal to n are out of range for a minibatch
        assert st["skipped"] == float(E * S), st
        tr.advantages()
        for k, a in two.items():
            assert_bits_equal(tr.read(k), a, "%s %s: one chunk against two" % (prec, k))


def test_update_optimises():
    g, pols = _env()
    # the value fit: eps 1e3, since the value clip around the fixed V_OLD would hold L_v near its start by design (PPO's clipped value loss)
    tv = g.ppo_trainer(0, seed=3)
    tv.advantages()
    hist = [tv.update(1, 256, 3e-3, 1e3, 5e-3) for _ in range(10)]
    assert hist[-1]["L_v"] < 0.5 * hist[0]["L_v"], [h["L_v"] for h in hist]
    # the surrogate at the reference's settings (epsilon 0.2, lr 3e-4) on the same fixed rollout
    tp = g.ppo_trainer(1, seed=4)
    tp.advantages()
    hist = [tp.update(1, 256, 3e-4, 0.2, 5e-3) for _ in range(10)]
    assert hist[-1]["L_pi"] < hist[0]["L_pi"], [h["L_pi"] for h in hist]
    assert hist[-1]["approx_kl"] != 0.0


def test_refusals():
    torch = _torch()
    g, pols = _env(record=False)
    L, h = g.L, g.h
    tr = g.ppo_trainer(0)
    assert L.hk_ppo_advantages(h, tr.t) == _lib.HK_ERR_INVALID                  # never opened
    assert L.hk_ppo_advantages(h, 9) == _lib.HK_ERR_INVALID                     # bad trainer
    assert L.hk_ppo_ptr(h, tr.t, 99) is None and L.hk_ppo_count(h, tr.t, -1) == _lib.HK_ERR_INVALID
    ids = _ids(torch, [0, 1])
    st = None
    g.rollout_begin(4)
    assert L.hk_ppo_advantages(h, tr.t) == _lib.HK_ERR_INVALID                  # open
    assert L.hk_ppo_publish(h, tr.t) == _lib.HK_ERR_INVALID                     # publish during an open rollout
    g.step(4 * P); g.rollout_close()
    assert L.hk_ppo_minibatch(h, tr.t, ids.data_ptr(), 2, 0.2, 0.0, st) == _lib.HK_ERR_INVALID    # no advantages yet
    tr.advantages()
    assert L.hk_ppo_minibatch(h, tr.t, ids.data_ptr(), 2, 0.2, 0.0, st) == 0
    g.rollout_begin(2); g.step(2 * P); g.rollout_close()
    assert L.hk_ppo_minibatch(h, tr.t, ids.data_ptr(), 2, 0.2, 0.0, st) == _lib.HK_ERR_INVALID    # advantages of an earlier rollout
    assert L.hk_ppo_update(h, tr.t, 1, 2, 1e-4, 0.2, 0.0, st) == _lib.HK_ERR_INVALID
    bad = Policy.random(pols[0][0].in_dim + 2, 64, 1, n_branch=1, normalize=False)
    with pytest.raises(_lib.HkError):
        g.ppo_trainer(0, critic=bad)                                            # in_dim does not fit
    wide = Policy.random(pols[0][0].in_dim, 512, 1, n_branch=1, normalize=False)
    with pytest.raises(_lib.HkError):
        g.ppo_trainer(0, critic=wide)                                           # hidden beyond the limits
    d, _keep = pols[0][0].desc()
    assert L.hk_ppo_create(h, 7, d, None) == _lib.HK_ERR_INVALID                # no such policy
