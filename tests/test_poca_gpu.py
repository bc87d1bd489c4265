"""POCA trainer on the device (include/hk.h "POCA") against the float64 torch restatement (poca_restate.py).  Four cases: 24 envs of 2v2 Oval
with a stochastic 312 -> 256 x 3 actor on slots [0, 1] and a critic of H = 256, 2 layers; the same with H = 36 (a head width of 9), 1 layer;
8 envs of the 8-agent default wiring (4v4) with the policy on slots [0 .. 3] and H = 64, so S = 4; the first set-up again with a critic of
H = 12, 3 layers.  R = 90 decisions of period 2 with
max_episode_steps 150: episodes end inside the rollout."""
import functools

import numpy as np
import pytest

import poca_restate as QR
import ppo_restate as PR
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.poca import PocaCritic
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.ppo import clip_coefficient, grad_norm, permutation
from hierarchicalkarting_amd.rollout import stacked_inputs, transition_rewards
from parity import assert_bits_equal

pytestmark = pytest.mark.gpu
RL, P, R = _lib.HK_LOW_RL, 2, 90
EPS, BETA, LR = 0.2, 5e-3, 3e-4
CASES = {
    "h256": dict(E=24, A=4, slots=[0, 1], other=[2, 3], actor=(256, 3), H=256, L=2),
    "h36": dict(E=24, A=4, slots=[0, 1], other=[2, 3], actor=(256, 3), H=36, L=1),
    "s4": dict(E=8, A=8, slots=[0, 1, 2, 3], other=[4, 5, 6, 7], actor=(64, 2), H=64, L=2),
    # three encoder layers: the backward swaps its two delta buffers once per layer above the first, so an even number of swaps only runs here
    # (H = 12 is the smallest width with more than one channel per head).  The env and the actors are h36's: 8 envs of 2v2 under a 64 x 2 actor
    # record no episode end or no group reward in 90 decisions, which _host refuses.
    "l3": dict(E=24, A=4, slots=[0, 1], other=[2, 3], actor=(256, 3), H=12, L=3),
}


def _kw(A):
    """the training scenes' set-up (karts scattered at reset, no start hold, every agent a training agent): checkpoints are passed within the 150
    steps of an episode, so the rollout holds group rewards as well as episode ends"""
    return dict(low_mode=[RL] * A, rewards=1, max_episode_steps=150, jitter_seed=4, env_mode=_lib.HK_MODE_TRAINING, training_agents=[1] * A)


def _torch():
    import torch
    torch.cuda.init()                      # torch's HIP runtime first (see RacingEnv.torch_views)
    return torch


def _ids(torch, a):
    return torch.as_tensor(np.asarray(a, np.int32), device="cuda:0")


def _env(case="h256", record=True, rows=R, other_actor=(64, 2), **over):
    import hierarchicalkarting_amd as hk
    _torch()
    c = CASES[case]
    kw = _kw(c["A"])
    kw.update(over)
    g = hk.RacingEnv(hk.make_config(c["E"], c["A"], **kw))
    g.reset()
    stack = min(4, _lib.HK_POLICY_MAX_IN // g.obs_dim)
    pols = [(Policy.random(g.obs_dim * stack, c["actor"][0], c["actor"][1], stack=stack, seed=1), c["slots"]),
            (Policy.random(g.obs_dim * stack, other_actor[0], other_actor[1], stack=stack, seed=2, deterministic=True), c["other"])]
    for k, (pol, slots) in enumerate(pols):
        assert g.attach_policy(pol, slots, P) == k
    if record:
        g.rollout_begin(rows)
        g.step(rows * P)
        g.rollout_close()
    return g, pols


def _critic(case, pol, seed=3):
    c = CASES[case]
    cr = PocaCritic.random(pol.in_dim, pol.n_branch, c["H"], c["L"], seed)
    rng = np.random.default_rng(seed + 100)
    for n in cr.arrays:          # biases off zero, so that a forward that dropped one would show
        if n.startswith("b"):
            cr.arrays[n] = (rng.standard_normal(cr.arrays[n].shape) * 0.05).astype(np.float32)
    return cr


def _host(g, pols):
    """host view of policy 0's rows: X [R, E, S, in], bootstrap inputs [E, S, in], per-agent fields [R, E, S], done [R, E]"""
    ro = g.rollout()
    pol, slots = pols[0]
    X = stacked_inputs(ro, slots, pol.stack)
    boot = np.concatenate([X[-1][:, :, ro["obs"].shape[3]:], ro["next_obs"][:, slots, :]], axis=2)
    f = {k: ro[k][:, :, slots] for k in ("raw", "mu", "logp_cont", "logp_disc", "branch")}
    f["logits"] = ro["logits"][:, :, slots, :pol.n_branch]
    d = ro["done"][:, :, None] != 0
    f["r"] = transition_rewards(ro)[:, :, slots]
    f["g"] = np.where(d, ro["term_group_reward"], ro["group_reward"])[:, :, slots]
    f["done"] = ro["done"]
    assert (ro["done"] != 0).any() and (ro["group_reward"] != 0).any()
    return X, boot, f


@functools.lru_cache(maxsize=None)
def _setup(case):
    """one env, rollout and un-normalised trainer per case, with the restatement's V, B over every group (computed once, never changed)"""
    torch = _torch()
    g, pols = _env(case)
    pol = pols[0][0]
    tr = g.poca_trainer(0, critic=_critic(case, pol), normalize_advantages=False)
    tr.advantages()
    X, boot, f = _host(g, pols)
    Rr, E, S, _ = X.shape
    flat = tr.read("params")
    cp = PR.tensors(tr.critic_params(flat))
    Xn = PR.normalise(X, pol.norm_mean, pol.norm_std)
    with torch.no_grad():
        V, B = QR.critic(Xn.reshape(Rr * E, S, -1), QR.action_features(f["raw"], f["branch"], pol.n_branch).reshape(Rr * E, S, -1), cp, CASES[case]["L"])
        Vb, _ = QR.critic(PR.normalise(boot, pol.norm_mean, pol.norm_std), torch.zeros(E, S, 1 + pol.n_branch, dtype=torch.float64), cp, CASES[case]["L"])
    ref = dict(V=V.numpy().reshape(Rr, E), B=B.numpy().reshape(Rr, E, S), Vb=Vb.numpy())
    for a in ref.values():
        a.setflags(write=False)
    return g, pols, tr, X, Xn, f, flat, ref


def _close(dev, ref, rel, what):
    err, scale = np.abs(np.asarray(dev, np.float64) - ref).max(), max(1.0, np.abs(ref).max())
    print("%s: worst error %.3g against max(1, max|ref|) = %.3g (relative %.3g, bound %.3g)" % (what, err, scale, err / scale, rel))
    assert err <= rel * scale, (what, err, scale)


@pytest.mark.parametrize("case", list(CASES))
def test_values_baselines_team_reward_and_returns_against_the_restatement(case):
    """The bound is the PPO tests' form, 1e-5 max(1, max|ref|) (test_critic_and_gae_against_the_restatement), and it holds: observed on these
    shapes (the figures are printed), relative to max(1, max|ref|): V_OLD 1.3e-6 / 4.4e-7 / 9.9e-7 (h256 / h36 / s4), B_OLD 9.5e-7 / 5.3e-7 /
    6.3e-7, RET <= 2.7e-7, ADV <= 3.1e-7 — LayerNorm and the softmax stay inside it, so no wider bound is taken."""
    g, pols, tr, X, Xn, f, flat, ref = _setup(case)
    Rr, E, S, _ = X.shape
    v = tr.read("v_old").reshape(Rr, E, S)
    b = tr.read("b_old").reshape(Rr, E, S)
    for j in range(1, S):
        assert_bits_equal(v[:, :, j], v[:, :, 0], "a group's rows share one V_OLD")
    _close(v[:, :, 0], ref["V"], 1e-5, case + " V_OLD")
    _close(b, ref["B"], 1e-5, case + " B_OLD")
    assert_bits_equal(tr.read("team_reward").reshape(Rr, E, S), QR.team_reward_f32(f["r"], f["g"]), "TEAM_REWARD")
    # the returns from the device's own V (as the PPO test does), the bootstrap value from the restatement
    G = QR.lambda_returns(QR.team_reward(f["r"], f["g"]), f["done"], v[:, :, 0], ref["Vb"], 0.99, 0.95)
    _close(tr.read("ret").reshape(Rr, E, S), G, 1e-5, case + " RET")
    _close(tr.read("adv").reshape(Rr, E, S), G - b, 1e-5, case + " ADV")


def _restate_grad(tr, pol, L, Xn, f, rows, gids, flat):
    torch = _torch()
    ap = PR.tensors(tr.actor_params(flat), True)
    cp = PR.tensors(tr.critic_params(flat), True)
    Rr, E, S = f["raw"].shape
    pick = lambda a: np.asarray(a).reshape(Rr * E, S, *np.asarray(a).shape[3:])[gids]
    T = lambda a: torch.tensor(np.asarray(pick(a), np.float64))
    Lo, st, heads = QR.loss(ap, cp, len(pol.W), L, Xn.reshape(Rr * E, S, -1)[gids], T(f["raw"]), torch.tensor(pick(f["branch"]).astype(np.int64)),
                            T(f["logp_cont"]), T(f["logp_disc"]), T(rows["adv"]), T(rows["v_old"]), T(rows["b_old"]), T(rows["ret"]), EPS, BETA)
    Lo.backward()
    return ap, cp, st


def _gradient_case(case, sizes):
    """Relative error of the whole critic and the whole actor gradient against autograd, each bounded at 10x the worst observed (printed
    below; both far under the cap of 1e-3): the critic 5.4e-6 (observed <= 5.31e-7: 2.7e-7 .. 5.3e-7 over the five sizes of h256, 3.6e-7 on
    h36, 3.1e-7 on s4), the actor 1.4e-4 (observed <= 1.34e-5: 6.1e-6 .. 1.34e-5 on h256, 3.0e-6 on h36, 2.2e-6 on s4; the PPO trainer's own
    test observes 1e-5).  Per tensor 1e-4, the PPO test's figure, with two exceptions, both sums over rows whose terms cancel and so keep
    the fp32 rounding of their terms: the actor's b_mu (the PPO test's exception, same cause, same bound 5e-3) and the critic's b_k — the softmax is invariant to
    a shift of a score row, so the exact gradient of b_k is 0 and the device's is rounding noise: it is compared in absolute terms,
    against 1e-5 of the critic gradient's norm."""
    torch = _torch()
    g, pols, tr, X, Xn, f, flat, ref = _setup(case)
    pol = pols[0][0]
    Rr, E, S, _ = X.shape
    G = Rr * E
    rows = {k: tr.read(k).reshape(Rr, E, S) for k in ("adv", "v_old", "b_old", "ret")}
    rng = np.random.default_rng(5)
    for mg in sizes:
        mg = G if mg is None else mg
        gids = rng.permutation(G)[:mg]
        dev_ids = np.concatenate([gids[: mg // 2], [G + 3], gids[mg // 2:]]).astype(np.int32)       # one out of range: skipped
        st = tr.minibatch(_ids(torch, dev_ids), EPS, BETA)
        assert st["skipped"] == 1.0, st
        ap, cp, want_st = _restate_grad(tr, pol, CASES[case]["L"], Xn, f, rows, gids, flat)
        gd = tr.read("grad")
        for which, got, want in (("actor", tr.actor_params(gd), ap), ("critic", tr.critic_params(gd), cp)):
            dif = sum(np.sum((got[k].astype(np.float64) - want[k].grad.numpy()) ** 2) for k in want) ** 0.5
            ref_n = sum(np.sum(want[k].grad.numpy() ** 2) for k in want) ** 0.5
            print("%s mg %d: %s gradient relative error %.3g (norm %.3g)" % (case, mg, which, dif / ref_n, ref_n))
            assert dif <= (1.4e-4 if which == "actor" else 5.4e-6) * ref_n, (mg, which, dif / ref_n)
            for name in want:
                gr = want[name].grad.numpy()
                err = np.linalg.norm(got[name].astype(np.float64) - gr)
                if which == "critic" and name == "b_k":
                    assert np.linalg.norm(gr) <= 1e-12 * ref_n and err <= 1e-5 * ref_n, (mg, name, err, ref_n)
                    continue
                rel = err / max(np.linalg.norm(gr), 1e-30)
                assert rel <= (5e-3 if name == "b_mu" else 1e-4), (mg, which, name, rel)
        for k in ("L_pi", "L_v", "L_b", "entropy", "clip_fraction"):
            assert abs(st[k] - want_st[k]) <= 1e-5 * abs(want_st[k]) + 1e-6, (mg, k, st[k], want_st[k])
        assert st["approx_kl"] == 0.0 and abs(want_st["approx_kl"]) <= 2e-5


def test_gradients_against_autograd():
    _gradient_case("h256", (1, 31, 32, 33, None))


@pytest.mark.parametrize("case", ["h36", "s4", "l3"])
def test_gradients_against_autograd_odd_head_width_and_four_agents(case):
    _gradient_case(case, (33,))


def test_exact_properties_at_unchanged_parameters():
    torch = _torch()
    g, pols, tr, X, Xn, f, flat, ref = _setup("h256")
    Rr, E, S, _ = X.shape
    G = Rr * E
    st = tr.minibatch(_ids(torch, np.arange(G)), EPS, BETA)
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0, st
    assert_bits_equal(tr.read("mb_mu"), f["mu"].reshape(-1), "MB_MU against the recorded MU")
    assert_bits_equal(tr.read("mb_logits").reshape(G * S, -1), f["logits"].reshape(G * S, -1), "MB_LOGITS against the recorded LOGITS")
    # the same kernels in the same order per row, whatever chunk or minibatch the row falls in
    assert_bits_equal(tr.read("mb_value"), tr.read("v_old").reshape(G, S)[:, 0], "MB_VALUE against V_OLD per group")
    assert_bits_equal(tr.read("mb_baseline"), tr.read("b_old"), "MB_BASELINE against B_OLD")
    assert g.L.hk_ppo_count(g.h, tr.t, _lib.PPO_FIELDS["mb_value"]) == G and g.L.hk_poca_count(g.h, tr.t, _lib.POCA_FIELDS["mb_baseline"]) == G * S
    g1 = tr.read("grad")
    st2 = tr.minibatch(_ids(torch, np.arange(G)), EPS, BETA)
    assert_bits_equal(tr.read("grad"), g1, "GRAD of the same minibatch twice")
    assert st2 == st
    assert set(tr.views()) >= {"params", "grad", "v_old", "b_old", "team_reward", "mb_baseline", "mb_value"}


def test_adam_and_the_clip_aware_step_on_the_poca_vector():
    torch = _torch()
    g, pols = _env("h256")
    tr = g.poca_trainer(0, critic=_critic("h256", pols[0][0]))
    tr.advantages()
    G = R * CASES["h256"]["E"]
    f32b = lambda x: np.float32(x).view(np.uint32)
    for step in (1, 2):
        tr.minibatch(_ids(torch, np.arange(0, G, 3)), EPS, BETA, stats=False)
        p0, gr, m, v = tr.read("params"), tr.read("grad"), tr.read("adam_m"), tr.read("adam_v")
        assert p0.size == tr.n_actor + tr.critic_policy.flat().size
        if step == 1:
            tr.adam(LR)
            coef = np.float32(1.0)
        else:
            ref = grad_norm(gr)
            tr.adam(LR, max_grad_norm=0.5 * ref)
            w = tr.clip_words()
            assert abs(w["norm"] - ref) / ref <= p0.size * 2.0 ** -53
            assert f32b(w["coef"]) == f32b(clip_coefficient(w["norm"], 0.5 * ref)) and w["coef"] < 1.0
            coef = np.float32(w["coef"])
        pr, m, v = PR.adam_f32(p0, gr * coef, m, v, step, LR)
        for name, want in (("params", pr), ("adam_m", m), ("adam_v", v)):
            got = tr.read(name)
            ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            assert ulp.max() <= 1, (step, name, ulp.max())
    assert tr.counters() == (2, 0)


def test_update_on_group_ids():
    import hierarchicalkarting_amd as hk
    torch = _torch()
    g, pols = _env("h256")
    cr = _critic("h256", pols[0][0])
    t1, t2 = g.poca_trainer(0, critic=cr, seed=7), g.poca_trainer(0, critic=cr, seed=7)
    for t in (t1, t2):
        t.advantages()
    G, MB = R * CASES["h256"]["E"], 256
    s1 = t1.update(2, MB, LR, EPS, BETA)
    assert "L_b" in s1 and s1["skipped"] == 0.0
    perm = t1.read("perm")
    assert perm.size == G and np.array_equal(perm, permutation(G, 7, 1)) and np.array_equal(np.sort(perm), np.arange(G))
    # the same update issued by hand: minibatches of the two epochs' permutations, Adam after each, then publish
    last = []
    for ep in range(2):
        pm = permutation(G, 7, ep).astype(np.int32)
        for b in range(G // MB):
            st = t2.minibatch(_ids(torch, pm[b * MB:(b + 1) * MB]), EPS, BETA)
            t2.adam(LR)
            if ep == 1:
                last.append(st)
    t2.publish()
    for name in ("params", "adam_m", "adam_v"):
        assert_bits_equal(t1.read(name), t2.read(name), name + ": an update against its minibatches by hand")
    for k in ("L_pi", "L_v", "L_b", "approx_kl"):
        assert abs(s1[k] - np.mean([s[k] for s in last])) <= 1e-6 * max(1.0, abs(s1[k])), k
    assert t1.counters() == (2 * (G // MB), 2) and t2.counters() == (2 * (G // MB), 0)          # (the epoch count belongs to update)
    # target_kl stops
    t3 = g.poca_trainer(0, critic=cr, seed=7)
    t3.advantages()
    t3.update(5, MB, 3e-3, EPS, BETA, target_kl=1e-9)
    assert t3.last_report["stopped_by_kl"] == 1 and t3.last_report["epochs_run"] == 1
    # publish closes the loop: the next rollout's recorded heads are the published actor's (t3 published last)
    a = t3.actor()
    assert not np.array_equal(a.W[0], pols[0][0].W[0])
    h = hk.RacingEnv(hk.make_config(24, 4, **_kw(4)))
    h.reset()
    h.attach_policy(a, [0, 1], P)
    g.rollout_begin(8); g.step(8 * P); g.rollout_close()
    ro = g.rollout()
    Xs = stacked_inputs(ro, [0, 1], a.stack).reshape(-1, a.in_dim)
    mu, lg = h.policy_forward(0, Xs.astype(np.float32))
    assert_bits_equal(mu, ro["mu"][:, :, [0, 1]].reshape(-1), "next rollout MU")
    assert_bits_equal(lg, ro["logits"][:, :, [0, 1], :a.n_branch].reshape(-1, a.n_branch), "next rollout LOGITS")


def test_selfplay_takes_a_poca_trainer():
    import hierarchicalkarting_amd as hk
    g, pols = _env("h256", record=False, other_actor=CASES["h256"]["actor"])          # an opponent of the learner's shape
    tr = g.poca_trainer(0, critic=_critic("h256", pols[0][0]), seed=1)
    sp = hk.SelfPlay(g, tr, 1, window=2, save_steps=100, swap_steps=100, max_steps=10000, seed=0)
    out = sp.iteration(rows=8, epochs=1, minibatch=64, lr=LR)
    assert "L_b" in out["update"] and np.isfinite(list(out["update"].values())).all()
    assert out["steps"] == 8 * 24 * 2 and out["saved"] and out["swapped"]


def test_three_updates_lower_the_value_losses():
    g, pols = _env("h256")
    # eps 1e3: the value clips around the fixed V_OLD / B_OLD would hold the losses near their start by design (as in the PPO test)
    tr = g.poca_trainer(0, critic=_critic("h256", pols[0][0]), seed=3)
    tr.advantages()
    hist = [tr.update(1, 256, 3e-3, 1e3, BETA) for _ in range(3)]
    tot = [h["L_v"] + 0.5 * h["L_b"] for h in hist]
    assert tot[-1] < tot[0], tot


def test_resume_continues_bit_for_bit(tmp_path):
    g, pols = _env("h256")
    cr = _critic("h256", pols[0][0])
    t1 = g.poca_trainer(0, critic=cr, seed=9)
    t1.advantages()
    t1.update(1, 256, LR, EPS, BETA, max_grad_norm=1.0)
    path = str(tmp_path / "poca.npz")
    t1.save(path)
    g2, pols2 = _env("h256")                   # a fresh env: the same seeds record the same rollout up to the first publish
    t2 = g2.poca_trainer(0, critic=_critic("h256", pols2[0][0], seed=99), seed=9)
    t2.load(path)
    assert t2.counters() == t1.counters()
    # the same rollout on both: g's closed rollout is still the current one; g2 recorded the same rows before the load
    for t in (t1, t2):
        t.advantages()
    for k in ("v_old", "adv", "ret", "b_old"):
        assert_bits_equal(t1.read(k), t2.read(k), k + " after the load")
    s1 = t1.update(1, 256, LR, EPS, BETA, max_grad_norm=1.0)
    s2 = t2.update(1, 256, LR, EPS, BETA, max_grad_norm=1.0)
    assert s1 == s2 and t1.counters() == t2.counters()
    for name in ("params", "adam_m", "adam_v"):
        assert_bits_equal(t1.read(name), t2.read(name), name + " after the resumed update")
    # a PPO checkpoint does not load into a POCA trainer, nor the reverse
    tp = g.ppo_trainer(1)
    with pytest.raises(ValueError, match="kind"):
        t1.load_state_dict(tp.state_dict())
    with pytest.raises(ValueError, match="kind"):
        tp.load_state_dict(t1.state_dict())


def test_refusals():
    import hierarchicalkarting_amd as hk
    torch = _torch()
    g, pols = _env("h256")
    pol = pols[0][0]
    L, h = g.L, g.h
    INV = _lib.HK_ERR_INVALID

    def create(policy=0, **change):
        cr = _critic("h256", pol)
        d, keep = cr.desc()
        for k, v in change.items():
            setattr(d, k, v)
        return L.hk_ppo_create_poca(h, policy, d, None)
    assert create(hidden=258) == INV and create(hidden=0) == INV and create(hidden=260) == INV         # not a multiple of 4, out of range
    assert create(n_layers=0) == INV and create(n_layers=5) == INV
    assert create(reserved0=1) == INV and create(reserved1=1) == INV
    for name in ("W_obs", "b_act", "W_q", "b_k", "W_v", "b_out", "w_val", "b_val"):
        assert create(**{name: None}) == INV, name
    d, keep = _critic("h256", pol).desc()
    d.W[1] = None
    assert L.hk_ppo_create_poca(h, 0, d, None) == INV                                                   # a NULL encoder layer
    assert L.hk_ppo_create_poca(h, 0, None, None) == INV and create(policy=7) == INV
    bad_cfg = _lib.PpoConfig(0.99, 0.95, 1, 1.5, 0.999, 1e-8, 0)
    d, keep = _critic("h256", pol).desc()
    assert L.hk_ppo_create_poca(h, 0, d, bad_cfg) == INV                                                # what hk_ppo_create refuses
    assert b"hk_ppo_create_poca" in L.hk_last_error(h)
    # groups: one slot (S = 1), half a team, slots of two teams; rewards off
    def wired(slot_sets, A=4, **kw):
        e = hk.RacingEnv(hk.make_config(4, A, low_mode=[RL] * A, rewards=kw.pop("rewards", 1), max_episode_steps=150, **kw))
        e.reset()
        out = []
        for k, slots in enumerate(slot_sets):
            p = Policy.random(e.obs_dim * 4, 64, 1, seed=k)
            e.attach_policy(p, slots, P)
            dd, kp = PocaCritic.random(p.in_dim, p.n_branch, 16, 1, 0).desc()
            out.append(e.L.hk_ppo_create_poca(e.h, k, dd, None))
        return out
    assert wired([[0], [1, 2]]) == [INV, INV]                      # S = 1; two teams
    assert wired([[0, 1]], rewards=0) == [INV]
    assert wired([[0, 1], [2, 3]]) == [0, 1]
    e8 = hk.RacingEnv(hk.make_config(2, 8, low_mode=[RL] * 8, rewards=1))
    e8.reset()
    p8 = Policy.random(e8.obs_dim * 2, 64, 1, stack=2, seed=0)
    e8.attach_policy(p8, [0, 1], P)
    dd, kp = PocaCritic.random(p8.in_dim, p8.n_branch, 16, 1, 0).desc()
    assert e8.L.hk_ppo_create_poca(e8.h, 0, dd, None) == INV                                            # two of a team of four
    # bf16 is refused and nothing changes
    tr = g.poca_trainer(0, critic=_critic("h256", pol))
    assert L.hk_ppo_set_precision(h, tr.t, _lib.HK_PPO_PREC_BF16) == _lib.HK_ERR_UNSUPPORTED
    assert tr.precision == "f32" and L.hk_ppo_count(h, tr.t, _lib.PPO_FIELDS["shadow"]) == 0
    with pytest.raises(ValueError):
        tr.set_precision("bf16")
    with pytest.raises(ValueError):
        g.poca_trainer(0, precision="bf16")
    # the POCA fields belong to POCA trainers
    tp = g.ppo_trainer(0)
    assert L.hk_poca_count(h, tp.t, 0) == INV and L.hk_poca_ptr(h, tp.t, 0) is None and L.hk_poca_count(h, tr.t, 3) == INV
    assert L.hk_poca_stats(h, tr.t, None) == INV
    # a snapshot pool still refuses to load into a policy that has a (POCA) trainer
    pool = g.snapshot_pool(0, 2)
    pool.save(0, 0)
    with pytest.raises(_lib.HkError):
        pool.load(0, 0)


def test_a_ppo_and_a_poca_trainer_on_one_handle_do_not_disturb_each_other():
    torch = _torch()
    ids = None
    grads = []
    for with_poca in (False, True):
        g, pols = _env("h256")
        if with_poca:
            tq = g.poca_trainer(0, critic=_critic("h256", pols[0][0]))
        tp = g.ppo_trainer(0)
        if with_poca:
            tq.advantages()
            tq.minibatch(_ids(torch, np.arange(40)), EPS, BETA)
        tp.advantages()
        n = tp.read("adv").size
        ids = np.random.default_rng(2).permutation(n)[:300]
        tp.minibatch(_ids(torch, ids), EPS, BETA)
        if with_poca:
            tq.minibatch(_ids(torch, np.arange(7)), EPS, BETA)
        grads.append(tp.read("grad"))
    assert_bits_equal(grads[0], grads[1], "the PPO trainer's GRAD with and without a POCA trainer on the handle")
