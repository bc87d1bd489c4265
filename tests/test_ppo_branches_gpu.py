"""PPO trainer off its easy path (include/hk.h "PPO trainer") against the float64 restatement (ppo_restate.py):
  * the loss at PERTURBED parameters, where rho != 1 and v != V_OLD: every arm of the clipped surrogate and of the clipped value loss, the
    clip count, approx-KL, exact zeros for dead rows, and all of it again with the advantages negated;
  * the gather on a rollout that begins mid-episode (live RING0, clears inside the first and the last stack - 1 rows), stacks below the
    handle's largest, the fp32 product kernel at its N / K edges, 1 and 4 layers, a critic shaped unlike its actor;
  * hk_ppo_update against the same minibatches issued by hand.
The float64 restatement and the fp32 kernel may take different sides of a branch for a row ON a boundary; ppo_restate.classify names those
rows ("undecided", margin 1e-3: the device's rho is within a few 1e-5 of the float64 one) and no minibatch of the branch tests holds one."""
from types import SimpleNamespace

import numpy as np
import pytest

import ppo_restate as PR
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.ppo import permutation
from parity import assert_bits_equal
from test_ppo_gpu import KW, P, _env, _ids, _restate_grad, _rows, _torch

pytestmark = pytest.mark.gpu
RL = _lib.HK_LOW_RL
# The perturbation p (1 + S xi) (+ 0.1 S xi' on the vectors) and the clip range, chosen on the restatement (never on the device) so that the
# conditions of _branches() hold; the shares they give on the recorded rollout are in _branches()'s docstring.
S_NOISE, EPS, BETA, MARGIN = 0.05, 0.2, 5e-3, 1e-3
TOL, TOL_B_MU = 1e-4, 5e-3          # test_ppo_gpu.test_gradients_against_autograd's bounds: per tensor and overall; b_mu, whose terms cancel

_cache = {}


def _perturb(tr, torch, s, seed):
    flat = tr.read("params").copy()
    r = np.random.default_rng(seed)
    o = 0
    for name, shape in tr.actor_layout + tr.critic_layout:
        k = int(np.prod(shape))
        seg = flat[o:o + k]
        seg *= (1.0 + s * r.standard_normal(k)).astype(np.float32)
        if len(shape) == 1:
            seg += (0.1 * s * r.standard_normal(k)).astype(np.float32)
        o += k
    assert o == flat.size
    tr.views()["params"].copy_(torch.from_numpy(flat).to("cuda:0"))
    torch.cuda.synchronize()
    got = tr.read("params")
    assert_bits_equal(got, flat, "PARAMS as written")
    return got


def _terms(S, adv):
    torch = _torch()
    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    f = S.f
    return PR.row_terms(PR.tensors(S.tr.actor_params(S.flat)), PR.tensors(S.tr.critic_params(S.flat)), len(S.pol.W), len(S.tr.critic_policy.W), S.Xn,
                        T(f["raw"]), torch.tensor(f["branch"].astype(np.int64)), T(f["logp_cont"]), T(f["logp_disc"]), T(adv), T(S.v_old), T(S.ret),
                        EPS, BETA)


def _branches():
    """The shared set-up, built once and left unchanged: test_ppo_gpu's rollout (24 envs, 2v2 Oval, R = 90, policy 0, n = 4 320), advantages()
    at the recorded parameters, then PARAMS perturbed (V_OLD / ADV / RET stay the unperturbed critic's), the float64 terms of every row
    and their classes.  The conditions are asserted on the restatement before any minibatch runs.
    Measured on the restatement at s = 0.05, eps = 0.2 (the first pair tried): 2.94 % of the rows undecided; decided rows per class, in
    % of n — continuous column 25.35 / 5.07 / 18.01 / 2.78 / 45.86 (below-live, below-dead, above-dead, above-live, inside), discrete column
    5.88 / 2.52 / 7.55 / 1.83 / 79.28, value 47.78 / 37.94 / 11.34 (inside, live, dead); 117 rows dead in both columns, 490 value-dead,
    7 dead in all three."""
    if "S" in _cache:
        return _cache["S"]
    torch = _torch()
    g, pols = _env()
    pol = pols[0][0]
    tr = g.ppo_trainer(0)
    tr.advantages()
    X, f, _, _ = _rows(g, pols, 0)
    S = SimpleNamespace(g=g, pols=pols, pol=pol, tr=tr, f=f, n=X.shape[0])
    S.Xn = PR.normalise(X, pol.norm_mean, pol.norm_std)
    S.adv, S.v_old, S.ret = tr.read("adv"), tr.read("v_old"), tr.read("ret")
    S.flat = _perturb(tr, torch, S_NOISE, 11)
    S.terms = _terms(S, S.adv)
    S.cl = PR.classify(S.terms, S.adv, EPS, MARGIN)
    n, dec, pc, vc = S.n, S.cl["decided"], S.cl["policy"], S.cl["value"]
    S.decided = np.nonzero(dec)[0]
    shares = [np.bincount(pc[dec, q], minlength=5) / n for q in (0, 1)] + [np.bincount(vc[dec], minlength=3) / n]
    S.dead_pi = np.nonzero(dec & np.isin(pc, PR.POLICY_DEAD).all(1))[0]
    S.dead_v = np.nonzero(dec & (vc == PR.V_DEAD))[0]
    S.dead_all = np.intersect1d(S.dead_pi, S.dead_v)
    print("branch set-up: s %g eps %g: undecided %.2f %%; shares of n (decided rows) continuous %s discrete %s value %s; dead in both columns %d, "
          "value-dead %d, dead in all three %d" % (S_NOISE, EPS, 100.0 * (n - S.decided.size) / n, np.round(100 * shares[0], 2), np.round(100 * shares[1], 2),
                                                  np.round(100 * shares[2], 2), S.dead_pi.size, S.dead_v.size, S.dead_all.size))
    assert n == 4320 and n - S.decided.size <= 0.10 * n
    for sh in shares:
        assert sh.min() >= 0.01, shares
    assert S.dead_pi.size >= 16 and S.dead_v.size >= 16 and S.dead_all.size >= 2
    assert np.abs(S.terms["dv"]).min() > 0.0
    _cache["S"] = S
    return S


def _grad_check(S, ids, beta, adv=None, what=""):
    """one minibatch of the rows ids (an id >= n inserted: skipped) -> (stats, restatement stats, {tensor: relative error}); asserts the bounds"""
    torch = _torch()
    adv = S.adv if adv is None else adv
    ids = np.asarray(ids)
    dev_ids = np.concatenate([ids[: ids.size // 2], [S.n + 7], ids[ids.size // 2:]]).astype(np.int32)
    st = S.tr.minibatch(_ids(torch, dev_ids), EPS, beta)
    assert st["skipped"] == 1.0
    ap, cp, ref = _restate_grad(S.tr, S.pol, S.Xn, S.f, adv, S.v_old, S.ret, ids, EPS, beta, S.flat)
    gd = S.tr.read("grad")
    errs = {}
    for net, got, want in (("actor", S.tr.actor_params(gd), ap), ("critic", S.tr.critic_params(gd), cp)):
        dif = sum(np.sum((got[k].astype(np.float64) - want[k].grad.numpy()) ** 2) for k in want) ** 0.5
        ref_n = sum(np.sum(want[k].grad.numpy() ** 2) for k in want) ** 0.5
        errs[net] = dif / max(ref_n, 1e-30)
        for name in want:
            gr = want[name].grad.numpy()
            errs[net + "." + name] = np.linalg.norm(got[name].astype(np.float64) - gr) / max(np.linalg.norm(gr), 1e-30)
    print("%s m %d: %s" % (what, ids.size, " ".join("%s %.2g" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e <= (TOL_B_MU if k == "actor.b_mu" else TOL), (what, ids.size, k, e)
    return st, ref, errs


def test_heads_and_stats_off_the_tie_point():
    torch = _torch()
    S = _branches()
    ids, n = S.decided, S.n
    m = ids.size
    st = S.tr.minibatch(_ids(torch, np.concatenate([ids, [n + 3]])), EPS, BETA)
    assert st["skipped"] == 1.0
    for name, ref in (("mb_mu", S.terms["mu"]), ("mb_logits", S.terms["logits"]), ("mb_value", S.terms["v"])):
        got = S.tr.read(name).reshape((m + 1,) + ref.shape[1:])[:m]
        err, bound = np.abs(got - ref[ids]).max(), 1e-5 * max(1.0, np.abs(ref[ids]).max())
        print("%s: max error %.3g (bound %.3g)" % (name, err, bound))
        assert err <= bound, name
    _, _, ref = _restate_grad(S.tr, S.pol, S.Xn, S.f, S.adv, S.v_old, S.ret, ids, EPS, BETA, S.flat)
    count = int((S.cl["policy"][ids] != PR.INSIDE).sum())
    x = st["clip_fraction"] * 2 * m
    print("clipped columns: device %.6f restatement %d of %d; stats %s; restatement %s" % (x, count, 2 * m, st, ref))
    assert count > 0 and round(x) == count and abs(x - count) <= 1e-6 * count
    assert round(ref["clip_fraction"] * 2 * m) == count
    for k in ("L_pi", "L_v", "entropy", "approx_kl"):
        assert abs(st[k] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-6, (k, st[k], ref[k])
    assert st["approx_kl"] != 0.0 and abs(ref["approx_kl"]) > 1e-3


def test_gradients_off_the_tie_point():
    """GRAD of both networks against autograd, per tensor, on minibatches of decided rows: m = 1, 63, 64, 65, all (4 193) in a shuffled order,
    and per class up to 64 rows of that class only.  Measured worst relative errors (MI355X): actor W / b / heads <= 1.1e-5, log_sigma
    5.1e-5, b_mu 9.4e-5 (all rows; bound 5e-3), critic <= 9.2e-6 and 3.9e-5 for its b_mu — every tensor inside the bounds of the tie point,
    none had to be reset from a float32 restatement."""
    S = _branches()
    rng = np.random.default_rng(6)
    order = rng.permutation(S.decided)
    worst = {}
    batches = [("shuffled", order[:m]) for m in (1, 63, 64, 65, order.size)]
    dec = S.cl["decided"]
    for q, col in enumerate(("continuous", "discrete")):
        for c in range(5):
            batches.append(("%s class %d" % (col, c), rng.permutation(np.nonzero(dec & (S.cl["policy"][:, q] == c))[0])[:64]))
    for c in range(3):
        batches.append(("value class %d" % c, rng.permutation(np.nonzero(dec & (S.cl["value"] == c))[0])[:64]))
    for what, ids in batches:
        assert ids.size >= 1
        st, ref, errs = _grad_check(S, ids, BETA, what=what)
        for k in ("L_pi", "L_v", "entropy", "approx_kl", "clip_fraction"):
            assert abs(st[k] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-6, (what, k, st[k], ref[k])
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    print("worst relative gradient errors off the tie point: %s" % " ".join("%s %.2g" % kv for kv in sorted(worst.items())))


def _all_zero_bits(a):
    return not (np.ascontiguousarray(a, np.float32).view(np.uint32) & 0x7FFFFFFF).any()


def test_dead_rows_give_exact_zeros():
    torch = _torch()
    S = _branches()
    tr, na = S.tr, S.tr.n_actor
    # dead in both policy columns, beta 0: the actor's gradient is +-0 bit for bit (log_sigma included); the critic's is not
    tr.minibatch(_ids(torch, S.dead_pi), EPS, 0.0, stats=False)
    gd = tr.read("grad")
    assert _all_zero_bits(gd[:na]) and gd[na:].any()
    # value-dead rows: the critic's gradient is +-0; the actor's is not
    tr.minibatch(_ids(torch, S.dead_v), EPS, 0.0, stats=False)
    gd = tr.read("grad")
    assert _all_zero_bits(gd[na:]) and gd[:na].any()
    # dead in all three: GRAD is +-0, and Adam on it moves nothing
    tr.minibatch(_ids(torch, S.dead_all), EPS, 0.0, stats=False)
    assert _all_zero_bits(tr.read("grad"))
    tr.adam(3e-4)
    assert_bits_equal(tr.read("params"), S.flat, "PARAMS after Adam on a zero gradient")
    assert _all_zero_bits(tr.read("adam_m")) and _all_zero_bits(tr.read("adam_v"))
    # the first minibatch again with beta 5e-3: what is left of the actor's gradient is the entropy's
    ids = S.dead_pi
    tr.minibatch(_ids(torch, ids), EPS, BETA, stats=False)
    got = tr.actor_params(tr.read("grad"))
    ap = PR.tensors(tr.actor_params(S.flat), True)
    H = PR.entropy(ap, len(S.pol.W), S.Xn[ids])
    (-BETA * H.mean()).backward()
    assert _all_zero_bits(got["W_mu"]) and _all_zero_bits(got["b_mu"])          # (the entropy does not depend on mu)
    tot = 0.0
    for name, p in ap.items():
        gr = np.zeros(p.shape) if p.grad is None else p.grad.numpy()
        err = np.linalg.norm(got[name].astype(np.float64) - gr) / max(np.linalg.norm(gr), 1e-30)
        print("entropy gradient %s: relative error %.2g" % (name, err))
        assert err <= (TOL_B_MU if name == "b_mu" else TOL), (name, err)
        tot += np.linalg.norm(gr)
    assert tot > 0.0


def test_flipped_advantages_swap_live_and_dead():
    """the same rows with ADV negated (through views()["adv"]): what was live is dead and the gradient matches autograd again — a test of
    the branches that passes because one sign of A dominates the rollout would fail here"""
    torch = _torch()
    S = _branches()
    cl = PR.classify(S.terms, -S.adv, EPS, MARGIN)
    swap = np.array([PR.BELOW_DEAD, PR.BELOW_LIVE, PR.ABOVE_LIVE, PR.ABOVE_DEAD, PR.INSIDE])
    assert np.array_equal(cl["policy"], swap[S.cl["policy"]]) and np.array_equal(cl["decided"], S.cl["decided"])
    assert np.array_equal(cl["value"], S.cl["value"])
    live_now = S.dead_pi
    adv_view = S.tr.views()["adv"]
    try:
        adv_view.neg_()
        torch.cuda.synchronize()
        assert_bits_equal(S.tr.read("adv"), -S.adv, "ADV negated")
        order = np.random.default_rng(8).permutation(S.decided)
        for what, ids in (("flipped", order), ("flipped", order[:65]), ("flipped, was dead in both columns", live_now)):
            st, ref, _ = _grad_check(S, ids, BETA, adv=-S.adv, what=what)
            for k in ("L_pi", "L_v", "entropy", "approx_kl", "clip_fraction"):
                assert abs(st[k] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-6, (what, k, st[k], ref[k])
        # rows that were dead in both columns are live in both now; rows that are dead in both now were live
        S.tr.minibatch(_ids(torch, live_now), EPS, 0.0, stats=False)
        assert S.tr.read("grad")[:S.tr.n_actor].any()
        dead_now = np.nonzero(cl["decided"] & np.isin(cl["policy"], PR.POLICY_DEAD).all(1))[0]
        assert dead_now.size >= 1 and not np.intersect1d(dead_now, live_now).size
        S.tr.minibatch(_ids(torch, dead_now), EPS, 0.0, stats=False)
        assert _all_zero_bits(S.tr.read("grad")[:S.tr.n_actor])
    finally:
        adv_view.neg_()
        torch.cuda.synchronize()
    assert_bits_equal(S.tr.read("adv"), S.adv, "ADV restored")


# ---------------------------------------------------------------------------------------------------------------------
# The gather, the shapes and the critic off the easy path.  A handle of 8 envs whose two actors are (stack, hidden, layers, normaliser);
# the trained one and its critic (hidden, layers; None: the actor's shape).  Episodes time out after 100 ticks (hk_create takes no less).
# 58 ticks, a reset of envs 0 .. 3 alone, then 37 + 1 ticks (37 is mid-interval: a rollout begins on a decision, a multiple of the
# decision period 2): the rollout begins on step 38 of envs 0 .. 3' episode and step 96 of the others', so that the others time out in
# interval 1 (FIRST on row 2: a clear that hides live RING0 entries) and envs 0 .. 3 in interval 30 (FIRST on row 31 = R - 1: the
# bootstrap input follows a late clear).
PRE_TICKS, RESET_ENVS, R_SHAPES = 58, [0, 1, 2, 3], 32
SHAPES = {
    # stack 8 = smax at 4 agents (K = 624), hidden 32 (half a tile) x 4 layers
    "stack8_h32x4": dict(agents=4, actors=[(8, 32, 4, True), (2, 96, 2, True)], train=0, critic=None),
    # stack 2 under smax 8 (K = 156), hidden 96 x 2 layers, a 32 x 1 critic
    "stack2_of_8_h96x2": dict(agents=4, actors=[(8, 32, 4, True), (2, 96, 2, True)], train=1, critic=(32, 1)),
    # stack 1 under smax 4 (K = 78), one layer, no normaliser, a 256 x 3 critic under the 32 x 1 actor
    "stack1_of_4_h32x1": dict(agents=4, actors=[(1, 32, 1, False), (4, 256, 3, True)], train=0, critic=(256, 3)),
    # a 64 x 2 critic under the 256 x 3 actor (stack 4 beside the stack-1 actor)
    "stack4_h256x3_critic64x2": dict(agents=4, actors=[(1, 32, 1, False), (4, 256, 3, True)], train=1, critic=(64, 2)),
    # a 2-agent handle, stack 2 (K = 108)
    "two_agents_stack2": dict(agents=2, actors=[(2, 96, 2, True), (2, 64, 1, True)], train=0, critic=None),
}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_gather_shapes_and_critic(case):
    import hierarchicalkarting_amd as hk
    torch = _torch()
    c = SHAPES[case]
    E, A, R = 8, c["agents"], R_SHAPES
    g = hk.RacingEnv(hk.make_config(E, A, low_mode=[RL] * A, rewards=1, max_episode_steps=100, jitter_seed=4))
    g.reset()
    half = A // 2
    pols = []
    for k, (stack, hidden, layers, norm) in enumerate(c["actors"]):
        pol = Policy.random(g.obs_dim * stack, hidden, layers, stack=stack, seed=21 + k, normalize=norm)
        slots = list(range(k * half, (k + 1) * half))
        assert g.attach_policy(pol, slots, P) == k
        pols.append((pol, slots))
    g.step(PRE_TICKS)
    g.reset(RESET_ENVS)
    g.step(37 + 1)
    g.rollout_begin(R)
    g.step(R * P)
    g.rollout_close()
    p = c["train"]
    pol, slots = pols[p]
    stack, S = pol.stack, len(slots)
    smax = max(q.stack for q, _ in pols)
    n = R * E * S
    X, f, boot, ro = _rows(g, pols, p)
    # ---- the rollout is the one this test is about
    first = ro["first"][:, :, slots]
    assert ro["ring0"].shape[2] == smax - 1 and ro["ring0"].any() and (ro["done"] != 0).any()
    if stack > 1:
        assert all(ro["ring0"][:, a, smax - stack:].any() for a in slots), "RING0 of the driven slots"
    if stack > 2:           # (a clear on a row t >= stack - 1 finds no RING0 entry left in the stack)
        assert first[1:stack - 1].any(), "no clear that hides live RING0 entries"
    if stack > 1:           # (a stack of 1 holds nothing a clear could remove)
        assert first[R - (stack - 1):].any() and not (ro["done"][R - 1] != 0).all(), "no late clear ahead of a bootstrap that is used"
    # ---- unchanged parameters, fp32: the training forward is the recorded one bit for bit
    cr = c["critic"]
    critic = None if cr is None else Policy.random(pol.in_dim, cr[0], cr[1], n_branch=1, stack=stack, seed=77, normalize=False)
    tr = g.ppo_trainer(p, critic=critic, normalize_advantages=True, gamma=0.99, lambd=0.95)
    assert tr.precision == "f32"
    tr.advantages()
    st = tr.minibatch(_ids(torch, np.arange(n)), EPS, BETA)
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0 and st["skipped"] == 0.0, st
    assert_bits_equal(tr.read("mb_mu"), f["mu"], case + " mu")
    assert_bits_equal(tr.read("mb_logits").reshape(n, -1), f["logits"], case + " logits")
    # eps 0 at unchanged parameters: rho == 1 == lo == hi, inside the inclusive band — no column counts as clipped
    st = tr.minibatch(_ids(torch, np.arange(n)), 0.0, BETA)
    assert st["approx_kl"] == 0.0 and st["clip_fraction"] == 0.0, st
    # ---- the critic and GAE on the host's stacked inputs
    Lc = len(tr.critic_policy.W)
    cp = PR.tensors(tr.critic_params())
    Xn = PR.normalise(X, pol.norm_mean, pol.norm_std)
    v_ref = PR.critic_values(Xn, cp, Lc).numpy()
    bound = 1e-5 * max(1.0, np.abs(v_ref).max())
    v_dev = tr.read("v_old")
    assert np.abs(tr.read("mb_value") - v_ref).max() <= bound and np.abs(v_dev - v_ref).max() <= bound
    vb = PR.critic_values(PR.normalise(boot, pol.norm_mean, pol.norm_std), cp, Lc).numpy()
    Adv, RET = PR.gae(f["r"], f["done"], v_dev.reshape(R, E, S), vb.reshape(E, S), 0.99, 0.95)
    for name, ref in (("adv", PR.normalise_adv(Adv)), ("ret", RET)):
        err = np.abs(tr.read(name).reshape(ref.shape) - ref).max()
        print("%s %s: max error %.3g (bound %.3g)" % (case, name, err, 1e-5 * max(1.0, np.abs(ref).max())))
        assert err <= 1e-5 * max(1.0, np.abs(ref).max()), name
    # ---- one gradient: the fp32 product kernel at this case's N and K in its three epilogues
    Sx = SimpleNamespace(tr=tr, pol=pol, Xn=Xn, f=f, n=n, adv=tr.read("adv"), v_old=v_dev, ret=tr.read("ret"), flat=tr.read("params"))
    _grad_check(Sx, np.random.default_rng(9).permutation(n)[:65], BETA, what=case)


# ---------------------------------------------------------------------------------------------------------------------
def test_update_is_its_minibatches_issued_by_hand():
    import hierarchicalkarting_amd as hk
    torch = _torch()
    g, pols = _env()
    seed, lr, mb = 13, 3e-4, 512
    t1, t2 = g.ppo_trainer(0, seed=seed), g.ppo_trainer(0, seed=seed)
    for t in (t1, t2):
        t.advantages()
    n = t1.read("adv").size
    nmb = n // mb
    assert n == 4320 and nmb == 8 and n - nmb * mb == 224
    s1 = t1.update(2, mb, lr, EPS, BETA)
    assert np.array_equal(t1.read("perm"), permutation(n, seed, 1))
    x = np.random.default_rng(3).standard_normal((300, pols[0][0].in_dim)).astype(np.float32) * 2
    mu1, lg1 = g.policy_forward(0, x)
    fed = []
    for c in (0, 1):
        perm = permutation(n, seed, c)
        hist = []
        for b in range(nmb):
            ids = perm[mb * b: mb * (b + 1)]
            fed.append(ids)
            hist.append(t2.minibatch(_ids(torch, ids), EPS, BETA))
            t2.adam(lr)
    t2.publish()
    assert len(fed) == 2 * nmb and all(np.unique(np.concatenate(fed[e * nmb:(e + 1) * nmb])).size == nmb * mb for e in (0, 1))
    for name in ("params", "adam_m", "adam_v"):
        assert_bits_equal(t1.read(name), t2.read(name), "%s: update against its minibatches by hand" % name)
    # the stats: the mean over the last epoch's minibatches, averaged in fp64 and rounded once
    for k in s1:
        mean = float(np.mean([np.float64(h[k]) for h in hist]))
        ulp = float(np.spacing(np.float32(abs(mean))))
        print("update stat %s: %.9g against the mean %.9g of %s (%.2f ulp)" % (k, s1[k], mean, [h[k] for h in hist], abs(s1[k] - mean) / ulp))
        assert abs(s1[k] - mean) <= ulp, (k, s1[k], mean)
    # publish: the handle acts with t1's weights after update(), and they are what a fresh handle computes with actor() attached
    h = hk.RacingEnv(hk.make_config(24, 4, **KW))
    h.reset()
    h.attach_policy(t2.actor(), [0, 1], P)
    mu_h, lg_h = h.policy_forward(0, x)
    assert not np.array_equal(t2.actor().W[0], pols[0][0].W[0])
    for what, (mu, lg) in (("after update()", (mu1, lg1)), ("after publish()", g.policy_forward(0, x))):
        assert_bits_equal(mu, mu_h, "mu " + what)
        assert_bits_equal(lg, lg_h, "logits " + what)
    # a minibatch size beyond n: one minibatch of all n rows, in the order of the trainer's next epoch (its third: count 2)
    t1.update(1, 10 ** 6, lr, EPS, BETA)
    perm = permutation(n, seed, 2)
    assert np.array_equal(t1.read("perm"), perm)
    t2.minibatch(_ids(torch, perm), EPS, BETA, stats=False)
    t2.adam(lr)
    for name in ("params", "adam_m", "adam_v"):
        assert_bits_equal(t1.read(name), t2.read(name), "%s: one minibatch of n rows" % name)
