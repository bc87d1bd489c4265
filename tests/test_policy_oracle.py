"""RL low-level policy, CPU side: the ONNX reader and the oracle's actor are checked against an INDEPENDENT
evaluation of the exported graph (a small numpy interpreter of the ONNX node list, float64), on the reference's own
trained actors (the arrays of tests/golden/reference_actors.npz and reference_actor_312.npz, written as mlagents-learn
exports them by tests/onnx_write.py) and on synthetic actors; plus the runtime pieces around the actor (StackingSensor
order, zero fill after a reset, DecisionPeriod, action repeat)."""
import os
import numpy as np
import pytest
import oracle_lib as O
import onnx_write
from hierarchicalkarting_amd import _lib, onnx_read
from hierarchicalkarting_amd.config import make_config
from hierarchicalkarting_amd.policy import Policy

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAINED = ["HierarchicalAgent-Team-allscaledown14.onnx", "HierarchicalAgent-NonLSTM-allsolo6.onnx", "FixedHierarchicalAgent-NonLSTM-allsolo10.onnx",
           "HierarchicalAgent-TeamDOE-all28.onnx", "FixedHierarchicalAgent-Team-all33.onnx"]


def run_graph(model, obs, deterministic=True):
    """interpret the exported graph node by node in float64 (only the deterministic outputs: no random ops)"""
    v = {k: a.astype(np.float64) for k, a in model["init"].items()}
    v["obs_0"] = obs.astype(np.float64)
    v["action_masks"] = np.ones((obs.shape[0], 3))
    for n in model["nodes"]:
        i = [v.get(x) for x in n["in"]]
        op, a = n["op"], n["attr"]
        if op in ("RandomNormalLike", "Multinomial"):
            v[n["out"][0]] = None
            continue
        if any(x is None for x in i):
            v[n["out"][0]] = None
            continue
        if op == "Sub": r = i[0] - i[1]
        elif op == "Add": r = i[0] + i[1]
        elif op == "Mul": r = i[0] * i[1]
        elif op == "Div": r = i[0] / i[1]
        elif op == "Clip": r = np.clip(i[0], a["min"], a["max"])
        elif op == "Concat": r = np.concatenate(i, axis=a["axis"])
        elif op == "Gemm": r = a.get("alpha", 1.0) * (i[0] @ (i[1].T if a.get("transB") else i[1])) + a.get("beta", 1.0) * i[2]
        elif op == "Sigmoid": r = 1.0 / (1.0 + np.exp(-i[0]))
        elif op == "Constant": r = np.asarray(a["value"], np.float64)
        elif op == "Exp": r = np.exp(i[0])
        elif op == "Log": r = np.log(i[0])
        elif op == "Slice": r = i[0][:, a["starts"][0]:a["ends"][0]]
        elif op == "Softmax":
            e = np.exp(i[0] - i[0].max(axis=1, keepdims=True)); r = e / e.sum(axis=1, keepdims=True)
        elif op == "ArgMax": r = np.argmax(i[0], axis=a["axis"]).reshape(-1, 1)
        else: raise AssertionError("op " + op)
        v[n["out"][0]] = r
    return v


def _oracle_env(A, low_mode):
    b = make_config(3, A, low_mode=low_mode, jitter_seed=11)
    o = O.OracleEnv(b)
    o.reset()
    return o, b


def _trained(pattern):
    """a trained actor of the reference, from the arrays the repository carries"""
    for f in ("reference_actors.npz", "reference_actor_312.npz"):
        d = np.load(os.path.join(GOLD, f))
        if pattern + "/W0" in d:
            return Policy.from_arrays(d, pattern + "/")
    raise KeyError(pattern)


@pytest.mark.parametrize("pattern,A", [("HierarchicalAgent-Team-allscaledown14.onnx", 4), ("HierarchicalAgent-NonLSTM-allsolo6.onnx", 2),
                                       ("FixedHierarchicalAgent-NonLSTM-allsolo10.onnx", 2), ("HierarchicalAgent-TeamDOE-all28.onnx", 4),
                                       ("FixedHierarchicalAgent-Team-all33.onnx", 4)])
def test_reference_models_through_the_oracle(pattern, A, tmp_path):
    src = _trained(pattern)
    path = onnx_write.write_actor(str(tmp_path / pattern), src)
    model = onnx_read.load(path)
    o, b = _oracle_env(A, [_lib.HK_LOW_RL] * A)
    in_dim = model["inputs"][0][1][1]
    assert in_dim % o.obs_dim == 0 and in_dim // o.obs_dim in (4, 8)      # trained on this observation layout, 4 or 8 stacked
    pol = Policy.from_onnx(path, stack=in_dim // o.obs_dim, deterministic=True)
    assert all(np.array_equal(pol.arrays()[k], v) for k, v in src.arrays().items())        # every array read back bit for bit
    idx = o.attach_policy(pol, list(range(A)), 2)
    r = np.random.default_rng(5)
    obs = (r.standard_normal((64, pol.in_dim)) * 3.0 + pol.norm_mean).astype(np.float32)
    mu, lg = o.policy_forward(idx, obs)
    v = run_graph(model, obs)
    mu_name = [n for n in model["nodes"] if n["op"] == "Gemm" and "mu.weight" in n["in"][1]][0]["out"][0]
    lg_name = [n for n in model["nodes"] if n["op"] == "Gemm" and "branches.0.weight" in n["in"][1]][0]["out"][0]
    assert np.abs(mu - v[mu_name][:, 0]).max() < 2e-5
    assert np.abs(lg - v[lg_name]).max() < 2e-5
    # deterministic outputs of the graph = what the oracle latches as actions
    det_c = v["deterministic_continuous_actions"][:, 0]
    assert np.abs(np.clip(mu, -3, 3) / 3 - det_c).max() < 1e-5
    assert (v["deterministic_discrete_actions"][:, 0] == np.argmax(lg, axis=1)).all()


def test_every_reference_hka_model_parses(tmp_path):
    """every trained actor the repository carries, exported and read back"""
    n = 0
    for m in TRAINED:
        pol = Policy.from_onnx(onnx_write.write_actor(str(tmp_path / m), _trained(m)))
        assert pol.in_dim in (212, 216, 312, 624) and pol.hidden in (128, 256) and pol.n_branch == 3 and len(pol.W) in (2, 3)
        assert pol.norm_std.min() > 0
        n += 1
    assert n == len(TRAINED)


@pytest.mark.parametrize("in_dim,hidden,layers,A", [(216, 128, 3, 2), (312, 256, 3, 4), (216, 64, 1, 2)])
def test_oracle_actor_vs_float64(in_dim, hidden, layers, A):
    pol = Policy.random(in_dim, hidden, layers, seed=in_dim + hidden)
    o, b = _oracle_env(A, [_lib.HK_LOW_RL] * A)
    idx = o.attach_policy(pol, [0], 2)
    r = np.random.default_rng(1)
    obs = r.standard_normal((33, in_dim)).astype(np.float32) * 4
    mu, lg = o.policy_forward(idx, obs)
    x = np.clip((obs.astype(np.float64) - pol.norm_mean) / pol.norm_std, -5, 5)
    for W, bb in zip(pol.W, pol.b):
        s = x @ W.T.astype(np.float64) + bb
        x = s / (1 + np.exp(-s))
    assert np.abs(mu - (x @ pol.W_mu.astype(np.float64) + pol.b_mu)).max() < 1e-4
    assert np.abs(lg - (x @ pol.W_branch.T.astype(np.float64) + pol.b_branch)).max() < 1e-4


def test_stacking_decision_period_and_reset():
    A = 2
    pol = Policy.random(54 * 4, 64, 2, seed=3, deterministic=True)
    o, b = _oracle_env(A, [_lib.HK_LOW_RL, _lib.HK_LOW_LQR])
    idx = o.attach_policy(pol, [0], 2)
    hist = []
    acts = []
    for t in range(9):
        if t % 2 == 0:                      # decision ticks: the Academy observes BEFORE the tick's scripts run
            hist.append(o.observations()[:, 0].copy())
        o.step(1)
        acts.append(o.get_actions()[0][:, 0].copy())
        if t % 2 == 1:
            assert (acts[-1] == acts[-2]).all()          # repeated between decisions
        # expected stacked input: last 4 decision observations, oldest first, zeros before the first
        k = len(hist)
        st = np.zeros((o.E, 4, 54), np.float32)
        for i in range(min(k, 4)):
            st[:, 3 - i] = hist[k - 1 - i]
        mu, _ = o.policy_forward(idx, st.reshape(o.E, -1))
        assert (acts[-1] == np.clip(mu, -3, 3) / np.float32(3)).all(), t
    # LQ agent's action slots are never written by the policy
    assert (o.get_actions()[0][:, 1] == 0).all()
    # an explicit reset clears the stack: the next decision sees one fresh observation and three zero slots
    o.reset()
    if o_academy(9) % 2 == 1:
        o.step(1)                                         # tick 9 is not a decision tick (the Academy keeps counting)
    fresh = o.observations()[:, 0].copy()
    o.step(1)
    st = np.zeros((o.E, 4, 54), np.float32)
    st[:, 3] = fresh
    mu, _ = o.policy_forward(idx, st.reshape(o.E, -1))
    assert (o.get_actions()[0][:, 0] == np.clip(mu, -3, 3) / np.float32(3)).all()


def o_academy(ticks_so_far):
    return ticks_so_far


def test_sampling_statistics():
    A = 2
    pol = Policy.random(54 * 4, 64, 2, seed=9)
    b = make_config(512, A, low_mode=[_lib.HK_LOW_RL] * A, jitter_seed=3)
    o = O.OracleEnv(b)
    o.reset()
    idx = o.attach_policy(pol, [0, 1], 2)
    steer_all = []; br_all = []; mu_all = []; p_all = []
    for _ in range(3):
        obs = o.observations()
        o.step(2)
        s, br = o.get_actions()
        steer_all.append(s); br_all.append(br)
    s = np.concatenate(steer_all).ravel(); br = np.concatenate(br_all).ravel()
    assert np.abs(s).max() <= 1.0 and set(np.unique(br)) <= {0, 1, 2}
    assert len(np.unique(s)) > 0.9 * s.size              # continuous draws differ per agent / decision
    assert all((br == k).mean() > 0.02 for k in range(3)) # every branch is drawn
