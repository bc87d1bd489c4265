"""Build and run the host twin of policy_lstm_kernel (tests/policy_lstm_host_check.cpp): the bit reference of a recurrent actor.
Test infrastructure shared by tests/test_policy_lstm_cpu.py, tests/test_policy_lstm_gpu.py and tests/test_policy_lstm_fields_gpu.py; nothing is
preloaded, the sanitizers are linked into the stand-alone program."""
import os
import subprocess
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "policy_lstm_host_check.cpp")
MAGIC = 0x4C53544D
_exe = {}


def build(sanitize=True):
    """-> path of the compiled twin (once per process, in a temporary directory that lives as long as the process)"""
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="hk_lstm_twin_")
        exe = os.path.join(d, "policy_lstm_host_check")
        cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread"]
        if sanitize:
            cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call(cmd + [SRC, "-o", exe])
        _exe[sanitize] = exe
    return _exe[sanitize]


def case_bytes(pol, obs, mem):
    """the twin's case file of a Policy with an LSTM, stacked inputs [rows, in_dim] and memory [rows, 2m]"""
    f = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    obs = np.ascontiguousarray(obs, np.float32).reshape(-1, pol.in_dim)
    m = pol.memory_size // 2
    mem = np.ascontiguousarray(mem, np.float32).reshape(obs.shape[0], 2 * m)
    out = [np.array([MAGIC, pol.in_dim, pol.hidden, len(pol.W), pol.n_branch, int(pol.norm_mean is not None), m, obs.shape[0]], "<i4").tobytes()]
    if pol.norm_mean is not None:
        out += [f(pol.norm_mean), f(pol.norm_std)]
    for W, b in zip(pol.W, pol.b):
        out += [f(W), f(b)]
    out += [f(pol.lstm[k]) for k in ("W_ih", "W_hh", "b_ih", "b_hh")]
    out += [f(pol.W_mu), f(pol.b_mu), f(pol.W_branch), f(pol.b_branch), f(obs), f(mem)]
    return b"".join(out)


def step(pol, obs, mem=None, sanitize=True):
    """one step of the twin -> (mu [rows], logits [rows, n_branch], memory_out [rows, 2m]); mem None: zeros"""
    obs = np.ascontiguousarray(obs, np.float32).reshape(-1, pol.in_dim)
    rows, nb, mm = obs.shape[0], pol.n_branch, pol.memory_size
    if mem is None:
        mem = np.zeros((rows, mm), np.float32)
    exe = build(sanitize)
    with tempfile.TemporaryDirectory() as d:
        cin, cout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(cin, "wb") as fh:
            fh.write(case_bytes(pol, obs, mem))
        subprocess.check_call([exe, cin, cout])
        a = np.fromfile(cout, "<f4")
    assert a.size == rows * (1 + nb + mm)
    return a[:rows].copy(), a[rows:rows * (1 + nb)].reshape(rows, nb).copy(), a[rows * (1 + nb):].reshape(rows, mm).copy()


# ---- what the GPU tests of both files share (tests/test_policy_lstm_gpu.py, tests/test_policy_lstm_fields_gpu.py)
def rl_env(E, A=2, **kw):
    """a reset field of E envs with A karts, every kart LowMode RL"""
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    kw.setdefault("low_mode", [_lib.HK_LOW_RL] * A)
    g = hk.RacingEnv(hk.make_config(E, A, **kw))
    g.reset()
    return g


def lstm_actor(D, seed=3, **kw):
    """the reference shape on a stack of 4 observations of width D: -> 128 x 3 -> m = 128"""
    from hierarchicalkarting_amd.policy import Policy
    return Policy.random(D * 4, 128, 3, 3, seed=seed, memory_size=256, **kw)


def replay(ro, pol, slots, tag):
    """every row of a recorded rollout from its stacked input and MEMORY[t] alone, through the twin; -> the twin's memory after the last row"""
    from hierarchicalkarting_amd.rollout import stacked_inputs
    from parity import assert_bits_equal
    R, E = ro["obs"].shape[:2]
    S, mm = len(slots), pol.memory_size
    x = stacked_inputs(ro, slots, pol.stack)
    first = ro["first"][:, :, slots]
    mem = ro["memory"][:, :, slots, :mm]
    zero = ~mem.any(axis=-1)
    assert np.array_equal(zero, first == 1), tag            # zero exactly where the episode starts
    out = None
    for t in range(R):
        mu, lg, out = step(pol, x[t].reshape(E * S, -1), mem[t].reshape(E * S, mm))
        assert_bits_equal(ro["mu"][t][:, slots].reshape(-1), mu, (tag, t, "mu"))
        assert_bits_equal(ro["logits"][t][:, slots, :pol.n_branch].reshape(E * S, -1), lg, (tag, t, "logits"))
        if t + 1 < R:
            keep = first[t + 1].reshape(-1) == 0
            assert_bits_equal(mem[t + 1].reshape(E * S, mm)[keep], out[keep], (tag, t, "memory chain"))
    return out.reshape(E, S, mm)


def sweep():
    """the twin's --sweep -> dict name -> float"""
    out = subprocess.check_output([build(True), "--sweep"], text=True)
    return {k: float(v) for k, v in (ln.split() for ln in out.splitlines() if ln.strip())}
