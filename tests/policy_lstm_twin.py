"""Build and run the host twin of policy_lstm_kernel (tests/policy_lstm_host_check.cpp): the bit reference of a recurrent actor.
Test infrastructure shared by tests/test_policy_lstm_cpu.py and tests/test_policy_lstm_gpu.py; nothing is preloaded, the sanitizers are
linked into the stand-alone program."""
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


def sweep():
    """the twin's --sweep -> dict name -> float"""
    out = subprocess.check_output([build(True), "--sweep"], text=True)
    return {k: float(v) for k, v in (ln.split() for ln in out.splitlines() if ln.strip())}
