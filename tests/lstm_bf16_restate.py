"""Restatement of the recurrent bf16 chain (include/hk.h "RECURRENT ACTORS IN BF16"), shared by tests/test_lstm_bf16_cpu.py and
tests/test_lstm_bf16_gpu.py.  It reuses ppo_bf16_restate's rounding (ppo.bf16_round, to nearest even) and bound (gamma).

gates_ref    the float64 sum over the SAME bf16 values with the bound the device is held to: 2 gamma_K sum |a| |b| + one ulp of the seed,
             K = Hpad + m (a bf16 x bf16 product is exact in fp32, so only the additions round: ppo_bf16_restate's argument, nothing new).
gates_steps  the chain step by step: the accumulator seeded with fp32(b_ih + b_hh), stepped over a padded with +0.0 to whole chunks of 64 (every
             step issued, the all-zero ones included), then over h in m / 16 whole steps; a step adds the float64 sum of its 16 exact products and
             rounds to fp32 once.  How the matrix instruction orders the additions inside a step is not modelled, so this is bit-exact only where
             every step's sum is exactly representable — the hand cases of the CPU test — and the device is compared with gates_ref, not with it.
cell         hk_lstm_cell through a host build of the kernels' own definition (tests/lstm_cell_host_check.cpp, policy_lstm_twin's flags).
step         one decision from the trunk's last post-activation on: the rounding points of the contract, FIRST zeroing, gates_steps, cell.
compose      the device chain composed from the trainer's taps (ppo.gemm_bf16 epi 1, ppo.lstm_gates_bf16), the host cell and the host heads:
             the bit reference of policy_forward in bf16."""
import os
import subprocess
import tempfile

import numpy as np

import policy_bf16_restate as PB
from ppo_bf16_restate import gamma, ulp32
from hierarchicalkarting_amd.ppo import bf16_round, bf16_value

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lstm_cell_host_check.cpp")
MAGIC = 0x4C43454C
_exe = {}


def pad64(k):
    return (int(k) + 63) & ~63


def bsum(b_ih, b_hh):
    """fp32(b_ih + b_hh), as policy_lstm_upload and ppo_lstm_bsum_kernel form it"""
    return (np.asarray(b_ih, np.float32) + np.asarray(b_hh, np.float32)).astype(np.float32)


def gates_ref(a, h, W_ih, W_hh, bs):
    """-> (reference, tolerance), float64 [rows, 4m], of the gate pre-activations on bf16 bit patterns a [rows, H], h [rows, m], W_ih [4m, H],
    W_hh [4m, m] and the fp32 seed bs [4m]"""
    av, hv, wi, wh = (bf16_value(x).astype(np.float64) for x in (a, h, W_ih, W_hh))
    seed = np.asarray(bs, np.float32).astype(np.float64)[None, :]
    K = pad64(av.shape[1]) + hv.shape[1]
    ref = seed + av @ wi.T + hv @ wh.T
    tol = 2.0 * gamma(K) * (np.abs(av) @ np.abs(wi).T + np.abs(hv) @ np.abs(wh).T) + ulp32(np.broadcast_to(seed, ref.shape))
    return ref, tol


def gates_steps(a, h, W_ih, W_hh, bs):
    """the chain step by step -> (z float32 [rows, 4m], number of steps issued)"""
    av, hv, wi, wh = (bf16_value(x).astype(np.float64) for x in (a, h, W_ih, W_hh))
    rows, H = av.shape
    m = hv.shape[1]
    Hp = pad64(H)
    ap = np.zeros((rows, Hp)); ap[:, :H] = av                    # +0.0 padding of the 64-wide chunks
    wp = np.zeros((wi.shape[0], Hp)); wp[:, :H] = wi
    acc = np.repeat(np.asarray(bs, np.float32)[None, :], rows, axis=0)
    steps = 0
    for A, W, K in ((ap, wp, Hp), (hv, wh, m)):
        assert K % 16 == 0
        for s in range(0, K, 16):
            acc = (acc.astype(np.float64) + A[:, s:s + 16] @ W[:, s:s + 16].T).astype(np.float32)
            steps += 1
    return acc, steps


def build(sanitize=True):
    """-> path of the compiled host cell (once per process; policy_lstm_twin.build's flags)"""
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="hk_lstm_cell_")
        exe = os.path.join(d, "lstm_cell_host_check")
        cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread"]
        if sanitize:
            cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call(cmd + [SRC, "-o", exe])
        _exe[sanitize] = exe
    return _exe[sanitize]


def cell(z, c, sanitize=True):
    """hk_lstm_cell on z [rows, 4m] (gates i f g o) and c [rows, m] -> (h' [rows, m], c' [rows, m]), float32"""
    z, c = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(c, np.float32)
    rows, m = c.shape
    assert z.shape == (rows, 4 * m)
    with tempfile.TemporaryDirectory() as d:
        cin, cout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(cin, "wb") as fh:
            fh.write(np.array([MAGIC, rows, m], "<i4").tobytes() + z.tobytes() + c.tobytes())
        subprocess.check_call([build(sanitize), cin, cout])
        out = np.fromfile(cout, "<f4")
    assert out.size == 2 * rows * m
    return out[:rows * m].reshape(rows, m).copy(), out[rows * m:].reshape(rows, m).copy()


def step(a_f32, mem, first, W_ih, W_hh, b_ih, b_hh):
    """one decision from the trunk's last fp32 post-activation a_f32 [rows, H] on: a rounded once, the fp32 weights rounded once, h rounded once
    where it is an operand, h and c exactly zero where first, the seed fp32(b_ih + b_hh), the cell fp32 on the fp32 c -> (h', c', operands)"""
    mem = np.asarray(mem, np.float32)
    m = mem.shape[1] // 2
    h = np.where(np.asarray(first, bool)[:, None], np.float32(0), mem[:, :m])
    c = np.where(np.asarray(first, bool)[:, None], np.float32(0), mem[:, m:])
    ops = dict(a=bf16_round(a_f32), h=bf16_round(h), W_ih=bf16_round(W_ih), W_hh=bf16_round(W_hh), bsum=bsum(b_ih, b_hh))
    z, _ = gates_steps(ops["a"], ops["h"], ops["W_ih"], ops["W_hh"], ops["bsum"])
    hn, cn = cell(z, c)
    return hn, cn, ops


def compose(env, pol, obs, mem):
    """policy_forward of a recurrent Policy in bf16, composed: the trunk through ppo.gemm_bf16 epi 1 as policy_bf16_restate composes it with the
    LAST post-activation rounded too, the gates through ppo.lstm_gates_bf16, the cell on the host, the heads by the host tail
    -> (mu [rows], logits [rows, nb], memory_out [rows, 2m])"""
    from hierarchicalkarting_amd import ppo
    obs = np.asarray(obs, np.float32).reshape(-1, pol.in_dim)
    m = pol.memory_size // 2
    mem = np.zeros((obs.shape[0], 2 * m), np.float32) if mem is None else np.asarray(mem, np.float32).reshape(obs.shape[0], 2 * m)
    X = bf16_round(PB.normalise(obs, pol.norm_mean, pol.norm_std))
    for W, b in zip(pol.W, pol.b):
        X = bf16_round(ppo.gemm_bf16(env, 1, X, bf16_round(W), np.asarray(b, np.float32)))
    ls = pol.lstm
    z = ppo.lstm_gates_bf16(env, X, bf16_round(mem[:, :m]), bf16_round(ls["W_ih"]), bf16_round(ls["W_hh"]), bsum(ls["b_ih"], ls["b_hh"]))
    hn, cn = cell(z, mem[:, m:])
    mu, lg = PB.heads(hn, pol.W_mu, pol.b_mu, pol.W_branch, pol.b_branch)
    return mu, lg, np.concatenate([hn, cn], axis=1)
