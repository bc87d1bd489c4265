"""The recurrent bf16 mode without a GPU (include/hk.h "RECURRENT ACTORS IN BF16"): the library exports the three new entry points
with the ctypes signatures hk.h declares, and the restatement the GPU tests lean on (tests/lstm_bf16_restate.py) is checked against hand cases:
the rounding points of the contract, the padding steps, the -0.0 seed and FIRST zeroing."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import lstm_bf16_restate as LB
from hierarchicalkarting_amd.ppo import bf16_round, bf16_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hk_policy_lstm_set_precision", "hk_ppo_recurrent_set_precision", "hk_ppo_lstm_gates_bf16")
CTYPE = {"hk_handle": C.c_void_p, "int": C.c_int, "const void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p}


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from hierarchicalkarting_amd import _lib
    return _lib


def test_new_entry_points_are_exported_with_the_declared_signatures(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hk.h")).read(), flags=re.S)
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name), "libhk.so does not export %s" % name
        mt = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert mt, "include/hk.h does not declare %s" % name
        want = []
        for arg in mt.group(1).split(","):
            ty = re.sub(r"\s*\*\s*", "* ", arg.strip()).rsplit(" ", 1)[0].strip()          # the type without the parameter's name
            want.append(CTYPE[ty])
        restype, argtypes = lib.SYMBOLS[name]
        assert restype is C.c_int
        got = [C.c_void_p if (t is lib._H or t is C.c_void_p or t is lib._fp) else t for t in argtypes]
        assert got == want, (name, argtypes)
    # ... and the Python surface that calls them
    from hierarchicalkarting_amd import ppo
    from hierarchicalkarting_amd.env import RacingEnv
    assert callable(RacingEnv.policy_lstm_set_precision) and callable(ppo.PPOTrainer.set_recurrent_precision) and callable(ppo.lstm_gates_bf16)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_padding_steps_and_step_count():
    # H = 32 is padded to one chunk of 64 (4 steps), H = 96 to 128 (8), then m / 16 whole steps: the steps issued, all-zero ones included
    for H, m, steps in ((32, 32, 4 + 2), (96, 96, 8 + 6), (128, 128, 8 + 8), (256, 64, 16 + 4)):
        z, n = LB.gates_steps(np.zeros((1, H), np.uint16), np.zeros((1, m), np.uint16), np.zeros((4 * m, H), np.uint16), np.zeros((4 * m, m), np.uint16),
                              np.zeros(4 * m, np.float32))
        assert n == steps and z.shape == (1, 4 * m) and not _bits(z).any()


def test_minus_zero_seed_with_all_zero_operands_gives_plus_zero():
    # an accumulator seeded -0.0 and stepped with all-zero operands: -0.0 + (+0.0) = +0.0 to nearest even, so skipping the padding steps
    # would change the sign bit; the float64 reference and its tolerance agree that the value is zero
    H, m = 32, 32
    seed = np.full(4 * m, -0.0, np.float32)
    assert (_bits(seed) == 0x80000000).all()
    zero = lambda *s: np.zeros(s, np.uint16)
    z, _ = LB.gates_steps(zero(2, H), zero(2, m), zero(4 * m, H), zero(4 * m, m), seed)
    assert not _bits(z).any()
    ref, tol = LB.gates_ref(zero(2, H), zero(2, m), zero(4 * m, H), zero(4 * m, m), seed)
    assert not ref.any() and (tol < 1e-40).all()


def test_ascending_k_and_the_order_of_the_two_parts():
    # 2^24 + 1 is not an fp32 value: a seed of 2^24 swallows a +1 step by step but not a +2, so the sum depends on which step carries what.
    # a then h, ascending k: step 0 of the a part carries +1 (lost), the h part's one step carries -2^24, a later a step +1 (lost) -> 0;
    # any order that met -2^24 before the +1s would end at 2.
    H, m = 32, 32
    one = bf16_round(np.float32(1.0)).item()
    a = np.zeros((1, H), np.uint16); a[0, 0] = one; a[0, 17] = one
    h = np.zeros((1, m), np.uint16); h[0, 3] = one
    W_ih = np.zeros((4 * m, H), np.uint16); W_ih[0, 0] = one; W_ih[0, 17] = one
    W_hh = np.zeros((4 * m, m), np.uint16); W_hh[0, 3] = bf16_round(np.float32(-2.0 ** 24)).item()
    seed = np.zeros(4 * m, np.float32); seed[0] = 2.0 ** 24
    z, _ = LB.gates_steps(a, h, W_ih, W_hh, seed)
    assert z[0, 0] == 0.0 and not z[0, 1:].any()
    ref, tol = LB.gates_ref(a, h, W_ih, W_hh, seed)
    assert ref[0, 0] == 2.0 and abs(z[0, 0] - ref[0, 0]) <= tol[0, 0]          # ... and the bound covers exactly this kind of loss


def test_rounding_points_and_first_zeroing():
    rng = np.random.default_rng(5)
    H, m, rows = 32, 32, 3
    W_ih = (rng.standard_normal((4 * m, H)) * 0.2).astype(np.float32)
    W_hh = (rng.standard_normal((4 * m, m)) * 0.2).astype(np.float32)
    b_ih, b_hh = (rng.standard_normal(4 * m) * 0.1).astype(np.float32), (rng.standard_normal(4 * m) * 0.1).astype(np.float32)
    a = rng.standard_normal((rows, H)).astype(np.float32)
    mem = rng.standard_normal((rows, 2 * m)).astype(np.float32)
    first = np.array([0, 1, 0])
    hn, cn, ops = LB.step(a, mem, first, W_ih, W_hh, b_ih, b_hh)
    # each operand rounded ONCE to nearest even: rounding what is already bf16 changes nothing, and the operands are what the products read
    for k, src in (("a", a), ("W_ih", W_ih), ("W_hh", W_hh)):
        assert np.array_equal(ops[k], bf16_round(src)) and np.array_equal(bf16_round(bf16_value(ops[k])), ops[k])
    assert bf16_round(np.float32(1.00390625)).item() == 0x3F80          # a tie goes to the even neighbour (1.0), not up
    assert bf16_round(np.float32(1.01171875)).item() == 0x3F82          # ... and up where up is even
    # the seed is summed in fp32, not in float64
    assert np.array_equal(_bits(ops["bsum"]), _bits(b_ih + b_hh))
    # FIRST: h and c exactly zero — the row equals a run from zero memory, whatever its memory held; the others read theirs
    assert not ops["h"][1].any() and ops["h"][0].any() and ops["h"][2].any()
    h0, c0, _ = LB.step(a, np.zeros_like(mem), np.zeros(rows, int), W_ih, W_hh, b_ih, b_hh)
    assert np.array_equal(_bits(hn[1]), _bits(h0[1])) and np.array_equal(_bits(cn[1]), _bits(c0[1]))
    assert not np.array_equal(_bits(hn[0]), _bits(h0[0]))
    # c stays fp32: an fp32 c that is not a bf16 value changes c' against its rounded twin (it would not if c were rounded on the way in)
    mem2 = mem.copy(); mem2[:, m:] = bf16_value(bf16_round(mem[:, m:]))
    _, cn2, _ = LB.step(a, mem2, first, W_ih, W_hh, b_ih, b_hh)
    assert not np.array_equal(_bits(cn[0]), _bits(cn2[0])) and np.array_equal(_bits(cn[1]), _bits(cn2[1]))
    # h is an operand in bf16 only: rounding the stored h beforehand changes nothing
    mem3 = mem.copy(); mem3[:, :m] = bf16_value(bf16_round(mem[:, :m]))
    hn3, cn3, _ = LB.step(a, mem3, first, W_ih, W_hh, b_ih, b_hh)
    assert np.array_equal(_bits(hn), _bits(hn3)) and np.array_equal(_bits(cn), _bits(cn3))
    # the step-wise chain lies within the bound of the float64 sum over the same bf16 values
    z, _ = LB.gates_steps(ops["a"], ops["h"], ops["W_ih"], ops["W_hh"], ops["bsum"])
    ref, tol = LB.gates_ref(ops["a"], ops["h"], ops["W_ih"], ops["W_hh"], ops["bsum"])
    assert (np.abs(z - ref) <= tol).all()


def test_host_cell_is_the_kernels_definition():
    # the cell against its formulas in float64: c' = f c + i g~, h' = o tanh(c') (the fast exp is good to ~1e-6), and exact saturation
    rng = np.random.default_rng(6)
    z = (rng.standard_normal((4, 4 * 32)) * 2).astype(np.float32)
    c = rng.standard_normal((4, 32)).astype(np.float32)
    hn, cn = LB.cell(z, c)
    sg = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    i, f, g, o = sg(z[:, :32]), sg(z[:, 32:64]), np.tanh(z[:, 64:96].astype(np.float64)), sg(z[:, 96:])
    cr = f * c + i * g
    assert np.abs(cn - cr).max() < 1e-5 and np.abs(hn - o * np.tanh(cr)).max() < 1e-5
    big = np.zeros((1, 4 * 32), np.float32); big[:, :32] = 100; big[:, 32:64] = -100; big[:, 64:96] = 100; big[:, 96:] = 100
    hn, cn = LB.cell(big, np.full((1, 32), 7.0, np.float32))
    assert (cn == 1.0).all() and np.allclose(hn, np.tanh(1.0), atol=1e-6)
