"""Recurrent actors (hk.h "RECURRENT ACTORS") without a GPU: the host twin of policy_lstm_kernel against an independent float64
restatement, the shared sigmoid / tanh against libm over every finite fp32 input, the Python round trips (arrays, ONNX) and the ABI."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import policy_lstm_restate as RS                          # noqa: E402
import policy_lstm_twin as TW                             # noqa: E402
from hierarchicalkarting_amd.policy import Policy         # noqa: E402

# (in_dim, stack, hidden, n_layers, m, rows, seed): the K remainder modulo 8, an odd block count, the reference shape on a 4-agent input
CASES = [(52, 4, 32, 1, 32, 24, 11), (52, 4, 96, 2, 96, 24, 12), (312, 4, 128, 3, 128, 24, 13), (216, 4, 256, 2, 64, 24, 14),
         # the widths tests/test_policy_lstm_fields_gpu.py holds the kernel to: three layer-0 chunks at the largest footprint, a chunked input
         # with remainder 2 modulo 8 on an odd block count, one observation of a 4-kart field
         (624, 8, 256, 2, 128, 24, 15), (546, 7, 96, 2, 96, 24, 16), (78, 1, 160, 1, 32, 24, 17)]
# Measured here on CASES: the twin's largest absolute deviation from the float64 restatement over mu, logits and the memory is 1.672e-06
# (the 624 -> 256 x 2 -> m = 128 case: fp32 chains of up to 624 terms and the <= 2 ulp exp; 1.135e-06 on 216 -> 256 x 2 -> m = 64, which set
# the figure before the 624-, 546- and 78-input cases joined, and 4.3e-07 .. 1.0e-06 on the others); the tolerance is 4 x that, rounded up to
# one significant digit.  The mutated restatements are 0.76 .. 2.6 away: five orders of magnitude more.
TWIN_MAX_DEV = 1.672e-06
TWIN_TOL = 7e-06
# the largest absolute error of hk_sigmoidf / hk_tanhf_fast over every finite fp32 input against libm in double, measured once
# (8.931e-08 and 8.994e-08, recorded rounded up)
SIGMOID_MAX_ERR = 8.94e-08
TANH_MAX_ERR = 9.00e-08


def make_case(in_dim, stack, hidden, n_layers, m, rows, seed):
    pol = Policy.random(in_dim, hidden, n_layers, 3, stack=stack, seed=seed, memory_size=2 * m)
    r = np.random.default_rng(1000 + seed)
    obs = (pol.norm_mean + pol.norm_std * r.standard_normal((rows, in_dim))).astype(np.float32)
    mem = r.uniform(-1.0, 1.0, (rows, 2 * m)).astype(np.float32)
    return pol, obs, mem


@pytest.fixture(scope="module")
def twin_results():
    return [(c, make_case(*c)) for c in CASES]


def _dev(a, b):
    return max(float(np.max(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)))) for x, y in zip(a, b))


def test_twin_matches_float64_restatement(twin_results):
    """the twin (fp32, the kernel's arithmetic) against the float64 restatement: measured deviation 1.672e-06, asserted 7e-06 (4 x, rounded
    up); each of the four mutated restatements must miss that tolerance by at least 100 x, which proves the inputs discriminate"""
    worst = 0.0
    for c, (pol, obs, mem) in twin_results:
        got = TW.step(pol, obs, mem)
        want = RS.step(pol.arrays(), obs, mem)
        d = _dev(got, want)
        print("case %s: twin vs float64 restatement %.3e" % (c, d))
        worst = max(worst, d)
        for mut in RS.MUTATIONS:
            dm = _dev(got, RS.step(pol.arrays(), obs, mem, mutate=mut))
            print("   mutation %-16s %.3e" % (mut, dm))
            assert dm >= 100.0 * TWIN_TOL, "case %s: mutation %s is only %.3e away" % (c, mut, dm)
    print("worst %.3e" % worst)
    assert worst <= TWIN_TOL


def test_twin_null_memory_is_zero_memory_and_chains(twin_results):
    _, (pol, obs, mem) = twin_results[0]
    a = TW.step(pol, obs, None)
    b = TW.step(pol, obs, np.zeros_like(mem))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    s1 = TW.step(pol, obs, mem)
    s2 = TW.step(pol, obs[::-1], s1[2])
    r1 = RS.step(pol.arrays(), obs, mem)
    r2 = RS.step(pol.arrays(), obs[::-1], r1[2])
    assert _dev(s2, r2) <= 2 * TWIN_TOL        # (two steps: the first step's deviation enters the second through the memory)


def test_sigmoid_tanh_sweep():
    """every finite fp32 input against libm's double tanh and 1 / (1 + exp(-x)); exact values at +-Inf, NaN at NaN"""
    s = TW.sweep()
    print(s)
    assert s["sigmoid_max_abs_err"] <= SIGMOID_MAX_ERR
    assert s["tanh_max_abs_err"] <= TANH_MAX_ERR
    assert s["sigmoid_pinf"] == 1.0 and s["sigmoid_ninf"] == 0.0 and np.isnan(s["sigmoid_nan"])
    assert s["tanh_pinf"] == 1.0 and s["tanh_ninf"] == -1.0 and np.isnan(s["tanh_nan"])


# ---- Python round trips
def _same_policy(a, b):
    da, db = a.arrays(), b.arrays()
    assert sorted(da) == sorted(db)
    for k in da:
        assert da[k].dtype == db[k].dtype and np.array_equal(da[k], db[k]), k
    assert a.memory_size == b.memory_size


def test_arrays_round_trip():
    pol = Policy.random(52, 64, 2, 3, seed=3, memory_size=128)
    assert pol.memory_size == 128 and pol.W_mu.shape == (64,) and pol.W_branch.shape == (3, 64)
    d = pol.arrays("p_")
    assert {"p_lstm_W_ih", "p_lstm_W_hh", "p_lstm_b_ih", "p_lstm_b_hh"} <= set(d)
    _same_policy(pol, Policy.from_arrays(d, "p_"))
    plain = Policy.random(52, 64, 2, 3, seed=3)
    assert plain.memory_size == 0 and plain.lstm is None and not any(k.startswith("lstm_") for k in plain.arrays())
    # memory_size = 0 keeps the draws of the signature's defaults; with memory the trunk and the normaliser are the same draws
    assert np.array_equal(plain.W[1], pol.W[1]) and np.array_equal(plain.b[0], pol.b[0])
    with pytest.raises(ValueError):
        Policy(pol.W, pol.b, pol.W_mu, pol.b_mu, pol.log_sigma, pol.W_branch, pol.b_branch, lstm={"W_ih": pol.lstm["W_ih"]})


def test_onnx_round_trip_and_refusals(tmp_path):
    from onnx_write_lstm import write_lstm_actor, VARIANTS
    pol = Policy.random(52, 64, 2, 3, seed=5, memory_size=64)
    back = Policy.from_onnx(write_lstm_actor(str(tmp_path / "lstm.onnx"), pol))
    _same_policy(pol, back)
    words = {"bidirectional": "bidirectional", "reverse": "direction", "peepholes": "peepholes", "sequence_lens": "sequence_lens",
             "activations": "activations", "hidden_size": "hidden_size", "two_cells": "stacked", "not_after_swish": "Swish"}
    assert set(words) == set(VARIANTS)
    for v in VARIANTS:
        with pytest.raises(ValueError) as e:
            Policy.from_onnx(write_lstm_actor(str(tmp_path / (v + ".onnx")), pol, variant=v))
        assert words[v] in str(e.value), (v, str(e.value))


# ---- ABI
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from hierarchicalkarting_amd import _lib
    return _lib


def test_lstm_desc_layout_matches_c(built, tmp_path):
    src = tmp_path / "sz.c"
    fields = ("memory_size", "reserved", "W_ih", "W_hh", "b_ih", "b_hh")
    exprs = ["sizeof(hk_policy_lstm_desc)"] + ["offsetof(hk_policy_lstm_desc, %s)" % f for f in fields] + [
        "(size_t)HK_POLICY_MAX_MEMORY", "(size_t)HK_RO_MEMORY", "(size_t)HK_RO_NEXT_MEMORY", "(size_t)HK_RO_FIELDS"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){\n%s\nreturn 0;}\n'
                   % (os.path.join(ROOT, "include", "hk.h"), "\n".join('printf("%%zu\\n", %s);' % e for e in exprs)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(built.PolicyLstmDesc)] + [getattr(built.PolicyLstmDesc, f).offset for f in fields] + [
        built.HK_POLICY_MAX_MEMORY, built.RO_FIELDS["memory"][0], built.RO_FIELDS["next_memory"][0], built.HK_RO_FIELDS]
    assert got == want


def test_new_symbols_are_exported(built):
    L = built.load()
    for n in ("hk_policy_attach_lstm", "hk_policy_memory_size", "hk_policy_forward_mem", "hk_policy_memory_get", "hk_policy_memory_set"):
        assert hasattr(L, n) and n in built.SYMBOLS
