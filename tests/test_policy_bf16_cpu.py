"""HK_POLICY_PREC_BF16 without a GPU: the host fmaf twin and the chain composed from it (policy_bf16_restate.py) against the CPU oracle bit for
bit — which validates the twin test_policy_bf16_gpu.py builds its heads from — the rounding twin on the tie, Inf and NaN patterns, and the two
new entry points declared alike in hk.h, _lib.py and HkNative.cs."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import policy_bf16_restate as PB
import test_csharp_layout as CSL
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.config import make_config
from hierarchicalkarting_amd.env import RacingEnv
from hierarchicalkarting_amd.policy import Policy
from hierarchicalkarting_amd.ppo import bf16_round, bf16_value
from parity import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hk_policy_set_precision", "hk_policy_get_precision")


def test_fmaf_twin_where_rounding_twice_goes_wrong():
    f32 = np.float32
    # c = 1 + 2^-23 (last bit odd), product = 2^-24 (1 - 2^-46): the exact sum lies 2^-70 BELOW the fp32 tie 1 + 2^-23 + 2^-24.  float64 cannot
    # hold that: its sum is the tie itself, and rounding it again goes to even, 1 + 2^-22.  Rounded once, the result is c.
    x, y, c = f32(1.0 + 2.0 ** -23), f32(2.0 ** -24 - 2.0 ** -47), f32(1.0 + 2.0 ** -23)
    assert float(x) * float(y) == 2.0 ** -24 * (1.0 - 2.0 ** -46)
    assert (np.float64(x) * np.float64(y) + np.float64(c)).astype(f32) == f32(1.0 + 2.0 ** -22)        # the naive way
    assert PB.fmaf(x, y, c) == c
    assert PB.fmaf(-x, y, -c) == -c
    # c = 1 (last bit even), product = 2^-24 (1 + 2^-23)^2 > the tie: up, and the mirrored product < the tie: down
    assert PB.fmaf(f32(2.0 ** -24 + 2.0 ** -47), f32(1.0 + 2.0 ** -23), f32(1.0)) == f32(1.0 + 2.0 ** -23)
    assert PB.fmaf(y, x, f32(1.0)) == f32(1.0)
    assert PB.fmaf(f32(2.0 ** -24), f32(1.0), f32(1.0)) == f32(1.0)                                      # the exact tie goes to even
    # exact cases are untouched
    rng = np.random.default_rng(0)
    v = rng.integers(-1000, 1000, (3, 4096)).astype(f32)
    assert np.array_equal(PB.fmaf(v[0], v[1], v[2]), v[0] * v[1] + v[2])


@pytest.mark.parametrize("shape", [dict(agents=4, stack=4, hidden=64, layers=2, rows=5, normalize=True),
                                   dict(agents=2, stack=1, hidden=96, layers=3, rows=3, normalize=False)])
def test_composed_fp32_chain_is_the_oracles(shape):
    o = O.OracleEnv(make_config(1, shape["agents"], low_mode=[_lib.HK_LOW_RL] * shape["agents"]))
    K = o.obs_dim * shape["stack"]
    pol = Policy.random(K, shape["hidden"], shape["layers"], stack=shape["stack"], seed=11, normalize=shape["normalize"])
    assert o.attach_policy(pol, [0], 2) == 0
    rng = np.random.default_rng(1)
    obs = (3.0 * rng.standard_normal((shape["rows"], K))).astype(np.float32)
    mu, lg = PB.policy_f32(O.lib(), pol, obs)
    want_mu, want_lg = o.policy_forward(0, obs)
    assert_bits_equal(mu, want_mu, "mu %s" % shape)
    assert_bits_equal(lg, want_lg, "logits %s" % shape)


def test_rounding_twin_on_ties_inf_nan():
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.4028234e38, 1e-40], np.float32)
    got = bf16_round(x)
    assert list(got) == [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0x3F82, 0x3F81, 0x7F80, 0x0001]
    neg_nan = np.array([0xFFC00001, 0x7F800001], np.uint32).view(np.float32)
    assert list(bf16_round(neg_nan)) == [0x7FC0, 0x7FC0]
    assert np.array_equal(bf16_round(bf16_value(got[:4])), got[:4])


def test_new_symbols_agree_in_header_ctypes_and_csharp():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hk.h")).read(), flags=re.S)
    _, imports = CSL._parse_cs()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert n in _lib.SYMBOLS and n in imports, n
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr)
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[n][1]), n
    vals = {k: int(v) for k, v in re.findall(r"\b(HK_POLICY_PREC_\w+)\s*=\s*(\d+)", hdr)}
    assert vals == {"HK_POLICY_PREC_F32": _lib.HK_POLICY_PREC_F32, "HK_POLICY_PREC_BF16": _lib.HK_POLICY_PREC_BF16}
    assert RacingEnv.POLICY_PRECISIONS == {"f32": _lib.HK_POLICY_PREC_F32, "bf16": _lib.HK_POLICY_PREC_BF16}
    cs = open(os.path.join(ROOT, "host", "HkNative.cs")).read()
    for k, v in vals.items():
        assert re.search(r"\b%s = %d\b" % (k, v), cs), k
    # ... and the library exports them
    L = _lib.load()
    for n in NEW:
        assert getattr(L, n) is not None, n
