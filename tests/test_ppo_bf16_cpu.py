"""PPO trainer, bf16 mode, without a GPU: the numpy twin of the device's rounding against torch's bfloat16 conversion, and the new entry points
declared alike in hk.h, _lib.py and HkNative.cs."""
import os
import re

import numpy as np

from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.ppo import bf16_round, bf16_value, PRECISIONS
import test_csharp_layout as CSL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4028234e38, 2.0 ** -126], np.float32)
NEW = ("hk_ppo_set_precision", "hk_ppo_get_precision", "hk_ppo_gemm_bf16")


def test_rounding_twin_against_torch():
    import torch
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(10 ** 5).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 10 ** 5).astype(np.float32),
                        rng.integers(0, 2 ** 32, 10 ** 4, dtype=np.uint64).astype(np.uint32).view(np.float32), SPECIALS])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = bf16_round(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(bf16_value(got[nan])).all() and np.isnan(bf16_value(want[nan])).all()
    assert (got[nan] == 0x7FC0).all()
    # ties go to even, Inf and the signed zeros survive, the largest fp32 value rounds to Inf
    assert list(bf16_round(SPECIALS[[0, 1, 2, 3, 7, 8, 9]])) == [0x0000, 0x8000, 0x7F80, 0xFF80, 0x3F80, 0x3F82, 0x7F80]
    # a bf16 value is a fixed point
    assert np.array_equal(bf16_round(bf16_value(got[~nan])), got[~nan])


def test_new_symbols_agree_in_header_ctypes_and_csharp():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hk.h")).read(), flags=re.S)
    _, imports = CSL._parse_cs()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert n in _lib.SYMBOLS and n in imports, n
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr)
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[n][1]), n
    vals = dict(re.findall(r"\b(HK_PPO_PREC_\w+)\s*=\s*(\d+)", hdr))
    assert {k: int(v) for k, v in vals.items()} == {"HK_PPO_PREC_F32": _lib.HK_PPO_PREC_F32, "HK_PPO_PREC_BF16": _lib.HK_PPO_PREC_BF16}
    assert PRECISIONS == {"f32": _lib.HK_PPO_PREC_F32, "bf16": _lib.HK_PPO_PREC_BF16}
    cs = open(os.path.join(ROOT, "host", "HkNative.cs")).read()
    for k, v in vals.items():
        assert re.search(r"\b%s = %s\b" % (k, v), cs), k
    assert "HK_PPO_SHADOW = %d" % _lib.PPO_FIELDS["shadow"] in cs and "HK_PPO_FIELDS = %d" % _lib.HK_PPO_FIELDS in cs
