"""Long runs on the host (include/hk.h "LONG RUNS"): the clip twins against torch.nn.utils.clip_grad_norm_, the .npz checkpoint
round trip, SelfPlay's resume against an uninterrupted run on a fake pool, and the two new structs' layouts in C, ctypes and C#.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import test_csharp_layout as CSL
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.ppo import (CHECKPOINT_FORMAT, checkpoint_read, checkpoint_write, clip_coefficient, grad_norm, param_layout,
                                         split_params)
from hierarchicalkarting_amd.selfplay import SelfPlay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the clip twins
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_clip_twins_against_torch_clip_grad_norm():
    """The device's coefficient is the float64 expression rounded ONCE to float32, so it sits up to 2^-24 (relative) from torch's float64
    coefficient: the 1e-12 comparison of the scaled gradients is made with the expression before that rounding (dtype=np.float64), and the
    float32 form is asserted to be exactly its rounding."""
    import torch
    layout = param_layout(20, 32, 2, 3) + [("c_" + n, s) for n, s in param_layout(20, 32, 2, 0)]      # one flat vector: actor, then critic
    P = sum(int(np.prod(s)) for _, s in layout)
    assert P % 4 != 0
    rng = np.random.default_rng(11)
    g = rng.standard_normal(P) * np.exp(rng.uniform(-6, 2, P))
    norm = grad_norm(g)
    assert norm.dtype == np.float64
    for max_norm in (0.5 * norm, 1e-3, 2.0 * norm, norm * (1 + 1e-3), np.inf):
        bound = float(np.float32(max_norm))                      # the bound as the C ABI receives it
        params = []
        for name, part in split_params(g, layout).items():
            p = torch.zeros(part.shape, dtype=torch.float64, requires_grad=True)
            p.grad = torch.from_numpy(part.copy())
            params.append(p)
        total = float(torch.nn.utils.clip_grad_norm_(params, bound))
        assert abs(total - norm) <= 1e-12 * total
        want = np.concatenate([p.grad.numpy().reshape(-1) for p in params])
        c64 = clip_coefficient(norm, max_norm, dtype=np.float64)
        got = g * c64
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), max_norm
        c32 = clip_coefficient(norm, max_norm)
        assert type(c32) is np.float32 and _bits(c32) == _bits(np.float32(c64))
        if norm < bound:
            assert _bits(c32) == _bits(np.float32(1.0)) and np.array_equal(got, g)
        else:
            assert c32 < 1.0


def test_coefficient_is_exactly_one_below_the_bound_and_for_inf():
    for norm in (0.0, 1e-30, 0.37, 5.0, 1e20):
        assert _bits(clip_coefficient(norm, np.inf)) == _bits(np.float32(1.0))
        assert _bits(clip_coefficient(norm, 2.0 * norm + 1.0)) == _bits(np.float32(1.0))
    assert clip_coefficient(4.0, 1.0) == np.float32(1.0 / (4.0 + 1e-6))
    # the bound is the float32 the library is handed
    assert clip_coefficient(1.0, 1e-3) == np.float32(float(np.float32(1e-3)) / (1.0 + 1e-6))


def test_grad_norm_is_the_rounded_exact_sum_and_flags_non_finite():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(1001) * np.exp(rng.uniform(-20, 20, 1001))).astype(np.float32)
    exact = sum(Fraction(float(x)) ** 2 for x in g)
    assert grad_norm(g) == math.sqrt(float(exact))          # float(Fraction) rounds correctly, as math.fsum does
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[17] = bad
        assert not np.isfinite(grad_norm(h))
    assert grad_norm(np.zeros(5, np.float32)) == 0.0


# ---- the checkpoint file
def test_checkpoint_round_trip_keeps_bits_and_dtypes(tmp_path):
    rng = np.random.default_rng(0)
    f32 = rng.standard_normal(1003).astype(np.float32)
    f32[5:8] = np.array([0x7FC00001, 0xFF800000, 0x80000000], np.uint32).view(np.float32)        # a NaN with a payload, -Inf, -0
    d = dict(params=f32, f64=rng.standard_normal(77), i64=rng.integers(-2 ** 62, 2 ** 62, 9), u16=rng.integers(0, 65536, 33).astype(np.uint16),
             empty=np.zeros(0, np.int64), adam_steps=12345, lr=0.25, precision="bf16",
             cfg=dict(gamma=0.99, seed=4000000000), normalizer=dict(steps=90, mean=rng.standard_normal(6), m2=rng.random(6) + 0.5))
    path = tmp_path / "t.ckpt"
    checkpoint_write(str(path), d)
    assert path.exists() and not (tmp_path / "t.ckpt.npz").exists()
    back = checkpoint_read(str(path))
    assert back.pop("format") == CHECKPOINT_FORMAT

    def same(a, b, where):
        assert set(a) == set(b), where
        for k in a:
            if isinstance(a[k], dict):
                same(a[k], b[k], where + k + "/")
            elif isinstance(a[k], np.ndarray):
                assert isinstance(b[k], np.ndarray) and b[k].dtype == a[k].dtype and b[k].shape == a[k].shape and b[k].tobytes() == a[k].tobytes(), where + k
            else:
                assert type(b[k]) is type(a[k]) and b[k] == a[k], where + k
    same(d, back, "")
    assert [back[k].dtype for k in ("params", "f64", "i64", "u16")] == [np.float32, np.float64, np.int64, np.uint16]
    assert back["normalizer"]["steps"] == 90 and back["normalizer"]["mean"].dtype == np.float64
    # no pickle inside: every entry loads with allow_pickle=False
    with np.load(str(path), allow_pickle=False) as z:
        assert "normalizer/mean" in z.files and "cfg/seed" in z.files
        for k in z.files:
            z[k]
    with pytest.raises(ValueError):
        checkpoint_write(str(tmp_path / "o.ckpt"), dict(x=np.array([object()])))


def test_checkpoint_refuses_an_unknown_version_and_a_missing_key(tmp_path):
    p = str(tmp_path / "v.ckpt")
    checkpoint_write(p, dict(format=CHECKPOINT_FORMAT + 98, x=np.zeros(3)))
    with pytest.raises(ValueError, match="format"):
        checkpoint_read(p)
    with open(p, "wb") as f:
        np.savez(f, x=np.zeros(3))
    with pytest.raises(ValueError, match="format"):
        checkpoint_read(p)


# ---- SelfPlay resume against a fake pool
class _FakePool:
    """slots hold the learner's `version` at save time; the opponent policy is what the last load put there"""

    def __init__(self, slots):
        self.slot = {}
        self.version = 0.0
        self.opponent = None
        self.n = slots

    def save(self, slot, policy_index=None):
        self.slot[slot] = np.full(5, self.version, np.float32)

    def load(self, slot, policy_index):
        self.opponent = self.slot[slot].copy()

    def get_flat(self, slot):
        return self.slot[slot].copy()

    def put_flat(self, slot, flat):
        self.slot[slot] = np.array(flat, np.float32)


class _FakeTrainer:
    index = 0


KW = dict(window=3, save_steps=5, swap_steps=3, play_against_latest_model_ratio=0.5, initial_elo=400.0, seed=7)


def _round(sp, pool, i):
    pool.version = float(i + 1)                   # the learner has been trained once more
    sp.record_results(3 + i % 4, i % 3, 2 + (i * 5) % 7)
    sp.advance(3)


def test_selfplay_resumes_as_the_uninterrupted_run(tmp_path):
    pa = _FakePool(4)
    a = SelfPlay(None, _FakeTrainer(), 1, pool=pa, **KW)
    for i in range(17):
        _round(a, pa, i)
    path = str(tmp_path / "sp.ckpt")
    checkpoint_write(path, a.state_dict())
    cut = len(a.history)
    pb = _FakePool(4)
    b = SelfPlay(None, _FakeTrainer(), 1, pool=pb, **dict(KW, seed=12345))     # (another seed: the generator comes from the state)
    b.load_state_dict(checkpoint_read(path))
    assert np.array_equal(pb.opponent, pa.opponent) and b.opponent == a.opponent
    for i in range(17, 40):
        _round(a, pa, i)
        _round(b, pb, i)
    assert b.history == a.history and len(a.history) == 40
    assert b.ratings == a.ratings and b.elo == a.elo and b.attached_elo == a.attached_elo and b.cursor == a.cursor
    assert (b.steps, b.last_save, b.last_swap, b.opponent) == (a.steps, a.last_save, a.last_swap, a.opponent)
    assert set(pb.slot) == set(pa.slot) and all(np.array_equal(pb.slot[s], pa.slot[s]) for s in pa.slot)
    assert np.array_equal(pb.opponent, pa.opponent)
    # the run holds "latest" and window picks on both sides of the cut, and the window has wrapped
    for part in (a.history[:cut], a.history[cut:]):
        assert "latest" in part and any(isinstance(x, int) for x in part), part
    assert a.cursor > 2 * KW["window"]
    # without the generator's state the draws differ: the state is what continues them
    pc = _FakePool(4)
    c = SelfPlay(None, _FakeTrainer(), 1, pool=pc, **dict(KW, seed=12345))
    sd = checkpoint_read(path)
    c.load_state_dict(sd)
    c.rng = np.random.default_rng(12345)
    for i in range(17, 40):
        _round(c, pc, i)
    assert c.history != a.history


def test_selfplay_state_refusals_and_pool_option():
    pool = _FakePool(4)
    sp = SelfPlay(None, _FakeTrainer(), 1, pool=pool, **KW)
    sd = sp.state_dict()
    assert sd["opponent"] == -2 and set(sd["pool"]) == {"slot0"} and sd["history"].dtype == np.int64
    assert "pool" not in sp.state_dict(include_pool=False)
    for k in ("rng", "ratings", "cursor"):
        bad = dict(sd)
        del bad[k]
        with pytest.raises(ValueError, match=k):
            sp.load_state_dict(bad)
    with pytest.raises(ValueError, match="format"):
        sp.load_state_dict(dict(sd, format=CHECKPOINT_FORMAT + 1))
    other = SelfPlay(None, _FakeTrainer(), 1, pool=_FakePool(6), **dict(KW, window=5))
    with pytest.raises(ValueError, match="window"):
        other.load_state_dict(sd)


# ---- hk_ppo_update_opts / hk_ppo_update_report: C, ctypes and C#
def test_long_run_struct_layouts(tmp_path):
    pairs = [("hk_ppo_update_opts", "HkPpoUpdateOpts", _lib.PpoUpdateOpts), ("hk_ppo_update_report", "HkPpoUpdateReport", _lib.PpoUpdateReport)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "hk.h"), "int main(){"]
    want = []
    for cname, _, ct in pairs:
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(C.sizeof(ct))
        for fname, _ in ct._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
            want.append(getattr(ct, fname).offset)
    lines += ['printf("%d\\n", HK_PPO_CLIP);', 'printf("%d\\n", HK_PPO_FIELDS);', "return 0;}"]
    want += [_lib.PPO_FIELDS["clip"], _lib.HK_PPO_FIELDS]
    src = tmp_path / "lr.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "lr"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert C.sizeof(_lib.PpoUpdateOpts) == 32 and C.sizeof(_lib.PpoUpdateReport) == 48
    assert _lib.PPO_FIELDS["clip"] == _lib.HK_PPO_FIELDS - 1 and len(_lib.PPO_CLIP_NAMES) == 8
    structs, imports = CSL._parse_cs()
    for _, cs, ct in pairs:
        fields = structs[cs]
        assert [f[0] for f in fields] == [n for n, _ in ct._fields_]
        off = 0
        for (name, typ, ptr, cnt), (fname, ftype) in zip(fields, ct._fields_):
            kind, esz, n = CSL._flatten(ftype)
            assert not ptr and CSL.CS_TYPES[typ] == (kind, esz) and cnt == n
            off = (off + esz - 1) // esz * esz
            assert off == getattr(ct, fname).offset
            off += esz * n
        assert off == C.sizeof(ct)
    new = {"hk_ppo_update_opt", "hk_ppo_adam_clipped", "hk_ppo_get_counters", "hk_ppo_set_counters"}
    assert new <= set(imports) and new <= set(_lib.SYMBOLS)
    cs = open(os.path.join(ROOT, "host", "HkNative.cs")).read()
    assert "HK_PPO_CLIP = %d" % _lib.PPO_FIELDS["clip"] in cs
