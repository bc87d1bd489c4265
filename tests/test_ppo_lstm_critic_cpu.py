"""Host-side checks of the recurrent critic (include/hk.h "PPO trainer" RECURRENT CRITIC), no GPU: the restatement's critic gradients
against float64 central differences, the critic part of the parameter layout, the checkpoint round trip and check_state's refusals, and the
three-way declaration of the new symbol, struct and field numbers in hk.h / _lib.py / HkNative.cs."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalkarting_amd import _lib, ppo  # noqa: E402


def _toy(seed=3):
    """2 sequences per window (E = 1, S = 2), R = 6 rows in windows of L = 4 (a dead tail of 2), a FIRST strictly inside window 0 and one on
    window 1's first row, and a non-zero initial critic memory"""
    import torch
    r = np.random.default_rng(seed)
    R, L, E, S, D, Ha, m, Hc, mv, nb = 6, 4, 1, 2, 5, 4, 3, 4, 2, 2
    t64 = lambda *s: torch.tensor(r.standard_normal(s) * 0.6, requires_grad=True)
    ap = {"W0": t64(Ha, D), "b0": t64(Ha), "W_ih": t64(4 * m, Ha), "W_hh": t64(4 * m, m), "b_ih": t64(4 * m), "b_hh": t64(4 * m), "W_mu": t64(m),
          "b_mu": t64(1), "log_sigma": t64(1), "W_branch": t64(nb, m), "b_branch": t64(nb)}
    cp = {"W0": t64(Hc, D), "b0": t64(Hc), "W1": t64(Hc, Hc), "b1": t64(Hc), "W_ih": t64(4 * mv, Hc), "W_hh": t64(4 * mv, mv), "b_ih": t64(4 * mv),
          "b_hh": t64(4 * mv), "W_mu": t64(mv), "b_mu": t64(1)}
    n = R * E * S
    first = np.zeros((R, E * S), np.int32)
    first[2, 0] = 1
    first[4, 1] = 1
    f = dict(raw=r.standard_normal(n), branch=r.integers(0, nb, n), logp_cont=r.standard_normal(n) * 0.1 - 1.0, logp_disc=r.standard_normal(n) * 0.1 - 0.7)
    d = dict(ap=ap, cp=cp, X=torch.tensor(r.standard_normal((R, E * S, D))), memory=r.uniform(-1, 1, (R, E * S, 2 * m)),
             critic_memory=r.uniform(-1, 1, (2, E * S, 2 * mv)), first=first, f=f, adv=r.standard_normal(n), v_old=r.standard_normal(n) * 0.3,
             ret=r.standard_normal(n), dims=(R, L, E, S))
    assert d["critic_memory"].any()
    return d


def _loss(d, sids, mutate=None):
    import ppo_lstm_critic_restate as CR
    return CR.loss(d["ap"], d["cp"], 1, 2, d["X"], d["memory"], d["critic_memory"], d["first"], d["f"], d["adv"], d["v_old"], d["ret"], sids,
                   *d["dims"], 0.2, 5e-3, mutate)[0]


def test_restated_critic_gradients_against_central_differences():
    import torch
    d = _toy()
    sids = [0, 1, 2, 3, 7]          # both windows of both agents, one id skipped
    _loss(d, sids).backward()
    worst = 0.0
    for name, p in d["cp"].items():
        g = p.grad.clone()
        flat = p.detach().reshape(-1)
        num = torch.zeros_like(flat)
        for i in range(flat.numel()):
            vals = []
            for sgn in (1.0, -1.0):
                with torch.no_grad():
                    p.reshape(-1)[i] += sgn * 1e-6
                vals.append(_loss(d, sids).item())
                with torch.no_grad():
                    p.reshape(-1)[i] -= sgn * 1e-6
            num[i] = (vals[0] - vals[1]) / 2e-6
        err = float((g.reshape(-1) - num).norm() / max(float(num.norm()), 1e-30))
        worst = max(worst, err)
        assert num.norm() > 0, name
        assert err <= 1e-6, (name, err)          # central differences at h = 1e-6 in float64: truncation h^2, rounding 1e-16 / h
    # both biases: the same gradient; the initial critic memory is a constant
    assert torch.equal(d["cp"]["b_ih"].grad, d["cp"]["b_hh"].grad)
    # every mutation changes some critic gradient on this toy
    import ppo_lstm_critic_restate as CR
    ref = {k: v.grad.clone() for k, v in d["cp"].items()}
    for mut in CR.MUTATIONS:
        for p in list(d["cp"].values()) + list(d["ap"].values()):
            p.grad = None
        _loss(d, sids, mut).backward()
        assert max(float((d["cp"][k].grad - ref[k]).norm() / ref[k].norm()) for k in ref) > 1e-3, mut


def test_restated_value_pass_is_the_window_forward():
    """the value pass's values and CRITIC_MEMORY feed the window forward: v of the loss's heads at unchanged parameters equals the pass's"""
    import torch
    import ppo_lstm_critic_restate as CR
    d = _toy(5)
    R, L, E, S = d["dims"]
    cp = {k: v.detach() for k, v in d["cp"].items()}
    mem_in = d["critic_memory"][0]
    boot = torch.tensor(np.random.default_rng(1).standard_normal((E * S, 5)))
    v, vb, cm, out = CR.value_pass(cp, 2, d["X"], boot, d["first"], np.array([0, 1]), mem_in, L)
    assert v.shape == (R, E * S) and vb.shape == (E * S,) and cm.shape == (2, E * S, 4)
    assert np.array_equal(cm[0], mem_in) and not out[1].any() and out[0].any()
    d["critic_memory"] = cm
    heads = CR.loss(d["ap"], d["cp"], 1, 2, d["X"], d["memory"], cm, d["first"], d["f"], d["adv"], d["v_old"], d["ret"], [0, 1, 2, 3], R, L, E, S, 0.2,
                    5e-3)[2]
    live = heads["rowid"] >= 0
    assert np.abs(heads["v"][live] - v.reshape(-1)[heads["rowid"][live]]).max() <= 1e-14
    # the memory the critic's cell wrote in window 0's last row is what window 1 starts from
    assert np.abs(heads["critic_mem"][L - 1, :2] - cm[1]).max() <= 1e-14


def test_param_layout_of_the_critic_part():
    lay = ppo.param_layout(216, 96, 3, 0, 128)
    assert [n for n, _ in lay] == ["W0", "b0", "W1", "b1", "W2", "b2", "W_ih", "W_hh", "b_ih", "b_hh", "W_mu", "b_mu"]
    shapes = dict(lay)
    assert shapes["W_ih"] == (256, 96) and shapes["W_hh"] == (256, 64) and shapes["b_ih"] == shapes["b_hh"] == (256,)
    assert shapes["W_mu"] == (64,) and shapes["b_mu"] == (1,)
    assert ppo.param_layout(216, 96, 3, 0) == ppo.param_layout(216, 96, 3, 0, 0)          # the feed-forward critic is as it was
    flat = np.arange(sum(int(np.prod(s)) for _, s in lay), dtype=np.float32)
    parts = ppo.split_params(flat, lay)
    assert parts["b_mu"][0] == flat[-1] and parts["W_mu"][0] == flat[-65]
    with pytest.raises(ValueError):
        ppo.param_layout(216, 96, 3, 0, 127)


def _state(mv2=64, es=4):
    r = np.random.default_rng(0)
    return dict(format=ppo.CHECKPOINT_FORMAT, actor_shape=np.array([216, 32, 2, 3, 64]), critic_shape=np.array([216, 32, 2, 0, mv2]), sequence_length=4,
                params=r.standard_normal(10).astype(np.float32), critic_mem_in=r.standard_normal(es * mv2).astype(np.float32),
                critic_mem_out=r.standard_normal(es * mv2).astype(np.float32))


def test_checkpoint_round_trip_and_check_state(tmp_path):
    d = _state()
    path = str(tmp_path / "critic.ckpt")
    ppo.checkpoint_write(path, d)
    back = ppo.checkpoint_read(path)
    for k in ("critic_mem_in", "critic_mem_out", "params"):
        assert back[k].dtype == np.float32 and np.array_equal(back[k].view(np.int32), d[k].view(np.int32)), k
    assert back["critic_shape"].tolist() == [216, 32, 2, 0, 64] and back["sequence_length"] == 4
    ppo.check_state(back, "ppo", d["actor_shape"], d["critic_shape"], sequence_length=4)
    with pytest.raises(ValueError, match="critic_shape"):          # another critic memory size
        ppo.check_state(back, "ppo", d["actor_shape"], np.array([216, 32, 2, 0, 128]), sequence_length=4)
    with pytest.raises(ValueError, match="critic_shape"):          # a feed-forward critic's trainer does not take it
        ppo.check_state(back, "ppo", d["actor_shape"], np.array([216, 32, 2, 0]), sequence_length=4)
    ff = {k: v for k, v in d.items() if not k.startswith("critic_mem")}
    ff["critic_shape"] = np.array([216, 32, 2, 0])
    with pytest.raises(ValueError, match="critic_shape"):          # a feed-forward critic's checkpoint
        ppo.check_state(ff, "ppo", d["actor_shape"], d["critic_shape"], sequence_length=4)
    ppo.check_state(ff, "ppo", d["actor_shape"], ff["critic_shape"], sequence_length=4)          # ... loads where it belongs, without the memories
    for key in ("critic_mem_in", "critic_mem_out"):
        miss = {k: v for k, v in d.items() if k != key}
        with pytest.raises(ValueError, match=key):
            ppo.check_state(miss, "ppo", d["actor_shape"], d["critic_shape"], sequence_length=4)
        wrong = dict(d, **{key: d[key].astype(np.float64)})
        with pytest.raises(ValueError, match=key):
            ppo.check_state(wrong, "ppo", d["actor_shape"], d["critic_shape"], sequence_length=4)


def test_the_three_declarations_agree():
    hdr = open(os.path.join(ROOT, "include", "hk.h")).read()
    cs = open(os.path.join(ROOT, "host", "HkNative.cs")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    # the symbol
    assert re.search(r"\bint\s+hk_ppo_create_recurrent_critic\s*\(\s*hk_handle\s+h\s*,\s*int\s+policy\s*,\s*const\s+hk_policy_desc\s*\*\s*critic\s*,\s*"
                     r"const\s+hk_policy_lstm_desc\s*\*\s*critic_cell\s*,\s*const\s+hk_ppo_config\s*\*\s*cfg\s*,\s*"
                     r"const\s+hk_ppo_recurrent_critic_desc\s*\*\s*r\s*\)\s*;", code)
    res, args = _lib.SYMBOLS["hk_ppo_create_recurrent_critic"]
    assert res is C.c_int and args[1] is C.c_int and len(args) == 6
    assert [a._type_ for a in args[2:]] == [_lib.PolicyDesc, _lib.PolicyLstmDesc, _lib.PpoConfig, _lib.PpoRecurrentCriticDesc]
    assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern int hk_ppo_create_recurrent_critic\(IntPtr h, int policy, HkPolicyDesc\* critic, "
                     r"HkPolicyLstmDesc\* criticCell, HkPpoConfig\* cfg, HkPpoRecurrentCriticDesc\* r\);", cs)
    # the struct: four int32 words
    m = re.search(r"typedef struct hk_ppo_recurrent_critic_desc \{(.*?)\} hk_ppo_recurrent_critic_desc;", code, flags=re.S)
    assert re.findall(r"int32_t\s+(\w+)(?:\[(\d+)\])?\s*;", m.group(1)) == [("sequence_length", ""), ("value_chunk_steps", ""), ("reserved", "2")]
    ct = _lib.PpoRecurrentCriticDesc
    assert [(n, getattr(ct, n).offset, getattr(ct, n).size) for n, _ in ct._fields_] == [("sequence_length", 0, 4), ("value_chunk_steps", 4, 4), ("reserved", 8, 8)]
    assert C.sizeof(ct) == 16
    m = re.search(r"public unsafe struct HkPpoRecurrentCriticDesc\s*\{(.*?)\n    \}", cs, flags=re.S)
    assert re.findall(r"public\s+(fixed\s+)?int\s+(\w+)(?:\[(\d+)\])?;", m.group(1)) == [("", "sequence_length", ""), ("", "value_chunk_steps", ""),
                                                                                         ("fixed ", "reserved", "2")]
    # the field numbers, outside [0, HK_PPO_FIELDS) and behind hk_ppo_recurrent_field
    want = {"critic_memory": 33, "critic_mem_in": 34, "critic_mem_out": 35, "mb_critic_memory": 36}
    assert _lib.PPO_RECURRENT_CRITIC_FIELDS == want and _lib.PPO_RECURRENT_FIELDS == {"mb_memory": 32}
    assert not set(want.values()) & set(_lib.PPO_FIELDS.values()) and min(want.values()) > max(_lib.PPO_FIELDS.values())
    for name, num in want.items():
        assert re.search(r"\bHK_PPO_%s\s*=\s*%d\b" % (name.upper(), num), code), name
        assert re.search(r"\bHK_PPO_%s = %d\b" % (name.upper(), num), cs), name
