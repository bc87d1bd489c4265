#!/usr/bin/env python3
"""What a host-side refactor of the trainers (hk_train.hip, and hk_handle.h under it) must leave bit for bit: one fixed course through the PPO trainer (f32, then bf16), the POCA
trainer and the recurrent PPO trainer (feed-forward critic, then recurrent critic), with a SHA-256 of every readable trainer field, of the
returned stats and of the update report after each step, printed as one JSON document.  Run it once per library, each in a fresh process, and
compare the two outputs byte for byte:

    HK_LIB_PATH=build/libhk_parent.so python tools/trainer_identity.py --out a.json
    python tools/trainer_identity.py --out b.json && cmp a.json b.json

Under `rocprofv3 --kernel-trace --stats` the same course gives the launch counts to compare.  The set-ups are those of tests/test_ppo_gpu.py
(24 envs of 2v2, R = 90), the h36 and s4 cases of tests/test_poca_gpu.py and the field of tests/test_ppo_lstm_gpu.py (5 envs of 2 karts, R = 11,
L = 4, staggered resets) under an actor (H, m) = (96, 32) and a critic (Hc, m_v) = (64, 128), restated here so that the tool stands without the
tests.  --courses picks some of the six (ppo_f32 ppo_bf16 poca_h36 poca_s4 lstm lstm_critic); the document holds the ones run."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hierarchicalkarting_amd as hk
from hierarchicalkarting_amd import _lib, ppo
from hierarchicalkarting_amd.poca import PocaCritic
from hierarchicalkarting_amd.policy import Policy

RL, P, R = _lib.HK_LOW_RL, 2, 90
PPO_ENV = dict(E=24, A=4, slots=[0, 1], other=[2, 3], actor=(256, 3), other_actor=(128, 2), kw={})
POCA_ENVS = {
    "h36": dict(E=24, A=4, slots=[0, 1], other=[2, 3], actor=(256, 3), other_actor=(64, 2), H=36, L=1),
    "s4": dict(E=8, A=8, slots=[0, 1, 2, 3], other=[4, 5, 6, 7], actor=(64, 2), other_actor=(64, 2), H=64, L=2),
}
TRAINING = dict(env_mode=_lib.HK_MODE_TRAINING)
COURSES = ("ppo_f32", "ppo_bf16", "poca_h36", "poca_s4", "lstm", "lstm_critic")
LSTM_ENV = dict(E=5, R=11, L=4, actor=(96, 32), critic=(64, 128))          # all four widths differ; 10 sequences per window


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def env_of(c, training):
    kw = dict(low_mode=[RL] * c["A"], rewards=1, max_episode_steps=150, jitter_seed=4)
    if training:
        kw.update(TRAINING, training_agents=[1] * c["A"])
    g = hk.RacingEnv(hk.make_config(c["E"], c["A"], **kw))
    g.reset()
    stack = min(4, _lib.HK_POLICY_MAX_IN // g.obs_dim)
    pols = [(Policy.random(g.obs_dim * stack, c["actor"][0], c["actor"][1], stack=stack, seed=1), c["slots"]),
            (Policy.random(g.obs_dim * stack, c["other_actor"][0], c["other_actor"][1], stack=stack, seed=2, deterministic=True), c["other"])]
    for pol, slots in pols:
        g.attach_policy(pol, slots, P)
    g.rollout_begin(R)
    g.step(R * P)
    g.rollout_close()
    return g


def fields(tr, poca, live=None):
    """name -> SHA-256 of the field, or the library's refusal where it is not readable yet.  live (the recurrent courses): which rows of the
    last minibatch were neither dead nor skipped; the loss kernel writes the taps MB_MU / MB_LOGITS / MB_VALUE of no other row, and what an
    unwritten row of a fresh workspace holds differs from process to process on one library"""
    out = {}
    names = list(_lib.PPO_FIELDS) + (list(_lib.POCA_FIELDS) if poca else [])
    if getattr(tr, "sequence_length", 0):
        names += list(_lib.PPO_RECURRENT_FIELDS) + (list(_lib.PPO_RECURRENT_CRITIC_FIELDS) if tr.critic_memory_size else [])
    for name in names:
        try:
            a = tr.read(name)
            if live is not None and name in ("mb_mu", "mb_logits", "mb_value"):
                a = a.reshape(live.size, -1)[live.reshape(-1)]
            out[name] = sha(a)
        except _lib.HkError as e:
            out[name] = "refused: %s" % e
    return out


def course(g, tr, n_ids, minibatch, poca):
    """advantages; one minibatch on ids that include out-of-range ones; update of 2 epochs; one update with both options; normaliser init and
    update; advantages again; then the recorded MU of a further 8-row rollout -> [(step, hashes)]"""
    import torch
    log = []

    def mark(step, **extra):
        log.append(dict(step=step, fields=fields(tr, poca), **{k: sha(np.asarray(v, np.float64)) if not isinstance(v, str) else v for k, v in extra.items()}))
    tr.advantages()
    mark("advantages")
    ids = np.random.default_rng(5).permutation(n_ids)[:min(n_ids, 300)].astype(np.int32)
    ids[[3, 77, 200]] = [n_ids, n_ids + 9, -1]
    st = tr.minibatch(torch.as_tensor(ids, device="cuda:0"), 0.2, 5e-3)
    mark("minibatch", stats=[st[k] for k in sorted(st)])
    st = tr.update(2, minibatch, 3e-4, 0.2, 5e-3)
    mark("update", stats=[st[k] for k in sorted(st)])
    st = tr.update(1, minibatch, 3e-4, 0.2, 5e-3, max_grad_norm=0.5, target_kl=0.02)
    rep = tr.last_report
    mark("update_opt", stats=[st[k] for k in sorted(st)], report=[float(rep[k]) for k in sorted(rep)])
    tr.normalizer_init()
    tr.normalizer_update()
    n, mean, m2 = tr.normalizer_state()
    mark("normalizer", state=np.concatenate([[n], mean, m2]))
    tr.advantages()
    mark("advantages again")
    g.rollout_begin(8)
    g.step(8 * P)
    g.rollout_close()
    log.append(dict(step="rollout of 8 rows", mu=sha(g.rollout()["mu"])))
    return log


def lstm_field():
    """the field of tests/test_ppo_lstm_gpu.py at tick 92: the envs with env % 4 == k restarted after k ticks, a recurrent actor on both karts"""
    c = LSTM_ENV
    g = hk.RacingEnv(hk.make_config(c["E"], 2, low_mode=[RL] * 2, rewards=1, max_episode_steps=100, jitter_seed=9))
    g.reset()
    H, m = c["actor"]
    g.attach_policy(Policy.random(g.obs_dim * 4, H, 2, 3, seed=4, memory_size=2 * m), [0, 1], P)
    for k in (1, 2, 3):
        g.step(1)
        g.reset(np.array([e for e in range(c["E"]) if e % 4 == k], np.int32))
    g.step(89)
    return g


def lstm_rollout(g, rows):
    g.rollout_begin(rows)
    g.step(rows * P)
    g.rollout_close()


def lstm_course(recurrent_critic):
    """advantages; one minibatch of sequence ids that include out-of-range ones; update of 2 epochs; one update with both options; normaliser init
    and update; publish; a second rollout and advantages again (a recurrent critic carries its memory); then the recorded MU and MEMORY of a
    further 3-row rollout -> [(step, hashes)]"""
    import torch
    c = LSTM_ENV
    g = lstm_field()
    lstm_rollout(g, c["R"])
    kw = {}
    if recurrent_critic:
        Hc, mv = c["critic"]
        kw = dict(critic=Policy.random(g.obs_dim * 4, Hc, 2, 1, seed=21, normalize=False, memory_size=2 * mv), critic_memory_size=2 * mv)
    tr = g.ppo_trainer(0, sequence_length=c["L"], **kw)
    n_seq = -(-c["R"] // c["L"]) * c["E"] * 2
    log = []
    last = []          # the sequence ids of the last minibatch

    def mark(step, **extra):
        live = None
        if len(last):          # [L][ms], time-major: the rows a window has, none for an id out of range
            live = np.zeros((c["L"], len(last)), bool)
            for q, s in enumerate(last):
                live[:len(ppo.sequence_rows(int(s), c["R"], c["L"], c["E"], 2)), q] = True
        log.append(dict(step=step, fields=fields(tr, False, live), **{k: sha(np.asarray(v, np.float64)) for k, v in extra.items()}))

    def update(**kw):
        # An update's last minibatch is taken to be the last whole one of PERM, its last epoch's permutation.  That rests on two rules of
        # hk_ppo_update / hk_ppo_update_opt (hk.h): the ragged tail of an epoch (n_seq % minibatch ids) is dropped, and the KL stop acts between
        # epochs, never inside one.  If either changes, the taps' hashes below cover the wrong rows
        st = tr.update(kw.pop("epochs"), 7, 3e-4, 0.2, 5e-3, **kw)
        last[:] = tr.read("perm")[(n_seq // 7 - 1) * 7:n_seq // 7 * 7]
        return st
    tr.advantages()
    mark("advantages")
    ids = np.random.default_rng(5).permutation(n_seq).astype(np.int32)
    ids[[3, 11, 20]] = [n_seq, n_seq + 9, -1]
    st = tr.minibatch(torch.as_tensor(ids, device="cuda:0"), 0.2, 5e-3)
    last[:] = ids
    mark("minibatch", stats=[st[k] for k in sorted(st)])
    st = update(epochs=2)
    mark("update", stats=[st[k] for k in sorted(st)])
    st = update(epochs=1, max_grad_norm=0.5, target_kl=0.02)
    rep = tr.last_report
    mark("update_opt", stats=[st[k] for k in sorted(st)], report=[float(rep[k]) for k in sorted(rep)])
    tr.normalizer_init()
    tr.normalizer_update()
    n, mean, m2 = tr.normalizer_state()
    mark("normalizer", state=np.concatenate([[n], mean, m2]))
    tr.publish()
    mark("publish")
    g.step(78)
    lstm_rollout(g, c["R"])
    tr.advantages()
    mark("second rollout, advantages")
    lstm_rollout(g, 3)
    ro = g.rollout()
    log.append(dict(step="rollout of 3 rows", mu=sha(ro["mu"]), memory=sha(ro["memory"])))
    return log


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the JSON here (default: stdout)")
    ap.add_argument("--courses", nargs="+", choices=COURSES, default=list(COURSES), help="the courses to run (default: all six)")
    a = ap.parse_args()
    import torch
    torch.cuda.init()                      # torch's HIP runtime first (see RacingEnv.torch_views)
    out = {}
    for prec in ("f32", "bf16"):
        if "ppo_" + prec in a.courses:
            g = env_of(PPO_ENV, False)
            out["ppo " + prec] = course(g, g.ppo_trainer(0, precision=prec), R * PPO_ENV["E"] * 2, 512, False)
    for case, c in POCA_ENVS.items():
        if "poca_" + case in a.courses:
            g = env_of(c, True)
            pol = g._policies[0]
            out["poca " + case] = course(g, g.poca_trainer(0, critic=PocaCritic.random(pol.in_dim, pol.n_branch, c["H"], c["L"], 3)), R * c["E"], 256, True)
    for name in ("lstm", "lstm_critic"):
        if name in a.courses:
            out[name] = lstm_course(name == "lstm_critic")
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
