#!/usr/bin/env python3
"""What a host-side refactor of the trainers must leave bit for bit: one fixed course through the PPO trainer (f32, then bf16) and the POCA
trainer, with a SHA-256 of every readable trainer field, of the returned stats and of the update report after each step, printed as one JSON
document.  Run it once per library, each in a fresh process, and compare the two outputs byte for byte:

    HK_LIB_PATH=build/libhk_parent.so python tools/trainer_identity.py --out a.json
    python tools/trainer_identity.py --out b.json && cmp a.json b.json

Under `rocprofv3 --kernel-trace --stats` the same course gives the launch counts to compare.  The set-ups are those of tests/test_ppo_gpu.py
(24 envs of 2v2, R = 90) and the h36 and s4 cases of tests/test_poca_gpu.py, restated here so that the tool stands without the tests."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hierarchicalkarting_amd as hk
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.poca import PocaCritic
from hierarchicalkarting_amd.policy import Policy

RL, P, R = _lib.HK_LOW_RL, 2, 90
PPO_ENV = dict(E=24, A=4, slots=[0, 1], other=[2, 3], actor=(256, 3), other_actor=(128, 2), kw={})
POCA_ENVS = {
    "h36": dict(E=24, A=4, slots=[0, 1], other=[2, 3], actor=(256, 3), other_actor=(64, 2), H=36, L=1),
    "s4": dict(E=8, A=8, slots=[0, 1, 2, 3], other=[4, 5, 6, 7], actor=(64, 2), other_actor=(64, 2), H=64, L=2),
}
TRAINING = dict(env_mode=_lib.HK_MODE_TRAINING)


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


def fields(tr, poca):
    """name -> SHA-256 of the field, or the library's refusal where it is not readable yet"""
    out = {}
    for name in list(_lib.PPO_FIELDS) + (list(_lib.POCA_FIELDS) if poca else []):
        try:
            out[name] = sha(tr.read(name))
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the JSON here (default: stdout)")
    a = ap.parse_args()
    import torch
    torch.cuda.init()                      # torch's HIP runtime first (see RacingEnv.torch_views)
    out = {}
    for prec in ("f32", "bf16"):
        g = env_of(PPO_ENV, False)
        out["ppo " + prec] = course(g, g.ppo_trainer(0, precision=prec), R * PPO_ENV["E"] * 2, 512, False)
    for case, c in POCA_ENVS.items():
        g = env_of(c, True)
        pol = g._policies[0]
        out["poca " + case] = course(g, g.poca_trainer(0, critic=PocaCritic.random(pol.in_dim, pol.n_branch, c["H"], c["L"], 3)), R * c["E"], 256, True)
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
