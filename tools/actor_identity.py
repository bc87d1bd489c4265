#!/usr/bin/env python3
"""What a refactor of the actor kernels must leave bit for bit: one fixed course through every actor kernel — policy_mlp_kernel<0 / 1 / 2>,
policy_mlp_bf16_kernel<false / true>, policy_lstm_kernel, and the stack / memory / recorder kernels around them — with a SHA-256 of every
output, printed as one JSON document.  Run it once per library, each in a fresh process, and compare the two outputs byte for byte:

    HK_LIB_PATH=build/libhk_parent.so python tools/actor_identity.py --out a.json
    python tools/actor_identity.py --out b.json && cmp a.json b.json

The course: hk_policy_forward at rows 1, 64, 65 and 130 for the nine shapes of tests/test_policy_gpu.py::test_actor_bit_exact (MODE 0 / 1 / 2;
one, two and three input chunks; a K remainder modulo 8), in f32 and after hk_policy_set_precision bf16; hk_policy_forward_mem for the (H, m)
of tests/test_policy_lstm_gpu.py::test_forward_against_the_twin; one recorded rollout of 12 rows at 70 envs with a recurrent and a plain
sampled actor on one handle (every HK_RO_* field and the final hk_policy_memory_get).  The shapes are restated here so that the tool stands
without the tests.  tools/trainer_identity.py is its sibling for the trainers (hk_ppo_publish, RING0)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hierarchicalkarting_amd as hk
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy

RL, P = _lib.HK_LOW_RL, 2
ROWS = (1, 64, 65, 130)
# (agents, stack, hidden, layers, normalize)
MLP_SHAPES = [(2, 4, 128, 3, True), (4, 4, 256, 3, True), (4, 8, 256, 3, True), (2, 4, 64, 1, False), (2, 4, 192, 2, True), (2, 4, 32, 4, True),
              (4, 1, 256, 2, True), (4, 7, 256, 2, True), (2, 3, 96, 2, False)]
LSTM_SHAPES = [(32, 32), (128, 128), (256, 64), (96, 96), (256, 128), (160, 32)]          # (hidden, m)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def env(E, A, **kw):
    g = hk.RacingEnv(hk.make_config(E, A, low_mode=[RL] * A, **kw))
    g.reset()
    return g


def observations(rows, in_dim, seed):
    obs = (np.random.default_rng(seed).standard_normal((rows, in_dim)) * 4).astype(np.float32)
    obs[0, :7] = [0.0, -0.0, 1e-30, -1e30, 5.0, -5.0, 1e30]
    return obs


def forward_mlp():
    out = {}
    for A, stack, hidden, layers, normalize in MLP_SHAPES:
        g = env(2, A)
        in_dim = g.obs_dim * stack
        k = g.attach_policy(Policy.random(in_dim, hidden, layers, stack=stack, seed=hidden + stack, normalize=normalize), [0], P)
        for prec in ("f32", "bf16"):
            g.policy_set_precision(k, prec)
            for rows in ROWS:
                mu, lg = g.policy_forward(k, observations(rows, in_dim, rows))
                out["%d->%dx%d %s rows %d" % (in_dim, hidden, layers, prec, rows)] = {"mu": sha(mu), "logits": sha(lg)}
        g.close()
    return out


def forward_lstm():
    out = {}
    for H, m in LSTM_SHAPES:
        g = env(2, 2)
        D = g.obs_dim
        pols = [Policy.random(D * 2, H, 2, 3, stack=2, seed=H + m, memory_size=2 * m),
                Policy.random(D * 4, H, 3, 3, stack=4, seed=H + m + 1, memory_size=2 * m, normalize=(H != 96))]
        for k, pol in enumerate(pols):
            g.attach_policy(pol, [k], P)
            for rows in ROWS:
                mem = np.random.default_rng(7 * H + m + rows).uniform(-1.0, 1.0, (rows, 2 * m)).astype(np.float32)
                mu, lg, mem_out = g.policy_forward(k, observations(rows, pol.in_dim, rows), mem)
                out["%d->%dx%d m %d rows %d" % (pol.in_dim, H, len(pol.W), m, rows)] = {"mu": sha(mu), "logits": sha(lg), "mem_out": sha(mem_out)}
        g.close()
    return out


def rollout():
    g = env(70, 2, rewards=1, max_episode_steps=100, jitter_seed=3)
    D = g.obs_dim
    g.attach_policy(Policy.random(D * 4, 128, 3, 3, seed=4, memory_size=256), [0], P)
    g.attach_policy(Policy.random(D * 4, 128, 3, 3, seed=5), [1], P)
    g.step(90)                             # time-outs at tick 100: episode ends, FIRST and cleared memory inside the rollout
    g.rollout_begin(12)
    g.step(12 * P)
    g.rollout_close()
    out = {name: sha(a) for name, a in g.rollout().items()}
    out["hk_policy_memory_get"] = sha(g.policy_memory(0))
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the JSON here (default: stdout)")
    a = ap.parse_args()
    out = {"hk_policy_forward": forward_mlp(), "hk_policy_forward_mem": forward_lstm(), "rollout of 12 rows": rollout()}
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
