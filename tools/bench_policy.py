#!/usr/bin/env python3
"""Time the actor's inference kernel alone (HIP events around the launch, via hk_prof) inside the decision loop of a 4-agent env:
rows per launch = E * 4 (one actor drives every agent).  --policy-precision f32 bf16 alternates the two chains (hk_policy_set_precision) in
one process, window by window; per shape and precision the median per-launch time of --repeats windows of 200 ticks, and their min / max."""
import argparse, sys, os, json, statistics
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hierarchicalkarting_amd as hk
from hierarchicalkarting_amd import _lib
from hierarchicalkarting_amd.policy import Policy

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("envs", type=int, nargs="?", default=32768)
ap.add_argument("--policy-precision", nargs="+", choices=("f32", "bf16"), default=["f32"], help="hk_policy_set_precision; several: alternated")
ap.add_argument("--repeats", type=int, default=5, help="windows per precision (>= 5 for a spread)")
a = ap.parse_args()
E = a.envs
out = {}
for (A, stack, hidden, layers) in ((4, 4, 256, 3), (4, 4, 128, 3), (4, 8, 256, 3), (4, 4, 192, 3)):      # (hidden 192: policy_mlp_kernel<2>)
    env = hk.RacingEnv(hk.make_config(E, A, low_mode=[_lib.HK_LOW_RL] * A, jitter_seed=1))
    in_dim = env.obs_dim * stack
    pol = Policy.random(in_dim, hidden, layers, stack=stack, seed=1)
    env.attach_policy(pol, list(range(A)), 2)
    env.reset()
    env.step(100)
    env.prof_enable(True)
    runs = {prec: [] for prec in a.policy_precision}
    obs_ms = []
    for prec in a.policy_precision:           # (first launches, and the bf16 copies, outside the windows)
        env.policy_set_precision(0, prec)
        env.step(20)
    for _ in range(a.repeats):
        for prec in a.policy_precision:
            env.policy_set_precision(0, prec)
            env.prof_reset()
            env.step(200)
            pr = env.prof_read()
            ms, n = pr["policy_mlp_kernel"]
            runs[prec].append(ms / n)
            obs_ms.append(pr["observe+stack"][0] / max(pr["observe+stack"][1], 1))
    rows = E * A
    flop = rows * 2.0 * (in_dim * hidden + (layers - 1) * hidden * hidden + 4 * hidden)
    key = "%d->%dx%d" % (in_dim, hidden, layers)
    res = {}
    for prec, v in runs.items():
        med = statistics.median(v)
        res[prec] = {"ms": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "tflops": round(flop / (med * 1e-3) / 1e12, 1)}
    if list(runs) == ["f32"]:
        out[key] = dict(res["f32"], obs_ms=round(statistics.median(obs_ms), 4))
    else:
        out[key] = dict(res, obs_ms=round(statistics.median(obs_ms), 4))
        if "f32" in res and "bf16" in res:
            out[key]["bf16_over_f32"] = round(res["bf16"]["ms"] / res["f32"]["ms"], 3)
    env.close()
print(os.path.basename(os.environ.get("HK_LIB_PATH", "default")), json.dumps(out))
