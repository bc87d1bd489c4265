#!/usr/bin/env python3
"""What a POCA update costs beside a PPO update, on the RL workload's shape (16 384 envs of 2v2 Oval, every agent LowMode RL, a 312 -> 256 x 3
actor on team 0's two slots, DecisionPeriod 2, rewards on, R = 64 rows): ONE rollout is collected, then a POCA trainer (attention critic
H = 256, 2 layers) and a PPO trainer (critic 312 -> 256 x 3) of that policy each time one advantages() plus update(3 epochs) at ML-Agents'
batch_size — 512 groups for POCA, the same 1024 agent rows for PPO.  --repeats rounds, the two trainers alternating inside a round, every
window closed by a device synchronise; median and range per trainer, one JSON line.
--trace: no timing; one advantages() and a one-epoch update of the POCA trainer alone, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/bench_poca.py --trace); tools/kernel_stats.py-style shares are then read off the stats file:
the kernels named poca_* are the new non-matrix kernels, ppo_gemm_kernel the matrix products."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=64, help="R: rows (decisions) per rollout")
    ap.add_argument("--groups", type=int, default=512, help="POCA minibatch in groups; PPO takes the same agent rows")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace", action="store_true", help="one untimed POCA advantages + one-epoch update (for a profiler run of its own)")
    a = ap.parse_args()
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    E, A, P, R, S = a.envs, 4, 2, a.rows, 2
    env = hk.RacingEnv(hk.make_config(E, A, low_mode=[_lib.HK_LOW_RL] * A, jitter_seed=0x5EED0000, rewards=1))
    in_dim = env.obs_dim * 4
    env.attach_policy(Policy.random(in_dim, 256, 3, seed=101), [0, 1], P)
    env.attach_policy(Policy.random(in_dim, 256, 3, seed=202), [2, 3], P)
    env.reset()
    env.step(256)
    env.synchronize()
    t0 = time.perf_counter()
    env.rollout_begin(R); env.step(R * P); env.rollout_close()
    env.synchronize()
    collect_ms = (time.perf_counter() - t0) * 1e3
    poca = env.poca_trainer(0, seed=1)
    if a.trace:
        poca.advantages()
        poca.update(1, a.groups, 1e-5, 0.2, 5e-3)
        env.synchronize()
        env.close()
        return
    ppo = env.ppo_trainer(0, seed=1)
    trainers = {"poca": (poca, a.groups), "ppo": (ppo, a.groups * S)}

    def timed(f):
        env.synchronize()
        t = time.perf_counter()
        f()
        env.synchronize()
        return (time.perf_counter() - t) * 1e3

    for tr, mb in trainers.values():          # allocate the workspaces; first launches
        tr.advantages()
        tr.update(1, mb, 1e-5, 0.2, 5e-3)
    runs = {k: {"adv": [], "upd": []} for k in trainers}
    for _ in range(a.repeats):
        for k, (tr, mb) in trainers.items():
            runs[k]["adv"].append(timed(tr.advantages))
            runs[k]["upd"].append(timed(lambda: tr.update(a.epochs, mb, 1e-5, 0.2, 5e-3)))
    env.close()
    out = {"metric": "POCA beside PPO: advantages + update(%d epochs) on one rollout of the RL workload" % a.epochs, "collect_ms": collect_ms,
           "config": {"envs": E, "agents": A, "rows": R, "agent_rows": R * E * S, "groups": R * E, "poca_minibatch_groups": a.groups,
                      "ppo_minibatch_rows": a.groups * S, "epochs": a.epochs, "repeats": a.repeats}}
    for k, r in runs.items():
        tot = [x + y for x, y in zip(r["adv"], r["upd"])]
        out[k] = {"advantages_ms": statistics.median(r["adv"]), "advantages_range": [min(r["adv"]), max(r["adv"])],
                  "update_ms": statistics.median(r["upd"]), "update_range": [min(r["upd"]), max(r["upd"])],
                  "total_ms": statistics.median(tot), "total_range": [min(tot), max(tot)]}
    out["poca_over_ppo"] = out["poca"]["total_ms"] / out["ppo"]["total_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
