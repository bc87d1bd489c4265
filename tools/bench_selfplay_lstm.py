#!/usr/bin/env python3
"""What an opponent swap of a recurrent actor costs: one hk_policy_pool_save + hk_policy_pool_load of a recurrent pool's slot at
obs_dim * 4 = 312 -> 128 x 3, m = 128, beside the feed-forward pool's save + load of the same trunk (an unchanged path: what it cost before
recurrent pools existed).  ONE handle of `--envs` envs, 4 karts, four attached actors: two plain and two with the cell.  A window is `--pairs`
save + load pairs issued back to back and one device synchronise; windows of the two kinds alternate, `--repeats` of each.  With
--clear a third kind adds hk_policy_memory_clear after every recurrent load (what SelfPlay(reset_opponent_memory=True) issues).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
A, P, H, M = 4, 2, 128, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clear", action="store_true")
    a = ap.parse_args()
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    env = hk.RacingEnv(hk.make_config(a.envs, A, low_mode=[_lib.HK_LOW_RL] * A, jitter_seed=0x5EED0000))
    in_dim = env.obs_dim * 4
    for k in range(2):
        env.attach_policy(Policy.random(in_dim, H, 3, seed=101 + k), [k], P)
    for k in range(2):
        env.attach_policy(Policy.random(in_dim, H, 3, seed=201 + k, memory_size=2 * M), [2 + k], P)
    env.reset()
    env.step(8)
    pools = {"feed_forward": (env.snapshot_pool(0, 2), 0, 1), "recurrent": (env.snapshot_pool(2, 2), 2, 3)}
    kinds = ["feed_forward", "recurrent"] + (["recurrent_clear"] if a.clear else [])

    def window(kind):
        pool, src, dst = pools[kind.replace("_clear", "")]
        env.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.pairs):
            pool.save(0, src)
            pool.load(0, dst)
            if kind.endswith("_clear"):
                env.policy_memory_clear(dst)
        env.synchronize()
        return (time.perf_counter() - t0) / a.pairs

    for kind in kinds:          # one window of each first, not counted
        window(kind)
    times = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for kind in kinds:
            times[kind].append(window(kind))
    out = {"shape": "%d -> %d x 3, m = %d" % (in_dim, H, M), "envs": a.envs, "pairs_per_window": a.pairs, "windows": a.repeats,
           "slot_floats": {k: pools[k][0].count for k in pools}}
    for kind in kinds:
        out[kind + "_us"] = {"median": 1e6 * statistics.median(times[kind]), "min": 1e6 * min(times[kind]), "max": 1e6 * max(times[kind])}
    out["recurrent_over_feed_forward"] = out["recurrent_us"]["median"] / out["feed_forward_us"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
