#!/usr/bin/env python3
"""What recording a rollout costs on the RL workload (bench.py --workload rl: 2v2 Oval, every agent LowMode RL, one 312 -> 256 x 3 actor per
team, DecisionPeriod 2), here with reward shaping on (rewards=1).  One process, one handle: windows of K back-to-back rollouts of R rows
(hk_rollout_begin, ONE hk_step(R * 2), hk_rollout_close) alternate with windows of the same hk_step calls unrecorded, `--repeats` of each;
every window ends in a device synchronise.  For contrast, a second handle without actors runs the host-driven loop of
tests/test_device_loop_gpu.py over the same number of decisions (hk_observe, hk_step(2), hk_rewards_device, hk_synchronize per decision —
no actor runs there, so it times the loop and the env alone).  One JSON line: env-steps/s medians, min / max and the recording overhead."""
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
    ap.add_argument("--rollouts", type=int, default=8, help="K: rollouts per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="windows per mode (>= 5)")
    ap.add_argument("--warmup", type=int, default=256, help="untimed ticks before the first window")
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--policy-precision", nargs="+", choices=("f32", "bf16"), default=["f32"],
                    help="hk_policy_set_precision of both actors; several: alternated window by window, reported per precision")
    a = ap.parse_args()
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    E, A, P, R, K = a.envs, 4, 2, a.rows, a.rollouts
    kw = dict(low_mode=[_lib.HK_LOW_RL] * A, jitter_seed=0x5EED0000, rewards=1)
    env = hk.RacingEnv(hk.make_config(E, A, **kw))
    in_dim = env.obs_dim * 4
    env.attach_policy(Policy.random(in_dim, 256, 3, seed=101), [0, 1], P)
    env.attach_policy(Policy.random(in_dim, 256, 3, seed=202), [2, 3], P)
    env.reset()
    env.step(a.warmup - a.warmup % P)
    env.rollout_begin(R); env.step(R * P); env.rollout_close()        # (allocates the rows; first launches of the recording kernels)
    env.synchronize()
    ticks = K * R * P

    def window(record):
        t0 = time.perf_counter()
        for _ in range(K):
            if record:
                env.rollout_begin(R)
            env.step(R * P)
            if record:
                env.rollout_close()
        env.synchronize()
        return E * ticks / (time.perf_counter() - t0)

    precs = list(dict.fromkeys(a.policy_precision))
    by_prec = {p: {"off": [], "on": []} for p in precs}

    def set_precision(p):
        for k in (0, 1):
            env.policy_set_precision(k, p)

    if precs != ["f32"]:
        for p in precs[1:] + precs[:1]:       # (the bf16 copies and every kernel's first launch, outside the windows)
            set_precision(p)
            env.step(4 * P)
    for _ in range(a.repeats):
        for p in precs:
            if len(precs) > 1 or p != "f32":
                set_precision(p)
            by_prec[p]["off"].append(window(False))
            by_prec[p]["on"].append(window(True))
    env.close()
    rates = by_prec[precs[0]]
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    out = {"metric": "env-steps/s, rollout recording off / on (RL workload, rewards on)", "unit": "env-steps/s",
           "off": stat(rates["off"]), "on": stat(rates["on"]),
           "overhead": 1.0 - statistics.median(rates["on"]) / statistics.median(rates["off"]),
           "config": {"envs": E, "agents": A, "decision_period": P, "rows": R, "rollouts_per_window": K, "ticks_per_window": ticks,
                      "repeats": a.repeats, "policy_precision": precs[0], "row_bytes_per_env_step": A * (env.obs_dim + 9 + 3 + 2) * 4 / P}}
    if len(precs) > 1:
        out["by_policy_precision"] = {p: {"off": stat(r["off"]), "on": stat(r["on"])} for p, r in by_prec.items()}
        if "f32" in by_prec and "bf16" in by_prec:
            out["bf16_over_f32_env_steps"] = {m: statistics.median(by_prec["bf16"][m]) / statistics.median(by_prec["f32"][m]) for m in ("off", "on")}
    if not a.no_host_loop:
        h = hk.RacingEnv(hk.make_config(E, A, **kw))
        h.reset()
        h.step(a.warmup - a.warmup % P)
        h.synchronize()
        host = []
        for _ in range(max(1, a.repeats // 2)):
            t0 = time.perf_counter()
            for _ in range(R):
                h.observe(); h.step(P); h.rewards_device(); h.synchronize()
            host.append(E * R * P / (time.perf_counter() - t0))
        h.close()
        out["host_loop"] = stat(host)
        out["host_loop"]["note"] = "hk_observe + hk_step(2) + hk_rewards_device + hk_synchronize per decision, no actor"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
