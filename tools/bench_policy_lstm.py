#!/usr/bin/env python3
"""What a recurrent actor costs: the RL workload's field — 16 384 envs, 2v2 Oval, every agent LowMode RL, DecisionPeriod 2 —
with one actor per team of obs_dim * 4 -> 128 x 3, once plain and once with the same trunks + an LSTM of m = 128 (memory_size 256).
One process, two handles on the same config: windows of K hk_step(R * 2) calls alternate between the plain and the recurrent handle,
`--repeats` of each, every window ending in a device synchronise.  Then, by the protocol of tools/bench_rollout.py, windows of K rollouts of
R rows recorded against the same calls unrecorded, on both handles: the recurrent one's rows carry MEMORY (4 * 2m bytes per agent and row).
Last, unless --no-profile, a child process of its own under `rocprofv3 --kernel-trace --stats` (this program with --profile-child, started
after both handles are closed) gives the time per launch of policy_lstm_kernel against policy_mlp_kernel<0>, the yardstick in that same
run; the multiply-adds per row, in_dim H + 2 H H for the trunk and (H + m) 4m more for the cell, are printed with their ratio (3.17 at
in_dim 216, 2.80 at the 312 inputs of this 4-agent field).  One JSON line.
--bf16 adds a third handle whose recurrent actors run in HK_POLICY_PREC_BF16 (hk_policy_lstm_set_precision), its windows alternated
with the other two, and policy_lstm_bf16_kernel's row of the kernel trace."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
A, P, H, M = 4, 2, 128, 128


def make(envs, recurrent, bf16=False):
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    env = hk.RacingEnv(hk.make_config(envs, A, low_mode=[_lib.HK_LOW_RL] * A, jitter_seed=0x5EED0000, rewards=1))
    in_dim = env.obs_dim * 4
    for seed, slots in ((101, [0, 1]), (202, [2, 3])):
        env.attach_policy(Policy.random(in_dim, H, 3, seed=seed, memory_size=2 * M if recurrent else 0), slots, P)
    if bf16:
        for i in (0, 1):
            env.policy_lstm_set_precision(i, "bf16")
    env.reset()
    return env


def profile_child(a):
    """both handles, a few hundred decisions each: the kernel trace's rows are what the parent reads"""
    for recurrent, bf16 in ((False, False), (True, False)) + (((True, True),) if a.bf16 else ()):
        env = make(a.envs, recurrent, bf16)
        env.step(a.warmup - a.warmup % P)
        env.step(a.rows * P * 4)
        env.synchronize()
        env.close()


def kernel_times(outdir):
    """-> {kernel name fragment: (calls, mean ns per launch)} from the *kernel_stats.csv rocprofv3 wrote under outdir"""
    out = {}
    for d, _, files in os.walk(outdir):
        for f in files:
            if not f.endswith("kernel_stats.csv"):
                continue
            for row in csv.DictReader(open(os.path.join(d, f))):
                name = row.get("Name", "")
                for frag in ("policy_lstm_kernel", "policy_lstm_bf16_kernel", "policy_mlp_kernel<0>", "policy_memory_kernel", "policy_stack_kernel"):
                    if frag in name:
                        calls = int(row["Calls"])
                        out[frag] = (calls, float(row["TotalDurationNs"]) / calls)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=64, help="R: decisions per hk_step call / rows per rollout")
    ap.add_argument("--calls", type=int, default=8, help="K: calls (rollouts) per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="windows per mode (>= 5)")
    ap.add_argument("--warmup", type=int, default=256, help="untimed ticks before the first window")
    ap.add_argument("--bf16", action="store_true", help="also run the recurrent actors in HK_POLICY_PREC_BF16 on a third handle (DESIGN §20)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-dir", default=None, help="where the child's kernel trace is written and kept (default: a temporary directory)")
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.profile_child:
        return profile_child(a)
    E, R, K = a.envs, a.rows, a.calls
    envs = {"plain": make(E, False), "lstm": make(E, True), **({"lstm_bf16": make(E, True, True)} if a.bf16 else {})}
    for env in envs.values():
        env.step(a.warmup - a.warmup % P)
        env.rollout_begin(R); env.step(R * P); env.rollout_close()        # (allocates the rows; first launches of every kernel)
        env.synchronize()
    ticks = K * R * P

    def window(env, record):
        t0 = time.perf_counter()
        for _ in range(K):
            if record:
                env.rollout_begin(R)
            env.step(R * P)
            if record:
                env.rollout_close()
        env.synchronize()
        return E * ticks / (time.perf_counter() - t0)

    rates = {k: {"off": [], "on": []} for k in envs}
    for _ in range(a.repeats):
        for k, env in envs.items():
            rates[k]["off"].append(window(env, False))
            rates[k]["on"].append(window(env, True))
    obs_dim = envs["plain"].obs_dim
    for env in envs.values():
        env.close()
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    med = lambda k, m: statistics.median(rates[k][m])
    out = {"metric": "env-steps/s, plain actors against the same trunks + LSTM (m = 128); rollout recording off / on", "unit": "env-steps/s",
           "plain": {m: stat(v) for m, v in rates["plain"].items()}, "lstm": {m: stat(v) for m, v in rates["lstm"].items()},
           **({"lstm_bf16": {m: stat(v) for m, v in rates["lstm_bf16"].items()}, "lstm_bf16_over_lstm_env_steps": med("lstm_bf16", "off") / med("lstm", "off")}
              if a.bf16 else {}),
           "lstm_over_plain_env_steps": med("lstm", "off") / med("plain", "off"),
           "recording_overhead": {k: 1.0 - med(k, "on") / med(k, "off") for k in rates},
           "config": {"envs": E, "agents": A, "decision_period": P, "in_dim": obs_dim * 4, "hidden": H, "layers": 3, "m": M, "rows": R, "calls_per_window": K,
                      "ticks_per_window": ticks, "repeats": a.repeats, "memory_row_bytes_per_agent": 4 * 2 * M, "obs_row_bytes_per_agent": 4 * obs_dim,
                      "multiply_adds_per_row": {"plain": obs_dim * 4 * H + 2 * H * H, "lstm": obs_dim * 4 * H + 2 * H * H + (H + M) * 4 * M}}}
    if not a.no_profile:
        import shutil
        import tempfile
        if a.profile_dir is None:
            a.profile_dir = tempfile.mkdtemp(prefix="bench_policy_lstm_trace_")
        os.makedirs(a.profile_dir, exist_ok=True)
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.profile_dir, "--", sys.executable, os.path.abspath(__file__), "--profile-child",
               "--envs", str(E), "--rows", str(R), "--warmup", str(a.warmup)] + (["--bf16"] if a.bf16 else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("rocprofv3 failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        kt = kernel_times(a.profile_dir)
        if "policy_lstm_kernel" not in kt or "policy_mlp_kernel<0>" not in kt:
            raise SystemExit("the kernel trace under %s has no policy_lstm_kernel / policy_mlp_kernel<0> row: %s" % (a.profile_dir, sorted(kt)))
        ma = out["config"]["multiply_adds_per_row"]
        out["kernel_trace"] = {k: {"calls": c, "mean_us_per_launch": ns / 1e3} for k, (c, ns) in kt.items()}
        out["lstm_over_mlp_kernel_time"] = kt["policy_lstm_kernel"][1] / kt["policy_mlp_kernel<0>"][1]
        if "policy_lstm_bf16_kernel" in kt:
            out["lstm_bf16_over_lstm_kernel_time"] = kt["policy_lstm_bf16_kernel"][1] / kt["policy_lstm_kernel"][1]
        out["multiply_add_ratio"] = ma["lstm"] / ma["plain"]
        out["expected_at_most"] = 1.25 * ma["lstm"] / ma["plain"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
