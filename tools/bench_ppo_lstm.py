#!/usr/bin/env python3
"""What recurrent training costs: one hk_ppo_update (3 epochs) on a 16 384-env 2v2 Oval rollout of R = 64 rows, every agent
LowMode RL, DecisionPeriod 2.  ONE handle, two actors of obs_dim * 4 = 312 -> 128 x 3: team 0 plain with a plain trainer, team 1 with an LSTM of
m = 128 and a recurrent trainer at sequence_length 64.  Both trainers see the same number of rows per minibatch (--minibatch-rows; the
recurrent one takes minibatch-rows / 64 sequences).  Windows of one update each alternate between the two trainers, `--repeats` of each, every
window ending in a device synchronise; advantages are computed once, outside the windows.  Last, unless --no-profile, a child process of its own
under `rocprofv3 --kernel-trace --stats` (this program with --profile-child) gives the time per launch of the two step kernels.  The
multiply-adds per row, in_dim H + 2 H H for the trunk and 4m (H + m) more for the cell, are printed with their ratio.  One JSON line.
--critic adds, on the same handle and actor, two trainers with a RECURRENT CRITIC (m_v = 128; value_chunk_steps at its default and
at 1) and times, windows alternated: hk_ppo_advantages of the recurrent-critic trainer against the recurrent trainer with the feed-forward critic
(to hold against the same multiply-add ratio), the same value pass at value_chunk_steps = 1 (what the multi-step launch buys), and one
hk_ppo_update of the recurrent-critic trainer beside the other two; the kernel trace then lists ppo_lstm_value_kernel too.
--precision: f32 (the default: everything above, unchanged), bf16 (the recurrent trainer runs in HK_PPO_PREC_BF16,
hk_ppo_recurrent_set_precision) or both (a second recurrent trainer "lstm_bf16" on the same actor, its windows alternated with the others'); the
kernel trace then lists the bf16 step and backward kernels and ppo_gemm_bf16_kernel beside the fp32 ones."""
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
A, P, H, M, L = 4, 2, 128, 128, 64


def make(envs, rows, critic=False, precision="f32"):
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    env = hk.RacingEnv(hk.make_config(envs, A, low_mode=[_lib.HK_LOW_RL] * A, jitter_seed=0x5EED0000, rewards=1))
    in_dim = env.obs_dim * 4
    env.attach_policy(Policy.random(in_dim, H, 3, seed=101), [0, 1], P)
    env.attach_policy(Policy.random(in_dim, H, 3, seed=202, memory_size=2 * M), [2, 3], P)
    env.reset()
    env.step(256)
    env.rollout_begin(rows); env.step(rows * P); env.rollout_close()
    tr = {"plain": env.ppo_trainer(0, seed=1), "lstm": env.ppo_trainer(1, sequence_length=L, seed=1)}
    if precision == "bf16":
        tr["lstm"].set_recurrent_precision("bf16")
    elif precision == "both":
        tr["lstm_bf16"] = env.ppo_trainer(1, sequence_length=L, seed=1)
        tr["lstm_bf16"].set_recurrent_precision("bf16")
    if critic:
        for name, chunk in (("critic", 0), ("critic_chunk1", 1)):
            tr[name] = env.ppo_trainer(1, critic=Policy.random(in_dim, H, 3, n_branch=1, seed=303, normalize=False, memory_size=2 * M), sequence_length=L,
                                       critic_memory_size=2 * M, value_chunk_steps=chunk, seed=1)
    for t in tr.values():
        t.advantages()
    env.synchronize()
    return env, tr


def update(tr, kind, a):
    mb = a.minibatch_rows if kind == "plain" else max(1, a.minibatch_rows // L)          # (every recurrent kind counts sequences)
    tr[kind].update(a.epochs, mb, 3e-4, 0.2, 5e-3)


def profile_child(a):
    env, tr = make(a.envs, a.rows, a.critic, a.precision)
    for kind in tr:
        if kind != "critic_chunk1":
            update(tr, kind, a)
    for kind in tr:
        tr[kind].advantages()
    env.synchronize()
    env.close()


def kernel_times(outdir):
    out = {}
    for d, _, files in os.walk(outdir):
        for f in files:
            if not f.endswith("kernel_stats.csv"):
                continue
            for row in csv.DictReader(open(os.path.join(d, f))):
                name = row.get("Name", "")
                for frag in ("ppo_lstm_step_kernel", "ppo_lstm_back_kernel", "ppo_loss_kernel", "ppo_lstm_value_kernel", "ppo_lstm_step_bf16_kernel",
                             "ppo_lstm_back_bf16_kernel", "ppo_gemm_bf16_kernel<0>", "ppo_gemm_bf16_kernel<1>", "ppo_gemm_bf16_kernel<2>", "ppo_gemm_kernel<0>",
                             "ppo_combine_kernel"):
                    if frag in name:
                        calls = int(row["Calls"])
                        out[frag] = (calls, float(row["TotalDurationNs"]) / calls)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=64, help="R: rows of the rollout")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--minibatch-rows", type=int, default=16384, help="rows per minibatch of both trainers (a multiple of 64)")
    ap.add_argument("--repeats", type=int, default=5, help="windows per trainer (>= 5)")
    ap.add_argument("--critic", action="store_true", help="also time the trainers with a recurrent critic (DESIGN §18)")
    ap.add_argument("--precision", choices=("f32", "bf16", "both"), default="f32", help="the recurrent trainer's precision (DESIGN §20)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-dir", default=None)
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.profile_child:
        return profile_child(a)
    env, tr = make(a.envs, a.rows, a.critic, a.precision)
    in_dim = env.obs_dim * 4
    upd = [k for k in tr if k != "critic_chunk1"]          # (value_chunk_steps changes nothing in an update)
    for kind in upd:                     # untimed: allocates the workspaces, first launches of every kernel
        update(tr, kind, a)
        tr[kind].advantages()
    env.synchronize()
    adv = {k: [] for k in tr if k not in ("plain", "lstm_bf16")} if a.critic else {}
    for kind in adv:
        tr[kind].advantages()
    env.synchronize()
    for _ in range(a.repeats):           # the value passes, alternated; a repeated call on one rollout starts from the same MEM_IN
        for kind in adv:
            t0 = time.perf_counter()
            tr[kind].advantages()
            env.synchronize()
            adv[kind].append(time.perf_counter() - t0)
    secs = {k: [] for k in upd}
    for _ in range(a.repeats):
        for kind in upd:
            t0 = time.perf_counter()
            update(tr, kind, a)
            env.synchronize()
            secs[kind].append(time.perf_counter() - t0)
            tr[kind].advantages()        # (outside the window; the published actor did not record this rollout, which changes no launch)
            env.synchronize()
    env.close()
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    ma = {"plain": in_dim * H + 2 * H * H, "lstm": in_dim * H + 2 * H * H + 4 * M * (H + M)}
    n_rows = a.rows * a.envs * 2
    out = {"metric": "seconds per hk_ppo_update, a plain trainer against a recurrent one (truncated BPTT, L = 64) on one handle", "unit": "s",
           "plain": stat(secs["plain"]), "lstm": stat(secs["lstm"]), **({"critic": stat(secs["critic"])} if a.critic else {}),
           **({"lstm_bf16": stat(secs["lstm_bf16"]), "lstm_bf16_over_lstm_update_time": statistics.median(secs["lstm_bf16"]) / statistics.median(secs["lstm"])}
              if "lstm_bf16" in secs else {}),
           "lstm_over_plain_update_time": statistics.median(secs["lstm"]) / statistics.median(secs["plain"]),
           "multiply_add_ratio": ma["lstm"] / ma["plain"],
           "config": {"envs": a.envs, "agents": A, "rows": a.rows, "rows_per_trainer": n_rows, "epochs": a.epochs, "minibatch_rows": a.minibatch_rows,
                      "sequence_length": L, "sequences_per_minibatch": max(1, a.minibatch_rows // L), "in_dim": in_dim, "hidden": H, "layers": 3, "m": M,
                      "step_launches_per_minibatch": 2 * L, "repeats": a.repeats, "multiply_adds_per_row": ma, "precision": a.precision}}
    if a.critic:
        med = {k: statistics.median(v) for k, v in adv.items()}
        out["advantages_seconds"] = {k: stat(v) for k, v in adv.items()}
        out["critic_over_lstm_advantages_time"] = med["critic"] / med["lstm"]
        out["chunk1_over_default_advantages_time"] = med["critic_chunk1"] / med["critic"]
        out["critic_over_lstm_update_time"] = statistics.median(secs["critic"]) / statistics.median(secs["lstm"])
    if not a.no_profile:
        import shutil
        import tempfile
        if a.profile_dir is None:
            a.profile_dir = tempfile.mkdtemp(prefix="bench_ppo_lstm_trace_")
        os.makedirs(a.profile_dir, exist_ok=True)
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.profile_dir, "--",
               sys.executable, os.path.abspath(__file__), "--profile-child", "--envs", str(a.envs), "--rows", str(a.rows), "--epochs", str(a.epochs),
               "--minibatch-rows", str(a.minibatch_rows), "--precision", a.precision] + (["--critic"] if a.critic else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("rocprofv3 failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        kt = kernel_times(a.profile_dir)
        out["kernel_trace"] = {k: {"calls": c, "mean_us_per_launch": ns / 1e3} for k, (c, ns) in kt.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
