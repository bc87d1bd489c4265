#!/usr/bin/env python3
"""What a PPO update costs on the RL workload (bench.py --workload rl: 2v2 Oval, every agent LowMode RL, one 312 -> 256 x 3 actor per team,
DecisionPeriod 2, rewards on): one rollout of R rows is collected (timed), then for team 0's trainer (critic 312 -> 256 x 3):
hk_ppo_advantages, one-epoch hk_ppo_update calls at minibatch 512 (ML-Agents' batch_size) and at a GPU-sized minibatch, and
hk_ppo_normalizer_update (normalizer_ms; the state is put back after every call, which republishes the attached statistics bit for bit, so
the other timings run on what they always ran on), and the self-play facilities on the same rollout: hk_rollout_episode_stats of team 0
(episode_stats_ms), hk_policy_pool_save of team 0's actor into a pool slot and hk_policy_pool_load of that slot into team 1's actor, which has
no trainer (pool_save_ms, pool_load_ms; the load runs last, after every other timing); every timing ends in a device synchronise, medians of --repeats.  One JSON line per --precision; with several, the precisions alternate round by round
(after a switch: advantages and one untimed update at the large minibatch, which allocate the workspace of that precision).
--max-grad-norm C / --target-kl T (hk.h "LONG RUNS"): every plain update window is followed, in the same round, by a window of the same update
with the clip-aware step (C = inf measures only) and / or with the per-epoch KL read (a T above any KL stops nothing): clip_* and kl_* per
minibatch size, each with its ratio to the same process's plain update.
FLOP count per trained row (stated, not measured): forward + backward of actor and critic = 3 x forward, forward = 2 x (weights of the trunks
and heads) per row: 3 x 2 x (312 x 256 + 2 x 256 x 256 + 4 x 256 + 312 x 256 + 2 x 256 x 256 + 256) = 6 x 423 168 = 2.54 MFLOP per row at this shape."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = {"f32": 157.3, "bf16": 16 * 157.3}          # MI355X MFMA peaks (TFLOP/s): f32 in / f32 acc, and bf16 at 16 x that rate
PEAK_HBM_TB = 8.0                                     # MI355X HBM3E peak (TB/s)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=64, help="R: rows (decisions) per rollout")
    ap.add_argument("--big", type=int, default=32768, help="the GPU-sized minibatch")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", nargs="+", choices=("f32", "bf16"), default=["f32"], help="hk_ppo_set_precision; several: alternated")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="also time the update with this global-norm bound (inf: measure only)")
    ap.add_argument("--target-kl", type=float, default=None, help="also time the update with this KL stop (above any KL: nothing stops)")
    a = ap.parse_args()
    import numpy as np
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    E, A, P, R = a.envs, 4, 2, a.rows
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
    tr = env.ppo_trainer(0, seed=1)
    n = R * E * 2

    H, K0 = 256, in_dim
    w = K0 * H + 2 * H * H + 4 * H + K0 * H + 2 * H * H + H
    flop_row = 3 * 2 * w
    sizes = (a.big, 512)
    extras = {k: v for k, v in (("clip", {"max_grad_norm": a.max_grad_norm}), ("kl", {"target_kl": a.target_kl})) if list(v.values())[0] is not None}
    runs = {p: {"adv": [], "norm": [], **{mb: [] for mb in sizes}, **{(k, mb): [] for k in extras for mb in sizes}} for p in a.precision}
    reports = {}
    # what hk_ppo_normalizer_update reads, once each: the trainer's slots of OBS [R][E][S][D] and FIRST [R][E][S], RING0 [E][S][stack - 1][D]
    D, S, stack = env.obs_dim, 2, 4
    norm_bytes = 4 * (R * E * S * D + R * E * S + E * S * (stack - 1) * D)
    tr.normalizer_init(1)
    norm_state = tr.normalizer_state()
    tr.normalizer_update()                               # (allocates the partials; first launches)
    tr.normalizer_load(*norm_state)

    def timed(f):
        env.synchronize()
        t = time.perf_counter()
        f()
        env.synchronize()
        return (time.perf_counter() - t) * 1e3

    # what hk_rollout_episode_stats reads, once each: REWARD, GROUP_REWARD, TERM_REWARD, TERM_GROUP_REWARD of the policy's slots [R][E][S], DONE [R][E]
    stats_bytes = 4 * (4 * R * E * S + R * E)
    pool = env.snapshot_pool(0, 2)
    pool_bytes = 4 * pool.count
    env.episode_stats(0)                                 # (allocates; first launches)
    pool.save(0)
    sp_runs = {"stats": [], "save": []}
    for _ in range(a.repeats):
        sp_runs["stats"].append(timed(lambda: env.episode_stats(0)))
        sp_runs["save"].append(timed(lambda: pool.save(0)))
    for _ in range(a.repeats):
        for prec in a.precision:
            tr.set_precision(prec)
            tr.advantages()                              # (allocates; first launches)
            tr.update(1, a.big, 1e-5, 0.2, 5e-3)
            runs[prec]["adv"].append(timed(tr.advantages))
            for mb in sizes:
                runs[prec][mb].append(timed(lambda: tr.update(1, mb, 1e-5, 0.2, 5e-3)))
                for k, opt in extras.items():
                    runs[prec][(k, mb)].append(timed(lambda: tr.update(1, mb, 1e-5, 0.2, 5e-3, **opt)))
                    reports[(prec, k, mb)] = tr.last_report
            runs[prec]["norm"].append(timed(tr.normalizer_update))
            tr.normalizer_load(*norm_state)
    sp_runs["load"] = [timed(lambda: pool.load(0, 1)) for _ in range(a.repeats + 1)][1:]       # (the first call is the warm-up)
    env.close()
    selfplay = {"episode_stats_ms": statistics.median(sp_runs["stats"]), "episode_stats_runs": sp_runs["stats"], "episode_stats_bytes": stats_bytes,
                "episode_stats_hbm_fraction": stats_bytes / (statistics.median(sp_runs["stats"]) * 1e-3) / (PEAK_HBM_TB * 1e12),
                "pool_save_ms": statistics.median(sp_runs["save"]), "pool_save_runs": sp_runs["save"],
                "pool_load_ms": statistics.median(sp_runs["load"]), "pool_load_runs": sp_runs["load"], "pool_slot_bytes": pool_bytes}
    for prec in a.precision:
        res = {}
        for mb in sorted(sizes):
            ms = statistics.median(runs[prec][mb])
            rows = (n // min(mb, n)) * min(mb, n)
            tf = rows * flop_row / (ms * 1e-3) / 1e12
            res[str(mb)] = {"update_ms_per_epoch": ms, "runs": runs[prec][mb], "rows_per_s": rows / (ms * 1e-3), "tflops": tf,
                            "peak_fraction": tf / PEAK_TF[prec], "update_over_collection": ms / collect_ms}
            for k in extras:
                xs = runs[prec][(k, mb)]
                res[str(mb)].update({k + "_update_ms_per_epoch": statistics.median(xs), k + "_runs": xs, k + "_over_plain": statistics.median(xs) / ms,
                                     k + "_report": reports[(prec, k, mb)]})
        print(json.dumps({"metric": "PPO update on the RL workload (one actor + critic, one epoch)", "precision": prec,
                          "advantages_ms": statistics.median(runs[prec]["adv"]), "advantages_runs": runs[prec]["adv"], "collect_ms": collect_ms,
                          "normalizer_ms": statistics.median(runs[prec]["norm"]), "normalizer_runs": runs[prec]["norm"], "normalizer_bytes": norm_bytes,
                          "normalizer_hbm_fraction": norm_bytes / (statistics.median(runs[prec]["norm"]) * 1e-3) / (PEAK_HBM_TB * 1e12),
                          **selfplay, "minibatch": res, "config": {"envs": E, "agents": A, "rows": R, "n_rows": n, "flop_per_row": flop_row,
                                                       "peak_tflops": PEAK_TF[prec], "max_grad_norm": None if a.max_grad_norm is None else str(a.max_grad_norm), "target_kl": a.target_kl}}))


if __name__ == "__main__":
    main()
