#!/usr/bin/env python3
"""Closed-loop pin against the ONLY outcome data the reference holds: ExperimentLogs/<ExperimentName>.txt.

For every experiment set-up of the reference's Compete scenes whose agents are all HierarchicalKartAgents
(tests/golden/reference_experiments.json, 22 set-ups: {Fixed-RL, MCTS-RL, MCTS-LQR} x {Fixed-LQR, MCTS-LQR, Fixed-RL} on Oval,
OvalDuos, Complex, ComplexDuos) this runs the CPU oracle on the same set-up — same Agents[] order, wiring, gameParams, rules,
orderings e % A!, and for LowMode == RL agents the reference's own trained actors (tests/golden/reference_actors.npz) —
writes the races in the reference's log grammar, reads both logs back with the same in-repo reader
(hierarchicalkarting_amd/telemetry.py) and prints the statistics side by side.  No reference code is executed; the logs,
scenes and .onnx files are read as data (build container only — /root/reference does not exist on the GPU box).

  --update     store the reference-side statistics in tests/golden/reference_log_stats.json and the oracle-side results
               (statistics + a hash of every race's hk_episode_result) in tests/golden/experiment_oracle.json; the GPU
               parity test compares libhk's races with those hashes, the CPU test re-derives them for a subset
  --markdown   print the residual table of DESIGN.md
  --only a,b   substrings of experiment names

  --e2e        the 16 EndToEndKartAgent set-ups of the *All scenes instead (tests/golden/reference_e2e_experiments.json, tests/e2e_setups.py),
               raced through libhk on the GPU (the oracle has no E2E agent).  Set-ups without a log of their own name are raced and
               hashed but have no reference column.  With --update: tests/golden/e2e_experiment_gpu.json (statistics + hash of every race)
               and, where the reference's logs are at hand, tests/golden/reference_e2e_log_stats.json
  --logs-only  with --e2e --update: write the log statistics only (no GPU)"""
import argparse, hashlib, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalkarting_amd import telemetry as T          # noqa: E402
import experiments as X                                     # noqa: E402
import e2e_setups as E2E                                    # noqa: E402

REF_LOGS = "/root/reference/ExperimentLogs"
STATS = ("races", "wins", "dnfs", "mean_total_time", "median_best_lap", "collisions_per_race", "illegal_lane_changes_per_race",
         "mean_lane_difference", "mean_vel_difference")


def setup_names():
    """the set-ups that have a log of the same name in the reference (the latest generation: suffix 2 / 3)"""
    return [n for n in sorted(X.experiments()) if n.endswith(("2", "3"))]


def results_hash(res):
    h = hashlib.sha256()
    for name in res.dtype.names:
        h.update(res[name].tobytes())
    return h.hexdigest()


def run_ours(name, env_cls, mcts_iterations=128):
    s = X.Setup(name, mcts_iterations=mcts_iterations)
    res = s.run(env_cls)
    with tempfile.TemporaryDirectory() as d:
        stats = s.stats(res, os.path.join(d, "ours.txt"))
    return res, stats


def run_e2e(name, mcts_iterations=128):
    import hierarchicalkarting_amd as hk
    s = E2E.Setup(name, mcts_iterations=mcts_iterations)
    res = s.run(hk.RacingEnv)
    with tempfile.TemporaryDirectory() as d:
        stats = s.stats(res, os.path.join(d, "ours.txt"))
    return res, stats


def log_record(path):
    """the statistics of one reference log, and its experiment 0 as parsed (for checks against numbers read off the file by hand)"""
    recs = T.read_experiment_log(path)
    first = recs[0]
    return {"log": "ExperimentLogs/" + os.path.basename(path), "stats": T.summarize_log(recs),
            "experiment_0": {n: {k: a[k] for k in ("Total Time", "Best Lap") if k in a} for n, a in first["agents"].items()}}


def main_e2e(a):
    gref = os.path.join(ROOT, "tests", "golden", "reference_e2e_log_stats.json")
    ggpu = os.path.join(ROOT, "tests", "golden", "e2e_experiment_gpu.json")
    ref_all = json.load(open(gref)) if os.path.exists(gref) else {}
    gpu_all = json.load(open(ggpu)) if os.path.exists(ggpu) else {}
    names = [n for n in sorted(E2E.experiments()) if not a.only or any(o in n for o in a.only.split(","))]
    if os.path.isdir(REF_LOGS):
        for name in names:
            path = os.path.join(REF_LOGS, name + ".txt")
            if os.path.exists(path):
                ref_all[name] = log_record(path)
    if a.logs_only:
        for name in names:
            print("%-32s %s" % (name, ref_all[name]["log"] if name in ref_all else "no log of this name"))
        if a.update:
            json.dump(ref_all, open(gref, "w"), indent=1, sort_keys=True)
            print("wrote", gref)
        return
    rows = []
    for name in names:
        t0 = time.time()
        res, ours = run_e2e(name, a.mcts_iterations)
        gpu_all[name] = {"mcts_iterations": a.mcts_iterations, "results_sha256": results_hash(res), "stats": ours}
        ref = ref_all.get(name, {}).get("stats", {})
        print("== %s  (reference: %s; libhk %.1f s)" % (name, ref_all[name]["log"] if name in ref_all else "no log of this name", time.time() - t0))
        print("  %-10s %-32s %12s %12s" % ("", "", "reference", "libhk"))
        for typ in ours:
            r = ref.get(typ, {})
            for k in STATS:
                rv, ov = r.get(k), ours[typ][k]
                ratio = "" if not isinstance(rv, (int, float)) or not isinstance(ov, (int, float)) or not rv else "  x%.3f" % (ov / rv)
                print("  %-10s %-32s %12s %12s%s" % (typ if k == STATS[0] else "", k, fmt(rv), fmt(ov), ratio))
            rows.append((name, typ, r, ours[typ]))
        sys.stdout.flush()
    if a.markdown:
        print("| experiment | agent | wins | DNFs | mean total time [s] | median best lap [s] | lane difference [m] |")
        print("|---|---|---|---|---|---|---|")
        for name, typ, r, o in rows:
            c = lambda k: "%s / %s" % (fmt(r.get(k)), fmt(o.get(k)))
            x = lambda k: "" if not r.get(k) else " (x%.3f)" % (o[k] / r[k])
            print("| %s | %s | %s | %s | %s%s | %s%s | %s |" % (name, typ, c("wins"), c("dnfs"), c("mean_total_time"), x("mean_total_time"),
                                                              c("median_best_lap"), x("median_best_lap"), c("mean_lane_difference")))
    if a.update:
        json.dump(gpu_all, open(ggpu, "w"), indent=1, sort_keys=True)
        print("wrote", ggpu)


def fmt(v):
    return "-" if v is None else ("%d" % v if isinstance(v, int) else "%.3f" % v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--mcts-iterations", type=int, default=128)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--logs-only", action="store_true")
    a = ap.parse_args()
    if a.e2e:
        return main_e2e(a)
    import oracle_lib as O
    gref = os.path.join(ROOT, "tests", "golden", "reference_log_stats.json")
    gora = os.path.join(ROOT, "tests", "golden", "experiment_oracle.json")
    ref_all = json.load(open(gref)) if os.path.exists(gref) else {}
    ora_all = json.load(open(gora)) if os.path.exists(gora) else {}
    rows = []
    for name in setup_names():
        if a.only and not any(o in name for o in a.only.split(",")):
            continue
        path = os.path.join(REF_LOGS, name + ".txt")
        if os.path.exists(path):
            ref_all[name] = {"log": "ExperimentLogs/%s.txt" % name, "stats": T.summarize_log(T.read_experiment_log(path))}
        if name not in ref_all:
            continue
        t0 = time.time()
        res, ours = run_ours(name, O.OracleEnv, a.mcts_iterations)
        ora_all[name] = {"mcts_iterations": a.mcts_iterations, "results_sha256": results_hash(res), "stats": ours}
        ref = ref_all[name]["stats"]
        print("== %s  (reference: %s; oracle %.1f s)" % (name, ref_all[name]["log"], time.time() - t0))
        for typ in ours:
            r = ref.get(typ, {})
            print("  %-10s %-32s %12s %12s" % (typ, "", "reference", "oracle"))
            for k in STATS:
                rv, ov = r.get(k), ours[typ][k]
                ratio = "" if not isinstance(rv, (int, float)) or not isinstance(ov, (int, float)) or not rv else "  x%.3f" % (ov / rv)
                print("  %-10s %-32s %12s %12s%s" % ("", k, fmt(rv), fmt(ov), ratio))
            rows.append((name, typ, r, ours[typ]))
        sys.stdout.flush()
    if a.markdown:
        print("| experiment | agent | wins | DNFs | mean total time [s] | median best lap [s] | collisions / race | illegal lane changes / race | lane difference [m] |")
        print("|---|---|---|---|---|---|---|---|---|")
        for name, typ, r, o in rows:
            c = lambda k: "%s / %s" % (fmt(r.get(k)), fmt(o.get(k)))
            print("| %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (name, typ, c("wins"), c("dnfs"), c("mean_total_time"), c("median_best_lap"),
                                                                   c("collisions_per_race"), c("illegal_lane_changes_per_race"), c("mean_lane_difference")))
    if a.update:
        json.dump(ref_all, open(gref, "w"), indent=1, sort_keys=True)
        json.dump(ora_all, open(gora, "w"), indent=1, sort_keys=True)
        print("wrote", gref, "and", gora)


if __name__ == "__main__":
    main()
