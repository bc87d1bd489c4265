#!/usr/bin/env python3
"""The trained actors the reference's experiment scenes run (BehaviorParameters.m_Model of the agents in
tests/golden/reference_experiments.json), as plain float32 arrays: tests/golden/reference_actors.npz.

Build container only: reads the .onnx DATA files under /root/reference/Assets/Karting/Prefabs/AI with the in-repo protobuf
reader (hierarchicalkarting_amd/onnx_read.py).  The fixture holds numbers only (weights, biases, the observation normaliser,
log sigma) under "<model file name>/<array>", so that the closed-loop races of tests/test_reference_logs.py run on any box.
The one 312 -> 256 x 3 team actor tests/test_policy_oracle.py exports goes the same way into tests/golden/reference_actor_312.npz.

  --e2e   the actors of the EndToEndKartAgent set-ups (tests/golden/reference_e2e_experiments.json) that reference_actors.npz lacks,
          E2E and hierarchical alike, into tests/golden/reference_e2e_actors_<k>.npz; the other two files are left as they are.
          The arrays are spread over shards of at most SHARD_BYTES each, so that no file of the repository is large: an array larger
          than that is stored as row blocks "<name>@<i>" (tests/e2e_setups.py joins them again)"""
import argparse, glob, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hierarchicalkarting_amd.policy import Policy          # noqa: E402

MODELS = "/root/reference/Assets/Karting/Prefabs/AI"
TEAM_312 = "HierarchicalAgent-Team-allscaledown14.onnx"
SHARD_BYTES = 320 * 1024


def write_shards(arrays, stem):
    """arrays -> <stem>_0.npz, <stem>_1.npz ... of at most SHARD_BYTES of array data each; -> the paths"""
    pieces = []
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        if a.nbytes <= SHARD_BYTES:
            pieces.append((k, a))
            continue
        rows = max(1, SHARD_BYTES // (a.nbytes // a.shape[0]))
        pieces += [("%s@%d" % (k, i), a[r:r + rows]) for i, r in enumerate(range(0, a.shape[0], rows))]
    shards, cur, size = [], {}, 0
    for k, a in pieces:
        if cur and size + a.nbytes > SHARD_BYTES:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    shards.append(cur)
    for old in glob.glob(stem + "_*.npz"):
        os.remove(old)
    paths = []
    for i, sh in enumerate(shards):
        paths.append("%s_%d.npz" % (stem, i))
        np.savez_compressed(paths[-1], **sh)
    return paths


def main_e2e():
    have = {k.split("/")[0] for k in np.load(os.path.join(ROOT, "tests", "golden", "reference_actors.npz")).files}
    wanted = set()
    for e in json.load(open(os.path.join(ROOT, "tests", "golden", "reference_e2e_experiments.json"))):
        for a in e["agents"]:
            m = (a.get("behavior") or {}).get("model")
            if m and (a.get("script") == "EndToEndKartAgent.cs" or a.get("LowMode") == 0) and m not in have:
                wanted.add(m)
    out = {}
    for m in sorted(wanted):
        p = Policy.from_onnx(os.path.join(MODELS, m))
        out.update(p.arrays(m + "/"))
        print("%-50s in %d hidden %d layers %d branches %d" % (m, p.in_dim, p.hidden, len(p.W), p.n_branch))
    for dst in write_shards(out, os.path.join(ROOT, "tests", "golden", "reference_e2e_actors")):
        print("wrote", dst, os.path.getsize(dst), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e2e", action="store_true")
    if ap.parse_args().e2e:
        return main_e2e()
    exps = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_experiments.json")))
    wanted = set()
    for e in exps:
        if not str(e.get("ExperimentName", "")).endswith(("2", "3")) or "E2E" in str(e.get("ExperimentName")):
            continue
        for a in e["agents"]:
            m = (a.get("behavior") or {}).get("model")
            if m and a.get("LowMode") == 0:
                wanted.add(m)
    out = {}
    for m in sorted(wanted):
        p = Policy.from_onnx(os.path.join(MODELS, m))
        out.update(p.arrays(m + "/"))
        print("%-50s in %d hidden %d layers %d branches %d" % (m, p.in_dim, p.hidden, len(p.W), p.n_branch))
    dst = os.path.join(ROOT, "tests", "golden", "reference_actors.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    dst = os.path.join(ROOT, "tests", "golden", "reference_actor_312.npz")
    np.savez_compressed(dst, **Policy.from_onnx(os.path.join(MODELS, TEAM_312)).arrays(TEAM_312 + "/"))
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
