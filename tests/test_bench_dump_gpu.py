"""bench.py --dump-outputs: after the timed steps the driver writes what the timed path computed in its last step as DIR/<name>.npy
(float32 / float64, <= 64 MB); the inputs are seeded, so two runs with the same arguments write the same arrays.  --steps sets the
number of timed ticks and the line carries ms_per_step."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "7", "--warmup", "3", "--envs-per-gpu", "384", "--no-secondary", "--no-cpu-baseline"]


def _bench(out_dir, args=ARGS):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_repeat_bit_for_bit(tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for out in (a, b):
        assert out["steps"] == 7 and out["config"]["timed_tick_range"] == [512 + 3, 512 + 3 + 7]
        assert out["ms_per_step"] > 0            # (that exactly 7 ticks were timed: the oracle comparison at tick 512 + 3 + 7 below)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == a["dump_outputs"]["files"]
    assert {"agent_px.npy", "agent_pz.npy", "agent_section_index.npy", "observations.npy", "action_steer.npy", "result_time_steps.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), n
        assert x.shape[:1] == (384,) and np.array_equal(x, y, equal_nan=True), n
        total += x.nbytes
    assert total == a["dump_outputs"]["bytes"] <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "sample_env_ids.npy"), np.arange(384))
    # the state after the timed ticks: the CPU oracle, run to the same tick on the same seeded inputs, agrees bit for bit
    import oracle_lib as O
    import hierarchicalkarting_amd as hk
    o = O.OracleEnv(hk.make_config(384, 4, jitter_seed=0x5EED0000))
    o.reset()
    o.step(512 + 3 + 7)
    st = o.agent_state()
    for f in ("px", "pz", "yaw", "vx", "vz", "wy", "section_index", "lane", "flags"):
        assert np.array_equal(np.load(tmp_path / "a" / ("agent_%s.npy" % f)), st[f].astype(np.float64 if st[f].dtype.kind in "iu" else st[f].dtype)), f
    assert np.array_equal(np.load(tmp_path / "a" / "observations.npy"), o.observations())


@pytest.mark.gpu
def test_lqbatch_steps_and_dump(tmp_path):
    """--workload lqbatch: exactly --steps timed calls per player count (the library's own launch count), and the controls of the last one,
    the same from run to run; the 256 distinct games are tiled over the batch, so every tile holds the same controls"""
    args = ["--gpus", "1", "--workload", "lqbatch", "--lq-batch", "1024", "--steps", "5", "--warmup", "2"]
    a, b = _bench(tmp_path / "a", args), _bench(tmp_path / "b", args)
    for out in (a, b):
        assert out["steps"] == 5 and out["ms_per_step"] > 0
        assert [out["per_N"][k]["kernel_launches"] for k in ("N2", "N4")] == [5, 5]
    assert sorted(os.listdir(tmp_path / "a")) == ["u_N2.npy", "u_N4.npy"]
    for n in ("u_N2.npy", "u_N4.npy"):
        u, v = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert u.dtype == np.float64 and u.shape == (1024, 2) and np.isfinite(u).all() and np.array_equal(u, v)
        assert np.array_equal(u.reshape(4, 256, 2), np.broadcast_to(u[:256], (4, 256, 2))) and np.abs(u).max() > 0
