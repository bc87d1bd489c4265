#!/usr/bin/env python3
"""The launch schedule hk_step chooses, pinned: tests/golden/schedule_trace.json.gz.

Every handle below runs one fixed pattern of calls (forty one-tick calls, then calls of 2, 3, 20, 63, 64, 65, 130 and 520 ticks, a getter, a full
and a partial reset).  After every call the script records what hk_schedule_info() says the call ran (not the games meter: its copy is
asynchronous), and at the checkpoints the launches per profiled stage since the last one (hk_prof_read).  The meter could steer the launches of
the default schedule, so every mode fixes HK_INWAVE.

  python tests/golden/make_schedule_trace.py <mode>      print the trace of one mode (a child process per mode: the switches are read in hk_create)
  python tests/golden/make_schedule_trace.py --write     run every mode and rewrite the golden (on the GPU)"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "schedule_trace.json.gz")

MODES = {
    "inwave": {"HK_INWAVE": "1"},
    "queues": {"HK_INWAVE": "0"},
    "one_stream": {"HK_INWAVE": "1", "HK_SPLIT": "0"},
    "fused": {"HK_INWAVE": "1", "HK_FISSION": "0"},
    "fixed_rounds": {"HK_INWAVE": "1", "HK_FIXED_ROUNDS": "1"},
    "no_optimistic": {"HK_INWAVE": "1", "HK_NO_OPTIMISTIC": "1"},
    "optimistic_skew": {"HK_INWAVE": "1", "HK_OPTIMISTIC_SKEW": "1"},
    "mcts_no_pause": {"HK_INWAVE": "1", "HK_MCTS_NO_PAUSE": "1"},
    "mcts_no_overlap": {"HK_INWAVE": "1", "HK_MCTS_NO_OVERLAP": "1"},
}
HANDLES = ("plain_split", "plain", "two_agents", "eight_agents", "planner", "planner_actor_lq", "actor_lq", "training")
FIELDS = ("call_ticks", "rounds", "rounds_issued", "kernel", "streams", "ticks_per_launch", "optimistic_plan", "armed_in_first_launch", "planner",
          "actors", "multi_player_games")
CALLS = [1] * 40 + [2, 3, 20, "prof", 63, 64, 65, "get", 130, "reset_part", 520, "prof", "reset", 1, 2, 20, 64, "prof"]


def make_env(kind):
    import hierarchicalkarting_amd as hk
    from hierarchicalkarting_amd import _lib
    from hierarchicalkarting_amd.policy import Policy
    MC, FX, LQ, RL = _lib.HK_HIGH_MCTS, _lib.HK_HIGH_FIXED, _lib.HK_LOW_LQR, _lib.HK_LOW_RL
    kw = dict(jitter_seed=0x5EED0000, laps=1, max_episode_steps=260)
    planner = dict(high_mode=[MC, MC, FX, FX], tree_search_depth=[8, 8, 5, 5], mcts_iterations=12)
    cfg = {"plain_split": lambda: hk.make_config(8192 + 96, 4, **kw),
           "plain": lambda: hk.make_config(160, 4, **kw),
           "two_agents": lambda: hk.make_config(160, 2, **kw),
           "eight_agents": lambda: hk.make_config(40, 8, **kw),
           "planner": lambda: hk.make_config(160, 4, **planner, **kw),
           "planner_actor_lq": lambda: hk.make_config(160, 4, low_mode=[RL, RL, LQ, LQ], **planner, **kw),
           "actor_lq": lambda: hk.make_config(160, 4, low_mode=[RL, RL, LQ, LQ], **kw),
           "training": lambda: hk.make_config(160, 4, env_mode=_lib.HK_MODE_TRAINING, training_agents=[1, 1, 0, 0], rewards=1, jitter_seed=0, laps=1,
                                              max_episode_steps=260)}[kind]()
    g = hk.RacingEnv(cfg)
    if "actor" in kind:
        g.attach_policy(Policy.random(g.obs_dim * 4, 64, 2, seed=78), [0, 1], 2)
    return g


def trace(kind):
    import numpy as np
    g = make_env(kind)
    g.prof_enable(True)
    g.reset()
    g.prof_reset()
    out = []
    for c in CALLS:
        if c == "prof":
            out.append({"launches": {name: int(n) for name, (_, n) in g.prof_read().items()}})
            g.prof_reset()
        elif c == "get":
            g.agent_state()
            out.append("get")
        elif c == "reset":
            g.reset()
            out.append("reset")
        elif c == "reset_part":
            g.reset(np.arange(0, g.E, 3))
            out.append("reset_part")
        else:
            g.step(c)
            s = g.schedule_info()
            out.append({k: s[k] for k in FIELDS})
    g.synchronize()
    g.close()
    return out


def run_mode(mode, timeout=600):
    """the trace of one mode, from a child process with only that mode's switches set"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HK_") or k == "HK_LIB_PATH"}
    env.update(MODES[mode])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("schedule trace, mode %s: exit %d\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def main():
    if sys.argv[1:] == ["--write"]:
        golden = {m: run_mode(m) for m in MODES}
        with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
            f.write(json.dumps(golden, indent=0, sort_keys=True).encode() + b"\n")
        return
    sys.path.insert(0, ROOT)
    print(json.dumps({k: trace(k) for k in HANDLES}, sort_keys=True))


if __name__ == "__main__":
    main()
