"""The one rule of the GPU tests, written once: libhk is bit-identical to the CPU oracle.

Imported like oracle_lib (not a conftest, no fixtures, not collected).
  assert_bits_equal   arrays, structured or plain, nested dtypes too, every float compared as the unsigned integer of its width
  assert_same_state   agent_state() and every env_state() field but `reserved`; on request observations, episode results, planner state
  twin / step_both    a reset (RacingEnv, OracleEnv) pair, and both stepped through the same call sizes with a look every few calls
  run_child           a module-level function of a test module in a fresh interpreter: the HK_* switches are read once per process
                      (hk_create), so every setting of them gets a child of its own"""
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
from hierarchicalkarting_amd import _lib as HL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
ENV_FIELDS = tuple(n for n in np.dtype(HL.EnvState).names if n != "reserved")   # `reserved`: library-internal progress words of hk_step


def _bits(x):
    return np.ascontiguousarray(x).view("u%d" % x.dtype.itemsize) if x.dtype.kind == "f" else x


def assert_bits_equal(a, b, tag, exclude=None, path=""):
    """a and b bit for bit, field by field.  exclude: {dotted field path: boolean mask over the leading axes of the elements to skip};
    path: the name of a, which the field paths (of exclude and of the message) start with"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (tag, path, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.names:
        for n in a.dtype.names:
            p = path + "." + n if path else n
            x, y = a[n], b[n]
            if exclude and p in exclude:
                x, y = x[~exclude[p]], y[~exclude[p]]
            assert_bits_equal(x, y, tag, exclude, p)
        return
    bad = np.argwhere(_bits(a) != _bits(b))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError("%r %s: %d mismatch(es) at %s ...; first %r vs %r"
                             % (tag, path or "array", len(bad), bad[:4].tolist(), a[i], b[i]))


def assert_same_state(g, o, tag, *, obs=False, results=False, mcts=False, env_fields=None, exclude=None):
    """exclude: as assert_bits_equal's, the paths starting with the getter ("agent_state.cum_reward")"""
    assert_bits_equal(g.agent_state(), o.agent_state(), tag, exclude, "agent_state")
    ge, oe = g.env_state(), o.env_state()
    for n in env_fields or ENV_FIELDS:
        assert_bits_equal(ge[n], oe[n], tag, path="env_state." + n)
    for getter, asked in (("observations", obs), ("episode_results", results), ("mcts_state", mcts)):
        if asked:
            assert_bits_equal(getattr(g, getter)(), getattr(o, getter)(), tag, exclude, getter)


def twin(cfg, attach=None):
    """-> (RacingEnv, OracleEnv) on the same config, the actor attach = (policy, slots, decision period) attached to both before the
    reset; attach may be a function of the observation size that returns that triple"""
    import hierarchicalkarting_amd as hk
    import oracle_lib as O
    g, o = hk.RacingEnv(cfg), O.OracleEnv(cfg)
    if callable(attach):
        attach = attach(g.obs_dim)
    for e in (g, o):
        if attach:
            e.attach_policy(*attach)
        e.reset()
    return g, o


def step_both(g, o, calls, look_every=1, check=assert_same_state):
    """step both through the call sizes; check(g, o, ticks) after every look_every-th call and, after synchronize, at the end.  -> ticks"""
    t = 0
    for k, n in enumerate(calls, 1):
        g.step(n); o.step(n); t += n
        if k % look_every == 0:
            check(g, o, t)
    g.synchronize()
    check(g, o, t)
    return t


# ---------------------------------------------------------------- child processes
KEEP = object()             # run_child(lib=KEEP): HK_LIB_PATH as the parent has it
DONE = "parity.run_child: returned"
_PROLOGUE = """\
import importlib, json, sys
root, tests, module, name, args, done = sys.argv[1:]
sys.path[:0] = [root, tests]
getattr(importlib.import_module(module), name)(*json.loads(args))
print(done, flush=True)
"""
Child = namedtuple("Child", "ok returncode output")


def run_child(fn, *args, switches=None, lib=KEEP, timeout):
    """fn(*args) in a fresh interpreter, waited for.  Environment: the parent's without any HK_* but HK_LIB_PATH, then `switches`;
    lib: a path for HK_LIB_PATH, None to remove it.  ok: exit status 0 and the runner's completion line (a child that exits early fails)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HK_") or k == "HK_LIB_PATH"}
    if lib is None:
        env.pop("HK_LIB_PATH", None)
    elif lib is not KEEP:
        env["HK_LIB_PATH"] = lib
    env.update(switches or {})
    r = subprocess.run([sys.executable, "-c", _PROLOGUE, ROOT, TESTS, fn.__module__, fn.__name__, json.dumps(args), DONE],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    ok = r.returncode == 0 and DONE in r.stdout.splitlines()
    return Child(ok, r.returncode, "%s(%s) exit %d\n--- stdout ---\n%s\n--- stderr ---\n%s"
                 % (fn.__name__, ", ".join(map(repr, args)), r.returncode, r.stdout[-2000:], r.stderr[-4000:]))


def assert_child(fn, *args, **kw):
    r = run_child(fn, *args, **kw)
    assert r.ok, r.output
    return r
