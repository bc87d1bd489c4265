"""tests/parity.py, the compare and the child runner every GPU parity test is built on, on the CPU oracle and tiny child functions."""
import json
import os
import sys
import numpy as np
import pytest
import oracle_lib as O
from hierarchicalkarting_amd.config import make_config
from parity import assert_bits_equal, assert_same_state, run_child

NESTED = np.dtype([("a", np.float32), ("inner", [("x", np.float64, (3,)), ("n", np.int32)])])


def _nested():
    r = np.zeros((4, 2), NESTED)
    r["a"] = np.arange(8, dtype=np.float32).reshape(4, 2)
    r["inner"]["x"] = np.linspace(0.5, 2.0, 24).reshape(4, 2, 3)
    r["inner"]["n"] = 7
    return r


def test_signed_zero_differs():
    with pytest.raises(AssertionError, match="array: 1 mismatch"):
        assert_bits_equal(np.array([0.0, 1.0], np.float32), np.array([-0.0, 1.0], np.float32), "zero")


def test_one_ulp_in_a_nested_field_is_found_and_named():
    a, b = _nested(), _nested()
    assert_bits_equal(a, b, "same")
    b["inner"]["x"][2, 1, 0] = np.nextafter(b["inner"]["x"][2, 1, 0], np.inf)
    with pytest.raises(AssertionError, match=r"'ulp' inner\.x: 1 mismatch\(es\) at \[\[2, 1, 0\]\]"):
        assert_bits_equal(a, b, "ulp")


def test_nan_payload_differs():
    a = np.array([np.nan], np.float32)
    b = a.view(np.uint32).copy()
    b[0] ^= 1
    assert np.isnan(b.view(np.float32)).all()
    assert_bits_equal(a, a.copy(), "nan")
    with pytest.raises(AssertionError):
        assert_bits_equal(a, b.view(np.float32), "nan")


def test_masked_elements_are_skipped():
    a, b = _nested(), _nested()
    b["inner"]["x"][1, 0] = -1.0
    b["a"][3, 1] = -0.0
    mask = np.zeros((4, 2), bool)
    mask[1, 0] = True
    with pytest.raises(AssertionError, match="'m' a"):
        assert_bits_equal(a, b, "m", exclude={"inner.x": mask})
    mask[3, 1] = True
    assert_bits_equal(a, b, "m", exclude={"inner.x": mask, "a": mask})


def _oracle_twins():
    b = make_config(3, 4, jitter_seed=5)
    x, y = O.OracleEnv(b), O.OracleEnv(b)
    for e in (x, y):
        e.reset()
        e.step(90)
    return x, y


def test_same_state_of_oracle_twins():
    x, y = _oracle_twins()
    assert_same_state(x, y, 90, obs=True, results=True, mcts=True)
    es = y.env_state()
    es["reserved"][:, 0] = 5                      # hk_step's progress words: library-internal, never compared
    y.set_env_state(es)
    assert (y.env_state()["reserved"] != x.env_state()["reserved"]).any()
    assert_same_state(x, y, 90)
    st = y.agent_state()
    st["vx"][1, 2] = np.nextafter(st["vx"][1, 2], np.float32(np.inf))
    y.set_agent_state(st)
    with pytest.raises(AssertionError, match=r"agent_state\.vx: 1 mismatch\(es\) at \[\[1, 2\]\]"):
        assert_same_state(x, y, 90)


# ---------------------------------------------------------------- run_child on functions that need no GPU
def _child_report_env():
    print(json.dumps({k: v for k, v in os.environ.items() if k.startswith("HK_")}))


def _child_fails(n):
    assert n == 3, "the child's own assertion, n=%d" % n


def _child_exits_early():
    sys.exit(0)


def _env_of(r):
    assert r.ok, r.output
    return json.loads(r.output.split("--- stdout ---\n")[1].splitlines()[0])


def test_child_environment(monkeypatch):
    monkeypatch.setenv("HK_SPLIT", "1")
    monkeypatch.setenv("HK_LIB_PATH", "/parent/libhk.so")
    assert _env_of(run_child(_child_report_env, timeout=120)) == {"HK_LIB_PATH": "/parent/libhk.so"}
    r = run_child(_child_report_env, switches={"HK_INWAVE": "0"}, lib="/variant/libhk.so", timeout=120)
    assert _env_of(r) == {"HK_INWAVE": "0", "HK_LIB_PATH": "/variant/libhk.so"}
    assert _env_of(run_child(_child_report_env, lib=None, timeout=120)) == {}


def test_child_failure_brings_its_traceback():
    r = run_child(_child_fails, 4, timeout=120)
    assert not r.ok and r.returncode == 1
    assert "Traceback" in r.output and "the child's own assertion, n=4" in r.output
    assert run_child(_child_fails, 3, timeout=120).ok


def test_child_that_exits_early_is_not_ok():
    r = run_child(_child_exits_early, timeout=120)
    assert r.returncode == 0 and not r.ok
