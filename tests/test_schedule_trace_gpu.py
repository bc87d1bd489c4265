"""The launch schedule of every kind of handle, call size and scheduling switch against tests/golden/schedule_trace.json.gz (what hk_schedule_info()
reports after each call, and the launches per stage at the checkpoints): a change of the host's scheduling code that is meant to leave the
schedule alone must leave this trace alone.  Every mode runs in a child process (the switches are read once, in hk_create)."""
import os
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_schedule_trace as T      # noqa: E402


@pytest.mark.parametrize("mode", sorted(T.MODES))
def test_schedule_trace(mode):
    golden = T.load_golden()[mode]
    got = T.run_mode(mode)
    assert sorted(got) == sorted(golden)
    for kind in golden:
        want, have = golden[kind], got[kind]
        assert len(have) == len(want), (mode, kind)
        for i, (a, b) in enumerate(zip(have, want)):
            assert a == b, (mode, kind, "step %d of the call pattern" % i, a, b)
