"""HK_SPLIT=1: the batch as two halves on two streams (hk_api.hip issue_rounds over two parts) must change nothing but the speed.
The switch is read once per process, so the comparison runs in a child process."""
import pytest
from parity import assert_child, step_both, twin


def _child_split():
    import hierarchicalkarting_amd as hk
    g, o = twin(hk.make_config(8192 + 64, 4, jitter_seed=0x5EED0000))        # (not a multiple of 128: the halves are unequal)
    t = step_both(g, o, (70, 130, 20, 7, 100))                                # start hold, race start in packs, short and long calls
    assert t == 327, t
    print("split ok", t)


@pytest.mark.gpu
def test_split_batch_matches_the_oracle():
    assert "split ok 327" in assert_child(_child_split, switches={"HK_SPLIT": "1"}, timeout=600).output
