"""GPU: the fp32 forward gives, bit for bit, what the commit named in tests/golden/fwd_f32_pinned_digests.json gave.

The digests were recorded on an MI355X from THAT commit's library by tests/tools/forward_pinned_digests.py (never from the tree under
test): the cfg2 fixture with the plain and the sharp weight set, and one odd-sized render (130 rays, 31 + 65 samples), in inference
and in saving form -- C_coarse, C_fine and the workspace views sig_c, rgb_c, t_f, sig_f, rgb_f.  A kernel change that claims to leave
the results alone (csrc/field_fwd_reg.hip: encode, accumulator start, colour head) is held to them."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import forward_pinned_digests as fpd  # noqa: E402

TENSORS = ["C_coarse", "C_fine"] + fpd.VIEWS


@pytest.fixture(scope="module")
def got(oracle, pkg, dev):
    return fpd.digests(oracle, pkg, dev)


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(HERE, "golden", "fwd_f32_pinned_digests.json")) as f:
        doc = json.load(f)
    assert doc["recorded_from_commit"]
    return doc["digests"]


@pytest.mark.parametrize("form", ["inference", "saving"])
@pytest.mark.parametrize("case", fpd.CASES)
def test_forward_bits_are_the_pinned_ones(got, want, case, form):
    bad = [t for t in TENSORS if got[case][form][t] != want[case][form][t]]
    assert set(want[case][form]) == set(TENSORS)
    assert not bad, f"{case} / {form}: {bad} differ from the recorded digests"
