"""GPU: the LDS-stream MLP kernels (bf16 variant, split-fp32 modes; forward and train step) give, bit for bit, what the commit named in
tests/golden/stream_pinned_digests.json gave.

The digests were recorded on an MI355X from THAT commit's library by tests/tools/stream_pinned_digests.py (never from the tree under
test; every case twice, written only when both recordings agreed): 131, 515 and 853 rays at 64 + 128 samples and 130 rays at 31 + 65, each
as bf16 inference, bf16 inference on the 32x32x16 form, bf16 train step, split-fp32 inference and split-fp32 train step, and both train
steps again with an early event.  Inference: C_coarse, C_fine and the workspace views sig_c, rgb_c, t_f, sig_f, rgb_f; train step:
C_coarse, C_fine, the loss and all 24 gradients.
A change that claims to leave the stream kernels and the weight packers alone (csrc/bf16_common.h's stream tables, bf16_stream.h,
bf16_split.h, bf16_weights.h and the units built on them), or the launch structures of the weight-gradient phase (csrc/dw_bf16.hip), is
held to them."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import stream_pinned_digests as spd  # noqa: E402
import ws_operands as W  # noqa: E402

# ---- which launch structure of the bf16 / split-fp32 weight-gradient phase a train-step entry selects (restated from the library, as
# tests/test_gpu_weight_gradients.py::expected_path does): all four are pinned in both arithmetics
DW_BF16_MULTI_MAX_WB = 5120  # csrc/dw_bf16.hip DW_BF16_MULTI_MAX_WB


def dw_structure(B, Nc, Nf, event):
    wb_tot = W.wave_blocks(B, Nc) + W.wave_blocks(B, Nf)  # csrc/api.hip wave_blocks(), backward_impl()
    small = wb_tot <= DW_BF16_MULTI_MAX_WB                  # csrc/dw_bf16.hip dw_bf16_multi(), launch_dw_bf16_phase()
    return ("small-event" if event else "small") if small else ("large-event" if event else "large")


_reached = {("split" if "split_train" in attrs else "bf16", dw_structure(B, Nc, Nf, event))
            for (B, Nc, Nf, _) in spd.CASES.values() for attrs, train, event in spd.MODES.values() if train}
assert _reached == {(a, s) for a in ("bf16", "split") for s in ("small", "small-event", "large", "large-event")}, _reached


@pytest.fixture(scope="module")
def got(oracle, pkg, dev):
    return spd.digests(oracle, pkg, dev)


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(HERE, "golden", "stream_pinned_digests.json")) as f:
        doc = json.load(f)
    assert doc["recorded_from_commit"]
    return doc["digests"]


@pytest.mark.parametrize("mode", list(spd.MODES))
@pytest.mark.parametrize("case", list(spd.CASES))
def test_stream_bits_are_the_pinned_ones(got, want, case, mode):
    tensors = spd.train_tensors() if spd.MODES[mode][1] else spd.INFERENCE_TENSORS
    assert set(want[case][mode]) == set(tensors)
    bad = [t for t in tensors if got[case][mode][t] != want[case][mode][t]]
    assert not bad, f"{case} / {mode}: {bad} differ from the recorded digests"
