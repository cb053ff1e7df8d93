"""SHA-256 digests of what the LDS-stream MLP kernels give (bf16 variant and split-fp32 modes, forward and train step), for
tests/test_gpu_stream_pinned_bits.py.

A change of those kernels, their weight packers or their shared headers that must not move a bit is held to digests RECORDED FROM THE
PARENT COMMIT'S LIBRARY, never from the tree under test.  To record (on an MI355X): build the parent commit's library somewhere, then

    NERF_HIP_LIB=/path/to/parent/libnerf_hip.so python tests/tools/stream_pinned_digests.py <parent commit> tests/golden/stream_pinned_digests.json

Every case is recorded twice; the file is written only if the two runs agree in every digest.

The cases are the smallest that reach every instantiation of the stream kernels:
  * 131 rays, 64 + 128 samples: a partial last ray pair of the pair kernel, the 4-wave training workgroups, the fused ray stages, a partial
    coarse workgroup;
  * 515 rays, 64 + 128: both passes exceed 256 workgroups -- the 8-wave training kernels, separate ray-stage launches, a partial last
    workgroup, no pair kernel;
  * 130 rays, 31 + 65: partial waves, no fusion, the non-pair 16x16x32 inference form;
  * 853 rays, 64 + 128: 5128 wave blocks, the smallest batch that selects the large-batch structures of the bf16 / split-fp32
    weight-gradient phase (csrc/dw_bf16.hip DW_BF16_MULTI_MAX_WB = 5120).
Each in seven modes: bf16_mlp inference, bf16_mlp inference with force_tile_kernel (the 32x32x16 form), bf16_mlp train_step, split_mlp
inference, split_train train_step, and the two train steps again with an overlap bucket (parallel.GradBucket.enable_overlap(): the library
records the early event, which selects the other launch structure of the weight-gradient phase).  Digested (raw little-endian fp32 bytes, C order): for inference C_coarse, C_fine and the workspace
views sig_c, rgb_c, t_f, sig_f, rgb_f; for a train step C_coarse, C_fine, the loss and all 24 gradients.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
VIEWS = ["sig_c", "rgb_c", "t_f", "sig_f", "rgb_f"]
CASES = {"r131_64_128": (131, 64, 128, 11), "r515_64_128": (515, 64, 128, 12), "r130_31_65": (130, 31, 65, 9),
         "r853_64_128": (853, 64, 128, 13)}  # rays, Nc, Nf, seed
# mode -> (model attributes, train step?, with an early event?)
MODES = {
    "bf16_inference": ({"bf16_mlp": True}, False, False),
    "bf16_tile_inference": ({"bf16_mlp": True, "force_tile_kernel": True}, False, False),
    "bf16_train_step": ({"bf16_mlp": True}, True, False),
    "split_inference": ({"split_mlp": True}, False, False),
    "split_train_step": ({"split_train": True}, True, False),
    "bf16_train_step_event": ({"bf16_mlp": True}, True, True),
    "split_train_step_event": ({"split_train": True}, True, True),
}
INFERENCE_TENSORS = ["C_coarse", "C_fine"] + VIEWS
N_GRADS = 24


def train_tensors():
    return ["C_coarse", "C_fine", "loss"] + [f"grad{i:02d}" for i in range(N_GRADS)]


def _sha(x):
    a = np.ascontiguousarray(x.detach().cpu().numpy())
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


def digests(oracle, pkg, dev):
    """{case: {mode: {tensor: sha256}}} of whatever library the package has loaded."""
    from nerf_tiny_amd import _abi, parallel

    out = {}
    for name, (B, Nc, Nf, seed) in CASES.items():
        row, col, pb, K, C_true = oracle.fern_inputs(B, seed=seed)
        w = oracle.make_weights(seed, sharp=True)
        shapes = {"sig_c": (B * Nc,), "rgb_c": (B * Nc, 3), "t_f": (B * Nf,), "sig_f": (B * Nf,), "rgb_f": (B * Nf, 3)}
        out[name] = {}
        for mode, (attrs, train, event) in MODES.items():
            m = pkg.NeRFModel(Nc, Nf, B)
            m.load_state_dict(w)
            m = m.to(dev)
            for k, v in attrs.items():
                setattr(m, k, v)
            if train:
                if event:  # the overlap bucket of tests/test_gpu_weight_gradients.py::_step_with_early_copy; p.grad are its views
                    m.grad_bucket = parallel.GradBucket(m.network.parameters()).enable_overlap()
                Cc, Cf, loss = m.train_step(row, col, pb, K, C_true)
                torch.cuda.synchronize()
                if event:
                    m.grad_bucket.consume()
                ps = list(m.network.parameters())
                assert len(ps) == N_GRADS
                d = {"C_coarse": _sha(Cc), "C_fine": _sha(Cf), "loss": _sha(loss)}
                d.update({f"grad{i:02d}": _sha(p.grad) for i, p in enumerate(ps)})
            else:
                with torch.no_grad():
                    Cc, Cf = m(row, col, pb, K)
                torch.cuda.synchronize()
                ws = m.last_workspace
                flags = next(f for f, (_, buf) in m._ws.items() if buf is ws)
                d = {"C_coarse": _sha(Cc), "C_fine": _sha(Cf)}
                d.update({n: _sha(_abi.ws_view(ws, B, Nc, Nf, flags, n, shapes[n])) for n in VIEWS})
            out[name][mode] = d
    return out


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import nerf_oracle
    import nerf_tiny_amd
    from nerf_tiny_amd import _abi

    commit, dst = sys.argv[1], sys.argv[2]
    dev = torch.device("cuda:0")
    d = digests(nerf_oracle, nerf_tiny_amd, dev)
    again = digests(nerf_oracle, nerf_tiny_amd, dev)
    unstable = [(c, mo, t) for c in d for mo in d[c] for t in d[c][mo] if d[c][mo][t] != again[c][mo][t]]
    if unstable:
        sys.exit(f"not written: the two recordings differ in {unstable}")
    doc = {"recorded_from_commit": commit, "device": torch.cuda.get_device_name(0), "library": os.path.basename(_abi.LIB_PATH),
           "what": "sha256 of the raw fp32 bytes; see tests/tools/stream_pinned_digests.py", "digests": d}
    with open(dst, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))
