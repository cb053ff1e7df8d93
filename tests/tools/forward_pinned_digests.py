"""SHA-256 digests of the fp32 forward's outputs, for tests/test_gpu_forward_pinned_bits.py.

A change of the forward kernels that must not move a bit is held to digests RECORDED FROM THE PARENT COMMIT'S LIBRARY, never from the
tree under test.  To record (on an MI355X): build the parent commit's library somewhere, then

    NERF_HIP_LIB=/path/to/parent/libnerf_hip.so python tests/tools/forward_pinned_digests.py <parent commit> tests/golden/fwd_f32_pinned_digests.json

The cases: the cfg2 fixture's 4096 rays (64 + 128 samples) with the plain and the sharp weight set of its seed, and one odd-sized render
(130 rays, 31 + 65 samples: partial waves, a partial last tile), each in inference and in saving form.  Digested: C_coarse, C_fine and
the workspace views sig_c, rgb_c, t_f, sig_f, rgb_f (raw little-endian fp32 bytes, C order).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
VIEWS = ["sig_c", "rgb_c", "t_f", "sig_f", "rgb_f"]
CASES = ["cfg2_plain", "cfg2_sharp", "odd_130_31_65"]


def _case(oracle, name):
    """-> (row, col, poses_bound, K_inv, Nc, Nf, weights)"""
    if name == "odd_130_31_65":
        row, col, pb, K, _ = oracle.fern_inputs(130, seed=9)
        return row, col, pb, K, 31, 65, oracle.make_weights(8, sharp=True)
    z = np.load(os.path.join(ROOT, "tests", "golden", "cfg2_lego_rand4096.npz"))
    t = torch.from_numpy
    w = oracle.make_weights(int(z["seed"]), sharp=(name == "cfg2_sharp"))
    return t(z["row"]), t(z["col"]), t(z["poses_bound"]), t(z["K_inv"]), int(z["Nc"]), int(z["Nf"]), w


def _sha(x):
    a = np.ascontiguousarray(x.detach().cpu().numpy())
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


def digests(oracle, pkg, dev):
    """{case: {"inference" | "saving": {tensor: sha256}}} of whatever library the package has loaded."""
    from nerf_tiny_amd import _abi

    out = {}
    for name in CASES:
        row, col, pb, K, Nc, Nf, w = _case(oracle, name)
        B = row.shape[0]
        m = pkg.NeRFModel(Nc, Nf, B)
        m.load_state_dict(w)
        m = m.to(dev)
        shapes = {"sig_c": (B * Nc,), "rgb_c": (B * Nc, 3), "t_f": (B * Nf,), "sig_f": (B * Nf,), "rgb_f": (B * Nf, 3)}
        with torch.no_grad():
            Cc, Cf = m(row, col, pb, K)
        torch.cuda.synchronize()
        ws = m._ws[0][1]
        inf = {"C_coarse": _sha(Cc), "C_fine": _sha(Cf)}
        inf.update({n: _sha(_abi.ws_view(ws, B, Nc, Nf, 0, n, shapes[n])) for n in VIEWS})
        Cc, Cf = m(row, col, pb, K)  # with grad: the saving forward
        torch.cuda.synchronize()
        ws = m.last_workspace
        sav = {"C_coarse": _sha(Cc), "C_fine": _sha(Cf)}
        sav.update({n: _sha(_abi.ws_view(ws, B, Nc, Nf, _abi.SAVE_FOR_BACKWARD, n, shapes[n])) for n in VIEWS})
        out[name] = {"inference": inf, "saving": sav}
    return out


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import nerf_oracle
    import nerf_tiny_amd
    from nerf_tiny_amd import _abi

    commit, dst = sys.argv[1], sys.argv[2]
    d = digests(nerf_oracle, nerf_tiny_amd, torch.device("cuda:0"))
    doc = {"recorded_from_commit": commit, "device": torch.cuda.get_device_name(0), "library": os.path.basename(_abi.LIB_PATH),
           "what": "sha256 of the raw fp32 bytes; see tests/tools/forward_pinned_digests.py", "digests": d}
    with open(dst, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))
