"""CPU checks of the bf16 stream / buffer layout constants in csrc/bf16_common.h and bf16_weights.h: the segment starts (the rows of
the two segment tables, from which the header derives its named offsets)
must be the running sums of (tiles x k-steps) in the order the kernels consume them, the streams must be whole 16-fragment
chunks (or padded up to one), and the training buffers' per-wave-block sizes must add up.  A silent edit of one constant
would otherwise only show as wrong numbers on the GPU.  And the training workspace's layout around the weight-gradient slabs."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf-tiny_amd", "csrc")


def _consts(path):
    txt = open(path).read()
    out = {}
    for name, val in re.findall(r"\b([A-Z][A-Z0-9_]*)\s*=\s*(\d+)\s*[,;]", txt):
        out[name] = int(val)
    return out, txt


def _seg_table(txt, table, prefix):
    """rows (s0, nft, ksa, ksb, bt0, pieces) of a BfSeg table of bf16_common.h, keyed by the row names of its enum (without the prefix)"""
    body = re.search(r"constexpr BfSeg %s\[\w+\] = \{(.*?)\};" % table, txt, re.S).group(1)
    rows = [tuple(int(v) for v in m) for m in re.findall(r"\{(-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+)\}", body)]
    names = re.findall(r"\b%s([A-Z0-9]+)\b" % prefix, re.search(r"enum \{ (%s[^}]*) \};" % prefix, txt).group(1))
    assert names[-1] == "N" and len(names) - 1 == len(rows)
    return dict(zip(names[:-1], rows))


def _derived(txt, name, table, row, field="s0"):
    """the header computes `name` from the table row, not from a literal of its own"""
    return re.search(r"\b%s = %s\[%s\]\.%s\b" % (name, table, row, field), txt) is not None


def test_forward_stream_32x32x16():
    c, txt = _consts(os.path.join(CSRC, "bf16_common.h"))
    t = _seg_table(txt, "kFwdSegs", "FSEG_")
    # point_info is folded into dir_info: the sigma head is a tile of its own on h7, dir_info reads gamma_d (2) + h7 (16)
    want = [("L0", 8, 4, 0), ("L1", 8, 16, 0), ("L2", 8, 16, 0), ("L3", 8, 16, 0), ("L4", 8, 16, 4), ("L5", 8, 16, 0), ("L6", 8, 16, 0),
            ("L7", 8, 16, 0), ("SIG", 1, 16, 0), ("DIR", 4, 2, 16), ("COL", 1, 8, 0)]
    assert list(t) == [w[0] for w in want]
    pos = tiles = 0
    start = {}
    for name, nft, ksa, ksb in want:
        s0, r_nft, r_ksa, r_ksb, bt0, pieces = t[name]
        assert (s0, r_nft, r_ksa, r_ksb, bt0) == (pos, nft, ksa, ksb, tiles), name  # starts and bias tiles are running sums
        assert pieces == (2 * nft if nft > 1 else 0), name                            # a ReLU layer's output: two 1-KiB pieces per tile
        start[name] = pos
        pos += nft * (ksa + ksb)
        tiles += nft
    segs = [("BFS_L0", "L0", 0), ("BFS_L1", "L1", 32), ("BFS_L4", "L4", 416), ("BFS_L5", "L5", 576), ("BFS_SIG", "SIG", 960),
            ("BFS_DIR", "DIR", 976), ("BFS_COL", "COL", 1048)]
    for cname, row, at in segs:
        assert start[row] == at and _derived(txt, cname, "kFwdSegs", "FSEG_" + row), cname
    assert re.search(r"BF_NFRAG = bf_seg_end\(kFwdSegs\[FSEG_N - 1\]\)", txt) and pos == 1056 and pos % c["BF_CHUNK"] == 0
    assert "static_assert(bf_segs_tile(kFwdSegs, FSEG_N, BF_NFRAG)" in txt
    # bias tiles: 8 layers x 8, sigma 1, dir 4, colour 1
    assert (t["L0"][4], t["SIG"][4], t["DIR"][4], t["COL"][4], tiles) == (0, 64, 65, 69, 70)
    for cname, row in (("BFB_L0", "L0"), ("BFB_SIGMA", "SIG"), ("BFB_DIR", "DIR"), ("BFB_COL", "COL")):
        assert _derived(txt, cname, "kFwdSegs", "FSEG_" + row, "bt0"), cname
    assert "BF_NBIAS_TILES = BFB_COL + kFwdSegs[FSEG_COL].nft" in txt
    assert tiles * 32 * 4 <= c["BF_BIAS_BYTES"]


def test_backward_stream():
    _, txt = _consts(os.path.join(CSRC, "bf16_common.h"))
    t = _seg_table(txt, "kBwdSegs", "BSEG_")
    want = [("COLT", 4, 4, 0, 8), ("FOLDT", 8, 8, 1, 16)] + [("L%dT" % l, 8, 16, 0, 16) for l in range(7, 0, -1)] + [("G0T", 2, 16, 16, 0)]
    assert list(t) == [w[0] for w in want]
    pos = 0
    start = {}
    for name, nft, ksa, ksb, pieces in want:
        assert t[name] == (pos, nft, ksa, ksb, -1, pieces), name  # no biases in the chain
        start[name] = pos
        pos += nft * (ksa + ksb)
    segs = [("BBS_COLT", "COLT", 0), ("BBS_FOLDT", "FOLDT", 16), ("BBS_L7T", "L7T", 88), ("BBS_L4T", "L4T", 472), ("BBS_L3T", "L3T", 600),
            ("BBS_G0T", "G0T", 984)]
    for cname, row, at in segs:
        assert start[row] == at and _derived(txt, cname, "kBwdSegs", "BSEG_" + row), cname
    # the coarse pass stops in front of the d gamma_p segments
    assert "BBC_NFRAG = BBS_G0T, BBF_NFRAG = bf_seg_end(kBwdSegs[BSEG_G0T])" in txt and start["G0T"] == 984 and pos == 1048
    assert "bf_segs_tile(kBwdSegs, BSEG_G0T, BBC_NFRAG) && bf_segs_tile(kBwdSegs, BSEG_N, BBF_NFRAG)" in txt


def test_forward_stream_16x16x32():
    c, _ = _consts(os.path.join(CSRC, "bf16_weights.h"))  # (the 16x16x32 image's segment table lives beside its element function)
    segs = [("BXS_L0", 16 * 2), ("BXS_L1", 3 * 16 * 8), ("BXS_L4", 16 * 10), ("BXS_L5", 3 * 16 * 8), ("BXS_SIG", 1 * 8),
            ("BXS_DIR", 8 * 9), ("BXS_COL", 1 * 4)]
    pos = 0
    for name, n in segs:
        assert c[name] == pos, name
        pos += n
    assert c["BX_NFRAG"] == pos == 1044
    assert -(-pos // 16) * 16 <= 1056  # padded to whole chunks, it still fits the workspace region of the 32x32x16 image


def test_training_buffers():
    _, txt = _consts(os.path.join(CSRC, "bf16_common.h"))
    # bs_ks: gamma_p 4, h0..h7 16 each, c 8, gamma_d 2;  bg_ks: dpre0..7 16 each, dpre_dir 8, (dz, dspre) 2
    assert "t == BS_GP ? 4 : t < BS_C ? 16 : t == BS_C ? 8 : 2" in txt
    assert "t < BG_D ? 16 : t == BG_D ? 8 : 2" in txt
    assert 4 + 8 * 16 + 8 + 2 == 142 and 8 * 16 + 8 + 2 == 138
    assert "// 142 KiB per wave block" in txt and "// 138" in txt


def test_python_decoder_matches_header():
    """tests/test_gpu_bf16.py decodes the fragment layout with its own copies of the k-step tables"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("t_bf16", os.path.join(ROOT, "tests", "test_gpu_bf16.py"))
    src = open(spec.origin).read()
    assert "BS_KS = [4] + [16] * 8 + [8, 2]" in src and "BG_KS = [16] * 8 + [8, 2]" in src


def _ws_layouts():
    import json

    with open(os.path.join(ROOT, "tests", "golden", "bf16_ws_layout.json")) as f:
        doc = json.load(f)
    assert doc["recorded_from_commit"]
    return doc["layouts"]


WS_MODES = ("bf16_mlp", "split_mlp")
WS_SHAPES = [(2, 2, 1), (131, 64, 128), (853, 64, 128), (3, 1024, 1024)]


@pytest.mark.parametrize("B,Nc,Nf", WS_SHAPES)
@pytest.mark.parametrize("mode", WS_MODES)
def test_training_workspace_layout_is_the_recorded_one(pkg, mode, B, Nc, Nf):
    """The slab region of the bf16 / split-fp32 weight-gradient phase (csrc/dw_bf16.hip dw_bf16_slab_floats(), computed from the product
    table) is part of the workspace layout: bG lies in front of it, mbuf and drgb_c behind it, so either moves if its size does.  Held to
    the values the commit named in tests/golden/bf16_ws_layout.json gave (host-only calls)."""
    import ctypes as C

    _abi = pkg._abi
    want = _ws_layouts()[f"{mode}-{B}x{Nc}+{Nf}"]
    flags = _abi.SAVE_FOR_BACKWARD | {"bf16_mlp": _abi.BF16_MLP, "split_mlp": _abi.SPLIT_MLP}[mode]
    got = {"ws_bytes": _abi.ws_bytes(B, Nc, Nf, flags)}
    for name in ("mbuf", "drgb_c", "bG"):
        off = C.c_size_t(0)
        _abi.check(_abi.lib().nerf_hip_ws_offset(B, Nc, Nf, flags, name.encode(), C.byref(off)))
        got[name] = int(off.value)
    assert got == want
