"""CPU: what the per-ray stage entries and the forward / backward entries REFUSE (include/nerf_hip.h), call by call.

Every call here ends in a refusal that returns before any device work, so the test needs no GPU: pointers are addresses inside one small
host buffer that nothing dereferences.  Each case asserts the return code AND the fragment of nerf_hip_last_error that names the check.

The stage entries share two texts ("null argument", "bad sizes"), so a size that lies INSIDE a bound can only be shown where a later
refusal exists: the quantile entries check q / nq behind the sizes, and an inside size given with nq = 0 must come back with the quantile
text.  The other stage entries launch right behind their size check; for them only the outside values are called.
"""
import ctypes as C

import pytest

ERR_ARG, ERR_WORKSPACE = -1, -2
SAVE = 1  # NERF_HIP_SAVE_FOR_BACKWARD

_buf = (C.c_char * 1024)()
_ADDR = (C.addressof(_buf) + 255) & ~255  # 256-byte aligned (a workspace must be), inside the buffer
_W24 = (C.c_void_p * 24)(*[_ADDR] * 24)   # 24 non-null, 16-byte aligned "tensors"
_Q = (C.c_float * 4)(0.5, 0.25, 0.75, 0.9)

# one row per argument, in the C signature's order: (name, kind).  kind: "req" a pointer the entry refuses when null, "opt" one it accepts
# as null, "q" the three quantile arguments (q, nq, qdepth), "f" / "i" a float / an int, "B" / "Nc" / "Nf" the sizes, "stream"
_COARSE_HEAD = [("t_c", "req"), ("sigma_c", "req"), ("rgb_c", "req"), ("near_far", "req"), ("delta0", "f"), ("B", "B"), ("Nc", "Nc"), ("Nf", "Nf")]
_COARSE_OUT = [("w_c", "opt"), ("C_coarse", "opt"), ("t_f", "req"), ("status", "opt")]
_COARSE_BWD = [("dC_coarse", "req"), ("dt_f", "req")]
_MERGE_HEAD = [("t_c", "req"), ("t_f", "req"), ("sigma_c", "req"), ("sigma_f", "req"), ("rgb_c", "req"), ("rgb_f", "req"), ("B", "B"),
               ("Nc", "Nc"), ("Nf", "Nf"), ("last", "f"), ("bundle", "opt"), ("w", "opt"), ("C_fine", "req")]
_MERGE_BWD_OUT = [("dsig_c", "req"), ("dsig_f", "req"), ("drgb_c", "req"), ("drgb_f", "req"), ("dt_f", "req")]
_MERGE_BWD_HEAD = [("bundle", "req"), ("perm", "req"), ("dC_fine", "req"), ("dmaps", "opt"), ("B", "B"), ("Nc", "Nc"), ("Nf", "Nf"), ("last", "f")]
_ST = [("stream", "stream")]

# name -> (stage kind, the smallest Nc its size check accepts, arguments)
STAGES = {
    "nerf_hip_coarse_composite": ("coarse", 2, _COARSE_HEAD + _COARSE_OUT + _ST),
    "nerf_hip_coarse_composite_maps": ("coarse", 2, _COARSE_HEAD + _COARSE_OUT + [("maps", "req")] + _ST),
    # (this one accepts Nc = 1 where its siblings need Nc >= 2: tests/test_gpu_quantile.py runs it there)
    "nerf_hip_coarse_composite_quantiles": ("coarse", 1, _COARSE_HEAD + _COARSE_OUT + [("maps", "req")] + _ST + [("q", "q")]),
    "nerf_hip_coarse_composite_distortion": ("coarse", 2, _COARSE_HEAD + _COARSE_OUT + [("maps", "req")] + _ST + [("dist", "req")]),
    "nerf_hip_coarse_composite_backward": ("coarse", 2, _COARSE_HEAD + _COARSE_BWD + [("dsig_c", "req"), ("drgb_c", "req")] + _ST),
    "nerf_hip_coarse_composite_backward_maps": ("coarse", 2, _COARSE_HEAD + _COARSE_BWD + [("dmaps", "opt"), ("dsig_c", "req"), ("drgb_c", "req")] + _ST),
    "nerf_hip_coarse_composite_backward_distortion": ("coarse", 2, _COARSE_HEAD + _COARSE_BWD + [("dmaps", "opt"), ("dsig_c", "req"), ("drgb_c", "req")]
                                                      + _ST + [("ddist", "req")]),
    "nerf_hip_merge_composite": ("merge", 1, _MERGE_HEAD + _ST),
    "nerf_hip_merge_composite_train": ("merge", 1, _MERGE_HEAD + [("perm", "req"), ("joint", "i"), ("maps", "opt")] + _ST),
    "nerf_hip_merge_composite_quantiles": ("merge", 1, _MERGE_HEAD + [("perm", "opt"), ("joint", "i"), ("maps", "req")] + _ST + [("q", "q")]),
    "nerf_hip_merge_composite_distortion": ("merge", 1, _MERGE_HEAD + [("perm", "req"), ("joint", "i"), ("maps", "req")] + _ST
                                            + [("near_far", "req"), ("dist", "req")]),
    "nerf_hip_merge_composite_backward": ("merge", 1, _MERGE_BWD_HEAD + _MERGE_BWD_OUT + _ST),
    "nerf_hip_merge_composite_backward_distortion": ("merge", 1, _MERGE_BWD_HEAD + _MERGE_BWD_OUT + _ST + [("near_far", "req"), ("ddist", "req")]),
}

# sizes just outside each bound of the two stage kinds (B, Nc, Nf); Nc = 1 is added for the entries whose bound is Nc >= 2
OUTSIDE = {
    "coarse": [(0, 4, 4), (2, 0, 4), (2, 1025, 4), (2, 4, 0), (2, 4, 1025)],
    "merge": [(0, 4, 4), (2, 0, 4), (2, 4, 0), (2, 1025, 1024), (2, 1, 2048)],  # (Nc + Nf = 2049, twice)
}
# ... and just inside (the smallest Nc is added per entry)
INSIDE = {
    "coarse": [(1, 4, 4), (2, 1024, 4), (2, 4, 1), (2, 4, 1024)],
    "merge": [(1, 4, 4), (2, 4, 1), (2, 1024, 1024), (2, 1025, 1023), (2, 1, 2047)],  # (Nc + Nf = 2048, three ways)
}


def _call(lib, name, args, **over):
    """The entry `name` with every pointer set and sizes (2, 4, 4), except what `over` replaces (a pointer: None = null)."""
    vals = []
    for arg, kind in args:
        if kind == "q":
            vals += [over.get("q", _Q), over.get("nq", 1), over.get("qdepth", _ADDR)]
        elif kind in ("req", "opt"):
            vals.append(over.get(arg, _ADDR))
        elif kind == "f":
            vals.append(0.5)
        elif kind in ("i", "stream"):
            vals.append(None if kind == "stream" else 0)
        else:
            vals.append(over.get(kind, {"B": 2, "Nc": 4, "Nf": 4}[kind]))
    rc = getattr(lib, name)(*vals)
    return rc, lib.nerf_hip_last_error().decode()


def _refused(lib, name, args, text, code=ERR_ARG, **over):
    rc, err = _call(lib, name, args, **over)
    assert rc == code and text in err, (name, over, rc, err)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._abi.lib()


def test_the_table_names_every_stage_entry(pkg):
    stage = [n for n in pkg._abi.EXPORTS if n.startswith(("nerf_hip_coarse_composite", "nerf_hip_merge_composite"))]
    assert sorted(stage) == sorted(STAGES) and len(STAGES) == 13
    for name, (_, _, args) in STAGES.items():  # one row per C argument (the quantile row stands for three)
        assert sum(3 if k == "q" else 1 for _, k in args) == len(pkg._abi._PROTOS[name][1]), name


@pytest.mark.parametrize("name", sorted(STAGES))
def test_stage_entry_refuses_each_null_pointer(lib, name):
    _, _, args = STAGES[name]
    required = [a for a, k in args if k == "req"]
    assert required
    for a in required:
        _refused(lib, name, args, "null argument", **{a: None})
    # null pointers come before sizes: a null pointer AND a bad size is still the null pointer's refusal
    _refused(lib, name, args, "null argument", **{required[0]: None, "B": 0})


@pytest.mark.parametrize("name", sorted(STAGES))
def test_stage_entry_refuses_each_size_outside_its_bounds(lib, name):
    kind, nc_min, args = STAGES[name]
    cases = OUTSIDE[kind] + ([(2, 1, 4)] if nc_min == 2 else [])
    for B, Nc, Nf in cases:
        _refused(lib, name, args, "bad sizes", B=B, Nc=Nc, Nf=Nf)
    if any(k == "q" for _, k in args):  # sizes come before quantiles
        _refused(lib, name, args, "bad sizes", B=0, nq=0)


@pytest.mark.parametrize("name", ["nerf_hip_coarse_composite_quantiles", "nerf_hip_merge_composite_quantiles"])
def test_quantile_stage_entry_accepts_the_sizes_inside_its_bounds(lib, name):
    """Shown by the refusal BEHIND the size check: nq = 0 with a good size is refused with the quantile text.  The optional pointers are
    null here too, so they are shown to be optional the same way."""
    kind, nc_min, args = STAGES[name]
    assert nc_min == 1
    optional = {a: None for a, k in args if k == "opt"}
    for B, Nc, Nf in INSIDE[kind] + [(2, 1, 4)]:  # (Nc = 1: accepted here, refused by every coarse sibling above)
        _refused(lib, name, args, "quantiles per call", B=B, Nc=Nc, Nf=Nf, nq=0, **optional)


@pytest.mark.parametrize("name", ["nerf_hip_coarse_composite_quantiles", "nerf_hip_merge_composite_quantiles"])
def test_quantile_stage_entry_refuses_bad_quantiles(lib, name):
    _, _, args = STAGES[name]
    _refused(lib, name, args, "nq=0: 1 .. 4 quantiles per call", nq=0)
    _refused(lib, name, args, "nq=5: 1 .. 4 quantiles per call", nq=5)
    _refused(lib, name, args, "q or qdepth is null", q=None)
    _refused(lib, name, args, "q or qdepth is null", qdepth=None)
    for bad in (0.0, 1.0, float("nan"), -0.25, 1.5):
        _refused(lib, name, args, "q[0]=", q=(C.c_float * 1)(bad))
        _refused(lib, name, args, "q[2]=", q=(C.c_float * 3)(0.5, 0.5, bad), nq=3)  # (equal quantiles are fine; the third is not)
    rc, err = _call(lib, name, args, q=(C.c_float * 1)(1.0))
    assert rc == ERR_ARG and "strictly inside (0, 1)" in err


# ---- the five forward and the four backward entries ----
_FWD_HEAD = [("weights24", "req"), ("row", "req"), ("col", "req"), ("poses_bound", "req"), ("K_inv9", "req"), ("ray0_near_far", "opt"), ("B", "B"),
             ("Nc", "Nc"), ("Nf", "Nf"), ("last", "f"), ("C_coarse", "req"), ("C_fine", "req")]
_WS = [("ws", "req"), ("ws_bytes", "wsb"), ("flags", "flags"), ("stream", "stream")]
_BWD_HEAD = [("weights24", "req"), ("dC_coarse", "req"), ("dC_fine", "req")]
_BWD_TAIL = [("ray0_near_far", "opt"), ("B", "B"), ("Nc", "Nc"), ("Nf", "Nf"), ("last", "f"), ("dweights24", "req")] + _WS
# name -> (the flags a good call carries, arguments)
FORWARDS = {
    "nerf_hip_forward": (0, _FWD_HEAD + _WS),
    "nerf_hip_forward_maps": (0, _FWD_HEAD + [("maps", "req")] + _WS),
    "nerf_hip_forward_quantiles": (0, _FWD_HEAD + [("maps", "req")] + _WS + [("q", "q")]),
    "nerf_hip_forward_maps_train": (SAVE, _FWD_HEAD + [("maps", "req")] + _WS),
    "nerf_hip_forward_distortion_train": (SAVE, _FWD_HEAD + [("maps", "req")] + _WS + [("dist", "req")]),
}
BACKWARDS = {
    "nerf_hip_backward": (SAVE, _BWD_HEAD + _BWD_TAIL),
    "nerf_hip_backward_overlap": (SAVE, _BWD_HEAD + _BWD_TAIL + [("early_event", "opt")]),
    "nerf_hip_backward_maps": (SAVE, _BWD_HEAD + [("dmaps", "req")] + _BWD_TAIL + [("early_event", "opt")]),
    "nerf_hip_backward_distortion": (SAVE, _BWD_HEAD + [("dmaps", "req")] + _BWD_TAIL + [("early_event", "opt"), ("ddist", "req")]),
}
_B, _NC, _NF = 8, 16, 24


def _call_whole(pkg, name, args, flags, short=0, **over):
    """A forward / backward entry with every pointer set, sizes (8, 16, 24) and a workspace `short` bytes short of nerf_hip_ws_bytes."""
    lib = pkg._abi.lib()
    vals = []
    for arg, kind in args:
        if kind == "q":
            vals += [over.get("q", _Q), over.get("nq", 1), over.get("qdepth", _ADDR)]
        elif arg in ("weights24", "dweights24"):
            vals.append(_W24)
        elif kind in ("req", "opt"):
            vals.append(over.get(arg, None if arg == "early_event" else _ADDR))
        elif kind == "f":
            vals.append(1e-4)
        elif kind == "stream":
            vals.append(None)
        elif kind == "flags":
            vals.append(flags)
        elif kind == "wsb":
            vals.append(pkg._abi.ws_bytes(_B, _NC, _NF, flags) - short)
        else:
            vals.append({"B": _B, "Nc": _NC, "Nf": _NF}[kind])
    rc = getattr(lib, name)(*vals)
    return rc, lib.nerf_hip_last_error().decode()


def test_the_tables_match_the_bindings(pkg):
    for name, (_, args) in {**FORWARDS, **BACKWARDS}.items():
        assert sum(3 if k == "q" else 1 for _, k in args) == len(pkg._abi._PROTOS[name][1]), name


@pytest.mark.parametrize("name", sorted(FORWARDS) + sorted(BACKWARDS))
def test_whole_entry_refuses_a_workspace_one_byte_short(pkg, name):
    flags, args = {**FORWARDS, **BACKWARDS}[name]
    rc, err = _call_whole(pkg, name, args, flags, short=1)
    need = pkg._abi.ws_bytes(_B, _NC, _NF, flags)
    assert rc == ERR_WORKSPACE and f"workspace {need - 1} < {need} bytes" in err, (name, rc, err)


@pytest.mark.parametrize("name,arg,text", [
    ("nerf_hip_forward_maps", "maps", "maps is null"),
    ("nerf_hip_forward_quantiles", "maps", "maps is null"),
    ("nerf_hip_forward_maps_train", "maps", "maps is null"),
    ("nerf_hip_forward_distortion_train", "maps", "maps or dist is null"),
    ("nerf_hip_forward_distortion_train", "dist", "maps or dist is null"),
    ("nerf_hip_backward_maps", "dmaps", "dmaps is null"),
    ("nerf_hip_backward_distortion", "dmaps", "dmaps or ddist is null"),
    ("nerf_hip_backward_distortion", "ddist", "dmaps or ddist is null"),
])
def test_whole_entry_refuses_a_null_optional_output_or_upstream(pkg, name, arg, text):
    flags, args = {**FORWARDS, **BACKWARDS}[name]
    rc, err = _call_whole(pkg, name, args, flags, **{arg: None})
    assert rc == ERR_ARG and err == text, (name, rc, err)


def test_forward_entries_refuse_the_wrong_mode(pkg):
    for name in ("nerf_hip_forward_maps", "nerf_hip_forward_quantiles"):
        rc, err = _call_whole(pkg, name, FORWARDS[name][1], SAVE)
        assert rc == ERR_ARG and err == f"{name} is inference only (NERF_HIP_SAVE_FOR_BACKWARD set)", (name, rc, err)
    for name in ("nerf_hip_forward_maps_train", "nerf_hip_forward_distortion_train"):
        rc, err = _call_whole(pkg, name, FORWARDS[name][1], 0)
        assert rc == ERR_ARG and err == f"{name} is training only (NERF_HIP_SAVE_FOR_BACKWARD not set)", (name, rc, err)
    # the mode comes before the null check
    rc, err = _call_whole(pkg, "nerf_hip_forward_maps", FORWARDS["nerf_hip_forward_maps"][1], SAVE, maps=None)
    assert rc == ERR_ARG and "inference only" in err


def test_forward_quantiles_refuses_bad_quantiles_before_its_workspace(pkg):
    name, args = "nerf_hip_forward_quantiles", FORWARDS["nerf_hip_forward_quantiles"][1]
    for over, text in (({"nq": 0}, "nq=0: 1 .. 4 quantiles per call"), ({"nq": 5}, "nq=5: 1 .. 4 quantiles per call"),
                       ({"q": None}, "q or qdepth is null"), ({"qdepth": None}, "q or qdepth is null"),
                       ({"q": (C.c_float * 1)(0.0)}, "q[0]=0"), ({"q": (C.c_float * 1)(1.0)}, "q[0]=1"),
                       ({"q": (C.c_float * 1)(float("nan"))}, "q[0]=")):
        rc, err = _call_whole(pkg, name, args, 0, short=1, **over)
        assert rc == ERR_ARG and text in err, (over, rc, err)


@pytest.mark.parametrize("name", sorted(BACKWARDS))
def test_backward_entry_refuses_a_call_without_the_save_flag(pkg, name):
    rc, err = _call_whole(pkg, name, BACKWARDS[name][1], 0)
    assert rc == ERR_ARG and "backward needs a forward run with NERF_HIP_SAVE_FOR_BACKWARD" in err, (name, rc, err)
