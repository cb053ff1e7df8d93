"""CPU: the training side of the depth / opacity maps -- nerf_hip_forward_maps_train and nerf_hip_backward_maps are
declared, bound and exported under ABI version 7 and refuse what they must before anything touches a device; the driver and the ini parse
the mask weight; the Blender loader keeps each pixel's alpha and leaves the composited RGB as it was."""
import ast
import ctypes
import importlib
import os
import re
from configparser import ConfigParser

import numpy as np
import pytest
import torch

from conftest import ROOT


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)


def test_training_maps_entries_declared_bound_and_exported(pkg):
    hdr = _header()
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr)
    abi = pkg._abi
    so = ctypes.CDLL(abi.LIB_PATH)
    for name in ("nerf_hip_forward_maps_train", "nerf_hip_backward_maps"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in abi.EXPORTS
        assert hasattr(so, name)
    # the training forward takes nerf_hip_forward_maps's arguments; the backward nerf_hip_backward_overlap's with dmaps behind dC_fine
    assert abi._PROTOS["nerf_hip_forward_maps_train"] == abi._PROTOS["nerf_hip_forward_maps"]
    ov = abi._PROTOS["nerf_hip_backward_overlap"][1]
    assert abi._PROTOS["nerf_hip_backward_maps"][1] == ov[:3] + [ctypes.c_void_p] + ov[3:]
    assert abi._PROTOS["nerf_hip_backward_maps"][0] is ctypes.c_int
    assert abi.lib().nerf_hip_abi_version() == 7
    # the entries that existed before keep their prototypes
    assert abi._PROTOS["nerf_hip_forward_maps"][1] == abi._PROTOS["nerf_hip_forward"][1][:12] + [ctypes.c_void_p] + abi._PROTOS["nerf_hip_forward"][1][12:]


def _ptrs():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    w = (ctypes.c_void_p * 24)(*([1 << 20] * 24))  # (pointer values only: nothing is dereferenced before the refusal)
    return buf, p, w


def test_forward_maps_train_refuses_inference_calls_and_null_maps(pkg):
    abi = pkg._abi
    L = abi.lib()
    buf, p, w = _ptrs()
    K9 = abi.f32_array([1, 0, 0, 0, 1, 0, 0, 0, 1])
    call = lambda flags, maps: L.nerf_hip_forward_maps_train(w, p, p, p, K9, None, 8, 64, 128, 1e-4, p, p, maps, ctypes.c_void_p(1 << 20),
                                                             1 << 30, flags, None)
    for flags in (0, abi.BF16_MLP, abi.SPLIT_MLP, abi.CORRECTED, abi.FORCE_TILE_KERNEL):
        with pytest.raises(abi.NerfHipError, match="training only"):
            abi.check(call(flags, p))
    S = abi.SAVE_FOR_BACKWARD
    for flags in (S, S | abi.BF16_MLP, S | abi.SPLIT_MLP, S | abi.CORRECTED, S | abi.FORCE_TILE_KERNEL):
        with pytest.raises(abi.NerfHipError, match="maps is null"):
            abi.check(call(flags, None))
    assert call(0, p) == -1 and call(S, None) == -1  # NERF_HIP_ERR_ARG


def test_backward_maps_refuses_null_dmaps(pkg):
    abi = pkg._abi
    L = abi.lib()
    buf, p, w = _ptrs()
    S = abi.SAVE_FOR_BACKWARD
    for flags in (S, S | abi.BF16_MLP, S | abi.SPLIT_MLP, S | abi.CORRECTED):
        rc = L.nerf_hip_backward_maps(w, p, p, None, None, 8, 64, 128, 1e-4, w, ctypes.c_void_p(1 << 20), 1 << 30, flags, None, None)
        assert rc == -1
        with pytest.raises(abi.NerfHipError, match="dmaps is null"):
            abi.check(rc)


def test_cli_and_ini_parse_the_mask_weight(pkg, tmp_path):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    assert ap.parse_args(["--mask-weight", "0.25"]).mask_weight == 0.25
    assert ap.parse_args([]).mask_weight is None  # -> the ini's MASK_WEIGHT, default 0
    src = open(os.path.join(ROOT, "nerf-tiny_amd", "main.py")).read()
    assert 'kw["mask_weight"] = args.mask_weight if args.mask_weight is not None else float(c("MASK_WEIGHT", 0.0))' in src
    ini = tmp_path / "x.ini"
    ini.write_text("[x]\nMASK_WEIGHT = 0.5\n")
    conf = ConfigParser()
    conf.read(str(ini))
    assert float(conf.get("x", "MASK_WEIGHT", fallback=0.0)) == 0.5
    assert float(conf.get("x", "NOPE", fallback=0.0)) == 0.0
    import inspect

    sig = inspect.signature(pkg.NeRFRunner.__init__)
    assert sig.parameters["mask_weight"].default == 0.0


def test_runner_refuses_a_mask_weight_without_alpha_before_the_gpu(pkg):
    with pytest.raises(ValueError, match="LLFF"):
        pkg.NeRFRunner(data_type="llff", mask_weight=0.1)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mask_weight"):
            pkg.NeRFRunner(mask_weight=bad)


def _write_rgba(tmp, n=3, H=5, W=7):
    import json

    from PIL import Image

    root = str(tmp) + "/"
    os.makedirs(root + "train", exist_ok=True)
    rng = np.random.default_rng(7)
    frames, imgs = [], []
    for i in range(n):
        rgba = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        rgba[0, 0, 3], rgba[0, 1, 3] = 0, 255
        Image.fromarray(rgba, "RGBA").save(root + f"train/r_{i}.png")
        imgs.append(rgba)
        m = np.eye(4)
        m[:3, :4] = rng.standard_normal((3, 4))
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": m.tolist()})
    json.dump({"camera_angle_x": 0.69, "frames": frames}, open(root + "transforms_train.json", "w"))
    return root, imgs


def test_sync_dataset_keeps_alpha_and_its_rgb(pkg, tmp_path):
    from PIL import Image

    root, imgs = _write_rgba(tmp_path)
    ds = pkg.data.NeRFDataset(root_dir=root, low_res=1, transform=None, type="sync", mode="train")
    n, H, W = len(imgs), imgs[0].shape[0], imgs[0].shape[1]
    want_a = torch.from_numpy(np.stack([im[..., 3] for im in imgs]).reshape(-1).astype(np.float64) / 255.0).float()
    assert ds.all_alpha.dtype == torch.float32 and ds.all_alpha.shape == (n * H * W,)
    assert torch.equal(ds.all_alpha, want_a)
    assert float(ds.all_alpha[0]) == 0.0 and float(ds.all_alpha[1]) == 1.0
    # the composited RGB, formed as the loader always formed it (loader.py:67-71): the same bits
    ref = torch.zeros(n, H, W, 3)
    for i, path in enumerate(ds.file_list):
        with Image.open(path) as im:
            im.load()
            bg = Image.new("RGB", im.size, (255, 255, 255))
            bg.paste(im, mask=im.split()[3])
            ref[i] = torch.tensor(np.array(bg) / 255.0)
    assert torch.equal(ds.all_pix, ref.flatten(0, 2))
    assert len(ds[5]) == 5  # the reference's __getitem__ tuple


def test_array_dataset_alpha_is_optional(pkg):
    imgs = torch.rand(2, 3, 4, 3)
    pb = np.zeros((2, 17))
    assert pkg.data.ArrayDataset(imgs, pb).all_alpha is None
    a = torch.rand(2, 3, 4)
    ds = pkg.data.ArrayDataset(imgs, pb, a)
    assert torch.equal(ds.all_alpha, a.flatten())
    with pytest.raises(ValueError, match="alpha"):
        pkg.data.ArrayDataset(imgs, pb, torch.rand(2, 3))
    assert pkg.data.synthetic_scene(n_pic=2, H=4, W=4).all_alpha is None
