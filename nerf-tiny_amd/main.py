"""Driver with the reference's command line (``python main.py --conf=lego``, main.py:10-56) for the MI355X path.

The reference's own main.py cannot run against its shipped configs (three ini keys are missing,
``trainer()`` is called without its required argument, ``LR_MILESTONE`` is parsed into characters); this driver reads
the same 17 keys with defaults for the three missing ones, parses the milestone list properly and calls
``trainer("train")``.  ``--synthetic`` trains on a procedural scene when the datasets are not on disk.

The 8-GPU job of BASELINE.json cfg3 / cfg5 is the same file under a launcher (one process per GPU, RCCL over xGMI):

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \
        nerf-tiny_amd/main.py --conf lego --synthetic --bf16-mlp

Every rank trains on its contiguous slice of each BATCH_RAY batch (ONE flat SUM all-reduce of the gradients per step), rank 0 logs and
checkpoints, ``display()`` renders the frames tile-sharded (``NeRFRunner`` docstring).
"""
import argparse
import ast
import os
import sys
from configparser import ConfigParser

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="NeRF argument parser.")
    ap.add_argument("--conf", type=str, default="lego")
    ap.add_argument("--conf-dir", type=str, default=os.path.join(HERE, "conf"))
    ap.add_argument("--synthetic", action="store_true", help="procedural scene instead of IMG_DIR")
    ap.add_argument("--total-iter", type=int, default=None)
    ap.add_argument("--bf16-mlp", action="store_true", help="run the MLP on bf16 MFMA (cfg3; also ini key BF16_MLP = True)")
    ap.add_argument("--on-resample-fault", choices=["raise", "warn", "ignore"], default=None,
                    help="what to do when a forward met the reference's exit(0) condition (nerf.py:251-253); default raise, like the reference stops")
    ap.add_argument("--split-train", action="store_true", help="train in split-fp32 arithmetic (forward, dX chain and weight gradients on bf16 MFMA with "
                                                               "two-part operands): 2x the exact fp32 step, opt-in (also ini key SPLIT_TRAIN = True)")
    ap.add_argument("--split-mlp", action="store_true", help="render (validation, display) on the split-fp32 inference kernels: same 1e-4 bar, "
                                                             "3x the rate; training is unaffected (also ini key SPLIT_MLP = True)")
    ap.add_argument("--density-grid", type=int, default=None, metavar="RES",
                    help="after display(): write sigma on a RES^3 lattice over --grid-bbox to <RESULTS_PATH><time>_<iter>_sigma<RES>.npz "
                         "(rank 0 only).  With CONTINUE = True and --total-iter at the checkpoint's iteration this exports without training")
    ap.add_argument("--grid-bbox", type=float, nargs=6, default=[-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="box of --density-grid, --mesh and --volume: its lowest and highest lattice corner (default -1.5 .. 1.5 on every axis)")
    ap.add_argument("--mesh", type=int, default=None, metavar="RES",
                    help="after display(): extract the isosurface sigma == --mesh-level on a RES^3 lattice over --grid-bbox (marching cubes on "
                         "the device, vertex colours) to <RESULTS_PATH><time>_<iter>_mesh<RES>.ply (rank 0 only)")
    ap.add_argument("--mesh-level", type=float, default=50.0, metavar="SIGMA", help="density threshold of --mesh (default 50.0)")
    ap.add_argument("--mesh-normals", choices=["grid", "field"], default="grid",
                    help="vertex normals of --mesh: grid = central differences of the lattice (default), field = the field's analytic "
                         "gradient at each vertex (not limited by the grid spacing)")
    ap.add_argument("--mesh-band", type=int, default=None, metavar="R",
                    help="--mesh evaluates the field only in a band of R^3-point blocks around the surface (R >= 2; narrow-band grid: the "
                         "same mesh wherever the band finds the surface, a component smaller than a block can be missed; default: dense)")
    ap.add_argument("--mesh-simplify", type=int, default=None, metavar="K",
                    help="--mesh simplifies the mesh on the device by vertex clustering in cells of K lattice steps (K >= 2; roughly 1 / K^2 "
                         "of the faces), after the floaters are dropped and before normals and colours are queried (default: no simplification)")
    ap.add_argument("--mesh-smooth", type=int, default=None, metavar="N",
                    help="--mesh smooths the vertex positions on the device by N Taubin iterations (N >= 1; boundary vertices stay), after the "
                         "floaters are dropped and before --mesh-simplify; prints the mesh's edge topology (default: no smoothing)")
    ap.add_argument("--mesh-min-faces", type=int, default=None, metavar="N",
                    help="--mesh drops the floaters: connected components of fewer than N faces, labelled and removed on the device before "
                         "normals and colours are queried (with --mesh-band the band may already have missed islands smaller than a block; "
                         "this removes the rest; default: keep everything)")
    ap.add_argument("--mesh-keep-largest", type=int, default=None, metavar="K",
                    help="--mesh keeps only the K connected components with the most faces (ties: the lower component id; combines with "
                         "--mesh-min-faces; default: keep everything)")
    ap.add_argument("--mesh-visible", nargs="?", const="train", default=None, choices=["train", "val", "test"], metavar="SPLIT",
                    help="--mesh drops the faces that no camera of SPLIT (train, val or test; default train) sees: one shadow ray per face "
                         "and camera on the device, after the floaters are dropped and before smoothing, simplification, normals and "
                         "colours; prints the number of faces seen (default: keep everything)")
    ap.add_argument("--mesh-tsdf", nargs="?", const="train", default=None, choices=["train", "val", "test"], metavar="SPLIT",
                    help="--mesh extracts the zero set of a TSDF volume fused on the device from the rendered depth of SPLIT's cameras "
                         "(train, val or test; default train) instead of the isosurface of sigma: --mesh-level and --mesh-band are ignored, "
                         "the file is <...>_mesh<RES>_tsdf.ply (default: the isosurface)")
    ap.add_argument("--mesh-tsdf-trunc", type=float, default=None, metavar="D",
                    help="truncation distance of --mesh-tsdf in world units (default: 4 lattice steps)")
    ap.add_argument("--mesh-tsdf-every", type=int, default=1, metavar="N", help="--mesh-tsdf fuses every N-th camera of the split (default 1)")
    ap.add_argument("--mesh-tsdf-color", action="store_true",
                    help="--mesh-tsdf fuses the colours the rendered views show beside their depth and colours the vertices from that volume; "
                         "only vertices without a fused colour query the field; the file is <...>_tsdf_fused.ply (default: the field's colours)")
    ap.add_argument("--mesh-tsdf-unseen", default="solid", choices=["solid", "empty", "skip"],
                    help="what --mesh-tsdf makes of lattice points no view observed: solid (the mesh closes behind what was seen), empty, or "
                         "skip -- masked marching cubes, only the surface the cameras saw; the file is <...>_tsdf_skip.ply (default solid)")
    ap.add_argument("--mesh-tsdf-depth", default="mean", choices=["mean", "median"],
                    help="the depth --mesh-tsdf fuses: each ray's expected depth, or its median depth (half of the ray's weight in front), which "
                         "stays on one surface at silhouettes and behind thin floaters; the file is <...>_tsdf_median.ply (default mean)")
    ap.add_argument("--mesh-tsdf-max-spread", type=float, default=None, metavar="S",
                    help="--mesh-tsdf leaves out the pixels whose interquartile depth range exceeds S world units (smeared or bimodal rays) "
                         "and prints how many (default: keep every pixel)")
    ap.add_argument("--mesh-texture", type=int, nargs="?", const=2048, default=None, metavar="SIZE",
                    help="--mesh also bakes a texture atlas of at most SIZE x SIZE texels (default 2048) for the final mesh -- the field queried "
                         "at every texel along the inward normal, or with --mesh-tsdf-color the fused colours -- and writes "
                         "<...>_mesh<RES>.obj / .mtl / .png beside the .ply (every face gets the same chart: --mesh-simplify makes the faces "
                         "more uniform first)")
    ap.add_argument("--mesh-compare", default=None, metavar="FILE",
                    help="--mesh measures the extracted mesh against the ground-truth triangle mesh in FILE (PLY, ASCII or binary "
                         "little-endian) on the device: Chamfer distance, precision / recall / F-score, area and volume, printed and written "
                         "to <RESULTS_PATH><time>_<iter>_mesh_eval.json (rank 0)")
    ap.add_argument("--mesh-compare-samples", type=int, default=200_000, metavar="N",
                    help="surface samples per mesh of --mesh-compare (default 200000)")
    ap.add_argument("--mesh-compare-tau", type=float, nargs="+", default=(), metavar="T",
                    help="distance thresholds of --mesh-compare's precision / recall / F-score (up to 8; default: none)")
    ap.add_argument("--volume", type=int, default=None, metavar="RES",
                    help="after display(): bake the field into an SH radiance volume on a RES^3 lattice over --grid-bbox (sigma plus "
                         "spherical-harmonic colour coefficients per lattice point; renders without the network: volume.py) and write it "
                         "to <RESULTS_PATH><time>_<iter>_volume<RES>.npz")
    ap.add_argument("--volume-degree", type=int, default=2, choices=[0, 1, 2],
                    help="spherical-harmonic degree of --volume: 1, 4 or 9 colour coefficients per channel (default 2)")
    ap.add_argument("--volume-sigma-min", type=float, default=0.0, metavar="S",
                    help="--volume sets densities below S to 0 before the bake (default 0: the field's fog is baked too)")
    ap.add_argument("--volume-preview", nargs="?", const="test", default=None, choices=["train", "val", "test"], metavar="SPLIT",
                    help="--volume renders SPLIT's views (train, val or test; default test) from the volume to <i>_volume.png beside the "
                         "frames and prints their PSNR / SSIM against the model's own render of the same views")
    ap.add_argument("--volume-compact", default=None, choices=["fp32", "fp16"],
                    help="--volume writes the compact form: only the rows of the active lattice points behind an int32 slot lattice, the "
                         "coefficients fp32 or fp16 (volume.CompactVolume; the march gives the dense form's bits, fp16 those of the rounded "
                         "coefficients), to <...>_volume<RES>_c32.npz / _c16.npz; the dense coefficient array is never allocated unless "
                         "--volume-finetune is given (default: the dense form)")
    ap.add_argument("--volume-vq", type=int, default=None, metavar="K",
                    help="--volume-compact also writes the vector-quantised FILE form (volume.quantize): every row is scored by the "
                         "rendering weight the train views give it, the rows are replaced by an index into a K-code k-means codebook "
                         "(1 .. 65536), to <the compact file's stem>_vq<K>.npz; volume.dequantize turns the file back into the compact "
                         "form, device memory is not reduced (default: none)")
    ap.add_argument("--volume-vq-iters", type=int, default=10, metavar="N", help="k-means iterations of --volume-vq (default 10)")
    ap.add_argument("--volume-vq-prune", type=float, default=None, metavar="SHARE",
                    help="--volume-vq drops the least important rows that together hold at most SHARE of the importance (default: none)")
    ap.add_argument("--volume-vq-keep", type=float, default=0.0, metavar="SHARE",
                    help="--volume-vq keeps verbatim the most important rows that together hold at most SHARE of the importance (default 0)")
    ap.add_argument("--volume-vq-finetune", type=int, default=0, metavar="ITERS",
                    help="--volume-vq then fine-tunes the quantised form for ITERS Adam steps against the train split's own pixels -- the "
                         "codebook, the kept rows and sigma, the codes frozen (volume.finetune_vq) -- and also writes "
                         "<...>_vq<K>_ft<ITERS>.npz, a file of the same size (default 0: the quantisation alone)")
    ap.add_argument("--volume-vq-finetune-batch", type=int, default=4096, metavar="N",
                    help="rays per --volume-vq-finetune step, at most 2^20 (default 4096)")
    ap.add_argument("--volume-vq-lr-sigma", type=float, default=None, metavar="X",
                    help="--volume-vq-finetune's Adam rate of sigma (default: volume.VQFinetuner's 0.1)")
    ap.add_argument("--volume-vq-lr-coef", type=float, default=None, metavar="X",
                    help="--volume-vq-finetune's Adam rate of the codebook and the kept rows (default: volume.VQFinetuner's 0.01)")
    ap.add_argument("--volume-finetune", type=int, default=0, metavar="ITERS",
                    help="--volume then fine-tunes the baked sigma and coefficients for ITERS Adam steps against the train split's own "
                         "pixels with the support frozen (volume.finetune; rank 0) and also writes <...>_volume<RES>_ft<ITERS>.npz; with "
                         "--volume-preview the PSNR / SSIM against the split's ground-truth images before and after are printed (default 0: "
                         "the bake alone)")
    ap.add_argument("--volume-finetune-compact", action="store_true",
                    help="--volume-finetune trains the compact form itself (needs --volume-compact): the bake goes straight into fp32 rows, "
                         "the accumulators and the Adam moments are kept per row (volume.finetune_compact), and the dense coefficient array "
                         "is never allocated; the files hold the same arrays as without it (default: fine-tune the dense form)")
    ap.add_argument("--volume-finetune-batch", type=int, default=4096, metavar="N",
                    help="rays per --volume-finetune step (default 4096)")
    ap.add_argument("--volume-lr-sigma", type=float, default=None, metavar="X",
                    help="--volume-finetune's Adam rate of sigma (default: volume.Finetuner's 0.1)")
    ap.add_argument("--volume-lr-coef", type=float, default=None, metavar="X",
                    help="--volume-finetune's Adam rate of the SH coefficients (default: volume.Finetuner's 0.01)")
    ap.add_argument("--volume-tv-sigma", type=float, default=0.0, metavar="X",
                    help="--volume-finetune adds X * the mean total variation of sigma over the active lattice points to its loss "
                         "(default 0: no prior)")
    ap.add_argument("--volume-tv-coef", type=float, default=0.0, metavar="X",
                    help="--volume-finetune adds X * the mean total variation of the SH coefficients (summed over the words) to its loss "
                         "(default 0)")
    ap.add_argument("--volume-upsample-at", type=int, nargs="+", default=(), metavar="I",
                    help="--volume-finetune doubles the lattice (2 n - 1 points per axis, trilinear) after step I (strictly increasing, each in "
                         "(0, ITERS)) and goes on with a fresh optimiser; k of them write <...>_volume<RES>_ft<ITERS>_up<k>.npz")
    ap.add_argument("--volume-prune", type=float, default=None, metavar="X",
                    help="before each --volume-upsample-at doubling, densities at or below X become 0 and the coefficients nothing reads "
                         "any more are cleared (default: no pruning)")
    ap.add_argument("--mask-weight", type=float, default=None, metavar="LAMBDA",
                    help="train with ray_loss + LAMBDA * the alpha-mask loss on the opacity maps (needs RGBA images; ini key MASK_WEIGHT; default 0)")
    ap.add_argument("--dist-weight", type=float, default=None, metavar="LAMBDA",
                    help="train with ray_loss + LAMBDA * the distortion loss of the fine pass (mip-NeRF 360's regulariser against floaters, "
                         "per-ray depths in units of [near, far]; ini key DIST_WEIGHT; default 0)")
    ap.add_argument("--maps", action="store_true",
                    help="display() also renders every frame's expected depth and opacity: <RESULTS_PATH><time>_<iter>_maps.npz (depth, acc, "
                         "near, far) and <i>_depth.png / <i>_acc.png previews beside the frames (rank 0 writes)")
    ap.add_argument("--normal-map", action="store_true",
                    help="display() also renders every frame's composited field normals (the fine pass; implies --maps): <i>_normal.png "
                         "beside the frames, 0.5 + 0.5 * the unit normal in the world frame, background mid grey (rank 0 writes)")
    ap.add_argument("--eval", action="store_true",
                    help="after display(): PSNR / SSIM / MSE of the display split (the \"test\" dataset) against its ground truth, printed and "
                         "written to <RESULTS_PATH><time>_<iter>_eval.json (rank 0)")
    ap.add_argument("--eval-every", type=int, default=None, metavar="N",
                    help="during training, every N iterations: PSNR / SSIM of the val split, logged and printed (training is unchanged)")
    ap.add_argument("--eval-views", type=int, nargs="+", default=None, metavar="I",
                    help="view indices of --eval and --eval-every (default: every view)")
    return ap


def dist_weight_of(args, conf: ConfigParser) -> float:
    """NeRFRunner's dist_weight: the command line's --dist-weight, else the ini section's DIST_WEIGHT, else 0"""
    return args.dist_weight if args.dist_weight is not None else float(conf.get(args.conf, "DIST_WEIGHT", fallback=0.0))


if __name__ == "__main__":
    import nerf_tiny_amd as P

    args = build_parser().parse_args()
    if args.volume_vq is not None and args.volume_compact is None:
        raise ValueError("--volume-vq needs --volume-compact")  # before any training
    if args.volume_vq_finetune and args.volume_vq is None:
        raise ValueError("--volume-vq-finetune needs --volume-vq")  # before any training
    if args.volume_finetune_compact and (args.volume_compact is None or args.volume_finetune <= 0):
        raise ValueError("--volume-finetune-compact needs --volume-compact and --volume-finetune ITERS > 0")  # before any training
    conf = ConfigParser()
    conf.read(os.path.join(args.conf_dir, args.conf + ".ini"))
    c = lambda k, d=None: conf.get(args.conf, k, fallback=d)
    kw = dict(gpu=int(c("GPU", 0)), img_dir=c("IMG_DIR"), results_path=c("RESULTS_PATH", "./results/"), ckpt_path=c("CKPT_PATH", "./checkpoint/"),
              low_res=int(c("LOW_RES", 1)), total_iter=int(args.total_iter or c("TOTAL_ITER", c("EPOCH", 100000))), batch_ray=int(c("BATCH_RAY", 400)),
              learning=float(c("LEARNING", 1e-3)), lr_gamma=float(c("LR_GAMMA", 0.1)), lr_milestone=list(ast.literal_eval(c("LR_MILESTONE", "[10, 200]"))),
              n_coarse=int(c("N_COARSE", 64)), n_fine=int(c("N_FINE", 128)), data_type=c("DATA_TYPE", "sync"), step=int(c("STEP", 100)),
              decay_end=float(c("DECAY_END", 200000)), sched=c("SCHED", "EXP"), continue_=ast.literal_eval(c("CONTINUE", "False")))
    if args.synthetic:
        scene = P.data.synthetic_scene(n_pic=8, H=64, W=64)
        kw["datasets"] = {"train": scene, "val": scene, "test": scene}
    kw["bf16_mlp"] = args.bf16_mlp or ast.literal_eval(c("BF16_MLP", "False"))
    kw["split_mlp"] = args.split_mlp or ast.literal_eval(c("SPLIT_MLP", "False"))
    kw["split_train"] = args.split_train or ast.literal_eval(c("SPLIT_TRAIN", "False"))
    if args.on_resample_fault or c("ON_RESAMPLE_FAULT"):
        kw["on_resample_fault"] = args.on_resample_fault or c("ON_RESAMPLE_FAULT")
    kw["mask_weight"] = args.mask_weight if args.mask_weight is not None else float(c("MASK_WEIGHT", 0.0))
    kw["dist_weight"] = dist_weight_of(args, conf)
    if args.eval_every is not None:
        kw["eval_every"], kw["eval_views"] = args.eval_every, args.eval_views
    # data-parallel: started as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 .../main.py ...`
    # every rank runs this file; NeRFRunner reads RANK / WORLD_SIZE / LOCAL_RANK from the environment before its first GPU call
    run = P.NeRFRunner(**kw)
    run.trainer("train")
    if args.normal_map:
        run.display(maps=True, normals=True)
    else:
        run.display(maps=args.maps)
    if args.eval:
        r = run.evaluate("disp", views=args.eval_views, save=True)
        if r is not None:
            print(f"[EVAL] {r['iter']} disp [PSNR] {r['psnr']:.3f} dB [SSIM] {r['ssim']:.4f} [MSE] {r['mse']:.3e} [{len(r['views'])} views, "
                  f"{r['seconds']:.2f} s]")
    if args.density_grid is not None:
        run.density_grid(args.density_grid, lo=args.grid_bbox[:3], hi=args.grid_bbox[3:], save=True)
    if args.volume is not None:
        run.bake_volume(args.volume, lo=args.grid_bbox[:3], hi=args.grid_bbox[3:], degree=args.volume_degree, sigma_min=args.volume_sigma_min,
                        save=True, preview=args.volume_preview, finetune=args.volume_finetune, finetune_batch=args.volume_finetune_batch,
                        finetune_lr={k: x for k, x in (("lr_sigma", args.volume_lr_sigma), ("lr_coef", args.volume_lr_coef)) if x is not None},
                        finetune_tv=(args.volume_tv_sigma, args.volume_tv_coef) if (args.volume_tv_sigma or args.volume_tv_coef) else None,
                        finetune_upsample=tuple(args.volume_upsample_at), finetune_prune=args.volume_prune, compact=args.volume_compact,
                        finetune_compact=args.volume_finetune_compact, vq=args.volume_vq, vq_iters=args.volume_vq_iters,
                        vq_prune=args.volume_vq_prune, vq_keep=args.volume_vq_keep, vq_finetune=args.volume_vq_finetune,
                        vq_finetune_batch=args.volume_vq_finetune_batch, vq_lr_sigma=args.volume_vq_lr_sigma,
                        vq_lr_coef=args.volume_vq_lr_coef)
    if args.mesh is not None:
        m = run.extract_mesh(args.mesh, args.mesh_level, lo=args.grid_bbox[:3], hi=args.grid_bbox[3:], save=True, normals=args.mesh_normals,
                             band=args.mesh_band, min_faces=args.mesh_min_faces, keep_largest=args.mesh_keep_largest,
                             simplify=args.mesh_simplify, smooth=args.mesh_smooth, compare=args.mesh_compare,
                             compare_samples=args.mesh_compare_samples, compare_tau=tuple(args.mesh_compare_tau), visible_from=args.mesh_visible,
                             tsdf_from=args.mesh_tsdf, tsdf_trunc=args.mesh_tsdf_trunc, tsdf_every=args.mesh_tsdf_every,
                             tsdf_color=args.mesh_tsdf_color, tsdf_unseen=args.mesh_tsdf_unseen, tsdf_depth_stat=args.mesh_tsdf_depth,
                             tsdf_max_spread=args.mesh_tsdf_max_spread, texture=args.mesh_texture)
        if m is not None and args.mesh_smooth is not None:  # (new with --mesh-smooth; a run without it prints what it printed before)
            import torch

            t = P.mesh.topology(torch.from_numpy(m.faces).to(run.device), len(m.verts))
            print(f"[MESH] {len(m.verts)} vertices, {len(m.faces)} faces; topology: {t.summary()}")
