"""Drop-in for the reference's match_single.py / match_single_ui.py entry points.

    python -m scenedepthestimation_amd.match_single [-g GPU] [-i ID] [-f FILE]
           [--checkpoint PATH|synthetic] [--cpu-path [--lr-check]] [--ndisp N] [--ui]
           [--subpixel] [--bilateral] [--calib FILE [--depth-out PATH]]
           [--unique X] [--speckle-size N [--speckle-range X]] [--fill mean4|interpolate]

Same flags, paths and outputs as match_single.py:15-57 (and, with --ui,
match_single_ui.py:20-58): reads ``./eval/left_{id}.png`` / ``right_{id}.png``
(``./UI_use/`` with --ui) as grayscale, z-normalises each image in NumPy exactly
as match_single.py:40-43, computes MC-CNN features (compute_feature), runs the
GPU path (disparity_compute_by_gpu) and writes ``./result/{file}/ld{id}.png`` as
``uint8(disparity)`` (x2 with --ui, match_single_ui.py:55).

--cpu-path selects the reference's commented CPU alternative
``WTA1(compute_cost_volume(fl, fr, 128))`` (match_single.py:51-53), computed by
the fused GPU kernel, bit-identical to the NumPy path.  --lr-check (with --cpu-path
only) writes that path's left map after the reference's post-processing instead
(StereoMatcher.match_lr: the right view's map, the left-right check, LRC fill and
the 5x5 median of process_functional.py:977-1088, :840-879).

--subpixel and --bilateral switch on the two stages the reference carries commented out: the parabola step
on the winner's two neighbours (process_functional.py:813-819) and the 9x9 bilateral filter of the median's
output (:882-974).  Both are off by default; --bilateral needs a path that has a median (the SGM path or
--cpu-path --lr-check).  The written PNG is still ``uint8(disparity)``.

--calib FILE (new; the reference rectifies beforehand with OpenCV, Calibration/mycalibration.cpp:826-839): the two
inputs are raw camera images and FILE a calibration (rectify.StereoCalibration: .npz or .json); the pair is rectified
on the device before anything else sees it.  --depth-out PATH then also writes the depth of the result
(rectify.Rectifier.depth, 0 where there is no disparity) as a one-channel .pfm.  Without them nothing changes.

--unique X (new; off by default) applies the uniqueness check (include/sde_unique.h) on whichever path runs: a
winner whose cost is less than X below the best cost at least two disparities away becomes -1 (255 in the PNG, depth
0); on the paths with a left-right check such a left pixel is filled from its neighbours instead.

--speckle-size N (new; 0 = off) removes, as the last stage of whichever path runs, every region of at most N pixels
of the map as matched whose 4-neighbours differ by at most --speckle-range (default 1.0; include/sde_filter.h): its
pixels become -1, which the PNG's uint8 cast shows as 255 and --depth-out as depth 0.

--fill interpolate (new; the default mean4 is the reference's LRC fill) on the paths with a left-right check (the SGM
path, --cpu-path --lr-check): a flagged left pixel is classified as an occlusion or a mismatch and takes the nearest
good value on the background side or the median of the nearest good values along 16 rays (include/sde_interp.h).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from .local_method import add_fill_flag, add_speckle_flags, add_unique_flag, speckle_option, unique_option

DEFAULT_CKPT = r"./check_points_11_11/model_epoch14.ckpt"   # match_single.py:46


def build_parser(ui: bool = False):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="stereo matching based on trained model and post-processing")
    p.add_argument("-g", "--gpu", type=str, default="1,2",
                   help="gpu id to use, multiple ids should be separated by commas (e.g. 0,1,2,3)")
    p.add_argument("-i", "--id", type=int, default=0, help="image_id")
    p.add_argument("-f", "--file", type=str, default="UI_disparity" if ui else "11_11", help="file to save result")
    p.add_argument("--checkpoint", type=str, default=DEFAULT_CKPT,
                   help="weights: .npz/.safetensors with conv{k}/weights:0, conv{k}/biases:0, or 'synthetic[:seed]'")
    p.add_argument("--cpu-path", action="store_true", help="WTA1(compute_cost_volume(...)) instead of the SGM path")
    p.add_argument("--lr-check", action="store_true",
                   help="with --cpu-path: left-right check, LRC fill and 5x5 median on the fused kernels' two views")
    p.add_argument("--ndisp", type=int, default=128, help="disparity range (the reference hard-codes 128)")
    p.add_argument("--ui", action="store_true", default=ui, help="match_single_ui.py paths and x2 output scaling")
    p.add_argument("--subpixel", action="store_true",
                   help="parabola refinement of the winner (process_functional.py:813-819, off in the reference)")
    p.add_argument("--bilateral", action="store_true",
                   help="9x9 bilateral filter after the median (process_functional.py:882-974, off in the reference)")
    p.add_argument("--calib", type=str, default=None,
                   help="stereo calibration (.npz / .json): the inputs are raw images, rectified on the device")
    p.add_argument("--depth-out", type=str, default=None, help="with --calib: write the depth map as a .pfm")
    add_unique_flag(p)
    add_speckle_flags(p)
    add_fill_flag(p)
    return p


def rectified_pair(rectifier, left_raw, right_raw):
    """Two raw host u8 images -> the rectified host pair (one upload, one remap launch, one download)."""
    import torch
    raw2 = torch.from_numpy(np.ascontiguousarray(np.stack([left_raw, right_raw]), np.uint8)).to(rectifier.device)
    pair = rectifier.remap(raw2).cpu().numpy()
    return pair[0], pair[1]


def write_depth(rectifier, disp, path):
    """Host disparity map -> rectifier.depth on the device -> one-channel .pfm."""
    import torch

    from . import pfm
    d = torch.from_numpy(np.ascontiguousarray(disp, np.float32)).to(rectifier.device)
    pfm.save_pfm(path, rectifier.depth(d).cpu().numpy())


def speckle_filtered(disp, speckle):
    """Host disparity map -> ops.speckle on the device -> host map (regions of at most speckle[0] pixels -> -1)."""
    import torch

    from . import ops
    d = torch.from_numpy(np.ascontiguousarray(disp, np.float32)).cuda()
    return ops.speckle(d, speckle[0], speckle[1], out=d)[0].cpu().numpy()


def normalise(img_f32):
    """match_single.py:40-43: per-image (I - mean) / std over axes (0,1), then a channel axis."""
    x = (img_f32 - np.mean(img_f32, axis=(0, 1))) / np.std(img_f32, axis=(0, 1))
    return np.expand_dims(x, axis=2)


def parse_args(argv=None, ui: bool = False):
    p = build_parser(ui)
    args = p.parse_args(argv)
    if args.lr_check and not args.cpu_path:
        p.error("--lr-check needs --cpu-path (the SGM path has its own left-right check)")
    if args.bilateral and args.cpu_path and not args.lr_check:
        p.error("--bilateral filters the median's output: use the SGM path or --cpu-path --lr-check")
    if args.depth_out and not args.calib:
        p.error("--depth-out needs --calib (depth comes from the calibration's Q)")
    if args.fill != "mean4" and args.cpu_path and not args.lr_check:
        p.error("--fill fills what a left-right check flags: use the SGM path or --cpu-path --lr-check")
    args.speckle = speckle_option(p, args)
    args.unique = unique_option(p, args)
    return args


def lr_checked_disparity(left, right, ndisp, checkpoint, subpixel=False, bilateral=False, left_u8=None,
                         speckle=None, unique=None, fill="mean4"):
    """The --lr-check map: compute_feature's tower on the normalised images (the same padded input, so the same
    features as the plain --cpu-path run), then StereoMatcher.lr_checked on them.  bilateral=True needs the left
    u8 image (the filter's intensities); speckle, unique, fill: StereoMatcher's options."""
    import torch

    from . import mc_cnn
    from .pipeline import StereoMatcher
    nlayers = 11 // 2
    H, W = left.shape[:2]
    m = StereoMatcher(H, W, ndisp, weights=mc_cnn.load_weights(checkpoint, nlayers), nlayers=nlayers,
                      subpixel=subpixel, bilateral=bilateral, speckle=speckle, unique=unique, fill=fill)
    if bilateral:
        m.img_u8[0].copy_(torch.from_numpy(np.ascontiguousarray(left_u8, np.uint8)))
    m.load_normalised(left[..., 0], right[..., 0])
    m.features_from_padded()
    disp, _, _ = m.lr_checked()
    return disp.cpu().numpy()


def run(args) -> str:
    # match_single.py:25 sets CUDA_VISIBLE_DEVICES; on ROCm the equivalent is HIP_VISIBLE_DEVICES,
    # set before torch initialises HIP.
    os.environ["HIP_VISIBLE_DEVICES"] = args.gpu
    from . import imageio
    from .process_functional import WTA1, compute_cost_volume, compute_feature, disparity_compute_by_gpu

    image_path = "./UI_use/" if args.ui else "./eval/"
    lp = os.path.join(image_path, "left_{}.png".format(args.id))
    rp = os.path.join(image_path, "right_{}.png".format(args.id))
    _left = imageio.imread_gray(lp)
    _right = imageio.imread_gray(rp)
    if _left is None or _right is None:
        # cv2.imread returns None and the reference then fails on `.astype` (AttributeError)
        raise AttributeError(f"'NoneType' object has no attribute 'astype' (cannot read {lp} / {rp})")
    rectifier = None
    if getattr(args, "calib", None):
        from .rectify import Rectifier, StereoCalibration
        rectifier = Rectifier(StereoCalibration.load(args.calib))
        _left, _right = rectified_pair(rectifier, _left, _right)
    left = normalise(_left.astype(np.float32))
    right = normalise(_right.astype(np.float32))
    subpixel, bilateral = getattr(args, "subpixel", False), getattr(args, "bilateral", False)
    speckle, unique = getattr(args, "speckle", None), getattr(args, "unique", None)
    fill = getattr(args, "fill", "mean4")
    if args.cpu_path and getattr(args, "lr_check", False):
        disp = lr_checked_disparity(left, right, args.ndisp, args.checkpoint, subpixel, bilateral, _left, speckle,
                                    unique, fill)
    else:
        fl, fr = compute_feature(left, right, 11, 11, 64, args.checkpoint)
        if args.cpu_path and (subpixel or unique is not None):
            import torch

            from . import ops
            vol = torch.from_numpy(compute_cost_volume(fl, fr, args.ndisp)).cuda()
            disp = (ops.wta_subpixel if subpixel else ops.wta)(vol, "DHW", "inf")
            assert bool((disp >= 0).all())    # as WTA1 (:109)
            if unique is not None:
                ops.wta_unique(vol, unique, "DHW", "inf", disp=disp, want=())
            disp = disp.cpu().numpy()
        elif args.cpu_path:
            disp = WTA1(compute_cost_volume(fl, fr, args.ndisp))
        else:
            detail_time = np.zeros(shape=[7], dtype=np.float32)
            disp, _, detail_time = disparity_compute_by_gpu(_left, _right, fl, fr, detail_time, ndisp=args.ndisp,
                                                            subpixel=subpixel, bilateral=bilateral, unique=unique,
                                                            fill=fill)
        if speckle is not None:
            disp = speckle_filtered(disp, speckle)
    out = disp.astype("uint8") * 2 if args.ui else disp.astype("uint8")
    path = "./result/{}/ld{}.png".format(args.file, args.id)
    imageio.imwrite(path, out)
    if rectifier is not None and getattr(args, "depth_out", None):
        write_depth(rectifier, disp, args.depth_out)
    return path


def main(argv=None, ui: bool = False):
    args = parse_args(argv, ui)
    path = run(args)
    print(path, file=sys.stderr)


def main_ui(argv=None):
    main(argv, ui=True)


if __name__ == "__main__":
    main()
