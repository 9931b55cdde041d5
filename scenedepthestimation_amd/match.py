"""Drop-in for the reference's match.py batch entry point (match.py:19-103).

    python -m scenedepthestimation_amd.match [-g GPUS] [--checkpoint PATH|synthetic] [--cpu-path]
           [--subpixel] [--bilateral] [--calib FILE [--depth-out DIR]] [--unique X] [--speckle-size N [--speckle-range X]]
           [--fill mean4|interpolate]

Loops over ``./test/left_{i}.jpg`` / ``right_{i}.jpg`` for i = 1..18 (match.py:46),
builds the tower once (weights packed and uploaded once, like the single TF
graph of match.py:34-37), and writes ``./disparity/ld{i}.png`` as
``uint8(disparity) * 2`` (match.py:90).  ``detail_time`` accumulates per-stage
seconds as in match.py:71-75 and is printed at the end (the reference's print is
commented out, match.py:95-103).  --subpixel / --bilateral switch on the parabola refinement and the 9x9
bilateral filter the reference carries commented out (process_functional.py:813-819, :882-974); --bilateral
belongs to the SGM path (it filters the median's output).  --calib FILE (new): the inputs are raw camera images
of one rig, rectified on the device from the calibration FILE (rectify.StereoCalibration) before anything else sees
them; --depth-out DIR then also writes ``DIR/depth{i}.pfm`` (rectify.Rectifier.depth).  Without them nothing changes.
--unique X (new; off by default): the uniqueness check with the absolute margin X (see match_single).
--speckle-size N (new; 0 = off): speckle removal as the last stage (see match_single).
--fill interpolate (new; SGM path): occlusion / mismatch interpolation of the flagged pixels (see match_single).

Multi-GPU (new; the reference has none): under torchrun every rank takes pairs
i = rank+1, rank+1+N, ... (pair data-parallel, no collective).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from .local_method import add_fill_flag, add_speckle_flags, add_unique_flag, speckle_option, unique_option
from .match_single import DEFAULT_CKPT, normalise, rectified_pair, write_depth


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="stereo matching based on trained model and post-processing")
    p.add_argument("-g", "--gpu", type=str, default="0,1,2,3,4,5,6,7",
                   help="gpu id to use, multiple ids should be separated by commas (e.g. 0,1,2,3)")
    p.add_argument("--checkpoint", type=str, default=DEFAULT_CKPT)
    p.add_argument("--cpu-path", action="store_true")
    p.add_argument("--ndisp", type=int, default=128)
    p.add_argument("--pairs", type=int, default=18, help="number of pairs (match.py:46 uses 1..18)")
    p.add_argument("--image-path", type=str, default="./test/")
    p.add_argument("--out-path", type=str, default="./disparity/")
    p.add_argument("--subpixel", action="store_true", help="parabola refinement of the winner (off in the reference)")
    p.add_argument("--bilateral", action="store_true",
                   help="9x9 bilateral filter after the median (off in the reference; SGM path only)")
    p.add_argument("--calib", type=str, default=None,
                   help="stereo calibration (.npz / .json): the inputs are raw images, rectified on the device")
    p.add_argument("--depth-out", type=str, default=None, help="with --calib: a directory for depth{i}.pfm")
    add_unique_flag(p)
    add_speckle_flags(p)
    add_fill_flag(p)
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.bilateral and args.cpu_path:
        parser.error("--bilateral filters the median's output: it belongs to the SGM path")
    if args.depth_out and not args.calib:
        parser.error("--depth-out needs --calib (depth comes from the calibration's Q)")
    if args.fill != "mean4" and args.cpu_path:
        parser.error("--fill fills what a left-right check flags: it belongs to the SGM path")
    speckle = speckle_option(parser, args)
    unique = unique_option(parser, args)
    if "WORLD_SIZE" not in os.environ:
        os.environ["HIP_VISIBLE_DEVICES"] = args.gpu     # match.py:24 (CUDA_VISIBLE_DEVICES)
    import torch

    from . import imageio, mc_cnn, ops
    from .parallel import init_from_env, pairs_for_rank
    from .pipeline import StereoMatcher
    from .process_functional import add_detail_time

    rank, world, _ = init_from_env()
    weights = mc_cnn.load_weights(args.checkpoint, 5)
    detail_time = np.zeros(shape=[7], dtype=np.float32)
    matcher = rectifier = None
    if args.calib:
        from .rectify import Rectifier, StereoCalibration
        rectifier = Rectifier(StereoCalibration.load(args.calib))
    for i in [k + 1 for k in pairs_for_rank(args.pairs, world, rank)]:
        lp = os.path.join(args.image_path, "left_{}.jpg".format(i))
        rp = os.path.join(args.image_path, "right_{}.jpg".format(i))
        _l, _r = imageio.imread_gray(lp), imageio.imread_gray(rp)
        if _l is None or _r is None:
            raise AttributeError(f"'NoneType' object has no attribute 'astype' (cannot read {lp} / {rp})")
        if rectifier is not None:
            _l, _r = rectified_pair(rectifier, _l, _r)
        H, W = _l.shape
        if matcher is None or (matcher.H, matcher.W) != (H, W):
            matcher = StereoMatcher(H, W, args.ndisp, weights=weights, subpixel=args.subpixel,
                                    bilateral=args.bilateral, speckle=speckle, unique=unique, fill=args.fill)
        import time
        t0 = time.time()
        # the 5-pixel zero padding of process_functional.py:13-19 (match.py:58-63)
        matcher.load_normalised(*(normalise(img.astype(np.float32))[..., 0] for img in (_l, _r)))
        fl, fr = matcher.features_from_padded()
        torch.cuda.synchronize()
        detail_time[0] += time.time() - t0
        if args.cpu_path:
            if unique is not None:
                disp = ops.cv_wta_unique(fl, fr, 0, args.ndisp, unique, want=("disp",))[0]
            else:
                disp = ops.cv_wta(fl, fr, 0, args.ndisp)[0]
            if args.subpixel:
                ops.cv_subpixel(fl, fr, 0, args.ndisp, disp, "left", out=disp)
            if speckle is not None:
                ops.speckle(disp, speckle[0], speckle[1], out=disp)
            disp = disp.cpu().numpy()
        else:
            # disparity_compute_by_gpu (match.py:85) on the device-resident features: no host round trip
            matcher.load_images(_l, _r)
            timings = {}
            dl, _ = matcher.sgm_path(timings=timings)
            disp = dl.cpu().numpy()
            add_detail_time(detail_time, timings)
        imageio.imwrite(os.path.join(args.out_path, "ld{}.png".format(i)), disp.astype("uint8") * 2)
        if rectifier is not None and args.depth_out:
            os.makedirs(args.depth_out, exist_ok=True)
            write_depth(rectifier, disp, os.path.join(args.depth_out, "depth{}.pfm".format(i)))
    n = max(1, len(pairs_for_rank(args.pairs, world, rank)))
    names = ["computing features", "computing cost volume", '"*" cost aggregation', "SGM",
             "WTA & Subpixel refinement", "LR Check", "Filtering"]
    for name, t in zip(names, detail_time):
        print("time of {}: {}s".format(name, t / n), file=sys.stderr)


if __name__ == "__main__":
    main()
