"""Time the fill of left-right-flagged pixels: the mean of four (sde_lrc_fill) against classify + interpolate
(include/sde_interp.h), round-robin (measurement driver).

    python tools/interp_only.py [H W D] [--rounds 30] [--out FILE.json]

The maps are the raw left and right maps of StereoMatcher.match_lr on a synthetic pair (synthetic weights).  Variants,
each timed with HIP events around bare ctypes calls with their arguments prepared beforehand, visited in turn within
every round, the starting variant rotating, so that drift of the device's clocks and the position in the round hit
all of them alike:
    mean4        sde_lr_consistency + sde_lrc_fill                       (a: what the checked path runs today)
    interpolate  sde_lr_consistency + sdi_classify + sdi_interpolate     (b)
    check        sde_lr_consistency alone
    classify     sdi_classify alone, on the flags of the check
    interp       sdi_interpolate alone, on the classes of the maps
    corner       sdi_interpolate alone on a map of mismatches whose only source is the corner pixel (c: the longest
                 walks a map of this size can hold)
    match_lr_mean4 / match_lr_interpolate   StereoMatcher.match_lr() per pair, through the Python host layer
Prints one JSON object: per variant the median, minimum and maximum ms over the rounds, the shares of flagged pixels,
occlusions and mismatches, and the ratios (b)/(a) and (c)/(b).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scenedepthestimation_amd import _lib, ops  # noqa: E402
from scenedepthestimation_amd.pipeline import StereoMatcher  # noqa: E402
from scenedepthestimation_amd.synthetic import stereo_pair  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[1024, 1024, 192])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    H, W, D = args.shape
    left, right, _ = stereo_pair(H, W, D, seed=args.seed)
    matchers = {}
    for fill in ops.FILLS:
        matchers[fill] = StereoMatcher(H, W, D, weights="synthetic", fill=fill)
        matchers[fill].load_images(left, right)
    m = matchers["interpolate"]
    _, disp_r, lrc_l = m.match_lr()
    disp_l = m.disp
    cls = m.checked.interp.cls
    torch.cuda.synchronize()
    shares = {"flagged": float((lrc_l == 1).float().mean()), "occlusions": float((cls == 1).float().mean()),
              "mismatches": float((cls == 2).float().mean())}

    u8 = lambda: torch.empty((H, W), dtype=torch.uint8, device="cuda")   # noqa: E731
    f32 = lambda: torch.empty((H, W), device="cuda")                     # noqa: E731
    fl, fr, c2, filled, out = u8(), u8(), u8(), u8(), f32()
    ws = torch.empty(ops.interpolate_workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    corner_d = torch.full((H, W), -1.0, device="cuda")
    corner_c = torch.full((H, W), 2, dtype=torch.uint8, device="cuda")
    corner_d[0, 0], corner_c[0, 0] = 5.0, 0
    stream = torch.cuda.current_stream().cuda_stream
    lib, LEFT, one = _lib.lib, _lib.SDE_SIDE_LEFT, ctypes.c_float(1.0)
    pl, pr, pfl, pfr, pc, pcls = (t.data_ptr() for t in (disp_l, disp_r, fl, fr, c2, cls))
    pf, po, pw, nw = filled.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()
    pcd, pcc = corner_d.data_ptr(), corner_c.data_ptr()

    def check():
        assert lib.sde_lr_consistency(pl, pr, H, W, one, pfl, pfr, stream) == 0

    def classify():
        assert lib.sdi_classify(pr, pfl, H, W, D, LEFT, one, pc, stream) == 0

    def interp(pd=pl, pk=pcls):
        assert lib.sdi_interpolate(pd, pk, H, W, LEFT, po, pf, pw, nw, stream) == 0

    def mean4():
        check()
        assert lib.sde_lrc_fill(pl, pfl, H, W, po, stream) == 0

    def interpolate():
        check()
        classify()
        interp(pl, pc)

    variants = {"mean4": mean4, "interpolate": interpolate, "check": check, "classify": classify, "interp": interp,
                "corner": lambda: interp(pcd, pcc),
                "match_lr_mean4": matchers["mean4"].match_lr, "match_lr_interpolate": m.match_lr}
    for run in variants.values():      # warm-up
        run()
    torch.cuda.synchronize()
    assert torch.equal(c2, cls)
    times = {k: [] for k in variants}
    names = list(variants)
    for r in range(args.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            variants[k]()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"shape": [H, W, D], "rounds": args.rounds, "seed": args.seed, "device": torch.cuda.get_device_name(0),
           "shares": shares,
           "variants": {k: {"median_ms": med[k], "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
                        for k, v in times.items()},
           "ratio_b_over_a": med["interpolate"] / med["mean4"], "ratio_c_over_b": med["corner"] / med["interpolate"]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
