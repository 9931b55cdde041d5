"""Time the geometry stage next to what it sits beside, on a 1024x1024 pair by default (D = 192 for the matcher):

    sdg_remap_u8 on the pair (one launch, with and without the valid mask) against the bytes it must move:
        per image and output pixel 8 B of map and 1 B of output, plus each source once;
    the one-off build of both maps (sdg_rectify_map twice), and sdg_reproject (depth, XYZ);
    StereoMatcher.load_raw + match() beside load_images + match(), from host arrays (each call uploads its pair) and
    from device tensors (no upload: what the remap itself adds).

    python tools/rectify_only.py [H W D] [--rounds N] [--iters K] [--path-iters K] [--json PATH]

The calibration is a rig with radial and tangential distortion and a small relative rotation, so the gathers
wander across source rows as they do for a real camera.  The variants alternate within each round (after a
warm-up of every variant), each timed with device events around K back-to-back calls; per variant the JSON
holds every round's ms per call, their median, minimum and maximum.  What must agree is compared once, before the
timing: load_raw with an identity calibration gives load_images' disparity bytes.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scenedepthestimation_amd import ops  # noqa: E402
from scenedepthestimation_amd.pipeline import StereoMatcher  # noqa: E402
from scenedepthestimation_amd.rectify import Rectifier, StereoCalibration, rodrigues  # noqa: E402
from scenedepthestimation_amd.synthetic import stereo_pair  # noqa: E402

HBM_PEAK = 8.0e12   # B/s, the peak DESIGN.md uses


def rig(H, W, identity=False):
    if identity:
        # a power-of-two focal length and an integer centre: the map is (32u, 32v) exactly
        K = np.array([[1024.0, 0, W // 2], [0, 1024.0, H // 2], [0, 0, 1.0]])
        return StereoCalibration(K, np.zeros(5), K, np.zeros(5), np.eye(3), [-0.12, 0, 0], (H, W))
    f = 0.9 * W
    K1 = np.array([[f, 0, W / 2 + 3.5], [0, f, H / 2], [0, 0, 1.0]])
    K2 = np.array([[f, 0, W / 2], [0, f, H / 2 - 2.25], [0, 0, 1.0]])
    return StereoCalibration(K1, [-0.28, 0.09, 0.0008, -0.0006, -0.01], K2, [-0.27, 0.08, -0.0005, 0.0007, -0.012],
                             rodrigues([0.01, -0.02, 0.008]), [-0.12, 0.002, -0.001], (H, W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[1024, 1024, 192])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="calls per timed window, single kernels")
    ap.add_argument("--path-iters", type=int, default=5, help="calls per timed window, matcher paths")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    H, W, D = args.shape
    left, right, _ = stereo_pair(H, W, D, seed=4)
    m = StereoMatcher(H, W, D)

    # what must agree: an identity calibration's load_raw leaves what load_images leaves
    m.load_images(left, right)
    want = m.match().clone()
    m.load_raw(left, right, Rectifier(rig(H, W, identity=True)))
    identity_agrees = bool(torch.equal(m.match(), want))

    rect = Rectifier(rig(H, W))
    raw2 = torch.from_numpy(np.stack([left, right])).cuda()
    dl, dr = raw2[0].clone(), raw2[1].clone()
    out = torch.empty((2, H, W), dtype=torch.uint8, device="cuda")
    valid = torch.empty_like(out)
    rect.remap(raw2, out=out, valid=valid)
    valid_share = float(valid.float().mean())
    maps = torch.empty_like(rect.maps)
    disp = m.match().clone()
    depth = torch.empty((H, W), device="cuda")
    xyz = torch.empty((H, W, 3), device="cuda")

    def build_maps():
        for i in range(2):
            ops.rectify_map(rect.cal[i], H, W, out=maps[i])

    def raw_then_match(l, r):
        m.load_raw(l, r, rect)
        m.match()

    def images_then_match(l, r):
        m.load_images(l, r)
        m.match()

    kernels = {
        "remap_u8_pair": lambda: rect.remap(raw2, out=out),
        "remap_u8_pair_valid": lambda: rect.remap(raw2, out=out, valid=valid),
        "rectify_map_pair": build_maps,
        "reproject_depth": lambda: ops.reproject(disp, rect.Q, 0.0, depth=depth, want=()),
        "reproject_xyz": lambda: ops.reproject(disp, rect.Q, 0.0, xyz=xyz, want=()),
    }
    paths = {
        "load_images_match_host": lambda: images_then_match(left, right),
        "load_raw_match_host": lambda: raw_then_match(left, right),
        "load_images_match_device": lambda: images_then_match(dl, dr),
        "load_raw_match_device": lambda: raw_then_match(dl, dr),
    }
    variants = {**kernels, **paths}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            n = args.iters if name in kernels else args.path_iters
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n)
    med = {k: statistics.median(v) for k, v in times.items()}
    npix, nsrc = H * W, H * W
    # the bytes each kernel cannot avoid
    floor_bytes = {"remap_u8_pair": 2 * (8 + 1) * npix + 2 * nsrc, "remap_u8_pair_valid": 2 * (8 + 2) * npix + 2 * nsrc,
                   "rectify_map_pair": 2 * 8 * npix, "reproject_depth": 8 * npix, "reproject_xyz": 16 * npix}
    floor_ms = {k: b / HBM_PEAK * 1e3 for k, b in floor_bytes.items()}
    result = {"shape": [H, W, D], "rounds": args.rounds, "iters_per_round": args.iters,
              "path_iters_per_round": args.path_iters, "unit": "ms per call", "device": torch.cuda.get_device_name(0),
              "identity_calibration_agrees": identity_agrees, "valid_share_of_rectified_pair": valid_share,
              "hbm_peak_Bps": HBM_PEAK, "floor_bytes": floor_bytes, "floor_ms_at_peak": floor_ms,
              "ratio_to_floor": {k: med[k] / floor_ms[k] for k in floor_bytes},
              "achieved_GBps_of_floor_bytes": {k: b / (med[k] * 1e-3) / 1e9 for k, b in floor_bytes.items()},
              "ratios": {"load_raw_match_over_load_images_match_host":
                         med["load_raw_match_host"] / med["load_images_match_host"],
                         "load_raw_match_over_load_images_match_device":
                         med["load_raw_match_device"] / med["load_images_match_device"]},
              "added_ms": {"host": med["load_raw_match_host"] - med["load_images_match_host"],
                           "device": med["load_raw_match_device"] - med["load_images_match_device"]},
              "variants": {k: {"median": med[k], "min": min(v), "max": max(v), "rounds": v} for k, v in times.items()}}
    text = json.dumps(result, indent=1)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")
    print(text)
    if not identity_agrees:
        sys.exit("load_raw with an identity calibration disagrees with load_images")


if __name__ == "__main__":
    main()
