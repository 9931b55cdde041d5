"""Time the local matcher's fused cost + WTA kernels next to their unfused compositions, at 1024x1024 with
D = 192 (the north-star shape) and D = 200, k = 5 (the reference script's shape).

    python tools/local_only.py [H W] [--rounds N] [--window S] [--json PATH]

Per shape, alternating within each round (after a warm-up of every variant):
  census_wta               both views, fused (ops.census_wta)
  census_cost+wta          both volumes (ops.census_cost) and ops.wta on each
  ad_wta_k5 / ad_wta_k10   fused SAD+SSD (ops.ad_wta) at radius 5 and 10
  ad_cost+wta_k5           the volume (ops.ad_cost) and ops.wta
Each variant is timed with device events around enough back-to-back calls for a window of at least --window
seconds (sized from one timed call); the JSON holds every round's ms per call, their median, minimum and maximum,
and the ratios unfused / fused and k10 / k5.  The outputs of the variants that must agree are compared once,
before the timing.  Exits non-zero when a fused form is not faster than its unfused composition.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scenedepthestimation_amd import ops  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run_shape(H, W, D, rounds, window):
    rng = np.random.default_rng(11)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = np.roll(left, -7, axis=1)                       # a textured pair with a true disparity
    right[:, -7:] = rng.integers(0, 256, (H, 7), dtype=np.uint8)
    pair = torch.from_numpy(np.stack([left, right])).cuda()
    il, ir = pair[0], pair[1]
    census = ops.census_transform(pair)
    cl, cr = census[0], census[1]
    f32 = lambda: torch.empty((H, W), dtype=torch.float32, device="cuda")   # noqa: E731
    dl, dr, ul, ur, da, ua = f32(), f32(), f32(), f32(), f32(), f32()
    vol_l = torch.empty((H, W, D), dtype=torch.float32, device="cuda")
    vol_r = torch.empty((H, W, D), dtype=torch.float32, device="cuda")

    def census_unfused():
        ops.census_cost(cl, cr, D, right=True, out_left=vol_l, out_right=vol_r)
        ops.wta(vol_l, "HWD", "d0", out=ul)
        ops.wta(vol_r, "HWD", "d0", out=ur)

    def ad_unfused():
        ops.ad_cost(il, ir, D, 5, out=vol_l)
        ops.wta(vol_l, "HWD", "d0", out=ua)

    variants = {
        "census_wta": lambda: ops.census_wta(cl, cr, D, disp_l=dl, disp_r=dr),
        "census_cost+wta": census_unfused,
        "ad_wta_k5": lambda: ops.ad_wta(il, ir, D, 5, disp=da),
        "ad_cost+wta_k5": ad_unfused,
        "ad_wta_k10": lambda: ops.ad_wta(il, ir, D, 10, disp=da),
    }
    variants["census_wta"]()
    census_unfused()
    same_census = bool(torch.equal(dl, ul) and torch.equal(dr, ur))
    variants["ad_wta_k5"]()
    ad_unfused()
    same_ad = bool(torch.equal(da, ua))
    iters = {}
    for name, fn in variants.items():
        fn()
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, math.ceil(window * 1e3 / max(timed(fn, 2), 1e-3)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, iters[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"shape": [H, W, D], "unit": "ms per call", "iters_per_round": iters,
            "fused_equals_unfused": {"census": same_census, "ad": same_ad},
            "volume_bytes": 4 * H * W * D,
            "ratios": {"census_unfused_over_fused": med["census_cost+wta"] / med["census_wta"],
                       "ad_unfused_over_fused_k5": med["ad_cost+wta_k5"] / med["ad_wta_k5"],
                       "ad_wta_k10_over_k5": med["ad_wta_k10"] / med["ad_wta_k5"]},
            "variants": {k: {"median": med[k], "min": min(v), "max": max(v), "rounds": v} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[1024, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timing")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    H, W = args.shape
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "shapes": [run_shape(H, W, D, args.rounds, args.window) for D in (192, 200)]}
    text = json.dumps(out, indent=1)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")
    print(text)
    bad = []
    for s in out["shapes"]:
        if not all(s["fused_equals_unfused"].values()):
            bad.append(f"D = {s['shape'][2]}: a fused form differs from its unfused composition")
        for k in ("census_unfused_over_fused", "ad_unfused_over_fused_k5"):
            if s["ratios"][k] <= 1.0:
                bad.append(f"D = {s['shape'][2]}: {k} = {s['ratios'][k]:.2f} (the fused form is not faster)")
    if bad:
        sys.exit("; ".join(bad))


if __name__ == "__main__":
    main()
