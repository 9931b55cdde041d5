"""Time the right view of the fused CV+WTA next to the left view and next to what could be written without it,
flip(cv_wta(flip(fr), flip(fl))), and StereoMatcher.match_lr() next to match(), at 1024x1024x192 by default.

    python tools/cv_right_only.py [H W D] [--rounds N] [--iters K] [--json PATH]

The variants alternate within each round (after a warm-up of every variant), each timed with device events
around K back-to-back calls; per variant the JSON holds every round's ms per call, their median, minimum and
maximum.  The outputs of the variants that must agree are compared once, before the timing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scenedepthestimation_amd import ops  # noqa: E402
from scenedepthestimation_amd.pipeline import StereoMatcher  # noqa: E402
from scenedepthestimation_amd.synthetic import features, stereo_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[1024, 1024, 192])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    H, W, D = args.shape
    fl = torch.from_numpy(features(H, W, seed=0)).cuda()
    fr = torch.from_numpy(features(H, W, seed=1)).cuda()
    ws = torch.empty(ops.cv_wta_workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    disp = torch.empty((H, W), device="cuda")
    disp_f = torch.empty((H, W), device="cuda")
    left, right, _ = stereo_pair(H, W, D, seed=4)
    m = StereoMatcher(H, W, D)
    m.load_images(left, right)

    def flipped():
        # the right view through the left-view entry point: two feature flips, the sweep, one map flip
        ops.cv_wta(fr.flip(1).contiguous(), fl.flip(1).contiguous(), 0, D, disp=disp_f, want=(), workspace=ws)
        return disp_f.flip(1)

    variants = {
        "cv_wta_left": lambda: ops.cv_wta(fl, fr, 0, D, disp=disp, want=(), workspace=ws),
        "cv_wta_right": lambda: ops.cv_wta_right(fl, fr, 0, D, disp=disp, want=(), workspace=ws),
        "flip_cv_wta_flip": flipped,
        "match": m.match,
        "match_lr": m.match_lr,
    }
    ops.cv_wta_right(fl, fr, 0, D, disp=disp, want=(), workspace=ws)
    fix_right = ops.cv_wta_fixups(ws)
    same = bool(torch.equal(disp, flipped()))
    ops.cv_wta(fl, fr, 0, D, disp=disp, want=(), workspace=ws)
    fix_left = ops.cv_wta_fixups(ws)
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    out = {"shape": [H, W, D], "rounds": args.rounds, "iters_per_round": args.iters, "unit": "ms per call",
           "device": torch.cuda.get_device_name(0), "right_equals_flipped_left_of_flipped": same,
           "fixups": {"left": fix_left, "right": fix_right},
           "variants": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}
                        for k, v in times.items()}}
    text = json.dumps(out, indent=1)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")
    print(text)
    if not same:
        sys.exit("the right view differs from flip(cv_wta(flip(fr), flip(fl)))")


if __name__ == "__main__":
    main()
