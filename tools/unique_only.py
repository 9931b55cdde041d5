"""Time the certified fused CV + WTA with and without the uniqueness check, round-robin (measurement driver).

    python tools/unique_only.py [H W D] [--tau 0.1] [--rounds 30] [--parent-lib PATH] [--out FILE.json]

Variants, each timed with HIP events around one call of the C entry point (every variant through the same bare
ctypes call with its arguments prepared beforehand: host work between the two events counts as kernel time at this
size), visited in turn within every round, the starting variant rotating, so that drift of the device's clocks
and the position in the round hit all of them alike:
    parent   sde_cv_wta (certified) of a libsde.so built from the parent commit (--parent-lib; skipped without it)
    plain    sde_cv_wta (certified) of this tree
    unique   sdu_cv_wta_unique (certified) of this tree at --tau
    exact    sdu_cv_wta_unique (exact) of this tree, a few rounds only (the fallback's cost)
Features: unit-norm Gaussian noise, the base features of tests/unique_cases.margin_pair (no planted pairs: at
1024^2 the Gram solves would take minutes on the host).  Prints one JSON object: per variant the median, minimum
and maximum ms over the rounds and the fix-up count, plus the share of pixels rejected.
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


def unit_noise(H, W, seed):
    x = np.random.default_rng(seed).standard_normal((H, W, 64)).astype(np.float32)
    return (x / np.sqrt((x.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[1024, 1024, 192])
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    H, W, D = args.shape
    fl = torch.from_numpy(unit_noise(H, W, 0)).cuda()
    fr = torch.from_numpy(unit_noise(H, W, 1)).cuda()
    ws = torch.empty(ops.cv_wta_workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    disp = torch.empty((H, W), device="cuda")
    rej = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    variants = {}
    pl, pr, pd, pj, pw, nw = fl.data_ptr(), fr.data_ptr(), disp.data_ptr(), rej.data_ptr(), ws.data_ptr(), ws.numel()
    CERT, EXACT, LEFT = _lib.SDE_CV_CERTIFIED, _lib.SDE_CV_EXACT, _lib.SDE_SIDE_LEFT
    tau = ctypes.c_float(args.tau)

    def plain_call(fn):
        def run():
            assert fn(pl, pr, H, W, 64, 0, D, pd, None, None, CERT, pw, nw, stream) == 0
        return run

    def unique_call(mode):
        fn = _lib.lib.sdu_cv_wta_unique

        def run():
            assert fn(pl, pr, H, W, 64, 0, D, LEFT, tau, pd, None, None, pj, mode, pw, nw, stream) == 0
        return run
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.sde_cv_wta.restype, parent.sde_cv_wta.argtypes = _lib.SIGNATURES["sde_cv_wta"]
        variants["parent"] = plain_call(parent.sde_cv_wta)
    variants["plain"] = plain_call(_lib.lib.sde_cv_wta)
    variants["unique"] = unique_call(CERT)
    variants["exact"] = unique_call(EXACT)
    times = {k: [] for k in variants}
    fix = {}
    for k, run in variants.items():      # warm-up, and the fix-up count of each certified variant
        run()
        fix[k] = ops.cv_wta_fixups(ws) if k != "exact" else 0
    rejected = float(rej.float().mean().item())
    names = [k for k in variants if k != "exact"]
    for r in range(args.rounds):
        order = names[r % len(names):] + names[:r % len(names)] + (["exact"] if r < 3 else [])
        for k in order:
            run = variants[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    out = {"shape": [H, W, D], "tau": args.tau, "rounds": args.rounds, "rejected_share": rejected,
           "device": torch.cuda.get_device_name(0), "variants": {
               k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                   "fixups": int(fix[k]), "listed_share": fix[k] / float(H * W)} for k, v in times.items()}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
