"""The interpolation of left-right-flagged pixels (include/sde_interp.h) restated in plain Python loops, written from
the header's text and independent of the kernels (csrc/interp.hip).

    classify             the brute-force scan over the integer candidates dh, as the header states it
    classify_coverage    the second formulation: each other-view pixel marks the columns it makes consistent
    interpolate          the per-pixel walk: row scans for occlusions, 16 ray walks for mismatches
    interpolate_chain    the second formulation: nearest(p) along a ray is the first source among steps 1 and 2,
                         else nearest(p + step 2), so one ordered sweep per direction serves every pixel

A float32 converts to a Python float exactly and every compare below is the float64 one the kernel does; outputs are
copies of inputs (or +0.0), so results are compared by bytes.
"""
import math

import numpy as np

# the 16 directions: the integer pairs (a, b) with max(|a|, |b|) == 2
DIRECTIONS = [(a, b) for a in range(-2, 3) for b in range(-2, 3) if max(abs(a), abs(b)) == 2]


def valid(v):
    v = float(v)
    return math.isfinite(v) and v >= 0.0   # -0.0 >= 0.0


def offset(a, i):
    """o(a, i): +-i for a = +-2, +-ceil(i / 2) for a = +-1, 0 for a = 0."""
    if a == 0:
        return 0
    n = i if abs(a) == 2 else (i + 1) // 2
    return n if a > 0 else -n


def consistent(dh, v, max_diff):
    """NOT (dh - v > max_diff or dh - v < -max_diff) in float64, max_diff a float32 widened."""
    mn = float(dh) - float(v)
    md = float(np.float32(max_diff))
    return not (mn > md or mn < -md)


def classify(disp_other, lrc, D, side, max_diff):
    other = np.asarray(disp_other, dtype=np.float32)
    H, W = other.shape
    rows = other.tolist()
    cls = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if lrc[y, x] != 1:
                continue
            c = 1
            last = min(D - 1, x if side == "left" else W - 1 - x)
            for dh in range(last + 1):
                v = rows[y][x - dh if side == "left" else x + dh]
                if valid(v) and consistent(dh, v, max_diff):
                    c = 2
                    break
            cls[y, x] = c
    return cls


def classify_coverage(disp_other, lrc, D, side, max_diff):
    """Other-view pixel x' with a valid value v covers the columns x' + dh (left view; x' - dh for the right view)
    for the integers dh in [0, D - 1] consistent with v: a handful around v."""
    other = np.asarray(disp_other, dtype=np.float32)
    H, W = other.shape
    covered = np.zeros((H, W), bool)
    md = float(np.float32(max_diff))
    for y in range(H):
        for xo in range(W):
            v = float(other[y, xo])
            if not valid(v):
                continue
            lo = max(0, math.floor(v - md) - 1)
            hi = min(D - 1, math.ceil(v + md) + 1)
            for dh in range(lo, hi + 1):
                x = xo + dh if side == "left" else xo - dh
                if 0 <= x < W and consistent(dh, v, max_diff):
                    covered[y, x] = True
    flagged = np.asarray(lrc) == 1
    return np.where(flagged, np.where(covered, 2, 1), 0).astype(np.uint8)


def _sources(disp, cls):
    c = np.asarray(cls)
    c = np.where((c == 1) | (c == 2), c, 0)
    d = np.asarray(disp, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        src = (c == 0) & np.isfinite(d) & (d >= 0)
    return d, c, src, d + np.float32(0.0)   # a source's value: -0.0 + 0.0 = +0.0


def _median(vals):
    """Element n / 2 of the values sorted ascending (all non-negative finite float32: sorted() is by bits too)."""
    s = sorted(vals, key=float)
    return s[len(s) // 2]


def _occlusion(src_row, val_row, x, W, side):
    left = range(x - 1, -1, -1)
    right = range(x + 1, W)
    for scan in ((left, right) if side == "left" else (right, left)):
        for q in scan:
            if src_row[q]:
                return val_row[q]
    return None


def interpolate(disp, cls, side):
    """-> (out float32, filled uint8) by the per-pixel walk."""
    d, c, src, val = _sources(disp, cls)
    H, W = d.shape
    out = d.copy()
    filled = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if c[y, x] == 0:
                continue
            if c[y, x] == 1:
                got = _occlusion(src[y], val[y], x, W, side)
            else:
                vals = []
                for a, b in DIRECTIONS:
                    i = 1
                    while True:
                        qx, qy = x + offset(a, i), y + offset(b, i)
                        if not (0 <= qx < W and 0 <= qy < H):
                            break
                        if src[qy, qx]:
                            vals.append(val[qy, qx])
                            break
                        i += 1
                got = _median(vals) if vals else None
            if got is not None:
                out[y, x] = got
                filled[y, x] = 1
    return out, filled


def ray_nearest_chain(src, val, a, b):
    """near[y][x] = the value the ray (a, b) from (x, y) yields (None = nothing), for every pixel, by the two-step
    recurrence: the first source among steps 1 and 2, else what the ray from the step-2 pixel yields.  Rows are
    swept so that the step-2 pixel's row is finished first (for a horizontal ray, the columns)."""
    H, W = src.shape
    s1, s2 = (offset(a, 1), offset(b, 1)), (offset(a, 2), offset(b, 2))
    near = [[None] * W for _ in range(H)]
    ys = range(H - 1, -1, -1) if s2[1] > 0 else range(H)
    xs = range(W - 1, -1, -1) if s2[0] > 0 else range(W)
    for y in ys:
        for x in xs:
            got = None
            for k, (dx, dy) in enumerate((s1, s2)):
                qx, qy = x + dx, y + dy
                if not (0 <= qx < W and 0 <= qy < H):
                    break
                if src[qy, qx]:
                    got = val[qy, qx]
                    break
                if k == 1:
                    got = near[qy][qx]
            near[y][x] = got
    return near


def interpolate_chain_sides(disp, cls):
    """interpolate() for both sides, {"left": (out, filled), "right": (out, filled)}, with every ray by
    ray_nearest_chain (the occlusion rows are the rays (-2, 0) and (2, 0)): the sweeps do not depend on the side."""
    d, c, src, val = _sources(disp, cls)
    H, W = d.shape
    near = {ab: ray_nearest_chain(src, val, *ab) for ab in DIRECTIONS}
    left, right = near[(-2, 0)], near[(2, 0)]
    res = {}
    for side in ("left", "right"):
        out = d.copy()
        filled = np.zeros((H, W), np.uint8)
        first, second = (left, right) if side == "left" else (right, left)
        for y in range(H):
            for x in range(W):
                if c[y, x] == 0:
                    continue
                if c[y, x] == 1:
                    got = first[y][x] if first[y][x] is not None else second[y][x]
                else:
                    vals = [near[ab][y][x] for ab in DIRECTIONS if near[ab][y][x] is not None]
                    got = _median(vals) if vals else None
                if got is not None:
                    out[y, x] = got
                    filled[y, x] = 1
        res[side] = (out, filled)
    return res


def interpolate_chain(disp, cls, side):
    return interpolate_chain_sides(disp, cls)[side]


def bad_share(disp, gt, threshold=1.0):
    """The share of pixels with |d - gt| > threshold (a non-finite d counts as bad)."""
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(disp, np.float64) - np.asarray(gt, np.float64))
    return float(np.mean(~(err <= threshold)))
