"""Literal restatement of sdf_speckle, written from the text of include/sde_filter.h: a plain flood fill over
4-neighbours with NumPy float32 arithmetic.  Slow and obvious on purpose; the GPU result is compared with it by
bytes."""
from __future__ import annotations

import numpy as np


def is_valid(v) -> bool:
    """finite and >= 0.0f (-0.0f is)."""
    v = np.float32(v)
    return bool(np.isfinite(v)) and bool(v >= np.float32(0.0))


def linked(a, b, max_diff) -> bool:
    """Both valid and fabsf(a - b) <= max_diff, the subtraction one float32 operation."""
    if not (is_valid(a) and is_valid(b)):
        return False
    return bool(np.abs(np.float32(a) - np.float32(b)) <= np.float32(max_diff))


def region_sizes(disp, max_diff):
    """int32 [H,W]: n(p) for a valid pixel, 0 otherwise."""
    disp = np.asarray(disp, np.float32)
    H, W = disp.shape
    md = np.float32(max_diff)
    ok = np.isfinite(disp) & (disp >= np.float32(0.0))
    vals = disp.tolist()                      # Python floats hold every float32 exactly
    okl = ok.tolist()
    sizes = np.zeros((H, W), np.int32)
    seen = [[False] * W for _ in range(H)]
    f32 = np.float32
    for y0 in range(H):
        for x0 in range(W):
            if not okl[y0][x0] or seen[y0][x0]:
                continue
            seen[y0][x0] = True
            stack, region = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                region.append((y, x))
                v = f32(vals[y][x])
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < H and 0 <= xx < W and okl[yy][xx] and not seen[yy][xx]:
                        # one float32 subtraction, rounded to nearest, then |.| and the comparison in float32
                        if np.abs(v - f32(vals[yy][xx])) <= md:
                            seen[yy][xx] = True
                            stack.append((yy, xx))
            n = len(region)
            for y, x in region:
                sizes[y, x] = n
    return sizes


def speckle(disp, max_size, max_diff, fill):
    """-> (out float32, mask uint8, sizes int32), each [H,W]."""
    disp = np.ascontiguousarray(disp, np.float32)
    sizes = region_sizes(disp, max_diff)
    ok = np.isfinite(disp) & (disp >= np.float32(0.0))
    gone = ok & (sizes <= int(max_size))
    out = disp.copy()                         # bit for bit, NaN payloads and -0.0 included
    out[gone] = np.float32(fill)
    return out, gone.astype(np.uint8), sizes
