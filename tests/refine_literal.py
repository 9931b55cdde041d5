"""The sub-pixel step and the 9x9 bilateral filter restated in NumPy scalars and Python floats, independent of the
kernels (csrc/wta.hip, refine.hip).  include/sde.h states the same three definitions; this file is what the GPU tests compare
against, by bytes.

    refine         the parabola step of WTA_and_SupixelRefinement_kernel (process_functional.py:813-819), with
                   Numba's promotion: float32 difference and sum of the neighbours, float64 from `2*c` on
    wta_subpixel   sde_wta_subpixel: post_literal.wta's winner (imported, not copied), then refine on the volume
    cv_subpixel    sde_cv_subpixel, on the stored [D, H, W] volume of the view (what the kernel recomputes)
    bilateral9     Bilateral_Filter_kernel (:882-974) for one view, the 81 taps in the reference's order

A float32 converts to a Python float exactly and Python's float arithmetic is IEEE float64 with one rounding per
operation, so every float64 step below is the one the kernels do; the float32 steps are np.float32 scalar operations.
"""
import math

import numpy as np

from post_literal import wta

F = np.float32

# the reference's literals (:920-924), stored into a float32 array; entries 5..9 are unreachable behind `< 5`
WEIGHTS = tuple(F(w) for w in (0.167747, 0.165145, 0.157581, 0.145735, 0.130632))


def refine(i, lo, hi, cm, c0, cp):
    """float32(i) unless lo < i < hi - 1, the three float32 costs are finite and den > 0; then
    float32(i - float32(cp - cm) / (2 * (float32(cm + cp) - 2 * c0))) with everything after the two float32
    operations in float64.  No clamp."""
    i = int(i)
    cm, c0, cp = F(cm), F(c0), F(cp)
    if not lo < i < hi - 1:
        return F(i)
    if not (math.isfinite(cm) and math.isfinite(c0) and math.isfinite(cp)):
        return F(i)
    with np.errstate(all="ignore"):
        num = cp - cm                   # np.float32 - np.float32: one float32 rounding
        s = cm + cp
        assert num.dtype == np.float32 and s.dtype == np.float32
        den = 2.0 * (float(s) - 2.0 * float(c0))
        if not den > 0.0:
            return F(i)
        return F(float(i) - float(num) / den)


def wta_subpixel(vol, layout, rule):
    """post_literal.wta's winner, then refine(i, 0, D, ...) on the three costs as they stand in the volume; -1 (no
    winner) stays -1."""
    vol = np.asarray(vol, dtype=np.float32)
    idx = wta(vol, layout, rule)
    hwd = np.moveaxis(vol, 0, 2) if layout == "DHW" else vol
    H, W, D = hwd.shape
    out = np.empty((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            i = int(idx[y, x])
            if 0 < i < D - 1:
                out[y, x] = refine(i, 0, D, hwd[y, x, i - 1], hwd[y, x, i], hwd[y, x, i + 1])
            else:
                out[y, x] = F(i)
    return out


def cv_subpixel(vol_dhw, disp, d0, d1):
    """sde_cv_subpixel given the view's stored [D, H, W] volume (D >= d1): a pixel whose value is an integer i in
    [d0, d1) becomes refine(i, d0, d1, vol[i-1], vol[i], vol[i+1]); any other pixel keeps its bits."""
    vol = np.asarray(vol_dhw, dtype=np.float32)
    disp = np.asarray(disp, dtype=np.float32)
    out = disp.copy()
    H, W = disp.shape
    for y in range(H):
        for x in range(W):
            v = float(disp[y, x])
            if not (v >= d0 and v < d1) or v != int(v):
                continue
            i = int(v)
            if d0 < i < d1 - 1:
                out[y, x] = refine(i, d0, d1, vol[i - 1, y, x], vol[i, y, x], vol[i + 1, y, x])
            else:
                out[y, x] = F(i)
    return out


def bilateral_taps(img, y, x):
    """The 81 taps of pixel (y, x) in the reference's order: (inside the image, row, column, a) with
    a = |int(img[y, x]) - int(I')| and I' = 0 outside the image."""
    H, W = img.shape
    c = int(img[y, x])
    for i in range(-4, 5):
        for j in range(-4, 5):
            r, q = y + i, x + j
            inside = 0 <= r < H and 0 <= q < W
            yield inside, r, q, abs(c - (int(img[r, q]) if inside else 0))


def bilateral9(img, src):
    """wsum and dsum start at 0.0 in float64; every tap with a < 5 adds float64(w) and float64(float32(w * d'))
    with w = WEIGHTS[a] and d' = 0.0 outside the image; the result is float32(dsum / wsum)."""
    img = np.asarray(img, dtype=np.uint8)
    src = np.asarray(src, dtype=np.float32)
    H, W = img.shape
    out = np.empty((H, W), np.float32)
    zero = F(0.0)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                wsum, dsum = 0.0, 0.0
                for inside, r, q, a in bilateral_taps(img, y, x):
                    if a < 5:
                        w = WEIGHTS[a]
                        d = src[r, q] if inside else zero
                        wsum += float(w)
                        dsum += float(w * d)          # np.float32 * np.float32: one float32 rounding
                out[y, x] = F(dsum / wsum)            # the centre tap always counts: wsum > 0
    return out
