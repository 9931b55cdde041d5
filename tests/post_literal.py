"""Post-processing and the stored-volume WTA restated in NumPy and Python floats (float64), independent of the C
oracle (oracle/sde_oracle.c) and of the kernels (csrc/postprocess.hip, csrc/wta.hip).

    lr_check         is_error_match_kernel (process_functional.py:977-1000) with the in-row rule of include/sde.h
    lr_consistency   sde_lr_consistency: the statement in test_right_view_host.py, imported, not copied
    lrc_fill         LRC_kernel's left output (:1003-1088), by index scans instead of walks or wave scans
    median5          Median_Filter_kernel (:840-879): the selection sort as written
    wta              WTA1 / WTA (:96-113 / :76-93, rule 'inf') and the SGM WTA kernel (:800-837, rule 'd0')

A float32 converts to a Python float exactly, and every compare and subtraction below is the float64 one the kernels
do, so the results are compared by bytes.  The one rounding is lrc_fill's float64 mean to float32.
"""
import math

import numpy as np

from test_right_view_host import lr_consistency_np as lr_consistency  # noqa: F401


def lr_check(dl, dr, init_l, init_r):
    """(lrc_l, lrc_r, skipped).  A left pixel with d = dl[y, x] looks at c = x - d: when c >= 0 and c is finite,
    col = int(c) & 255 (truncation toward zero, then the low byte of the two's-complement integer, which is
    what Python's & gives for a negative int); when col < W the flag is 1 if |d - dr[y, col]| > 1 else 0.  A
    right pixel likewise with c = x + d, the condition c < W, and dl[y, col].  Every other pixel keeps its init
    byte.  skipped counts the pixels (both sides) that keep it because c is not finite or col >= W, i.e. not
    merely because c is out of the range the reference tests."""
    H, W = dl.shape
    a = np.array(init_l, dtype=np.uint8, copy=True)
    b = np.array(init_r, dtype=np.uint8, copy=True)
    skipped = 0
    for y in range(H):
        for x in range(W):
            d = float(dl[y, x])
            c = x - d
            if not math.isfinite(c):
                skipped += 1
            elif c >= 0:
                col = int(c) & 255
                if col < W:
                    a[y, x] = 1 if abs(d - float(dr[y, col])) > 1 else 0
                else:
                    skipped += 1
            d = float(dr[y, x])
            c = x + d
            if not math.isfinite(c):
                skipped += 1
            elif c < W:
                col = int(c) & 255
                if col < W:
                    b[y, x] = 1 if abs(d - float(dl[y, col])) > 1 else 0
                else:
                    skipped += 1
    return a, b, skipped


def lrc_fill(dl, flags):
    """Every flagged pixel (byte == 1; any other byte is unflagged) becomes the mean of the nearest unflagged
    pixels above, below, to the right and to the left, those that exist, summed in that order in float64 from 0.0,
    divided by their number and rounded to float32 once; with none of the four it keeps its value, as every
    unflagged pixel does.  The four neighbours come from running maxima / minima over index arrays."""
    dl = np.asarray(dl, dtype=np.float32)
    H, W = dl.shape
    flagged = np.asarray(flags) == 1
    rows = np.broadcast_to(np.arange(H)[:, None], (H, W))
    cols = np.broadcast_to(np.arange(W)[None, :], (H, W))
    # nearest unflagged index at or before / at or after each pixel; for a flagged pixel "at" is excluded by itself
    up = np.maximum.accumulate(np.where(flagged, -1, rows), axis=0)
    down = np.minimum.accumulate(np.where(flagged, H, rows)[::-1], axis=0)[::-1]
    left = np.maximum.accumulate(np.where(flagged, -1, cols), axis=1)
    right = np.minimum.accumulate(np.where(flagged, W, cols)[:, ::-1], axis=1)[:, ::-1]
    d64 = dl.astype(np.float64)
    total = np.zeros((H, W), np.float64)
    number = np.zeros((H, W), np.int64)
    for idx, axis, n in ((up, 0, H), (down, 0, H), (right, 1, W), (left, 1, W)):
        ok = (idx >= 0) & (idx < n)
        val = np.take_along_axis(d64, np.clip(idx, 0, n - 1), axis=axis)
        total = np.where(ok, total + val, total)
        number += ok
    with np.errstate(all="ignore"):
        mean = (total / np.maximum(number, 1)).astype(np.float32)
    return np.where(flagged & (number > 0), mean, dl)


def median5(src, dst_init):
    """The 13th value of the reference's partial selection sort of each 5x5 window (row-major), strict `>`, the
    swap written as `w[ci] = w[i]`; interior pixels only, the 2-pixel border keeps dst_init."""
    src = np.asarray(src, dtype=np.float32)
    H, W = src.shape
    out = np.array(dst_init, dtype=np.float32, copy=True)
    rows = src.tolist()
    for y in range(2, H - 2):
        for x in range(2, W - 2):
            w = [rows[y + i][x + j] for i in range(-2, 3) for j in range(-2, 3)]
            cur = 0.0
            for i in range(13):
                cur = w[i]
                ci = i
                for j in range(i + 1, 25):
                    if cur > w[j]:
                        cur = w[j]
                        ci = j
                w[ci] = w[i]
            out[y, x] = cur
    return out


def wta(vol, layout, rule):
    """Sequential scan in increasing d of a 'DHW' or 'HWD' volume -> float32 [H, W].  rule 'inf': start at
    (+inf, -1), replace on v < best.  rule 'd0': start at (vol[0], 0), replace on best > v."""
    vol = np.asarray(vol, dtype=np.float32)
    if layout == "DHW":
        vol = np.moveaxis(vol, 0, 2)
    H, W, D = vol.shape
    out = np.empty((H, W), np.float32)
    for y, row in enumerate(vol.tolist()):
        for x, v in enumerate(row):
            if rule == "inf":
                best, arg = math.inf, -1
                for d in range(D):
                    if v[d] < best:
                        best, arg = v[d], d
            else:
                best, arg = v[0], 0
                for d in range(1, D):
                    if best > v[d]:
                        best, arg = v[d], d
            out[y, x] = arg
    return out
