"""Case tables of the post-processing and stored-volume WTA tests, shared by test_post_host.py (literal against the
C oracle, CPU) and test_gpu_postprocess.py (kernels against the literal).  Inputs are built once per case and handed
out read-only; what makes a case worth running (both flag values present, pixels skipped, ties, NaN that meet a
compare) is asserted in test_post_host.py.
"""
import functools

import numpy as np

from test_right_view_host import lr_maps

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ----------------------------------------------------------------------------
# left-right check
# ----------------------------------------------------------------------------
LR_H = 6
LR_WIDTHS = (40, 255, 256, 257, 300)


@functools.lru_cache(maxsize=None)
def lr_edge_maps(W, H=LR_H):
    """lr_maps (integers, fractions, disparities that point off both row ends) plus what the reference's uint8 column
    cast meets nowhere else: -1 entries (the 'inf' WTA rule's "no winner"), among them a left one in the last
    column of the last row (column W) and a right one in column 0 (column 255); -0.5 (truncates to column 0 from
    c = -0.5); NaN and +-inf; 1e9 and -1e9 (columns far outside the row before the cast); +-3e38 (no int64)."""
    rng = np.random.default_rng(1000 + W)
    dl, dr = lr_maps(rng, H, W, W, negatives=False)
    dl[rng.random((H, W)) < 0.05] = -1.0
    dr[rng.random((H, W)) < 0.05] = -1.0
    dl[H - 1, W - 1] = -1.0
    dl[0, W - 1] = -1.0
    dr[0, 0] = -1.0
    dr[H - 1, 0] = -1.0
    dr[3, 3] = -4.0            # x + d = -1 away from the row end
    dl[2, 3] = -0.5
    dr[2, 0] = -0.5
    for k, v in enumerate((NAN, INF, -INF, 1e9, -1e9, 3e38, -3e38)):
        dl[1, 5 + 2 * k] = v
        dr[4, 6 + 2 * k] = v
        dl[4, W - 2 - 2 * k] = v
        dr[1, W - 3 - 2 * k] = v
    return _frozen(dl, dr)


def lr_nonneg_maps(W, H=LR_H):
    """The maps of the assertion that sde_lr_consistency equals sde_lr_check for W <= 256: no negative entry."""
    return lr_maps(np.random.default_rng(2000 + W), H, W, W, negatives=False)


# ----------------------------------------------------------------------------
# LRC fill
# ----------------------------------------------------------------------------
FILL_SHAPES = ((1, 1), (1, 70), (70, 1), (63, 64), (64, 65), (65, 63), (129, 130))
FILL_FRACS = (0.3, 0.9)
FILL_WIDE = (32768, 32769, 65534)      # 2 B per column of LDS: 64 KiB, the first width past it, the widest accepted


def _fill_disparities(rng, H, W):
    """Integers and fractions, with NaN and +inf entries.  Only +inf: inf - inf would make a NaN whose sign
    depends on the machine, and the comparison is by bytes."""
    dl = rng.integers(0, 60, (H, W)).astype(np.float32) + rng.random((H, W)).astype(np.float32)
    r = rng.random((H, W))
    dl[r < 0.03] = NAN
    dl[r > 0.97] = INF
    return dl


@functools.lru_cache(maxsize=None)
def fill_case(H, W, frac):
    """Flag bytes from {0, 1, 2, 255}: 1 with probability frac, the other three are unflagged."""
    rng = np.random.default_rng(H * 100003 + W * 101 + int(frac * 10))
    dl = _fill_disparities(rng, H, W)
    flags = rng.choice(np.array([0, 2, 255], np.uint8), (H, W))
    flags[rng.random((H, W)) < frac] = 1
    return _frozen(dl, flags)


@functools.lru_cache(maxsize=None)
def fill_wide_case(W, H=3, run=5000):
    """Flag fraction 0.2, a flagged run of `run` columns in row 0 that crosses 64-column chunks, row 1 fully
    flagged."""
    rng = np.random.default_rng(W)
    dl = _fill_disparities(rng, H, W)
    flags = rng.choice(np.array([0, 2, 255], np.uint8), (H, W))
    flags[rng.random((H, W)) < 0.2] = 1
    start = W // 2 - run // 2 + 7
    flags[0, start:start + run] = 1
    flags[0, start - 1] = 0
    flags[0, start + run] = 2
    flags[1, :] = 1
    return _frozen(dl, flags)


# ----------------------------------------------------------------------------
# 5x5 median
# ----------------------------------------------------------------------------
MEDIAN_SHAPES = ((4, 9), (9, 4), (5, 5), (5, 21), (21, 5), (20, 21), (37, 36))
MEDIAN_KINDS = ("ties", "zeros", "nan", "inf", "nan_window")


@functools.lru_cache(maxsize=None)
def median_case(H, W, kind):
    rng = np.random.default_rng(H * 1009 + W * 13 + MEDIAN_KINDS.index(kind))
    src = rng.integers(0, 4, (H, W)).astype(np.float32)               # heavy ties
    if kind == "zeros":
        src = np.where(rng.random((H, W)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        src[rng.random((H, W)) < 0.1] = -1.0
        src[rng.random((H, W)) < 0.1] = 1.0
    elif kind == "nan":
        src[rng.random((H, W)) < 0.05] = NAN
        src[H // 2, W // 2] = NAN
    elif kind == "inf":
        r = rng.random((H, W))
        src[r < 0.3] = INF
        src[r > 0.7] = -INF
        src[rng.random((H, W)) < 0.05] = NAN
        src[0, 0] = NAN
    elif kind == "nan_window":
        src[max(H - 5, 0):, max(W - 5, 0):] = NAN                    # the last interior pixel's window
    return _frozen(src)


# ----------------------------------------------------------------------------
# stored-volume WTA
# ----------------------------------------------------------------------------
WTA_D = (1, 2, 15, 16, 17, 33, 192)
WTA_PIXELS = ((1, 1), (3, 5), (7, 37))
WTA_KINDS = ("ties", "all_inf", "nan", "infs", "nan_row")


@functools.lru_cache(maxsize=None)
def wta_case(H, W, D, kind):
    """An [H, W, D] volume of small integers (ties all over the 16 residues of d the HWD kernel's lanes take),
    and on top of it: nothing; all +inf; NaN at d = 0 of a third of the pixels and at a tenth of the other
    voxels; -inf and +inf entries (+inf at d = 0 too); every voxel of image row H - 1 NaN."""
    rng = np.random.default_rng((H * 64 + W) * 1000 + D * 8 + WTA_KINDS.index(kind))
    vol = rng.integers(0, 4, (H, W, D)).astype(np.float32)
    if D >= 17:
        vol[:, :, 0] += 1.0              # more first minima past lane 0's first element
    if kind == "all_inf":
        vol[:] = INF
    elif kind == "nan":
        vol[rng.random((H, W, D)) < 0.1] = NAN
        vol[rng.random((H, W)) < 0.34, 0] = NAN
        vol[0, 0, 0] = NAN
    elif kind == "infs":
        r = rng.random((H, W, D))
        vol[r < 0.05] = -INF
        vol[r > 0.8] = INF
        vol[rng.random((H, W)) < 0.5, 0] = INF
        vol[H - 1, W - 1, :] = -INF      # all equal at -inf: d = 0 wins
        vol[0, 0, 0], vol[0, 0, D - 1] = INF, -INF
    elif kind == "nan_row":
        vol[H - 1] = NAN
    return _frozen(vol)


def as_layout(vol_hwd, layout):
    return vol_hwd if layout == "HWD" else np.ascontiguousarray(np.moveaxis(vol_hwd, 2, 0))
