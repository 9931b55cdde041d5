"""Inputs and closed forms of the cross-based aggregation tests, shared by test_oracle_cbca.py (CPU: the literal and
the box form against the C oracle) and test_gpu_cbca.py (the kernels against the oracle and the box form).  numpy
only.  Inputs are built once per case and handed out read-only.

The images of the older tests (4 grey levels in 3-pixel runs) give support arms of a few pixels whatever L1 is;
plateau_pair gives arms of every length up to M = L1 - 1, and line_covered is the condition every case that uses
it asserts before it runs: which arm lengths the min of both images' arms really reaches.
"""
import functools

import numpy as np

TAU = 0.03                      # with plateau_pair: plateaus differ by >= 0.05, noise sigma 0.002
COVER_DS = (0, 3, 5)            # disparities of the coverage condition: 3 is the pair's own shift
DIRS = ("l", "r", "u", "d")     # byte k of an arms word


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _cuts(rng, n, M):
    """Plateau index of each of n positions: plateau sizes uniform in 1 .. 2M + 3."""
    idx = np.empty(n, np.int64)
    at = k = 0
    while at < n:
        size = int(rng.integers(1, 2 * M + 4))
        idx[at:at + size] = k
        at, k = at + size, k + 1
    return idx


def plateau_pair(rng, H, W, M):
    """Left and right f32 [H, W] images for tau = TAU.  Piecewise constant: plateau (i, j) is the outer product of
    row cuts and column cuts, its level 0.1 * (random integer in 0..4) + 0.05 * ((i + j) & 1), so the four
    neighbours of a plateau (opposite parity) differ from it by an odd multiple of 0.05 and equal random levels
    never merge two plateaus.  Gaussian noise of sigma 0.002 per image.  The right image is the same layout shifted
    by 3 columns (right[y, x] = layout[y, x + 3]: at d = 3 both images' arms are the plateau's own)."""
    ri, ci = _cuts(rng, H, M), _cuts(rng, W + 3, M)
    level = rng.integers(0, 5, (int(ri[-1]) + 1, int(ci[-1]) + 1))
    layout = (0.1 * level[ri][:, ci] + 0.05 * ((ri[:, None] + ci[None, :]) & 1)).astype(np.float32)
    left = layout[:, :W] + rng.standard_normal((H, W)).astype(np.float32) * np.float32(0.002)
    right = layout[:, 3:] + rng.standard_normal((H, W)).astype(np.float32) * np.float32(0.002)
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


# Seeds of the plateau images by (H, W, M); 1 unless that seed misses the case's coverage condition (line_covered,
# asserted by every test that uses the images).
PLATEAU_SEEDS = {(5, 2, 1): 2, (5, 33, 16): 4, (5, 33, 31): 4, (5, 49, 31): 4, (5, 64, 31): 4, (33, 70, 31): 2,
                 (49, 70, 31): 2,
                 # the non-finite cases also need a plateau edge between rows 0 and 3 (a row above it is out of
                 # reach of the poisoned rows 3..8)
                 (9, 300, 13): 23, (9, 300, 31): 23}


@functools.lru_cache(maxsize=None)
def plateau_images(H, W, M):
    return _frozen(*plateau_pair(np.random.default_rng(PLATEAU_SEEDS.get((H, W, M), 1)), H, W, M))


def arm_coverage(al, ar, W, ds):
    """Per direction ("l", "r", "u", "d"): the set of support arms min(al[y, q], ar[y, q - d]) over the valid
    voxels (q >= d) of the disparities ds."""
    al, ar = np.asarray(al, np.uint32), np.asarray(ar, np.uint32)
    out = {k: set() for k in DIRS}
    for d in ds:
        if d >= W:
            continue
        for k, name in enumerate(DIRS):
            a = np.minimum((al[:, d:] >> (8 * k)) & 255, (ar[:, :W - d] >> (8 * k)) & 255)
            out[name].update(int(v) for v in np.unique(a))
    return out


def line_covered(al, ar, axis, M):
    """The coverage condition along the lines of `axis` ("h": rows, length N = W, arms l and r; "v": columns,
    N = H, arms u and d): the support arms over COVER_DS include 0 and min(M, N - 1), and every length 0..M when
    N >= 2M + 3."""
    H, W = al.shape
    N = W if axis == "h" else H
    need = {0, min(M, N - 1)}
    if N >= 2 * M + 3:
        need |= set(range(M + 1))
    cov = arm_coverage(al, ar, W, COVER_DS)
    return all(need <= cov[k] for k in (("l", "r") if axis == "h" else ("u", "d")))


def fill_invalid(cv, value=1.0):
    """In place: the voxels x < d of a left-referenced volume (as the cost-volume kernels fill them)."""
    H, W, D = cv.shape
    for d in range(1, D):
        cv[:, :min(d, W), d] = value
    return cv


def shear(cl, cr):
    """cr with its valid voxels (x + d < W) set to cl[y, x + d, d], the others kept (new array)."""
    H, W, D = cl.shape
    out = np.array(cr, copy=True)
    for d in range(min(D, W)):
        out[:, :W - d, d] = cl[:, d:, d]
    return out


def box_expected(cv, M):
    """One iteration on a flat image (every arm = min(M, distance to the border)) of integer-valued costs, in
    closed form and in int64: for a valid voxel d <= q, l = min(M, q - d), r = min(M, W - 1 - q), u = min(M, y),
    dn = min(M, H - 1 - y); T = sum of cv over [q - l, q + r]; out = f32(f64(sum of T over rows y - u .. y + dn) *
    (1.0 / f64(sum of l + r + 1 over those rows))).  Invalid voxels unchanged.  Every fp64 partial sum of integers
    this small is exact, so the value does not depend on where prefix chains restart."""
    H, W, D = cv.shape
    iv = np.asarray(cv).astype(np.int64)
    assert (iv == cv).all()
    q = np.arange(W)[:, None]
    d = np.arange(D)[None, :]
    valid = d <= q                                              # [W, D]
    lo = np.maximum(np.maximum(q - M, d), 0)                    # q - l
    hi = np.broadcast_to(np.minimum(q + M, W - 1), (W, D))      # q + r
    lo = np.where(valid, lo, 0)
    P = np.zeros((H, W + 1, D), np.int64)
    np.cumsum(iv, axis=1, out=P[:, 1:])
    T = np.take_along_axis(P, np.broadcast_to(hi + 1, (H, W, D)), 1) - \
        np.take_along_axis(P, np.broadcast_to(lo, (H, W, D)), 1)
    n = np.broadcast_to(hi - lo + 1, (H, W, D))
    Q = np.zeros((H + 1, W, D), np.int64)
    C = np.zeros((H + 1, W, D), np.int64)
    np.cumsum(T, axis=0, out=Q[1:])
    np.cumsum(n, axis=0, out=C[1:])
    y = np.arange(H)
    top, bot = np.maximum(y - M, 0), np.minimum(y + M, H - 1) + 1
    num = (Q[bot] - Q[top]).astype(np.float64)
    cnt = (C[bot] - C[top]).astype(np.float64)
    out = (num * (1.0 / cnt)).astype(np.float32)
    return np.where(valid[None], out, np.asarray(cv, np.float32))


def same_f32(a, b):
    """NaN at the same positions, everything else equal byte for byte (NaN payloads are not part of the
    contract: the host and the GPU generate different default NaNs)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.nan_to_num(a, nan=7.0, posinf=np.inf, neginf=-np.inf).tobytes() == \
        np.nan_to_num(b, nan=7.0, posinf=np.inf, neginf=-np.inf).tobytes()


# ----------------------------------------------------------------------------
# line-length sweep
# ----------------------------------------------------------------------------
SWEEP_L1 = (1, 2, 14, 15, 16, 17, 32)
# a greedy cover of the distinct block schedules (first and later segments, peeled blocks, both loop exits,
# tail-block count and parity, the exact seams) of the templates at L1 = 2, 14, 16, 17 and 32
SWEEP_N = (1, 2, 33, 49, 64, 81, 97, 99, 113, 128, 145, 161, 177, 211, 239, 255, 256, 257, 270, 286, 314, 322, 337,
           342, 354, 368, 382, 386, 401, 410, 432, 450, 467, 482, 512, 513, 560)
SWEEP_D = 70


def sweep_shape(axis, N):
    return (5, N, SWEEP_D) if axis == "h" else (N, 70, SWEEP_D)


@functools.lru_cache(maxsize=None)
def _sweep_base(axis):
    H, W, D = sweep_shape(axis, max(SWEEP_N))
    rng = np.random.default_rng(2024 + (axis == "v"))
    return _frozen((rng.standard_normal((H, W, D)) * 3 + 20).astype(np.float32))   # far from 0: rounding matters


def sweep_costs(axis, N, side):
    """The [H, W, D] corner of one standard-normal * 3 + 20 volume per axis; left: voxels x < d hold 1.0."""
    H, W, D = sweep_shape(axis, N)
    cv = np.array(_sweep_base(axis)[:H, :W, :D], order="C", copy=True)
    return fill_invalid(cv) if side == "left" else cv


# ----------------------------------------------------------------------------
# box-filter identity
# ----------------------------------------------------------------------------
BOX_CASES = ((40, 300, 20, 32), (300, 40, 45, 16), (70, 70, 70, 14), (290, 290, 3, 32))     # H, W, D, L1


@functools.lru_cache(maxsize=None)
def box_case(H, W, D, L1):
    """Integer costs in [-8, 8] and their box_expected."""
    rng = np.random.default_rng(H * 1009 + W * 13 + D)
    cv = rng.integers(-8, 9, (H, W, D)).astype(np.float32)
    return _frozen(cv, box_expected(cv, L1 - 1))


# ----------------------------------------------------------------------------
# non-finite costs
# ----------------------------------------------------------------------------
NONFINITE_SHAPES = ((9, 300, 70), (300, 9, 70))
NAN, INF = np.float32(np.nan), np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def nonfinite_volume(H, W, D):
    """(volume, rows): a left-coordinate volume of finite costs (x < d at 1.0) poisoned along the long axis of
    the shape, each poison on a line (row, or column) of its own: a single NaN; +inf and -inf on one line, 5 apart;
    a NaN at the line's last position; NaN at positions 255 and 256; a NaN in an invalid voxel; a whole pixel NaN.
    `rows` are rows without a poisoned voxel, one of which no support of one iteration connects to poison (a
    vertical chain carries a NaN down to the end of its segment, so such a row lies above the poison): rows 0..2
    above the poisoned rows 3..8 (those above a plateau edge of the images the test uses), or row 10, whose
    supports end at row 10 + 31 or above while the first poisoned valid voxel is in row 100."""
    rng = np.random.default_rng(H * 31 + W)
    cv = fill_invalid((rng.standard_normal((H, W, D)) * 3 + 20).astype(np.float32))
    if W >= H:                      # lines = rows, positions = columns
        cv[3, 100, 7] = NAN
        cv[4, 120, 9], cv[4, 125, 9] = INF, -INF
        cv[5, W - 1, 3] = NAN
        cv[6, 255, 11], cv[6, 256, 11] = NAN, NAN
        cv[7, 20, 40] = NAN         # invalid: x < d
        cv[8, 200, :] = NAN
        rows = (0, 1, 2)
    else:                          # lines = columns, positions = rows
        cv[100, 0, 0] = NAN
        cv[120, 1, 1], cv[125, 1, 1] = INF, -INF
        cv[H - 1, 2, 2] = NAN
        cv[255, 3, 3], cv[256, 3, 3] = NAN, NAN
        cv[40, 4, 40] = NAN         # invalid: x < d
        cv[200, 5, :] = NAN
        rows = (10,)
    return _frozen(cv), rows


def to_right(cl):
    """The right-referenced volume of a left-coordinate one, invalid voxels included: cr[y, x, d] =
    cl[y, (x + d) mod W, d] (the rotation the aggregation of a right volume undoes first)."""
    H, W, D = cl.shape
    cr = np.empty_like(cl)
    for d in range(D):
        cr[:, :, d] = np.roll(cl[:, :, d], -(d % W), axis=1)
    return cr
