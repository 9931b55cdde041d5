"""Case tables of the sub-pixel and bilateral tests, shared by test_refine_host.py (the literal itself, CPU) and
test_gpu_refine.py (kernels against the literal).  Inputs are built once per case and handed out read-only; that a
case is not vacuous (enough pixels refined, enough taps on both sides of the threshold) is asserted in
test_refine_host.py.
"""
import functools

import numpy as np

NAN, INF = np.float32(np.nan), np.float32(np.inf)
ONE = np.float32(1.0)
ULP = np.float32(2.0 ** -23)            # ulp(1.0f)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ----------------------------------------------------------------------------
# hand-computed pictures: one pixel each, (costs over d, the refined disparity under rule 'inf')
# ----------------------------------------------------------------------------
def _near_tie(k):
    """[2, c + k u, c, c, 3] at c = 1, u = ulp(c): the winner is d = 2 (first minimum), num = -k u and
    s = float32(2 + k u), which lands on the even neighbour among the multiples of 2u."""
    return [2.0, float(ONE + np.float32(k) * ULP), 1.0, 1.0, 3.0]


HAND = (
    ([3.0, 1.0, 2.0], 1.0 - (2.0 - 3.0) / (2.0 * (5.0 - 2.0))),    # 1.1666...
    (_near_tie(2), 2.5),            # s = 2 + 2u, den = 4u, 2 + 2u/4u
    (_near_tie(3), 2.375),          # s = 2 + 4u (tie to even), den = 8u, 2 + 3u/8u
    (_near_tie(5), 2.625),          # s = 2 + 4u (tie to even), den = 8u, 2 + 5u/8u: past 0.5, no clamp
    (_near_tie(1), 2.0),            # s = 2 (tie to even), den = 0: the integer stays
    ([1.0, 1.0, 1.0], 0.0),         # flat: the first minimum is d = 0
    ([1.0, 2.0, 3.0], 0.0),         # winner at 0
    ([3.0, 2.0, 1.0], 2.0),         # winner at D - 1
    ([5.0], 0.0),                   # D = 1
    ([5.0, 4.0], 1.0),              # D = 2
    ([float("nan"), 1.0, 2.0], 1.0),
    ([2.0, 1.0, float("nan")], 1.0),
    ([float("inf"), 1.0, 2.0], 1.0),
    ([2.0, 1.0, float("inf")], 1.0),
    ([3.0, float("-inf"), 2.0], 1.0),           # the winner's own cost is not finite
    ([float("inf")] * 3, -1.0),                 # no winner under 'inf' passes through
    ([float("nan")] * 4, -1.0),
    ([3e38, -3e38, 3e38], 1.0),                 # s overflows to +inf: den = +inf, the offset is 0
    ([3.0, 1.0, 1.5, 0.5, 0.75], 3.0 - (0.75 - 1.5) / (2.0 * (2.25 - 1.0))),   # 3.3
)


@functools.lru_cache(maxsize=None)
def hand_volume():
    """The HAND pictures of one length as [1, n, D] HWD volumes: D -> (volume, wanted float32 row)."""
    out = {}
    for D in sorted({len(c) for c, _ in HAND}):
        rows = [(c, w) for c, w in HAND if len(c) == D]
        vol = np.array([[c for c, _ in rows]], dtype=np.float32)
        out[D] = _frozen(vol, np.array([[w for _, w in rows]], dtype=np.float32))
    return out


# ----------------------------------------------------------------------------
# stored-volume WTA + refinement
# ----------------------------------------------------------------------------
SUB_D = (1, 2, 3, 5, 40, 70, 130)           # below, at and above a wave's 64 lanes and a float4 multiple
SUB_PIXELS = ((1, 1), (3, 67), (5, 130))
SUB_KINDS = ("random", "ties", "nonfinite", "fill")
SUB_RANDOM = ("random",)                    # the kind test_refine_host.py holds to "at least half refined" (D >= 3)


@functools.lru_cache(maxsize=None)
def sub_case(H, W, D, kind):
    """An [H, W, D] volume.
    random     uniform costs with a well two deep at an interior d of nine pixels in ten (pixel (0, 0) always)
    ties       small integers: ties everywhere, flat minima (den = 0) and plateaus next to the winner
    nonfinite  `random` with NaN, +inf and -inf sprinkled, NaN at d = 0 of some pixels, an all-NaN pixel
    fill       `random` in [-1, 0] with the HWD cost volume's 1.0 fill at d > x"""
    rng = np.random.default_rng((H * 256 + W) * 1000 + D * 8 + SUB_KINDS.index(kind))
    if kind == "ties":
        return _frozen(rng.integers(0, 3, (H, W, D)).astype(np.float32))
    vol = rng.random((H, W, D), dtype=np.float32)
    if D >= 3:
        t = rng.integers(1, D - 1, (H, W))
        well = rng.random((H, W)) < 0.9
        well[0, 0] = True
        ys, xs = np.nonzero(well)
        vol[ys, xs, t[ys, xs]] -= np.float32(2.0)
    if kind == "nonfinite":
        r = rng.random((H, W, D))
        vol[r < 0.04] = NAN
        vol[(r >= 0.04) & (r < 0.08)] = INF
        vol[(r >= 0.08) & (r < 0.10)] = -INF
        vol[rng.random((H, W)) < 0.2, 0] = NAN
        vol[H - 1, W - 1, :] = NAN
    elif kind == "fill":
        vol = (vol / np.float32(4.0) - np.float32(0.5)).astype(np.float32)        # within [-1, 0]
        d = np.arange(D)[None, None, :]
        x = np.arange(W)[None, :, None]
        vol = np.where(d > x, ONE, vol).astype(np.float32)
    return _frozen(np.ascontiguousarray(vol))


def as_layout(vol_hwd, layout):
    return vol_hwd if layout == "HWD" else np.ascontiguousarray(np.moveaxis(vol_hwd, 2, 0))


# ----------------------------------------------------------------------------
# the quadratic volume: c = s (d - t)^2, t uniform in [1, D - 2]
# ----------------------------------------------------------------------------
QUAD_SHAPE, QUAD_D, QUAD_SCALES, QUAD_BOUND = (8, 64), 32, (1.0, 0.01), 1e-5


@functools.lru_cache(maxsize=None)
def quad_case(scale):
    rng = np.random.default_rng(int(scale * 1000) + 17)
    t = rng.uniform(1.0, QUAD_D - 2.0, QUAD_SHAPE)
    d = np.arange(QUAD_D, dtype=np.float64)[None, None, :]
    vol = (scale * (d - t[:, :, None]) ** 2).astype(np.float32)
    return _frozen(vol, t)


# ----------------------------------------------------------------------------
# volume-free refinement (sde_cv_subpixel)
# ----------------------------------------------------------------------------
CV_H, CV_D = 3, 12
CV_CHANNELS = (64, 24)
CV_WIDTHS = (5, 70)
CV_RANGES = ((0, CV_D), (3, CV_D - 2))


def cv_winners_refined(W, d0, d1):
    """Whether the WTA map of this case must have at least half of its pixels refined.  With W = 5 and the shard
    [3, 10) only three voxels of a row are not the -0.0 fill, so the winners sit on d0: that case is there for the
    fill and for D > W: three -0.0 costs give den = 0, so nearly every pixel must come back as it went in."""
    return not (W == 5 and d0 > 0)


@functools.lru_cache(maxsize=None)
def cv_features(W, C, d0, d1):
    """Smooth unit features with a planted fractional shift t per row: fl[y, x] = g(x), fr[y, x'] = g(x' + t), so
    cost(x, d) is smooth in d with its minimum next to t in both views.  t lies inside (d0 + 1, d1 - 2), within
    the row for W = 5."""
    rng = np.random.default_rng(W * 100 + C + d0)
    lo, hi = (1.2, 1.8) if W == 5 else (d0 + 1.3, d1 - 2.3)
    t = rng.uniform(lo, hi, CV_H)
    om = rng.uniform(0.15, 0.6, C)
    ph = rng.uniform(0, 2 * np.pi, C)
    x = np.arange(W, dtype=np.float64)

    def g(pos):
        f = np.cos(pos[..., None] * om + ph) + 0.02 * rng.standard_normal(pos.shape + (C,))
        return (f / np.sqrt((f ** 2).sum(-1, keepdims=True))).astype(np.float32)
    fl = g(np.broadcast_to(x, (CV_H, W)))
    fr = g(x[None, :] + t[:, None])
    return _frozen(np.ascontiguousarray(fl), np.ascontiguousarray(fr))


@functools.lru_cache(maxsize=None)
def cv_probe_map(W, d0, d1):
    """A map that is not a WTA result: integers from d0 - 2 to d1 + 1 (in and out of range, any of them may sit on
    a maximum, where den <= 0), and in fixed places what must come back bit for bit: fractions, -1, NaN, -0.5,
    +-inf, 1e9, a NaN with a payload."""
    rng = np.random.default_rng(W * 31 + d0)
    m = rng.integers(d0 - 2, d1 + 2, (CV_H, W)).astype(np.float32)
    odd = np.array([0.5, -1.0, np.nan, -0.5, np.inf, -np.inf, 1e9, d0 + 1.25, d1 - 0.5, float(d1), float(d0) - 1.0],
                   np.float32)
    flat = m.reshape(-1)
    pos = rng.permutation(flat.size)[: min(len(odd), flat.size // 2)]
    flat[pos] = odd[: len(pos)]
    bits = flat.view(np.uint32)
    bits[pos[2 % len(pos)]] = 0xFFC12345          # a negative quiet NaN with a payload
    return _frozen(m)


# ----------------------------------------------------------------------------
# 9x9 bilateral filter
# ----------------------------------------------------------------------------
BIL_SHAPES = ((1, 1), (7, 9), (16, 16), (17, 33), (35, 50))
BIL_KINDS = ("plain", "nonfinite")
BIL_LEVELS = np.array([0, 3, 4, 5, 9, 250, 255], np.uint8)     # a on both sides of 5; near 0 at the zero padding


@functools.lru_cache(maxsize=None)
def bil_case(H, W, kind):
    """Intensities from BIL_LEVELS in patches of a few pixels (so that windows hold accepted and rejected taps),
    disparities with fractions; `nonfinite` adds NaN and +inf entries (only +inf: inf - inf would make a NaN whose
    sign depends on the machine, and the comparison is by bytes)."""
    rng = np.random.default_rng(H * 1009 + W * 7 + BIL_KINDS.index(kind))
    coarse = rng.choice(BIL_LEVELS, (-(-H // 3), -(-W // 3)))
    img = np.repeat(np.repeat(coarse, 3, axis=0), 3, axis=1)[:H, :W].copy()
    noise = rng.random((H, W)) < 0.3
    img[noise] = rng.choice(BIL_LEVELS, int(noise.sum()))
    src = (rng.integers(0, 60, (H, W)).astype(np.float32) + rng.random((H, W), dtype=np.float32)).astype(np.float32)
    if kind == "nonfinite":
        r = rng.random((H, W))
        src[r < 0.02] = NAN
        src[r > 0.98] = INF
        src[H // 2, W // 2] = NAN
        src[0, W - 1] = INF
    return _frozen(np.ascontiguousarray(img), src)


# ----------------------------------------------------------------------------
# composition through StereoMatcher
# ----------------------------------------------------------------------------
COMP_SHAPE, COMP_D, COMP_SEED = (24, 48), 16, 11
