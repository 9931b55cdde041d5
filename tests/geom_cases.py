"""Inputs shared by test_geom_host.py and test_gpu_geom.py: calibrations, `cal` vectors and hand-built maps.  Every
case is built from a fixed seed and returned read-only where it is cached."""
import functools

import numpy as np

NO_SAMPLE = -2147483648
LIM = (1 << 30) - 1


def plain_calibration(H, W, shift=0):
    """K = diag(64, 64, 1) with the integer centre (W/2, H/2), no distortion, R = I: with shift = 0 the rectified
    pair is the raw pair.  shift moves the RECTIFIED principal point (P1, P2, Q) by that many columns, so a
    rectified pixel u samples the raw column u - shift."""
    from scenedepthestimation_amd.rectify import StereoCalibration
    cx, cy, f, tx = float(W // 2), float(H // 2), 64.0, -0.1
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    P1 = np.array([[f, 0, cx + shift, 0], [0, f, cy, 0], [0, 0, 1.0, 0]])
    P2 = P1.copy()
    P2[0, 3] = f * tx
    Q = np.array([[1.0, 0, 0, -(cx + shift)], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, -1 / tx, 0]])
    extra = dict(R1=np.eye(3), R2=np.eye(3), P1=P1, P2=P2, Q=Q) if shift else {}
    return StereoCalibration(K, np.zeros(5), K, np.zeros(5), np.eye(3), [tx, 0, 0], (H, W), **extra)


def shifted(img, n):
    """img moved n columns to the right, zeros on the left."""
    out = np.zeros_like(img)
    out[:, n:] = img[:, :img.shape[1] - n]
    return out


def distorted_cal():
    """A 41 x 70 camera with radial, tangential and rational terms and a 5 degree rectifying rotation."""
    from scenedepthestimation_amd.rectify import camera_cal, rodrigues
    K = np.array([[61.5, 0.3, 34.25], [0, 60.75, 20.5], [0, 0, 1.0]])
    D = [-0.4, 0.15, 0.002, -0.003, 0.01, 0.02]
    P = np.array([[58.0, 0, 35.0, 0], [0, 58.0, 20.0, 0], [0, 0, 1.0, 0]])
    return camera_cal(K, D, rodrigues(np.deg2rad(5.0) * np.array([0.6, 0.8, 0.0])), P)


def zero_crossing_cal():
    """Minv's third row makes Wd = u/8 - 2 cross zero at u = 16: a column of infinities (and one NaN where X is
    zero too), with both signs of huge coordinates beside it."""
    cal = distorted_cal().copy()
    cal[17:] = [1 / 58.0, 0, -16 / 58.0, 0, 1 / 58.0, -20 / 58.0, 0.125, 0, -2.0]
    return cal


def huge_cal():
    """A focal length of 1e8: columns away from the centre land past 2^30 / 32 pixels, the ones near it do not."""
    cal = distorted_cal().copy()
    cal[9:17] = 0
    cal[0] = 1e8
    return cal


# (a, b) entries for a source of Hs x Ws, in the order of the remap test's list of cases
def edge_entries(Hs, Ws):
    X, Y = 32 * (Ws - 1), 32 * (Hs - 1)
    e = [(32 * 7, 32 * 5), (32 * 7 + 31, 32 * 5), (32 * 7, 32 * 5 + 31), (32 * 7 + 31, 32 * 5 + 31),   # fractions 0 / 31
         (-1, 32 * 4 + 9), (-32, 32 * 4), (X, 32 * 4), (X + 1, 32 * 4),                                 # x edges
         (32 * 6 + 9, -1), (32 * 6, -32), (32 * 6, Y), (32 * 6, Y + 1),                                 # y edges
         (NO_SAMPLE, NO_SAMPLE), (LIM, -LIM), (-LIM, LIM),
         (-1, -1), (X + 1, Y + 1), (X, Y), (-32, -32), (NO_SAMPLE, 32), (32, NO_SAMPLE), (LIM, LIM), (2 ** 31 - 1, 5),
         (X + 31, Y + 31), (X + 32, 0), (0, Y + 32), (0, 0)]
    return np.array(e, np.int64)


@functools.lru_cache(maxsize=None)
def remap_case(nimg, H, W, Hs=37, Ws=53, seed=0):
    """(src u8 [nimg][Hs][Ws], maps int32 [nimg][H][W][2]): each image has its own random source and its own map --
    the edge entries first (cycled, started at another place per image), then random coordinates from two pixels
    outside the source to two pixels outside on the other side, any fraction."""
    rng = np.random.default_rng(1000 * seed + 97 * nimg + H * W)
    src = rng.integers(0, 256, (nimg, Hs, Ws), dtype=np.uint8)
    edges = edge_entries(Hs, Ws)
    maps = np.empty((nimg, H * W, 2), np.int64)
    maps[..., 0] = rng.integers(-64, 32 * (Ws + 2), (nimg, H * W))
    maps[..., 1] = rng.integers(-64, 32 * (Hs + 2), (nimg, H * W))
    for i in range(nimg):
        n = min(H * W, 2 * len(edges))
        maps[i, :n] = edges[(np.arange(n) + 5 * i) % len(edges)]
    maps = maps.astype(np.int32).reshape(nimg, H, W, 2)
    src.setflags(write=False)
    maps.setflags(write=False)
    return src, maps


def reproject_disp(min_disp):
    """9 x 13 disparities: -1 (no winner), 0, NaN, +-inf, the 2.625 of the parabola step, a value equal to min_disp,
    the float32 just above and just below it, and ordinary values around them."""
    rng = np.random.default_rng(5)
    d = rng.uniform(0.25, 14.0, (9, 13)).astype(np.float32)
    md = np.float32(min_disp)
    special = [-1.0, 0.0, np.nan, np.inf, -np.inf, 2.625, md, np.nextafter(md, np.float32(np.inf)),
               np.nextafter(md, np.float32(-np.inf)), -0.0]
    d.reshape(-1)[3:3 + 4 * len(special):4] = np.array(special, np.float32)
    return d


def dense_Q():
    """A Q whose 16 entries are all non-zero (no structure to lean on)."""
    return np.array([[1.0, 0.01, -0.02, -47.5], [0.015, 0.99, 0.03, -31.25], [0.002, -0.001, 0.004, 63.5],
                     [0.0003, 0.0002, 9.75, 0.5]])
