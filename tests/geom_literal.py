"""Plain NumPy / Python-integer restatements of the three definitions of include/sde_geom.h, written from their
text and not from the kernels: the sampling map (float64, every operation on its own), the integer bilinear remap
(one pixel at a time) and the reprojection.  tests/test_geom_host.py checks them against hand-made pictures; the
GPU tests compare the kernels with them by bytes.
"""
import numpy as np

NO_SAMPLE = -2147483648


def rectify_map(cal, H, W):
    """cal: 26 float64 = K (9), dist k1 k2 p1 p2 k3 k4 k5 k6 (8), Minv (9) -> int32 [H][W][2]."""
    cal = np.asarray(cal, np.float64).reshape(26)
    K, (k1, k2, p1, p2, k3, k4, k5, k6), M = cal[:9], cal[9:17], cal[17:]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    one, two = np.float64(1.0), np.float64(2.0)
    with np.errstate(all="ignore"):
        X = (M[0] * u + M[1] * v) + M[2]
        Y = (M[3] * u + M[4] * v) + M[5]
        Wd = (M[6] * u + M[7] * v) + M[8]
        x = X / Wd
        y = Y / Wd
        xx = x * x
        yy = y * y
        xy = x * y
        r2 = xx + yy
        kr = (one + ((k3 * r2 + k2) * r2 + k1) * r2) / (one + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + (two * p1) * xy) + p2 * (r2 + two * xx)
        yd = (y * kr + p1 * (r2 + two * yy)) + (two * p2) * xy
        us = (K[0] * xd + K[1] * yd) + K[2]
        vs = K[4] * yd + K[5]
        a = np.rint(us * np.float64(32.0))
        b = np.rint(vs * np.float64(32.0))
        ok = np.isfinite(a) & np.isfinite(b) & (np.abs(a) < 2.0 ** 30) & (np.abs(b) < 2.0 ** 30)
    out = np.full((H, W, 2), NO_SAMPLE, np.int32)
    out[ok, 0] = a[ok].astype(np.int64)
    out[ok, 1] = b[ok].astype(np.int64)
    return out


def remap_pixel(src, a, b):
    """One map entry on one u8 [Hs][Ws] source -> (dst, valid), in Python integers."""
    Hs, Ws = src.shape
    a, b = int(a), int(b)
    if a == NO_SAMPLE and b == NO_SAMPLE:
        return 0, 0
    x0, fx, y0, fy = a >> 5, a & 31, b >> 5, b & 31
    total, valid = 0, 1
    for w, y, x in (((32 - fx) * (32 - fy), y0, x0), (fx * (32 - fy), y0, x0 + 1), ((32 - fx) * fy, y0 + 1, x0),
                    (fx * fy, y0 + 1, x0 + 1)):
        if w == 0:
            continue                      # not read
        if 0 <= y < Hs and 0 <= x < Ws:
            total += w * int(src[y, x])
        else:
            valid = 0                     # a read tap outside contributes 0
    return (total + 512) >> 10, valid


def remap_u8(src, maps):
    """src u8 [N][Hs][Ws], maps int32 [N][H][W][2] -> (dst u8 [N][H][W], valid u8 [N][H][W])."""
    N, H, W, _ = maps.shape
    dst = np.zeros((N, H, W), np.uint8)
    valid = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        for y in range(H):
            for x in range(W):
                d, ok = remap_pixel(src[i], maps[i, y, x, 0], maps[i, y, x, 1])
                assert 0 <= d <= 255
                dst[i, y, x], valid[i, y, x] = d, ok
    return dst, valid


def reproject(disp, Q, min_disp=0.0):
    """disp float32 [H][W], Q 4x4 float64 -> (depth float32 [H][W], xyz float32 [H][W][3])."""
    disp = np.asarray(disp, np.float32)
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    H, W = disp.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        ok = np.isfinite(disp) & (disp > np.float32(min_disp))
        d = disp.astype(np.float64)
        v = [((Q[r, 0] * x + Q[r, 1] * y) + Q[r, 2] * d) + Q[r, 3] for r in range(4)]
        xyz = np.stack([(v[r] / v[3]).astype(np.float32) for r in range(3)], axis=-1)
    xyz[~ok] = 0.0
    return np.ascontiguousarray(xyz[..., 2]), xyz
