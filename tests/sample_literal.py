"""A pure NumPy / Python-int statement of sde_triplet_centres, sde_train_sample_gather's draw and sde_bad_pixels
(include/sde.h).  Philox runs on Python integers, positions on Python floats (IEEE doubles, one rounding per
operation), so nothing here shares code with the kernels or with training.TripletSampler."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Four 32-bit counter words, two key words -> four words."""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def words(seed, step, i, tag):
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return philox4x32_10((i, step & MASK32, step >> 32, tag), (seed & MASK32, seed >> 32))


def unit(x):
    """U in [0, 1): 53 bits of x0, x1, exact in a double."""
    return float((x[0] << 21) | (x[1] >> 11)) * 2.0 ** -53


def centres(disp_l, disp_r, nlayers, zero_is_invalid):
    """-> int32 array of y*W + x, ascending."""
    dl = np.asarray(disp_l, np.float32)
    dr = None if disp_r is None else np.asarray(disp_r, np.float32)
    H, W = dl.shape
    h = nlayers
    out = []
    for y in range(h, H - h):
        for x in range(h, W - h):
            d = float(dl[y, x])
            if not math.isfinite(d) or not d >= 0 or (zero_is_invalid and d == 0):
                continue
            if not d + h <= x:
                continue
            if dr is not None:
                r = float(dr[y, int(x - d)])
                if not math.isfinite(r) or (zero_is_invalid and r == 0) or not abs(r - d) <= 1:
                    continue
            out.append(y * W + x)
    return np.array(out, np.int32)


def draw(scenes, nlayers, seed, step, B, max_rounds=32):
    """scenes: [(disp_l float32 [H][W], centres int32)] in table order.
    -> idx int32 [B][4], scene int32 [B], rounds int [B][2] (rounds used by the positive / the negative draw;
    max_rounds + 1 where the fallback fired)."""
    h = nlayers
    firsts = np.concatenate([[0], np.cumsum([len(c) for _, c in scenes])])
    N = int(firsts[-1])
    assert 1 <= N < 2 ** 31
    idx, scene, rounds = np.zeros((B, 4), np.int32), np.zeros(B, np.int32), np.zeros((B, 2), np.int64)
    for i in range(B):
        g = (words(seed, step, i, 0)[0] * N) >> 32
        s = max(k for k in range(len(scenes)) if firsts[k] <= g)
        assert firsts[s] <= g < firsts[s + 1]
        dl, cs = scenes[s]
        W = dl.shape[1]
        c = int(cs[g - int(firsts[s])])
        y, x = c // W, c % W
        rc = float(x) - float(dl[y, x])

        def inside(p):
            return h <= p < W - h

        pos, used_p = int(rc), max_rounds + 1
        for r in range(max_rounds):
            u = unit(words(seed, step, i, 1 + r))
            t = 1.002 * u
            o = -0.501 + t
            p = int(rc + o)
            if inside(p):
                pos, used_p = p, r + 1
                break
        neg, used_n = (pos + 2 if inside(pos + 2) else pos - 2), max_rounds + 1
        for r in range(max_rounds):
            w = words(seed, step, i, 33 + r)
            t = 4.5 * unit(w)
            dev = 1.5 + t
            n = int(rc - dev) if w[2] & 1 else int(rc + dev)
            if inside(n):
                neg, used_n = n, r + 1
                break
        idx[i], scene[i], rounds[i] = (y, x, pos, neg), s, (used_p, used_n)
    return idx, scene, rounds


def bad_pixels(disp, gt, threshold):
    """-> (evaluated, bad, area uint8 [H][W][3])."""
    disp, gt = np.asarray(disp, np.float32), np.asarray(gt, np.float32)
    H, W = gt.shape
    area = np.zeros((H, W, 3), np.uint8)
    evaluated = bad = 0
    for y in range(H):
        for x in range(W):
            g = float(gt[y, x])
            if g == math.inf or g == 0:
                continue
            evaluated += 1
            if abs(float(disp[y, x]) - g) > threshold:
                bad += 1
                area[y, x, 2] = 255
            else:
                area[y, x, 1] = 255
    return evaluated, bad, area


def right_map(gt):
    """The right-view map of a synthetic.stereo_pair ground truth, as training.synthetic_triplets builds it."""
    H, W = gt.shape
    ys, xs = np.mgrid[0:H, 0:W]
    ok = xs - gt >= 0
    out = np.full((H, W), np.inf)
    out[ys[ok], (xs - gt)[ok]] = gt[ok]
    return out


def handmade_maps():
    """13x40 (left, right) float32 maps for nlayers = 5 (centre rows 5..7, columns 5..34) holding every edge of the
    centre rule; the comments name the centre each entry decides."""
    left = np.full((13, 40), 3.0, np.float32)
    right = np.full((13, 40), 3.0, np.float32)
    left[6, 10], left[6, 11], left[6, 13] = np.inf, np.nan, -2.0
    left[6, 12], right[6, 12] = 0.0, 0.5            # (6,12): d = 0, a centre only without the flag
    left[6, 14] = -0.0                              # like 0
    left[5, 12] = left[5, 11] = right[5, 5] = 7.0   # d + h == x exactly at (5,12); one short at (5,11)
    right[7, 17] = 4.0                              # (7,20): |r - d| == 1 exactly
    right[7, 22] = np.nextafter(np.float32(4.0), np.float32(5.0))   # (7,25): just above 1
    right[7, 27] = np.nextafter(np.float32(2.0), np.float32(1.0))   # (7,30): just above 1, from below
    left[5, 20], right[5, 17] = 2.5, 3.25           # (5,20): trunc(17.5) = 17, |0.75|
    left[5, 22], right[5, 19] = 2.75, 1.5           # (5,22): trunc(19.25) = 19, |1.25|
    left[6, 23], right[6, 22] = 0.75, 0.0           # (6,23): r = 0, a centre only without the flag
    right[6, 27], right[6, 26] = np.nan, np.inf     # (6,30), (6,29)
    left[7, 33] = 30.0                              # d + h > x
    return left, right


def reject_scene():
    """11x23 scene for nlayers = 5 (one centre row, inside columns 5..17), zero_is_invalid off.  Columns 10..12 with
    d = x - 5 have rc == h: half the positive draws and every leftward negative fall outside.  Column 17 = W - h - 1
    with d == 0: every rightward negative falls outside."""
    left = np.full((11, 23), np.inf, np.float32)
    for x in (10, 11, 12):
        left[5, x] = x - 5
    left[5, 17] = 0.0
    rng = np.random.default_rng(23)
    return rng.integers(0, 256, (2, 11, 23)).astype(np.uint8), left
