"""NumPy restatement of the local matcher's definitions (include/sde.h, "Local matcher"): the expected values of
tests/test_local_host.py and tests/test_gpu_local.py.

Written from the definitions, in integer arithmetic.  Every definition has a loop form (one voxel or pixel at a
time, for tiny shapes) and a pixel-vectorised form for the larger cases; test_local_host.py asserts the two equal
on (9, 23, D = 8).  Volumes are float32 [H][W][D], images uint8 [H][W], a pixel outside the image reads as 0.
"""
import numpy as np

INVALID = np.float32(999999999999)      # 999999995904, bits 0x5368d4a5
MAX_RADIUS = 32


def px(img, r, c):
    H, W = img.shape
    return int(img[r, c]) if 0 <= r < H and 0 <= c < W else 0


# ---------------------------------------------------------------------------------------------------------
# loop forms
# ---------------------------------------------------------------------------------------------------------
def census_loop(img):
    H, W = img.shape
    out = np.zeros((H, W), np.uint32)
    for y in range(H):
        for x in range(W):
            bits = []
            for r in range(y - 3, y):
                for c in range(x - 4, x):
                    bits.append(px(img, r, c) > px(img, 2 * y - r, 2 * x - c))
            for r in range(y - 3, y):
                bits.append(px(img, r, x) > px(img, 2 * y - r, x))
            for c in range(x - 4, x):
                bits.append(px(img, y, c) > px(img, y, 2 * x - c))
            assert len(bits) == 19
            w = 0
            for b in bits:                   # most-significant bit first
                w = (w << 1) | int(b)
            out[y, x] = w
    return out


def rank_loop(img):
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            n = 0
            for r in range(y - 3, y + 4):
                for c in range(x - 3, x + 4):
                    n += px(img, y, x) >= px(img, r, c)
            out[y, x] = n
    return out


def popcount(a):
    a = np.asarray(a, np.uint32)
    n = np.zeros(a.shape, np.int64)
    for b in range(32):
        n += (a >> np.uint32(b)) & np.uint32(1)
    return n


def census_cost_loop(cl, cr, D, invalid=INVALID):
    H, W = cl.shape
    L = np.full((H, W, D), invalid, np.float32)
    R = np.full((H, W, D), invalid, np.float32)
    for y in range(H):
        for x in range(W):
            for d in range(D):
                if x - d >= 0:
                    L[y, x, d] = bin(int(cl[y, x]) ^ int(cr[y, x - d])).count("1")
                if x + d < W:
                    R[y, x, d] = bin(int(cl[y, x + d]) ^ int(cr[y, x])).count("1")
    return L, R


def ad_columns(x, W, D, k):
    if x < D + k:
        return x, x + k
    if x + k < W - k:
        return x - k, x + k
    return x - k, x


def ad_sums_loop(il, ir, D, k):
    """The exact integer window sums (int64 [H][W][D]; -1 where x - d < 0)."""
    H, W = il.shape
    assert W >= D + 2 * k and 0 <= k <= MAX_RADIUS
    out = np.full((H, W, D), -1, np.int64)
    for y in range(H):
        for x in range(W):
            c0, c1 = ad_columns(x, W, D, k)
            for d in range(D):
                if x - d < 0:
                    continue
                s = 0
                for r in range(max(y - k, 0), min(y + k, H - 1) + 1):
                    for c in range(c0, c1 + 1):
                        df = int(il[r, c]) - int(ir[r, c - d])
                        s += abs(df) + df * df
                out[y, x, d] = s
    return out


def wta_loop(vol):
    """best = c(0); for d = 1..D-1 take d if best > c(d).  Returns (disp f32, min f32)."""
    H, W, D = vol.shape
    disp = np.zeros((H, W), np.float32)
    mn = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            best, bd = vol[y, x, 0], 0
            for d in range(1, D):
                if best > vol[y, x, d]:
                    best, bd = vol[y, x, d], d
            disp[y, x], mn[y, x] = bd, best
    return disp, mn


# ---------------------------------------------------------------------------------------------------------
# pixel-vectorised forms
# ---------------------------------------------------------------------------------------------------------
def _shift(img, dr, dc):
    """out[y, x] = I(y + dr, x + dc), 0 outside the image."""
    H, W = img.shape
    out = np.zeros((H, W), np.int64)
    ys, xs = np.arange(H) + dr, np.arange(W) + dc
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    if oky.any() and okx.any():
        out[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
    return out


def census(img):
    w = np.zeros(img.shape, np.uint32)

    def push(a, b):
        nonlocal w
        w = (w << np.uint32(1)) | (a > b).astype(np.uint32)

    for dr in range(-3, 0):
        for dc in range(-4, 0):
            push(_shift(img, dr, dc), _shift(img, -dr, -dc))
    for dr in range(-3, 0):
        push(_shift(img, dr, 0), _shift(img, -dr, 0))
    for dc in range(-4, 0):
        push(_shift(img, 0, dc), _shift(img, 0, -dc))
    return w


def rank(img):
    centre = img.astype(np.int64)
    n = np.zeros(img.shape, np.int64)
    for dr in range(-3, 4):
        for dc in range(-3, 4):
            n += centre >= _shift(img, dr, dc)
    return n.astype(np.uint8)


def census_cost(cl, cr, D, invalid=INVALID):
    H, W = cl.shape
    L = np.full((H, W, D), invalid, np.float32)
    R = np.full((H, W, D), invalid, np.float32)
    for d in range(min(D, W)):
        h = popcount(cl[:, d:] ^ cr[:, :W - d]).astype(np.float32)     # pairs (x, x - d), x = d..W-1
        L[:, d:, d] = h
        R[:, :W - d, d] = h
    return L, R


def ad_sums(il, ir, D, k):
    """ad_sums_loop by box sums: per d, e over the image, rows by a clipped running window, columns by zone."""
    H, W = il.shape
    assert W >= D + 2 * k and 0 <= k <= MAX_RADIUS
    out = np.full((H, W, D), -1, np.int64)
    a = il.astype(np.int64)
    b = ir.astype(np.int64)
    xs = np.arange(W)
    c0 = np.where(xs < D + k, xs, xs - k)
    c1 = np.where(xs < D + k, xs + k, np.where(xs + k < W - k, xs + k, xs))
    for d in range(D):
        e = np.zeros((H, W), np.int64)                 # e[r, c] for c >= d
        df = a[:, d:] - b[:, :W - d]
        e[:, d:] = np.abs(df) + df * df
        rows = np.zeros((H + 1, W), np.int64)
        rows[1:] = np.cumsum(e, axis=0)
        y = np.arange(H)
        v = rows[np.minimum(y + k, H - 1) + 1] - rows[np.maximum(y - k, 0)]      # vertical sums [H][W]
        cols = np.zeros((H, W + 1), np.int64)
        cols[:, 1:] = np.cumsum(v, axis=1)
        s = cols[:, c1 + 1] - cols[:, c0]
        ok = xs >= d
        out[:, ok, d] = s[:, ok]
    return out


def ad_cost(il, ir, D, k, invalid=INVALID):
    s = ad_sums(il, ir, D, k)
    return np.where(s >= 0, s.astype(np.float32), np.float32(invalid)).astype(np.float32)


def ad_cost_loop(il, ir, D, k, invalid=INVALID):
    s = ad_sums_loop(il, ir, D, k)
    return np.where(s >= 0, s.astype(np.float32), np.float32(invalid)).astype(np.float32)


def wta(vol):
    """First strict minimum: np.argmin returns the first occurrence of the minimum."""
    d = np.argmin(vol, axis=2)
    return d.astype(np.float32), np.take_along_axis(vol, d[..., None], axis=2)[..., 0].astype(np.float32)


def tie_share(vol):
    """Share of pixels whose minimum is attained by more than one disparity."""
    return float(((vol == vol.min(axis=2, keepdims=True)).sum(axis=2) > 1).mean())
