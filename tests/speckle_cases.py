"""Inputs of the speckle filter's tests, built deterministically.  Every map is at most 150 x 199, so the literal
restatement takes well under a second per case, and the large ones hold seams of any tile size up to 64 inside the
image (64- and 128-aligned rows and columns exist in 150 x 199; 70 x 131 has one 64-aligned seam each way).

A case is a dict: name, disp (float32 [H,W]), max_size, max_diff, fill, and `full`: True where the literal's result
must show removed and kept pixels, a kept region spanning more than 64 pixels each way, and invalid pixels
(test_speckle_host.py asserts it)."""
from __future__ import annotations

import numpy as np

F = np.float32
NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(np.float32)[0]   # a quiet NaN that is not the default one
NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
BIG, SMALL = (150, 199), (70, 131)


def canvas(shape, value=-1.0):
    return np.full(shape, value, np.float32)


def case(name, disp, max_size, max_diff=1.0, fill=-1.0, full=False):
    return dict(name=name, disp=np.ascontiguousarray(disp, np.float32), max_size=int(max_size),
                max_diff=float(max_diff), fill=float(fill), full=bool(full))


def spiral_path(H, W):
    """Cells of a one-pixel-wide spiral from (0, 0) inwards with one-pixel gaps between its turns, in order."""
    g = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = True
    path = [(0, 0)]

    def free(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and not g[yy, xx]

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            # the next cell may touch the path nowhere but at the cell it comes from
            around = [(ny + a, nx + b) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1)) if (ny + a, nx + b) != (y, x)]
            if free(ny, nx) and all(free(*c) or not (0 <= c[0] < H and 0 <= c[1] < W) for c in around):
                break
            dy, dx = dx, -dy          # turn right
        else:
            return path
        y, x = ny, nx
        g[y, x] = True
        path.append((y, x))


def serpentine_path(H, W):
    """Every even row in full, joined alternately at the right and the left end through the odd rows."""
    path = []
    for k, y in enumerate(range(0, H, 2)):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, W - 1 if k % 2 == 0 else 0))
    return path


def draw(disp, path, value):
    for y, x in path:
        disp[y, x] = value
    return disp


def speckle_dots(disp, rng, n, value, only_on=-1.0):
    """n single pixels of `value` on cells that hold `only_on` (a value far from the neighbours': regions of 1)."""
    ys, xs = np.nonzero(disp == F(only_on))
    pick = rng.permutation(len(ys))[:n]
    disp[ys[pick], xs[pick]] = value
    return disp


def spiral_case():
    d = draw(canvas(BIG), spiral_path(*BIG), 5.0)
    speckle_dots(d, np.random.RandomState(1), 40, 50.0)
    return case("spiral", d, 3, full=True)


def serpentine_case():
    d = draw(canvas(BIG), serpentine_path(*BIG), 5.0)
    speckle_dots(d, np.random.RandomState(2), 40, 50.0)
    return case("serpentine", d, 2, full=True)


def comb_rows_case():
    """Teeth down every even column, joined only by a spine along row 16 and one along row 64, the first rows of a
    16- and of a 64-aligned tile: every tooth is a component of its own in every tile it crosses."""
    d = canvas(BIG)
    d[:, 0::2] = 5.0
    d[16, :] = 5.0
    d[64, :] = 5.0
    d[100, :] = -1.0          # cuts the teeth: below it they hang together through nothing
    d[101:, 0::2] = 6.5       # and are regions of their own, 49 pixels each
    speckle_dots(d, np.random.RandomState(3), 30, 50.0)
    return case("comb_rows", d, 49, full=True)


def comb_cols_case():
    """Teeth along every even row, joined only by a spine down column 63, the last of a 64-aligned tile, and one
    down column 128."""
    d = canvas(BIG)
    d[0::2, :] = 7.25
    d[:, 63] = 7.25
    d[:, 128] = 7.25
    d[:, 180] = NAN_PAYLOAD
    d[1::2, 181:] = np.inf    # the teeth right of the NaN column: 18 pixels each
    speckle_dots(d, np.random.RandomState(4), 30, 50.0)
    return case("comb_cols", d, 18, full=True)


def u_case():
    """Two arms in the same 16-, 32- and 64-aligned tile (rows and columns 64..79), joined only through row 140."""
    d = canvas(BIG)
    d[66:141, 66] = 9.0
    d[66:141, 70] = 9.0
    d[140, 66:71] = 9.0
    d[66:141, 74] = 9.0       # a third arm that stays alone: 75 pixels
    d[10, 10:120] = 9.0       # and a bar of 110 that is kept
    d[30:140, 150] = 9.0
    d[30, 60:151] = 9.0       # an L spanning more than 64 both ways
    return case("u_through_neighbour", d, 100, full=True)


def rings_case():
    """Nested rectangular rings, alternately 5 and 20 (every pixel valid, neighbouring rings not linked)."""
    H, W = SMALL
    d = canvas(SMALL, 5.0)
    for k in range(0, min(H, W) // 2 + 1):
        d[k:H - k, k:W - k] = 5.0 if k % 2 == 0 else 20.0
    d[35, 3] = NAN_PAYLOAD    # opens ring 3 without cutting it in two
    return case("rings", d, 300, full=True)


def constant_cases():
    H, W = SMALL
    d = canvas(SMALL, 3.0)
    return [case("constant_kept", d, H * W - 1), case("constant_gone", d, H * W, fill=np.nan)]


def checkerboard_cases():
    H, W = SMALL
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.where((yy + xx) % 2 == 0, F(2.0), F(5.0))
    return [case("checkerboard_gone", d, 1), case("checkerboard_kept", d, 0)]


def blob_case():
    """Blobs of exactly max_size (12) and max_size + 1 pixels on the corner where four 64-aligned tiles meet and at
    the image border, on a background they are not linked to."""
    H, W = BIG
    d = canvas(BIG, 30.0)
    d[63:66, 62:66] = 5.0                    # 12, over the corner (64, 64)
    d[63:66, 126:130] = 5.0
    d[66, 126] = 5.0                         # 13, over the corner (64, 128)
    d[126:129, 62:66] = 5.5
    d[129, 65] = 5.5                         # 13, over the corner (128, 64)
    d[127:130, 126:130] = 5.5                # 12, over the corner (128, 128)
    d[0:3, 0:4] = 5.0                        # 12, top left
    d[H - 3:, W - 4:] = 5.0
    d[H - 4, W - 1] = 5.0                    # 13, bottom right
    d[0:4, W - 3:] = 6.0                     # 12, top right
    d[H - 1, 0:13] = 6.0                     # 13, bottom left, one row
    d[20, 20] = np.nan
    d[90, 150] = -1.0
    return case("blobs_at_corners", d, 12, full=True)


def threshold_case():
    """Neighbours differing by exactly max_diff (linked) and by the next float32 above it (not linked)."""
    d = canvas((5, 67))
    up = np.nextafter(F(9.0), F(np.inf))
    d[0, 0:2] = (8.0, 9.0)                   # linked: 2
    d[0, 3:5] = (8.0, up)                    # not: 1 + 1
    d[0, 6:9] = (8.0, 9.0, 10.0)             # a ramp of exact steps: 3
    d[2, 0], d[3, 0] = 9.0, 8.0              # vertical, linked
    d[2, 3], d[3, 3] = up, 8.0               # vertical, not
    d[2, 60:67] = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0)      # over column 64
    d[4, 10:13] = (16777216.0, 16777217.0, 16777218.0)      # 2^24 + 1 rounds to 2^24: 0 and 2 apart
    return case("threshold", d, 2)


def threshold_tenth_case():
    """max_diff = 0.1, which float32 does not hold: the comparison is against float32(0.1)."""
    d = canvas((3, 40))
    vals = np.arange(0, 20, dtype=np.float32) * F(0.1)     # steps of about 0.1, rounded each its own way
    d[1, :20] = vals
    d[1, 21:40] = np.arange(19, dtype=np.float32) * F(0.05) + F(0.3)
    return case("threshold_tenth", d, 3, max_diff=0.1)


def ramp_cases():
    row = (np.arange(199, dtype=np.float32) * F(0.75)).reshape(1, 199)
    col = (np.arange(150, dtype=np.float32) * F(0.75)).reshape(150, 1).copy()
    col[40, 0] = -1.0
    col[41:50, 0] += F(0.375)
    col[50, 0] = np.nan
    col[120, 0] = -np.inf
    return [case("ramp_1xW", row, 100), case("ramp_1xW_gone", row, 199, fill=7.0),
            case("ramp_Hx1", col, 40)]


def invalid_kinds_case():
    """Every kind of invalid pixel as a separator between regions of 4.0 and inside them; -0.0 is valid.  Columns
    0..99 are one region; column 100 separates it, with every kind in turn, from strips of 98 columns that rows of
    one kind each separate from one another."""
    H, W = BIG
    d = canvas(BIG, 4.0)
    kinds = [-1.0, -3.5, NAN_PAYLOAD, np.inf, -np.inf, NEG_NAN, -1e-30]
    rng = np.random.RandomState(5)
    for v in kinds:
        d[rng.randint(0, H, 20), rng.randint(0, W, 20)] = v     # holes inside the regions
    for y in range(H):
        d[y, 100] = kinds[y % len(kinds)]
    for y, v in zip((20, 45, 70, 95, 120), kinds[:5]):
        d[y, 101:] = v                                           # strips of 20, 24, 24, 24, 24 and 29 rows
    d[30:33, 5:9] = -0.0       # valid, 4 away from its surroundings: a region of 12
    d[29, 5:9] = d[33, 5:9] = d[30:33, 4] = d[30:33, 9] = 4.0   # (its surroundings, whatever the holes did)
    d[31, 6] = 0.5             # linked to -0.0: still one region of 12
    d[100:110, 110:120] = 0.0
    d[104, 114] = -0.0         # inside a block of +0.0: the same region, 100
    return case("invalid_kinds", d, 2000, full=True)


def random_map(seed=7, shape=BIG, subpixel=False):
    """Disparities from {1, 2, 4}: 1 and 2 are linked, 4 is not, so one region runs through the image and others
    of many sizes lie in it; 2 % invalid pixels of several kinds."""
    rng = np.random.RandomState(seed)
    d = rng.choice(np.array([1.0, 2.0, 4.0], np.float32), size=shape).astype(np.float32)
    if subpixel:
        d += (rng.randint(0, 8, size=shape) / 16.0).astype(np.float32)   # quarter steps and finer: still <= 1 + 7/16
    bad = rng.rand(*shape) < 0.02
    kinds = np.array([-1.0, np.nan, np.inf, -np.inf, -7.0], np.float32)
    d[bad] = rng.choice(kinds, size=int(bad.sum()))
    return d


def random_cases():
    d = random_map()
    s = random_map(11, subpixel=True)
    return [case("random", d, 8, full=True),
            case("random_fill_nan", d, 8, fill=np.nan, full=True),
            case("random_fill_7", d, 8, fill=7.0, full=True),
            case("random_max_size_0", d, 0),
            case("random_subpixel", s, 6),
            case("random_small", random_map(13, SMALL), 5, max_diff=0.0),
            case("random_narrow", random_map(17, (37, 19)), 4)]


def tiny_cases():
    one = lambda v: np.array([[v]], np.float32)   # noqa: E731
    return [case("1x1_gone", one(3.0), 1), case("1x1_kept", one(3.0), 0), case("1x1_nan", one(NAN_PAYLOAD), 5),
            case("1x1_negzero", one(-0.0), 1, fill=7.0),
            case("2x2", np.array([[1.0, 1.5], [-1.0, 9.0]], np.float32), 1)]


def all_cases():
    cases = [spiral_case(), serpentine_case(), comb_rows_case(), comb_cols_case(), u_case(), rings_case(),
             blob_case(), threshold_case(), threshold_tenth_case(), invalid_kinds_case()]
    cases += constant_cases() + checkerboard_cases() + ramp_cases() + random_cases() + tiny_cases()
    return cases


_EXPECTED = {}


def expected(c):
    """The literal's (out, mask, sizes) of a case, computed once per process and shared (read-only)."""
    if c["name"] not in _EXPECTED:
        from speckle_literal import speckle
        res = speckle(c["disp"], c["max_size"], c["max_diff"], c["fill"])
        for a in res:
            a.setflags(write=False)
        _EXPECTED[c["name"]] = res
    return _EXPECTED[c["name"]]
