"""CPU: the NumPy / Python-float restatement of post-processing and the stored-volume WTA (post_literal.py) against
hand-computed pictures and against the C oracle on every case table of post_cases.py, and the properties of those
tables that make the GPU comparisons of test_gpu_postprocess.py mean something.  Every comparison is by bytes.
"""
import numpy as np
import pytest

import post_cases as pc
import post_literal as pl

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def f32(rows):
    return np.array(rows, dtype=np.float32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------
# hand-computed pictures
# ----------------------------------------------------------------------------
def test_lr_check_pictures():
    init = np.full((1, 4), 7, np.uint8)
    # left: |0-0|, |1-0| = 1 (not > 1), c = 3: |-1-1| = 2, c = 2: |1-5|; right: c = 7 and c = 4 are past the row
    a, b, skipped = pl.lr_check(f32([[0, 1, -1, 1]]), f32([[0, 0, 5, 1]]), init, init)
    assert a.tolist() == [[0, 0, 1, 1]] and b.tolist() == [[0, 0, 7, 7]] and skipped == 0
    # left x = 3: c = 4 -> column 4 = W; right: c = -1 -> column 255, then NaN, +inf, -inf.  The left pixels that
    # are checked meet -1 (|0+1| = 1), NaN (no compare holds) and +inf
    a, b, skipped = pl.lr_check(f32([[0, 0, 0, -1]]), f32([[-1, NAN, INF, -INF]]), init, init)
    assert a.tolist() == [[0, 0, 1, 7]] and b.tolist() == [[7, 7, 7, 7]] and skipped == 5
    # the uint8 wrap at W = 300: x = 299 reads column 299 & 255 = 43
    dl, dr = np.zeros((1, 300), np.float32), np.zeros((1, 300), np.float32)
    dr[0, 43] = 5.0
    z = np.zeros((1, 300), np.uint8)
    a, b, skipped = pl.lr_check(dl, dr, z, z)
    assert np.flatnonzero(a[0]).tolist() == [43, 299] and np.flatnonzero(b[0]).tolist() == [43] and skipped == 0
    # -0.5 truncates toward zero (column 0), -1.5 to -1 (column 255 >= W)
    a, b, skipped = pl.lr_check(f32([[9, 9]]), f32([[-0.5, -2.5]]), init[:, :2], init[:, :2])
    assert a.tolist() == [[7, 7]] and b.tolist() == [[1, 7]] and skipped == 1


def test_lrc_fill_pictures():
    dl = f32([[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    flags = np.zeros((3, 3), np.uint8)
    flags[1, 1] = 1
    want = dl.copy()
    want[1, 1] = (2 + 8 + 6 + 4) / 4
    assert same(pl.lrc_fill(dl, flags), want)
    # bytes 2 and 255 are unflagged; (0,0): below 4, right 3 past the flagged (0,1); (0,1): below 5, right 3
    flags = np.array([[1, 1, 0], [0, 2, 0], [0, 0, 255]], np.uint8)
    want = dl.copy()
    want[0, 0], want[0, 1] = 3.5, 4.0
    assert same(pl.lrc_fill(dl, flags), want)
    # float64 sum in the order right, left; one rounding to float32
    a, b = np.float32(0.1), np.float32(0.2)
    got = pl.lrc_fill(f32([[a, 50, 60, b]]), np.array([[0, 1, 1, 0]], np.uint8))
    mean = np.float32((float(b) + float(a)) / 2)
    assert same(got, f32([[a, mean, mean, b]]))
    # three neighbours: 5 / 3 rounded once
    got = pl.lrc_fill(f32([[1, 9, 2], [7, 2, 7]]), np.array([[0, 1, 0], [0, 0, 0]], np.uint8))
    assert got[0, 1] == np.float32(5.0 / 3.0)
    # nothing unflagged: unchanged; NaN and +inf neighbours pass through the mean
    assert same(pl.lrc_fill(dl, np.ones((3, 3), np.uint8)), dl)
    got = pl.lrc_fill(f32([[INF, 5, 1], [NAN, 5, 1]]), np.array([[0, 1, 0], [0, 1, 0]], np.uint8))
    assert got[0, 1] == INF and np.isnan(got[1, 1])


def test_median5_pictures():
    rng = np.random.default_rng(3)
    src = rng.permutation(25).astype(np.float32).reshape(5, 5)
    dst = np.full((5, 5), -7, np.float32)
    want = dst.copy()
    want[2, 2] = 12
    assert same(pl.median5(src, dst), want)
    # not a sort once NaN is in the window: a NaN in front is "selected" first, a NaN at the back never is
    front = np.arange(25, dtype=np.float32).reshape(5, 5)
    front[0, 0] = NAN
    assert pl.median5(front, dst)[2, 2] == 12
    back = np.arange(1, 26, dtype=np.float32).reshape(5, 5)
    back[4, 4] = NAN
    assert pl.median5(back, dst)[2, 2] == 13
    assert np.isnan(pl.median5(np.full((5, 5), NAN), dst)[2, 2])
    # 13 equal zeros of both signs before anything larger: the 13th pick is the 13th in window order
    z = np.ones((5, 5), np.float32)
    z.ravel()[:13] = [0.0, -0.0] * 6 + [-0.0]
    got = pl.median5(z, dst)[2, 2]
    assert got == 0 and np.signbit(got)
    # no interior: dst untouched
    assert same(pl.median5(np.zeros((4, 9), np.float32), np.full((4, 9), 5, np.float32)), np.full((4, 9), 5, np.float32))


def test_wta_pictures():
    rows = [([3, 1, 1, 0, 0], 3, 3), ([INF, INF], -1, 0), ([NAN, 1, 0], 2, 0), ([2, NAN, 1, NAN, 1], 2, 2),
            ([-INF, -INF], 0, 0), ([INF, 5], 1, 1), ([NAN, NAN], -1, 0), ([4], 0, 0), ([INF], -1, 0)]
    for v, want_inf, want_d0 in rows:
        hwd = f32(v).reshape(1, 1, -1)
        for layout in ("HWD", "DHW"):
            vol = pc.as_layout(hwd, layout)
            assert pl.wta(vol, layout, "inf").tolist() == [[want_inf]], (v, layout)
            assert pl.wta(vol, layout, "d0").tolist() == [[want_d0]], (v, layout)


# ----------------------------------------------------------------------------
# the case tables: literal == oracle, and each case is not vacuous
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("W", pc.LR_WIDTHS)
def test_lr_check_cases(oracle, W):
    dl, dr = pc.lr_edge_maps(W)
    H = dl.shape[0]
    init = np.full((H, W), 0xA5, np.uint8)
    a, b, skipped = pl.lr_check(dl, dr, init, init)
    oa, ob = oracle.lr_check(dl, dr, init, init)
    assert same(a, oa) and same(b, ob)
    za, zb, _ = pl.lr_check(dl, dr, np.zeros_like(init), np.zeros_like(init))
    oa, ob = oracle.lr_check(dl, dr)
    assert same(za, oa) and same(zb, ob)
    for f in (a, b):
        assert {0, 1, 0xA5} <= set(np.unique(f).tolist())
    x = np.arange(W, dtype=np.float64)
    nonfinite = int((~np.isfinite(x - dl)).sum() + (~np.isfinite(x + dr)).sum())
    assert nonfinite >= 12 and skipped >= nonfinite
    # columns >= W exist exactly when the cast can produce one
    assert (skipped > nonfinite) == (W < 256)
    # the -1 entries that sent the parent's reads out of the row
    assert dl[H - 1, W - 1] == -1 and dr[0, 0] == -1
    assert (a[H - 1, W - 1] == 0xA5) == (W < 256) and (b[0, 0] == 0xA5) == (W < 256)


@pytest.mark.parametrize("W", pc.LR_WIDTHS)
def test_lr_consistency_cases(oracle, W):
    dl, dr = pc.lr_edge_maps(W)
    for md in (0.0, 0.5, 1.0):
        a, b = pl.lr_consistency(dl, dr, md)
        assert a.any() and not a.all() and b.any() and not b.all()
    if W <= 256:
        nl, nr = pc.lr_nonneg_maps(W)
        assert (nl >= 0).all() and (nr >= 0).all()
        a, b = pl.lr_consistency(nl, nr, 1.0)
        z = np.zeros(nl.shape, np.uint8)
        la, lb, skipped = pl.lr_check(nl, nr, z, z)
        assert same(a, la) and same(b, lb) and skipped == 0
        oa, ob = oracle.lr_check(nl, nr)
        assert same(a, oa) and same(b, ob)


@pytest.mark.parametrize("frac", pc.FILL_FRACS)
@pytest.mark.parametrize("H,W", pc.FILL_SHAPES)
def test_lrc_fill_cases(oracle, H, W, frac):
    dl, flags = pc.fill_case(H, W, frac)
    got = pl.lrc_fill(dl, flags)
    assert same(got, oracle.lrc_fill(dl, flags))
    assert set(np.unique(flags).tolist()) <= {0, 1, 2, 255}
    if H * W >= 64:
        assert abs((flags == 1).mean() - frac) < 0.15
    if H * W >= 1000:
        assert set(np.unique(flags).tolist()) == {0, 1, 2, 255}
        clear = flags != 1
        assert np.isnan(dl[clear]).any() and np.isinf(dl[clear]).any()
        filled = got[~clear]
        assert np.isnan(filled).any() and np.isinf(filled).any() and np.isfinite(filled).any()


@pytest.mark.parametrize("W", pc.FILL_WIDE)
def test_lrc_fill_wide_cases(oracle, W):
    """The widths around the kernel's 64 KiB of LDS.  The oracle's walks over the fully flagged row are quadratic
    in W (4 * 10^9 steps at W = 65534, a couple of seconds), so it is compared at the full widths; the flagged run and the
    fully flagged row are also checked by hand."""
    dl, flags = pc.fill_wide_case(W)
    got = pl.lrc_fill(dl, flags)
    assert same(got, oracle.lrc_fill(dl, flags))
    assert (flags[1] == 1).all() and 0.15 < (flags[[0, 2]] == 1).mean() < 0.3
    start = W // 2 - 2500 + 7
    assert (flags[0, start:start + 5000] == 1).all() and flags[0, start - 1] != 1 and flags[0, start + 5000] != 1
    # inside the run: below is flagged (row 1) down to row 2; right and left are the run's two ends
    x = start + 2500
    nb = [dl[2, x]] if flags[2, x] != 1 else []
    nb += [dl[0, start + 5000], dl[0, start - 1]]
    assert got[0, x].tobytes() == np.float32(sum(float(v) for v in nb) / len(nb)).tobytes()
    # the fully flagged row: only above and below
    x = int(np.flatnonzero((flags[0] != 1) & (flags[2] != 1))[0])
    assert got[1, x].tobytes() == np.float32((float(dl[0, x]) + float(dl[2, x])) / 2).tobytes()


@pytest.mark.parametrize("kind", pc.MEDIAN_KINDS)
@pytest.mark.parametrize("H,W", pc.MEDIAN_SHAPES)
def test_median5_cases(oracle, H, W, kind):
    src = pc.median_case(H, W, kind)
    dst = np.frombuffer(b"\xa5" * (4 * H * W), np.float32).reshape(H, W)
    got = pl.median5(src, dst)
    assert same(got, oracle.median5(src, dst))
    if H < 5 or W < 5:
        assert same(got, dst)
        return
    border = np.ones((H, W), bool)
    border[2:H - 2, 2:W - 2] = False
    assert got[border].tobytes() == dst[border].tobytes()
    win = np.lib.stride_tricks.sliding_window_view(src, (5, 5)).reshape(-1, 25)
    inner = got[2:H - 2, 2:W - 2].ravel()
    if kind == "ties":
        assert ((win == inner[:, None]).sum(1) >= 2).mean() > 0.1
    if kind == "zeros":
        assert (src == 0).mean() > 0.5 and np.signbit(src[src == 0]).any() and not np.signbit(src[src == 0]).all()
    if kind in ("nan", "inf"):
        nn = np.isnan(win).sum(1)
        assert ((nn > 0) & (nn < 25)).any()             # a NaN meets a number in some window
    if kind == "inf":
        assert np.isinf(src).any() and (src == -INF).any()
    if kind == "nan_window":
        assert np.isnan(win[-1]).all() and np.isnan(inner[-1])


@pytest.mark.parametrize("kind", pc.WTA_KINDS)
@pytest.mark.parametrize("H,W", pc.WTA_PIXELS)
@pytest.mark.parametrize("D", pc.WTA_D)
def test_wta_cases(oracle, D, H, W, kind):
    vol = pc.wta_case(H, W, D, kind)
    dhw = pc.as_layout(vol, "DHW")
    inf, d0 = pl.wta(vol, "HWD", "inf"), pl.wta(vol, "HWD", "d0")
    assert same(inf, oracle.WTA(vol, strict=False))
    assert same(inf, oracle.WTA1(dhw, strict=False))
    assert same(d0, oracle.wta_sgm(vol))
    assert same(pl.wta(dhw, "DHW", "inf"), inf) and same(pl.wta(dhw, "DHW", "d0"), d0)
    big = H * W >= 15
    if kind == "ties" and D >= 2 and big:
        mn = vol.min(2, keepdims=True)
        assert ((vol == mn).sum(2) >= 2).mean() > 0.1
        if D >= 17:
            assert ((inf % 16) != 0).any()                # first minima outside lane 0's residue
    if kind == "all_inf":
        assert (inf == -1).all() and (d0 == 0).all()
    if kind == "nan" and D >= 2:
        assert np.isnan(vol[0, 0, 0])
        if big:
            assert np.isnan(vol[:, :, 0]).any() and np.isnan(vol[:, :, 1:]).any()
            assert (inf != d0).any()                    # a NaN at d = 0 is kept by 'd0' and passed over by 'inf'
    if kind == "infs" and D >= 2 and big:
        assert (vol == -INF).any() and (vol[:, :, 0] == INF).any()
    if kind == "nan_row":
        assert (inf[H - 1] == -1).all() and (d0[H - 1] == 0).all()
