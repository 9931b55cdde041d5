"""GPU: sdi_classify and sdi_interpolate (csrc/interp.hip) against the restatement in tests/interp_literal.py, by bytes.
Outputs and the workspace arrive filled with 0xAA bytes, the u8 maps with guard bytes on both sides.  The references
of the larger pictures come from the restatement's chain form (interpolate_chain_sides), which tests/test_interp_host.py
holds against the per-pixel walk; the small pictures are checked against the walk itself as well."""
import functools

import numpy as np
import pytest
import torch

import interp_literal as il
import post_literal as pl

pytestmark = pytest.mark.gpu

AA = 0xAA
LEAD, TAIL = 5, 8
F = np.float32
SIDES = ("left", "right")


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def junk(shape, dtype=torch.float32):
    """A buffer of 0xAA bytes."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), AA, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def guarded(H, W):
    """A u8 [H,W] view with guard bytes around it -> (whole buffer, view)."""
    buf = junk((LEAD + H * W + TAIL,), torch.uint8)
    return buf, buf[LEAD:LEAD + H * W].view(H, W)


def guards_kept(buf):
    b = host(buf)
    return (b[:LEAD] == AA).all() and (b[-TAIL:] == AA).all()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bits = {1: np.uint8, 4: np.uint32}[got.dtype.itemsize]
        where = np.argwhere(got.view(bits) != want.view(bits))
        raise AssertionError(f"{what}: {len(where)} differ, first {where[:5].tolist()}: "
                             f"got {got[tuple(where[0])]!r}, want {want[tuple(where[0])]!r}")


# ----------------------------------------------------------------------------
# pictures
# ----------------------------------------------------------------------------
def random_picture(seed, H, W, flagged):
    """disp with ties, -0.0 and invalid values, cls with both classes and a few bytes that read as 0."""
    rng = np.random.default_rng(seed)
    disp = (rng.random((H, W)) * 60).astype(F)
    disp[rng.random((H, W)) < 0.2] = F(7.0)
    bad = rng.random((H, W)) < 0.08
    nan = np.frombuffer(np.uint32(0xffc00abc).tobytes(), F)[0]
    disp[bad] = rng.choice(np.array([nan, -1.0, np.inf, -0.0], F), int(bad.sum()))
    cls = np.where(rng.random((H, W)) < flagged, rng.choice(np.array([1, 2, 2], np.uint8), (H, W)), 0).astype(np.uint8)
    odd = rng.random((H, W)) < 0.02
    cls[odd] = rng.choice(np.array([3, 255], np.uint8), int(odd.sum()))
    return disp, cls


def corner_picture(H=96, W=130):
    """The only source is the corner pixel (0, 0): the longest walks; pixels off its rays stay as they are."""
    rng = np.random.default_rng(1)
    disp = np.full((H, W), -1.0, F)
    cls = rng.choice(np.array([1, 2, 2, 2], np.uint8), (H, W))
    disp[0, 0], cls[0, 0] = 11.5, 0
    cls[95, 95] = cls[47, 94] = 2     # step 95 of the ray (-2, -2) and step 94 of the ray (-2, -1) are (0, 0)
    cls[60, 60] = cls[30, 60] = 1     # the same pixels' kind as occlusions: their rows hold no source
    return disp, cls


def runs_picture(H=5, W=130):
    """Flagged runs that start, end and cross at the 32- and 64-column boundaries of the bitmap's words."""
    disp = (np.arange(H * W, dtype=F).reshape(H, W) % 97) + F(0.25)
    cls = np.zeros((H, W), np.uint8)
    for y, kind, runs in ((0, 2, ((60, 70), (31, 33), (127, 130))),        # mismatches across the boundaries
                          (1, 1, ((60, 70), (0, 33), (96, 129))),          # occlusions across them
                          (2, 1, ((1, 128),)),                             # one run over three words and a half
                          (3, 1, ((63, 65), (31, 32), (0, 1), (129, 130))),
                          (4, 1, ((0, 64), (65, 130)))):                   # the only source starts the second chunk
        for lo, hi in runs:
            cls[y, lo:hi] = kind
    return disp, cls


PICTURES = {
    "1x1_source": lambda: (np.array([[3.0]], F), np.array([[0]], np.uint8)),
    "1x1_mismatch": lambda: (np.array([[np.nan]], F), np.array([[2]], np.uint8)),
    "1x130_p50": lambda: random_picture(2, 1, 130, 0.5),
    "65x1_p50": lambda: random_picture(3, 65, 1, 0.5),
    "5x63_p95": lambda: random_picture(4, 5, 63, 0.95),
    "5x64_p50": lambda: random_picture(5, 5, 64, 0.5),
    "5x65_p05": lambda: random_picture(6, 5, 65, 0.05),
    "5x130_p95": lambda: random_picture(7, 5, 130, 0.95),
    "65x63_p50": lambda: random_picture(8, 65, 63, 0.5),
    "65x64_p95": lambda: random_picture(9, 65, 64, 0.95),
    "65x65_p05": lambda: random_picture(10, 65, 65, 0.05),
    "65x130_p05": lambda: random_picture(11, 65, 130, 0.05),
    "65x130_p50": lambda: random_picture(12, 65, 130, 0.5),
    "65x130_p95": lambda: random_picture(13, 65, 130, 0.95),
    "all_flagged": lambda: (random_picture(14, 33, 70, 0.0)[0], np.random.default_rng(14).choice(
        np.array([1, 2], np.uint8), (33, 70))),
    "corner_source": corner_picture,
    "runs_across_chunks": runs_picture,
}
SMALL = ("1x1_source", "1x1_mismatch", "1x130_p50", "65x1_p50", "5x63_p95", "5x64_p50", "5x65_p05", "5x130_p95",
         "runs_across_chunks")


@functools.lru_cache(maxsize=None)
def picture(name):
    disp, cls = PICTURES[name]()
    want = il.interpolate_chain_sides(disp, cls)
    for a in (disp, cls) + tuple(x for pair in want.values() for x in pair):
        a.setflags(write=False)
    return disp, cls, want


def run_interp(disp, cls, side, filled=True, workspace=None):
    from scenedepthestimation_amd import ops
    H, W = disp.shape
    out = junk((H, W))
    fbuf, f = guarded(H, W) if filled else (None, None)
    ws = junk((ops.interpolate_workspace_bytes(H, W),), torch.uint8) if workspace is None else workspace
    ro, rf = ops.interpolate(dev(disp), dev(cls), side, out=out, filled=f, want=(), workspace=ws)
    assert ro is out and rf is f
    if filled:
        assert guards_kept(fbuf), "guard bytes of filled"
    return host(out), host(f) if filled else None


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", sorted(PICTURES))
def test_interpolate_picture(gpu, name, side):
    disp, cls, want = picture(name)
    out, filled = run_interp(disp, cls, side)
    same(out, want[side][0], f"{name} {side} out")
    same(filled, want[side][1], f"{name} {side} filled")
    if name in SMALL:
        walk = il.interpolate(disp, cls, side)
        same(out, walk[0], f"{name} {side} out against the walk")
        same(filled, walk[1], f"{name} {side} filled against the walk")


def test_pictures_are_not_vacuous(gpu):
    for name in PICTURES:
        disp, cls, want = picture(name)
        if name == "all_flagged":
            assert not want["left"][1].any() and not want["right"][1].any()       # nothing is filled
            assert want["left"][0].tobytes() == disp.tobytes()
        elif name == "corner_source":
            out, f = want["left"]
            assert f[0, 1:].all() and f[95, 95] == 1 and f[47, 94] == 1 and out[95, 95] == out[47, 94] == 11.5
            assert f[60, 60] == 0 and f[30, 60] == 0 and f[46, 93] == 0 and not f.all()
        elif not name.startswith("1x1"):
            assert want["left"][1].any()
            if disp.shape[1] > 1:
                assert want["left"][0].tobytes() != want["right"][0].tobytes(), name


@pytest.mark.parametrize("name", ["65x130_p50", "runs_across_chunks", "1x1_mismatch"])
def test_interpolate_without_filled(gpu, name):
    disp, cls, want = picture(name)
    out, _ = run_interp(disp, cls, "left", filled=False)
    same(out, want["left"][0], name)


@pytest.mark.parametrize("name", ["65x130_p95", "5x65_p05"])
def test_interpolate_workspace_alignment(gpu, name):
    """The header asks for 4-byte alignment of the workspace and no more: a view 4 bytes into an allocation."""
    from scenedepthestimation_amd import ops
    disp, cls, want = picture(name)
    n = ops.interpolate_workspace_bytes(*disp.shape)
    buf = junk((n + 16,), torch.uint8)
    ws = buf[4:4 + n]
    assert ws.data_ptr() % 8 == 4
    out, filled = run_interp(disp, cls, "right", workspace=ws)
    same(out, want["right"][0], name)
    same(filled, want["right"][1], name)
    assert (host(buf)[n + 4:] == AA).all() and (host(buf)[:4] == AA).all()


@pytest.mark.parametrize("name", ["65x130_p50", "corner_source"])
def test_interpolate_twice_on_the_same_buffers(gpu, name):
    from scenedepthestimation_amd import ops
    disp, cls, want = picture(name)
    H, W = disp.shape
    d, c, out, f = dev(disp), dev(cls), junk((H, W)), junk((H, W), torch.uint8)
    ws = junk((ops.interpolate_workspace_bytes(H, W),), torch.uint8)
    for k in range(2):
        ops.interpolate(d, c, "left", out=out, filled=f, workspace=ws)
        same(host(out), want["left"][0], f"{name} call {k}")
        same(host(f), want["left"][1], f"{name} call {k}")
    same(host(d), disp, "disp is left as it is")
    same(host(c), cls, "cls is left as it is")


# ----------------------------------------------------------------------------
# classify
# ----------------------------------------------------------------------------
def classify_maps(seed, H, W, D, flagged):
    rng = np.random.default_rng(seed)
    other = (rng.random((H, W)) * (D + 3) - 1.5).astype(F)
    whole = rng.random((H, W)) < 0.5
    other[whole] = np.round(other[whole] * 4) / 4        # quarters: compares that land exactly on max_diff
    bad = rng.random((H, W)) < 0.1
    other[bad] = rng.choice(np.array([np.nan, -1.0, np.inf, -0.0], F), int(bad.sum()))
    lrc = np.where(rng.random((H, W)) < flagged, 1, rng.choice(np.array([0, 0, 2, 255], np.uint8), (H, W)))
    return other, lrc.astype(np.uint8)


CLASSIFY = [(1, 1, 1, 0.5, 1.0), (1, 130, 40, 0.5, 1.0), (65, 1, 5, 0.5, 0.0), (5, 63, 70, 0.95, 0.5),
            (5, 64, 16, 0.05, 2.75), (5, 65, 1, 0.5, 0.25), (65, 130, 24, 0.5, 1.0), (65, 130, 200, 0.95, 1.5),
            # the kernel works in 256-column segments: rows of one segment exactly, two, three; D within a segment,
            # across one boundary, across two
            (3, 256, 40, 0.5, 1.0), (3, 257, 9, 0.5, 0.5), (2, 600, 300, 0.9, 1.0), (2, 515, 700, 0.5, 3.0)]


@functools.lru_cache(maxsize=None)
def classify_case(H, W, D, flagged, md):
    """The maps and, per side, the header-literal scan (il.classify); the coverage restatement must agree with it."""
    other, lrc = classify_maps(H * 1000 + W + D, H, W, D, flagged)
    want = {side: il.classify(other, lrc, D, side, md) for side in SIDES}
    for side in SIDES:
        assert np.array_equal(want[side], il.classify_coverage(other, lrc, D, side, md))
    return other, lrc, want


@pytest.mark.parametrize("in_place", (False, True))
@pytest.mark.parametrize("H, W, D, flagged, md", CLASSIFY)
def test_classify(gpu, H, W, D, flagged, md, in_place):
    from scenedepthestimation_amd import ops
    other, lrc, wants = classify_case(H, W, D, flagged, md)
    for side in SIDES:
        want = wants[side]
        buf, cls = guarded(H, W)
        if in_place:
            cls.copy_(dev(lrc))
        got = ops.classify(dev(other), cls if in_place else dev(lrc), D, side, md, out=cls)
        assert got is cls and guards_kept(buf)
        same(host(cls), want, f"{H}x{W} D={D} {side} max_diff={md}")


def test_bad_arguments_launch_nothing(gpu):
    """The argument checks on device pointers: every refused call leaves the 0xAA outputs as they were."""
    from scenedepthestimation_amd import _lib, ops
    lib, ERR = _lib.lib, _lib.SDE_ERR_ARG
    H, W = 4, 6
    d, c = dev(np.zeros((H, W), F)), dev(np.ones((H, W), np.uint8))
    out, cls, fl = junk((H, W)), junk((H, W), torch.uint8), junk((H, W), torch.uint8)
    n = ops.interpolate_workspace_bytes(H, W)
    ws = junk((n + 8,), torch.uint8)
    p = lambda t: t.data_ptr()   # noqa: E731
    L = _lib.SDE_SIDE_LEFT
    for md in (-1.0, float("nan"), float("inf")):
        assert lib.sdi_classify(p(d), p(c), H, W, 4, L, md, p(cls), None) == ERR
    assert lib.sdi_classify(p(d), p(c), H, W, 0, L, 1.0, p(cls), None) == ERR
    assert lib.sdi_classify(p(d), p(c), H, W, 4, 0, 1.0, p(cls), None) == ERR
    assert lib.sdi_classify(p(d), p(c), H, W, 4, 3, 1.0, p(cls), None) == ERR
    assert lib.sdi_classify(None, p(c), H, W, 4, L, 1.0, p(cls), None) == ERR
    assert lib.sdi_classify(p(d), p(c), H, 0, 4, L, 1.0, p(cls), None) == ERR
    assert lib.sdi_interpolate(p(d), p(c), H, W, L, p(d), p(fl), p(ws), n, None) == ERR          # out == disp
    assert lib.sdi_interpolate(p(d), p(c), H, W, 0, p(out), p(fl), p(ws), n, None) == ERR
    assert lib.sdi_interpolate(p(d), p(c), 0, W, L, p(out), p(fl), p(ws), n, None) == ERR
    assert lib.sdi_interpolate(p(d), None, H, W, L, p(out), p(fl), p(ws), n, None) == ERR
    assert lib.sdi_interpolate(p(d), p(c), H, W, L, p(out), p(fl), None, n, None) == ERR
    assert lib.sdi_interpolate(p(d), p(c), H, W, L, p(out), p(fl), p(ws) + 2, n, None) == ERR
    assert lib.sdi_interpolate(p(d), p(c), H, W, L, p(out), p(fl), p(ws), n - 1, None) == _lib.SDE_ERR_WORKSPACE
    for t in (out, cls, fl, ws):
        assert (host(t.view(torch.uint8)) == AA).all()
    assert not host(d).any() and host(c).all()
    with pytest.raises(ValueError, match="side"):
        ops.interpolate(d, c, "up")
    with pytest.raises(_lib.SdeError, match="sdi_interpolate"):
        ops.interpolate(d, c, out=d)
    with pytest.raises(_lib.SdeError, match="sdi_classify"):
        ops.classify(d, c, 4, max_diff=-1.0)
    with pytest.raises(TypeError, match="uint8"):
        ops.classify(d, d, 4)


# ----------------------------------------------------------------------------
# the stage in the pipelines
# ----------------------------------------------------------------------------
H_, W_, D_ = 48, 160, 32


@functools.lru_cache(maxsize=None)
def pair(H=H_, W=W_, D=D_, seed=4):
    from scenedepthestimation_amd.synthetic import stereo_pair
    left, right, _ = stereo_pair(H, W, D, seed=seed)
    return left, right


def composed(raw_l, raw_r, lrc, D, max_diff, border=None):
    """classify + interpolate + 5x5 median of the left map through the restatements -> (checked, cls, filled map,
    filled mask); border: the map whose 2-pixel border the median keeps (default: the interpolated map)."""
    cls = il.classify(raw_r, lrc, D, "left", max_diff)
    filled, mask = il.interpolate_chain(raw_l, cls, "left")
    assert (cls == 1).any() and (cls == 2).any() and mask.any()
    return pl.median5(filled, filled if border is None else border), cls, filled, mask


def check_checked_path(m, what):
    got, got_r, got_lrc = (host(t).copy() for t in m.match_lr())
    raw_l = host(m.disp).copy()
    lrc = pl.lr_consistency(raw_l, got_r, 1.0)[0]
    same(got_lrc, lrc, what + " lrc_l")
    want, cls, filled, mask = composed(raw_l, got_r, lrc, m.D, 1.0)
    same(host(m.checked.interp.cls), cls, what + " cls")
    same(host(m.checked.bufs["filled"]), filled, what + " interpolated map")
    same(host(m.checked.interp.filled), mask, what + " filled mask")
    same(got, want, what + " match_lr()")
    return got, raw_l, got_r, lrc


def test_local_matcher_interpolates(gpu):
    from scenedepthestimation_amd.local_method import LocalMatcher
    plain, explicit = LocalMatcher(H_, W_, D_, method="census"), LocalMatcher(H_, W_, D_, method="census", fill="mean4")
    m = LocalMatcher(H_, W_, D_, method="census", fill="interpolate")
    for x in (plain, explicit, m):
        x.load_images(*pair())
    a, b = plain.match_lr(), explicit.match_lr()
    for x, y in zip(a, b):
        same(host(x), host(y), "fill='mean4' is the call without the argument")
    assert explicit.checked.interp is None and plain.checked.interp is None
    got, raw_l, raw_r, lrc = check_checked_path(m, "LocalMatcher")
    same(raw_l, host(plain.disp), "raw left map")
    same(raw_r, host(a[1]), "raw right map")
    same(lrc, host(a[2]), "flags")
    assert got.tobytes() != host(a[0]).tobytes()


def test_stereo_matcher_interpolates(gpu):
    from scenedepthestimation_amd.pipeline import StereoMatcher
    plain = StereoMatcher(H_, W_, D_, weights="synthetic")
    explicit = StereoMatcher(H_, W_, D_, weights="synthetic", fill="mean4")
    m = StereoMatcher(H_, W_, D_, weights="synthetic", fill="interpolate")
    for x in (plain, explicit, m):
        x.load_images(*pair())
    a, b = plain.match_lr(), explicit.match_lr()
    for x, y in zip(a, b):
        same(host(x), host(y), "fill='mean4' is the call without the argument")
    assert explicit.checked.interp is None and explicit.sgm.interp is None
    got, raw_l, raw_r, lrc = check_checked_path(m, "StereoMatcher")
    same(raw_l, host(plain.disp), "raw left map")
    same(lrc, host(a[2]), "flags")
    assert got.tobytes() != host(a[0]).tobytes()
    with pytest.raises(ValueError, match="fill"):
        StereoMatcher(H_, W_, D_, weights="synthetic", fill="median")


@pytest.mark.parametrize("unique", (False, True))
def test_sgm_path_interpolates(gpu, unique):
    """post=True with fill='interpolate': the path's own check (bound 1), the uniqueness OR when set, classify +
    interpolate instead of the LRC fill, the median into the raw left map; the right map as without the option."""
    from scenedepthestimation_amd import ops
    from scenedepthestimation_amd.pipeline import StereoMatcher
    H, W, D = 24, 64, 16
    imgs = pair(H, W, D, 6)
    tau = None
    if unique:
        probe = StereoMatcher(H, W, D, weights="synthetic", unique=0.0)
        probe.load_images(*imgs)
        probe.features()
        probe.sgm_path(post=False)
        tau = float(ops.wta_unique(probe.sgm.bufs["S"][0], 0.0, "HWD", "d0", want=("margin",))[0].median())
    plain, explicit = (StereoMatcher(H, W, D, weights="synthetic", unique=tau, **kw) for kw in ({}, {"fill": "mean4"}))
    m = StereoMatcher(H, W, D, weights="synthetic", unique=tau, fill="interpolate")
    for x in (plain, explicit, m):
        x.load_images(*imgs)
        x.features()
    a = [host(t).copy() for t in plain.sgm_path()]
    for x, y in zip(a, explicit.sgm_path()):
        same(x, host(y), "fill='mean4' is the call without the argument")
    m.sgm_path(post=False)
    if unique:
        raw_l, raw_r = (host(ops.wta(s, "HWD", "d0")).copy() for s in m.sgm.bufs["S"])
        rej = host(m.sgm.unique_mask).copy()
        assert rej.any() and not rej.all()
    else:
        raw_l, raw_r = (host(t).copy() for t in m.sgm.bufs["disp"])
        rej = np.zeros((H, W), np.uint8)
    got_l, got_r = (host(t).copy() for t in m.sgm_path())
    zero = np.zeros((H, W), np.uint8)
    lrc = pl.lr_check(raw_l, raw_r, zero, zero)[0] | rej
    same(host(m.sgm.bufs["lrc"][0]), lrc, "flags")
    want, cls, filled, mask = composed(raw_l, raw_r, lrc, D, 1.0, border=raw_l)
    same(host(m.sgm.interp.cls), cls, "cls")
    same(host(m.sgm.bufs["disp_a"]), filled, "interpolated map")
    same(got_l, want, "sgm left")
    same(got_r, a[1], "sgm right")


def test_cli_fill_interpolate(gpu, tmp_path):
    from scenedepthestimation_amd import imageio, local_method
    from scenedepthestimation_amd.local_method import LocalMatcher
    left, right = pair()
    imageio.imwrite(str(tmp_path / "eval" / "left_0.png"), left)
    imageio.imwrite(str(tmp_path / "eval" / "right_0.png"), right)
    common = ["--image-dir", str(tmp_path / "eval"), "-n", "1", "--ndisp", str(D_), "--method", "census", "--lr-check"]
    local_method.main(common + ["--fill", "interpolate", "--out-dir", str(tmp_path / "interp")])
    local_method.main(common + ["--out-dir", str(tmp_path / "mean4")])
    maps = {}
    for fill in ("interpolate", "mean4"):
        m = LocalMatcher(H_, W_, D_, "census", fill=fill)
        m.load_images(left, right)
        maps[fill] = host(m.match_lr()[0]).astype("uint8")
    assert imageio.imread_gray(str(tmp_path / "interp" / "ld0.png")).tobytes() == maps["interpolate"].tobytes()
    assert imageio.imread_gray(str(tmp_path / "mean4" / "ld0.png")).tobytes() == maps["mean4"].tobytes()
    assert maps["interpolate"].tobytes() != maps["mean4"].tobytes()
