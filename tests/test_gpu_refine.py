"""sde_wta_subpixel, sde_cv_subpixel and sde_bilateral9 against the NumPy / Python-float restatement in
refine_literal.py, on the case tables of refine_cases.py (test_refine_host.py checks the restatement against
hand-computed pictures and that each case is not vacuous), and the two flags through StereoMatcher.

Every comparison is by bytes (no tolerances).  Output buffers arrive filled with 0xA5 bytes, so nothing depends on
what was there.  References are computed once per case.
"""
import functools

import numpy as np
import pytest
import torch

import post_literal as pl
import refine_cases as rc
import refine_literal as rl

pytestmark = pytest.mark.gpu

A5 = 0xA5


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()      # the case tables are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def junk(shape, dtype=torch.float32):
    """A buffer of 0xA5 bytes."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), A5, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def flip(a):
    return np.ascontiguousarray(a[:, ::-1])


# ----------------------------------------------------------------------------
# stored-volume WTA + refinement
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sub_want(H, W, D, kind, rule):
    return rl.wta_subpixel(rc.sub_case(H, W, D, kind), "HWD", rule).tobytes()


@pytest.mark.parametrize("H,W", rc.SUB_PIXELS)
@pytest.mark.parametrize("D", rc.SUB_D)
@pytest.mark.parametrize("rule", ["inf", "d0"])
@pytest.mark.parametrize("layout", ["DHW", "HWD"])
def test_wta_subpixel_volumes(gpu, layout, rule, D, H, W):
    """Both layouts and rules; D below, at and above the HWD kernel's 16 lanes per pixel, a wave's 64 and a float4
    multiple; one pixel, a last wave with idle lanes, more than one block.  Random wells, tie-heavy integers, NaN and
    +-inf, and the HWD cost volume's 1.0 fill."""
    from scenedepthestimation_amd import ops
    for kind in rc.SUB_KINDS:
        vol = rc.as_layout(rc.sub_case(H, W, D, kind), layout)
        got = host(ops.wta_subpixel(dev(vol), layout, rule, junk((H, W))))
        assert got.tobytes() == sub_want(H, W, D, kind, rule), kind


@pytest.mark.parametrize("layout", ["DHW", "HWD"])
def test_wta_subpixel_hand_pictures(gpu, layout):
    """The hand-computed pictures: 1.1666..., the near ties 2.5 / 2.375 / 2.625, den = 0, winners at 0 and D - 1,
    NaN and +-inf neighbours, -1 passing through."""
    from scenedepthestimation_amd import ops
    for D, (vol, want) in rc.hand_volume().items():
        got = host(ops.wta_subpixel(dev(rc.as_layout(vol, layout)), layout, "inf", junk(want.shape)))
        assert got.tobytes() == want.tobytes(), (D, got, want)
        got = host(ops.wta_subpixel(dev(rc.as_layout(vol, layout)), layout, "d0", junk(want.shape)))
        assert got.tobytes() == rl.wta_subpixel(vol, "HWD", "d0").tobytes(), D


@pytest.mark.parametrize("scale", rc.QUAD_SCALES)
def test_wta_subpixel_quadratic_volume(gpu, scale):
    from scenedepthestimation_amd import ops
    vol, _ = rc.quad_case(scale)
    got = host(ops.wta_subpixel(dev(vol), "HWD", "d0"))
    assert got.tobytes() == rl.wta_subpixel(vol, "HWD", "d0").tobytes()


def test_wta_subpixel_integer_part_is_wta(gpu):
    """The winner is sde_wta's: where nothing is refined the two maps agree, and rounding toward the winner never
    lands more than one away on the random wells."""
    from scenedepthestimation_amd import ops
    vol = dev(rc.sub_case(5, 130, 70, "random"))
    whole, sub = host(ops.wta(vol, "HWD", "d0")), host(ops.wta_subpixel(vol, "HWD", "d0"))
    assert (np.abs(sub - whole) < 1.0).all() and (sub != whole).mean() >= 0.5


def test_refusals(gpu):
    from scenedepthestimation_amd import _lib, ops
    from scenedepthestimation_amd._lib import SdeError
    vol, out = dev(np.zeros((2, 3, 4), np.float32)), junk((2, 3))
    st = torch.cuda.current_stream().cuda_stream
    assert _lib.lib.sde_wta_subpixel(vol.data_ptr(), 2, 3, 4, 7, 0, out.data_ptr(), st) == -1
    assert _lib.lib.sde_wta_subpixel(vol.data_ptr(), 2, 3, 4, 1, 2, out.data_ptr(), st) == -1
    assert _lib.lib.sde_wta_subpixel(None, 2, 3, 4, 1, 0, out.data_ptr(), st) == -1
    f = dev(np.zeros((2, 3, 8), np.float32))
    for side in (0, 3):                                   # neither, and both together
        assert _lib.lib.sde_cv_subpixel(f.data_ptr(), f.data_ptr(), 2, 3, 8, 0, 2, side, out.data_ptr(),
                                        out.data_ptr(), st) == -1
    assert _lib.lib.sde_cv_subpixel(f.data_ptr(), f.data_ptr(), 2, 3, 8, 2, 2, 1, out.data_ptr(), out.data_ptr(),
                                    st) == -1
    with pytest.raises(ValueError):
        ops.cv_subpixel(f, f, 0, 2, out, side="both")
    img, src = dev(np.zeros((2, 3), np.uint8)), dev(np.zeros((2, 3), np.float32))
    with pytest.raises(SdeError):
        ops.bilateral9(img, src, out=src)                 # dst == src
    assert host(out).tobytes() == host(junk((2, 3))).tobytes()


# ----------------------------------------------------------------------------
# volume-free refinement
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("d0,d1", rc.CV_RANGES)
@pytest.mark.parametrize("W", rc.CV_WIDTHS)
@pytest.mark.parametrize("C", rc.CV_CHANNELS)
def test_cv_subpixel(gpu, C, W, d0, d1):
    """Left view: on cv_wta's map over [d0, d1) the kernel equals the literal on the stored DHW volume, and over the
    whole range ops.wta_subpixel of that volume.  Right view: the flipped-image identity of ops.cv_wta_right's
    docstring -- the right view of (fl, fr) is the flip of the left view of (flip(fr), flip(fl)).  In place equals
    out of place.  A probe map of arbitrary integers, fractions, -1, NaN (one with a payload), +-inf and
    out-of-range values: what is not an integer in [d0, d1) comes back bit for bit."""
    from scenedepthestimation_amd import ops
    H, D = rc.CV_H, rc.CV_D
    fl, fr = rc.cv_features(W, C, d0, d1)
    dfl, dfr = dev(fl), dev(fr)
    vol_l = ops.cost_volume(dfl, dfr, D, layout="DHW")
    vol_r = host(ops.cost_volume(dev(flip(fr)), dev(flip(fl)), D, layout="DHW"))[:, :, ::-1]
    probe = rc.cv_probe_map(W, d0, d1)
    views = (("left", ops.cv_wta, host(vol_l)), ("right", ops.cv_wta_right, vol_r))
    for side, fused, vol in views:
        win, _, _ = fused(dfl, dfr, d0, d1, mode="exact")
        hwin = host(win).copy()
        want = rl.cv_subpixel(vol, hwin, d0, d1)
        got = ops.cv_subpixel(dfl, dfr, d0, d1, win, side, out=junk((H, W)))
        assert host(got).tobytes() == want.tobytes(), side
        assert host(win).tobytes() == hwin.tobytes()                   # the input is left alone
        if rc.cv_winners_refined(W, d0, d1):
            assert (want != hwin).mean() >= 0.5
        if side == "left" and (d0, d1) == (0, D):
            assert host(ops.wta_subpixel(vol_l, "DHW", "inf")).tobytes() == want.tobytes()
        same = ops.cv_subpixel(dfl, dfr, d0, d1, win, side, out=win)   # in place
        assert same is win and host(win).tobytes() == want.tobytes(), side
        got = host(ops.cv_subpixel(dfl, dfr, d0, d1, dev(probe), side, out=junk((H, W))))
        assert got.tobytes() == rl.cv_subpixel(vol, probe, d0, d1).tobytes(), side
        ok = (probe >= d0) & (probe < d1) & (probe == np.floor(probe))
        assert (got.view(np.uint32)[~ok] == probe.view(np.uint32)[~ok]).all() and (~ok).sum() >= 5


# ----------------------------------------------------------------------------
# 9x9 bilateral filter
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bil_want(H, W, kind):
    return rl.bilateral9(*rc.bil_case(H, W, kind)).tobytes()


@pytest.mark.parametrize("kind", rc.BIL_KINDS)
@pytest.mark.parametrize("H,W", rc.BIL_SHAPES)
def test_bilateral9(gpu, H, W, kind):
    """One pixel, an image smaller than the window, one full tile, tile seams and ragged edges; intensities on both
    sides of the threshold and near 0 at the zero padding; NaN and +inf in the map.  Image and map are the middle
    rows of taller tensors whose guard rows hold values that would change the result if they were read in place of
    the zero padding."""
    from scenedepthestimation_amd import ops
    img, src = rc.bil_case(H, W, kind)
    G = 5
    for guard_i, guard_d in ((0, 0.0), (4, float("nan")), (255, 1e6)):
        ti = torch.full((H + 2 * G, W), guard_i, dtype=torch.uint8, device="cuda")
        td = torch.full((H + 2 * G, W), guard_d, dtype=torch.float32, device="cuda")
        ti[G:G + H] = dev(img)
        td[G:G + H] = dev(src)
        out = junk((H + 2 * G, W))
        ops.bilateral9(ti[G:G + H], td[G:G + H], out=out[G:G + H])
        got = host(out)
        assert got[G:G + H].tobytes() == bil_want(H, W, kind), (guard_i, guard_d)
        a5 = host(junk((G, W))).tobytes()
        assert got[:G].tobytes() == a5 and got[G + H:].tobytes() == a5      # nothing written outside dst
    assert host(ops.bilateral9(dev(img), dev(src))).tobytes() == bil_want(H, W, kind)


# ----------------------------------------------------------------------------
# the flags through StereoMatcher
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def comp_pair():
    from scenedepthestimation_amd.synthetic import stereo_pair
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    left, right, _ = stereo_pair(H, W, D, seed=rc.COMP_SEED)
    return left, right


def matcher(**kw):
    from scenedepthestimation_amd.pipeline import StereoMatcher
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    m = StereoMatcher(H, W, D, weights="synthetic", **kw)
    m.load_images(*comp_pair())
    return m


def test_match_subpixel_equals_stored_volume(gpu):
    """StereoMatcher(subpixel=True).match() == wta_subpixel of the stored DHW volume of its own features; with
    the flag off the map is the plain matcher's."""
    from scenedepthestimation_amd import ops
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    m = matcher(subpixel=True)
    got = host(m.match()).copy()
    vol = ops.cost_volume(m.feat[0], m.feat[1], D, layout="DHW")
    assert got.tobytes() == host(ops.wta_subpixel(vol, "DHW", "inf")).tobytes()
    assert got.tobytes() == rl.wta_subpixel(host(vol), "DHW", "inf").tobytes()
    plain = host(matcher().match()).copy()
    assert host(matcher(subpixel=False, bilateral=False).match()).tobytes() == plain.tobytes()
    assert (got != plain).mean() > 0.3 and (np.abs(got - plain) < 1.0).all()
    assert plain.tobytes() == pl.wta(host(vol), "DHW", "inf").tobytes()


@functools.lru_cache(maxsize=None)
def lr_chain(subpixel, bilateral, oracle):
    """match_lr restated: the C oracle's exact cost volumes of both views from the device features, then the
    literals -- WTA (+ refinement), the wrap-free check, LRC fill, median (the border keeps the filled values),
    bilateral filter of the median's output with the left image."""
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    m = matcher()
    m.features()
    fl, fr = host(m.feat[0]).copy(), host(m.feat[1]).copy()
    vl = oracle.compute_cost_volume(fl, fr, D)
    vr = oracle.compute_cost_volume(flip(fr), flip(fl), D)[:, :, ::-1]
    if subpixel:
        dl, dr = rl.wta_subpixel(vl, "DHW", "inf"), rl.wta_subpixel(vr, "DHW", "inf")
    else:
        dl, dr = pl.wta(vl, "DHW", "inf"), pl.wta(vr, "DHW", "inf")
    a, _ = pl.lr_consistency(dl, dr, 1.0)
    filled = pl.lrc_fill(dl, a)
    out = pl.median5(filled, filled)
    if bilateral:
        out = rl.bilateral9(comp_pair()[0], out)
    return dl, dr, a, out


@pytest.mark.parametrize("bilateral", [False, True])
@pytest.mark.parametrize("subpixel", [False, True])
def test_match_lr_flags(gpu, oracle, subpixel, bilateral):
    m = matcher(subpixel=subpixel, bilateral=bilateral)
    checked, disp_r, lrc_l = (host(t).copy() for t in m.match_lr())
    dl, dr, a, want = lr_chain(subpixel, bilateral, oracle)
    assert host(m.disp).tobytes() == dl.tobytes()
    assert disp_r.tobytes() == dr.tobytes()
    assert lrc_l.tobytes() == a.tobytes() and 0 < a.sum() < a.size
    assert checked.tobytes() == want.tobytes()
    if not subpixel and not bilateral:
        plain = matcher()
        for got, ref in zip((checked, disp_r, lrc_l), plain.match_lr()):
            assert got.tobytes() == host(ref).tobytes()


@functools.lru_cache(maxsize=None)
def sgm_chain(subpixel, bilateral, oracle):
    """sgm_path restated: the C oracle's volumes, penalties and 8-path sums from the device features, then the
    literals -- WTA rule 'd0' (+ refinement), the reference's check, LRC fill, medians (borders keep the WTA maps),
    bilateral filter of each median's output with its own image."""
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    left, right = comp_pair()
    m = matcher()
    m.features()
    fl, fr = host(m.feat[0]).copy(), host(m.feat[1]).copy()
    cl, cr = oracle.cost_volume_hwd(fl, fr, D, invalid=1.0)
    Sl = oracle.sgm_8path(cl, oracle.sgm_penalties(left))
    Sr = oracle.sgm_8path(cr, oracle.sgm_penalties(right))
    if subpixel:
        wl, wr = rl.wta_subpixel(Sl, "HWD", "d0"), rl.wta_subpixel(Sr, "HWD", "d0")
    else:
        wl, wr = pl.wta(Sl, "HWD", "d0"), pl.wta(Sr, "HWD", "d0")
    z = np.zeros((H, W), np.uint8)
    a, _, _ = pl.lr_check(wl, wr, z, z)
    outl, outr = pl.median5(pl.lrc_fill(wl, a), wl), pl.median5(wr, wr)
    if bilateral:
        outl, outr = rl.bilateral9(left, outl), rl.bilateral9(right, outr)
    return wl, wr, outl, outr


@pytest.mark.parametrize("bilateral", [False, True])
@pytest.mark.parametrize("subpixel", [False, True])
def test_sgm_path_flags(gpu, oracle, subpixel, bilateral):
    m = matcher(sgm=True, subpixel=subpixel, bilateral=bilateral)
    m.features()
    wl, wr, outl, outr = sgm_chain(subpixel, bilateral, oracle)
    raw = [host(t).copy() for t in m.sgm_path(post=False)]
    assert raw[0].tobytes() == wl.tobytes() and raw[1].tobytes() == wr.tobytes()
    if subpixel:
        assert (wl != np.floor(wl)).mean() > 0.1
    got = [host(t).copy() for t in m.sgm_path()]
    assert got[0].tobytes() == outl.tobytes() and got[1].tobytes() == outr.tobytes()
    if not subpixel and not bilateral:
        plain = matcher(sgm=True)
        plain.features()
        for g, ref in zip(got, plain.sgm_path()):
            assert g.tobytes() == host(ref).tobytes()


def test_function_api_flags(gpu, oracle):
    """disparity_compute_by_gpu(..., subpixel=True, bilateral=True) is sgm_path with the flags on the same inputs."""
    from scenedepthestimation_amd import process_functional as pf
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    left, right = comp_pair()
    m = matcher(sgm=True, subpixel=True, bilateral=True)
    m.features()
    want = [host(t).copy() for t in m.sgm_path()]
    fl, fr = host(m.feat[0]).copy(), host(m.feat[1]).copy()
    dl, dr, _ = pf.disparity_compute_by_gpu(left, right, fl, fr, np.zeros(7, np.float32), ndisp=D, subpixel=True,
                                            bilateral=True)
    assert dl.tobytes() == want[0].tobytes() and dr.tobytes() == want[1].tobytes()
    assert dl.tobytes() == sgm_chain(True, True, oracle)[2].tobytes()


def test_shard_refuses_subpixel(gpu):
    from scenedepthestimation_amd.pipeline import StereoMatcher
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    with pytest.raises(ValueError):
        StereoMatcher(H, W, D, weights="synthetic", d_range=(0, D // 2), subpixel=True)
    StereoMatcher(H, W, D, weights="synthetic", d_range=(0, D // 2), bilateral=True)


def test_cli_flags(gpu, tmp_path, monkeypatch):
    """match_single with --subpixel / --bilateral writes uint8 of what the matcher returns with the flags on, on
    each of its three paths; the flags are refused where there is no median to filter."""
    from scenedepthestimation_amd import imageio, match_single
    (H, W), D = rc.COMP_SHAPE, rc.COMP_D
    left, right = comp_pair()
    imageio.imwrite(str(tmp_path / "eval" / "left_3.png"), left)
    imageio.imwrite(str(tmp_path / "eval" / "right_3.png"), right)
    monkeypatch.chdir(tmp_path)
    base = ["-i", "3", "-g", "0", "--checkpoint", "synthetic", "--ndisp", str(D)]

    def written(name):
        return imageio.imread_gray(str(tmp_path / "result" / name / "ld3.png"))

    match_single.main(base + ["--cpu-path", "--subpixel", "-f", "sub"])
    assert written("sub").tobytes() == host(matcher(subpixel=True).match()).astype("uint8").tobytes()
    match_single.main(base + ["--cpu-path", "--lr-check", "--subpixel", "--bilateral", "-f", "lr"])
    want = host(matcher(subpixel=True, bilateral=True).match_lr()[0]).astype("uint8")
    assert written("lr").tobytes() == want.tobytes()
    match_single.main(base + ["--subpixel", "--bilateral", "-f", "sgm"])
    m = matcher(sgm=True, subpixel=True, bilateral=True)
    m.features()
    assert written("sgm").tobytes() == host(m.sgm_path()[0]).astype("uint8").tobytes()
    with pytest.raises(SystemExit):
        match_single.main(base + ["--cpu-path", "--bilateral"])
