"""sdg_rectify_map, sdg_remap_u8 and sdg_reproject against the NumPy restatement in geom_literal.py on the inputs of
geom_cases.py (test_geom_host.py checks the restatement against hand-made pictures), and the stage through
Rectifier and StereoMatcher.load_raw.

Every comparison is by bytes (no tolerances).  Output buffers arrive filled with 0xAA bytes, with guard bytes on both
sides where a kernel writes single bytes.  References are computed once per case.
"""
import functools

import numpy as np
import pytest
import torch

import geom_cases as gc
import geom_literal as gl

pytestmark = pytest.mark.gpu

AA = 0xAA


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()      # the cached cases are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def junk(shape, dtype=torch.float32):
    """A buffer of 0xAA bytes."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), AA, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


# ----------------------------------------------------------------------------
# the map
# ----------------------------------------------------------------------------
MAP_CALS = {"distorted": gc.distorted_cal, "zero_crossing": gc.zero_crossing_cal, "huge": gc.huge_cal}


@functools.lru_cache(maxsize=None)
def map_want(name, H, W):
    return gl.rectify_map(MAP_CALS[name](), H, W)


@pytest.mark.parametrize("H,W", [(41, 70), (5, 3), (1, 1), (3, 259)])
@pytest.mark.parametrize("name", sorted(MAP_CALS))
def test_rectify_map(gpu, name, H, W):
    """Radial, tangential and rational terms under a 5 degree rotation; a Wd that crosses zero inside the image
    (infinities and a NaN -> SDG_NO_SAMPLE); coordinates past 2^30 (-> SDG_NO_SAMPLE, beside ones that fit).  One
    pixel, fewer pixels than a wave, more than one block, a row longer than a block."""
    from scenedepthestimation_amd import ops
    want = map_want(name, H, W)
    if (H, W) == (41, 70) and name != "distorted":
        none = (want == gl.NO_SAMPLE).all(axis=2)
        assert none.any() and not none.all()                     # the case is not vacuous
    out = junk((H, W, 2), torch.int32)
    cal = MAP_CALS[name]()
    ops.rectify_map(cal, H, W, out=out)
    cal[:] = np.nan                                              # the host array was copied by value on the call
    got = host(out)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]


# ----------------------------------------------------------------------------
# the remap
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def remap_want(nimg, H, W):
    src, maps = gc.remap_case(nimg, H, W)
    return gl.remap_u8(src, maps)


def guarded(nimg, npix, lead):
    """A u8 buffer of 0xAA with `lead` guard bytes in front and 8 behind; (whole buffer, the [nimg * npix] view)."""
    buf = junk((lead + nimg * npix + 8,), torch.uint8)
    return buf, buf[lead:lead + nimg * npix]


@pytest.mark.parametrize("lead_dst,lead_valid", [(0, 0), (1, 3), (2, 0), (3, 2)])
@pytest.mark.parametrize("nimg,H,W", [(2, 41, 70), (2, 5, 3), (1, 41, 70), (1, 5, 3)])
def test_remap_edges(gpu, nimg, H, W, lead_dst, lead_valid):
    """A 37 x 53 source per image, each image through its own map: fractions 0 and 31 on each axis, a = -1 (x0 = -1,
    fx = 31), x0 = -1 with fx = 0 (nothing inside), x0 = Ws - 1 with fx = 0 (valid) and fx = 1 (not), the same in
    y, SDG_NO_SAMPLE in both words and in one, +-(2^30 - 1), INT_MAX, then random entries straddling all four
    borders.  H * W = 2870 and 15 are no multiples of 4, so the second image starts off a dword boundary; the
    lead bytes move dst and valid onto every alignment, together and apart.  dst, valid and the guard bytes around
    them start as 0xAA."""
    from scenedepthestimation_amd import ops
    src, maps = gc.remap_case(nimg, H, W)
    want_dst, want_valid = remap_want(nimg, H, W)
    n = H * W
    dbuf, dst = guarded(nimg, n, lead_dst)
    vbuf, valid = guarded(nimg, n, lead_valid)
    ops.remap_u8(dev(src), dev(maps), out=dst.view(nimg, H, W), valid=valid.view(nimg, H, W))
    got, gv = host(dst).reshape(nimg, H, W), host(valid).reshape(nimg, H, W)
    assert got.tobytes() == want_dst.tobytes(), np.argwhere(got != want_dst)[:5]
    assert gv.tobytes() == want_valid.tobytes(), np.argwhere(gv != want_valid)[:5]
    for buf, lead in ((dbuf, lead_dst), (vbuf, lead_valid)):
        b = host(buf)
        assert (b[:lead] == AA).all() and (b[lead + nimg * n:] == AA).all()
    # without valid: the same picture
    dbuf, dst = guarded(nimg, n, lead_dst)
    ops.remap_u8(dev(src), dev(maps), out=dst.view(nimg, H, W))
    assert host(dst).tobytes() == want_dst.tobytes()


def test_remap_half_and_saturation(gpu):
    """A sum that lands exactly on a half rounds up (p = 1, 0 at fx = 16 gives 1; 0, 1 likewise), and an all-255
    source gives 255 at every fraction: no overflow past a byte."""
    from scenedepthestimation_amd import ops
    Hs, Ws = 37, 53
    src = np.zeros((2, Hs, Ws), np.uint8)
    src[0, :, ::2] = 1
    src[1] = 255
    v, u = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    m0 = np.stack([32 * u + 16, 32 * v], axis=-1)                 # between a 1 and a 0
    m1 = np.stack([32 * 3 + u, 32 * 4 + v], axis=-1)              # every (fx, fy)
    maps = np.stack([m0, m1]).astype(np.int32)
    want_dst, want_valid = gl.remap_u8(src, maps)
    assert (want_dst[0] == 1).all() and (want_dst[1] == 255).all() and want_valid.all()
    dst, valid = junk((2, 32, 32), torch.uint8), junk((2, 32, 32), torch.uint8)
    ops.remap_u8(dev(src), dev(maps), out=dst, valid=valid)
    assert host(dst).tobytes() == want_dst.tobytes() and host(valid).tobytes() == want_valid.tobytes()


def test_remap_refuses_overlap(gpu):
    from scenedepthestimation_amd import ops
    buf = torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        ops.remap_u8(buf, torch.zeros((2, 8, 8, 2), dtype=torch.int32, device="cuda"), out=buf)


# ----------------------------------------------------------------------------
# the reprojection
# ----------------------------------------------------------------------------
def rectified_Q():
    from scenedepthestimation_amd.rectify import rodrigues, stereo_rectify
    K1 = np.array([[61.5, 0, 6.25], [0, 60.75, 4.5], [0, 0, 1.0]])
    K2 = np.array([[60.5, 0, 6.75], [0, 61.25, 4.0], [0, 0, 1.0]])
    return stereo_rectify(K1, K2, rodrigues([0.02, -0.03, 0.015]), [-0.12, 0.004, -0.003])[4]


@pytest.mark.parametrize("outputs", ["depth", "xyz", "both"])
@pytest.mark.parametrize("min_disp", [0.0, 1.5])
@pytest.mark.parametrize("q", ["rectified", "dense"])
def test_reproject(gpu, q, min_disp, outputs):
    """-1, 0, -0, NaN, +-inf, 2.625, a value equal to min_disp and its two float32 neighbours among ordinary values;
    the Q of stereo_rectify and one with 16 non-zero entries; each output alone and both together."""
    from scenedepthestimation_amd import ops
    Q = rectified_Q() if q == "rectified" else gc.dense_Q()
    disp = gc.reproject_disp(min_disp)
    want_depth, want_xyz = gl.reproject(disp, Q, min_disp)
    assert not np.isnan(want_xyz).any()                          # NaN payloads are not part of the contract
    depth = junk((9, 13)) if outputs != "xyz" else None
    xyz = junk((9, 13, 3)) if outputs != "depth" else None
    ops.reproject(dev(disp), Q, min_disp, depth=depth, xyz=xyz, want=())
    if depth is not None:
        assert host(depth).tobytes() == want_depth.tobytes()
    if xyz is not None:
        assert host(xyz).tobytes() == want_xyz.tobytes()


def test_reproject_infinite_depth(gpu):
    """depth is what the arithmetic gives, infinities included: a Q whose last row vanishes at d = 2."""
    from scenedepthestimation_amd import ops
    Q = np.array([[1.0, 0, 0, -6], [0, 1, 0, -4], [0, 0, 0, 64], [0, 0, 8.0, -16.0]])
    disp = np.full((9, 13), 2.0, np.float32)
    disp[4] = 3.0
    want_depth, want_xyz = gl.reproject(disp, Q, 0.0)
    assert np.isinf(want_depth[0]).all() and np.isfinite(want_depth[4]).all()
    want_xyz = want_xyz[:, 7:]                                    # x = 6 on a d = 2 row is 0 / 0
    depth, xyz = ops.reproject(dev(disp), Q, 0.0, want=("depth", "xyz"))
    assert host(depth).tobytes() == want_depth.tobytes()
    assert np.ascontiguousarray(host(xyz)[:, 7:]).tobytes() == np.ascontiguousarray(want_xyz).tobytes()


# ----------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e():
    """One matcher, one pair, and the disparity bytes of load_images + match on it and on the pair moved 3 columns."""
    from scenedepthestimation_amd.pipeline import StereoMatcher
    from scenedepthestimation_amd.synthetic import stereo_pair
    H, W, D = 64, 96, 16
    left, right, _ = stereo_pair(H, W, D, seed=3)
    m = StereoMatcher(H, W, D)
    m.load_images(left, right)
    plain = host(m.match()).copy()
    m.load_images(gc.shifted(left, 3), gc.shifted(right, 3))
    moved = host(m.match()).copy()
    assert plain.tobytes() != moved.tobytes()
    return m, left, right, plain, moved


def test_load_raw_identity_calibration(gpu):
    from scenedepthestimation_amd.rectify import Rectifier
    m, left, right, plain, _ = e2e()
    rect = Rectifier(gc.plain_calibration(m.H, m.W))
    m.img_u82.fill_(AA)
    m.load_raw(left, right, rect)
    assert host(m.img_u82).tobytes() == np.stack([left, right]).tobytes()
    assert host(m.match()).tobytes() == plain.tobytes()


def test_load_raw_shifted_calibration_and_depth(gpu):
    from scenedepthestimation_amd.rectify import Rectifier
    m, left, right, _, moved = e2e()
    rect = Rectifier(gc.plain_calibration(m.H, m.W, shift=3))
    want_maps = np.stack([gl.rectify_map(c, m.H, m.W) for c in rect.cal])
    assert host(rect.maps).tobytes() == want_maps.tobytes()
    m.img_u82.fill_(AA)
    m.load_raw(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), rect)      # device tensors too
    assert host(m.img_u82).tobytes() == np.stack([gc.shifted(left, 3), gc.shifted(right, 3)]).tobytes()
    disp = m.match()
    assert host(disp).tobytes() == moved.tobytes()
    want_depth, want_xyz = gl.reproject(moved, rect.Q, 0.0)
    assert (want_depth > 0).any()
    assert host(rect.depth(disp)).tobytes() == want_depth.tobytes()
    assert host(rect.points(disp)).tobytes() == want_xyz.tobytes()
    valid = junk((2, m.H, m.W), torch.uint8)
    rect.remap(m.raw_u82, valid=valid)
    assert not host(valid)[:, :, :3].any() and host(valid)[:, :, 3:].all()
    with pytest.raises(ValueError, match="raw pair"):
        rect.remap(m.raw_u82[:, :-1].contiguous())
    with pytest.raises(ValueError, match="rectifier writes"):
        from scenedepthestimation_amd.pipeline import StereoMatcher
        StereoMatcher(32, 48, 8).load_raw(left, right, rect)


def test_cli_calib_and_depth_out(gpu, tmp_path, monkeypatch):
    """match_single --calib with an identity calibration writes the picture it writes without the flag, and
    --depth-out the restatement's depth of it (the --cpu-path map holds integers, so the PNG is the map)."""
    from scenedepthestimation_amd import imageio, match_single, pfm
    from scenedepthestimation_amd.synthetic import stereo_pair
    H, W, D = 48, 96, 16
    left, right, _ = stereo_pair(H, W, D, seed=9)
    imageio.imwrite(str(tmp_path / "eval" / "left_3.png"), left)
    imageio.imwrite(str(tmp_path / "eval" / "right_3.png"), right)
    cal = gc.plain_calibration(H, W)
    cal.save(tmp_path / "rig.json")
    monkeypatch.chdir(tmp_path)
    common = ["-i", "3", "-g", "0", "--checkpoint", "synthetic", "--cpu-path", "--ndisp", str(D)]
    match_single.main(common)
    plain = imageio.imread_gray(str(tmp_path / "result" / "11_11" / "ld3.png"))
    match_single.main(common + ["-f", "raw", "--calib", "rig.json", "--depth-out", str(tmp_path / "depth.pfm")])
    assert np.array_equal(imageio.imread_gray(str(tmp_path / "result" / "raw" / "ld3.png")), plain)
    depth, _ = pfm.load_pfm(str(tmp_path / "depth.pfm"))
    want, _ = gl.reproject(plain.astype(np.float32), cal.rectify()[4], 0.0)
    assert (want > 0).any() and np.ascontiguousarray(depth[..., 0]).tobytes() == want.tobytes()
