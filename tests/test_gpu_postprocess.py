"""sde_lr_check, sde_lr_consistency, sde_lrc_fill, sde_median5 and sde_wta against the NumPy / Python-float
restatement in post_literal.py, on the case tables of post_cases.py (test_post_host.py checks the restatement against
hand-computed pictures and the C oracle, and that each case is not vacuous).

Every comparison is by bytes (no tolerances).  Output buffers arrive filled with 0xA5 bytes, so nothing depends on
what was there and a byte the kernel must not write is seen to survive.  References are computed once per case.
"""
import functools

import numpy as np
import pytest
import torch

import post_cases as pc
import post_literal as pl

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


def junk_np(shape, dtype=np.float32):
    return np.frombuffer(bytes([A5]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape)


# ----------------------------------------------------------------------------
# left-right check
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lr_check_want(W):
    dl, dr = pc.lr_edge_maps(W)
    init = junk_np(dl.shape, np.uint8)
    a, b, _ = pl.lr_check(dl, dr, init, init)
    return a.tobytes(), b.tobytes()


@pytest.mark.parametrize("W", pc.LR_WIDTHS)
def test_lr_check_never_leaves_the_row(gpu, W):
    """Maps with -1, -0.5, NaN, +-inf, +-1e9 and +-3e38 entries are the middle rows of taller tensors whose guard
    rows (enough to hold any column 0..255 counted from a row start) hold 0, NaN or 1e6.  The flags must not depend
    on the guard rows and must equal the literal's; skipped pixels keep the 0xA5 their buffer came with.  (Before
    the in-row rule the W = 40 and W = 255 cases failed here: a left -1 in column W - 1 read column W, a right -1
    in column 0 read column 255, both in the guard rows or a neighbouring row.)"""
    from scenedepthestimation_amd import ops
    dl, dr = pc.lr_edge_maps(W)
    H = dl.shape[0]
    G = -(-256 // W) + 1
    got = []
    for guard in (0.0, float("nan"), 1e6):
        tl = torch.full((H + 2 * G, W), guard, dtype=torch.float32, device="cuda")
        tr = torch.full((H + 2 * G, W), guard, dtype=torch.float32, device="cuda")
        tl[G:G + H] = dev(dl)
        tr[G:G + H] = dev(dr)
        a, b = junk((H, W), torch.uint8), junk((H, W), torch.uint8)
        ops.lr_check(tl[G:G + H], tr[G:G + H], a, b)
        got.append((host(a).tobytes(), host(b).tobytes()))
        assert host(tl[G:G + H]).tobytes() == dl.tobytes() and host(tr[G:G + H]).tobytes() == dr.tobytes()
    want = lr_check_want(W)
    for guard, g in zip(("0", "nan", "1e6"), got):
        assert g[0] == want[0], ("left", guard)
        assert g[1] == want[1], ("right", guard)
    # the default buffers are zeroed
    a, b = ops.lr_check(dev(dl), dev(dr))
    z = np.zeros((H, W), np.uint8)
    wa, wb, _ = pl.lr_check(dl, dr, z, z)
    assert host(a).tobytes() == wa.tobytes() and host(b).tobytes() == wb.tobytes()


@pytest.mark.parametrize("W", [w for w in pc.LR_WIDTHS if w <= 256])
def test_lr_consistency_equals_lr_check_up_to_256(gpu, W):
    """W <= 256, non-negative maps, max_diff = 1: the two kernels agree (sde_lr_check on zeroed buffers)."""
    from scenedepthestimation_amd import ops
    dl, dr = pc.lr_nonneg_maps(W)
    a, b = ops.lr_check(dev(dl), dev(dr))
    ca, cb = ops.lr_consistency(dev(dl), dev(dr), 1.0, junk(dl.shape, torch.uint8), junk(dl.shape, torch.uint8))
    assert host(a).tobytes() == host(ca).tobytes() and host(b).tobytes() == host(cb).tobytes()
    z = np.zeros(dl.shape, np.uint8)
    wa, wb, _ = pl.lr_check(dl, dr, z, z)
    assert host(a).tobytes() == wa.tobytes() and host(b).tobytes() == wb.tobytes()


@pytest.mark.parametrize("max_diff", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("W", pc.LR_WIDTHS)
def test_lr_consistency_edge_maps(gpu, W, max_diff):
    """The same maps, non-finite entries included; every pixel is written."""
    from scenedepthestimation_amd import ops
    dl, dr = pc.lr_edge_maps(W)
    a, b = ops.lr_consistency(dev(dl), dev(dr), max_diff, junk(dl.shape, torch.uint8), junk(dl.shape, torch.uint8))
    wa, wb = pl.lr_consistency(dl, dr, max_diff)
    assert host(a).tobytes() == wa.tobytes() and host(b).tobytes() == wb.tobytes()


# ----------------------------------------------------------------------------
# LRC fill
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("frac", pc.FILL_FRACS)
@pytest.mark.parametrize("H,W", pc.FILL_SHAPES)
def test_lrc_fill_edge_shapes(gpu, H, W, frac):
    """One pixel, one row, one column, shapes one off the 64-lane chunk both ways, more than two chunks; flag bytes
    from {0, 1, 2, 255} (only 1 is flagged); NaN and +inf among the neighbours."""
    from scenedepthestimation_amd import ops
    dl, flags = pc.fill_case(H, W, frac)
    got = host(ops.lrc_fill(dev(dl), dev(flags), junk((H, W))))
    assert got.tobytes() == pl.lrc_fill(dl, flags).tobytes()


@pytest.mark.parametrize("W", pc.FILL_WIDE)
def test_lrc_fill_lds_boundary(gpu, W):
    """2 B of LDS per column: 64 KiB exactly, the first width that needs the opt-in allocation, and the widest
    accepted; a 5000-column flagged run and a fully flagged row."""
    from scenedepthestimation_amd import ops
    dl, flags = pc.fill_wide_case(W)
    got = host(ops.lrc_fill(dev(dl), dev(flags), junk(dl.shape)))
    assert got.tobytes() == pl.lrc_fill(dl, flags).tobytes()


def test_lrc_fill_refusals(gpu):
    """H or W = 65535 (the 16-bit "none") and out == disp_l are refused on the host: nothing is written."""
    from scenedepthestimation_amd import ops
    from scenedepthestimation_amd._lib import SdeError
    for H, W in ((65535, 1), (1, 65535)):
        dl, flags, out = dev(np.ones((H, W), np.float32)), dev(np.ones((H, W), np.uint8)), junk((H, W))
        with pytest.raises(SdeError):
            ops.lrc_fill(dl, flags, out)
        assert host(out).tobytes() == junk_np((H, W)).tobytes()
    dl, flags = pc.fill_case(63, 64, 0.3)
    t = dev(dl)
    with pytest.raises(SdeError):
        ops.lrc_fill(t, dev(flags), t)
    assert host(t).tobytes() == dl.tobytes()


# ----------------------------------------------------------------------------
# 5x5 median
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.MEDIAN_KINDS)
@pytest.mark.parametrize("H,W", pc.MEDIAN_SHAPES)
def test_median5_edge_shapes(gpu, H, W, kind):
    """No interior (dst untouched, no error), a single window, one interior row / column, more than one 16 x 16
    block each way; ties, signed zeros, NaN, +-inf, an all-NaN window.  The whole dst is compared, so the 2-pixel
    border keeps its 0xA5."""
    from scenedepthestimation_amd import ops
    src = pc.median_case(H, W, kind)
    dst = junk((H, W))
    ops.median5(dev(src), dst)
    want = pl.median5(src, junk_np((H, W)))
    if H < 5 or W < 5:
        assert want.tobytes() == junk_np((H, W)).tobytes()
    assert host(dst).tobytes() == want.tobytes()


# ----------------------------------------------------------------------------
# stored-volume WTA
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wta_want(H, W, D, kind, rule):
    return pl.wta(pc.wta_case(H, W, D, kind), "HWD", rule).tobytes()


@pytest.mark.parametrize("H,W", pc.WTA_PIXELS)
@pytest.mark.parametrize("D", pc.WTA_D)
@pytest.mark.parametrize("rule", ["inf", "d0"])
@pytest.mark.parametrize("layout", ["DHW", "HWD"])
def test_wta_edge_volumes(gpu, layout, rule, D, H, W):
    """Both layouts and rules; D around the HWD kernel's 16 lanes per pixel; pixel counts that leave idle lanes in
    the last block and a last wave with fewer than 4 pixels.  Tie-heavy integers (the first minimum wins across
    lanes), all +inf, NaN at d = 0 and elsewhere, +-inf, a row of all NaN."""
    from scenedepthestimation_amd import ops
    for kind in pc.WTA_KINDS:
        vol = pc.as_layout(pc.wta_case(H, W, D, kind), layout)
        got = host(ops.wta(dev(vol), layout, rule, junk((H, W))))
        assert got.tobytes() == wta_want(H, W, D, kind, rule), kind
