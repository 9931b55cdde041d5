"""GPU: the cross-based aggregation kernels (csrc/cbca.hip) at the arm lengths, line lengths, volumes and scratch
contents at which their ring, block schedule and persistent grids take every path, bit for bit.

What each test is for is read off the kernels: three templates (R = 13, 15, 31 for L1 <= 14, <= 16, <= 32), per
wave a ring of 2R + 2 prefixes trailed by R + 1 positions, blocks of 2R + 2 positions (two peeled, a loop of two per
iteration, clamped tail blocks; an unclamped block needs a line of 4R + 4 positions), chains that restart every 256
positions after an M = L1 - 1 pre-roll, and grids that hand a wave several items once there are more items than
resident waves.  The expected values are the oracle's (oracle/sde_oracle.c, pinned to a literal restatement by
test_oracle_cbca.py), the closed form cbca_cases.box_expected, or the input itself; every comparison is exact.
The inputs are in cbca_cases.py; every case on plateau images first asserts which arm lengths it reaches.
"""
import os

import numpy as np
import pytest
import torch

import cbca_cases as cc

pytestmark = pytest.mark.gpu

I32 = np.int32


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()      # the case tables are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def oracle_threads(oracle):
    n = oracle.get_threads()
    oracle.set_threads(min(16, os.cpu_count() or 1))
    yield
    oracle.set_threads(n)


_ARMS = {}


def plateau_arms(oracle, H, W, L1, axis):
    """The oracle's arms of the plateau images of (H, W, L1 - 1), after the coverage condition along `axis`."""
    if (H, W, L1) not in _ARMS:
        il, ir = cc.plateau_images(H, W, L1 - 1)
        _ARMS[H, W, L1] = cc._frozen(oracle.cbca_arms(il, L1, cc.TAU), oracle.cbca_arms(ir, L1, cc.TAU))
    al, ar = _ARMS[H, W, L1]
    assert cc.line_covered(al, ar, axis, L1 - 1), ("arm coverage", H, W, L1, axis)
    return al, ar


def run_cbca(cv, al, ar, side, L1, iters, **scratch):
    """ops.cbca on a copy of cv; al / ar: the left / right image's arms."""
    from scenedepthestimation_amd import ops
    ref, oth = (al, ar) if side == "left" else (ar, al)
    got = dev(cv)
    ops.cbca(got, dev(ref.view(I32)), dev(oth.view(I32)), side, L1, iters, **scratch)
    return host(got)


def want_cbca(oracle, cv, al, ar, side, L1, iters):
    ref, oth = (al, ar) if side == "left" else (ar, al)
    return oracle.cbca(cv, ref, oth, side, iters, L1=L1)


def diff(got, want):
    """Where two volumes differ, for an assertion message."""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return f"{len(bad)} voxels differ, first (y, x, d) = {tuple(bad[0]) if len(bad) else None}"


# ----------------------------------------------------------------------------
# 1. line-length sweep
# ----------------------------------------------------------------------------
def sweep_case(oracle, L1, axis, side, N):
    H, W, D = cc.sweep_shape(axis, N)
    al, ar = plateau_arms(oracle, H, W, L1, axis)
    cv = cc.sweep_costs(axis, N, side)
    return cv, al, ar, want_cbca(oracle, cv, al, ar, side, L1, 1)


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("axis", ["h", "v"])
@pytest.mark.parametrize("L1", cc.SWEEP_L1)
def test_cbca_line_length_sweep(gpu, oracle, L1, axis, side):
    """Lines of every length in cbca_cases.SWEEP_N along the rows (5 x N x 70) or the columns (N x 70 x 70), with
    arms of every length up to L1 - 1: between them the lengths take every block schedule of the three templates
    (no unclamped block, one, two, the loop left by either exit, each tail-block count, one to three segments, a
    last segment of one position at 257 and 513).  side = right also runs both rotations."""
    failed = []
    for N in cc.SWEEP_N:
        cv, al, ar, want = sweep_case(oracle, L1, axis, side, N)
        got = run_cbca(cv, al, ar, side, L1, 1)
        if got.tobytes() != want.tobytes():
            failed.append(f"N = {N}: {diff(got, want)}")
    assert not failed, "; ".join(failed)


# ----------------------------------------------------------------------------
# 2. deep D in late segments
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("H,W,D,L1", [(3, 300, 330, 14), (3, 400, 330, 14), (3, 560, 330, 14), (3, 300, 330, 32),
                                      (3, 400, 330, 32), (3, 560, 330, 32), (6, 130, 512, 14)])
def test_cbca_deep_disparities(gpu, oracle, H, W, D, L1, side):
    """D = 330 on rows of two and three segments: chunks whose lanes' chains start inside a late segment's walk,
    chunks past the segment's end (no work), and disparities past the row's width; D = 512 on 130 columns: all 8
    chunks, the low columns of the vertical pass with fewer chunks than the rest.  Two iterations."""
    al, ar = plateau_arms(oracle, H, W, L1, "h")
    rng = np.random.default_rng(H * W + D + L1)
    cv = (rng.standard_normal((H, W, D)) * 3 + 20).astype(np.float32)
    if side == "left":
        cc.fill_invalid(cv)
    want = want_cbca(oracle, cv, al, ar, side, L1, 2)
    got = run_cbca(cv, al, ar, side, L1, 2)
    assert got.tobytes() == want.tobytes(), diff(got, want)


# ----------------------------------------------------------------------------
# 3. box-filter identity
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D,L1", cc.BOX_CASES)
def test_cbca_box_filter_identity(gpu, oracle, H, W, D, L1):
    """A flat image (every arm reaches min(L1 - 1, distance to the border)) and integer costs: the result is the
    closed form cbca_cases.box_expected, which owes nothing to the oracle or to where chains restart.  Interior
    pixels have the largest counts there are ((2 L1 - 1)^2 = 729 at L1 = 14, 3969 at L1 = 32).  sde_cbca_lr writes
    the shear of that result into the right volume's valid voxels and leaves the rest."""
    from scenedepthestimation_amd import ops
    cv, want = cc.box_case(H, W, D, L1)
    arms = oracle.cbca_arms(np.zeros((H, W), np.float32), L1, 1.0)
    M = L1 - 1
    assert int((arms & 255).max()) == min(M, W - 1) and int((arms >> 24).max()) == min(M, H - 1)
    got = run_cbca(cv, arms, arms, "left", L1, 1)
    assert got.tobytes() == want.tobytes(), diff(got, want)
    junk = np.full((H, W, D), -7.5, np.float32)
    gl, gr, a = dev(cv), dev(junk), dev(arms.view(I32))
    ops.cbca_lr(gl, gr, a, a, L1, 1)
    assert host(gl).tobytes() == want.tobytes()
    want_r = cc.shear(want, junk)
    assert host(gr).tobytes() == want_r.tobytes(), diff(host(gr), want_r)


# ----------------------------------------------------------------------------
# 4. non-finite costs
# ----------------------------------------------------------------------------
def nonfinite_case(oracle, H, W, D, L1, side):
    al, ar = plateau_arms(oracle, H, W, L1, "h" if W >= H else "v")
    cl, rows = cc.nonfinite_volume(H, W, D)
    return (cl if side == "left" else cc.to_right(cl)), al, ar, rows


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("L1", [14, 32])
@pytest.mark.parametrize("H,W,D", cc.NONFINITE_SHAPES)
def test_cbca_nonfinite_vs_oracle(gpu, oracle, H, W, D, L1, iters, side):
    """A NaN poisons its fp64 chain from its own position to the end of that segment's chain and nothing else: the
    per-lane select of the chain start, the clamped prefetch past the line's end and the out-of-range loads must
    neither drop nor spread it (cbca_cases.nonfinite_volume lists the poisoned voxels)."""
    cv, al, ar, rows = nonfinite_case(oracle, H, W, D, L1, side)
    want = want_cbca(oracle, cv, al, ar, side, L1, iters)
    assert np.isnan(want).any() and np.isfinite(want).any()
    got = run_cbca(cv, al, ar, side, L1, iters)
    assert cc.same_f32(got, want)
    if iters == 1:      # the footprint is bounded: a row that no support connects to a poisoned voxel
        assert all(np.isfinite(cv[y]).all() for y in rows)
        clean = [y for y in rows if np.isfinite(want[y]).all()]
        assert clean and all(np.isfinite(got[y]).all() for y in clean)


@pytest.mark.parametrize("L1", [14, 32])
@pytest.mark.parametrize("H,W,D", cc.NONFINITE_SHAPES)
def test_cbca_lr_nonfinite_vs_oracle(gpu, oracle, H, W, D, L1):
    from scenedepthestimation_amd import ops
    cl, al, ar, _ = nonfinite_case(oracle, H, W, D, L1, "left")
    junk = np.full((H, W, D), -7.5, np.float32)
    want_l, want_r = oracle.cbca_lr(cl, junk, al, ar, 2, L1=L1)
    assert np.isnan(want_r).any() and np.isfinite(want_r).any()
    gl, gr = dev(cl), dev(junk)
    ops.cbca_lr(gl, gr, dev(al.view(I32)), dev(ar.view(I32)), L1, 2)
    assert cc.same_f32(host(gl), want_l) and cc.same_f32(host(gr), want_r)


# ----------------------------------------------------------------------------
# 5. scratch independence
# ----------------------------------------------------------------------------
def _scratch(cv, extra=0):
    """tmp full of NaN and a workspace of 0xFF bytes, `extra` bytes longer than required."""
    from scenedepthestimation_amd import ops
    H, W, _ = cv.shape
    return {"tmp": torch.full(cv.shape, float("nan"), device="cuda"),
            "workspace": torch.full((ops.cbca_workspace_bytes(H, W) + extra,), 0xFF, dtype=torch.uint8, device="cuda")}


@pytest.mark.parametrize("which", ["sweep", "nonfinite"])
def test_cbca_scratch_contents_do_not_matter(gpu, oracle, which):
    """tmp and the workspace are outputs of the first kernels that touch them: a NaN-filled tmp, a workspace of
    0xFF bytes (arms of 255 wherever one is read unwritten) and a workspace longer than required change nothing."""
    if which == "sweep":
        L1, side, iters = 16, "left", 1
        cv, al, ar, want = sweep_case(oracle, L1, "v", side, 314)
    else:
        L1, side, iters = 32, "right", 2
        cv, al, ar, _ = nonfinite_case(oracle, 9, 300, 70, L1, side)
        want = want_cbca(oracle, cv, al, ar, side, L1, iters)
    assert cc.same_f32(run_cbca(cv, al, ar, side, L1, iters), want)
    assert cc.same_f32(run_cbca(cv, al, ar, side, L1, iters, **_scratch(cv)), want)
    assert cc.same_f32(run_cbca(cv, al, ar, side, L1, iters, **_scratch(cv, extra=64)), want)


def test_cbca_pair_scratch_contents_do_not_matter(gpu, oracle):
    from scenedepthestimation_amd import ops
    L1 = 16
    cl, al, ar, want_l = sweep_case(oracle, L1, "v", "left", 314)
    cr = cc.sweep_costs("v", 314, "right")
    want_r = want_cbca(oracle, cr, al, ar, "right", L1, 1)
    gl, gr = dev(cl), dev(cr)
    s = _scratch(cl)
    ops.cbca_pair(gl, gr, dev(al.view(I32)), dev(ar.view(I32)), L1, 1, tmp_l=s["tmp"], tmp_r=s["tmp"].clone(),
                  workspace=s["workspace"])
    assert host(gl).tobytes() == want_l.tobytes() and host(gr).tobytes() == want_r.tobytes()


# ----------------------------------------------------------------------------
# 6. more items than resident waves
# ----------------------------------------------------------------------------
LDS_PER_CU = 160 * 1024


def _wave_bound(R, kernel, cus):
    """An upper bound on the resident waves of a pass kernel: per CU, the workgroups whose static LDS fits (the
    __shared__ arrays of cbca_h_kernel / cbca_v_kernel: fp64 prefix ring, u16 count ring, fp64 reciprocal table)
    times the waves of a workgroup.  Registers can only lower the true number."""
    RS = 2 * R + 2
    if kernel == "h":
        return cus * (LDS_PER_CU // (RS * 64 * 8))
    wpb, table = (4, (2 * R + 1) ** 2 + 1) if R == 13 else (1, 1)
    return cus * (LDS_PER_CU // (wpb * RS * 64 * (8 + 2) + 8 * table)) * wpb


@pytest.mark.parametrize("kernel", ["h", "v"])
@pytest.mark.parametrize("R,L1", [(13, 14), (15, 16), (31, 32)])
def test_cbca_second_item_per_wave(gpu, oracle, R, L1, kernel):
    """At least twice as many items as waves can be resident, so every wave of the pass under test takes a second
    item on a ring that still holds the first one's prefixes and counts (only one slot is seeded per item)."""
    D, ndc = 256, 4
    bound = _wave_bound(R, kernel, torch.cuda.get_device_properties(0).multi_processor_count)
    if kernel == "h":                      # items = segments x rows x chunks
        H, W = -(-2 * bound // ndc), 40
        items = 1 * H * ndc
    else:                                  # items = segments x sum over chunks c of the columns x >= 64 c
        H, W = 8, -(-(2 * bound + 384) // ndc)
        items = 1 * sum(max(W - 64 * c, 0) for c in range(ndc))
    assert items >= 2 * bound and H * W * D * 4 <= 60e6, (H, W, items, bound)
    al, ar = plateau_arms(oracle, H, W, L1, kernel)
    rng = np.random.default_rng(R)
    cv = cc.fill_invalid((rng.standard_normal((H, W, D)) * 3 + 20).astype(np.float32))
    want = want_cbca(oracle, cv, al, ar, "left", L1, 1)
    got = run_cbca(cv, al, ar, "left", L1, 1)
    assert got.tobytes() == want.tobytes(), diff(got, want)


# ----------------------------------------------------------------------------
# 7. rotations in isolation
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 130])
def test_cbca_rotations_alone(gpu, W):
    """Zero arms: every support is the voxel itself and the fp64 differences of small integers are exact, so a
    right volume comes back from rotation, aggregation and rotation unchanged, and sde_cbca_lr writes exactly the
    shear.  Row widths around the 64-pixel tile, D around the 64-disparity tile and D > W (rows that wrap many
    times)."""
    from scenedepthestimation_amd import ops
    H = 2
    arms = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    y, x = np.arange(H).reshape(H, 1, 1), np.arange(W).reshape(1, W, 1)
    for D in (1, 63, 64, 65, 129, 512):
        d = np.arange(D).reshape(1, 1, D)
        cl = ((7 * y + 3 * x + d) % 13).astype(np.float32)
        cr = ((5 * y + 11 * x + 2 * d) % 17).astype(np.float32)
        got = dev(cl)
        ops.cbca(got, arms, arms, "right", 14, 1)
        assert host(got).tobytes() == cl.tobytes(), f"D = {D}: {diff(host(got), cl)}"
        want_r = cc.shear(cl, cr)
        for iters in (0, 1):
            gl, gr = dev(cl), dev(cr)
            ops.cbca_lr(gl, gr, arms, arms, 14, iters)
            assert host(gl).tobytes() == cl.tobytes(), f"D = {D}, iters = {iters}"
            assert host(gr).tobytes() == want_r.tobytes(), f"D = {D}, iters = {iters}: {diff(host(gr), want_r)}"


# ----------------------------------------------------------------------------
# 8. arms kernel
# ----------------------------------------------------------------------------
def gpu_arms(img, L1, tau):
    from scenedepthestimation_amd import ops
    return host(ops.cbca_arms(dev(np.asarray(img, np.float32)), L1, tau)).view(np.uint32)


def pack(l, r, u, d):
    return (np.asarray(l) | np.asarray(r) << 8 | np.asarray(u) << 16 | np.asarray(d) << 24).astype(np.uint32)


def border_arms(H, W, M):
    """Arms of an image where only the border and M stop an arm."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return pack(np.minimum(M, x + 0 * y), np.minimum(M, W - 1 - x + 0 * y), np.minimum(M, y + 0 * x),
                np.minimum(M, H - 1 - y + 0 * x))


@pytest.mark.parametrize("L1", [1, 2, 32])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (3, 300), (17, 257)])
def test_cbca_arms_shapes(gpu, oracle, H, W, L1):
    want, _ = plateau_arms(oracle, H, W, L1, "h" if W >= H else "v")
    img, _ = cc.plateau_images(H, W, L1 - 1)
    assert np.array_equal(gpu_arms(img, L1, cc.TAU), want)
    if H == W == 1:
        assert want.tolist() == [[0]]
    flat = np.full((H, W), 0.5, np.float32)
    assert np.array_equal(gpu_arms(flat, L1, 1.0), border_arms(H, W, L1 - 1))


def test_cbca_arms_threshold_is_strict(gpu, oracle):
    """|difference| == tau stops an arm (the comparison is <), one ulp more does not; differences are taken from
    the centre pixel, so a step of 0.25 per pixel lets an arm grow by one pixel only."""
    row = np.array([[0, .25, .5, .75]], np.float32)
    assert gpu_arms(row, 32, 0.25).tolist() == [[0, 0, 0, 0]]
    up = float(np.nextafter(np.float32(0.25), np.float32(1)))
    want = pack([0, 1, 1, 1], [1, 1, 1, 0], 0, 0).reshape(1, 4)
    assert np.array_equal(gpu_arms(row, 32, up), want)
    assert np.array_equal(oracle.cbca_arms(row, 32, 0.25), np.zeros((1, 4), np.uint32))
    assert np.array_equal(oracle.cbca_arms(row, 32, up), want)


@pytest.mark.parametrize("tau,full", [(0.0, False), (-1.0, False), (float("inf"), True), (float("nan"), False)])
def test_cbca_arms_degenerate_tau(gpu, oracle, tau, full):
    """On a flat image every difference is 0: 0 < tau fails for tau <= 0 and for NaN, holds for +inf."""
    flat = np.full((5, 40), 0.5, np.float32)
    want = border_arms(5, 40, 31) if full else np.zeros((5, 40), np.uint32)
    assert np.array_equal(gpu_arms(flat, 32, tau), want)
    assert np.array_equal(oracle.cbca_arms(flat, 32, tau), want)


def test_cbca_arms_nonfinite_pixels(gpu, oracle):
    """A NaN pixel and a +inf pixel stop every arm that meets them and have none of their own; three rows of the
    same pattern, so the vertical arms of the +inf column compare inf with inf (inf - inf is NaN: no arm)."""
    row = np.array([0, 0, 0, np.nan, 0, 0, np.inf, 0, 0], np.float32)
    img = np.stack([row, row, row])
    l, r = [0, 1, 2, 0, 0, 1, 0, 0, 1], [2, 1, 0, 0, 1, 0, 0, 1, 0]
    ok = np.isfinite(row)
    want = np.stack([pack(l, r, np.where(ok, y, 0), np.where(ok, 2 - y, 0)) for y in range(3)])
    assert np.array_equal(gpu_arms(img, 32, 1.0), want)
    assert np.array_equal(oracle.cbca_arms(img, 32, 1.0), want)


def test_cbca_arms_border_cut(gpu, oracle):
    """A flat 5 x 40 image at L1 = 32: every arm is min(31, distance to the border)."""
    flat = np.zeros((5, 40), np.float32)
    want = border_arms(5, 40, 31)
    assert int((want & 255).max()) == 31 and int((want >> 24).max()) == 4
    assert np.array_equal(gpu_arms(flat, 32, 0.5), want)
    assert np.array_equal(oracle.cbca_arms(flat, 32, 0.5), want)


@pytest.mark.parametrize("H,W,L1", [(37, 70, 32), (1, 70, 14)])
def test_cbca_arms_strided_views(gpu, oracle, H, W, L1):
    """A row-strided interior view of a padded image (pitch > W), also of a single row; the padding holds the
    value of the plateau beside it, so an arm that ignored the view's edge would run on into it."""
    from scenedepthestimation_amd import ops
    want, _ = plateau_arms(oracle, H, W, L1, "h")
    img, _ = cc.plateau_images(H, W, L1 - 1)
    pad = np.pad(img, 5, mode="edge")
    view = dev(pad)[5:5 + H, 5:5 + W]
    assert view.stride(0) == W + 10
    got = host(ops.cbca_arms(view, L1, cc.TAU)).view(np.uint32)
    assert np.array_equal(got, want)
