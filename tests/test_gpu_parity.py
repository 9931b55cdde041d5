"""GPU parity: libsde.so kernels (through the C ABI) vs the oracle and the golden vectors.

Bar: bit-exact for cost volumes, argmin maps, penalties, SGM S volumes and
post-processing; tower features within 1e-4 of the fp64 restatement.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def l2n(x):
    return (x / np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(-1, keepdims=True)), 1e-12)).astype(np.float32)


# ----------------------------------------------------------------------------
# cost volume / WTA against the reference's golden vectors
# ----------------------------------------------------------------------------
def test_golden_cost_volume_dhw(gpu, golden, golden_cases):
    from scenedepthestimation_amd import ops
    for n in golden_cases:
        fl, fr, d = golden[n + "__fl"], golden[n + "__fr"], int(golden[n + "__ndisp"])
        cv = host(ops.cost_volume(dev(fl), dev(fr), d, layout="DHW"))
        assert cv.tobytes() == golden[n + "__cv"].tobytes(), n


def test_golden_fused_cv_wta(gpu, golden, golden_cases):
    from scenedepthestimation_amd import ops
    for n in golden_cases:
        fl, fr, d = golden[n + "__fl"], golden[n + "__fr"], int(golden[n + "__ndisp"])
        disp, mn, am = ops.cv_wta(dev(fl), dev(fr), 0, d, want=("disp", "min", "argmin"))
        assert np.array_equal(host(disp), golden[n + "__disp"]), n
        assert np.array_equal(host(am).astype(np.float32), golden[n + "__disp"]), n


def test_golden_wta_variants(gpu, golden, golden_cases):
    from scenedepthestimation_amd import ops
    assert np.array_equal(host(ops.wta(dev(golden["wta_hwd__vol"]), "HWD")), golden["wta_hwd__disp"])
    assert np.array_equal(host(ops.wta(dev(golden["wta_dhw__vol"]), "DHW")), golden["wta_dhw__disp"])
    for n in golden_cases:
        cv = golden[n + "__cv"]
        assert np.array_equal(host(ops.wta(dev(cv), "DHW")), golden[n + "__disp"]), n
        hwd = np.ascontiguousarray(cv.transpose(1, 2, 0))
        assert np.array_equal(host(ops.wta(dev(hwd), "HWD")), golden[n + "__disp"]), n


def test_process_functional_api(gpu, golden, golden_cases):
    from scenedepthestimation_amd import process_functional as pf
    for n in golden_cases[:8]:
        fl, fr, d = golden[n + "__fl"], golden[n + "__fr"], int(golden[n + "__ndisp"])
        cv = pf.compute_cost_volume(fl, fr, d)
        assert cv.dtype == np.float32 and cv.tobytes() == golden[n + "__cv"].tobytes()
        assert np.array_equal(pf.WTA1(cv), golden[n + "__disp"])
        assert np.array_equal(pf.WTA(np.ascontiguousarray(cv.transpose(1, 2, 0))), golden[n + "__disp"])
    vol = np.full((2, 3, 4), np.inf, np.float32)
    with pytest.raises(AssertionError):          # the reference asserts min_disparity >= 0
        pf.WTA(vol)


# ----------------------------------------------------------------------------
# larger seeded sizes vs the C oracle
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,D", [(3, 200, 64), (2, 333, 192), (2, 130, 256), (1, 700, 128), (2, 96, 100)])
def test_cv_wta_vs_oracle(gpu, oracle, H, W, D):
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(H * W + D)
    fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    ref = oracle.WTA1(oracle.compute_cost_volume(fl, fr, D))
    disp, mn, am = ops.cv_wta(dev(fl), dev(fr), 0, D, want=("disp", "min", "argmin"))
    assert np.array_equal(host(disp), ref)
    omn, oam = oracle.cv_wta_shard(fl, fr, 0, D)
    assert host(mn).tobytes() == omn.tobytes()
    cv = host(ops.cost_volume(dev(fl), dev(fr), D, layout="DHW"))
    assert cv.tobytes() == oracle.compute_cost_volume(fl, fr, D).tobytes()


@pytest.mark.parametrize("nshards", [2, 3, 8])
def test_disparity_shards_merge_bit_exact(gpu, oracle, nshards):
    from scenedepthestimation_amd import ops
    from scenedepthestimation_amd.parallel import shard_range
    rng = np.random.default_rng(nshards)
    H, W, D = 4, 260, 192
    fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr[:, 100:140] = fr[:, 60:100]            # repeated texture -> exact cost ties across shards
    ref = oracle.WTA1(oracle.compute_cost_volume(fl, fr, D))
    mins = torch.empty((nshards, H, W), dtype=torch.float32, device="cuda")
    args = torch.empty((nshards, H, W), dtype=torch.int32, device="cuda")
    for s in range(nshards):
        d0, d1 = shard_range(D, nshards, s)
        ops.cv_wta(dev(fl), dev(fr), d0, d1, min_cost=mins[s], argmin=args[s], want=(),
                   mode="certified" if s % 2 else "exact")
    assert np.array_equal(host(ops.argmin_merge(mins, args)), ref)


def test_hwd_volumes_vs_oracle(gpu, oracle):
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(11)
    for (H, W, D) in [(3, 90, 64), (2, 70, 128), (2, 40, 100), (4, 300, 192), (2, 130, 200), (3, 64, 1),
                      (2, 1, 5), (2, 5, 64), (2, 128, 67), (1, 200, 130), (2, 63, 250), (1, 257, 190),
                      (1, 600, 512), (2, 129, 64), (1, 385, 192), (1, 127, 65), (1, 1100, 2)]:
        fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
        fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
        # one row sweep writes both; NaN-filled outputs catch any voxel it leaves unwritten
        L = torch.full((H, W, D), float("nan"), device="cuda")
        R = torch.full((H, W, D), float("nan"), device="cuda")
        ops.cost_volume(dev(fl), dev(fr), D, layout="HWD", right=True, invalid=1.0, out_left=L, out_right=R)
        oL, oR = oracle.cost_volume_hwd(fl, fr, D, invalid=1.0)
        assert host(L).tobytes() == oL.tobytes()
        assert host(R).tobytes() == oR.tobytes()
        R1 = torch.full((H, W, D), float("nan"), device="cuda")     # right side alone (its own kernel)
        ops.cost_volume(dev(fl), dev(fr), D, layout="HWD", right=True, left=False, invalid=1.0, out_right=R1)
        assert host(R1).tobytes() == oR.tobytes()
        L1 = torch.full((H, W, D), float("nan"), device="cuda")     # left side alone (the sweep, no R stores)
        ops.cost_volume(dev(fl), dev(fr), D, layout="HWD", invalid=1.0, out_left=L1)
        assert host(L1).tobytes() == oL.tobytes()


def test_hwd_volumes_nonfinite_features(gpu, oracle):
    """The L/R volume kernel on features holding inf / -inf / NaN (process_functional.py:120-131 takes
    whatever compute_feature returns): NaN exactly where the oracle has NaN, every other voxel
    bit-exact, across strip and chunk boundaries."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(21)
    H, W, D = 3, 300, 192
    fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fl[0, 10, 5] = np.inf
    fl[1, 127, 0] = np.nan
    fl[2, 128, 63] = -np.inf
    fr[2, 200, 63] = -np.inf
    fr[0, 5, 7] = np.nan
    fr[1, 64, 9] = np.inf
    L = torch.full((H, W, D), float("nan"), device="cuda")
    R = torch.full((H, W, D), float("nan"), device="cuda")
    ops.cost_volume(dev(fl), dev(fr), D, layout="HWD", right=True, invalid=1.0, out_left=L, out_right=R)
    oL, oR = oracle.cost_volume_hwd(fl, fr, D, invalid=1.0)
    for a, b in ((host(L), oL), (host(R), oR)):
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb)
        assert na.any() and np.isinf(b).any()
        assert a[~na].tobytes() == b[~nb].tobytes()


def test_generic_channel_counts(gpu, golden, golden_cases):
    """C != 64 takes the generic kernel (full NumPy pairwise recursion)."""
    from scenedepthestimation_amd import ops
    for n in [c for c in golden_cases if c.startswith("chan")]:
        fl, fr, d = golden[n + "__fl"], golden[n + "__fr"], int(golden[n + "__ndisp"])
        assert host(ops.cost_volume(dev(fl), dev(fr), d)).tobytes() == golden[n + "__cv"].tobytes(), n
        disp, _, _ = ops.cv_wta(dev(fl), dev(fr), 0, d)
        assert np.array_equal(host(disp), golden[n + "__disp"]), n


@pytest.mark.parametrize("H,W,D", [(2, 37, 9), (1, 5, 9)])
@pytest.mark.parametrize("C", [5, 24, 130])
def test_generic_hwd_volumes_vs_oracle(gpu, oracle, C, H, W, D):
    """C != 64 in the [H,W,D] layout (cv_generic_kernel<OUT_HWD>): both volumes together, the left alone and the
    right alone, byte-equal to the oracle.  C = 5 is below one 8-block, 24 the <= 128 loop, 130 the recursion;
    W is no multiple of anything and (1, 5, 9) has D > W.  NaN-filled outputs catch any voxel left unwritten."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(1000 * C + W)
    fl = l2n(rng.standard_normal((H, W, C)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, C)).astype(np.float32))
    oL, oR = oracle.cost_volume_hwd(fl, fr, D, invalid=1.0)

    def nan():
        return torch.full((H, W, D), float("nan"), device="cuda")
    L, R, L1, R1 = nan(), nan(), nan(), nan()
    ops.cost_volume(dev(fl), dev(fr), D, layout="HWD", right=True, invalid=1.0, out_left=L, out_right=R)
    assert host(L).tobytes() == oL.tobytes()
    assert host(R).tobytes() == oR.tobytes()
    ops.cost_volume(dev(fl), dev(fr), D, layout="HWD", invalid=1.0, out_left=L1)
    assert host(L1).tobytes() == oL.tobytes()
    ops.cost_volume(dev(fl), dev(fr), D, layout="HWD", right=True, left=False, invalid=1.0, out_right=R1)
    assert host(R1).tobytes() == oR.tobytes()


# ----------------------------------------------------------------------------
# tower
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x3", "f16x3w", "f16x3m32"])
@pytest.mark.parametrize("nlayers,H,W", [(5, 20, 37), (5, 41, 70), (3, 17, 33), (2, 9, 40), (1, 6, 7)])
def test_tower_vs_oracle(gpu, oracle, nlayers, H, W, precision):
    from scenedepthestimation_amd import mc_cnn, ops
    rng = np.random.default_rng(nlayers * 1000 + H)
    w = mc_cnn.synthetic_weights(nlayers, seed=nlayers)
    hw, hb = mc_cnn.layer_lists(w, nlayers)
    img = np.zeros((H + 2 * nlayers, W + 2 * nlayers), np.float32)
    img[nlayers:-nlayers, nlayers:-nlayers] = rng.standard_normal((H, W)).astype(np.float32)
    ref = oracle.tower_forward(img, hw, hb)
    packed = dev(ops.pack_tower_weights(hw, hb))
    out = host(ops.tower_forward(dev(img), packed, nlayers, precision=precision))
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() < 1e-4


def test_tower_precision_report(gpu, oracle):
    """Both tower arithmetics stay at fp32-level error vs the fp64 restatement (printed for the record)."""
    from scenedepthestimation_amd import mc_cnn, ops
    rng = np.random.default_rng(77)
    H, W, L = 64, 96, 5
    w = mc_cnn.synthetic_weights(L)
    hw, hb = mc_cnn.layer_lists(w, L)
    img = np.zeros((H + 2 * L, W + 2 * L), np.float32)
    img[L:-L, L:-L] = rng.standard_normal((H, W)).astype(np.float32)
    ref = oracle.tower_forward(img, hw, hb)
    packed = dev(ops.pack_tower_weights(hw, hb))
    errs = {}
    for prec in ("fp32", "bf16x6", "f16x3", "f16x3w", "f16x3m32"):
        out = host(ops.tower_forward(dev(img), packed, L, precision=prec))
        errs[prec] = float(np.abs(out - ref).max())
    print("tower max abs err vs fp64:", errs)
    assert all(e < 1e-5 for e in errs.values()), errs


@pytest.mark.parametrize("precision", ["f16x3", "f16x3w", "f16x3m32"])
@pytest.mark.parametrize("scale", [1e-6, 1e-3, 1e3, 1e12])
def test_tower_f16x3_dynamic_range(gpu, oracle, scale, precision):
    """f16x3 scales operands by powers of two from device bound words: an image and weights far
    outside fp16's range (tiny or huge) keep fp32-level accuracy (relative to the fp64 tower) and
    never overflow.  The last layer L2-normalises, so the features are scale-free."""
    from scenedepthestimation_amd import mc_cnn, ops
    rng = np.random.default_rng(5)
    H, W, L = 24, 70, 5
    w = mc_cnn.synthetic_weights(L, seed=9)
    hw, hb = mc_cnn.layer_lists(w, L)
    hw = [x * np.float32(scale ** (1 / L)) for x in hw]
    hb = [x * np.float32(scale ** ((k + 1) / L)) for k, x in enumerate(hb)]
    img = np.zeros((H + 2 * L, W + 2 * L), np.float32)
    img[L:-L, L:-L] = rng.standard_normal((H, W)).astype(np.float32)
    ref = oracle.tower_forward(img, hw, hb)
    packed = dev(ops.pack_tower_weights(hw, hb))
    out = host(ops.tower_forward(dev(img), packed, L, precision=precision))
    assert np.isfinite(out).all()
    err = float(np.abs(out - ref).max())
    print(precision, "scale", scale, err)
    assert err < 1e-5


@pytest.mark.parametrize("precision", ["bf16x6", "f16x3", "f16x3w", "f16x3m32"])
@pytest.mark.parametrize("nlayers,H,W", [(5, 700, 530), (3, 300, 1100), (2, 530, 517)])
def test_tower_bf16x6_large_vs_fp32(gpu, nlayers, H, W, precision):
    """Sizes with more output tiles than CUs (the persistent bf16x6 kernel's tile loop, partial
    edge tiles, the c-block-major intermediate layout): bf16x6 vs the fp32-MFMA kernel, both
    fp32-level accurate, agree to ~1e-6."""
    from scenedepthestimation_amd import mc_cnn, ops
    rng = np.random.default_rng(H + W)
    w = mc_cnn.synthetic_weights(nlayers, seed=3)
    packed = dev(ops.pack_tower_weights(*mc_cnn.layer_lists(w, nlayers)))
    img = torch.zeros((H + 2 * nlayers, W + 2 * nlayers), device="cuda")
    img[nlayers:-nlayers, nlayers:-nlayers] = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32)).cuda()
    a = ops.tower_forward(img, packed, nlayers, precision="fp32")
    b = ops.tower_forward(img, packed, nlayers, precision=precision)
    torch.cuda.synchronize()
    assert torch.isfinite(b).all()
    err = float((a - b).abs().max())
    print(precision, "vs fp32 tower", (nlayers, H, W), err)
    assert err < 1e-5


def test_tower_layer_api_matches_forward(gpu):
    """sde_tower_layer ([h][w][64] in/out) chained layer by layer == sde_tower_forward."""
    from scenedepthestimation_amd import mc_cnn, ops
    L, H, W = 5, 150, 610
    rng = np.random.default_rng(5)
    packed = dev(ops.pack_tower_weights(*mc_cnn.layer_lists(mc_cnn.synthetic_weights(L, seed=9), L)))
    img = torch.zeros((H + 2 * L, W + 2 * L), device="cuda")
    img[L:-L, L:-L] = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32)).cuda()
    for prec, lay in (("fp32", "hw"), ("bf16x6", "hw"), ("bf16x6", "cb"), ("f16x3", "hw"), ("f16x3", "cb"),
                      ("f16x3", "split"), ("f16x3w", "hw"), ("f16x3w", "cb"), ("f16x3m32", "hw"), ("f16x3m32", "cb")):
        full = ops.tower_forward(img, packed, L, precision=prec)
        x = img
        words = torch.zeros(64, device="cuda")         # f16x3 bound words (+ the split scale words at +32)
        ops.absmax(img, words[0:1])
        cbl, sp = lay == "cb", lay == "split"
        for layer in range(2, L + 1):
            shrink = 4 if layer == 2 else 2
            y = torch.empty((x.shape[0] - shrink, x.shape[1] - shrink, 64), device="cuda")
            ops.tower_layer(x, packed, L, layer, y, precision=prec, in_cblock=cbl and layer > 2,
                            out_cblock=cbl and layer < L, in_absmax=words[layer - 2:layer - 1],
                            out_absmax=words[layer - 1:layer] if layer < L else None,
                            in_split=sp and layer > 2, out_split=sp and layer < L)
            x = y
        torch.cuda.synchronize()
        if prec == "f16x3" and sp != ops.TOWER_SPLIT_ACT:
            # split activations take their scalings from a-priori bounds instead of the measured maxima:
            # a different rounding of the same fp32-level arithmetic than tower_forward's layout
            err = float((x - full).abs().max())
            assert err < 2e-6, (prec, lay, err)
        else:
            # same arithmetic in the same order whatever the activation layout: bit-identical
            assert torch.equal(x, full), (prec, lay)


def test_tower_split_activation_layout(gpu):
    """SDE_TOWER_OUT_SPLIT: layer 2's outputs as 16 planes [cblk32][part][quarter] of [h][w][8 fp16] --
    (hi + lo) / 2^sigma reproduces the fp32 layer output within the split's 2^-22 relative + 2^-25 / 2^sigma
    absolute bound, the bound word is the fp32 path's exactly, 2^sigma is published at word + 32 and keeps
    |hi| < 2^15 (no overflow); the next (last) layer reading the split planes (IN_SPLIT) matches the
    fp32-input layer to fp32-level error."""
    from scenedepthestimation_amd import mc_cnn, ops
    L, H, W = 3, 70, 90
    rng = np.random.default_rng(21)
    packed = dev(ops.pack_tower_weights(*mc_cnn.layer_lists(mc_cnn.synthetic_weights(L, seed=2), L)))
    img = torch.zeros((H + 2 * L, W + 2 * L), device="cuda")
    img[L:-L, L:-L] = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32)).cuda()
    h2, w2 = H + 2 * L - 4, W + 2 * L - 4
    wa, wb = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    ops.absmax(img, wa[0:1])
    ops.absmax(img, wb[0:1])
    ya = torch.empty((h2, w2, 64), device="cuda")
    yb = torch.empty((h2, w2, 64), device="cuda")
    ops.tower_layer(img, packed, L, 2, ya, precision="f16x3", in_absmax=wa[0:1], out_absmax=wa[1:2])
    ops.tower_layer(img, packed, L, 2, yb, precision="f16x3", in_absmax=wb[0:1], out_absmax=wb[1:2], out_split=True)
    torch.cuda.synchronize()
    assert wa[1].item() == wb[1].item() > 0                       # the measured bound word
    s = wb[1 + 32].item()
    sigma = int(np.log2(s))
    assert s == 2.0 ** sigma and wa[33].item() == 0
    planes = host(yb).view(np.float16).reshape(2, 2, 4, h2, w2, 8).astype(np.float64)   # [cb][part][q][h][w][8]
    hi, lo = planes[:, 0], planes[:, 1]
    assert np.abs(hi).max() < 2.0 ** 15
    val = (hi + lo).transpose(2, 3, 0, 1, 4).reshape(h2, w2, 64)                         # -> [h][w][cb q e]
    ref = host(ya).astype(np.float64) * s
    assert np.all(np.abs(val - ref) <= np.abs(ref) * 2.0 ** -22 + 2.0 ** -25)
    # the next layer from either layout
    za = torch.empty((h2 - 2, w2 - 2, 64), device="cuda")
    zb = torch.empty((h2 - 2, w2 - 2, 64), device="cuda")
    ops.tower_layer(ya, packed, L, 3, za, precision="f16x3", in_absmax=wa[1:2])
    ops.tower_layer(yb, packed, L, 3, zb, precision="f16x3", in_absmax=wb[1:2], in_split=True)
    torch.cuda.synchronize()
    err = float((za - zb).abs().max())       # L2-normalised features
    assert err <= 2e-6, err


def test_tower_layer_api_mixed_layouts_vs_oracle(gpu, oracle):
    """The layer-API instantiations no forward reaches, on a 4-layer tower (a first, a middle and a last layer) at
    9 x 40: a middle layer that changes the activation layout (c-block in / [h][w][64] out and the reverse; every
    split arithmetic), and a last layer that emits the hi / lo / norm planes from [h][w][64] or split activations.
    Features against the fp64 oracle; emitted planes against sde_feature_split of the features, bit for bit."""
    from scenedepthestimation_amd import mc_cnn, ops
    L, H, W = 4, 9, 40
    rng = np.random.default_rng(4009)
    hw, hb = mc_cnn.layer_lists(mc_cnn.synthetic_weights(L, seed=L), L)
    img = np.zeros((H + 2 * L, W + 2 * L), np.float32)
    img[L:-L, L:-L] = rng.standard_normal((H, W)).astype(np.float32)
    ref = oracle.tower_forward(img, hw, hb)
    packed = dev(ops.pack_tower_weights(hw, hb))
    # layout of layer 2's and layer 3's outputs; emit: the last layer writes the planes
    chains = [(prec, l2, l3, False) for prec in ("bf16x6", "f16x3", "f16x3w", "f16x3m32")
              for l2, l3 in (("cb", "hw"), ("hw", "cb"))]
    chains += [("f16x3", "hw", "hw", True), ("f16x3", "split", "split", True)]
    for prec, l2, l3, emit in chains:
        x = dev(img)
        words = torch.zeros(64, device="cuda")
        ops.absmax(x, words[0:1])
        lay = {1: "hw", 2: l2, 3: l3, 4: "hw"}      # lay[l]: layout of layer l's output
        planes = ops.new_split(H, W, "cuda") if emit else None
        for layer in range(2, L + 1):
            shrink = 4 if layer == 2 else 2
            y = torch.empty((x.shape[0] - shrink, x.shape[1] - shrink, 64), device="cuda")
            ops.tower_layer(x, packed, L, layer, y, precision=prec, split=planes if layer == L else None,
                            in_cblock=lay[layer - 1] == "cb", out_cblock=lay[layer] == "cb",
                            in_absmax=words[layer - 2:layer - 1], out_absmax=words[layer - 1:layer] if layer < L else None,
                            in_split=lay[layer - 1] == "split", out_split=lay[layer] == "split")
            x = y
        err = float(np.abs(host(x) - ref).max())
        print(prec, l2, l3, emit, "vs fp64 oracle", err)
        assert err < 1e-5, (prec, l2, l3, emit, err)
        if emit:
            again = ops.feature_split(x)
            assert torch.equal(planes[0], again[0]) and torch.equal(planes[1], again[1]), (prec, l2)
            true_n = np.sqrt((host(x).astype(np.float64) ** 2).sum(-1))
            assert np.all(host(planes[2]) >= true_n) and np.all(host(planes[2]) <= true_n * 1.00001 + 1e-30)


def test_tower_winograd_large_plane_takes_direct_kernel(gpu):
    """A 64->64 layer whose activation plane is >= 4 GiB (4100 x 4100 x 64 f32): the Winograd
    kernel's 32-bit descriptors cannot span it, so f16x3w must run the direct f16x3 kernel --
    bit-identical to precision "f16x3" (the wrapped record counts dropped stores)."""
    from scenedepthestimation_amd import mc_cnn, ops
    L, Hin, Win = 5, 4100, 4100
    assert Hin * Win * 256 >= 2 ** 32
    packed = dev(ops.pack_tower_weights(*mc_cnn.layer_lists(mc_cnn.synthetic_weights(L, seed=4), L)))
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand((Hin, Win, 64), device="cuda", generator=g)
    word = x.abs().max().reshape(1)
    outs = []
    for prec in ("f16x3", "f16x3w"):
        y = torch.empty((Hin - 2, Win - 2, 64), device="cuda")
        ob = torch.zeros(1, device="cuda")
        ops.tower_layer(x, packed, L, 3, y, precision=prec, in_absmax=word, out_absmax=ob)
        outs.append((y, ob))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    del x, outs
    torch.cuda.empty_cache()


@pytest.mark.parametrize("H,W", [(37, 53), (1, 9), (7, 1), (375, 450), (1024, 1024), (2000, 3000), (1110, 1390),
                                 (4097, 4099)])
def test_preprocess_u8(gpu, oracle, H, W):
    """Device z-norm + pad == NumPy's (I - np.mean(I)) / np.std(I) on the float32 image
    (match_single.py:40-41) bit for bit, at the configs' sizes: NumPy's float32 reduction order
    (pairwise sums of 8192-element pieces, added in order) restated on the device.  4097 x 4099 is an
    odd count above 2^24 pixels, where NumPy 2's fp64 quotient of the sum and the count differs from
    a float32 one (the count is not a float32)."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(H * 7 + W)
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    if H * W > 64:
        img[: H // 3] = (img[: H // 3] // 4 + 60).astype(np.uint8)     # not uniform: a skewed histogram
    out = host(ops.preprocess_u8(dev(img), 5))
    ref = oracle.pad_image(oracle.znorm(img.astype(np.float32)), 11)
    print(H, W, "max |device - numpy|", float(np.abs(out - ref).max()))
    assert out.tobytes() == ref.tobytes()


# ----------------------------------------------------------------------------
# SGM path
# ----------------------------------------------------------------------------
def test_penalties_bit_exact(gpu, oracle):
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (31, 45)).astype(np.uint8)
    img[5:9, 5:20] = 100
    assert host(ops.sgm_penalties(dev(img))).tobytes() == oracle.sgm_penalties(img).tobytes()


@pytest.mark.parametrize("H,W,D", [(6, 7, 8), (9, 3, 16), (3, 11, 64), (20, 30, 128), (17, 23, 192), (12, 9, 100),
                                   (2, 2, 4), (8, 8, 512)])
def test_sgm_8path_bit_exact(gpu, oracle, H, W, D):
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(H * W * D)
    cv = (rng.standard_normal((H, W, D)) * 0.5).astype(np.float32)
    cv[rng.random((H, W, D)) < 0.1] = 1.0
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    pen = oracle.sgm_penalties(img)
    ref = oracle.sgm_8path(cv, pen)
    S = host(ops.sgm_8path(dev(cv), dev(pen)))
    assert S.tobytes() == ref.tobytes()
    assert np.array_equal(host(ops.wta(dev(ref), "HWD", "d0")), oracle.wta_sgm(ref))


@pytest.mark.parametrize("H,W,D,L1,iters", [(23, 61, 40, 14, 2), (40, 33, 130, 16, 1), (70, 12, 7, 32, 2),
                                             (3, 2, 16, 14, 1), (16, 96, 192, 14, 3), (300, 270, 70, 14, 1)])
def test_cbca_pair_bit_exact(gpu, oracle, H, W, D, L1, iters):
    """Any two volumes (the right one through the rotation into left coordinates) == the oracle's
    per-side aggregation; lines longer than one segment (SDE_CBCA_SEG = 256) in the last case."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(7 * H + W + D)
    il, ir = _cbca_images(rng, H, W), _cbca_images(rng, H, W)
    al, ar = oracle.cbca_arms(il, L1, 0.03), oracle.cbca_arms(ir, L1, 0.03)
    cl = rng.standard_normal((H, W, D)).astype(np.float32)
    cr = rng.standard_normal((H, W, D)).astype(np.float32)
    want_l = oracle.cbca(cl, al, ar, "left", iters, L1=L1)
    want_r = oracle.cbca(cr, ar, al, "right", iters, L1=L1)
    gl, gr = dev(cl), dev(cr)
    ops.cbca_pair(gl, gr, dev(al.view(np.int32)), dev(ar.view(np.int32)), L1, iters)
    assert host(gl).tobytes() == want_l.tobytes()
    assert host(gr).tobytes() == want_r.tobytes()


def _sheared_pair(rng, H, W, D, scale=1.0, offset=0.0):
    """A left volume (invalid voxels x < d at 1.0, as the GPU path fills them) and its right shear."""
    cl = (rng.standard_normal((H, W, D)) * scale + offset).astype(np.float32)
    cr = np.ones_like(cl)
    for d in range(D):
        cl[:, :min(d, W), d] = 1.0
        if d < W:
            cr[:, :W - d, d] = cl[:, d:, d]
    return cl, cr


@pytest.mark.parametrize("H,W,D,L1,iters", [(23, 61, 40, 14, 2), (16, 96, 192, 14, 2), (40, 33, 130, 16, 1),
                                             (70, 12, 7, 32, 2), (270, 300, 66, 14, 2), (3, 2, 16, 14, 1),
                                             (23, 61, 40, 14, 0), (16, 96, 192, 14, 0)])
def test_cbca_lr_bit_exact(gpu, oracle, H, W, D, L1, iters):
    """The GPU path's pair: one volume aggregated + the shear == the oracle's sdeo_cbca_lr, and (the
    right volume being the left one's shear) == aggregating both volumes (cbca_pair)."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(11 * H + W + D)
    il, ir = _cbca_images(rng, H, W), _cbca_images(rng, H, W)
    al, ar = oracle.cbca_arms(il, L1, 0.03), oracle.cbca_arms(ir, L1, 0.03)
    cl, cr = _sheared_pair(rng, H, W, D, 2.0, 3.0)
    want_l, want_r = oracle.cbca_lr(cl, cr, al, ar, iters, L1=L1)
    # cv_r is an output (its valid voxels are never read): hand in garbage there
    cr_in = cr.copy()
    for d in range(min(D, W)):
        cr_in[:, :W - d, d] = -7.5
    gl, gr = dev(cl), dev(cr_in)
    ops.cbca_lr(gl, gr, dev(al.view(np.int32)), dev(ar.view(np.int32)), L1, iters)
    assert host(gl).tobytes() == want_l.tobytes()
    assert host(gr).tobytes() == want_r.tobytes()
    pl, pr = dev(cl), dev(cr)
    ops.cbca_pair(pl, pr, dev(al.view(np.int32)), dev(ar.view(np.int32)), L1, iters)
    assert torch.equal(pl, gl) and torch.equal(pr, gr)


def test_cbca_reciprocals_correctly_rounded(gpu):
    """The mean's 1/count (v_rcp_f64 + two Newton steps) is the IEEE quotient for every count the
    definition can produce: (2 * 31 + 1)^2 at L1 = 32."""
    from scenedepthestimation_amd import ops
    n = 63 * 63
    got = ops.cbca_reciprocals(n).cpu().numpy()
    want = 1.0 / np.arange(1, n + 1, dtype=np.float64)
    assert got.tobytes() == want.tobytes()


def test_cbca_pair_bench_width_bit_exact(gpu, oracle):
    """A band of rows at the benchmark's width and D (1024 x 192): every x - d / x + d edge regime."""
    test_cbca_pair_bit_exact(gpu, oracle, 24, 1024, 192, 14, 2)
    test_cbca_lr_bit_exact(gpu, oracle, 24, 1024, 192, 14, 2)


def test_cbca_pair_config3_identity(gpu):
    """Middlebury-2014 scale (2000 x 3000 x 256: 6 GB per volume, a column's offsets beyond 32 bits):
    with zero arms every support is the pixel itself, and for small-integer costs the fp64 prefix
    differences are exact, so both volumes must come back unchanged bit for bit -- any misaddressed
    row, column or disparity changes a value (the right one also through both rotations)."""
    from scenedepthestimation_amd import ops
    H, W, D = 2000, 3000, 256
    y = torch.arange(H, device="cuda").view(H, 1, 1)
    x = torch.arange(W, device="cuda").view(1, W, 1)
    d = torch.arange(D, device="cuda").view(1, 1, D)
    cl = ((7 * y + 3 * x + d) % 13).float()
    cr = ((5 * y + 11 * x + 2 * d) % 17).float()
    arms = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    gl, gr = cl.clone(), cr.clone()
    ops.cbca_pair(gl, gr, arms, arms, 14, 1)
    torch.cuda.synchronize()
    assert torch.equal(gl, cl) and torch.equal(gr, cr)
    del gl, gr
    # the shear: every valid right voxel becomes the left voxel at x + d, the invalid ones stay
    gl, gr = cl.clone(), cr.clone()
    ops.cbca_lr(gl, gr, arms, arms, 14, 1)
    torch.cuda.synchronize()
    assert torch.equal(gl, cl)
    xs = x + d
    want = torch.where(xs < W, ((7 * y + 3 * xs + d) % 13).float(), cr)
    assert torch.equal(gr, want)


@pytest.mark.parametrize("H,W,D", [(33, 70, 97), (19, 41, 192), (5, 130, 64), (70, 9, 300), (2, 50, 64)])
def test_sgm_8path_pair_bit_exact(gpu, oracle, H, W, D):
    """Both sides per launch; overwrite mode ignores S's contents, accumulate mode adds to them."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(H + W + D)
    cvs, pens, refs = [], [], []
    for k in range(2):
        cv = (rng.standard_normal((H, W, D)) * 0.5).astype(np.float32)
        cv[rng.random((H, W, D)) < 0.1] = 1.0
        cv[rng.random((H, W, D)) < 0.05] = -0.0          # signed zeros: DU's C + 0.0 vs C
        cv[rng.random((H, W, D)) < 0.05] = 0.0
        pen = oracle.sgm_penalties(rng.integers(0, 256, (H, W)).astype(np.uint8))
        cvs.append(cv), pens.append(pen), refs.append(oracle.sgm_8path(cv, pen))
    for fold in (False, True):          # DU folded into UD: penalties from sgm_penalties, finite costs
        S = [torch.full((H, W, D), float("nan"), device="cuda") for _ in range(2)]
        ops.sgm_8path_pair(dev(cvs[0]), dev(pens[0]), S[0], dev(cvs[1]), dev(pens[1]), S[1], zero_du_penalties=fold)
        for k in range(2):
            assert host(S[k]).tobytes() == refs[k].tobytes(), (fold, k)
    # one side, accumulate onto a non-zero S
    S0 = (rng.standard_normal((H, W, D))).astype(np.float32)
    want = oracle.sgm_8path(cvs[0], pens[0], S0.copy())
    got = dev(S0)
    ops.sgm_8path_pair(dev(cvs[0]), dev(pens[0]), got, accumulate=True)
    assert host(got).tobytes() == want.tobytes()
    got = dev(S0)
    ops.sgm_8path_pair(dev(cvs[0]), dev(pens[0]), got, accumulate=True, zero_du_penalties=True)
    assert host(got).tobytes() == want.tobytes()


# ----------------------------------------------------------------------------
# Cross-based aggregation (build-defined: bit-exact vs the oracle's restatement, parity unpinned vs the reference)
# ----------------------------------------------------------------------------
def _cbca_images(rng, H, W):
    base = rng.integers(0, 4, (H, W)).astype(np.float32) * 0.05
    return (np.repeat(base[:, ::3], 3, axis=1)[:, :W] + rng.standard_normal((H, W)).astype(np.float32) * 0.003)


@pytest.mark.parametrize("L1,tau", [(14, 0.02), (32, 0.08), (1, 1.0)])
def test_cbca_arms_bit_exact(gpu, oracle, L1, tau):
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(L1)
    img = _cbca_images(rng, 37, 70)
    pad = np.zeros((37 + 10, 70 + 10), np.float32)
    pad[5:-5, 5:-5] = img
    d = dev(pad)
    got = host(ops.cbca_arms(d[5:-5, 5:-5], L1, tau)).view(np.uint32)    # row-strided interior view
    assert np.array_equal(got, oracle.cbca_arms(img, L1, tau))


@pytest.mark.parametrize("H,W,D,L1,iters,side", [(23, 61, 40, 14, 2, "left"), (40, 33, 100, 16, 1, "right"),
                                                 (9, 130, 64, 20, 1, "left"), (70, 12, 7, 32, 2, "right"),
                                                 (5, 5, 3, 14, 0, "left"), (16, 96, 192, 14, 2, "left"),
                                                 (12, 300, 256, 14, 1, "left"), (300, 40, 70, 14, 2, "right"),
                                                 (280, 23, 30, 14, 1, "left")])
def test_cbca_bit_exact(gpu, oracle, H, W, D, L1, iters, side):
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(H * W + D)
    il, ir = _cbca_images(rng, H, W), _cbca_images(rng, H, W)
    al, ar = oracle.cbca_arms(il, L1, 0.03), oracle.cbca_arms(ir, L1, 0.03)
    ref, oth = (al, ar) if side == "left" else (ar, al)
    cv = rng.standard_normal((H, W, D)).astype(np.float32)
    want = oracle.cbca(cv, ref, oth, side, iters, L1=L1)
    got = dev(cv)
    ops.cbca(got, dev(ref.view(np.int32)), dev(oth.view(np.int32)), side, L1, iters)
    assert host(got).tobytes() == want.tobytes()


@pytest.mark.parametrize("H,W,D", [(33, 70, 97), (19, 41, 192), (5, 130, 64), (70, 9, 300), (2, 50, 64),
                                   (3, 2, 16), (2, 2, 4), (40, 33, 128)])
def test_sgm_8path_wta_pair_bit_exact(gpu, oracle, H, W, D):
    """WTA fused into the last direction == sgm_8path followed by the reference's WTA rule, both
    sides, with NaN / +inf / tie patterns in the final S (first-min and the d = 0 rule)."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(3 * H + W + D)
    cvs, pens, wants = [], [], []
    for k in range(2):
        cv = (rng.standard_normal((H, W, D)) * 0.5).astype(np.float32)
        cv[rng.random((H, W, D)) < 0.1] = 1.0
        cv[0, 0, :] = 0.25                      # a pixel whose costs tie at every d
        pen = oracle.sgm_penalties(rng.integers(0, 256, (H, W)).astype(np.uint8))
        ref = oracle.sgm_8path(cv, pen)
        cvs.append(cv), pens.append(pen), wants.append(oracle.wta_sgm(ref))
    for fold in (False, True):
        S = [torch.full((H, W, D), float("nan"), device="cuda") for _ in range(2)]
        dl, dr = ops.sgm_8path_wta_pair(dev(cvs[0]), dev(pens[0]), S[0], None, dev(cvs[1]), dev(pens[1]), S[1],
                                        None, zero_du_penalties=fold)
        assert np.array_equal(host(dl), wants[0]), fold
        assert np.array_equal(host(dr), wants[1]), fold
    # one side, accumulate mode onto an S with NaN / inf entries
    S0 = rng.standard_normal((H, W, D)).astype(np.float32)
    S0[rng.random((H, W, D)) < 0.02] = np.inf
    S0[0, :, 0] = np.nan
    want = oracle.wta_sgm(oracle.sgm_8path(cvs[0], pens[0], S0.copy()))
    d1, _ = ops.sgm_8path_wta_pair(dev(cvs[0]), dev(pens[0]), dev(S0), accumulate=True)
    assert np.array_equal(host(d1), want)


def test_matcher_cbca_sgm_end_to_end(gpu, oracle):
    """StereoMatcher.sgm_path with CBCA before SGM == the oracle composition on the same inputs."""
    from scenedepthestimation_amd.pipeline import StereoMatcher
    from scenedepthestimation_amd.synthetic import features, stereo_pair
    H, W, D = 24, 50, 16
    left, right, _ = stereo_pair(H, W, D, seed=4)
    fl, fr = features(H, W, seed=5), features(H, W, seed=6)
    m = StereoMatcher(H, W, D, weights="synthetic", cbca_iters=2, cbca_L1=14, cbca_tau=0.5)
    dl, dr = m.sgm_path(fl=dev(fl), fr=dev(fr), img_l=dev(left), img_r=dev(right), post=False)
    P = m.nlayers
    zl = host(m.img_pad[0])[P:P + H, P:P + W]      # the device z-norm the arms were built from
    zr = host(m.img_pad[1])[P:P + H, P:P + W]
    al, ar = oracle.cbca_arms(zl, 14, 0.5), oracle.cbca_arms(zr, 14, 0.5)
    assert ((al & 255) > 0).mean() > 0.2              # the arms are not trivial at this tau
    cl, cr = oracle.cost_volume_hwd(fl, fr, D, invalid=1.0, right=True)
    cl, cr = oracle.cbca(cl, al, ar, "left", 2, L1=14), oracle.cbca(cr, ar, al, "right", 2, L1=14)
    Sl = oracle.sgm_8path(cl, oracle.sgm_penalties(left))
    Sr = oracle.sgm_8path(cr, oracle.sgm_penalties(right))
    assert np.array_equal(host(dl), oracle.wta_sgm(Sl))
    assert np.array_equal(host(dr), oracle.wta_sgm(Sr))


@pytest.mark.parametrize("H,W,frac", [(37, 300, 0.9), (5, 4096, 0.5), (64, 129, 1.0), (64, 129, 0.0),
                                       (300, 70, 0.97)])
def test_lrc_fill_runs_bit_exact(gpu, oracle, H, W, frac):
    """Long flagged runs (quadratic for the reference's walks), fully flagged and clean maps."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(H * W)
    dl = rng.integers(0, 60, (H, W)).astype(np.float32) + rng.random((H, W)).astype(np.float32)
    flags = (rng.random((H, W)) < frac).astype(np.uint8)
    flags[H // 2, :] = 1                      # a whole flagged row and column
    flags[:, W // 3] = 1
    assert host(ops.lrc_fill(dev(dl), dev(flags))).tobytes() == oracle.lrc_fill(dl, flags).tobytes()


def test_post_processing_bit_exact(gpu, oracle):
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(12)
    H, W = 40, 300
    dl = rng.integers(0, 40, (H, W)).astype(np.float32)
    dr = rng.integers(0, 40, (H, W)).astype(np.float32)
    a, b = ops.lr_check(dev(dl), dev(dr))
    oa, ob = oracle.lr_check(dl, dr)
    assert np.array_equal(host(a), oa) and np.array_equal(host(b), ob)
    f = host(ops.lrc_fill(dev(dl), dev(oa)))
    assert f.tobytes() == oracle.lrc_fill(dl, oa).tobytes()
    dst = dev(dl.copy())
    ops.median5(dev(f), dst)
    assert host(dst).tobytes() == oracle.median5(f, dl).tobytes()


# ----------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------
def test_matcher_end_to_end(gpu, oracle):
    """u8 images -> tower -> fused CV+WTA; the disparity equals WTA1(compute_cost_volume) of the
    GPU features bit for bit, and the features match the fp64 tower within 1e-4."""
    from scenedepthestimation_amd import mc_cnn
    from scenedepthestimation_amd.pipeline import StereoMatcher
    from scenedepthestimation_amd.synthetic import stereo_pair
    H, W, D = 48, 96, 32
    left, right, _ = stereo_pair(H, W, D, seed=3)
    m = StereoMatcher(H, W, D)
    m.load_images(left, right)
    disp = host(m.match())
    fl, fr = host(m.feat[0]), host(m.feat[1])
    assert np.array_equal(disp, oracle.WTA1(oracle.compute_cost_volume(fl, fr, D)))
    w = mc_cnn.synthetic_weights(5)
    hw, hb = mc_cnn.layer_lists(w, 5)
    ref = oracle.tower_forward(host(m.img_pad[0]), hw, hb)
    assert np.abs(fl - ref).max() < 1e-4


def test_disparity_compute_by_gpu_vs_oracle(gpu, oracle):
    from scenedepthestimation_amd import process_functional as pf
    rng = np.random.default_rng(21)
    H, W, D = 24, 40, 128
    fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    il = rng.integers(0, 256, (H, W)).astype(np.uint8)
    ir = rng.integers(0, 256, (H, W)).astype(np.uint8)
    dt = np.zeros(7, np.float32)
    dl, dr, dt2 = pf.disparity_compute_by_gpu(il, ir, fl, fr, dt)
    assert dt2 is dt and dt[3] > 0
    cl, cr = oracle.cost_volume_hwd(fl, fr, D, invalid=1.0)
    Sl = oracle.sgm_8path(cl, oracle.sgm_penalties(il))
    Sr = oracle.sgm_8path(cr, oracle.sgm_penalties(ir))
    wl, wr = oracle.wta_sgm(Sl), oracle.wta_sgm(Sr)
    a, _ = oracle.lr_check(wl, wr)
    filled = oracle.lrc_fill(wl, a)
    assert np.array_equal(dl, oracle.median5(filled, wl))
    assert np.array_equal(dr, oracle.median5(wr, wr))


def test_dshard_matcher_rccl_world1(gpu, oracle):
    """The disparity-sharded matcher's collectives on RCCL (one rank on the single-GPU box)."""
    import os
    import socket
    import torch.distributed as dist
    from scenedepthestimation_amd.parallel import DisparityShardedMatcher
    from scenedepthestimation_amd.synthetic import stereo_pair
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        H, W, D = 40, 80, 24
        left, right, _ = stereo_pair(H, W, D, seed=5)
        dm = DisparityShardedMatcher(H, W, D, 0, 1)
        dm.m.load_images(left, right)
        disp = host(dm.match())
        fl, fr = host(dm.m.feat[0]), host(dm.m.feat[1])
        assert np.array_equal(disp, oracle.WTA1(oracle.compute_cost_volume(fl, fr, D)))
    finally:
        dist.destroy_process_group()


def test_rowband_matcher_rccl_world1(gpu, oracle):
    """The row-band matcher's collectives on RCCL (one rank on the single-GPU box)."""
    import os
    import socket
    import torch.distributed as dist
    from scenedepthestimation_amd.parallel import RowBandMatcher
    from scenedepthestimation_amd.pipeline import StereoMatcher
    from scenedepthestimation_amd.synthetic import stereo_pair
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        H, W, D = 40, 80, 24
        left, right, _ = stereo_pair(H, W, D, seed=6)
        rb = RowBandMatcher(H, W, D, 0, 1)
        rb.load_images(left, right)
        disp = host(rb.match())
        m = StereoMatcher(H, W, D)
        m.load_images(left, right)
        assert np.array_equal(disp, host(m.match()))
        fl, fr = host(rb.band.feat[0]), host(rb.band.feat[1])
        assert np.array_equal(disp, oracle.WTA1(oracle.compute_cost_volume(fl, fr, D)))
    finally:
        dist.destroy_process_group()


def test_cli_match_single_end_to_end(gpu, tmp_path, monkeypatch):
    from scenedepthestimation_amd import imageio, match_single
    from scenedepthestimation_amd.synthetic import stereo_pair
    left, right, _ = stereo_pair(48, 96, 16, seed=9)
    imageio.imwrite(str(tmp_path / "eval" / "left_3.png"), left)
    imageio.imwrite(str(tmp_path / "eval" / "right_3.png"), right)
    monkeypatch.chdir(tmp_path)
    match_single.main(["-i", "3", "-g", "0", "--checkpoint", "synthetic", "--cpu-path", "--ndisp", "16"])
    out = imageio.imread_gray(str(tmp_path / "result" / "11_11" / "ld3.png"))
    assert out.shape == (48, 96) and out.max() < 16
    match_single.main(["-i", "3", "-g", "0", "--checkpoint", "synthetic", "--ndisp", "16", "-f", "sgm"])
    assert imageio.imread_gray(str(tmp_path / "result" / "sgm" / "ld3.png")).shape == (48, 96)


# ----------------------------------------------------------------------------
# certified fast path: bit-identical to the exact kernel for every input
# ----------------------------------------------------------------------------
def _both_modes(fl, fr, d0, d1):
    from scenedepthestimation_amd import ops
    outs = {}
    for mode in ("exact", "certified"):
        ws = torch.empty(ops.cv_wta_workspace_bytes(*fl.shape[:2]), dtype=torch.uint8, device="cuda")
        disp, mn, am = ops.cv_wta(dev(fl), dev(fr), d0, d1, want=("disp", "min", "argmin"), mode=mode, workspace=ws)
        outs[mode] = (host(disp), host(mn), host(am), ops.cv_wta_fixups(ws) if mode == "certified" else 0)
    return outs


def test_certified_golden(gpu, golden, golden_cases):
    from scenedepthestimation_amd import ops
    for n in golden_cases:
        fl, fr, d = golden[n + "__fl"], golden[n + "__fr"], int(golden[n + "__ndisp"])
        disp, _, _ = ops.cv_wta(dev(fl), dev(fr), 0, d, mode="certified")
        assert np.array_equal(host(disp), golden[n + "__disp"]), n


@pytest.mark.parametrize("H,W,D,d0", [(3, 200, 64, 0), (2, 333, 192, 0), (2, 130, 256, 0), (2, 700, 512, 0),
                                      (3, 97, 100, 0), (2, 300, 192, 40), (2, 64, 192, 0), (1, 5, 9, 0),
                                      (2, 1000, 192, 0), (2, 129, 100, 33), (3, 250, 256, 17), (2, 70, 1, 0),
                                      (2, 600, 288, 32),
                                      # past one row sweep's window: 256-disparity chunks merged in d order
                                      (2, 900, 700, 5), (3, 300, 600, 100)])
def test_certified_matches_exact(gpu, oracle, H, W, D, d0):
    rng = np.random.default_rng(H * 1000 + W + D)
    fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    o = _both_modes(fl, fr, d0, D)
    for k in range(3):
        assert o["exact"][k].tobytes() == o["certified"][k].tobytes(), k
    omn, oam = oracle.cv_wta_shard(fl, fr, d0, D)
    assert np.array_equal(o["certified"][2], oam) and o["certified"][1].tobytes() == omn.tobytes()


@pytest.mark.parametrize("W,D", [(260, 96), (700, 512)])
def test_certified_adversarial_ties_and_nonfinite(gpu, oracle, W, D):
    """D = 512: the chunked row sweep, with exact ties straddling the 256-disparity chunk boundary."""
    rng = np.random.default_rng(123)
    H = 4
    fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr[0] = fr[0, 7]                       # a constant row: every valid d ties exactly
    fr[1, 100:160] = fr[1, 40:100]         # periodic texture: exact ties at two disparities
    if D > 256:
        fl[1, 600] = fr[1, 600 - 200]      # the same best at d = 200 and d = 300 (either side of the boundary)
        fr[1, 300] = fr[1, 400]
    fr[2, :, :32] *= 1.0 + 1e-6            # near-ties below the fast path's resolution
    fl[3, 50] = np.inf                     # non-finite features take the exact path
    fr[3, 10] = np.nan
    fl[3, 200] = 0.0                       # zero vector: all costs -0.0
    o = _both_modes(fl, fr, 0, D)
    for k in range(3):
        assert o["exact"][k].tobytes() == o["certified"][k].tobytes(), k
    # the constant row's ties are resolved by the row kernel's own exact scan; the non-finite
    # features (row 3) go to the IEEE fix-up kernel's list
    assert o["certified"][3] >= 1
    ref = oracle.WTA1(oracle.compute_cost_volume(np.nan_to_num(fl[:3]), fr[:3], D))
    assert np.array_equal(o["certified"][0][:3], ref)


def test_certified_past_64_chunks_is_exact(gpu, oracle):
    """A certified request over more than 64 chunks of 256 disparities (here 65, on 80 pixels) has no chunk
    planes in the workspace and runs the exact kernel: the oracle's and the exact mode's bytes on every output,
    and a fix-up count read from zeroed counters (the workspace arrives filled with 0xA5)."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(65)
    H, W, d1 = 2, 40, 16400
    fl = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr = l2n(rng.standard_normal((H, W, 64)).astype(np.float32))
    fr[:, 20:32] = fr[:, 4:16]                # repeated texture -> exact cost ties
    ws = torch.full((ops.cv_wta_workspace_bytes(H, W),), 0xA5, dtype=torch.uint8, device="cuda")
    disp, mn, am = ops.cv_wta(dev(fl), dev(fr), 0, d1, mode="certified", want=("disp", "min", "argmin"), workspace=ws)
    fix = ops.cv_wta_fixups(ws)
    ed, em, ea = ops.cv_wta(dev(fl), dev(fr), 0, d1, mode="exact", want=("disp", "min", "argmin"))
    omn, oam = oracle.cv_wta_shard(fl, fr, 0, d1)
    assert host(mn).tobytes() == omn.tobytes()
    assert host(am).tobytes() == oam.astype(np.int32).tobytes()
    assert host(disp).tobytes() == oam.astype(np.float32).tobytes()
    for got, ex in ((disp, ed), (mn, em), (am, ea)):
        assert host(got).tobytes() == host(ex).tobytes()
    assert 0 <= fix <= H * W


def test_certified_fixup_rate_is_small_on_textured_pairs(gpu):
    """On a textured synthetic pair through the real tower, almost every pixel is certified."""
    from scenedepthestimation_amd import ops
    from scenedepthestimation_amd.pipeline import StereoMatcher
    from scenedepthestimation_amd.synthetic import stereo_pair
    H, W, D = 128, 256, 64
    left, right, _ = stereo_pair(H, W, D, seed=4)
    m = StereoMatcher(H, W, D)
    m.load_images(left, right)
    m.features()
    m.cost_wta()
    fix = ops.cv_wta_fixups(m.cv_ws)
    exact, _, _ = ops.cv_wta(m.feat[0], m.feat[1], 0, D, mode="exact")
    assert np.array_equal(host(m.disp), host(exact))
    print("certified fix-up pixels:", fix, "of", H * W)
    assert fix < 0.2 * H * W


def test_feature_split_and_tower_emission(gpu, oracle):
    """hi + lo reproduces x to 2^-16, norms bound the true L2 norm, and the tower's last-layer
    emission equals sde_feature_split of its own output bit for bit."""
    from scenedepthestimation_amd import mc_cnn, ops
    rng = np.random.default_rng(31)
    H, W, L = 24, 70, 5
    img = np.zeros((H + 2 * L, W + 2 * L), np.float32)
    img[L:-L, L:-L] = rng.standard_normal((H, W)).astype(np.float32)
    w = mc_cnn.synthetic_weights(L)
    packed = dev(ops.pack_tower_weights(*mc_cnn.layer_lists(w, L)))
    for prec in ("fp32", "bf16x6", "f16x3", "f16x3m32"):
        emitted = ops.new_split(H, W, "cuda")
        feat = ops.tower_forward(dev(img), packed, L, precision=prec, split=emitted)
        again = ops.feature_split(feat)
        for a, b in zip(emitted[:2], again[:2]):
            assert torch.equal(a, b)
        f = host(feat).astype(np.float64)
        hi = (host(again[0]).astype(np.int32).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        lo = (host(again[1]).astype(np.int32).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        assert np.all(np.abs(f - hi - lo) <= np.abs(f) * 2.0 ** -16 + 1e-45)
        true_n = np.sqrt((f ** 2).sum(-1))
        for nb in (host(emitted[2]), host(again[2])):
            assert np.all(nb >= true_n) and np.all(nb <= true_n * 1.00001 + 1e-30)


def test_cv_wta_split_matches_exact(gpu, oracle):
    """The pipeline path: tower-emitted planes -> certified kernel == exact kernel == oracle."""
    from scenedepthestimation_amd import ops
    from scenedepthestimation_amd.pipeline import StereoMatcher
    from scenedepthestimation_amd.synthetic import stereo_pair
    for (H, W, D) in [(40, 200, 64), (33, 130, 192), (20, 96, 256)]:
        left, right, _ = stereo_pair(H, W, D, seed=H)
        m = StereoMatcher(H, W, D, emit_split=True)
        m.load_images(left, right)
        m.features()
        assert m.split_valid
        disp, mn, am = m.cost_wta(want=("disp", "min", "argmin"))
        ed, em, ea = ops.cv_wta(m.feat[0], m.feat[1], 0, D, mode="exact", want=("disp", "min", "argmin"))
        assert torch.equal(disp, ed) and torch.equal(am, ea)
        assert host(mn).tobytes() == host(em).tobytes()
        fl, fr = host(m.feat[0]), host(m.feat[1])
        assert np.array_equal(host(disp), oracle.WTA1(oracle.compute_cost_volume(fl, fr, D)))


@pytest.mark.parametrize("off,n", [(0, 0), (0, 1), (1, 3), (3, 1000), (2, 4097), (0, 1 << 20)])
def test_absmax(gpu, off, n):
    """sde_absmax_f32 (the f16x3 tower's image bound): unaligned heads and ragged tails."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(n + off)
    x = rng.standard_normal(off + n).astype(np.float32) * 3
    if n:
        x[off + rng.integers(n)] = -50.0
    xd = dev(x)[off:]
    word = torch.full((1,), 1.5, device="cuda")
    ops.absmax(xd, word)
    want = max(1.5, float(np.abs(x[off:]).max())) if n else 1.5
    assert float(word.cpu()[0]) == want


@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x3", "f16x3w", "f16x3m32"])
@pytest.mark.parametrize("nlayers,H,W,N", [(5, 150, 300, 2), (3, 70, 45, 3), (2, 33, 90, 2), (1, 9, 12, 2),
                                           (5, 40, 33, 1)])
def test_tower_forward_batch_equals_single(gpu, precision, nlayers, H, W, N):
    """sde_tower_forward_batch (all images in one persistent tile space, per-image bound words)
    gives every image exactly what sde_tower_forward gives it alone; the layer-by-layer batch API
    chained the same way gives the same bits."""
    from scenedepthestimation_amd import mc_cnn, ops
    rng = np.random.default_rng(N * 100 + H)
    packed = dev(ops.pack_tower_weights(*mc_cnn.layer_lists(mc_cnn.synthetic_weights(nlayers, seed=4), nlayers)))
    L = nlayers
    imgs = torch.zeros((N, H + 2 * L, W + 2 * L), device="cuda")
    for i in range(N):   # images of very different dynamic range: per-image f16x3 scalings
        imgs[i, L:-L, L:-L] = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32) * 10.0 ** (2 * i)).cuda()
    out = ops.tower_forward_batch(imgs, packed, L, precision=precision)
    for i in range(N):
        single = ops.tower_forward(imgs[i].contiguous(), packed, L, precision=precision)
        assert torch.equal(out[i], single), (precision, i)
    if L >= 2:
        # the forward's inter-layer layout: split activations on the default f16x3 tower, c-blocks otherwise
        sp = ops.TOWER_SPLIT_ACT and precision == "f16x3" and L > 2
        cbl = precision != "fp32" and not sp
        words = torch.zeros((N, 64), device="cuda")
        for i in range(N):
            ops.absmax(imgs[i], words[i, 0:1])
        x = imgs
        for layer in range(2, L + 1):
            sh = 4 if layer == 2 else 2
            y = torch.empty((N, x.shape[1] - sh, x.shape[2] - sh, 64), device="cuda")
            ops.tower_layer_batch(x, packed, L, layer, y, precision=precision, in_cblock=cbl and layer > 2,
                                  out_cblock=cbl and layer < L, in_absmax=words[:, layer - 2:layer - 1],
                                  out_absmax=words[:, layer - 1:layer] if layer < L else None,
                                  in_split=sp and layer > 2, out_split=sp and layer < L)
            x = y
        assert torch.equal(x, out)


def test_tower_split_chain_batch_many_tiles(gpu):
    """Split activations chained over a batch with more tiles than CUs (the 4-wave middle-layer kernel's
    persistent tile loop, its one-step-ahead LDS-DMA across tiles and images, partial edge tiles): the
    features match the c-block forward to fp32 level for images of very different dynamic range."""
    from scenedepthestimation_amd import mc_cnn, ops
    L, H, W, N = 5, 400, 700, 2
    rng = np.random.default_rng(8)
    packed = dev(ops.pack_tower_weights(*mc_cnn.layer_lists(mc_cnn.synthetic_weights(L, seed=6), L)))
    imgs = torch.zeros((N, H + 2 * L, W + 2 * L), device="cuda")
    for i in range(N):
        imgs[i, L:-L, L:-L] = torch.from_numpy(rng.standard_normal((H, W)).astype(np.float32) * 10.0 ** (3 * i)).cuda()
    ref = ops.tower_forward_batch(imgs, packed, L, precision="f16x3")
    words = torch.zeros((N, 64), device="cuda")
    for i in range(N):
        ops.absmax(imgs[i], words[i, 0:1])
    x = imgs
    for layer in range(2, L + 1):
        sh = 4 if layer == 2 else 2
        y = torch.empty((N, x.shape[1] - sh, x.shape[2] - sh, 64), device="cuda")
        ops.tower_layer_batch(x, packed, L, layer, y, precision="f16x3", in_absmax=words[:, layer - 2:layer - 1],
                              out_absmax=words[:, layer - 1:layer] if layer < L else None,
                              in_split=layer > 2, out_split=layer < L)
        x = y
    torch.cuda.synchronize()
    assert torch.isfinite(x).all()
    err = float((x - ref).abs().max())
    print("split chain vs c-block forward", err)
    assert err < 2e-6, err


def test_preprocess_and_absmax_batch(gpu):
    """sde_preprocess_u8_batch / sde_absmax_f32_batch (one launch per batch) == the per-image calls."""
    from scenedepthestimation_amd import ops
    rng = np.random.default_rng(3)
    N, H, W, P = 3, 37, 61, 5
    imgs = torch.from_numpy(rng.integers(0, 256, (N, H, W), dtype=np.uint8)).cuda()
    imgs[1] = imgs[1] // 7          # a different range per image
    out = ops.preprocess_u8_batch(imgs, P)
    words = torch.zeros((N, 4), device="cuda")
    ops.absmax_batch(out, words)
    for i in range(N):
        single = ops.preprocess_u8(imgs[i].contiguous(), P)
        assert torch.equal(out[i], single)
        w = torch.zeros(1, device="cuda")
        ops.absmax(single, w)
        assert float(words[i, 0]) == float(w[0]) == float(single.abs().max())
        assert torch.all(words[i, 1:] == 0)
