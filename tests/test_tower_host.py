"""tower_literal.py against the C oracle, its layout decoders against their encoders, and the conditions the GPU
tests in test_gpu_tower_epilogue.py lean on (spike placement and dominance, band image, zero-patch interior)."""
import numpy as np
import pytest

import tower_literal as tl


# (L, H, W, image, weights): signed biases everywhere; a spike; a dead channel (bias -1e3: dead under a Gaussian
# image, not under a 2^20 spike)
CASES = [(1, 6, 7, "gaussian", {}), (2, 9, 12, "gaussian", {}), (3, 17, 13, "spike", {}),
         (5, 5, 7, "gaussian", {"dead": (3, 17)}), (5, 12, 9, "spike", {}), (2, 12, 9, "gaussian", {"dead": (1, 5)}),
         (3, 8, 8, "gaussian", {"scale": 1e-6}), (2, 7, 9, "zero", {})]


def _image(kind, L, H, W):
    if kind == "gaussian":
        return tl.gaussian(L, H, W, 10 * H + W)
    if kind == "spike":
        return tl.spike(L, H, W, 10 * H + W, (H // 2, W // 3))
    return tl.zero(L, H, W)


@pytest.mark.parametrize("L,H,W,kind,opts", CASES)
def test_literal_features_equal_oracle(oracle, L, H, W, kind, opts):
    """Same fp64 arithmetic up to the order of the additions: the float32 features are the same bytes."""
    hw, hb = tl.weights(L, seed=L, **opts)
    img = _image(kind, L, H, W)
    acts, feats = tl.layers(img, hw, hb)
    assert [a.shape for a in acts] == [(H + 2 * (L - k), W + 2 * (L - k), 64) for k in range(1, L + 1)]
    ref = oracle.tower_forward(img, hw, hb)
    assert feats.astype(np.float32).tobytes() == ref.tobytes()
    if "dead" in opts:
        k, c = opts["dead"]
        assert not acts[k - 1][..., c].any() and acts[k - 1].any()
    assert all((a >= 0).all() for a in acts[:-1]) and (acts[-1] < 0).any()


def test_weights_options():
    hw, hb = tl.weights(5, seed=1)
    assert all(b.dtype == np.float32 and (b < 0).any() and (b > 0).any() and len(set(b.tolist())) == 64 for b in hb)
    assert 0.2 < np.concatenate(hb).std() < 0.4
    assert not np.array_equal(hb[1], hb[2])                        # per layer, not one vector
    assert [w.shape for w in hw] == [(3, 3, 1, 64)] + [(3, 3, 64, 64)] * 4
    _, zb = tl.weights(5, seed=1, zero_last_bias=True)
    assert not zb[4].any() and np.array_equal(zb[3], hb[3])
    _, nb = tl.weights(3, seed=1, nonpositive_bias=True)
    assert all((b <= 0).all() for b in nb)
    sw, sb = tl.weights(5, seed=1, scale=1e12)
    assert np.allclose(sw[2], hw[2] * 1e12 ** 0.2, rtol=1e-6) and np.allclose(sb[4], hb[4] * 1e12, rtol=1e-6)


def test_layer_and_layer32_agree_and_abs_sum_bounds():
    rng = np.random.default_rng(3)
    hw, hb = tl.weights(3, seed=8)
    x = np.maximum(rng.standard_normal((9, 11, 64)), 0).astype(np.float32)
    for last in (False, True):
        out, S = tl.layer(x, hw[1], hb[1], last)
        o32 = tl.layer32(x, hw[1], hb[1], last)
        assert out.dtype == np.float64 and o32.dtype == np.float32 and out.shape == S.shape == (7, 9, 64)
        assert (np.abs(out) <= S).all()
        rho32 = (np.abs(o32 - out) / S).max()
        assert 0 < rho32 <= 577 * 2.0 ** -24                        # K = 9 Cin + 1 roundings at most
        assert (out < 0).any() == last
    o1, S1 = tl.layer(rng.standard_normal((6, 7)).astype(np.float32), hw[0], hb[0], False)
    assert o1.shape == (4, 5, 64) and (np.abs(o1) <= S1).all()


def test_normalise_floor():
    x = np.zeros((2, 64))
    x[1, 0] = 1e-7                                                  # sum x^2 = 1e-14 < 1e-12: the x * 1e6 branch
    f = tl.normalise(x)
    assert not f[0].any() and f[1, 0] == pytest.approx(0.1) and np.isfinite(f).all()


def test_layout_decoders_invert_encoders():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (5, 7), (17, 33)):
        x = rng.standard_normal((h, w, 64)).astype(np.float32)
        assert np.array_equal(tl.cblock_decode(tl.cblock_encode(x)), x)
        enc = tl.cblock_encode(x)
        assert enc.reshape(4, h, w, 16)[2, h - 1, w - 1, 3] == x[h - 1, w - 1, 35]
        s = 2.0 ** 11
        buf = tl.split_encode(np.abs(x), s)
        assert buf.shape == (h, w, 64) and buf.dtype == np.float32
        val = tl.split_decode(buf, s)
        ref = np.abs(x).astype(np.float64)
        assert (np.abs(val - ref) <= ref * 2.0 ** -22 + 2.0 ** -25 / s).all()
        assert buf.view(np.float16).reshape(2, 2, 4, h, w, 8)[1, 0, 2, 0, 0, 5] == np.float16(abs(x[0, 0, 53]) * s)


@pytest.mark.parametrize("hout,wout", [(5, 7), (17, 33), (33, 49)])
def test_spiked_activation_places_the_maximum(hout, wout):
    hw, hb = tl.weights(3, seed=31)
    rng = np.random.default_rng(hout)
    x = np.maximum(rng.standard_normal((hout + 2, wout + 2, 64)), 0).astype(np.float32)
    for tx in (16, 32):
        for target in tl.spike_targets(hout, wout, tx):
            xs, c = tl.spiked_activation(x, hw[1], hb[1], target)
            assert (xs != x).sum() == 1 and 0 <= c < 64
            y, _ = tl.layer(xs, hw[1], hb[1], last=False)
            assert tl.spike_condition(y, target), target


def test_spike_targets_name_the_places():
    t32, t16 = set(tl.spike_targets(33, 49, 32)), set(tl.spike_targets(33, 49, 16))
    assert {(0, 0), (32, 48), (16, 48), (32, 24), (3, 15), (3, 16), (3, 31), (3, 32), (15, 5), (16, 5), (32, 5)} <= t32
    assert (32, 32) in t32 and (32, 48) in t16                       # first pixel of the last tile
    assert set(tl.spike_targets(5, 7, 32)) == {(0, 0), (4, 6), (2, 6), (4, 3)}


@pytest.mark.parametrize("where", ["right", "bottom", "corner"])
def test_edge_spike_is_larger_outside_the_output(where):
    """What a lane past the output's edge computes from the zero-filled input is >= 1.25 x the largest stored value."""
    hw, hb = tl.weights(3, seed=31)
    x = np.maximum(np.random.default_rng(2).standard_normal((19, 35, 64)), 0).astype(np.float32)
    xs, q = tl.edge_spiked_activation(x, hw[1], where)
    assert (xs != x).sum() == 1
    wide = np.zeros((21, 37, 64), np.float32)
    wide[:19, :35] = xs
    y, _ = tl.layer(wide, hw[1], hb[1], False)                      # [19, 35]: the 17 x 33 output and a rim of 2
    assert y.max() >= 1.25 * y[:17, :33].max() and y[:17, :33].max() > 0


def test_corner_spikes_place_layer2_maximum():
    """Layer 2 (conv1 fused) sees an input pixel through a 5 x 5 footprint: only a spike in an input corner reaches
    a single output, the first or the last one."""
    hw, hb = tl.weights(3, seed=31)
    for hout, wout in ((5, 7), (17, 33)):
        for corner, target in (((0, 0), (0, 0)), ((hout + 3, wout + 3), (hout - 1, wout - 1))):
            img = tl.corner_spike(hout + 4, wout + 4, corner)
            a1, _ = tl.layer(img, hw[0], hb[0], False)
            y, _ = tl.layer(a1, hw[1], hb[1], False)
            assert tl.spike_condition(y, target), (hout, wout, corner)


def test_band_image_condition():
    for H, W, world in tl.BAND_CASES:
        for u8 in tl.band_pair(H, W, seed=H):
            assert u8.max() == 255 and np.sort(u8.ravel())[-10] <= 20
            z = np.abs(tl.znorm_pad(u8, 5)[5:-5, 5:-5])
            band = -(-H // world)
            for r in range(world - 1):                              # bands plus their 2L halo rows
                assert z[r * band:min((r + 1) * band + 5, H - 5)].max() <= 0.25 * z.max()
            assert z[H - 5:].max() == z.max()


def test_zero_patch_interior():
    L, H, W, y0, x0, size = 5, 24, 26, 4, 6, 2 * 5 + 5
    img = tl.zero_patch(L, H, W, 2, y0, x0, size)
    ys, xs = tl.patch_interior(L, y0, x0, size)
    assert (ys.stop - ys.start, xs.stop - xs.start) == (5, 5)       # non-empty at the last layer, L = 5
    hw, hb = tl.weights(L, seed=4, zero_last_bias=True, nonpositive_bias=True)
    acts, feats = tl.layers(img, hw, hb)
    assert not feats[ys, xs].any() and np.isfinite(feats).all()
    assert feats[0, 0].any() and feats[-1, -1].any()                 # not a dead tower
