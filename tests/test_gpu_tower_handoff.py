"""conv64_h16s_kernel (16 x 16 tiles, outputs stored by the stager waves through the LDS hand-over buffer; the
default f16x3 kernel for layers 3..L with fp32 activations) against the retained 16 x 32-tile kernel ("f16x3t32" /
SDE_TOWER_TILE32): every accumulator takes the same MFMAs in the same order and every output the same epilogue
arithmetic, so features and bound words are compared bit for bit (torch.equal), never with a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEW, OLD = "f16x3", "f16x3t32"


def _packed(L, seed=3, scale=1.0):
    from scenedepthestimation_amd import mc_cnn, ops
    hw, hb = mc_cnn.layer_lists(mc_cnn.synthetic_weights(L, seed=seed), L)
    hw = [x * np.float32(scale ** (1 / L)) for x in hw]
    hb = [x * np.float32(scale ** ((k + 1) / L)) for k, x in enumerate(hb)]
    return torch.from_numpy(ops.pack_tower_weights(hw, hb)).cuda()


def _image(L, H, W, seed, gain=1.0):
    rng = np.random.default_rng(seed)
    img = np.zeros((H + 2 * L, W + 2 * L), np.float32)
    img[L:-L, L:-L] = rng.standard_normal((H, W)).astype(np.float32) * np.float32(gain)
    return torch.from_numpy(img).cuda()


def _same(a, b):
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} values differ"


# 5 x 7: one partial tile; 32 x 32: exact multiples of the tile at the last layer, partial tiles (34, 36, 38) at
# the earlier ones; 33 x 49 and 37 x 53: one row or column (and a few) into a new tile
@pytest.mark.parametrize("L,H,W", [(5, 5, 7), (5, 32, 32), (5, 33, 49), (5, 37, 53), (3, 33, 49), (2, 37, 53)])
def test_tile_edge_shapes(gpu, L, H, W):
    from scenedepthestimation_amd import ops
    packed, img = _packed(L), _image(L, H, W, 100 * H + W)
    _same(ops.tower_forward(img, packed, L, precision=NEW), ops.tower_forward(img, packed, L, precision=OLD))


@pytest.mark.parametrize("L", [5, 3])
def test_layer_api_hw64_layout(gpu, L):
    """The [h][w][64] activation layout between the layers (the forward passes c-block-major ones): layer 2, the
    middle layers and the last layer one launch each, activations and bound words equal after every layer."""
    from scenedepthestimation_amd import ops
    H, W = 33, 21
    packed, img = _packed(L), _image(L, H, W, 7)
    res = {}
    for prec in (NEW, OLD):
        words = torch.zeros(64, device="cuda")
        ops.absmax(img, words[0:1])
        x, outs = img, []
        for layer in range(2, L + 1):
            sh = 4 if layer == 2 else 2
            y = torch.full((x.shape[0] - sh, x.shape[1] - sh, 64), float("nan"), device="cuda")
            ops.tower_layer(x, packed, L, layer, y, precision=prec, in_absmax=words[layer - 2:layer - 1],
                            out_absmax=words[layer - 1:layer] if layer < L else None)
            outs.append(y)
            x = y
        res[prec] = (outs, words)
    for a, b in zip(res[NEW][0], res[OLD][0]):
        _same(a, b)
    _same(res[NEW][1], res[OLD][1])


@pytest.mark.parametrize("L", [5, 3, 2])
def test_pair_crosses_images(gpu, L):
    """Two 192 x 192 images in one batch: 2 x 144 = 288 last-layer tiles on at most 256 workgroups, so some
    workgroups run two tiles and cross from image 0 to image 1 (hand-over buffer reused, bound word flushed at the
    image change, last tile drained after the loop).  Image 1 is image 0 under another gain, so their scales
    differ; each image's features equal what it gets alone and what the 16 x 32 kernel gives, and the
    layer-by-layer driver (pipeline.run_tower) equals the one-call forward."""
    from scenedepthestimation_amd import ops, pipeline
    H = W = 192
    packed = _packed(L)
    a = _image(L, H, W, 11)
    pair = torch.stack([a, a * 37.0])
    both = ops.tower_forward_batch(pair, packed, L, precision=NEW)
    _same(both, ops.tower_forward_batch(pair, packed, L, precision=OLD))
    for i in range(2):
        _same(both[i], ops.tower_forward(pair[i].contiguous(), packed, L, precision=NEW))
    ws = torch.empty(ops.tower_batch_workspace_bytes(H, W, 2, L), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(both)
    pipeline.run_tower(pair, packed, L, out, ws, NEW)
    _same(out, both)


@pytest.mark.parametrize("L", [5, 3])
def test_small_workloads(gpu, L):
    """A pair of 16 x 16 images (most workgroups of the grid have no tile) and a batch of one image."""
    from scenedepthestimation_amd import ops
    packed = _packed(L)
    a = _image(L, 16, 16, 5)
    pair = torch.stack([a, a * 0.01])
    both = ops.tower_forward_batch(pair, packed, L, precision=NEW)
    _same(both, ops.tower_forward_batch(pair, packed, L, precision=OLD))
    one = ops.tower_forward_batch(pair[:1].contiguous(), packed, L, precision=NEW)
    _same(one[0], both[0])
    _same(one, ops.tower_forward_batch(pair[:1].contiguous(), packed, L, precision=OLD))


@pytest.mark.parametrize("scale", [1e-6, 1e12])
def test_scaling(gpu, scale):
    """Weights and biases far outside fp16's range (as test_tower_f16x3_dynamic_range scales them): the same bits
    as the 16 x 32 kernel and no non-finite output."""
    from scenedepthestimation_amd import ops
    L, H, W = 5, 24, 70
    packed, img = _packed(L, seed=9, scale=scale), _image(L, H, W, 5)
    _same(ops.tower_forward(img, packed, L, precision=NEW), ops.tower_forward(img, packed, L, precision=OLD))


def test_workspace_and_flags(gpu):
    """The selector needs no workspace of its own and is validated like the other kernel choices: f16x3 only,
    not with MFMA32.  With split activations it is accepted and changes nothing (those layers have only the
    16 x 32 kernel): the split planes and scale words are the same bytes with and without it."""
    from scenedepthestimation_amd import _lib, ops
    L, H, W = 3, 20, 37
    packed, img = _packed(L), _image(L, H, W, 3)
    ws = torch.empty(ops.tower_workspace_bytes(H, W, L), dtype=torch.uint8, device="cuda")
    _same(ops.tower_forward(img, packed, L, workspace=ws, precision=OLD),
          ops.tower_forward(img, packed, L, precision=NEW))
    assert ops.TOWER_PRECISIONS[OLD] == _lib.SDE_TOWER_F16X3 | _lib.SDE_TOWER_TILE32
    h2, w2 = H + 2 * L - 4, W + 2 * L - 4
    y = torch.empty((h2, w2, 64), device="cuda")
    words = torch.zeros(64, device="cuda")
    ops.absmax(img, words[0:1])

    def layer2(flags):
        return _lib.lib.sde_tower_layer_scaled(img.data_ptr(), H + 2 * L, W + 2 * L, packed.data_ptr(), L, 64, 2,
                                               y.data_ptr(), flags, None, None, None, words[0:1].data_ptr(),
                                               words[1:2].data_ptr(), None)
    assert layer2(_lib.SDE_TOWER_TILE32) != 0                                                  # not without f16x3
    assert layer2(_lib.SDE_TOWER_BF16X6 | _lib.SDE_TOWER_TILE32) != 0
    assert layer2(_lib.SDE_TOWER_F16X3 | _lib.SDE_TOWER_MFMA32 | _lib.SDE_TOWER_TILE32) != 0
    assert layer2(_lib.SDE_TOWER_F16X3 | _lib.SDE_TOWER_TILE32) == 0
    torch.cuda.synchronize()
    sp = {}
    for prec in (NEW, OLD):
        w = torch.zeros(64, device="cuda")
        ops.absmax(img, w[0:1])
        o = torch.zeros((h2, w2, 64), device="cuda")
        ops.tower_layer(img, packed, L, 2, o, precision=prec, in_absmax=w[0:1], out_absmax=w[1:2], out_split=True)
        f = torch.empty((H, W, 64), device="cuda")
        ops.tower_layer(o, packed, L, 3, f, precision=prec, in_absmax=w[1:2], in_split=True)
        sp[prec] = (o, w, f)
    for a, b in zip(sp[NEW], sp[OLD]):
        _same(a, b)
