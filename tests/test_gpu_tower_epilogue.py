"""The tower kernels' epilogues against tower_literal.py (NumPy, fp64) with inputs the other tower tests never use:
a signed bias per channel and layer, dead channels, spikes that put a layer's largest output on a chosen pixel,
guard rows of poison around every input and of 0xA5 around every output, persistent grids capped to 1-3 workgroups,
inputs whose scale exponents differ, and last-layer activations at the L2-norm floor.

Instantiations (launch_layer in tower.hip and the launchers in tower_<family>.hip), each with the tests that reach
it.  A: test_forward_*, test_layer_chains_vs_oracle;  B: test_each_layer_vs_fp64;  C: test_bound_word_*;
D: test_guard_rows_*;  E: test_capped_grid_* (and test_bound_word_pair_of_gains on one workgroup);  F:
test_workspace_reuse_*, test_matcher_reloaded_*, test_row_bands_* (whole towers: every default instantiation);
G: test_norm_floor_*.

  conv1_only_kernel                     L = 1                                  A
  conv64_mfma_kernel <first, last>      fp32: <1,0> <0,0> <0,1> <1,1>          A B D E G; planes <0,1>: A G
  conv64_x6p_kernel, bf16:  first <hw|cb out>, middle <hw|cb in, hw|cb out>, last <hw|cb in>, first+last
                                                                               A B D E G; planes on last: A G
  conv64_x6p_kernel, f16 (f16x3m32; every f16x3 variant at L = 2): the same nine
                                                                               A B C D E G; planes on last: A G
  conv64_h16_kernel FIRST <hw|cb|split out>  (f16x3, f16x3w, f16x3t32 layer 2) A B C D E
  conv64_h16_kernel middle <hw|cb in, hw|cb out>  (f16x3t32)                   A B C D E
  conv64_h16_kernel last <hw|cb in>  (f16x3t32)                                A B D E G
  conv64_h16_kernel last + planes <hw|cb in>                                   A B; G (hw in)
  conv64_h16_kernel last <split in>                                            A B D G
  conv64_h16_kernel last + planes <split in>                                   A B G
  conv64_h16q_kernel  (split in, split out)                                    A B C D E
  conv64_h16s_kernel middle <hw|cb in, hw|cb out>, last <hw|cb in>  (f16x3)    A B C D E G
  wino_kernel middle <hw|cb in, hw|cb out>, last <hw|cb in>  (f16x3w)          A B(hard bound only) C D E G

A launch that the argument rules reject returns a non-zero status (test_rejected_flag_combinations).

B's bounds.  rho = max |out - fp64(layer)(x)| / S, S = |W| (*) |x| + |b|, from the kernel's own input x.
Hard: rho <= K 2^-24 + p with K = 9 Cin + 1 roundings of an fp32 accumulation.  p: fp32 0; f16x3 2^-21 + 2^-23 (the
dropped l l' terms and the parts' roundings); bf16x6 2^-22: tower_x6p.h drops the three products x_i y_j with i + j >= 3, < 2^-23 |ab| in all
(|x_1| <= 2^-8 |x|, |x_2| <= 2^-16 |x|), and what three bf16 parts (24 bits) leave of each operand is <= 2^-24 of it,
another 2^-23 |ab| for the two operands.  Layer 2 is conv1 + conv2 in one kernel: its reference is the two layers in
fp64 and its bound gains conv1's own 10 roundings carried through |W2|.  A last layer is seen only normalised:
|d f_c| <= (|d y_c| + |f_c| ||d y||) / n with n = max(||y||, 1e-6), plus 68 roundings of the sum of squares, the
square root, the division and the product.  Split outputs add the split's 2^-22 relative + 2^-25 / 2^sigma.
Tight (direct kernels): rho <= 4 rho32 + p, rho32 the same statistic of the literal run in float32."""
import functools

import numpy as np
import pytest
import torch

import tower_literal as tl

pytestmark = pytest.mark.gpu

SIZES = [(5, 7), (16, 32), (17, 33), (33, 49)]
EPS = 2.0 ** -24
P_TERM = {"fp32": 0.0, "bf16x6": 2.0 ** -22}
P_F16 = 2.0 ** -21 + 2.0 ** -23
GUARD = 24        # guard rows: more than a tile's 18 input rows


def f16(prec):
    return prec.startswith("f16x3")


def p_term(prec):
    return P_F16 if f16(prec) else P_TERM[prec]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: cached references are read-only


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _tower(L, seed, opts):
    from scenedepthestimation_amd import ops
    hw, hb = tl.weights(L, seed, **dict(opts))
    return hw, hb, dev(ops.pack_tower_weights(hw, hb))


def tower(L, seed=None, **opts):
    return _tower(L, 40 + L if seed is None else seed, tuple(sorted(opts.items())))


def image(kind, L, H, W, gain=1.0):
    if kind == "spike":
        return tl.spike(L, H, W, 100 * H + W, (H // 2, W // 3))
    if kind == "zero":
        return tl.zero(L, H, W)
    return tl.gaussian(L, H, W, 100 * H + W, gain)


@functools.lru_cache(maxsize=None)
def oracle_features(L, H, W, kind, seed, opts):
    import oracle
    oracle.build()
    hw, hb, _ = _tower(L, seed, opts)
    ref = oracle.tower_forward(image(kind, L, H, W), hw, hb)
    ref.setflags(write=False)
    return ref


def kernel_of(prec, layer, L, lin, lout, emit):
    """launch_layer's choice of kernel family."""
    if not f16(prec):
        return "mfma32" if prec == "fp32" else "x6p-bf16"
    if prec == "f16x3w" and layer >= 3 and not emit:
        return "wino"
    if prec == "f16x3m32" or (layer == 2 and layer == L):
        return "x6p-f16"
    if layer >= 3 and lin == "split" and layer < L:
        return "h16q"
    if layer >= 3 and prec != "f16x3t32" and "split" not in (lin, lout) and not emit:
        return "h16s"
    return "h16"


def run_layer(x, packed, L, layer, prec, lin, lout, words, emit=None, out=None):
    from scenedepthestimation_amd import ops
    sh = 4 if layer == 2 else 2
    y = out if out is not None else torch.full((x.shape[0] - sh, x.shape[1] - sh, 64), float("nan"), device="cuda")
    ops.tower_layer(x, packed, L, layer, y, precision=prec, split=emit if layer == L else None,
                    in_cblock=lin == "cb", out_cblock=lout == "cb", in_split=lin == "split", out_split=lout == "split",
                    in_absmax=words[layer - 2:layer - 1], out_absmax=words[layer - 1:layer] if layer < L else None)
    return y


def decode(y, layout, scale=None):
    if layout == "cb":
        return tl.cblock_decode(y)
    if layout == "split":
        return tl.split_decode(y, scale)
    return y


def split_scale(bound):
    """2^sigma with bound 2^sigma in [2^14, 2^15) (tower_common.h xp_sigma)."""
    return 2.0 ** (14 - int(np.floor(np.log2(bound))))


def through_split(v, s):
    """What the split planes hold of the float32 value v: (fp16(v s) + fp16(v s - hi)) / s."""
    t = float(v) * float(s)
    hi = float(np.float16(t))
    return (hi + float(np.float16(t - hi))) / float(s)


def encode(x, layout, words, word):
    """x [h, w, 64] float32 in the input layout of a layer whose input bound word is words[word]."""
    words[word] = float(np.abs(x).max())
    if layout == "cb":
        return tl.cblock_encode(x)
    if layout == "split":
        s = split_scale(float(np.abs(x).max()))
        words[word + 32] = s
        return tl.split_encode(x, s)
    return x


# ---------------------------------------------------------------------------------------------------------------
# A. per-channel biases against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------
def all_precisions():
    from scenedepthestimation_amd import ops
    return sorted(ops.TOWER_PRECISIONS)


@pytest.mark.parametrize("kind", ["gaussian", "spike"])
@pytest.mark.parametrize("L", [5, 3, 2, 1])
def test_forward_signed_biases_vs_oracle(gpu, L, kind):
    from scenedepthestimation_amd import ops
    hw, hb, packed = tower(L)
    for H, W in SIZES:
        ref = oracle_features(L, H, W, kind, 40 + L, ())
        img = dev(image(kind, L, H, W))
        for prec in all_precisions():
            out = host(ops.tower_forward(img, packed, L, precision=prec))
            err = float(np.abs(out - ref).max())
            print(f"A {prec} L={L} {H}x{W} {kind}: {err:.3e}")
            assert np.isfinite(out).all() and err < 1e-5, (prec, L, H, W, kind, err)


@pytest.mark.parametrize("scale", [1e-6, 1e12])
def test_forward_signed_biases_scaled(gpu, scale):
    from scenedepthestimation_amd import ops
    L, H, W = 5, 17, 33
    _, _, packed = tower(L, scale=scale)
    ref = oracle_features(L, H, W, "gaussian", 40 + L, (("scale", scale),))
    for prec in [p for p in all_precisions() if f16(p)]:
        out = host(ops.tower_forward(dev(image("gaussian", L, H, W)), packed, L, precision=prec))
        assert np.isfinite(out).all() and np.abs(out - ref).max() < 1e-5, (prec, scale)


# (precision, layouts of the outputs of layers 2 .. L - 1, emit the planes)
def chains(L):
    if L == 2:
        return [(p, (), False) for p in all_precisions()]
    if L == 3:
        c = [(p, (lay,), e) for p in all_precisions() if p != "fp32" for lay in ("hw", "cb") for e in (False, True)]
        return c + [("fp32", ("hw",), False), ("fp32", ("hw",), True), ("f16x3", ("split",), False),
                    ("f16x3", ("split",), True)]
    assert L == 5
    c = [(p, lays, False) for p in all_precisions() if p != "fp32"
         for lays in (("hw",) * 3, ("cb",) * 3, ("hw", "cb", "hw"), ("cb", "hw", "cb"))]
    return c + [("fp32", ("hw",) * 3, False), ("f16x3", ("split",) * 3, False)]


def run_chain(img, packed, L, prec, lays, emit, H, W):
    """Layer by layer through the layer API: [(layer, input array, decoded output, raw words)], and the planes."""
    from scenedepthestimation_amd import ops
    words = torch.zeros(64, device="cuda")
    x = dev(img)
    ops.absmax(x, words[0:1])
    lay = {1: "hw", L: "hw", **{k + 2: v for k, v in enumerate(lays)}}
    planes = ops.new_split(H, W, "cuda") if emit else None
    steps, xin = [], img
    for layer in range(2, L + 1):
        y = run_layer(x, packed, L, layer, prec, lay[layer - 1], lay[layer], words, emit=planes)
        w = host(words)
        out = decode(host(y), lay[layer], w[layer - 1 + 32])
        steps.append((layer, xin, out, w.copy(), lay[layer - 1], lay[layer]))
        x, xin = y, out
    return steps, planes


@pytest.mark.parametrize("L", [5, 3, 2])
def test_layer_chains_vs_oracle(gpu, L):
    """Every layer-API chain (mixed layouts, split activations, emitted planes) with signed biases, at a size that is
    no tile multiple; a dead channel in layer L - 1 (layer 1 for L = 2) is exactly 0 and the next layer still matches."""
    from scenedepthestimation_amd import ops
    H, W = 17, 33
    dl, dc = max(L - 1, 1), 37
    for opts in ((), (("dead", (dl, dc)),)):
        hw, hb, packed = tower(L, **dict(opts))
        ref = oracle_features(L, H, W, "gaussian", 40 + L, opts)
        img = image("gaussian", L, H, W)
        for prec, lays, emit in chains(L):
            steps, planes = run_chain(img, packed, L, prec, lays, emit, H, W)
            feats = steps[-1][2]
            err = float(np.abs(feats - ref).max())
            assert err < 1e-5, (prec, lays, emit, opts, err)
            if opts and dl >= 2:
                dead = steps[dl - 2][2]
                assert not dead[..., dc].any() and dead[..., dc - 1].any(), (prec, lays)
            if emit:
                again = ops.feature_split(dev(feats))
                assert torch.equal(planes[0], again[0]) and torch.equal(planes[1], again[1]), (prec, lays)
                n = np.sqrt((feats.astype(np.float64) ** 2).sum(-1))
                assert np.all(host(planes[2]) >= n) and np.all(host(planes[2]) <= n * 1.00001 + 1e-30)


def test_rejected_flag_combinations(gpu):
    """What no kernel exists for is refused with a non-zero status, not run on another kernel."""
    from scenedepthestimation_amd import _lib, ops
    L, H, W = 4, 5, 7
    _, _, packed = tower(L)
    x = torch.zeros((H + 4, W + 4, 64), device="cuda")
    y = torch.zeros((H + 2, W + 2, 64), device="cuda")
    words = torch.zeros(64, device="cuda")
    words[1 + 32] = 1.0                              # a split input's scale word

    def status(prec, **lay):
        flags = ops._layout_flags(ops.TOWER_PRECISIONS[prec], lay.get("icb", False), lay.get("ocb", False),
                                  lay.get("isp", False), lay.get("osp", False))
        return _lib.lib.sde_tower_layer_scaled(x.data_ptr(), H + 4, W + 4, packed.data_ptr(), L, 64, 3, y.data_ptr(),
                                               flags, None, None, None, words[1:2].data_ptr(), words[2:3].data_ptr(),
                                               None)
    assert status("fp32", icb=True) != 0 and status("fp32", ocb=True) != 0
    assert status("bf16x6", isp=True, osp=True) != 0 and status("f16x3w", isp=True, osp=True) != 0
    assert status("f16x3m32", isp=True, osp=True) != 0
    assert status("f16x3", isp=True) != 0 and status("f16x3", osp=True) != 0      # a middle layer reads iff it writes
    assert status("f16x3", isp=True, icb=True, osp=True) != 0
    assert status("f16x3", isp=True, osp=True) == 0 and status("f16x3", icb=True) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# B. one layer at a time against fp64
# ---------------------------------------------------------------------------------------------------------------
REFS = {}


def layer_reference(x, hw, hb, layer, L):
    """(fp64 output, S, float32 output, conv1's error bound carried through layer 2) of `layer` from the input x, kept
    per input: chains that differ in layout only hand their layers the same bytes."""
    key = (id(hw), layer, L, x.shape, x.dtype.str, x.tobytes())
    if key not in REFS:
        w, b, last = hw[layer - 1], hb[layer - 1], layer == L
        if layer == 2:
            a1, S1 = tl.layer(x, hw[0], hb[0], False)
            ref, S = tl.layer(a1, w, b, last)
            o32 = tl.layer32(tl.layer32(x, hw[0], hb[0], False), w, b, last)
            REFS[key] = (ref, S, o32, tl._conv(10 * EPS * S1, np.abs(w), np.float64))
        else:
            ref, S = tl.layer(x, w, b, last)
            REFS[key] = (ref, S, tl.layer32(x, w, b, last), 0.0)
    return REFS[key]


def layer_errors(img, xin, out, hw, hb, layer, L, lout, scale):
    """(err / D, err32 / D, extra / D, split allowance / D) per element for the kernel's output `out` of `layer`
    from its own input (the image for layer 2, conv1 being fused into it)."""
    last = layer == L
    ref, S, o32, extra = layer_reference(img if layer == 2 else xin, hw, hb, layer, L)
    allow = np.abs(ref) * 2.0 ** -22 + 2.0 ** -25 / scale if lout == "split" else 0.0
    if not last:
        return np.abs(out - ref) / S, np.abs(o32 - ref) / S, extra / S, allow / S
    n = np.maximum(np.sqrt((ref * ref).sum(-1, keepdims=True)), 1e-6)
    f = tl.normalise(ref)
    D = (S + np.abs(f) * np.sqrt((S * S).sum(-1, keepdims=True))) / n
    ss = (o32 * o32).sum(-1, keepdims=True, dtype=np.float32)
    f32 = o32 / np.sqrt(np.maximum(ss, np.float32(1e-12)))
    if layer == 2:
        extra = (extra + np.abs(f) * np.sqrt((extra * extra).sum(-1, keepdims=True))) / n
    return np.abs(out - f) / D, np.abs(f32.astype(np.float64) - f) / D, extra / D, 0.0


RHO = {}     # (kernel, kind) -> [rho, rho32] maxima, printed for DESIGN.md 3.2


def check_layer(prec, kern, img, step, hw, hb, L, tag):
    layer, xin, out, words, lin, lout = step
    kind = "first+last" if L == 2 else "first" if layer == 2 else "last" if layer == L else "middle"
    r, r32, extra, allow = layer_errors(img, xin, out, hw, hb, layer, L, lout, words[layer - 1 + 32])
    K = 9 * 64 + 1 + (68 if layer == L else 0)
    rho, rho32, p = float(r.max()), float(r32.max()), p_term(prec)
    rec = RHO.setdefault((kern, kind), [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], rho), max(rec[1], rho32)
    print(f"B {kern} {prec} {kind} layer {layer}/{L} {lin}->{lout} {tag}: rho {rho:.3e} rho32 {rho32:.3e} "
          f"ratio {rho / rho32:.2f}")
    assert np.isfinite(out).all()
    assert (r <= K * EPS + p + extra + allow).all(), ("hard", kern, prec, kind, tag, rho)
    if kern != "wino":
        assert (r <= 4 * rho32 + p + allow).all(), ("tight", kern, prec, kind, tag, rho, rho32)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("L", [5, 3, 2])
def test_each_layer_vs_fp64(gpu, L, H, W):
    hw, hb, packed = tower(L)
    img = image("gaussian", L, H, W)
    for prec, lays, emit in chains(L):
        if emit and (H, W) != (17, 33):
            continue                                   # the planes' epilogues: one size that is no tile multiple
        steps, _ = run_chain(img, packed, L, prec, lays, emit, H, W)
        for step in steps:
            kern = kernel_of(prec, step[0], L, step[4], step[5], emit and step[0] == L)
            check_layer(prec, kern, img, step, hw, hb, L, f"{H}x{W}")
    for (kern, kind), (rho, rho32) in sorted(RHO.items()):
        print(f"B table {kern:9s} {kind:10s} rho {rho:.2e} rho32 {rho32:.2e} ratio {rho / rho32:.2f}")


# ---------------------------------------------------------------------------------------------------------------
# C. the bound word is the maximum of what was stored, bit for bit
# ---------------------------------------------------------------------------------------------------------------
MID = [(p, i, o) for p in ("f16x3", "f16x3t32", "f16x3w", "f16x3m32") for i in ("hw", "cb") for o in ("hw", "cb")] + \
    [("f16x3", "split", "split")]
FIRST = [("f16x3", "hw"), ("f16x3", "cb"), ("f16x3", "split"), ("f16x3w", "cb"), ("f16x3t32", "hw"),
         ("f16x3m32", "hw"), ("f16x3m32", "cb")]
LC = 4            # C's tower: layer 2 first, layer 3 middle


@functools.lru_cache(maxsize=None)
def mid_input(hout, wout):
    """A layer-3 input of (hout + 2) x (wout + 2): the literal's layer-2 activations of a Gaussian image."""
    hw, hb, _ = tower(LC)
    acts, _ = tl.layers(tl.gaussian(LC, hout - 2, wout - 2, hout * wout), hw, hb)
    x = acts[1].astype(np.float32)
    x.setflags(write=False)
    return x


def run_mid(x, prec, lin, lout, layer=3):
    """One middle layer of C's tower from the activation x: (decoded output, bound word, raw output, words)."""
    _, _, packed = tower(LC)
    w = np.zeros(64, np.float32)
    xe = encode(x, lin, w, layer - 2)
    words = dev(w)
    y = host(run_layer(dev(xe), packed, LC, layer, prec, lin, lout, words))
    w = host(words)
    return decode(y, lout, w[layer - 1 + 32]), w[layer - 1], y, w


def assert_word_is_max(prec, lin, lout, x, what):
    out, word, _, w = run_mid(x, prec, lin, lout)
    assert np.isfinite(out).all()
    if lout == "split":
        hw_out, hw_word, _, _ = run_mid(x, prec, "hw" if lin == "split" else lin, "hw")
        s = w[2 + 32]
        assert s == 2.0 ** round(np.log2(s)) and np.abs(out * s).max() < 2.0 ** 15
        if lin != "split":
            assert bits(word) == bits(hw_word), (prec, lin, lout, what)
        assert bits(hw_word) == bits(hw_out.max()), (prec, lin, lout, what)
        ref = hw_out.astype(np.float64)
        if lin != "split":
            assert (np.abs(out - ref) <= ref * 2.0 ** -22 + 2.0 ** -25 / s).all()
        # the split is monotone: the planes of the largest fp32 output are the largest stored value
        assert through_split(word, s) == out.max(), (prec, lin, what, float(word), out.max())
        return
    assert bits(word) == bits(out.max()), (prec, lin, lout, what, float(word), float(out.max()))


@pytest.mark.parametrize("hout,wout", SIZES)
def test_bound_word_middle_layers(gpu, hout, wout):
    """Gaussian activations, then a spike that puts the largest output on each of spike_targets' places: a word that
    misses a partial tile, a seam column, the last tile, or takes in an out-of-image lane differs from the stored
    maximum (by an exponent where the spike is missed)."""
    hw, hb, _ = tower(LC)
    x = mid_input(hout, wout)
    spiked = {}
    for target in sorted(set(tl.spike_targets(hout, wout, 16)) | set(tl.spike_targets(hout, wout, 32))):
        spiked[target], _ = tl.spiked_activation(x, hw[2], hb[2], target)
        y, _ = tl.layer(spiked[target], hw[2], hb[2], False)
        assert tl.spike_condition(y, target), target
    for prec, lin, lout in MID:
        assert_word_is_max(prec, lin, lout, x, "gaussian")
        tx = 16 if kernel_of(prec, 3, LC, lin, lout, False) in ("h16s", "wino") else 32     # the family's tile width
        for target in tl.spike_targets(hout, wout, tx):
            assert_word_is_max(prec, lin, lout, spiked[target], target)


@pytest.mark.parametrize("hout,wout", [(5, 7), (17, 33), (33, 49)])
def test_bound_word_ignores_lanes_outside_the_output(gpu, hout, wout):
    """A spike on the input's last column, last row and last pixel, in a channel whose strongest response falls on
    pixels past the output's edge: the lanes of the partial tiles that compute those pixels hold values above every
    stored one (test_tower_host checks that), and the word is still the stored maximum."""
    hw, hb, _ = tower(LC)
    x = mid_input(hout, wout)
    for where in ("right", "bottom", "corner"):
        xs, _ = tl.edge_spiked_activation(x, hw[2], where)
        wide = np.zeros((hout + 4, wout + 4, 64), np.float32)
        wide[:hout + 2, :wout + 2] = xs
        rim, _ = tl.layer(wide, hw[2], hb[2], False)
        assert rim.max() >= 1.25 * rim[:hout, :wout].max(), where
        for prec, lin, lout in MID:
            assert_word_is_max(prec, lin, lout, xs, where)


def run_first(img, prec, lout):
    _, _, packed = tower(LC)
    words = torch.zeros(64, device="cuda")
    words[0] = float(np.abs(img).max())
    y = host(run_layer(dev(img), packed, LC, 2, prec, "hw", lout, words))
    w = host(words)
    return decode(y, lout, w[1 + 32]), w[1], w


@pytest.mark.parametrize("hout,wout", SIZES)
def test_bound_word_layer2(gpu, hout, wout):
    """Layer 2 (conv1 fused): a Gaussian input, and a 2^20 spike in the first and the last input pixel, which reach
    only the first and the last output (the 5 x 5 footprint of conv1 + conv2 puts any other spike's largest outputs on
    25 pixels: no single-tile placement exists away from the corners)."""
    hw, hb, _ = tower(LC)
    inputs = [("gaussian", tl.gaussian(1, hout + 2, wout + 2, hout + wout), None)]
    for corner, target in (((0, 0), (0, 0)), ((hout + 3, wout + 3), (hout - 1, wout - 1))):
        inputs.append((corner, tl.corner_spike(hout + 4, wout + 4, corner), target))
    for what, img, target in inputs:
        if target is not None:
            y, _ = tl.layer(tl.layer(img, hw[0], hb[0], False)[0], hw[1], hb[1], False)
            assert tl.spike_condition(y, target), what
        res = {(p, lo): run_first(img, p, lo) for p, lo in FIRST}
        for (prec, lout), (out, word, w) in res.items():
            assert np.isfinite(out).all()
            if lout == "split":
                assert bits(word) == bits(res[(prec, "hw")][1]), (prec, what)
                assert through_split(word, w[1 + 32]) == out.max(), (prec, what)
                ref = res[(prec, "hw")][0].astype(np.float64)
                assert (np.abs(out - ref) <= ref * 2.0 ** -22 + 2.0 ** -25 / w[1 + 32]).all()
            else:
                assert bits(word) == bits(out.max()), (prec, lout, what, float(word), float(out.max()))


@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("order", ["dim first", "bright first"])
def test_bound_word_pair_of_gains(gpu, order, g):
    """Two images per launch, one 2^12 times dimmer, the brighter one spiked on its last pixel: each image's word is
    the maximum of its own outputs (a flush at the wrong image, or none, gives the dim image the bright word).  On
    the default grid every workgroup has one tile; capped to one workgroup (g = 1) the same waves cross from image 0
    to image 1 and flush the running maximum at the change."""
    from scenedepthestimation_amd import ops
    hout, wout = 17, 33
    hw, hb, packed = tower(LC)
    x = mid_input(hout, wout)
    xs, _ = tl.spiked_activation(x, hw[2], hb[2], (hout - 1, wout - 1))
    pair = [x * np.float32(2.0 ** -12), xs] if order == "dim first" else [xs, x * np.float32(2.0 ** -12)]
    for prec, lin, lout in MID:
        w = np.zeros((2, 64), np.float32)
        enc = np.stack([encode(a, lin, w[i], 1) for i, a in enumerate(pair)])
        words = dev(w)
        y = torch.full((2, hout, wout, 64), float("nan"), device="cuda")
        try:
            ops.set_persistent_grid(g)
            ops.tower_layer_batch(dev(enc), packed, LC, 3, y, precision=prec, in_cblock=lin == "cb",
                                  out_cblock=lout == "cb", in_split=lin == "split", out_split=lout == "split",
                                  in_absmax=words[:, 1:2], out_absmax=words[:, 2:3])
            torch.cuda.synchronize()
        finally:
            ops.set_persistent_grid(0)
        y, w = host(y), host(words)
        for i in range(2):
            out = decode(y[i], lout, w[i, 2 + 32])
            single, sword, _, _ = run_mid(pair[i], prec, lin, lout)
            assert np.array_equal(out, single) and bits(w[i, 2]) == bits(sword), (prec, lin, lout, i)
            if lout != "split":
                assert bits(w[i, 2]) == bits(out.max()), (prec, lin, lout, i)
        assert w[0, 2] != w[1, 2]


@pytest.mark.parametrize("case", ["zero image, non-positive biases", "zero image, zero conv1 bias"])
def test_bound_word_of_all_zero_outputs(gpu, case):
    """Nothing positive anywhere: the words stay 0, nothing is non-finite, and the layer after the zero activations
    gives its biases through the ReLU, exactly.  With conv1's bias zero and a zero image layer 2 gives its own."""
    from scenedepthestimation_amd import ops
    L, H, W = 5, 17, 33
    opts = {"nonpositive_bias": 3} if case.startswith("zero image, non") else {"zero_first_bias": True}
    hw, hb, packed = tower(L, **opts)
    img = tl.zero(L, H, W)
    for prec, lays, emit in chains(L):
        steps, _ = run_chain(img, packed, L, prec, lays, emit, H, W)
        for layer, _, out, w, _, lout in steps:
            assert np.isfinite(out).all()
            if "non-positive" in case and layer <= 3:
                assert not out.any() and (not f16(prec) or w[layer - 1] == 0), (prec, lays, layer)
            if ("non-positive" in case and layer == 4) or ("conv1" in case and layer == 2):
                want = np.maximum(hb[layer - 1], 0)
                if lout == "split":      # the planes hold 22 bits of a bias
                    assert (np.abs(out - want) <= want * 2.0 ** -22 + 2.0 ** -25 / w[layer - 1 + 32]).all()
                else:
                    assert (out == want).all(), (prec, lays, layer)
                if f16(prec):
                    assert bits(w[layer - 1]) == bits(want.max())
        ref = oracle_features(L, H, W, "zero", 40 + L, tuple(sorted(opts.items())))
        assert np.abs(steps[-1][2] - ref).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# D. guards
# ---------------------------------------------------------------------------------------------------------------
def guarded(arrs):
    """The arrays (one per image, same shape) as slices in the middle of one taller allocation whose other rows hold
    +-8 max |input|: (allocation, view [N, rows, ...] with the allocation's image stride)."""
    a = np.stack(arrs)
    rows = a.shape[1]
    poison = np.float32(8 * max(float(np.abs(a).max()), 1.0))
    big = np.empty((a.shape[0], rows + 2 * GUARD) + a.shape[2:], np.float32)
    big.reshape(-1)[0::2] = poison
    big.reshape(-1)[1::2] = -poison
    big[:, GUARD:GUARD + rows] = a
    big = dev(big)
    return big, big[:, GUARD:GUARD + rows]


def guarded_out(N, h, w, gap):
    """An output of N images of [h, w, 64] inside a buffer of 0xA5 bytes: guard rows above and below (and, with `gap`,
    between the images)."""
    rows = h + 2 * GUARD
    raw = torch.full(((N * rows if gap else N * h + 2 * GUARD) * w * 64 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    f = raw.view(torch.float32)
    if gap:
        return raw, f.view(N, rows, w, 64)[:, GUARD:GUARD + h]
    return raw, f.view(N * h + 2 * GUARD, w, 64)[GUARD:GUARD + N * h].view(N, h, w, 64)


def batch_layer(xv, packed, L, layer, yv, prec, lin, lout, words):
    """sde_tower_layer_batch on views with strides of their own (ops.tower_layer_batch takes contiguous tensors)."""
    from scenedepthestimation_amd import _lib, ops
    N, Hin, Win = xv.shape[:3]
    flags = ops._layout_flags(ops.TOWER_PRECISIONS[prec], lin == "cb", lout == "cb", lin == "split", lout == "split")
    assert xv[0].is_contiguous() and yv[0].is_contiguous()
    in_stride = xv.stride(0) if N > 1 else xv[0].numel()
    out_stride = yv.stride(0) if N > 1 else yv[0].numel()
    st = _lib.lib.sde_tower_layer_batch(xv.data_ptr(), N, in_stride, Hin, Win, packed.data_ptr(), L, 64, layer,
                                        yv.data_ptr(), out_stride, flags, words[:, layer - 2:].data_ptr(),
                                        words[:, layer - 1:].data_ptr() if layer < L else None, words.stride(0),
                                        ops._stream())
    assert st == 0, (st, prec, lin, lout, layer)


def guard_case(arrs, L, layer, prec, lin, lout, what):
    """The launch on guarded buffers against the same launch on plain ones: same bytes out, same words, guards kept."""
    _, _, packed = tower(L)
    N, last = len(arrs), layer == L
    w = np.zeros((N, 64), np.float32)
    enc = [encode(a, lin, w[i], layer - 2) if layer > 2 else a for i, a in enumerate(arrs)]
    for i, a in enumerate(arrs):
        w[i, layer - 2] = float(np.abs(a).max())
    sh = 4 if layer == 2 else 2
    h, wd = arrs[0].shape[0] - sh, arrs[0].shape[1] - sh
    plain_w, guard_w = dev(w), dev(w)
    plain = torch.full((N, h, wd, 64), float("nan"), device="cuda")
    batch_layer(dev(np.stack(enc)), packed, L, layer, plain, prec, lin, lout, plain_w)
    big, xv = guarded(enc)
    raw, yv = guarded_out(N, h, wd, gap=not last)
    batch_layer(xv, packed, L, layer, yv, prec, lin, lout, guard_w)
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all(), (what, prec)
    assert torch.equal(yv, plain), (what, prec, lin, lout, layer)
    assert torch.equal(plain_w.view(torch.int32), guard_w.view(torch.int32)), (what, prec, lin, lout, layer)
    mask = torch.ones_like(raw, dtype=torch.bool)
    fm = mask.view(-1, 4)
    if last:
        fm.view(N * h + 2 * GUARD, wd * 64, 4)[GUARD:GUARD + N * h] = False
    else:
        fm.view(N, h + 2 * GUARD, wd * 64, 4)[:, GUARD:GUARD + h] = False
    assert bool((raw[mask] == 0xA5).all()), (what, prec, lin, lout, layer, "guard bytes written")
    if f16(prec) and not last and lout != "split":
        yh, wh = host(yv), host(guard_w)
        for i in range(N):
            assert bits(wh[i, layer - 1]) == bits(decode(yh[i], lout).max()), (what, prec, lin, lout, i)


GUARD_MID = MID + [("bf16x6", "hw", "hw"), ("bf16x6", "cb", "cb"), ("fp32", "hw", "hw")]
GUARD_LAST = [(p, i) for p in ("f16x3", "f16x3t32", "f16x3w", "f16x3m32", "bf16x6") for i in ("hw", "cb")] + \
    [("f16x3", "split"), ("fp32", "hw")]
GUARD_FIRST = FIRST + [("bf16x6", "hw"), ("bf16x6", "cb"), ("fp32", "hw")]


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("hout,wout", [(5, 7), (17, 33)])
def test_guard_rows_around_inputs_and_outputs(gpu, hout, wout, N):
    """Every family, first / middle / last layer, [h][w][64], c-block and split inputs, one image and a batch with the
    guards between its images: a lane that read past its image would take in the poison (8 x the largest input), one
    that stored past its output would change a guard byte.  Every buffer is the test's own."""
    x = mid_input(hout, wout)
    mids = [x, x[::-1, ::-1].copy() * np.float32(3)][:N]
    imgs = [tl.gaussian(1, hout + 2, wout + 2, 7 + i, gain=1 + 5 * i) for i in range(N)]
    for prec, lout in GUARD_FIRST:
        guard_case(imgs, LC, 2, prec, "hw", lout, "first")
    for prec, lin, lout in GUARD_MID:
        guard_case(mids, LC, 3, prec, lin, lout, "middle")
    for prec, lin in GUARD_LAST:
        guard_case(mids, 3, 3, prec, lin, "hw", "last")
    for prec in all_precisions():
        guard_case(imgs, 2, 2, prec, "hw", "hw", "first+last")


# ---------------------------------------------------------------------------------------------------------------
# E. capped grids
# ---------------------------------------------------------------------------------------------------------------
def run_tower_words(batch, packed, L, prec):
    from scenedepthestimation_amd import ops, pipeline
    N, Hp, Wp = batch.shape
    H, W = Hp - 2 * L, Wp - 2 * L
    nws = ops.tower_batch_workspace_bytes(H, W, N, L)
    ws = torch.zeros(max(nws, 1), dtype=torch.uint8, device="cuda")
    out = torch.full((N, H, W, 64), float("nan"), device="cuda")
    pipeline.run_tower(batch, packed, L, out, ws, prec)
    torch.cuda.synchronize()
    return out, ws[nws - N * 256:nws].clone()


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("L", [5, 3, 2])
def test_capped_grid_batches(gpu, L, g):
    """sde_set_persistent_grid(1..3): many tiles per workgroup at sizes that are no tile multiples -- image changes in
    mid-workgroup under different scales, the drain after the loop, the hand-over buffer reused.  Results do not depend
    on the grid: features and bound words are the bytes of the default grid, and each image's those of it run alone."""
    from scenedepthestimation_amd import ops
    _, _, packed = tower(L)
    a, b = image("gaussian", L, 33, 49), image("gaussian", L, 17, 33)
    batches = [dev(np.stack([a, a * np.float32(2.0 ** 12)])),
               dev(np.stack([b * np.float32(2.0 ** -10), b, b * np.float32(2.0 ** 12)]))]
    for batch in batches:
        for prec in all_precisions():
            ref = ops.tower_forward_batch(batch, packed, L, precision=prec)
            ref_lw, ref_words = run_tower_words(batch, packed, L, prec)
            alone = torch.stack([ops.tower_forward(batch[i].contiguous(), packed, L, precision=prec)
                                 for i in range(batch.shape[0])])
            try:
                ops.set_persistent_grid(g)
                out = ops.tower_forward_batch(batch, packed, L, precision=prec)
                lw, words = run_tower_words(batch, packed, L, prec)
                torch.cuda.synchronize()
            finally:
                ops.set_persistent_grid(0)
            assert torch.isfinite(out).all()
            assert torch.equal(out, ref) and torch.equal(out, alone) and torch.equal(lw, ref), (prec, L, g)
            assert torch.equal(words, ref_words), (prec, L, g)
            assert torch.equal(ref_lw, ref)


@pytest.mark.parametrize("g", [1, 3])
def test_capped_grid_split_chain(gpu, g):
    """The split-activation chain (conv64_h16_kernel FIRST -> conv64_h16q_kernel -> ... -> the split-input last layer)
    over a batch of three, through the layer API, under a capped grid: the bytes of the default grid."""
    from scenedepthestimation_amd import ops
    L, H, W = 5, 17, 33
    _, _, packed = tower(L)
    b = image("gaussian", L, H, W)
    batch = dev(np.stack([b * np.float32(2.0 ** -10), b, b * np.float32(2.0 ** 12)]))

    def chain():
        words = torch.zeros((3, 64), device="cuda")
        ops.absmax_batch(batch, words)
        x, outs = batch, []
        for layer in range(2, L + 1):
            sh = 4 if layer == 2 else 2
            y = torch.full((3, x.shape[1] - sh, x.shape[2] - sh, 64), float("nan"), device="cuda")
            ops.tower_layer_batch(x, packed, L, layer, y, precision="f16x3", in_split=layer > 2, out_split=layer < L,
                                  in_absmax=words[:, layer - 2:layer - 1],
                                  out_absmax=words[:, layer - 1:layer] if layer < L else None)
            outs.append(y)
            x = y
        torch.cuda.synchronize()
        return outs + [words]
    ref = chain()
    try:
        ops.set_persistent_grid(g)
        got = chain()
    finally:
        ops.set_persistent_grid(0)
    for r, o in zip(ref, got):
        assert torch.equal(r.view(torch.int32), o.view(torch.int32))
    assert torch.isfinite(got[-2]).all()


# ---------------------------------------------------------------------------------------------------------------
# F. inputs whose scale exponents differ
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 2])
def test_workspace_reuse_after_a_brighter_image(gpu, L):
    """A workspace that held the bound words of an image 2^20 times brighter gives the next image the bytes a fresh
    one does (the words are zeroed per call: a stale word would change every scale)."""
    from scenedepthestimation_amd import ops, pipeline
    H, W = 17, 33
    _, _, packed = tower(L)
    img = dev(image("gaussian", L, H, W))
    bright = img * 2.0 ** 20
    for prec in all_precisions():
        fresh = ops.tower_forward(img, packed, L, precision=prec)
        ws = torch.zeros(max(ops.tower_workspace_bytes(H, W, L), 1), dtype=torch.uint8, device="cuda")
        ops.tower_forward(bright, packed, L, workspace=ws, precision=prec)
        assert torch.equal(ops.tower_forward(img, packed, L, workspace=ws, precision=prec), fresh), prec
        ws2 = torch.zeros(max(ops.tower_batch_workspace_bytes(H, W, 1, L), 1), dtype=torch.uint8, device="cuda")
        out = torch.empty((1, H, W, 64), device="cuda")
        pipeline.run_tower(bright[None], packed, L, out, ws2, prec)
        pipeline.run_tower(img[None], packed, L, out, ws2, prec)
        torch.cuda.synchronize()
        assert torch.equal(out[0], fresh), prec


def test_matcher_reloaded_with_a_dimmer_pair(gpu):
    from scenedepthestimation_amd.pipeline import StereoMatcher
    H, W = 44, 37
    lit = np.zeros((H, W), np.uint8)
    lit[H // 2, W // 2] = 255                       # one lit pixel: the largest z-normalised value an image can have
    dark = tl.band_pair(H, W, seed=3)
    for prec in ("f16x3", "f16x3w"):
        m = StereoMatcher(H, W, 16, tower_precision=prec)
        m.load_images(lit, lit)
        m.features()
        m.load_images(*dark)
        m.features()
        fresh = StereoMatcher(H, W, 16, tower_precision=prec)
        fresh.load_images(*dark)
        fresh.features()
        torch.cuda.synchronize()
        assert torch.isfinite(m.feat2).all() and torch.equal(m.feat2, fresh.feat2), prec


@pytest.mark.parametrize("H,W,world", tl.BAND_CASES)
def test_row_bands_need_the_combined_words(gpu, H, W, world):
    """A dark pair with one bright block in the last band: the bands' image maxima differ by more than 4 x, so their
    own bound words give other scales than the whole image's.  With the words combined by MAX the bands are the full
    tower byte for byte; without the combine they are not (the control: this input sees a missing all-reduce).  A
    power-of-two scale alone changes no bit of an exact fp16 split; what differs is the low part of the activations
    more than 2^17 below the bound, which the coarser scale pushes into fp16's subnormals.  Those are a few in 10^5,
    so the images are 600 wide: 44 x 37 and 48 x 40 pairs gave the same bytes with and without the combine, 600-wide
    ones 3,774 to 21,266 other values (measured on MI355X)."""
    from test_gpu_configs import _band_features
    from scenedepthestimation_amd.parallel import row_band
    from scenedepthestimation_amd.pipeline import StereoMatcher, run_tower
    from scenedepthestimation_amd import ops
    L = 5
    _, _, packed = tower(L)
    for prec in ("f16x3", "f16x3w", "f16x3m32"):
        m = StereoMatcher(H, W, 16, tower_precision=prec)
        m.packed = packed
        m.load_images(*tl.band_pair(H, W, seed=H))
        m.features()
        assert torch.isfinite(m.feat2).all()
        assert torch.equal(_band_features(m, world, prec), m.feat2), prec
        # the control: every band on its own words
        diff = False
        for r in range(world):
            r0, r1, _ = row_band(H, world, r)
            ws = torch.empty(ops.tower_batch_workspace_bytes(r1 - r0, W, 2, L), dtype=torch.uint8, device="cuda")
            out = torch.empty((2, r1 - r0, W, 64), device="cuda")
            run_tower(m.img_pad2[:, r0:r1 + 2 * L].contiguous(), packed, L, out, ws, prec)
            torch.cuda.synchronize()
            diff = diff or not torch.equal(out, m.feat2[:, r0:r1])
        assert diff, (prec, "bands without the MAX combine equal the full tower: the input is not sensitive")


# ---------------------------------------------------------------------------------------------------------------
# G. the L2-norm floor
# ---------------------------------------------------------------------------------------------------------------
def test_norm_floor_zero_patch(gpu):
    """A zero block in the image, no positive bias below the last layer and none in it: the pixels whose receptive
    field is the block have all-zero activations, so their features are x / sqrt(1e-12) = 0 exactly, not 0 / 0, on
    every last-layer epilogue -- and the emitted hi / lo / norm planes are 0 there."""
    from scenedepthestimation_amd import ops
    L, H, W, y0, x0, size = 5, 24, 26, 4, 6, 15
    opts = {"zero_last_bias": True, "nonpositive_bias": True}
    hw, hb, packed = tower(L, **opts)
    img = tl.zero_patch(L, H, W, 2, y0, x0, size)
    ys, xs = tl.patch_interior(L, y0, x0, size)
    _, ref = tl.layers(img, hw, hb)
    assert not ref[ys, xs].any() and ref[0, 0].any()
    for prec in all_precisions():
        for emit in (False, True):
            planes = ops.new_split(H, W, "cuda") if emit else None
            out = host(ops.tower_forward(dev(img), packed, L, precision=prec, split=planes))
            assert np.isfinite(out).all() and not out[ys, xs].any(), (prec, emit)
            assert np.abs(out - ref).max() < 1e-5, (prec, emit)
            if emit:
                assert all(not host(p)[ys, xs].any() for p in planes), prec
    # the layer API's planes from split activations
    steps, planes = run_chain(img, packed, L, "f16x3", ("split",) * 3, True, H, W)
    assert not steps[-1][2][ys, xs].any() and all(not host(p)[ys, xs].any() for p in planes)
    assert np.abs(steps[-1][2] - ref).max() < 1e-5


@pytest.mark.parametrize("hout,wout", [(5, 7), (17, 33)])
def test_norm_floor_threshold(gpu, hout, wout):
    """Last-layer activations scaled so that sum x^2 straddles 1e-12 (the median pixel sits on it): below it the
    features are x * 1e6, above it x / ||x||, both within B's bound of the literal."""
    L = 3
    hw, hb, packed = tower(L, zero_last_bias=True)
    x = mid_input(hout, wout)
    y, _ = tl.layer(x, hw[2], hb[2], True)
    x = (x * np.float32(1e-6 / np.median(np.sqrt((y * y).sum(-1))))).astype(np.float32)
    y, _ = tl.layer(x, hw[2], hb[2], True)
    ss = (y * y).sum(-1)
    assert (ss < 0.9e-12).sum() >= 3 and (ss > 1.1e-12).sum() >= 3
    for prec, lin in GUARD_LAST:
        w = np.zeros(64, np.float32)
        xe = encode(x, lin, w, 1)
        words = dev(w)
        out = host(run_layer(dev(xe), packed, L, 3, prec, lin, "hw", words))
        kern = kernel_of(prec, 3, L, lin, "hw", False)
        xin = tl.split_decode(xe, w[1 + 32]) if lin == "split" else x
        check_layer(prec, kern, None, (3, xin, out, host(words), lin, "hw"), hw, hb, L, f"floor {hout}x{wout}")
        low = ss < 0.9e-12
        assert np.abs(out[low] - y[low] * 1e6).max() < 1e-5
