"""The conv tower written out in NumPy, in fp64: what test_tower_host.py pins to the C oracle on the CPU and
test_gpu_tower_epilogue.py compares the HIP kernels with.  Unlike mc_cnn.synthetic_weights (every bias 0.01) the
weights here carry a signed bias per channel and per layer, so a permuted, mis-layered or sign-dropping bias read,
a dead channel and the L2-norm floor all show."""
import numpy as np

NF = 64
NORM_FLOOR = 1e-12     # tf.nn.l2_normalize's epsilon: x / sqrt(max(sum x^2, 1e-12)) (oracle/sde_oracle.c)


def weights(L, seed, bias_std=0.3, dead=None, zero_last_bias=False, scale=1.0, nonpositive_bias=0,
            zero_first_bias=False):
    """He-normal HWIO weights like mc_cnn.synthetic_weights, biases ~ N(0, bias_std) per channel and layer.
    dead = (layer, channel): that channel's bias is -1e3 (dead after the ReLU for any image of ordinary size);
    zero_last_bias / zero_first_bias: layer L's / layer 1's biases are 0; nonpositive_bias = k: the biases of layers
    1 .. k are -|b| (True: of every layer); scale: weights and biases scaled
    as test_tower_f16x3_dynamic_range scales them (weights by scale^(1/L), layer k's biases by scale^(k/L)).
    Returns (hw, hb): lists of float32 arrays [3, 3, cin, 64] and [64]."""
    rng = np.random.default_rng(seed)
    hw, hb = [], []
    for k in range(1, L + 1):
        cin = 1 if k == 1 else NF
        w = (rng.standard_normal((3, 3, cin, NF)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        b = (rng.standard_normal(NF) * bias_std).astype(np.float32)
        if k <= (L if nonpositive_bias is True else int(nonpositive_bias)):
            b = -np.abs(b)
        if dead is not None and dead[0] == k:
            b[dead[1]] = np.float32(-1e3)
        if (zero_last_bias and k == L) or (zero_first_bias and k == 1):
            b[:] = 0
        hw.append(w * np.float32(scale ** (1 / L)))
        hb.append(b * np.float32(scale ** (k / L)))
    return hw, hb


def _conv(x, w, dtype):
    """3 x 3 VALID cross-correlation of x [h, w, cin] with w [3, 3, cin, nf], accumulated tap by tap in dtype (fp64: a
    matrix product per tap; float32: channel by channel within a tap, 9 cin sequential additions per output)."""
    x, w = x.astype(dtype), w.astype(dtype)
    ho, wo = x.shape[0] - 2, x.shape[1] - 2
    acc = np.zeros((ho, wo, w.shape[-1]), dtype)
    for ky in range(3):
        for kx in range(3):
            xs = x[ky:ky + ho, kx:kx + wo]
            if dtype == np.float32:
                # one product at a time, as a plain fp32 convolution's loop adds them (a BLAS product would keep
                # several partial sums and round less)
                for c in range(x.shape[2]):
                    acc += xs[:, :, c, None] * w[ky, kx, c]
            else:
                acc += xs @ w[ky, kx]
    return acc


def layer(x_f32, w, b, last, dtype=np.float64):
    """One layer from a given input [h, w, cin] (or [h, w] for layer 1): (out, S) with out = conv + bias (ReLU unless
    last) and S = |W| (*) |x| + |b|, the sum of the absolute values of everything added into an output."""
    x = np.asarray(x_f32)
    if x.ndim == 2:
        x = x[:, :, None]
    out = _conv(x, w, dtype) + b.astype(dtype)
    if not last:
        out = np.maximum(out, 0)
    S = _conv(np.abs(x), np.abs(w), np.float64) + np.abs(b.astype(np.float64))
    return out, S


def layer32(x_f32, w, b, last):
    """The same layer in plain float32, accumulated tap by tap: the yardstick of what fp32 arithmetic gives."""
    return layer(x_f32, w, b, last, dtype=np.float32)[0]


def normalise(x):
    """x / sqrt(max(sum_c x^2, 1e-12)) in fp64."""
    x = np.asarray(x, np.float64)
    ss = (x * x).sum(-1, keepdims=True)
    return x / np.sqrt(np.maximum(ss, NORM_FLOOR))


def layers(img_pad, hw, hb):
    """(acts, feats): acts[l - 1] is layer l's fp64 output (ReLU on l < L, none on L), feats the L2-normalised
    features, from the padded image [H + 2L, W + 2L]."""
    x, acts = np.asarray(img_pad, np.float64), []
    for k, (w, b) in enumerate(zip(hw, hb), start=1):
        x, _ = layer(x, w, b, last=k == len(hw))
        acts.append(x)
    return acts, normalise(x)


# ---------------------------------------------------------------------------------------------------------------
# activation layouts (a tensor keeps its [h, w, 64] float32 shape in every layout; only the byte order differs)
# ---------------------------------------------------------------------------------------------------------------
def cblock_decode(buf):
    """c-block-major [4][h][w][16] stored in an [h, w, 64] float32 array -> [h, w, 64]."""
    h, w, _ = buf.shape
    return buf.reshape(4, h, w, 16).transpose(1, 2, 0, 3).reshape(h, w, NF)


def cblock_encode(x):
    h, w, _ = x.shape
    return np.ascontiguousarray(x.reshape(h, w, 4, 16).transpose(2, 0, 1, 3)).reshape(h, w, NF)


def split_decode(buf, s):
    """Split planes [cblk32 2][part 2][q 4][h][w][8 fp16] stored in an [h, w, 64] float32 array, with the scale
    s = 2^sigma the writer published at its bound word + 32 -> (hi + lo) / s as fp64 [h, w, 64]."""
    h, w, _ = buf.shape
    planes = np.ascontiguousarray(buf).view(np.float16).reshape(2, 2, 4, h, w, 8).astype(np.float64)
    return (planes[:, 0] + planes[:, 1]).transpose(2, 3, 0, 1, 4).reshape(h, w, NF) / s


def split_encode(x, s):
    """fp64 / fp32 [h, w, 64] -> the planes of hi = fp16(x s), lo = fp16(x s - hi), as an [h, w, 64] float32 array."""
    h, w, _ = x.shape
    v = np.asarray(x, np.float64) * s
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float64)).astype(np.float16)
    parts = np.stack([hi, lo]).reshape(2, h, w, 2, 4, 8).transpose(3, 0, 4, 1, 2, 5)     # [cb][part][q][h][w][8]
    return np.ascontiguousarray(parts).view(np.float32).reshape(h, w, NF)


# ---------------------------------------------------------------------------------------------------------------
# images: float32 [H + 2L, W + 2L] with a zero halo of L pixels
# ---------------------------------------------------------------------------------------------------------------
def zero(L, H, W):
    return np.zeros((H + 2 * L, W + 2 * L), np.float32)


def gaussian(L, H, W, seed, gain=1.0):
    img = zero(L, H, W)
    img[L:L + H, L:L + W] = np.random.default_rng(seed).standard_normal((H, W)).astype(np.float32) * np.float32(gain)
    return img


def spike(L, H, W, seed, pos, gain=2.0 ** 20):
    """A Gaussian image with one pixel (pos = (y, x) inside the H x W image) of value gain.  2^20 is the ratio a
    1024^2 u8 image with one lit pixel reaches after z-normalisation (sqrt(N) against 1 / sqrt(N))."""
    img = gaussian(L, H, W, seed)
    img[L + pos[0], L + pos[1]] = np.float32(gain)
    return img


def zero_patch(L, H, W, seed, y0, x0, size):
    """A Gaussian image with an all-zero size x size block at (y0, x0); size >= 2L + 3 leaves pixels whose whole
    receptive field is zero."""
    assert size >= 2 * L + 3 and y0 + size <= H and x0 + size <= W
    img = gaussian(L, H, W, seed)
    img[L + y0:L + y0 + size, L + x0:L + x0 + size] = 0
    return img


def patch_interior(L, y0, x0, size):
    """Feature-map slices of the pixels whose (2L + 1)^2 receptive field lies inside zero_patch's block."""
    return slice(y0 + L, y0 + size - L), slice(x0 + L, x0 + size - L)


BAND_CASES = [(44, 600, 2), (48, 600, 3)]      # H, W, world of the row-band tests


def band_pair(H, W, seed):
    """A u8 pair, dark (0..20) apart from a 3 x 3 block of 255 in the last rows: after z-normalisation the rows
    above the block stay far below the global maximum, so row bands measure different bound words."""
    rng = np.random.default_rng(seed)
    pair = rng.integers(0, 21, (2, H, W)).astype(np.uint8)
    pair[:, H - 5:H - 2, W // 2:W // 2 + 3] = 255
    return pair[0], pair[1]


def znorm_pad(img_u8, L):
    x = img_u8.astype(np.float64)
    z = (x - x.mean()) / x.std()
    out = np.zeros((x.shape[0] + 2 * L, x.shape[1] + 2 * L), np.float32)
    out[L:-L, L:-L] = z
    return out


# ---------------------------------------------------------------------------------------------------------------
# spiked activations: where a 64 -> 64 layer's largest output lands
# ---------------------------------------------------------------------------------------------------------------
def spiked_activation(x, w, b, target, gain_ratio=2.0 ** 12):
    """A copy of the activation x [h, w, 64] with one spiked element, placed so that the layer (w, b, ReLU) has
    its largest output at the output pixel `target`.  A spike at input pixel q reaches the 3 x 3 outputs q - 2 .. q:
    the spike goes to q = target + 1 clipped into the input (so every output it reaches lies in target's 3 x 3
    neighbourhood), in the input channel whose strongest response falls on `target`'s tap.  Returns (x', channel)."""
    h, wd, _ = x.shape
    ty, tx = target
    qy, qx = min(max(ty + 1, 0), h - 1), min(max(tx + 1, 0), wd - 1)
    ky, kx = qy - ty, qx - tx                          # the tap through which `target` sees the spike
    assert 0 <= ky < 3 and 0 <= kx < 3
    # taps through which outputs inside the layer's output see q
    taps = [(a, c) for a in range(3) for c in range(3) if 0 <= qy - a < h - 2 and 0 <= qx - c < wd - 2]
    best = None
    for c in range(NF):
        peak = {t: float(w[t[0], t[1], c].max()) for t in taps}
        others = max([v for t, v in peak.items() if t != (ky, kx)], default=0.0)
        margin = peak[(ky, kx)] - others
        if best is None or margin > best[0]:
            best = (margin, c)
    assert best[0] > 0, "no input channel puts its strongest response on the target"
    out = np.array(x, np.float32, copy=True)
    out[qy, qx, best[1]] = np.float32(np.abs(x).max() * gain_ratio)
    return out, best[1]


def spike_targets(hout, wout, tx):
    """The places test C puts a layer's largest output: first pixel, last pixel (of a partial corner tile), last
    column, last row, the tile seams in x (16 x `tx` tiles) and in y, and the first pixel of the last tile."""
    t = {(0, 0), (hout - 1, wout - 1), (hout // 2, wout - 1), (hout - 1, wout // 2),
         ((hout - 1) // 16 * 16, (wout - 1) // tx * tx)}
    t |= {(min(3, hout - 1), c) for c in (15, 16, 31, 32) if c < wout}
    t |= {(r, min(5, wout - 1)) for r in (15, 16, 31, 32) if r < hout}
    return sorted(t)


def spike_condition(y, target):
    """The largest output lies at `target` and is >= 4 x everything outside target's 3 x 3 neighbourhood."""
    m = y.max(-1)
    ty, tx = target
    if np.unravel_index(np.argmax(m), m.shape) != (ty, tx):
        return False
    rest = m.copy()
    rest[max(ty - 1, 0):ty + 2, max(tx - 1, 0):tx + 2] = 0
    return m[ty, tx] >= 4 * rest.max()


def corner_spike(Hin, Win, corner):
    """A Gaussian Hin x Win layer-2 input (no halo: the layer API takes any array) with 2^20 in one corner."""
    img = np.random.default_rng(Hin * Win).standard_normal((Hin, Win)).astype(np.float32)
    img[corner] = np.float32(2.0 ** 20)
    return img


def edge_spiked_activation(x, w, where, gain_ratio=2.0 ** 12):
    """A copy of x [h, w, 64] with a spike on its last column ("right"), last row ("bottom") or last pixel ("corner"),
    in the input channel whose response is strongest through a tap that lands OUTSIDE the (h - 2) x (w - 2) output:
    a lane of a partial tile that computes such a pixel holds a larger value than any stored one, so a bound word
    that takes in lanes outside the output is inflated.  Returns (x', q)."""
    h, wd, _ = x.shape
    q = {"right": (h // 2, wd - 1), "bottom": (h - 1, wd // 2), "corner": (h - 1, wd - 1)}[where]
    inside = [(a, c) for a in range(3) for c in range(3) if 0 <= q[0] - a < h - 2 and 0 <= q[1] - c < wd - 2]
    outside = [(a, c) for a in range(3) for c in range(3) if (a, c) not in inside]
    margin = [max(float(w[t[0], t[1], c].max()) for t in outside) - max(float(w[t[0], t[1], c].max()) for t in inside)
              for c in range(NF)]
    out = np.array(x, np.float32, copy=True)
    out[q[0], q[1], int(np.argmax(margin))] = np.float32(np.abs(x).max() * gain_ratio)
    return out, q
