"""The training arithmetic restated in torch on the CPU (float64 by default), written from the definition in
include/sde.h -- the reference the GPU training kernels are judged by.

    conv        out[y][x][co] = b[co] + sum in[y+ky][x+kx][ci] * w[ky][kx][ci][co]   (VALID), ReLU on all but the last
    normalise   y = x * r,  r = rsqrt(max(sum x^2, 1e-12))
    h_i = margin - l_i.p_i + l_i.n_i,   loss = mean_i max(0, h_i)

Gradients come from autograd through F.conv2d.  relu(z) is written z * [z > 0] and max(0, h) as h * [h > 0], so
the masks can be forced: with `relu_masks` / `hinge_mask` given, relu(z) -> z * mask and max(0, h) -> h * mask,
which makes the loss a smooth function of the parameters (finite differences) and lets a float32 computation be
compared on the very same branch decisions.
"""
import numpy as np
import torch
import torch.nn.functional as F


def var_names(nlayers):
    return [(f"conv{k}/weights:0", f"conv{k}/biases:0") for k in range(1, nlayers + 1)]


def run(patches, weights, nlayers, margin=0.3, relu_masks=None, hinge_mask=None, dtype=torch.float64, grads=True):
    """patches [3][B][P][P]; weights: dict of HWIO weights / biases.  relu_masks: list of nlayers - 1 arrays
    [3B][s][s][nf] (truthy = pass), hinge_mask: [B].  ->  dict with
        loss (float), h [B], feats [3B][nf], pre: the pre-activations z_k of layers 1..nlayers as [3B][s][s][nf],
        grads: {variable name: array} and dpre: d loss / d z_k, shaped as pre (if grads)."""
    patches = np.asarray(patches)
    B, P = patches.shape[1], patches.shape[2]
    params = {}
    for wn, bn in var_names(nlayers):
        params[wn] = torch.tensor(np.asarray(weights[wn]), dtype=dtype, requires_grad=grads)
        params[bn] = torch.tensor(np.asarray(weights[bn]), dtype=dtype, requires_grad=grads)
    x = torch.tensor(patches, dtype=dtype).reshape(3 * B, 1, P, P)
    pre, zs = [], []
    for k, (wn, bn) in enumerate(var_names(nlayers), start=1):
        z = F.conv2d(x, params[wn].permute(3, 2, 0, 1), params[bn])
        if grads:
            z.retain_grad()
            zs.append(z)
        pre.append(z.detach().permute(0, 2, 3, 1).numpy().copy())
        if k < nlayers:
            if relu_masks is not None:
                m = torch.tensor(np.asarray(relu_masks[k - 1]) != 0).permute(0, 3, 1, 2)
            else:
                m = z.detach() > 0
            x = z * m.to(dtype)
    z = z.reshape(3 * B, -1)
    r = torch.rsqrt(torch.clamp((z * z).sum(1, keepdim=True), min=1e-12))
    y = z * r
    l, p, n = y[:B], y[B:2 * B], y[2 * B:]
    h = margin - (l * p).sum(1) + (l * n).sum(1)
    hm = torch.tensor(np.asarray(hinge_mask) != 0) if hinge_mask is not None else h.detach() > 0
    loss = (h * hm.to(dtype)).mean()
    out = {"loss": float(loss.item()), "h": h.detach().numpy().copy(), "feats": y.detach().numpy().copy(), "pre": pre}
    if grads:
        loss.backward()
        out["grads"] = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(v.shape)) for k, v in params.items()}
        out["dpre"] = [z.grad.permute(0, 2, 3, 1).numpy().copy() for z in zs]
    return out


def gather_host(img_l, img_r, idx, patch: int) -> np.ndarray:
    """NumPy statement of sde_train_gather: slices of the zero-padded images -> [3][B][P][P]."""
    idx = np.asarray(idx, np.int64)
    r = patch // 2
    H, W = img_l.shape
    out = np.zeros((3, len(idx), patch, patch), np.float32)
    for which, img in enumerate((img_l, img_r, img_r)):
        for b, row in enumerate(idx):
            y, x = int(row[0]), int(row[1 + which])
            for py in range(patch):
                yy = y + py - r
                if not 0 <= yy < H:
                    continue
                x0, x1 = max(x - r, 0), min(x + r + 1, W)
                if x0 < x1:
                    out[which, b, py, x0 - (x - r):x1 - (x - r)] = img[yy, x0:x1]
    return out


def masks_of(result):
    """(relu masks of layers 1..L-1, hinge mask) a run took."""
    return [z > 0 for z in result["pre"][:-1]], result["h"] > 0


def momentum_np(p, v, g, lr, beta):
    """TF's non-Nesterov momentum in NumPy float32, one rounding per operation: v = fl(fl(beta*v) + g),
    p = fl(p - fl(lr*v)).  Every operand is a float32 array or scalar, so NumPy rounds after each operation."""
    p, v, g = (np.asarray(a, np.float32) for a in (p, v, g))
    lr, beta = np.float32(lr), np.float32(beta)
    bv = (beta * v).astype(np.float32)
    v = (bv + g).astype(np.float32)
    step = (lr * v).astype(np.float32)
    return (p - step).astype(np.float32), v


def train(patches, weights, nlayers, steps, margin=0.3, lr=1e-3, beta=0.9, factor=1, dtype=torch.float64):
    """`steps` momentum steps on one fixed batch at the learning rate float32(lr / factor).
    -> (weights after, [loss before each step])."""
    w = {k: np.asarray(v, np.float64) for k, v in weights.items()}
    vel = {k: np.zeros_like(v) for k, v in w.items()}
    rate = float(np.float32(lr / factor))
    losses = []
    for _ in range(steps):
        res = run(patches, w, nlayers, margin, dtype=dtype)
        losses.append(res["loss"])
        for k in w:
            vel[k] = beta * vel[k] + res["grads"][k]
            w[k] = w[k] - rate * vel[k]
    return w, losses
