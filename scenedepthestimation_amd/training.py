"""Training of the MC-CNN-fast branch on the device (the reference's train.py + data_generator.py).

  Trainer            device-resident parameters / velocity / gradients / workspace; one step = gather (optional),
                     forward + backward (sde_train_loss_grad) and the momentum update (sde_train_momentum), all
                     enqueued on the current stream with no read-back and no allocation
  TripletSampler     seeded host-side choice of (y, x_left, x_pos, x_neg) patch centres from a disparity map, by
                     the rule of the reference's patch preparation (image_patches_prepare/middlebury_2003.py:81-110)
  SceneSet           stereo scenes with ground truth resident on the device; its batches are drawn (counter-based
                     RNG) and gathered there in one launch, by the same rule (sde_triplet_centres,
                     sde_train_sample_gather): no host draw, no copy, no read-back per step
  PatchFileDataset   the reference's ImagePatchesGenerator over per-patch .pfm files (data_generator.py)

torch is plumbing here (device memory, streams): no torch.nn, no autograd.
"""
from __future__ import annotations

import os

import numpy as np

from . import mc_cnn
from .pfm import load_pfm

POS_HIGH, NEG_LOW, NEG_HIGH = 0.5, 1.5, 6.0     # middlebury_2003.py:53-55


def momentum_names(nlayers: int):
    return [(f"conv{k}/weights/Momentum:0", f"conv{k}/biases/Momentum:0") for k in range(1, nlayers + 1)]


def flatten(weights: dict, nlayers: int, names=None) -> np.ndarray:
    """dict of HWIO weights / biases -> the flat float32 blob (w1, b1, w2, b2, ...)."""
    names = names or mc_cnn.var_names(nlayers)
    return np.concatenate([np.asarray(weights[n], np.float32).ravel() for pair in names for n in pair])


def unflatten(blob, nlayers: int, nf: int = 64, names=None) -> dict:
    names = names or mc_cnn.var_names(nlayers)
    blob = np.asarray(blob, np.float32)
    out, off = {}, 0
    for k, (wn, bn) in enumerate(names, start=1):
        shape = (3, 3, 1 if k == 1 else nf, nf)
        n = int(np.prod(shape))
        out[wn] = blob[off:off + n].reshape(shape).copy()
        out[bn] = blob[off + n:off + n + nf].copy()
        off += n + nf
    if off != blob.size:
        raise ValueError(f"parameter blob has {blob.size} floats, {nlayers} layers need {off}")
    return out


def normalise(img_u8) -> np.ndarray:
    """(I - mean) / std in float32, as the reference prepares every image (middlebury_2003.py:78)."""
    img = np.asarray(img_u8).astype(np.float32)
    return ((img - np.mean(img, axis=(0, 1))) / np.std(img, axis=(0, 1))).astype(np.float32)


class TripletSampler:
    """Seeded patch centres from a left (and optionally right) disparity map.

    A centre (row, col) is valid when its disparity d is finite (and non-zero if zero_is_invalid: the Middlebury
    maps mark unknown pixels 0; the synthetic ground truth has no such sentinel), the patch lies inside the image,
    d + half <= col, and, with a right map, right[row, int(col - d)] is valid too and within 1 of d.  Then
    x_pos = int(col - d + U(-0.501, 0.501)) and x_neg = int(col - d +- U(1.5, 6)), each redrawn until the patch
    around it lies inside the row.
    """

    def __init__(self, left_disp, right_disp=None, patch: int = 11, seed: int = 0, zero_is_invalid: bool = True):
        self.left = np.asarray(left_disp, np.float64)
        self.right = None if right_disp is None else np.asarray(right_disp, np.float64)
        self.patch, self.half = int(patch), int(patch) // 2
        self.rng = np.random.default_rng(seed)
        H, W = self.left.shape
        h = self.half
        if H < self.patch or W < self.patch + 2 * int(NEG_HIGH):
            raise ValueError(f"a {H}x{W} map is too small for {patch}x{patch} triplets")

        def known(d):
            ok = np.isfinite(d)
            return ok & (d != 0) if zero_is_invalid else ok

        ok = known(self.left)
        ok[:h] = ok[H - h:] = False
        ok[:, :h] = ok[:, W - h:] = False
        cols = np.arange(W)[None, :]
        d0 = np.where(np.isfinite(self.left), self.left, 0.0)
        ok &= (d0 + h <= cols) & (d0 >= 0)
        if self.right is not None:
            rc = np.clip((cols - d0).astype(np.int64), 0, W - 1)
            rd = np.take_along_axis(self.right, rc, axis=1)
            with np.errstate(invalid="ignore"):
                ok &= known(rd) & (np.fabs(np.where(np.isfinite(rd), rd, np.inf) - d0) <= 1)
        self.centres = np.argwhere(ok)
        if len(self.centres) == 0:
            raise ValueError("the disparity map has no valid patch centre")

    def _inside(self, c: int) -> bool:
        return self.half <= c < self.left.shape[1] - self.half

    def sample(self, n: int) -> np.ndarray:
        """-> int32 [n][4] = (y, x_left, x_pos, x_neg), the layout sde_train_gather takes."""
        out = np.empty((n, 4), np.int32)
        pick = self.rng.integers(0, len(self.centres), n)
        for i, (row, col) in enumerate(self.centres[pick]):
            right_col = col - self.left[row, col]
            pos = -1
            while not self._inside(pos):
                pos = int(right_col + self.rng.uniform(-POS_HIGH - 0.001, POS_HIGH + 0.001))
            neg = -1
            while not self._inside(neg):
                dev = self.rng.uniform(NEG_LOW, NEG_HIGH)
                if self.rng.integers(-1, 1) == -1:
                    dev = -dev
                neg = int(right_col + dev)
            out[i] = (row, col, pos, neg)
        return out


def synthetic_triplets(seed: int, batch: int, patch: int = 11, H: int = 64, W: int = 160, D: int = 32):
    """One seeded batch from synthetic.stereo_pair(H, W, D, seed): (img_l, img_r normalised f32 [H][W], idx).
    The right-view disparity map the sampler's left-right check needs is built the way stereo_pair builds the
    right image (right pixel x - d shows left pixel x, the last writer wins); right pixels no left pixel maps to
    are unknown (inf), so centres whose match is occluded are not drawn."""
    from .synthetic import stereo_pair
    left, right, gt = stereo_pair(H, W, D, seed)
    ys, xs = np.mgrid[0:H, 0:W]
    ok = xs - gt >= 0
    right_gt = np.full((H, W), np.inf)
    right_gt[ys[ok], (xs - gt)[ok]] = gt[ok]
    idx = TripletSampler(gt, right_gt, patch=patch, seed=seed, zero_is_invalid=False).sample(batch)
    return normalise(left), normalise(right), idx


class SceneBatch:
    """What SceneSet.batch returns: batch `step` of `B` triplets, drawn when a Trainer resolves it."""
    __slots__ = ("scenes", "step", "B")

    def __init__(self, scenes, step: int, B: int):
        self.scenes, self.step, self.B = scenes, int(step), int(B)


class SceneSet:
    """Stereo scenes with ground truth, resident on the device, as a source of training batches.

    scenes: [(img_l_u8, img_r_u8, disp_l, disp_r or None)], images [H][W] (uint8 or anything `normalise` takes),
    disparity maps [H][W] floats.  Every image is normalised as the reference prepares it and uploaded with its
    left map; ops.triplet_centres compacts the scene's valid centres (TripletSampler's rule) on the device, with
    one count read back per scene, here and never later.  A scene without a centre is left out (its number is in
    `.skipped`); a set without any raises.  `.batch(step, B)` is a handle that Trainer.step / Trainer.loss resolve
    with ops.train_sample_gather into the trainer's own patch buffer: triplet i of batch `step` depends on
    (seed, step, i) and the scenes alone, whatever was drawn before.
    """

    def __init__(self, scenes, nlayers: int = 5, seed: int = 0, zero_is_invalid: bool = True, max_rounds: int = 32,
                 device=None):
        import torch

        from . import ops
        self.nlayers, self.seed, self.max_rounds = int(nlayers), int(seed), int(max_rounds)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise ValueError(f"SceneSet needs a GPU device, got {self.device}")

        def up(a, dtype=np.float32):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

        self.skipped, self.shapes, self.counts, self._keep, rows = [], [], [], [], []
        first = 0
        with torch.cuda.device(self.device):
            for k, (img_l, img_r, disp_l, disp_r) in enumerate(scenes):
                il, ir, dl = up(normalise(img_l)), up(normalise(img_r)), up(disp_l)
                if il.dim() != 2 or il.shape != ir.shape or il.shape != dl.shape:
                    raise ValueError(f"scene {k}: images and disparity map must share one [H][W] shape, got "
                                     f"{tuple(il.shape)} / {tuple(ir.shape)} / {tuple(dl.shape)}")
                dr = None if disp_r is None else up(disp_r)
                centres, count = ops.triplet_centres(dl, dr, self.nlayers, zero_is_invalid)
                n = int(count.item())
                if n == 0:
                    self.skipped.append(k)
                    continue
                centres = centres[:n].clone()
                H, W = il.shape
                rows.append([il.data_ptr(), ir.data_ptr(), dl.data_ptr(), centres.data_ptr(), H, W, first, n])
                self._keep.append((il, ir, dl, centres))
                self.shapes.append((H, W))
                self.counts.append(n)
                first += n
            if not rows:
                raise ValueError("no scene has a valid patch centre")
            self.N = first
            self.table = torch.tensor(rows, dtype=torch.int64).to(self.device)

    def __len__(self) -> int:
        return len(self.counts)

    def batch(self, step: int, B: int) -> SceneBatch:
        return SceneBatch(self, step, B)

    def gather(self, step: int, B: int, out=None, idx=None, scene=None):
        """Batch `step` into `out` (f32 [3][B][P][P]); idx / scene as ops.train_sample_gather takes them."""
        from . import ops
        return ops.train_sample_gather(self.table, self.N, B, self.nlayers, self.seed, step, self.max_rounds,
                                       out=out, idx=idx, scene=scene)


class PatchFileDataset:
    """The reference's ImagePatchesGenerator: per-patch files path.format(number), numbers head .. tail - 1, read
    in list order (a permutation drawn from NumPy's global state when shuffle, as the reference does; seed it with
    np.random.seed), batch_size at a time from `pointer`."""

    def __init__(self, path_left, path_right_pos, path_right_neg, number_of_data_set_head, number_of_data_set_tail,
                 patch_size=(11, 11), batch_size=128, shuffle=True):
        self._paths = (path_left, path_right_pos, path_right_neg)
        self._head, self._count = number_of_data_set_head, number_of_data_set_tail - number_of_data_set_head
        self.patch_size, self.batch_size, self.shuffle = patch_size, batch_size, shuffle
        self.dataset_size = self._count // batch_size
        self.reset_pointer()

    def load_pfm(self, fname):
        return load_pfm(fname)

    def next_batch(self):
        """-> (left, right_pos, right_neg), each float32 [batch][ph][pw][1]."""
        shape = (self.batch_size, self.patch_size[0], self.patch_size[1], 1)
        out = [np.empty(shape, np.float32) for _ in range(3)]
        for i in range(self.batch_size):
            number = self._head + self.patches_list[i + self.pointer]
            for arr, path in zip(out, self._paths):
                arr[i] = self.load_pfm(path.format(number))[0]
        self.update_pointer()
        return tuple(out)

    def update_pointer(self):
        self.pointer += self.batch_size

    def reset_pointer(self):
        self.pointer = 0
        n = self._count
        self.patches_list = np.random.permutation(n) if self.shuffle else np.arange(n, dtype=np.int32)


class Trainer:
    """Momentum SGD on the hinge loss, everything resident on one device."""

    def __init__(self, nlayers: int = 5, nf: int = 64, batch: int = 128, margin: float = 0.3, lr: float = 1e-3,
                 beta: float = 0.9, weights=None, device=None):
        import torch

        from . import ops
        self._torch, self._ops = torch, ops
        self.nlayers, self.nf, self.batch = int(nlayers), int(nf), int(batch)
        self.patch = 2 * self.nlayers + 1
        self.margin, self.lr, self.beta = float(margin), float(lr), float(beta)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise ValueError(f"Trainer needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        n = ops.train_param_floats(self.nlayers, self.nf)
        blob = flatten(mc_cnn.load_weights(weights, self.nlayers), self.nlayers)
        if blob.size != n:
            raise ValueError(f"weights hold {blob.size} floats, {self.nlayers} layers of {self.nf} maps need {n}")
        self.params = torch.from_numpy(blob).to(self.device)
        self.velocity = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros(n, dtype=torch.float32, device=self.device)
        self._bufs = {}
        self._buffers(self.batch)

    def _buffers(self, B: int):
        """(workspace, loss, patches) for a batch of B, allocated the first time B is seen."""
        if B not in self._bufs:
            t = self._torch
            self._bufs[B] = (t.empty(self._ops.train_workspace_bytes(B, self.nlayers, self.nf), dtype=t.uint8,
                                     device=self.device),
                             t.empty(1 + B, dtype=t.float32, device=self.device),
                             t.empty((3, B, self.patch, self.patch), dtype=t.float32, device=self.device))
        return self._bufs[B]

    def _on_device(self):
        """The kernels launch on HIP's current device and torch's current stream: make ours current, so that a
        Trainer on another device than the caller's never launches where its buffers are not."""
        return self._torch.cuda.device(self.device)

    def _dev(self, a, dtype):
        t = self._torch
        if not isinstance(a, t.Tensor):
            a = t.from_numpy(np.array(a, order="C"))      # a copy: the caller's array may be read-only
        return a.to(device=self.device, dtype=dtype).contiguous()

    def _patches(self, data):
        """[3,B,P,P] patches from: such a tensor / array; three [B,P,P(,1)] arrays (PatchFileDataset.next_batch);
        (img_l, img_r, idx), gathered on the device; or a SceneBatch, drawn and gathered on the device."""
        t = self._torch
        if isinstance(data, SceneBatch):
            if data.scenes.nlayers != self.nlayers or data.scenes.device != self.device:
                raise ValueError(f"the scene set is for {data.scenes.nlayers} layers on {data.scenes.device}, the "
                                 f"trainer for {self.nlayers} on {self.device}")
            return data.scenes.gather(data.step, data.B, out=self._buffers(data.B)[2])
        if isinstance(data, (tuple, list)) and len(data) == 3:
            third = data[2]
            if third.ndim == 2 and third.shape[1] == 4 and not (third.dtype.is_floating_point if isinstance(
                    third, t.Tensor) else np.issubdtype(third.dtype, np.floating)):
                idx = self._dev(third, t.int32)
                out = self._buffers(idx.shape[0])[2]
                return self._ops.train_gather(self._dev(data[0], t.float32), self._dev(data[1], t.float32), idx,
                                              self.nlayers, out=out)
            parts = [self._dev(p, t.float32).reshape(-1, self.patch, self.patch) for p in data]
            return t.stack(parts).contiguous()
        return self._dev(data, t.float32)

    def step(self, data, factor: float = 1):
        """One training step at learning rate float32(lr / factor).  Returns the loss buffer (device f32 [1+B]:
        the mean before the update, then every h_i); nothing is read back."""
        with self._on_device():
            return self._step(data, factor)

    def _step(self, data, factor):
        patches = self._patches(data)
        ws, loss, _ = self._buffers(patches.shape[1])
        self._ops.train_loss_grad(patches, self.params, self.nlayers, self.margin, loss=loss, grads=self.grads,
                                  workspace=ws, nf=self.nf)
        self._ops.train_momentum(self.params, self.velocity, self.grads, float(np.float32(self.lr / factor)), self.beta)
        return loss

    def loss(self, data) -> float:
        """Forward pass only: the mean hinge loss of a batch (read back)."""
        with self._on_device():
            return self._loss(data)

    def _loss(self, data) -> float:
        patches = self._patches(data)
        ws, loss, _ = self._buffers(patches.shape[1])
        self._ops.train_loss_grad(patches, self.params, self.nlayers, self.margin, loss=loss, workspace=ws,
                                  nf=self.nf, want_grads=False)
        return float(loss[0].item())

    def weights(self) -> dict:
        """The parameters under the reference's variable names (what mc_cnn.load_weights and StereoMatcher take)."""
        return unflatten(self.params.cpu().numpy(), self.nlayers, self.nf)

    def save(self, path) -> None:
        out = self.weights()
        out.update(unflatten(self.velocity.cpu().numpy(), self.nlayers, self.nf, momentum_names(self.nlayers)))
        with open(os.fspath(path), "wb") as fh:
            np.savez(fh, **out)

    def load(self, path) -> None:
        """Weights from anything mc_cnn.load_weights takes; velocities too if the file holds them (else zero)."""
        w = mc_cnn.load_weights(path, self.nlayers)
        self.params.copy_(self._torch.from_numpy(flatten(w, self.nlayers)))
        names = momentum_names(self.nlayers)
        if all(n in w for pair in names for n in pair):
            self.velocity.copy_(self._torch.from_numpy(flatten(w, self.nlayers, names)))
        else:
            self.velocity.zero_()
