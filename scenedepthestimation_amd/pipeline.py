"""Device-resident stereo matching: buffers allocated once, every stage a libsde launch.

``StereoMatcher`` is the hot path behind both the drop-in function API
(process_functional.py) and bench.py:

    u8 images (HBM) -> z-norm + zero pad -> MC-CNN tower (x2) -> fused cost
    volume + WTA over [d0, d1)                         (configs 1/2, north star)

optionally followed by the reference's post-processing on the two views' raw maps
(``match_lr``): the right view of the fused kernel -> wrap-free LR check -> LRC
fill -> 5x5 median,

and the GPU path of ``disparity_compute_by_gpu`` (process_functional.py:1093-1267):

    features -> [H,W,D] L/R volumes -> penalties -> 8-path SGM (L, R) -> WTA
    -> LR check -> LRC fill -> 5x5 median

All buffers are sized for one (H, W, D) problem and reused across calls, so a
call allocates nothing and can be captured into a HIP graph.
"""
from __future__ import annotations

import numpy as np
import torch

from . import mc_cnn, ops


AMAX_WORDS = ops.AMAX_ROW_WORDS   # f16x3 bound words per image in the tower workspace (TOWER_AMAX_BYTES / 4)
SPLIT_MAX_PIX = 1 << 24   # split activations: fewer input pixels per plane than this (tower.hip SPLIT_MAX_PIX)
# Placement draws of the four SGM volumes (SgmPath._place_volumes): volumes of [MIN, MAX] voxels are
# placed by up to this many allocate-and-time draws (larger ones would hold three 4-volume sets of > 6 GB each).
SGM_PLACEMENT_TRIALS = 16   # round 6: 8 draws missed the fast mode on some boxes (7 slow draws seen in a row)
SGM_PLACEMENT_MIN_VOXELS = 1 << 26
SGM_PLACEMENT_MAX_VOXELS = 1 << 29


def tower_steps(img_pad, packed, nlayers: int, out, ws, precision: str = "f16x3", nf: int = 64, on_launch=None):
    """sde_tower_forward_batch's launch sequence (mc_cnn_brunch.py:31-48), one layer at a time, as a
    generator: the same launches, bound-word memset and image absmax (each image's activations
    packed at its layer's own size rather than the C path's fixed act_stride), so the features are
    bit-identical to ops.tower_forward_batch.  It yields (stage, words) after the
    image bound (stage 1) and after every layer l < nlayers (stage l): the points at which a caller
    may combine the f16x3 bound words of row bands (all-reduce MAX, parallel.py) before the next
    layer reads them.  on_launch(layer, launch): optional wrapper around each layer's launch (timing).

    img_pad f32 [N, H+2L, W+2L] (contiguous), out f32 [N, H, W, nf], ws uint8 of
    ops.tower_batch_workspace_bytes(H, W, N, nlayers) bytes (or more)."""
    L = nlayers
    N, Hp, Wp = img_pad.shape
    H, W = Hp - 2 * L, Wp - 2 * L
    need = ops.tower_batch_workspace_bytes(H, W, N, L, nf)
    if ws.numel() < need:
        raise ValueError("tower workspace too small")
    h2, w2 = H + 2 * (L - 2), W + 2 * (L - 2)
    # between layers: what sde_tower_forward_batch passes -- split activations on the f16x3 tower when
    # built with them (ops.TOWER_SPLIT_ACT; <= 32 layers, < 2^24 pixels), else c-block-major fp32
    sp = ops.TOWER_SPLIT_ACT and precision == "f16x3" and 2 < L <= ops.SCALE_WORD and h2 * w2 < SPLIT_MAX_PIX
    cbl = not sp and precision in ops.TOWER_CBLOCK_PRECISIONS
    act = h2 * w2 * nf if L > 2 else 0
    wsf = ws[: 2 * N * act * 4 + N * AMAX_WORDS * 4].view(torch.float32)
    bufs = [wsf[: N * act], wsf[N * act: 2 * N * act]]
    words = wsf[2 * N * act:].view(N, AMAX_WORDS)
    f16 = precision in ops.TOWER_BOUND_WORD_PRECISIONS
    if f16:
        words.zero_()
        ops.absmax_batch(img_pad, words)
    yield 1, words

    def run(layer, fn):
        if on_launch is None:
            fn()
        else:
            on_launch(layer, fn)

    hin, win = H + 2 * L - 4, W + 2 * L - 4
    first = out if L == 2 else bufs[0][: N * hin * win * nf].view(N, hin, win, nf)
    run(2, lambda: ops.tower_layer_batch(img_pad, packed, L, 2, first, nf=nf, precision=precision,
                                         out_cblock=cbl and L > 2, in_absmax=words[:, 0:1] if f16 else None,
                                         out_absmax=words[:, 1:2] if (f16 and L > 2) else None, out_split=sp))
    cur = 0
    for layer in range(3, L + 1):
        yield layer - 1, words
        src = bufs[cur][: N * hin * win * nf].view(N, hin, win, nf)
        o = out if layer == L else bufs[cur ^ 1][: N * (hin - 2) * (win - 2) * nf].view(N, hin - 2, win - 2, nf)
        run(layer, lambda: ops.tower_layer_batch(src, packed, L, layer, o, nf=nf, precision=precision,
                                                 in_cblock=cbl, out_cblock=cbl and layer < L,
                                                 in_absmax=words[:, layer - 2:layer - 1] if f16 else None,
                                                 out_absmax=words[:, layer - 1:layer] if (f16 and layer < L) else None,
                                                 in_split=sp, out_split=sp and layer < L))
        hin, win = hin - 2, win - 2
        cur ^= 1


class SpeckleStage:
    """Speckle removal (ops.speckle, include/sde_filter.h) as the last stage of a path: regions of at most max_size
    4-connected valid pixels whose neighbours differ by at most max_diff become -1 ("no winner"), which
    rectify.Rectifier.depth / .points with the default min_disp = 0 turn into depth 0 / no point.  The filtered
    maps (one per slot: a path that returns two maps filters each into its own), the last call's mask and region
    sizes and the workspace are allocated on first use."""

    def __init__(self, H, W, device, max_size, max_diff: float = 1.0):
        self.H, self.W, self.device = int(H), int(W), torch.device(device)
        self.max_size, self.max_diff = int(max_size), float(max_diff)
        if self.max_size < 0 or not 0.0 <= self.max_diff < float("inf"):
            raise ValueError("speckle=(max_size, max_diff) needs max_size >= 0 and a finite max_diff >= 0")
        self.out, self.mask, self.sizes, self.ws = {}, None, None, None

    @classmethod
    def make(cls, H, W, device, speckle):
        """None, a (max_size, max_diff) pair or a stage to share -> None or a stage."""
        if speckle is None or isinstance(speckle, cls):
            return speckle
        max_size, max_diff = speckle
        return cls(H, W, device, max_size, max_diff)

    def run(self, disp, slot: int = 0):
        """-> the filtered map, in this stage's buffer for `slot`; disp is left as it is."""
        H, W, dev = self.H, self.W, self.device
        if self.ws is None:
            self.mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
            self.sizes = torch.empty((H, W), dtype=torch.int32, device=dev)
            self.ws = torch.empty((ops.speckle_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
        if slot not in self.out:
            self.out[slot] = torch.empty((H, W), dtype=torch.float32, device=dev)
        ops.speckle(disp, self.max_size, self.max_diff, -1.0, out=self.out[slot], mask=self.mask, sizes=self.sizes,
                    workspace=self.ws)
        return self.out[slot]


class InterpStage:
    """fill="interpolate" of a checked path (include/sde_interp.h): the flagged pixels of the left map are
    classified against the right map (ops.classify, the path's flags, the matcher's D) and interpolated
    (ops.interpolate) where fill="mean4" runs ops.lrc_fill.  The class map, the filled mask and the workspace are
    allocated on first use.  No later stage reads `cls` or `filled`: they are kept for the caller, as
    SpeckleStage.mask is (cls: 1 occlusion, 2 mismatch; filled: 1 where a value was taken, so a flagged pixel with
    filled == 0 kept its raw value)."""

    def __init__(self, H, W, D, device):
        self.H, self.W, self.D, self.device = int(H), int(W), int(D), torch.device(device)
        self.cls = self.filled = self.ws = None

    @classmethod
    def make(cls, H, W, D, device, fill):
        """fill -> None ("mean4") or a stage ("interpolate")."""
        return cls(H, W, D, device) if ops.fill_mode(fill) == "interpolate" else None

    def run(self, disp_l, disp_r, lrc_l, max_diff, out):
        """-> out, the left map with its flagged pixels interpolated; lrc_l is left as it is."""
        H, W, dev = self.H, self.W, self.device
        if self.ws is None:
            self.cls = torch.empty((H, W), dtype=torch.uint8, device=dev)
            self.filled = torch.empty((H, W), dtype=torch.uint8, device=dev)
            self.ws = torch.empty((ops.interpolate_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
        ops.classify(disp_r, lrc_l, self.D, "left", max_diff, out=self.cls)
        ops.interpolate(disp_l, self.cls, "left", out=out, filled=self.filled, workspace=self.ws)
        return out


def run_tower(img_pad, packed, nlayers, out, ws, precision="f16x3", nf=64, combine=None, on_launch=None):
    """Drive tower_steps to the end; combine(words) is applied at every yield (e.g. an all-reduce)."""
    for _stage, words in tower_steps(img_pad, packed, nlayers, out, ws, precision, nf, on_launch):
        if combine is not None:
            combine(words)
    return out


class StereoMatcher:
    def __init__(self, height: int, width: int, ndisp: int, weights=None, nlayers: int = 5,
                 nf: int = 64, device=None, d_range=None, sgm: bool = False, tower_precision: str = "f16x3",
                 cv_mode: str = "certified", cbca_iters: int = 0, cbca_L1: int = 14, cbca_tau: float = 0.02,
                 emit_split: bool = False, sgm_placement_trials: int = SGM_PLACEMENT_TRIALS,
                 subpixel: bool = False, bilateral: bool = False, speckle=None, unique=None, fill: str = "mean4"):
        self.H, self.W, self.D = int(height), int(width), int(ndisp)
        # fill="interpolate": the checked paths (match_lr, sgm_path with post=True) classify the flagged left pixels
        # and interpolate them (include/sde_interp.h) where "mean4" (the default) runs the reference's LRC fill
        self.fill = ops.fill_mode(fill)
        # unique=tau: the uniqueness check (include/sde_unique.h) inside the fused CV + WTA of match() / match_lr()
        # and on the SGM path's S volumes; None (the default) leaves every path's launches and allocations as they are
        self.unique = None if unique is None else ops.unique_tau(unique)
        # the two stages the reference carries switched off (process_functional.py:813-819, :882-974); off by
        # default, and with both off every call below makes the launches it made before they existed
        self.subpixel, self.bilateral = bool(subpixel), bool(bilateral)
        # cross-based aggregation before SGM (build-defined stage; 0 = the reference's GPU path)
        self.cbca_iters, self.cbca_L1, self.cbca_tau = int(cbca_iters), int(cbca_L1), float(cbca_tau)
        self.nlayers, self.nf = int(nlayers), int(nf)
        self.sgm_placement_trials = int(sgm_placement_trials)
        if tower_precision not in ops.TOWER_PRECISIONS:
            raise ValueError(f"tower_precision must be one of {sorted(ops.TOWER_PRECISIONS)}")
        self.tower_precision = tower_precision
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.d0, self.d1 = (0, self.D) if d_range is None else (int(d_range[0]), int(d_range[1]))
        if self.subpixel and (self.d0, self.d1) != (0, self.D):
            # a shard's winner may sit at the shard's end with its neighbour in the next shard; refine the
            # merged map instead (ops.cv_subpixel over the whole range)
            raise ValueError(f"subpixel=True needs the whole disparity range [0, {self.D}); this matcher holds "
                             f"the shard [{self.d0}, {self.d1})")
        if speckle is not None and (self.d0, self.d1) != (0, self.D):
            # a shard's map is not the final one: a region may exist only after the merge
            raise ValueError(f"speckle needs the whole disparity range [0, {self.D}); this matcher holds the shard "
                             f"[{self.d0}, {self.d1}): filter the merged map instead (ops.speckle)")
        if self.unique is not None and (self.d0, self.d1) != (0, self.D):
            # a shard's runner-up may sit in another shard: the merge of per-shard margins is not built
            raise ValueError(f"unique needs the whole disparity range [0, {self.D}); this matcher holds the shard "
                             f"[{self.d0}, {self.d1})")
        w = mc_cnn.load_weights(weights, self.nlayers)
        hw, hb = mc_cnn.layer_lists(w, self.nlayers)
        packed = ops.pack_tower_weights(hw, hb)
        dev = self.device
        H, W, L = self.H, self.W, self.nlayers
        self.packed = torch.from_numpy(packed).to(dev)
        self.img_u82 = torch.empty((2, H, W), dtype=torch.uint8, device=dev)
        self.img_u8 = [self.img_u82[0], self.img_u82[1]]
        self.raw_u82 = None    # the unrectified pair of load_raw, allocated on first use
        # both images in one allocation: the tower runs the pair per launch (sde_tower_forward_batch)
        self.img_pad2 = torch.empty((2, H + 2 * L, W + 2 * L), dtype=torch.float32, device=dev)
        self.img_pad = [self.img_pad2[0], self.img_pad2[1]]
        n = ops.preprocess_scratch_bytes(H, W)
        self.stats2 = torch.empty((2 * n,), dtype=torch.uint8, device=dev)
        self.stats = [self.stats2[:n], self.stats2[n:]]
        self.feat2 = torch.empty((2, H, W, nf), dtype=torch.float32, device=dev)
        self.feat = [self.feat2[0], self.feat2[1]]
        self._ws = None        # the tower workspace, allocated on first use (see ws)
        self.disp = torch.empty((H, W), dtype=torch.float32, device=dev)
        self.min_cost = torch.empty((H, W), dtype=torch.float32, device=dev)
        self.argmin = torch.empty((H, W), dtype=torch.int32, device=dev)
        self.cv_mode = cv_mode
        self.reject = torch.empty((H, W), dtype=torch.uint8, device=dev) if self.unique is not None else None
        self.cv_ws = torch.empty(ops.cv_wta_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
        # optional: bf16 split planes + norm bounds emitted by the tower's last layer, consumed by
        # sde_cv_wta_split.  The default certified path (sde_cv_wta, row-sweep kernel) splits the fp32
        # features itself and reads nothing else, so the planes are not written by default.
        self.split = [ops.new_split(H, W, dev) for _ in range(2)] \
            if (emit_split and cv_mode == "certified" and nlayers >= 2) else None
        self.split_valid = False
        self.lr_bufs = None    # the right view and the checked path's maps, allocated on first use (_lr_bufs)
        # speckle=(max_size, max_diff): speckle removal as the last stage of every path (SpeckleStage, one shared
        # by the paths); None (the default) leaves every path's launches and allocations as they are
        self.speckle = SpeckleStage.make(H, W, dev, speckle)
        # the GPU path of disparity_compute_by_gpu; its aggregation stage borrows the tower's input buffers for
        # the z-normalised images
        self.sgm = SgmPath(H, W, self.D, dev, self.cbca_iters, self.cbca_L1, self.cbca_tau, self.subpixel,
                           self.bilateral, self.sgm_placement_trials, scratch=(self.img_pad, self.stats, L),
                           speckle=self.speckle, unique=self.unique, fill=self.fill)
        if sgm:
            self.sgm.alloc()

    @property
    def sgm_bufs(self):
        """The SGM path's buffers (SgmPath.alloc), None until the path has run or sgm=True asked for them."""
        return self.sgm.bufs

    @property
    def sgm_placement_ms(self):
        return self.sgm.placement_ms

    @property
    def speckle_mask(self):
        """u8 [H,W], 1 where the last speckle filter call removed the pixel (None with the option off or before the
        first call); rectify.Rectifier.depth of the filtered map is 0 there."""
        return None if self.speckle is None else self.speckle.mask

    @property
    def speckle_sizes(self):
        """i32 [H,W], the region size of every valid pixel of the last map filtered (None as speckle_mask)."""
        return None if self.speckle is None else self.speckle.sizes

    @property
    def unique_mask(self):
        """u8 [H,W], 1 where the last match() / match_lr() / cost_wta() rejected a left-view winner by the
        uniqueness check (None with the option off); the SGM path keeps its own (sgm.unique_mask)."""
        return self.reject

    @property
    def ws(self):
        """Tower workspace (both images' activations + bound words, ~4 x H x W x 64 floats), allocated
        on first use: a matcher whose tower runs elsewhere (parallel.DisparityShardedMatcher's band
        tower) never holds it."""
        if self._ws is None:
            nws = ops.tower_batch_workspace_bytes(self.H, self.W, 2, self.nlayers, self.nf)
            self._ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=self.device)
        return self._ws

    # -- stages ----------------------------------------------------------------
    def load_images(self, left_u8, right_u8):
        """Host u8 [H,W] arrays (or device tensors) -> resident device images."""
        ops.upload_u8_pair(self.img_u82, left_u8, right_u8)

    def load_raw(self, left_raw, right_raw, rectifier):
        """Raw (unrectified) host u8 arrays or device tensors of the rectifier's raw size -> the resident pair,
        rectified on the device in one launch (rectify.Rectifier.remap into img_u82).  The raw pair's device
        buffer is allocated on the first call; everything after it is what load_images leaves behind."""
        if tuple(rectifier.out_size) != (self.H, self.W):
            raise ValueError(f"the rectifier writes {tuple(rectifier.out_size)} images, this matcher takes "
                             f"{(self.H, self.W)}")
        shape = (2,) + tuple(rectifier.raw_size)
        if self.raw_u82 is None or tuple(self.raw_u82.shape) != shape:
            self.raw_u82 = torch.empty(shape, dtype=torch.uint8, device=self.device)
        ops.upload_u8_pair(self.raw_u82, left_raw, right_raw)
        rectifier.remap(self.raw_u82, out=self.img_u82)

    def load_normalised(self, left, right):
        """Two normalised host images f32 [H,W] -> the tower's zero-padded input (process_functional.py:13-19),
        for features_from_padded()."""
        H, W, L = self.H, self.W, self.nlayers
        for dst, img in zip(self.img_pad, (left, right)):
            buf = np.zeros((H + 2 * L, W + 2 * L), np.float32)
            buf[L:L + H, L:L + W] = img
            dst.copy_(torch.from_numpy(buf))

    def features(self, on_launch=None):
        """Preprocess + tower for both images (compute_feature, process_functional.py:11-45).
        on_launch(layer, launch): run the tower layer by layer from Python (tower_steps: the same
        launches, bits and workspace as the one-call path) with each launch wrapped, e.g. timed."""
        ops.preprocess_u8_batch(self.img_u82, self.nlayers, out=self.img_pad2, stats=self.stats2)
        return self.features_from_padded(on_launch)

    def features_from_padded(self, on_launch=None):
        """Tower only, on already-normalised padded images in self.img_pad (the pair per launch)."""
        if on_launch is not None and self.split:
            raise ValueError("on_launch needs the layer-by-layer tower, which does not emit split planes "
                             "(emit_split=True): time the one-call tower instead")
        if on_launch is not None:
            run_tower(self.img_pad2, self.packed, self.nlayers, self.feat2, self.ws, self.tower_precision, self.nf,
                      on_launch=on_launch)
            self.split_valid = False
            return self.feat[0], self.feat[1]
        if self.split:
            for i in range(2):
                ops.tower_forward(self.img_pad[i], self.packed, self.nlayers, self.nf, out=self.feat[i],
                                  workspace=self.ws, precision=self.tower_precision, split=self.split[i])
        else:
            ops.tower_forward_batch(self.img_pad2, self.packed, self.nlayers, self.nf, out=self.feat2,
                                    workspace=self.ws, precision=self.tower_precision)
        self.split_valid = self.split is not None
        return self.feat[0], self.feat[1]

    def cost_wta(self, want=("disp",)):
        """Fused cost volume + WTA over this matcher's disparity range [d0, d1).  In certified mode with
        emit_split=True the tower-emitted split planes are used (sde_cv_wta_split) when the current
        features came from this matcher's tower; otherwise sde_cv_wta reads the fp32 features.  With unique set
        the fused unique form (ops.cv_wta_unique) on the fp32 features: disp is -1 where rejected, unique_mask the
        decision."""
        if self.unique is not None:
            return ops.cv_wta_unique(self.feat[0], self.feat[1], self.d0, self.d1, self.unique, "left",
                                     disp=self.disp if "disp" in want else None,
                                     min_cost=self.min_cost if "min" in want else None,
                                     argmin=self.argmin if "argmin" in want else None, reject=self.reject, want=(),
                                     mode=self.cv_mode, workspace=self.cv_ws)[:3]
        if self.cv_mode == "certified" and self.split_valid:
            return ops.cv_wta_split(self.feat[0], self.feat[1], self.split[0], self.split[1], self.d0, self.d1,
                                    disp=self.disp if "disp" in want else None,
                                    min_cost=self.min_cost if "min" in want else None,
                                    argmin=self.argmin if "argmin" in want else None, want=(),
                                    workspace=self.cv_ws)
        return ops.cv_wta(self.feat[0], self.feat[1], self.d0, self.d1,
                          disp=self.disp if "disp" in want else None,
                          min_cost=self.min_cost if "min" in want else None,
                          argmin=self.argmin if "argmin" in want else None, want=(),
                          mode=self.cv_mode, workspace=self.cv_ws)

    def match(self):
        """One pass of the hot path on the resident images: features + fused CV/WTA -> disparity; with
        subpixel=True followed by the parabola step on the winner's recomputed neighbours (ops.cv_subpixel), which
        passes the -1 of a pixel the uniqueness check rejected (unique=tau) through.  With
        speckle set the filtered map is returned, in a buffer of its own; self.disp keeps the unfiltered one."""
        self.features()
        self.cost_wta()
        if self.subpixel:
            ops.cv_subpixel(self.feat[0], self.feat[1], self.d0, self.d1, self.disp, "left", out=self.disp)
        if self.speckle is not None:
            return self.speckle.run(self.disp)
        return self.disp

    # -- left-right-checked fast path ------------------------------------------
    def _lr_bufs(self):
        """The right view's outputs and workspace and the checked path's maps, allocated on first use: a matcher
        that only runs match() never holds them."""
        if self.lr_bufs is None:
            H, W, dev = self.H, self.W, self.device
            self.disp_r = torch.empty((H, W), dtype=torch.float32, device=dev)
            self.min_cost_r = torch.empty((H, W), dtype=torch.float32, device=dev)
            self.argmin_r = torch.empty((H, W), dtype=torch.int32, device=dev)
            self.cv_ws_r = torch.empty(ops.cv_wta_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
            self.reject_r = torch.empty((H, W), dtype=torch.uint8, device=dev) if self.unique is not None else None
            self.checked = CheckedPath(H, W, dev, self.bilateral, self.speckle, self.fill, self.D)
            self.lr_bufs = self.checked.bufs
        return self.lr_bufs

    def cost_wta_right(self, want=("disp",)):
        """The right view of cost_wta over this matcher's [d0, d1) (ops.cv_wta_right), into disp_r / min_cost_r /
        argmin_r with its own workspace cv_ws_r.  Always reads the fp32 features (there is no right-view form
        of the pre-split kernel)."""
        self._lr_bufs()
        if self.unique is not None:
            return ops.cv_wta_unique(self.feat[0], self.feat[1], self.d0, self.d1, self.unique, "right",
                                     disp=self.disp_r if "disp" in want else None,
                                     min_cost=self.min_cost_r if "min" in want else None,
                                     argmin=self.argmin_r if "argmin" in want else None, reject=self.reject_r, want=(),
                                     mode=self.cv_mode, workspace=self.cv_ws_r)[:3]
        return ops.cv_wta_right(self.feat[0], self.feat[1], self.d0, self.d1,
                                disp=self.disp_r if "disp" in want else None,
                                min_cost=self.min_cost_r if "min" in want else None,
                                argmin=self.argmin_r if "argmin" in want else None, want=(),
                                mode=self.cv_mode, workspace=self.cv_ws_r)

    def _need_whole_range(self):
        if (self.d0, self.d1) != (0, self.D):
            raise ValueError(f"the left-right check needs both views over the whole range [0, {self.D}); this "
                             f"matcher holds the shard [{self.d0}, {self.d1})")

    def lr_checked(self, max_diff: float = 1.0):
        """match_lr's stages after the features, on the features this matcher currently holds.  subpixel=True
        refines both views' raw maps before the check; bilateral=True filters the median's output with the left
        image (the reference's dead call, :1260, would filter the LRC-filled map and overwrite the median's
        result: a documented divergence); speckle removal, when set, comes last.  With
        unique=tau both views come from the fused unique form: a rejected pixel is -1 in its raw map, which the
        check flags (d < 0), so rejected left pixels are filled by the LRC fill.  With fill="interpolate" the
        flagged left pixels are classified against the right map and interpolated (InterpStage) instead of
        LRC-filled."""
        self._need_whole_range()
        self._lr_bufs()
        self.cost_wta()
        self.cost_wta_right()
        if self.subpixel:
            ops.cv_subpixel(self.feat[0], self.feat[1], self.d0, self.d1, self.disp, "left", out=self.disp)
            ops.cv_subpixel(self.feat[0], self.feat[1], self.d0, self.d1, self.disp_r, "right", out=self.disp_r)
        return self.checked.run(self.disp, self.disp_r, max_diff, self.img_u8[0])

    def match_lr(self, max_diff: float = 1.0):
        """The hot path with the reference's post-processing (is_error_match / LRC / median,
        process_functional.py:977-1088, :840-879) on both views' raw maps: features, cost_wta, cost_wta_right,
        the wrap-free left-right check, LRC fill of the left map, 5x5 median.  Returns (disp_l_checked, disp_r,
        lrc_l); self.disp keeps the raw left map (refined with subpixel=True).  Not for a disparity shard
        (ValueError)."""
        self._need_whole_range()
        self.features()
        return self.lr_checked(max_diff)

    # -- GPU path of disparity_compute_by_gpu ---------------------------------
    def cbca(self, cv_l, cv_r, img_l, img_r):
        """SgmPath.cbca on this matcher's path (arms from the z-normalised images, in the tower's input buffers)."""
        return self.sgm.cbca(cv_l, cv_r, img_l, img_r)

    def sgm_path(self, fl=None, fr=None, img_l=None, img_r=None, timings=None, post=True):
        """SgmPath.run on this matcher's features and resident u8 images unless others are given."""
        return self.sgm.run(self.feat[0] if fl is None else fl, self.feat[1] if fr is None else fr,
                            self.img_u8[0] if img_l is None else img_l, self.img_u8[1] if img_r is None else img_r,
                            timings=timings, post=post)


class CheckedPath:
    """The reference's post-processing of two views' raw maps (is_error_match / LRC / median,
    process_functional.py:977-1088, :840-879) and the maps it writes: the wrap-free left-right check, LRC fill of
    the left map, 5x5 median and, with bilateral=True, the 9x9 bilateral filter of the median's output; with
    speckle=(max_size, max_diff) (or a SpeckleStage to share) speckle removal of the map that would be returned.
    fill="interpolate" (with ndisp, the matcher's D): the flagged left pixels are classified and interpolated
    (InterpStage) instead of LRC-filled.  Shared by StereoMatcher.lr_checked and LocalMatcher.match_lr."""

    def __init__(self, H, W, device, bilateral: bool = False, speckle=None, fill: str = "mean4", ndisp=None):
        self.speckle = SpeckleStage.make(H, W, device, speckle)
        if ops.fill_mode(fill) == "interpolate" and ndisp is None:
            raise ValueError("fill='interpolate' needs ndisp, the number of disparities of the two maps")
        self.interp = InterpStage.make(H, W, ndisp, device, fill)
        f32 = lambda: torch.empty((H, W), dtype=torch.float32, device=device)   # noqa: E731
        u8 = lambda: torch.empty((H, W), dtype=torch.uint8, device=device)      # noqa: E731
        self.bufs = dict(lrc=[u8(), u8()], filled=f32(), checked=f32())
        if bilateral:
            self.bufs["smoothed"] = f32()

    def run(self, disp_l, disp_r, max_diff: float = 1.0, img_l=None):
        """-> (disp_l_checked, disp_r, lrc_l).  img_l: the left u8 image (the bilateral filter's intensities)."""
        b = self.bufs
        ops.lr_consistency(disp_l, disp_r, max_diff, b["lrc"][0], b["lrc"][1])
        if self.interp is not None:
            self.interp.run(disp_l, disp_r, b["lrc"][0], max_diff, b["filled"])
        else:
            ops.lrc_fill(disp_l, b["lrc"][0], out=b["filled"])
        # the 5x5 median of the filled map into the interior of a copy of it: the 2-pixel border keeps the
        # filled values
        b["checked"].copy_(b["filled"])
        ops.median5(b["filled"], b["checked"])
        last = b["checked"]
        if "smoothed" in b:
            last = ops.bilateral9(img_l, b["checked"], out=b["smoothed"])
        if self.speckle is not None:
            last = self.speckle.run(last)
        return last, disp_r, b["lrc"][0]


class SgmPath:
    """The GPU path of disparity_compute_by_gpu (process_functional.py:1093-1267) on device tensors, for one
    (H, W, D) problem: it owns the path's buffers (`bufs`, allocated on first use) and takes the features and the
    u8 images as arguments, so it runs with or without a StereoMatcher around it.

    cbca_iters > 0 puts cross-based aggregation (build-defined; 0 = the reference's path) before SGM; its arms come
    from the z-normalised images, which need scratch = (img_pad, stats, pad): two f32 [H+2p, W+2p] buffers and
    two ops.preprocess_scratch_bytes(H, W) scratch tensors (StereoMatcher lends the tower's input buffers).
    subpixel / bilateral: the two stages the reference carries switched off (see run).  unique=tau: the uniqueness
    check on the final S volumes (see run; unique_mask is the left view's decision).  speckle: None, a
    (max_size, max_diff) pair or a SpeckleStage to share; with post=True the maps run() returns are filtered.
    fill="interpolate": with post=True the flagged left pixels (the uniqueness OR included) are classified and
    interpolated (InterpStage) where "mean4", the default, runs the LRC fill."""

    def __init__(self, height: int, width: int, ndisp: int, device, cbca_iters: int = 0, cbca_L1: int = 14,
                 cbca_tau: float = 0.02, subpixel: bool = False, bilateral: bool = False,
                 placement_trials: int = SGM_PLACEMENT_TRIALS, scratch=None, speckle=None, unique=None,
                 fill: str = "mean4"):
        self.H, self.W, self.D, self.device = int(height), int(width), int(ndisp), torch.device(device)
        self.fill = ops.fill_mode(fill)
        self.interp = InterpStage.make(self.H, self.W, self.D, self.device, fill)
        self.unique = None if unique is None else ops.unique_tau(unique)
        self.cbca_iters, self.cbca_L1, self.cbca_tau = int(cbca_iters), int(cbca_L1), float(cbca_tau)
        self.subpixel, self.bilateral = bool(subpixel), bool(bilateral)
        self.placement_trials = int(placement_trials)
        self.placement_ms = None     # the SGM pair time of each placement draw (_place_volumes)
        self.scratch = scratch
        self.speckle = SpeckleStage.make(self.H, self.W, self.device, speckle)
        self.bufs = None

    def _place_volumes(self, pen, disp):
        """The four [H,W,D] volumes of the GPU path (cost L/R, SGM S L/R), placed by allocate-and-time draws.

        The 7-launch SGM pair moves the same bytes through any four volumes, yet on MI355X it runs in one of two
        modes by where the allocation lands in HBM: ~5.3 or ~5.7-5.8 ms at 1024^2 x 192 (LR/RL 0.81 vs 0.95 ms
        per launch, the diagonals 0.80 vs 0.85; the same virtual addresses can come back in either mode,
        row strides and offsets inside one allocation do not decide it, the box's thermal / power state does not
        either -- tools/sgm_*_probe.py).  So for large volumes each draw allocates a fresh
        set (the previous one still held, so the draw gets other memory), times one pair on zero costs, and the
        fastest set is kept; the draws stop once one beats the slowest seen by 6 % (both modes seen).  One-time
        cost: ~20 ms per draw."""
        H, W, D, dev = self.H, self.W, self.D, self.device

        def new_set():
            return [torch.empty((H, W, D), dtype=torch.float32, device=dev) for _ in range(4)]
        trials = self.placement_trials if SGM_PLACEMENT_MIN_VOXELS <= H * W * D <= SGM_PLACEMENT_MAX_VOXELS else 1
        if trials <= 1:
            return new_set()
        for p in pen:
            p.zero_()

        def pair_ms(v):
            for t in v:
                t.zero_()
            run = lambda: ops.sgm_8path_wta_pair(v[0], pen[0], v[2], disp[0], v[1], pen[1], v[3], disp[1],  # noqa: E731
                                                 zero_du_penalties=True)
            run()
            best = float("inf")
            for _ in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize(dev)
                best = min(best, e0.elapsed_time(e1))
            return best
        best, best_ms, worst, prev, times = None, float("inf"), 0.0, None, []
        for _ in range(trials):
            cur = new_set()
            ms = pair_ms(cur)
            times.append(ms)
            worst = max(worst, ms)
            if ms < best_ms:
                best, best_ms = cur, ms
            prev = cur
            torch.cuda.empty_cache()
            if best_ms <= 0.94 * worst:
                break
        del prev, cur
        torch.cuda.empty_cache()
        self.placement_ms = times
        return best

    def alloc(self, arms: bool = False):
        """The path's buffers, allocated on first use; the aggregation's arms and workspace with cbca_iters > 0 or
        when asked for (a cbca() call on a path whose run() does not aggregate)."""
        H, W, dev = self.H, self.W, self.device
        if self.bufs is None:
            pen = [torch.empty((H, W, 16), dtype=torch.float32, device=dev) for _ in range(2)]
            disp = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(2)]
            cvl, cvr, sl, sr = self._place_volumes(pen, disp)
            # the right volume starts as the GPU path's invalid fill (1.0): with aggregation on, the cost
            # volume sweep writes the left volume only and sde_cbca_lr the right one's valid voxels, so its
            # invalid voxels (x + d >= W) keep this fill -- the value the two-volume sweep writes there
            cvr.fill_(1.0)
            self.bufs = dict(
                cv=[cvl, cvr],
                pen=pen,
                S=[sl, sr],
                disp=disp,
                lrc=[torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(2)],
                disp_a=torch.empty((H, W), dtype=torch.float32, device=dev),
                disp_b=torch.empty((H, W), dtype=torch.float32, device=dev),
            )
        if self.unique is not None and "rej" not in self.bufs:
            self.bufs["rej"] = [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
        if (arms or self.cbca_iters > 0) and "arms" not in self.bufs:
            self.bufs["arms"] = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(2)]
            self.bufs["cbca_ws"] = torch.empty((ops.cbca_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
        return self.bufs

    @property
    def unique_mask(self):
        """u8 [H,W], 1 where the last run() rejected a left-view winner (None with the option off or before it)."""
        return None if self.unique is None or self.bufs is None else self.bufs["rej"][0]

    def cbca(self, cv_l, cv_r, img_l, img_r):
        """Cross-based aggregation (build-defined) of the left [H,W,D] volume in
        place, and the right volume derived from it.  Arms come from the z-normalised images (the
        tower's input normalisation).

        cv_r is an OUTPUT: its valid voxels (x + d < W) are overwritten with the shear of the aggregated
        cv_l and their input is never read -- correct only because the GPU path's right volume IS the
        left one's shear (one sweep computes each voxel once, sec. 3.1).  Its invalid voxels are kept.
        For two independent volumes use ops.cbca_pair."""
        if self.scratch is None:
            raise ValueError("aggregation needs scratch=(img_pad, stats, pad) for the z-normalised images")
        b, H, W = self.alloc(arms=True), self.H, self.W
        img_pad, stats, P = self.scratch
        for k, img in enumerate((img_l, img_r)):
            ops.preprocess_u8(img, P, out=img_pad[k], stats=stats[k])
            ops.cbca_arms(img_pad[k][P:P + H, P:P + W], self.cbca_L1, self.cbca_tau, out=b["arms"][k])
        # the right volume is the left one's shear (valid voxels), so its aggregation is the shear of the
        # left one's (definition v2): one volume aggregated, then one shear pass writes cv_r's valid voxels
        # (their input is not read; its invalid voxels are kept).  The SGM S buffer (written later,
        # overwrite mode) is the scratch.
        ops.cbca_lr(cv_l, cv_r, b["arms"][0], b["arms"][1], self.cbca_L1, self.cbca_iters, tmp=b["S"][0],
                    workspace=b["cbca_ws"])
        return cv_l, cv_r

    def run(self, fl, fr, img_l, img_r, timings=None, post=True):
        """process_functional.py:1093-1267 on device tensors; returns (disp_l, disp_r).  subpixel=True: the
        unfused SGM pair followed by ops.wta_subpixel per side instead of the fused last direction;
        bilateral=True: the 9x9 bilateral filter of each median-filtered map with its own image.
        unique=tau: the unfused pair as for subpixel, ops.wta or ops.wta_subpixel per side, then ops.wta_unique per
        side on S (rule d0).  With post=False both maps carry -1 at their rejected pixels.  With post=True the
        left-right check runs on the unmasked maps, the left reject mask is OR-ed into lrc_l before the LRC fill
        (rejected left pixels are filled), and the right map gets its -1 after its median or bilateral filter.

        timings: optional dict receiving per-stage seconds (synchronised)."""
        import time
        b = self.alloc()

        def mark(name, t0):
            if timings is not None:
                torch.cuda.synchronize(self.device)
                t1 = time.time()
                timings[name] = timings.get(name, 0.0) + (t1 - t0)
                return t1
            return t0

        t = time.time() if timings is not None else 0.0
        # process_functional.py:120-131.  With aggregation the right volume comes from sde_cbca_lr (the
        # aggregated left volume's shear), so the sweep writes the left one only.
        ops.cost_volume(fl, fr, self.D, layout="HWD", right=self.cbca_iters <= 0, invalid=1.0,
                        out_left=b["cv"][0], out_right=b["cv"][1] if self.cbca_iters <= 0 else None)
        t = mark("cost_volume", t)
        if self.cbca_iters > 0:
            self.cbca(b["cv"][0], b["cv"][1], img_l, img_r)
            t = mark("cbca", t)
        ops.sgm_penalties(img_l, out=b["pen"][0])
        ops.sgm_penalties(img_r, out=b["pen"][1])
        # both sides per launch (the reference's k loop); S := 8-path sum, no zero-fill pass
        # penalties from sgm_penalties (channels 0/1 zero), finite costs: DU folds into UD;
        # WTA_and_SupixelRefinement_kernel (:800-837) fused into the last direction
        if self.subpixel or self.unique is not None:
            # the parabola step needs the final S around the winner, and the uniqueness check the whole of it,
            # which the fused last direction never stores: the unfused pair (S written in full), then WTA
            # (+ refinement) per side
            ops.sgm_8path_pair(b["cv"][0], b["pen"][0], b["S"][0], b["cv"][1], b["pen"][1], b["S"][1],
                               zero_du_penalties=True)
            wta = ops.wta_subpixel if self.subpixel else ops.wta
            wta(b["S"][0], "HWD", "d0", out=b["disp"][0])
            wta(b["S"][1], "HWD", "d0", out=b["disp"][1])
            if self.unique is not None:
                # post=False: both maps masked here.  post=True: the left decision only (for lrc_l); the right
                # map is masked after its filters, by the launch that takes its decision
                ops.wta_unique(b["S"][0], self.unique, "HWD", "d0", disp=None if post else b["disp"][0], want=(),
                               reject=b["rej"][0])
                if not post:
                    ops.wta_unique(b["S"][1], self.unique, "HWD", "d0", disp=b["disp"][1], want=(),
                                   reject=b["rej"][1])
        else:
            ops.sgm_8path_wta_pair(b["cv"][0], b["pen"][0], b["S"][0], b["disp"][0], b["cv"][1], b["pen"][1],
                                   b["S"][1], b["disp"][1], zero_du_penalties=True)
        t = mark("sgm", t)
        if not post:
            return b["disp"][0], b["disp"][1]
        b["lrc"][0].zero_()
        b["lrc"][1].zero_()
        ops.lr_check(b["disp"][0], b["disp"][1], b["lrc"][0], b["lrc"][1])
        if self.unique is not None:
            b["lrc"][0].bitwise_or_(b["rej"][0])
        if self.interp is not None:
            # the check's own bound is 1 (is_error_match_kernel), so the classification's is too
            self.interp.run(b["disp"][0], b["disp"][1], b["lrc"][0], 1.0, b["disp_a"])
        else:
            ops.lrc_fill(b["disp"][0], b["lrc"][0], out=b["disp_a"])
        t = mark("lrc", t)
        # Median_Filter_kernel(d_disparityl_a, d_disparityr_a, d_disparityl, d_disparityr) (:1250):
        # the interior of disp_l becomes the median of the LRC-filled map.  The reference's
        # right input d_disparityr_a is never written (:1227); here the right map is filtered
        # from its own WTA output (documented divergence, parity unpinned).
        disp_r_src = b["disp_b"]
        disp_r_src.copy_(b["disp"][1])
        ops.median5(b["disp_a"], b["disp"][0])
        ops.median5(disp_r_src, b["disp"][1])
        if self.bilateral:
            # Bilateral_Filter_kernel (:882-974) of the median's output, each map with its own image, into the
            # two maps the median has finished reading.  The reference's dead call (:1260) would filter the
            # LRC-filled map and overwrite the median's result (documented divergence).
            ops.bilateral9(img_l, b["disp"][0], out=b["disp_a"])
            ops.bilateral9(img_r, b["disp"][1], out=b["disp_b"])
            final = (b["disp_a"], b["disp_b"])
        else:
            final = (b["disp"][0], b["disp"][1])
        if self.unique is not None:
            ops.wta_unique(b["S"][1], self.unique, "HWD", "d0", disp=final[1], want=(), reject=b["rej"][1])
        if self.speckle is not None:
            # the right map first: the stage's mask and sizes are then the left map's
            right = self.speckle.run(final[1], slot=1)
            final = (self.speckle.run(final[0], slot=0), right)
        mark("filter", t)
        return final
