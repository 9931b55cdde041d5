"""Tensor-level wrappers over the C ABI (include/sde.h).

Every op takes CUDA (HIP) torch tensors, checks dtype / contiguity / shape on
the host, launches on torch's current stream and returns torch tensors.  torch
is only plumbing here (device memory, streams); all arithmetic runs in the HIP
kernels of libsde.so.  There is no CPU fallback: on a machine without a GPU
these functions raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import (SDE_LAYOUT_DHW, SDE_LAYOUT_HWD, SDE_SIDE_LEFT, SDE_SIDE_RIGHT, SDE_WTA_INIT_D0,
                   SDE_WTA_INIT_INF, check, lib)

LAYOUTS = {"DHW": SDE_LAYOUT_DHW, "HWD": SDE_LAYOUT_HWD}
RULES = {"inf": SDE_WTA_INIT_INF, "d0": SDE_WTA_INIT_D0}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, name: str, dtype=torch.float32, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device}); libsde has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)} (got {tuple(t.shape)})")
    return t.data_ptr()


def _empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _feat_pair(fl, fr):
    if fl.dim() != 3 or tuple(fl.shape) != tuple(fr.shape):
        raise ValueError(f"features must be matching [H,W,C] tensors, got {tuple(fl.shape)} / {tuple(fr.shape)}")
    H, W, C = fl.shape
    return _need(fl, "featuresl", shape=(H, W, C)), _need(fr, "featuresr", shape=(H, W, C)), H, W, C


def _lr_volumes(shape, like, left, right, out_left, out_right):
    """The left / right f32 volumes of a two-sided cost kernel: each side asked for is allocated on like's device
    unless given, and validated.  Returns (left pointer, right pointer, what the op returns): the left volume,
    (left, right) with right=True, the right one alone with left=False; a side not asked for is a null pointer."""
    if not left and not right:
        raise ValueError("nothing to compute")
    ol = orr = None
    if left:
        if out_left is None:
            out_left = _empty(shape, torch.float32, like)
        ol = _need(out_left, "out_left", shape=shape)
    if right:
        if out_right is None:
            out_right = _empty(shape, torch.float32, like)
        orr = _need(out_right, "out_right", shape=shape)
    if not left:
        return ol, orr, out_right
    return ol, orr, (out_left, out_right) if right else out_left


# ----------------------------------------------------------------------------
# cost volume / WTA (process_functional.py:48-131, 800-837)
# ----------------------------------------------------------------------------
def cost_volume(fl, fr, ndisp: int, layout: str = "DHW", right: bool = False, invalid=None,
                out_left=None, out_right=None, left: bool = True):
    """Exact cost volume.  DHW: compute_cost_volume (invalid -0.0).  HWD: GPU-path layout
    with left and optionally right volumes (invalid 1.0, process_functional.py:1111); both
    sides come from one pass (each voxel computed once, stored twice)."""
    pl, pr, H, W, C = _feat_pair(fl, fr)
    lay = LAYOUTS[layout]
    if invalid is None:
        invalid = -0.0 if layout == "DHW" else 1.0
    shape = (ndisp, H, W) if layout == "DHW" else (H, W, ndisp)
    if right and layout != "HWD":
        raise ValueError("the right volume exists in the HWD (GPU-path) layout only")
    ol, orr, result = _lr_volumes(shape, fl, left, right, out_left, out_right)
    sides = (SDE_SIDE_LEFT if left else 0) | (SDE_SIDE_RIGHT if right else 0)
    check(lib.sde_cost_volume(pl, pr, H, W, C, int(ndisp), lay, sides, ctypes.c_float(invalid), ol, orr,
                              _stream()), "sde_cost_volume")
    return result


CV_MODES = {"exact": _lib.SDE_CV_EXACT, "certified": _lib.SDE_CV_CERTIFIED}


def cv_wta_workspace_bytes(H: int, W: int) -> int:
    return int(lib.sde_cv_wta_workspace_bytes(H, W))


def cv_wta(fl, fr, d0: int, d1: int, disp=None, min_cost=None, argmin=None, want=("disp",), mode: str = "certified",
           workspace=None):
    """Fused cost volume + first-min over [d0, d1): WTA1(compute_cost_volume(fl, fr, d1)) when d0 = 0.

    mode 'exact' (VALU, NumPy order for every voxel) or 'certified' (fp16 hi/lo MFMA scores of the row
    sweep + error bound, exact resolution of uncertified pixels): identical outputs.  workspace: uint8
    tensor of cv_wta_workspace_bytes(H, W) bytes (allocated if None); cv_wta_fixups(workspace) is the
    number of pixels resolved exactly after the call."""
    return _cv_wta_view(lib.sde_cv_wta, "sde_cv_wta", fl, fr, d0, d1, disp, min_cost, argmin, want, mode, workspace)


def cv_wta_right(fl, fr, d0: int, d1: int, disp=None, min_cost=None, argmin=None, want=("disp",),
                 mode: str = "certified", workspace=None):
    """The right view of cv_wta (sde_cv_wta_right), indexed by right pixel: the first minimum over [d0, d1) of
    cost(x + d, d), i.e. flipW(WTA1(compute_cost_volume(flipW(fr), flipW(fl), d1))) when d0 = 0 (voxels with
    x + d >= W hold the -0.0 fill; ties go to the lower d).  fl / fr are the left / right maps as for cv_wta.
    Same arguments, modes (identical outputs), workspace and returns as cv_wta; cv_wta_fixups(workspace) counts
    the pixels resolved exactly."""
    return _cv_wta_view(lib.sde_cv_wta_right, "sde_cv_wta_right", fl, fr, d0, d1, disp, min_cost, argmin, want, mode,
                        workspace)


def _wta_outputs(fl, H, W, want, disp, min_cost, argmin):
    """The (disp, min_cost, argmin) maps of a fused CV + WTA call and their pointers: those named in `want` are
    allocated on fl's device unless given; every one given is validated, and an output neither wanted nor given
    stays None (a null pointer: the kernel skips it)."""
    if "disp" in want and disp is None:
        disp = _empty((H, W), torch.float32, fl)
    if "min" in want and min_cost is None:
        min_cost = _empty((H, W), torch.float32, fl)
    if "argmin" in want and argmin is None:
        argmin = _empty((H, W), torch.int32, fl)
    pd = _need(disp, "disp", shape=(H, W)) if disp is not None else None
    pm = _need(min_cost, "min_cost", shape=(H, W)) if min_cost is not None else None
    pa = _need(argmin, "argmin", dtype=torch.int32, shape=(H, W)) if argmin is not None else None
    return (disp, min_cost, argmin), (pd, pm, pa)


def _cv_wta_view(fn, what, fl, fr, d0, d1, disp, min_cost, argmin, want, mode, workspace):
    pl, pr, H, W, C = _feat_pair(fl, fr)
    (disp, min_cost, argmin), (pd, pm, pa) = _wta_outputs(fl, H, W, want, disp, min_cost, argmin)
    md = CV_MODES[mode]
    pws, wsb = None, 0
    if md == _lib.SDE_CV_CERTIFIED:
        need = cv_wta_workspace_bytes(H, W)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=fl.device)
        pws, wsb = _need(workspace, "workspace", dtype=torch.uint8), workspace.numel()
    check(fn(pl, pr, H, W, C, int(d0), int(d1), pd, pm, pa, md, pws, wsb, _stream()), what)
    return disp, min_cost, argmin


def cv_wta_split_workspace_bytes(H: int, W: int) -> int:
    return int(lib.sde_cv_wta_split_workspace_bytes(H, W))


def cv_wta_split(fl, fr, split_l, split_r, d0: int, d1: int, disp=None, min_cost=None, argmin=None,
                 workspace=None, want=("disp",)):
    """Certified fused CV + WTA on pre-split operands (tower-emitted or feature_split)."""
    pl, pr, H, W, C = _feat_pair(fl, fr)
    (disp, min_cost, argmin), (pd, pm, pa) = _wta_outputs(fl, H, W, want, disp, min_cost, argmin)
    if workspace is None:
        workspace = torch.empty(cv_wta_split_workspace_bytes(H, W), dtype=torch.uint8, device=fl.device)
    lh, ll, ln = _split_ptrs(split_l, (H, W))
    rh, rl, rn = _split_ptrs(split_r, (H, W))
    check(lib.sde_cv_wta_split(pl, pr, lh, ll, ln, rh, rl, rn, H, W, int(d0), int(d1), pd, pm, pa,
                               _need(workspace, "workspace", dtype=torch.uint8), workspace.numel(), _stream()),
          "sde_cv_wta_split")
    return disp, min_cost, argmin


def cv_wta_fixups(workspace) -> int:
    """Number of pixels the last certified cv_wta call resolved with the exact scan (synchronises): the sum of
    the workspace's 64 counter words (one per 256-disparity chunk on the chunked path, word 0 otherwise)."""
    return int(workspace[:256].view(torch.int32).sum().item())


def wta(vol, layout: str = "DHW", rule: str = "inf", out=None):
    """First-min over d: WTA1 (DHW), WTA (HWD) or the SGM WTA kernel (HWD, rule='d0')."""
    return _wta_volume(lib.sde_wta, "sde_wta", vol, layout, rule, out)


def _wta_volume(fn, what, vol, layout, rule, out):
    if vol.dim() != 3:
        raise ValueError("volume must be 3-D")
    if layout == "DHW":
        D, H, W = vol.shape
    else:
        H, W, D = vol.shape
    pv = _need(vol, "volume")
    if out is None:
        out = _empty((H, W), torch.float32, vol)
    po = _need(out, "disp", shape=(H, W))
    check(fn(pv, H, W, D, LAYOUTS[layout], RULES[rule], po, _stream()), what)
    return out


def argmin_merge(mins, args, out=None):
    """Ordered merge of per-shard (min [S,H,W], argmin [S,H,W]) -> float32 disparity [H,W]."""
    S = mins.shape[0]
    pm = _need(mins, "mins")
    pa = _need(args, "args", dtype=torch.int32, shape=tuple(mins.shape))
    npix = int(np.prod(mins.shape[1:]))
    if out is None:
        out = _empty(tuple(mins.shape[1:]), torch.float32, mins)
    po = _need(out, "disp")
    check(lib.sde_argmin_merge(pm, pa, S, npix, po, _stream()), "sde_argmin_merge")
    return out


# ----------------------------------------------------------------------------
# MC-CNN tower (mc_cnn_brunch.py:31-48) and preprocessing (match_single.py:34-43)
# ----------------------------------------------------------------------------
def tower_packed_floats(nlayers: int, nf: int = 64) -> int:
    n = lib.sde_tower_packed_floats(nlayers, nf)
    if n < 0:
        raise ValueError(f"unsupported tower shape nlayers={nlayers} nf={nf}")
    return int(n)


def pack_tower_weights(hwio_list, bias_list) -> np.ndarray:
    """Pack HWIO weights / biases (host numpy) into the device blob layout (host-side C helper)."""
    L = len(hwio_list)
    nf = int(hwio_list[0].shape[-1])
    ws = [np.ascontiguousarray(w, dtype=np.float32) for w in hwio_list]
    bs = [np.ascontiguousarray(b, dtype=np.float32) for b in bias_list]
    for l, (w, b) in enumerate(zip(ws, bs)):
        cin = 1 if l == 0 else nf
        if w.shape != (3, 3, cin, nf) or b.shape != (nf,):
            raise ValueError(f"layer {l + 1}: expected weights (3,3,{cin},{nf}) and biases ({nf},), "
                             f"got {w.shape} / {b.shape}")
    out = np.empty(tower_packed_floats(L, nf), np.float32)
    wp = (ctypes.c_void_p * L)(*[w.ctypes.data for w in ws])
    bp = (ctypes.c_void_p * L)(*[b.ctypes.data for b in bs])
    check(lib.sde_tower_pack_weights(wp, bp, L, nf, out.ctypes.data), "sde_tower_pack_weights")
    return out


def tower_workspace_bytes(H: int, W: int, nlayers: int, nf: int = 64) -> int:
    return int(lib.sde_tower_workspace_bytes(H, W, nlayers, nf))


# "f16x3w": f16x3 with the Winograd F(2x2, 3x3) kernel for layers 3..L (SDE_TOWER_WINOGRAD)
# "f16x3m32": f16x3 with layers 3..L on the 32x32x16 direct kernel (SDE_TOWER_MFMA32; the default f16x3
# runs them on the 16x16x32 kernel)
# "f16x3t32": f16x3 with every layer on the 16 x 32-tile kernel (SDE_TOWER_TILE32; the default f16x3 runs layers
# 3..L on the 16 x 16-tile kernel whose stagers store the outputs, where the activations are fp32): the same bits as "f16x3"
TOWER_PRECISIONS = {"fp32": _lib.SDE_TOWER_FP32, "bf16x6": _lib.SDE_TOWER_BF16X6, "f16x3": _lib.SDE_TOWER_F16X3,
                    "f16x3w": _lib.SDE_TOWER_F16X3 | _lib.SDE_TOWER_WINOGRAD,
                    "f16x3m32": _lib.SDE_TOWER_F16X3 | _lib.SDE_TOWER_MFMA32,
                    "f16x3t32": _lib.SDE_TOWER_F16X3 | _lib.SDE_TOWER_TILE32}


# the precisions whose layers scale by f16 bound words (every f16x3 variant): the words a layer-by-layer driver
# zeroes, fills from the image and hands from layer to layer (and row bands all-reduce) ...
TOWER_BOUND_WORD_PRECISIONS = frozenset(p for p, f in TOWER_PRECISIONS.items() if f & _lib.SDE_TOWER_F16X3)
# ... and those whose activations sde_tower_forward* pass between layers in the c-block-major layout (the split
# precisions; fp32 keeps [h, w, nf])
TOWER_CBLOCK_PRECISIONS = frozenset(p for p, f in TOWER_PRECISIONS.items()
                                    if f & (_lib.SDE_TOWER_BF16X6 | _lib.SDE_TOWER_F16X3))


def _split_ptrs(split, shape):
    """split = (hi int16 [..., 64], lo int16 [..., 64], norm f32 [...]) or None -> three pointers."""
    if split is None:
        return None, None, None
    hi, lo, nrm = split
    return (_need(hi, "feat_hi", dtype=torch.int16, shape=shape + (64,)),
            _need(lo, "feat_lo", dtype=torch.int16, shape=shape + (64,)),
            _need(nrm, "feat_norm", shape=shape))


def new_split(H: int, W: int, device):
    """Buffers for bf16 split planes + norm bound of an [H,W,64] feature map."""
    return (torch.empty((H, W, 64), dtype=torch.int16, device=device),
            torch.empty((H, W, 64), dtype=torch.int16, device=device),
            torch.empty((H, W), dtype=torch.float32, device=device))


def feature_split(feat, split=None):
    """[H,W,64] f32 -> (hi, lo, norm) for the certified cost volume (sde_feature_split)."""
    H, W, C = feat.shape
    if split is None:
        split = new_split(H, W, feat.device)
    ph, pl, pn = _split_ptrs(split, (H, W))
    check(lib.sde_feature_split(_need(feat, "features"), H * W, C, ph, pl, pn, _stream()), "sde_feature_split")
    return split


def tower_forward(img_pad, packed, nlayers: int, nf: int = 64, out=None, workspace=None, precision: str = "fp32",
                  split=None):
    """img_pad: f32 [H+2L, W+2L] -> L2-normalised features f32 [H, W, nf].
    precision: 'fp32' (fp32 MFMA), 'bf16x6' (exact 3-way bf16 split, 6 partial products, fp32 accumulate) or
    'f16x3' (power-of-two scaled exact 2-way fp16 split, 3 partial products, fp32 accumulate).
    split: optional (hi, lo, norm) buffers the last layer's epilogue fills (certified cost volume input)."""
    Hp, Wp = img_pad.shape
    return _tower_forward((), Hp, Wp, img_pad, packed, nlayers, nf, out, workspace, precision, split)


def _tower_forward(lead, Hp, Wp, img_pad, packed, nlayers, nf, out, workspace, precision, split):
    """tower_forward (lead = ()) and tower_forward_batch (lead = (N,)): the same call apart from the leading N."""
    H, W = Hp - 2 * nlayers, Wp - 2 * nlayers
    if H <= 0 or W <= 0:
        raise ValueError("padded image smaller than the tower's receptive field")
    pi = _need(img_pad, "img_pad")
    pw = _need(packed, "packed weights", shape=(tower_packed_floats(nlayers, nf),))
    if out is None:
        out = _empty(lead + (H, W, nf), torch.float32, img_pad)
    po = _need(out, "features", shape=lead + (H, W, nf))
    if lead:
        fn, what, need = lib.sde_tower_forward_batch, "sde_tower_forward_batch", \
            tower_batch_workspace_bytes(H, W, lead[0], nlayers, nf)
    else:
        fn, what, need = lib.sde_tower_forward, "sde_tower_forward", tower_workspace_bytes(H, W, nlayers, nf)
    if need > 0 and workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=img_pad.device)
    pws = _need(workspace, "workspace", dtype=torch.uint8) if need > 0 else None
    wsb = workspace.numel() if need > 0 else 0
    check(fn(pi, *lead, H, W, pw, nlayers, nf, po, pws, wsb, TOWER_PRECISIONS[precision],
             *_split_ptrs(split, (H, W)), _stream()), what)
    return out


def absmax(x, out):
    """out (f32 [1] device) = max(out, max |x|) (sde_absmax_f32)."""
    check(lib.sde_absmax_f32(_need(x, "absmax input"), x.numel(), _need(out, "absmax word", shape=(1,)), _stream()),
          "sde_absmax_f32")
    return out


def set_persistent_grid(cus: int = 0):
    """Cap the persistent tower kernels' grid at `cus` workgroups (0: one per device CU), for a tower that
    shares the device with work on CU-masked streams (sde_set_persistent_grid).  Results do not depend on it
    (tests/test_gpu_tower_epilogue.py, test_capped_grid_*: features and bound words under 1-3 workgroups)."""
    check(lib.sde_set_persistent_grid(int(cus)), "sde_set_persistent_grid")


def tower_batch_workspace_bytes(H: int, W: int, nimg: int, nlayers: int, nf: int = 64) -> int:
    return int(lib.sde_tower_batch_workspace_bytes(H, W, nimg, nlayers, nf))


def tower_forward_batch(img_pad, packed, nlayers: int, nf: int = 64, out=None, workspace=None,
                        precision: str = "f16x3"):
    """img_pad: f32 [N, H+2L, W+2L] -> features f32 [N, H, W, nf], all N images per launch
    (sde_tower_forward_batch); each image's result equals tower_forward on it alone."""
    N, Hp, Wp = img_pad.shape
    return _tower_forward((N,), Hp, Wp, img_pad, packed, nlayers, nf, out, workspace, precision, None)


def absmax_batch(x, out):
    """out [N, k] (f32 device, column 0 used) = max(out, max |x[i]|) per image i of x [N, ...]
    (sde_absmax_f32_batch, one launch)."""
    N = x.shape[0]
    _need(x, "absmax input")
    if out.dtype != torch.float32 or not out.is_cuda or out.shape[0] != N or out.stride(1) != 1:
        raise ValueError("absmax words must be a float32 [N, k] device tensor with unit column stride")
    check(lib.sde_absmax_f32_batch(x.data_ptr(), N, x[0].numel(), out.data_ptr(), out.stride(0), _stream()),
          "sde_absmax_f32_batch")
    return out


SCALE_WORD = 32   # split activations: 2^sigma at bound word + 32 (sde.h SDE_TOWER_OUT_SPLIT)
AMAX_ROW_WORDS = 64   # a batch's bound-word row per image (tower.hip TOWER_AMAX_BYTES / 4)
# whether sde_tower_forward* pass split activations between the default f16x3 tower's 64->64 layers, as built
# (sde_tower_split_act(), tower.hip SDE_SPLIT_ACT; the layer-by-layer drivers in pipeline.py follow it to stay
# bit-identical)
TOWER_SPLIT_ACT = bool(lib.sde_tower_split_act())


def _layout_flags(flags, in_cblock, out_cblock, in_split, out_split):
    if in_cblock:
        flags |= _lib.SDE_TOWER_IN_CBLOCK
    if out_cblock:
        flags |= _lib.SDE_TOWER_OUT_CBLOCK
    if in_split:
        flags |= _lib.SDE_TOWER_IN_SPLIT
    if out_split:
        flags |= _lib.SDE_TOWER_OUT_SPLIT
    return flags


def _check_scale_word(words, rows, name):
    """Split activations read / write words[i * stride + 32]: the storage behind the word view must hold it."""
    if words is None:
        return
    stride = words.stride(0) if words.dim() > 1 else 0
    last = words.storage_offset() + (rows - 1) * stride + SCALE_WORD
    if words.untyped_storage().nbytes() < (last + 1) * 4:
        raise ValueError(f"{name}: split activations need the bound-word array to extend {SCALE_WORD} words "
                         "past each image's word (the scale word)")


def tower_layer(inp, packed, nlayers: int, layer: int, out, nf: int = 64, precision: str = "fp32", split=None,
                in_cblock: bool = False, out_cblock: bool = False, in_absmax=None, out_absmax=None,
                in_split: bool = False, out_split: bool = False):
    """One tower layer = one kernel launch (layer 2 = conv1+conv2 fused from the padded image).
    in_cblock / out_cblock (bf16x6, f16x3): intermediate activations in the c-block-major layout
    [nf/16][h][w][16] that tower_forward uses between layers (tensors keep their [h, w, nf]
    shape; only the element order differs).
    in_split / out_split (f16x3): the split-activation layout the default f16x3 tower_forward uses between
    layers (16 planes [cblk32][part][quarter] of [h][w][8 fp16], same bytes as [h, w, nf] f32); the scale
    2^sigma travels at in_absmax / out_absmax + 32 (views into a >= 33-word array).
    in_absmax / out_absmax (f16x3): f32 [1] device words -- a bound of |input| (|image| for layer
    2) and the word this layer maxes its outputs into (zeroed by the caller)."""
    flags = _layout_flags(TOWER_PRECISIONS[precision], in_cblock, out_cblock, in_split, out_split)
    if in_split:
        _check_scale_word(in_absmax, 1, "in_absmax")
    if out_split:
        _check_scale_word(out_absmax, 1, "out_absmax")
    if layer == 2:
        Hin, Win = inp.shape
        oshape = (Hin - 4, Win - 4, nf)
    else:
        Hin, Win, _ = inp.shape
        oshape = (Hin - 2, Win - 2, nf)
    pin = _need(in_absmax, "in_absmax", shape=(1,)) if in_absmax is not None else None
    pout = _need(out_absmax, "out_absmax", shape=(1,)) if out_absmax is not None else None
    check(lib.sde_tower_layer_scaled(_need(inp, "layer input"), Hin, Win,
                                     _need(packed, "packed weights", shape=(tower_packed_floats(nlayers, nf),)),
                                     nlayers, nf, layer, _need(out, "layer output", shape=oshape),
                                     flags, *_split_ptrs(split, oshape[:2]), pin, pout, _stream()),
          "sde_tower_layer_scaled")
    return out


def tower_layer_batch(inp, packed, nlayers: int, layer: int, out, nf: int = 64, precision: str = "f16x3",
                      in_cblock: bool = False, out_cblock: bool = False, in_absmax=None, out_absmax=None,
                      in_split: bool = False, out_split: bool = False):
    """tower_layer over a batch per launch: inp [N, Hin, Win] (layer 2) or [N, Hin, Win, nf], out
    [N, h, w, nf]; in_absmax / out_absmax (f16x3): [N, k] device words, column 0 used (row stride k;
    k > 32 with split activations, whose scale word is column 32)."""
    flags = _layout_flags(TOWER_PRECISIONS[precision], in_cblock, out_cblock, in_split, out_split)
    N, Hin, Win = inp.shape[:3]
    if in_split:
        _check_scale_word(in_absmax, N, "in_absmax")
    if out_split:
        _check_scale_word(out_absmax, N, "out_absmax")
    if (in_split or out_split) and N > 1:
        for words, name in ((in_absmax, "in_absmax"), (out_absmax, "out_absmax")):
            if words is not None and words.stride(0) < AMAX_ROW_WORDS:
                raise ValueError(f"{name}: split activations over a batch need rows of >= {AMAX_ROW_WORDS} bound words "
                                 f"(got a row stride of {words.stride(0)}): a layer's scale word is {SCALE_WORD} "
                                 "words past its bound word")
    sh = 4 if layer == 2 else 2
    oshape = (N, Hin - sh, Win - sh, nf)
    ws = 0
    pin = pout = None
    if in_absmax is not None:
        pin, ws = in_absmax.data_ptr(), in_absmax.stride(0)
    if out_absmax is not None:
        pout = out_absmax.data_ptr()
    _need(inp, "layer input")
    _need(out, "layer output", shape=oshape)
    check(lib.sde_tower_layer_batch(inp.data_ptr(), N, inp[0].numel(), Hin, Win,
                                    _need(packed, "packed weights", shape=(tower_packed_floats(nlayers, nf),)),
                                    nlayers, nf, layer, out.data_ptr(), out[0].numel(), flags, pin, pout, ws,
                                    _stream()), "sde_tower_layer_batch")
    return out


def upload_u8_pair(dst2, left, right):
    """Host u8 [H,W] arrays (or device tensors) -> the resident pair dst2, u8 [2,H,W] on the device."""
    for dst, src in zip(dst2, (left, right)):
        t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src, np.uint8))
        dst.copy_(t, non_blocking=False)


def preprocess_scratch_bytes(H: int, W: int) -> int:
    """Device scratch one image's preprocess needs (sde_preprocess_scratch_bytes)."""
    n = int(lib.sde_preprocess_scratch_bytes(int(H), int(W)))
    if n < 0:
        raise ValueError("invalid image shape")
    return n


def preprocess_u8(img_u8, pad: int, out=None, stats=None):
    """u8 [H,W] -> zero-padded z-normalised f32 [H+2p, W+2p] on the device, bit-identical to
    NumPy's (I - np.mean(I)) / np.std(I) on the float32 image (match_single.py:40-41).
    stats: optional uint8 scratch tensor of preprocess_scratch_bytes(H, W) bytes."""
    H, W = img_u8.shape
    pi = _need(img_u8, "image", dtype=torch.uint8)
    nb = preprocess_scratch_bytes(H, W)
    if out is None:
        out = _empty((H + 2 * pad, W + 2 * pad), torch.float32, img_u8)
    if stats is None:
        stats = _empty((nb,), torch.uint8, img_u8)
    check(lib.sde_preprocess_u8(pi, H, W, pad, _need(out, "out_pad", shape=(H + 2 * pad, W + 2 * pad)),
                                _need(stats, "scratch", dtype=torch.uint8, shape=(nb,)),
                                _stream()), "sde_preprocess_u8")
    return out


def preprocess_u8_batch(imgs_u8, pad: int, out=None, stats=None):
    """u8 [N,H,W] -> zero-padded z-normalised f32 [N, H+2p, W+2p], all images per launch.
    stats: optional uint8 scratch tensor of N * preprocess_scratch_bytes(H, W) bytes."""
    N, H, W = imgs_u8.shape
    pi = _need(imgs_u8, "images", dtype=torch.uint8)
    nb = N * preprocess_scratch_bytes(H, W)
    if out is None:
        out = _empty((N, H + 2 * pad, W + 2 * pad), torch.float32, imgs_u8)
    if stats is None:
        stats = _empty((nb,), torch.uint8, imgs_u8)
    check(lib.sde_preprocess_u8_batch(pi, N, H, W, pad, _need(out, "out_pad", shape=(N, H + 2 * pad, W + 2 * pad)),
                                      _need(stats, "scratch", dtype=torch.uint8, shape=(nb,)),
                                      _stream()), "sde_preprocess_u8_batch")
    return out


# ----------------------------------------------------------------------------
# SGM and post-processing (process_functional.py:134-1088)
# ----------------------------------------------------------------------------
def sgm_penalties(img_u8, P1=2.3, P2=55.9, threshold=30, lamda=4, out=None):
    H, W = img_u8.shape
    pi = _need(img_u8, "image", dtype=torch.uint8)
    if out is None:
        out = _empty((H, W, 16), torch.float32, img_u8)
    check(lib.sde_sgm_penalties(pi, H, W, float(P1), float(P2), int(threshold), float(lamda),
                                _need(out, "penalties", shape=(H, W, 16)), _stream()), "sde_sgm_penalties")
    return out


def sgm_8path(cv_hwd, pen, S=None):
    H, W, D = cv_hwd.shape
    pc = _need(cv_hwd, "cost volume")
    pp = _need(pen, "penalties", shape=(H, W, 16))
    if S is None:
        S = torch.zeros((H, W, D), dtype=torch.float32, device=cv_hwd.device)
    # accumulates into S (the caller zeroes it, as the reference uploads np.zeros)
    check(lib.sde_sgm_8path(pc, pp, H, W, D, _need(S, "S", shape=(H, W, D)), _stream()), "sde_sgm_8path")
    return S


def sgm_8path_pair(cv_l, pen_l, S_l, cv_r=None, pen_r=None, S_r=None, accumulate=False, zero_du_penalties=False):
    """8-path SGM of both image sides, one launch per direction (sde_sgm_8path_pair).

    accumulate=False: S := the 8-path sum from zero (S need not be zeroed).
    zero_du_penalties=True: the penalties come from sgm_penalties (channels 0/1 zero) and
    the costs are finite -- direction DU is folded into the UD pass (same values)."""
    _sgm_pair(lib.sde_sgm_8path_pair, "sde_sgm_8path_pair", (cv_l, pen_l, S_l), (cv_r, pen_r, S_r), accumulate,
              zero_du_penalties)
    return S_l, S_r


def _sgm_pair(fn, what, left, right, accumulate, zero_du_penalties):
    """One launch sequence over both sides.  left / right: (cost volume, penalties, S[, disp]); the right side
    is null pointers when its volume is None (the left side alone)."""
    H, W, D = left[0].shape
    shapes = (None, (H, W, 16), (H, W, D), (H, W))
    names = ("cost volume", "penalties", "S", "disp")
    args = [_need(t, n, shape=sh) for t, n, sh in zip(left, names, shapes)]
    if right[0] is None:
        args += [None] * len(right)
    else:
        args += [_need(t, n, shape=sh) for t, n, sh in zip(right, names, ((H, W, D),) + shapes[1:])]
    flags = (_lib.SDE_SGM_ACCUMULATE if accumulate else 0) | \
        (_lib.SDE_SGM_ZERO_DU_PENALTIES if zero_du_penalties else 0)
    check(fn(*args, H, W, D, flags, _stream()), what)


def sgm_8path_wta_pair(cv_l, pen_l, S_l, disp_l=None, cv_r=None, pen_r=None, S_r=None, disp_r=None,
                       accumulate=False, zero_du_penalties=False):
    """sgm_8path_pair + WTA (rule "d0") fused into the last direction (sde_sgm_8path_wta_pair):
    returns the disparity maps; S is left holding the first seven directions' sum."""
    H, W, _ = cv_l.shape
    if disp_l is None:
        disp_l = _empty((H, W), torch.float32, cv_l)
    if cv_r is not None and disp_r is None:
        disp_r = _empty((H, W), torch.float32, cv_l)
    _sgm_pair(lib.sde_sgm_8path_wta_pair, "sde_sgm_8path_wta_pair", (cv_l, pen_l, S_l, disp_l),
              (cv_r, pen_r, S_r, disp_r), accumulate, zero_du_penalties)
    return disp_l, disp_r


def sgm_direction(cv_hwd, pen, direction: int, S):
    H, W, D = cv_hwd.shape
    check(lib.sde_sgm_direction(_need(cv_hwd, "cost volume"), _need(pen, "penalties", shape=(H, W, 16)), H, W, D,
                                int(direction), _need(S, "S", shape=(H, W, D)), _stream()), "sde_sgm_direction")
    return S


# ----------------------------------------------------------------------------
# Cross-based cost aggregation (build-defined; the reference has none)
# ----------------------------------------------------------------------------
CBCA_MAX_L1 = 32
SIDES = {"left": SDE_SIDE_LEFT, "right": SDE_SIDE_RIGHT}


def cbca_arms(img, L1=14, tau=0.02, out=None):
    """Cross arms of an f32 [H,W] device image (row-strided views allowed, e.g. the interior of the tower's
    padded input) -> int32-viewed u32 [H,W] packed l | r<<8 | u<<16 | d<<24 (sde_cbca_arms)."""
    if not isinstance(img, torch.Tensor) or img.dim() != 2 or img.dtype != torch.float32 or not img.is_cuda:
        raise ValueError("image must be a 2-D float32 GPU tensor")
    if img.stride(1) != 1:
        raise ValueError("image rows must be contiguous")
    H, W = img.shape
    if out is None:
        out = _empty((H, W), torch.int32, img)
    check(lib.sde_cbca_arms(img.data_ptr(), img.stride(0), H, W, int(L1), float(tau),
                            _need(out, "arms", dtype=torch.int32, shape=(H, W)), _stream()), "sde_cbca_arms")
    return out


def cbca_workspace_bytes(H, W):
    """Bytes of the aggregation workspace (column-major left-image arms, sde_cbca_workspace_bytes)."""
    return int(lib.sde_cbca_workspace_bytes(int(H), int(W)))


def _cbca_ws(ws, H, W, like):
    n = cbca_workspace_bytes(H, W)
    if ws is None:
        return _empty((n,), torch.uint8, like), n
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.numel() * ws.element_size() < n:
        raise ValueError(f"cbca workspace must be a GPU tensor of at least {n} bytes")
    return ws, ws.numel() * ws.element_size()


def cbca(cv_hwd, arms_ref, arms_other, side="left", L1=14, iters=2, tmp=None, workspace=None):
    """In-place cross-based aggregation of an [H,W,D] volume (sde_cbca); tmp: same-size scratch."""
    H, W, D = cv_hwd.shape
    if tmp is None:
        tmp = torch.empty_like(cv_hwd)
    ws, nws = _cbca_ws(workspace, H, W, cv_hwd)
    sd = SIDES[side]
    check(lib.sde_cbca(_need(cv_hwd, "cost volume"), _need(tmp, "tmp", shape=(H, W, D)),
                       _need(arms_ref, "arms_ref", dtype=torch.int32, shape=(H, W)),
                       _need(arms_other, "arms_other", dtype=torch.int32, shape=(H, W)), H, W, D, sd, int(L1),
                       int(iters), ws.data_ptr(), nws, _stream()), "sde_cbca")
    return cv_hwd


def cbca_pair(cv_l, cv_r, arms_l, arms_r, L1=14, iters=2, tmp_l=None, tmp_r=None, workspace=None):
    """cbca(cv_l, arms_l, arms_r, "left") and cbca(cv_r, arms_r, arms_l, "right") for any two volumes
    (sde_cbca_pair), in place; tmp_l / tmp_r: same-size scratch, distinct from every volume."""
    H, W, D = cv_l.shape
    tmp_l = torch.empty_like(cv_l) if tmp_l is None else tmp_l
    tmp_r = torch.empty_like(cv_l) if tmp_r is None else tmp_r
    ws, nws = _cbca_ws(workspace, H, W, cv_l)
    check(lib.sde_cbca_pair(_need(cv_l, "cost volume"), _need(tmp_l, "tmp", shape=(H, W, D)),
                            _need(cv_r, "cost volume", shape=(H, W, D)), _need(tmp_r, "tmp", shape=(H, W, D)),
                            _need(arms_l, "arms_l", dtype=torch.int32, shape=(H, W)),
                            _need(arms_r, "arms_r", dtype=torch.int32, shape=(H, W)), H, W, D, int(L1), int(iters),
                            ws.data_ptr(), nws, _stream()), "sde_cbca_pair")
    return cv_l, cv_r


def cbca_lr(cv_l, cv_r, arms_l, arms_r, L1=14, iters=2, tmp=None, workspace=None):
    """The GPU path's pair (sde_cbca_lr): cv_l aggregated in place, then cv_r's valid voxels set to its
    shear cv_r[y, x, d] = cv_l[y, x + d, d] (x + d < W; the others untouched).  Equal to cbca_pair when
    cv_r's valid voxels are cv_l's shear (as cost_volume(..., right=True) writes them)."""
    H, W, D = cv_l.shape
    tmp = torch.empty_like(cv_l) if tmp is None else tmp
    ws, nws = _cbca_ws(workspace, H, W, cv_l)
    check(lib.sde_cbca_lr(_need(cv_l, "cost volume"), _need(cv_r, "cost volume", shape=(H, W, D)),
                          _need(tmp, "tmp", shape=(H, W, D)),
                          _need(arms_l, "arms_l", dtype=torch.int32, shape=(H, W)),
                          _need(arms_r, "arms_r", dtype=torch.int32, shape=(H, W)), H, W, D, int(L1), int(iters),
                          ws.data_ptr(), nws, _stream()), "sde_cbca_lr")
    return cv_l, cv_r


def cbca_reciprocals(n, device=None):
    """The fp64 reciprocals 1/(i+1), i < n, as the aggregation kernels compute them."""
    out = torch.empty((int(n),), dtype=torch.float64, device=device or torch.device("cuda"))
    check(lib.sde_cbca_reciprocals(out.data_ptr(), int(n), _stream()), "sde_cbca_reciprocals")
    return out


def lr_check(disp_l, disp_r, lrc_l=None, lrc_r=None):
    H, W = disp_l.shape
    if lrc_l is None:
        lrc_l = torch.zeros((H, W), dtype=torch.uint8, device=disp_l.device)
    if lrc_r is None:
        lrc_r = torch.zeros((H, W), dtype=torch.uint8, device=disp_l.device)
    check(lib.sde_lr_check(_need(disp_l, "disp_l"), _need(disp_r, "disp_r", shape=(H, W)), H, W,
                           _need(lrc_l, "lrc_l", dtype=torch.uint8, shape=(H, W)),
                           _need(lrc_r, "lrc_r", dtype=torch.uint8, shape=(H, W)), _stream()), "sde_lr_check")
    return lrc_l, lrc_r


def lr_consistency(disp_l, disp_r, max_diff: float = 1.0, lrc_l=None, lrc_r=None):
    """Left-right consistency flags without lr_check's uint8 column cast (sde_lr_consistency): a left pixel is
    flagged when its disparity d is negative, or x - d is inside the row and |d - disp_r[y, int(x - d)]| >
    max_diff; a right pixel likewise with x + d and disp_l.  Every pixel is written (the buffers need no
    zeroing).  Returns (lrc_l, lrc_r) uint8 [H, W]."""
    H, W = disp_l.shape
    if lrc_l is None:
        lrc_l = _empty((H, W), torch.uint8, disp_l)
    if lrc_r is None:
        lrc_r = _empty((H, W), torch.uint8, disp_l)
    check(lib.sde_lr_consistency(_need(disp_l, "disp_l"), _need(disp_r, "disp_r", shape=(H, W)), H, W,
                                 ctypes.c_float(max_diff), _need(lrc_l, "lrc_l", dtype=torch.uint8, shape=(H, W)),
                                 _need(lrc_r, "lrc_r", dtype=torch.uint8, shape=(H, W)), _stream()),
          "sde_lr_consistency")
    return lrc_l, lrc_r


def lrc_fill(disp_l, lrc_l, out=None):
    H, W = disp_l.shape
    if out is None:
        out = _empty((H, W), torch.float32, disp_l)
    check(lib.sde_lrc_fill(_need(disp_l, "disp_l"), _need(lrc_l, "lrc_l", dtype=torch.uint8, shape=(H, W)), H, W,
                           _need(out, "out", shape=(H, W)), _stream()), "sde_lrc_fill")
    return out


def median5(src, dst):
    H, W = src.shape
    check(lib.sde_median5(_need(src, "src"), H, W, _need(dst, "dst", shape=(H, W)), _stream()), "sde_median5")
    return dst


# ----------------------------------------------------------------------------
# Sub-pixel disparities and the 9x9 bilateral filter (process_functional.py:813-819, :882-974; both switched off in
# the reference; definitions in include/sde.h)
# ----------------------------------------------------------------------------
def wta_subpixel(vol, layout: str = "DHW", rule: str = "inf", out=None):
    """wta(vol, layout, rule) followed by the parabola step on the winner's two neighbours in the stored volume
    (sde_wta_subpixel): a winner at d = 0 or D - 1, a non-finite neighbour, a parabola that is not convex and a
    pixel without a winner (-1) keep the integer."""
    return _wta_volume(lib.sde_wta_subpixel, "sde_wta_subpixel", vol, layout, rule, out)


def cv_subpixel(fl, fr, d0: int, d1: int, disp, side: str = "left", out=None):
    """The parabola step on a map of cv_wta (side 'left') or cv_wta_right ('right') over [d0, d1), whose volume was
    never stored: the three costs around every integer pixel of `disp` are recomputed in the cost volume's exact
    arithmetic (sde_cv_subpixel), so the result equals wta_subpixel of the stored DHW volume.  Anything that is
    not an integer in [d0, d1) is copied through.  out may be `disp` itself (in place); a new map when None."""
    pl, pr, H, W, C = _feat_pair(fl, fr)
    if side not in SIDES:
        raise ValueError(f"side must be 'left' or 'right' (got {side!r})")
    pi = _need(disp, "disp", shape=(H, W))
    if out is None:
        out = _empty((H, W), torch.float32, fl)
    po = _need(out, "out", shape=(H, W))
    check(lib.sde_cv_subpixel(pl, pr, H, W, C, int(d0), int(d1), SIDES[side], pi, po, _stream()), "sde_cv_subpixel")
    return out


# ----------------------------------------------------------------------------
# Uniqueness check (build-defined; definition in include/sde_unique.h)
# ----------------------------------------------------------------------------
def unique_tau(tau) -> float:
    """tau as the float32 the kernels compare against: a finite number >= 0."""
    with np.errstate(over="ignore"):
        t = float(np.float32(tau))
    if not (0.0 <= t < float("inf")):
        raise ValueError(f"the uniqueness margin must be a finite float32 >= 0 (got {tau!r})")
    return t


def wta_unique(vol, tau: float, layout: str = "DHW", rule: str = "inf", disp=None, want=("margin", "reject"),
               margin=None, reject=None):
    """The uniqueness check on a stored volume (sdu_wta_unique): with i = wta(vol, layout, rule)'s winner, c1 its
    cost and c2 the smallest cost at |d - i| >= 2 (+inf if there is none), margin = 0 if c2 == c1 else c2 - c1 and
    reject = margin < tau.  `disp`, when given, is masked in place: -1 where rejected, untouched elsewhere (so a
    map wta_subpixel refined keeps its fractions).  Returns (margin f32, reject u8): each is written when named in
    `want` or given, None otherwise."""
    if vol.dim() != 3:
        raise ValueError("volume must be 3-D")
    if layout == "DHW":
        D, H, W = vol.shape
    else:
        H, W, D = vol.shape
    pv = _need(vol, "volume")
    if "margin" in want and margin is None:
        margin = _empty((H, W), torch.float32, vol)
    if "reject" in want and reject is None:
        reject = _empty((H, W), torch.uint8, vol)
    pm = _need(margin, "margin", shape=(H, W)) if margin is not None else None
    pr = _need(reject, "reject", dtype=torch.uint8, shape=(H, W)) if reject is not None else None
    pd = _need(disp, "disp", shape=(H, W)) if disp is not None else None
    check(lib.sdu_wta_unique(pv, H, W, D, LAYOUTS[layout], RULES[rule], ctypes.c_float(unique_tau(tau)), pm, pr, pd,
                             _stream()), "sdu_wta_unique")
    return margin, reject


def cv_wta_unique(fl, fr, d0: int, d1: int, tau: float, side: str = "left", disp=None, min_cost=None, argmin=None,
                  reject=None, want=("disp", "reject"), mode: str = "certified", workspace=None):
    """cv_wta (side 'left') or cv_wta_right ('right') with the uniqueness check (sdu_cv_wta_unique): disp is -1
    where the winner's margin over the best cost at |d - i| >= 2 is below tau, min_cost / argmin stay the winner's,
    reject (u8) is the decision.  Modes, workspace and cv_wta_fixups as for cv_wta (identical outputs; the
    certified row sweep decides a pixel only when its fast margin is further from tau than the error bound).
    Returns (disp, min_cost, argmin, reject)."""
    pl, pr, H, W, C = _feat_pair(fl, fr)
    if side not in SIDES:
        raise ValueError(f"side must be 'left' or 'right' (got {side!r})")
    (disp, min_cost, argmin), (pd, pm, pa) = _wta_outputs(fl, H, W, want, disp, min_cost, argmin)
    if "reject" in want and reject is None:
        reject = _empty((H, W), torch.uint8, fl)
    prj = _need(reject, "reject", dtype=torch.uint8, shape=(H, W)) if reject is not None else None
    md = CV_MODES[mode]
    pws, wsb = None, 0
    if md == _lib.SDE_CV_CERTIFIED:
        if workspace is None:
            workspace = torch.empty(cv_wta_workspace_bytes(H, W), dtype=torch.uint8, device=fl.device)
        pws, wsb = _need(workspace, "workspace", dtype=torch.uint8), workspace.numel()
    check(lib.sdu_cv_wta_unique(pl, pr, H, W, C, int(d0), int(d1), SIDES[side], ctypes.c_float(unique_tau(tau)), pd, pm, pa,
                                prj, md, pws, wsb, _stream()), "sdu_cv_wta_unique")
    return disp, min_cost, argmin, reject


def bilateral9(img_u8, src, out=None):
    """Bilateral_Filter_kernel (process_functional.py:882-974) for one view: the 9x9 window of `src` f32 [H,W]
    weighted by the intensity difference in img_u8 [H,W] (taps with a difference of 5 or more are rejected, zero
    padding outside the image) -> f32 [H,W], every pixel written; out must not be src (sde_bilateral9)."""
    if img_u8.dim() != 2:
        raise ValueError("image must be a uint8 [H,W] tensor")
    H, W = img_u8.shape
    pi = _need(img_u8, "image", dtype=torch.uint8)
    ps = _need(src, "src", shape=(H, W))
    if out is None:
        out = _empty((H, W), torch.float32, src)
    check(lib.sde_bilateral9(pi, ps, H, W, _need(out, "out", shape=(H, W)), _stream()), "sde_bilateral9")
    return out


# ----------------------------------------------------------------------------
# Local matcher: SAD+SSD, rank and census (local_mathod.py:13-165; definitions in include/sde.h)
# ----------------------------------------------------------------------------
LOCAL_INVALID = _lib.SDE_LOCAL_INVALID
LOCAL_MAX_RADIUS = _lib.SDE_LOCAL_MAX_RADIUS


def _transform(fn, what, imgs, out, dtype, name):
    """A per-pixel transform of u8 [H,W] or [N,H,W] images into `dtype` words of the same shape, all images per
    launch."""
    if not isinstance(imgs, torch.Tensor) or imgs.dim() not in (2, 3):
        raise ValueError("images must be a uint8 [H,W] or [N,H,W] tensor")
    p = _need(imgs, "images", dtype=torch.uint8)
    H, W = imgs.shape[-2:]
    if out is None:
        out = _empty(tuple(imgs.shape), dtype, imgs)
    check(fn(p, imgs.shape[0] if imgs.dim() == 3 else 1, H, W, _need(out, name, dtype=dtype, shape=tuple(imgs.shape)),
             _stream()), what)
    return out


def census_transform(imgs, out=None):
    """u8 [H,W] or [N,H,W] -> the 19-bit census words as int32 of the same shape (sde_census_transform)."""
    return _transform(lib.sde_census_transform, "sde_census_transform", imgs, out, torch.int32, "census")


def rank_transform(imgs, out=None):
    """u8 [H,W] or [N,H,W] -> the 7x7 rank (1..49) as uint8 of the same shape (sde_rank_transform)."""
    return _transform(lib.sde_rank_transform, "sde_rank_transform", imgs, out, torch.uint8, "rank")


def _census_pair(census_l, census_r):
    if not isinstance(census_l, torch.Tensor) or census_l.dim() != 2:
        raise ValueError("census words must be int32 [H,W] tensors")
    H, W = census_l.shape
    return (_need(census_l, "census_l", dtype=torch.int32), _need(census_r, "census_r", dtype=torch.int32, shape=(H, W)),
            H, W)


def census_cost(census_l, census_r, ndisp: int, invalid: float = LOCAL_INVALID, left: bool = True,
                right: bool = False, out_left=None, out_right=None):
    """The Hamming volumes f32 [H,W,D] (sde_census_cost): the left one, (left, right) with right=True, the
    right one alone with left=False."""
    pl, pr, H, W = _census_pair(census_l, census_r)
    ol, orr, result = _lr_volumes((H, W, int(ndisp)), census_l, left, right, out_left, out_right)
    check(lib.sde_census_cost(pl, pr, H, W, int(ndisp), ctypes.c_float(invalid), ol, orr, _stream()),
          "sde_census_cost")
    return result


def census_wta(census_l, census_r, ndisp: int, left: bool = True, right: bool = True, want_min: bool = False,
               disp_l=None, min_l=None, disp_r=None, min_r=None):
    """Hamming cost + first-minimum WTA of both views in one pass, no volume (sde_census_wta).
    Returns (disp_l, min_l, disp_r, min_r); the entries not asked for are None."""
    pl, pr, H, W = _census_pair(census_l, census_r)
    if not left and not right:
        raise ValueError("nothing to compute")

    def view(on, disp, mn):
        if not on:
            return None, None
        if disp is None:
            disp = _empty((H, W), torch.float32, census_l)
        if want_min and mn is None:
            mn = _empty((H, W), torch.float32, census_l)
        return disp, mn

    disp_l, min_l = view(left, disp_l, min_l)
    disp_r, min_r = view(right, disp_r, min_r)
    ptr = lambda t, n: _need(t, n, shape=(H, W)) if t is not None else None   # noqa: E731
    check(lib.sde_census_wta(pl, pr, H, W, int(ndisp), ptr(disp_l, "disp_l"), ptr(min_l, "min_l"),
                             ptr(disp_r, "disp_r"), ptr(min_r, "min_r"), _stream()), "sde_census_wta")
    return disp_l, min_l, disp_r, min_r


def _image_pair(img_l, img_r):
    if not isinstance(img_l, torch.Tensor) or img_l.dim() != 2:
        raise ValueError("images must be uint8 [H,W] tensors")
    H, W = img_l.shape
    return _need(img_l, "img_l", dtype=torch.uint8), _need(img_r, "img_r", dtype=torch.uint8, shape=(H, W)), H, W


def _ad_rule(W, ndisp, radius):
    if W < ndisp + 2 * radius:
        raise ValueError(f"the SAD+SSD window needs W >= D + 2k (got W = {W}, D = {ndisp}, k = {radius}): the "
                         "reference reads column x + k out of bounds otherwise")


def ad_cost(img_l, img_r, ndisp: int, radius: int, invalid: float = LOCAL_INVALID, out=None):
    """The SAD+SSD volume f32 [H,W,D] of two u8 images (sde_ad_cost); W >= D + 2 * radius."""
    pl, pr, H, W = _image_pair(img_l, img_r)
    _ad_rule(W, int(ndisp), int(radius))
    if out is None:
        out = _empty((H, W, int(ndisp)), torch.float32, img_l)
    check(lib.sde_ad_cost(pl, pr, H, W, int(ndisp), int(radius), ctypes.c_float(invalid),
                          _need(out, "out", shape=(H, W, int(ndisp))), _stream()), "sde_ad_cost")
    return out


def ad_wta(img_l, img_r, ndisp: int, radius: int, want_min: bool = False, disp=None, min_cost=None):
    """SAD+SSD cost + first-minimum WTA, no volume (sde_ad_wta).  Returns (disp, min_cost or None)."""
    pl, pr, H, W = _image_pair(img_l, img_r)
    _ad_rule(W, int(ndisp), int(radius))
    if disp is None:
        disp = _empty((H, W), torch.float32, img_l)
    if want_min and min_cost is None:
        min_cost = _empty((H, W), torch.float32, img_l)
    pm = _need(min_cost, "min_cost", shape=(H, W)) if min_cost is not None else None
    check(lib.sde_ad_wta(pl, pr, H, W, int(ndisp), int(radius), _need(disp, "disp", shape=(H, W)), pm, _stream()),
          "sde_ad_wta")
    return disp, min_cost


# ----------------------------------------------------------------------------
# training step (train.py:71-99): gather, loss + gradients, momentum update
# ----------------------------------------------------------------------------
def train_param_floats(nlayers: int, nf: int = 64) -> int:
    n = lib.sde_train_param_floats(int(nlayers), int(nf))
    if n < 0:
        raise ValueError(f"unsupported training shape nlayers={nlayers} nf={nf}")
    return int(n)


def train_workspace_bytes(B: int, nlayers: int, nf: int = 64) -> int:
    n = lib.sde_train_workspace_bytes(int(B), int(nlayers), int(nf))
    if n < 0:
        raise ValueError(f"unsupported training shape B={B} nlayers={nlayers} nf={nf}")
    return int(n)


def train_gather(img_l, img_r, idx, nlayers: int, out=None):
    """f32 [H,W] normalised images + int32 [B,4] centres (y, x_left, x_pos, x_neg) -> patches f32 [3,B,P,P]
    (sde_train_gather); pixels outside the image read 0."""
    if img_l.dim() != 2 or tuple(img_l.shape) != tuple(img_r.shape):
        raise ValueError(f"images must be matching [H,W] tensors, got {tuple(img_l.shape)} / {tuple(img_r.shape)}")
    H, W = img_l.shape
    if idx.dim() != 2 or idx.shape[1] != 4:
        raise ValueError(f"idx must be [B,4], got {tuple(idx.shape)}")
    B, P = idx.shape[0], 2 * int(nlayers) + 1
    if out is None:
        out = _empty((3, B, P, P), torch.float32, img_l)
    check(lib.sde_train_gather(_need(img_l, "img_l"), _need(img_r, "img_r"), H, W,
                               _need(idx, "idx", dtype=torch.int32), B, int(nlayers),
                               _need(out, "patches", shape=(3, B, P, P)), _stream()), "sde_train_gather")
    return out


def train_loss_grad(patches, params, nlayers: int, margin: float, loss=None, grads=None, workspace=None,
                    nf: int = 64, want_grads: bool = True):
    """patches f32 [3,B,P,P], params f32 blob -> (loss f32 [1+B] = mean then every h_i, grads blob or None)
    (sde_train_loss_grad).  want_grads=False runs the forward pass only."""
    P = 2 * int(nlayers) + 1
    if patches.dim() != 4 or patches.shape[0] != 3:
        raise ValueError(f"patches must be [3,B,{P},{P}], got {tuple(patches.shape)}")
    B = patches.shape[1]
    n = train_param_floats(nlayers, nf)
    if loss is None:
        loss = _empty((1 + B,), torch.float32, patches)
    if want_grads and grads is None:
        grads = _empty((n,), torch.float32, patches)
    if workspace is None:
        workspace = torch.empty(train_workspace_bytes(B, nlayers, nf), dtype=torch.uint8, device=patches.device)
    pg = _need(grads, "grads", shape=(n,)) if want_grads else None
    check(lib.sde_train_loss_grad(_need(patches, "patches", shape=(3, B, P, P)), B, _need(params, "params", shape=(n,)),
                                  int(nlayers), int(nf), ctypes.c_float(margin), _need(loss, "loss", shape=(1 + B,)),
                                  pg, _need(workspace, "workspace", dtype=torch.uint8), workspace.numel(), _stream()),
          "sde_train_loss_grad")
    return loss, (grads if want_grads else None)


def train_export_activations(workspace, B: int, nlayers: int, layer: int, nf: int = 64, out=None):
    """What the last train_loss_grad on `workspace` kept for the 1-based `layer`: f32 [3B,h,w,nf] post-ReLU
    output (layer < nlayers) or the normalised features [3B,nf] (layer == nlayers)."""
    s = 2 * (int(nlayers) - int(layer)) + 1
    shape = (3 * B, nf) if layer == nlayers else (3 * B, s, s, nf)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=workspace.device)
    check(lib.sde_train_export_activations(_need(workspace, "workspace", dtype=torch.uint8), int(B), int(nlayers),
                                           int(nf), int(layer), _need(out, "out", shape=shape), _stream()),
          "sde_train_export_activations")
    return out


def train_momentum(params, velocity, grads, lr: float, beta: float):
    """In place: v = beta * v + g; p = p - lr * v, one fp32 rounding per operation (sde_train_momentum)."""
    n = params.numel()
    check(lib.sde_train_momentum(_need(params, "params", shape=(n,)), _need(velocity, "velocity", shape=(n,)),
                                 _need(grads, "grads", shape=(n,)), n, ctypes.c_float(lr), ctypes.c_float(beta),
                                 _stream()), "sde_train_momentum")
    return params


# ----------------------------------------------------------------------------
# training from resident scenes (image_patches_prepare/*.py) and the bad-pixel score (error_calculate.py)
# ----------------------------------------------------------------------------
def triplet_centres(disp_l, disp_r, nlayers: int, zero_is_invalid: bool = True, out=None, count=None):
    """f32 [H,W] disparity maps (disp_r may be None) -> (centres int32 [H*W], count int32 [1]): the first
    count[0] entries hold y*W + x of every valid patch centre in ascending order (sde_triplet_centres)."""
    if disp_l.dim() != 2 or (disp_r is not None and tuple(disp_r.shape) != tuple(disp_l.shape)):
        raise ValueError(f"disparity maps must be matching [H,W] tensors, got {tuple(disp_l.shape)}"
                         + ("" if disp_r is None else f" / {tuple(disp_r.shape)}"))
    H, W = disp_l.shape
    if out is None:
        out = _empty((H * W,), torch.int32, disp_l)
    if count is None:
        count = _empty((1,), torch.int32, disp_l)
    pr = None if disp_r is None else _need(disp_r, "disp_r")
    check(lib.sde_triplet_centres(_need(disp_l, "disp_l"), pr, H, W, int(nlayers),
                                  _lib.SDE_ZERO_IS_INVALID if zero_is_invalid else 0,
                                  _need(out, "centres", dtype=torch.int32, shape=(H * W,)),
                                  _need(count, "count", dtype=torch.int32, shape=(1,)), _stream()),
          "sde_triplet_centres")
    return out, count


def train_sample_gather(table, N: int, B: int, nlayers: int, seed: int, step: int, max_rounds: int = 32, out=None,
                        idx=None, scene=None):
    """Scene table int64 [S,8] (include/sde.h; its addresses are trusted) -> patches f32 [3,B,P,P] of B triplets
    drawn on the device from (seed, step) (sde_train_sample_gather).  idx int32 [B,4] / scene int32 [B], when
    given, receive (y, x_left, x_pos, x_neg) and the scene number of every triplet."""
    if table.dim() != 2 or table.shape[1] != _lib.SDE_SCENE_WORDS:
        raise ValueError(f"table must be [S,{_lib.SDE_SCENE_WORDS}], got {tuple(table.shape)}")
    S, B, P = table.shape[0], int(B), 2 * int(nlayers) + 1
    if out is None:
        out = _empty((3, B, P, P), torch.float32, table)
    pi = None if idx is None else _need(idx, "idx", dtype=torch.int32, shape=(B, 4))
    ps = None if scene is None else _need(scene, "scene", dtype=torch.int32, shape=(B,))
    mask = (1 << 64) - 1
    check(lib.sde_train_sample_gather(_need(table, "table", dtype=torch.int64), S, int(N), B, int(nlayers),
                                      int(seed) & mask, int(step) & mask, int(max_rounds),
                                      _need(out, "patches", shape=(3, B, P, P)), pi, ps, _stream()),
          "sde_train_sample_gather")
    return out


def bad_pixels(disp, gt, threshold: float = 1.0, counts=None, area=None):
    """f32 [H,W] result and ground truth -> counts uint32-in-int32 [2] = (evaluated, bad), ADDED to what `counts`
    holds (a fresh zeroed pair when None); area uint8 [H,W,3], when given, is the reference's error picture
    (sde_bad_pixels)."""
    if disp.dim() != 2 or tuple(gt.shape) != tuple(disp.shape):
        raise ValueError(f"disp and gt must be matching [H,W] tensors, got {tuple(disp.shape)} / {tuple(gt.shape)}")
    H, W = disp.shape
    if counts is None:
        counts = torch.zeros(2, dtype=torch.int32, device=disp.device)
    pa = None if area is None else _need(area, "area", dtype=torch.uint8, shape=(H, W, 3))
    check(lib.sde_bad_pixels(_need(disp, "disp"), _need(gt, "gt"), H, W, float(threshold),
                             _need(counts, "counts", dtype=torch.int32, shape=(2,)), pa, _stream()), "sde_bad_pixels")
    return counts


# ----------------------------------------------------------------------------
# geometry stage (include/sde_geom.h): rectification maps, remap, reprojection
# ----------------------------------------------------------------------------
NO_SAMPLE = _lib.SDG_NO_SAMPLE


def _host_f64(a, n: int, name: str):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"{name} must hold {n} numbers (got {a.size})")
    return a


def rectify_map(cal, H: int, W: int, out=None, device=None):
    """The int32 [H,W,2] sampling map of one camera in 1/32 pixel (sdg_rectify_map) from `cal`, 26 host float64:
    K (9), dist (8), inverse of P[:, :3] @ R (9).  out: a device tensor to fill, else one is made on `device`."""
    cal = _host_f64(cal, 26, "cal")
    if out is None:
        out = torch.empty((H, W, 2), dtype=torch.int32, device=device if device is not None else "cuda")
    check(lib.sdg_rectify_map(cal.ctypes.data, int(H), int(W), _need(out, "map", dtype=torch.int32, shape=(H, W, 2)),
                              _stream()), "sdg_rectify_map")
    return out


def remap_u8(src, maps, out=None, valid=None):
    """u8 [N,Hs,Ws] sources through int32 [N,H,W,2] maps -> u8 [N,H,W] (sdg_remap_u8), image i through map i, one
    launch.  valid: optional u8 [N,H,W], 1 where every tap read was inside the source."""
    if src.dim() != 3 or maps.dim() != 4 or maps.shape[0] != src.shape[0] or maps.shape[3] != 2:
        raise ValueError(f"src must be [N,Hs,Ws] and maps [N,H,W,2], got {tuple(src.shape)} / {tuple(maps.shape)}")
    N, Hs, Ws = src.shape
    _, H, W, _ = maps.shape
    if out is None:
        out = _empty((N, H, W), torch.uint8, src)
    po = _need(out, "out", dtype=torch.uint8, shape=(N, H, W))
    ps = _need(src, "src", dtype=torch.uint8)
    if ps < po + N * H * W and po < ps + N * Hs * Ws:
        raise ValueError("out must not overlap src")
    pv = None if valid is None else _need(valid, "valid", dtype=torch.uint8, shape=(N, H, W))
    check(lib.sdg_remap_u8(ps, N, Hs, Ws, _need(maps, "maps", dtype=torch.int32), H, W, po, pv, _stream()),
          "sdg_remap_u8")
    return out


def reproject(disp, Q, min_disp: float = 0.0, depth=None, xyz=None, want=("depth",)):
    """f32 [H,W] disparities through the 4x4 matrix Q (16 host float64) -> (depth f32 [H,W], xyz f32 [H,W,3])
    (sdg_reproject); an output is computed when given or named in `want`, else None.  Pixels that are not finite
    or not above min_disp get 0."""
    if disp.dim() != 2:
        raise ValueError(f"disp must be [H,W], got {tuple(disp.shape)}")
    H, W = disp.shape
    Q = _host_f64(Q, 16, "Q")
    if depth is None and "depth" in want:
        depth = _empty((H, W), torch.float32, disp)
    if xyz is None and "xyz" in want:
        xyz = _empty((H, W, 3), torch.float32, disp)
    pd = None if depth is None else _need(depth, "depth", shape=(H, W))
    px = None if xyz is None else _need(xyz, "xyz", shape=(H, W, 3))
    check(lib.sdg_reproject(_need(disp, "disp"), H, W, Q.ctypes.data, float(min_disp), pd, px, _stream()),
          "sdg_reproject")
    return depth, xyz


# ---------------------------------------------------------------- filters (include/sde_filter.h)
def speckle_workspace_bytes(H: int, W: int) -> int:
    """Bytes of sdf_speckle's workspace for an H x W map (sdf_speckle_workspace_bytes)."""
    return int(lib.sdf_speckle_workspace_bytes(int(H), int(W)))


def speckle(disp, max_size: int, max_diff: float = 1.0, fill: float = -1.0, out=None, mask=None, sizes=None,
            want=("out",), workspace=None):
    """Speckle removal of an f32 [H,W] disparity map (sdf_speckle) -> (out f32, mask u8, sizes i32), each [H,W]:
    the regions of 4-connected valid (finite, >= 0) pixels whose neighbours differ by at most max_diff are
    labelled on the device, and every region of at most max_size pixels is set to `fill` in out and to 1 in mask;
    sizes holds each valid pixel's region size.  out is always computed (out=disp filters in place); mask and
    sizes when given or named in `want`, else None.  workspace: a GPU tensor of speckle_workspace_bytes(H, W)
    bytes, 4-byte aligned, contents arbitrary; one is allocated when absent."""
    if disp.dim() != 2:
        raise ValueError(f"disp must be [H,W], got {tuple(disp.shape)}")
    H, W = disp.shape
    if out is None:
        out = _empty((H, W), torch.float32, disp)
    if mask is None and "mask" in want:
        mask = _empty((H, W), torch.uint8, disp)
    if sizes is None and "sizes" in want:
        sizes = _empty((H, W), torch.int32, disp)
    n = speckle_workspace_bytes(H, W)
    if workspace is None:
        workspace = _empty((n,), torch.uint8, disp)
    elif not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("speckle workspace must be a contiguous GPU tensor")
    pm = None if mask is None else _need(mask, "mask", dtype=torch.uint8, shape=(H, W))
    ps = None if sizes is None else _need(sizes, "sizes", dtype=torch.int32, shape=(H, W))
    check(lib.sdf_speckle(_need(disp, "disp"), H, W, int(max_size), float(max_diff), float(fill),
                          _need(out, "out", shape=(H, W)), pm, ps, workspace.data_ptr(),
                          workspace.numel() * workspace.element_size(), _stream()), "sdf_speckle")
    return out, mask, sizes


# ---------------------------------------------------------------- interpolation (include/sde_interp.h)
SIDES = {"left": SDE_SIDE_LEFT, "right": SDE_SIDE_RIGHT}
# what a checked path does with its flagged pixels: sde_lrc_fill, or classify + interpolate
FILLS = ("mean4", "interpolate")


def fill_mode(fill) -> str:
    """A checked path's fill= option, or ValueError."""
    if fill not in FILLS:
        raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
    return fill


def _side(side):
    if side not in SIDES:
        raise ValueError("side must be 'left' or 'right'")
    return SIDES[side]


def classify(disp_other, lrc, ndisp: int, side: str = "left", max_diff: float = 1.0, out=None):
    """Flagged pixels of one view into occlusions and mismatches (sdi_classify) -> cls u8 [H,W]: 0 unflagged
    (lrc byte != 1), 2 where some integer disparity in [0, ndisp) makes the pixel consistent with the OTHER view's
    map disp_other within max_diff, 1 otherwise.  out=lrc classifies in place."""
    if disp_other.dim() != 2:
        raise ValueError(f"disp_other must be [H,W], got {tuple(disp_other.shape)}")
    H, W = disp_other.shape
    if out is None:
        out = _empty((H, W), torch.uint8, disp_other)
    check(lib.sdi_classify(_need(disp_other, "disp_other"), _need(lrc, "lrc", dtype=torch.uint8, shape=(H, W)), H, W,
                           int(ndisp), _side(side), float(max_diff), _need(out, "out", dtype=torch.uint8, shape=(H, W)),
                           _stream()), "sdi_classify")
    return out


def interpolate_workspace_bytes(H: int, W: int) -> int:
    """Bytes of sdi_interpolate's workspace for an H x W map (sdi_interpolate_workspace_bytes)."""
    return int(lib.sdi_interpolate_workspace_bytes(int(H), int(W)))


def interpolate(disp, cls, side: str = "left", out=None, filled=None, want=("out",), workspace=None):
    """Interpolation of the classified pixels of an f32 [H,W] map (sdi_interpolate) -> (out f32, filled u8): an
    occlusion (cls 1) takes the nearest source of its row on the background side (left of it for the left view),
    a mismatch (cls 2) the median of the first sources along 16 rays; a source is a cls-0 pixel with a finite
    value >= 0.  out must not be disp.  filled (1 where a value was taken) when given or named in `want`, else
    None.  workspace: a GPU tensor of interpolate_workspace_bytes(H, W) bytes, 4-byte aligned, contents arbitrary;
    one is allocated when absent."""
    if disp.dim() != 2:
        raise ValueError(f"disp must be [H,W], got {tuple(disp.shape)}")
    H, W = disp.shape
    if out is None:
        out = _empty((H, W), torch.float32, disp)
    if filled is None and "filled" in want:
        filled = _empty((H, W), torch.uint8, disp)
    if workspace is None:
        workspace = _empty((interpolate_workspace_bytes(H, W),), torch.uint8, disp)
    elif not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("interpolate workspace must be a contiguous GPU tensor")
    pf = None if filled is None else _need(filled, "filled", dtype=torch.uint8, shape=(H, W))
    check(lib.sdi_interpolate(_need(disp, "disp"), _need(cls, "cls", dtype=torch.uint8, shape=(H, W)), H, W,
                              _side(side), _need(out, "out", shape=(H, W)), pf, workspace.data_ptr(),
                              workspace.numel() * workspace.element_size(), _stream()), "sdi_interpolate")
    return out, filled
