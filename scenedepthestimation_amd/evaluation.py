"""The bad-pixel rate of a disparity map against ground truth (the reference's error_calculate.py:58-88).

A pixel whose ground truth is +inf or 0 is unknown and skipped; any other is bad when the result is off by more
than `threshold`.  The reference divides the bad pixels by ALL pixels of the image (`rate_over_image`); the
rate over the pixels that were evaluated is reported next to it.  Counting runs on the device (ops.bad_pixels).
"""
from __future__ import annotations

import numpy as np


def halve(a) -> np.ndarray:
    """[H][W] -> [H//2][W//2] by the mean of each 2x2 block, float32 (a last odd row / column is dropped).

    This is what cv2.resize(a, (W//2, H//2)) computes at exactly half size (bilinear, each output sample midway
    between four inputs), as middlebury_2014.py:119-122 halves images and maps.  cv2 is absent here: parity of the
    last bit (its order of the three additions, and its rounding of 8-bit images) is unpinned.  A block holding an
    unknown (inf) disparity comes out inf or NaN, as it does there."""
    a = np.asarray(a)
    H, W = a.shape[0] // 2 * 2, a.shape[1] // 2 * 2
    f = a[:H, :W].astype(np.float32)
    with np.errstate(invalid="ignore"):
        return ((f[0::2, 0::2] + f[0::2, 1::2]) + (f[1::2, 0::2] + f[1::2, 1::2])) * np.float32(0.25)


def halve_u8(img) -> np.ndarray:
    """`halve` for an 8-bit image: rounded half up, as cv2 rounds its fixed-point 8-bit resize."""
    return np.floor(halve(img) + np.float32(0.5)).astype(np.uint8)


def _device_counts(disp, gt, threshold, want_area):
    import torch

    from . import ops

    def dev(a):
        if isinstance(a, torch.Tensor):
            return a.to(device="cuda" if not a.is_cuda else a.device, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()      # a copy: `a` may be read-only

    d, g = dev(disp), dev(gt)
    area = torch.empty(tuple(d.shape) + (3,), dtype=torch.uint8, device=d.device) if want_area else None
    counts = ops.bad_pixels(d, g, threshold, area=area)
    ev, bad = (int(v) for v in counts.cpu().numpy().view(np.uint32))
    return ev, bad, (area.cpu().numpy() if want_area else None)


def bad_pixel_rate(disp, gt, threshold: float = 1.0, area: bool = False) -> dict:
    """disp, gt: [H][W] arrays or tensors of one shape (any real dtype; compared as float32 widened to double).
    -> {evaluated, bad, rate_over_image = bad / (H*W) (the reference's figure), rate_over_evaluated (NaN when no
    pixel was evaluated)} and, with area=True, `area` uint8 [H][W][3]: skipped black, good (0,255,0), bad (0,0,255)."""
    if tuple(disp.shape) != tuple(gt.shape) or len(disp.shape) != 2:
        raise ValueError(f"disp and gt must share one [H][W] shape, got {tuple(disp.shape)} / {tuple(gt.shape)}")
    ev, bad, pic = _device_counts(disp, gt, float(threshold), area)
    H, W = disp.shape
    out = {"evaluated": ev, "bad": bad, "rate_over_image": bad / (H * W),
           "rate_over_evaluated": bad / ev if ev else float("nan")}
    if area:
        out["area"] = pic
    return out
