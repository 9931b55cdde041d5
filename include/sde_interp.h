/*
 * sde_interp.h -- C ABI of the interpolation of left-right-flagged pixels (exported by the same libsde.so).
 *
 * What sde.h's sde_lrc_fill does with a pixel the left-right check flagged is the reference's LRC_kernel: the mean
 * of the nearest unflagged pixels above, below, right and left.  For an occluded pixel that mean mixes foreground
 * and background and gives disparities that exist nowhere in the scene.  The interpolation step of the MC-CNN
 * pipeline (Zbontar & LeCun 2016, sec. 4.3, after Mei et al. 2011) is what stands here instead: a flagged pixel is
 * an OCCLUSION when no disparity would make it consistent with the other view, else a MISMATCH; an occlusion takes
 * the nearest good value on the background side, a mismatch the median of the nearest good values along 16 rays.
 *
 * Conventions are sde.h's: device pointers owned by the caller, nothing allocates, frees or synchronises, every
 * call is stream-ordered and capturable into a hipGraph, `stream` is a hipStream_t passed as void*, the return
 * value is SDE_OK or a negative sde_status, and errors are detected before any launch (argument checks) or right
 * after it.  The functions are additive: SDE_ABI_VERSION stays 4, and the other headers stay as they are.
 *
 * BUILD-DEFINED: WHDY/SceneDepthEstimation has no such stage.  The definition is stated in full below and restated
 * in plain Python loops under tests/ (bit-exact against that restatement: every output is a copy of an input value
 * or +0.0, and no arithmetic other than `+ 0.0f` touches a disparity).
 *
 * All maps are [H][W], row-major.  valid(v): v is finite and v >= 0.0f; -0.0f is valid, -1 ("no winner"), other
 * negatives, NaN and +-inf are not.
 */
#ifndef SDE_INTERP_H
#define SDE_INTERP_H

#include "sde.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Classification of the flagged pixels of one view.  lrc (uint8) is the flag map of sde_lr_check or
 * sde_lr_consistency for that view: a byte == 1 means flagged, any other byte unflagged (as in sde_lrc_fill).
 * disp_other is the OTHER view's disparity map.  D is the number of disparities.
 *
 *   side = SDE_SIDE_LEFT, pixel (y, x):
 *     cls = 0  if the pixel is unflagged;
 *     cls = 2  (mismatch) if an integer dh exists with 0 <= dh <= min(D - 1, x) such that v = disp_other[y][x - dh]
 *              is valid and NOT ((double)dh - (double)v > max_diff  or  (double)dh - (double)v < -max_diff): the
 *              float64 compare of sde_lr_consistency, max_diff widened to float64, so |dh - v| == max_diff counts
 *              as consistent;
 *     cls = 1  (occlusion) otherwise.
 *   side = SDE_SIDE_RIGHT: the same with the column x + dh and the range 0 <= dh <= min(D - 1, W - 1 - x).
 *
 * Every byte of cls is written.  cls == lrc (in place) is allowed; any other overlap is not.
 * SDE_ERR_ARG: a null disp_other, lrc or cls; H, W or D < 1; H*W > 2^31 - 1; a side other than the two; max_diff
 * negative, NaN or infinite.  All checks return before any launch.  One launch.
 */
int sdi_classify(const float *disp_other, const uint8_t *lrc, int H, int W, int D, int side, float max_diff,
                 uint8_t *cls, void *stream);

/* Device workspace bytes needed by sdi_interpolate for an H x W map (0 for a shape sdi_interpolate refuses). */
int64_t sdi_interpolate_workspace_bytes(int H, int W);

/*
 * Interpolation of the classified pixels of one view's map.  cls (uint8) is sdi_classify's output; a byte other
 * than 1 and 2 reads as 0.
 *
 * Sources.  A source is a pixel q with cls[q] == 0 and valid(disp[q]); its value is disp[q] + 0.0f, so a -0.0
 *   source reads as +0.0.  Every value is a non-negative finite float, so a median over values is unique by bits.
 *   Sources are always pixels of disp: a filled pixel is never a source, the result does not depend on the order of
 *   evaluation, and there is one pass.
 * cls == 0:  out = disp bit for bit (NaN payloads and -0.0 included), filled = 0.
 * cls == 1 (occlusion), side = SDE_SIDE_LEFT:  the value of the nearest source in the same row with x' < x; if
 *   there is none, of the nearest with x' > x; if the row has no source, out = disp bit for bit and filled = 0.
 *   side = SDE_SIDE_RIGHT looks at x' > x first, then x' < x.
 * cls == 2 (mismatch):  16 rays.  The directions are the integer pairs (a, b) with max(|a|, |b|) == 2.  Step
 *   i = 1, 2, ... of the ray (a, b) from (x, y) is the pixel (x + o(a, i), y + o(b, i)) with o(+-2, i) = +-i,
 *   o(+-1, i) = +-ceil(i / 2), o(0, i) = 0: the ray (2, 1) visits (1,1), (2,1), (3,2), (4,2), ...  A ray yields the
 *   value of the first source among its steps, and nothing once a step leaves the image.  With n >= 1 values, out
 *   is element n / 2 (integer division) of the values sorted ascending, filled = 1; with n == 0, out = disp bit for
 *   bit, filled = 0.  side plays no part.
 * filled (uint8, may be NULL): every byte written; 1 where out took a value from a source, else 0.
 * Workspace.  sdi_interpolate_workspace_bytes(H, W) bytes, 4-byte aligned: one bit per pixel (the source bitmap,
 *   rows padded to a multiple of 64 bits).  Its contents on entry are arbitrary and unspecified on return.
 * Launch behaviour.  No allocation, no host synchronisation and no device-to-host read inside the call: two
 *   launches on `stream`, fixed by H and W.  No workgroup waits for another.
 *
 * SDE_ERR_ARG: a null disp, cls, out or workspace; out == disp (no overlap of any two arrays is allowed); H or
 * W < 1; H*W > 2^31 - 1 (pixel indices are 32-bit); a side other than the two; a workspace that is not 4-byte
 * aligned.  SDE_ERR_WORKSPACE: workspace_bytes below sdi_interpolate_workspace_bytes(H, W).  All checks return
 * before any launch.
 */
int sdi_interpolate(const float *disp, const uint8_t *cls, int H, int W, int side, float *out, uint8_t *filled,
                    void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDE_INTERP_H */
