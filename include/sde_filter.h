/*
 * sde_filter.h -- C ABI of the disparity-map filters behind the matching path (exported by the same libsde.so).
 *
 * The step between a disparity map and its depth map or point cloud that sde.h's post-processing does not have:
 * removal of small isolated disparity blobs ("speckles").  The 5x5 median removes only blobs smaller than half its
 * window, the left-right check only matches the two views disagree on, and the bilateral filter smooths such
 * blobs; none of them removes a cluster of wrong winners on a textureless or occluded patch.
 *
 * Conventions are sde.h's: device pointers owned by the caller, nothing allocates, frees or synchronises, every
 * call is stream-ordered and capturable into a hipGraph, `stream` is a hipStream_t passed as void*, the return
 * value is SDE_OK or a negative sde_status, and errors are detected before any launch (argument checks) or right
 * after it.  The functions are additive: SDE_ABI_VERSION stays 4.
 *
 * BUILD-DEFINED: the definition below is stated in full and restated in NumPy under tests/ (bit-exact against
 * that restatement: the result depends only on the partition of the image into regions, not on the order in which
 * a parallel algorithm finds it).  The model is OpenCV's filterSpeckles (4-connectivity, a difference threshold
 * between neighbours, regions of at most maxSpeckleSize pixels replaced), restated for float32 maps with
 * "invalid" meaning not finite or negative where OpenCV uses "equal to newVal"; parity with OpenCV itself is
 * unpinned (no OpenCV was available to compare against), as for sde_geom.h.
 */
#ifndef SDE_FILTER_H
#define SDE_FILTER_H

#include "sde.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device workspace bytes needed by sdf_speckle for an H x W map (0 for a shape sdf_speckle refuses). */
int64_t sdf_speckle_workspace_bytes(int H, int W);

/*
 * Speckle removal by connected-component labelling.  All arrays are [H][W], row-major.
 *
 * Valid pixels.  Pixel p is valid iff disp[p] is finite and disp[p] >= 0.0f.  -0.0f is valid; -1 ("no winner"),
 *   other negatives, NaN and +-inf are not.
 * Links.  Two 4-adjacent pixels p, q are linked iff both are valid and fabsf(disp[p] - disp[q]) <= max_diff.  The
 *   subtraction is one float32 operation rounded to nearest; it is symmetric in p and q.
 * Regions.  The regions are the connected components of the valid pixels under links (the transitive closure): a
 *   ramp whose neighbouring steps are each <= max_diff is one region however far its ends differ.  n(p) is the
 *   number of pixels of p's region.
 * Outputs.
 *   out[p]   = fill if p is valid and n(p) <= max_size, otherwise disp[p] bit for bit (NaN payloads and -0.0
 *              included).
 *   mask[p]  = 1 if p is valid and n(p) <= max_size, else 0.  Every byte is written.
 *   sizes[p] = n(p) if p is valid, else 0.  Every word is written.
 *   mask (uint8) and sizes (int32) may each be NULL.  out == disp is allowed; any other overlap of the arrays or
 *   the workspace is not.
 * Passes.  There is one pass: filled pixels do not take part again, whatever fill is.
 * max_size = 0 makes out a copy of disp and mask all 0, with sizes still correct.
 * Workspace.  sdf_speckle_workspace_bytes(H, W) bytes, 4-byte aligned.  Its contents on entry are arbitrary (the
 *   caller need not zero it) and unspecified on return.
 * Launch behaviour.  No allocation, no host synchronisation and no device-to-host read inside the call: it is a
 *   sequence of launches on `stream` fixed by H and W.  No workgroup waits for another in any of them.
 *
 * SDE_ERR_ARG: a null disp, out or workspace; H or W < 1; H*W > 2^31 - 1; max_size < 0; max_diff negative, NaN or
 * infinite; a workspace that is not 4-byte aligned.  fill may be any float.  SDE_ERR_WORKSPACE: workspace_bytes
 * below sdf_speckle_workspace_bytes(H, W).  All checks return before any launch.
 */
int sdf_speckle(const float *disp, int H, int W, int max_size, float max_diff, float fill, float *out,
                uint8_t *mask, int32_t *sizes, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDE_FILTER_H */
