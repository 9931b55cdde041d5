/*
 * sde_unique.h -- C ABI of the uniqueness check behind the matching path (exported by the same libsde.so).
 *
 * The third standard guard against wrong winners, beside the left-right check (sde.h) and speckle removal
 * (sde_filter.h): a pixel whose best cost is barely better than the best cost outside the winner's immediate
 * neighbourhood is dropped.  It catches textureless and repetitive patches.  It is not a filter on the disparity
 * map: it needs the second-best cost, so it runs on a stored volume or inside the fused cost volume + WTA.
 *
 * Conventions are sde.h's: device pointers owned by the caller, nothing allocates, frees or synchronises, every
 * call is stream-ordered and capturable into a hipGraph, `stream` is a hipStream_t passed as void*, the return
 * value is SDE_OK or a negative sde_status, and errors are detected before any launch (argument checks) or right
 * after it.  The functions are additive: SDE_ABI_VERSION stays 4, and sde.h stays as it is.
 *
 * BUILD-DEFINED: WHDY/SceneDepthEstimation has no such stage.  The model is OpenCV's uniquenessRatio (block and
 * semi-global matchers), restated as an ABSOLUTE margin: MC-CNN costs are negated dot products, they are negative,
 * and a percentage of the best cost has no meaning there.  The definition is stated in full below and restated in
 * NumPy under tests/ (bit-exact against that restatement).
 *
 * Definition (one, by bytes, for every entry below).  Take a pixel's costs c[d] over the scanned range [d0, d1) --
 * exactly the voxels its winner scan reads, fills (-0.0 / 1.0 / SDE_LOCAL_INVALID) included -- and the winner i
 * that scan returns under its own rule; c1 = c[i].
 *   runner-up:  c2 = +inf; for d ascending with |d - i| >= 2: if (c[d] < c2) c2 = c[d]      (NaN never wins;
 *               c2 stays +inf if there is no such d)
 *   margin:     m = (c2 == c1) ? +0.0f : c2 - c1                 one float32 subtraction, nothing fused; a NaN
 *               result (only when c1 is NaN: SDE_WTA_INIT_D0 with a NaN at d = 0) is the quiet NaN 0x7fc00000
 *   rejection:  reject = (m < tau)                               IEEE: false for a NaN margin
 * A rejected pixel's disparity becomes -1.0f.  A pixel without a winner stays -1 with reject = 0, m = +0.0f.
 * tau: a finite float32 >= 0 (anything else: SDE_ERR_ARG); with tau = 0 nothing is rejected and the outputs are
 * the plain entry point's, byte for byte.
 */
#ifndef SDE_UNIQUE_H
#define SDE_UNIQUE_H

#include "sde.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The check on a stored volume (sde_wta's layouts and rules; i is sde_wta's winner).  margin (float32 [H][W]) and
 * reject (uint8 [H][W], 0 / 1) are optional outputs, every pixel written.  disp is optional and IN / OUT: a
 * rejected pixel is set to -1.0f, every other pixel is left untouched, so one launch masks a map that
 * sde_wta_subpixel has refined.  At least one of the three must be given; the other argument checks are sde_wta's.
 * The volume is read once.
 */
int sdu_wta_unique(const float *vol, int H, int W, int D, int layout, int rule, float tau, float *margin,
                   uint8_t *reject, float *disp, void *stream);

/*
 * The fused form for either view (side = SDE_SIDE_LEFT: sde_cv_wta, SDE_SIDE_RIGHT: sde_cv_wta_right): their
 * arguments, outputs, modes, workspace (sde_cv_wta_workspace_bytes) and counter words, with the check applied:
 * disp is -1.0f where rejected; min_cost and argmin stay the winner's; reject (uint8 [H][W], optional) is the
 * decision.  At least one of the four outputs must be given.  SDE_CV_EXACT and SDE_CV_CERTIFIED give identical
 * bytes: the certified row sweep decides a pixel itself only when its winner is certified and its fast margin is
 * further from tau than the error bound; every other pixel is resolved by the exact scan and counted.  A range
 * wider than one row sweep (e.g. D = 512) runs the exact form in either mode, the counters zeroed.  There is no
 * margin output: the certified mode certifies the decision, not the runner-up's value.
 */
int sdu_cv_wta_unique(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, int side, float tau,
                      float *disp, float *min_cost, int32_t *argmin, uint8_t *reject, int mode, void *workspace,
                      int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDE_UNIQUE_H */
