// cv_volume.hip -- sde_cost_volume: the disparity cost volume as a tensor (gfx950), [D,H,W] (CPU path, left
// only) or [H,W,D] (GPU path, L and/or R).  The kernels and their numerics are cv_exact.h's (any C, and C = 64
// per side) and cv_lr.h's (C = 64, both [H,W,D] volumes in one sweep).
#include "cv_lr.h"

using namespace sde;

SDE_EXPORT int sde_cost_volume(const float *fl, const float *fr, int H, int W, int C, int D, int layout,
                               int sides, float invalid, float *out_left, float *out_right, void *stream)
{
    if (!fl || !fr || H <= 0 || W <= 0 || C <= 0 || D <= 0) return SDE_ERR_ARG;
    if (layout != SDE_LAYOUT_DHW && layout != SDE_LAYOUT_HWD) return SDE_ERR_ARG;
    if ((sides & ~(SDE_SIDE_LEFT | SDE_SIDE_RIGHT)) || !sides) return SDE_ERR_ARG;
    if ((sides & SDE_SIDE_LEFT) && !out_left) return SDE_ERR_ARG;
    if ((sides & SDE_SIDE_RIGHT) && !out_right) return SDE_ERR_ARG;
    if (layout == SDE_LAYOUT_DHW && (sides & SDE_SIDE_RIGHT)) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    if (C == 64) {
        dim3 grid(cdiv(W, CV_TX), H);
        if (layout == SDE_LAYOUT_DHW) {
            cv64_kernel<SDE_SIDE_LEFT, OUT_DHW><<<grid, 256, 0, st>>>(fl, fr, H, W, 0, D, D, invalid, out_left,
                                                                       nullptr, nullptr, nullptr);
        } else if ((int64_t)W * D * 4 < (int64_t)BUF_OOB) {
            // one row sweep per (row, 64-disparity chunk) writes both volumes (the left one alone: the
            // same sweep without the right volume's stores).  (Rows of 2 GiB or more take the per-side
            // kernels below.)  A failed >64 KB dynamic-LDS opt-in surfaces as the failed launch:
            // SDE_ERR_LAUNCH from launch_status().
            const int nchunks = cdiv(D, CV_DC);
            const dim3 grid1((unsigned)(nchunks * H));
            if (sides == SDE_SIDE_LEFT)
                launch_lds<cvlr3_kernel<false>, C3_SMEM>(grid1, 256, st, fl, fr, H, W, D, nchunks, invalid, out_left,
                                                         nullptr);
            else if (sides == (SDE_SIDE_LEFT | SDE_SIDE_RIGHT))
                launch_lds<cvlr3_kernel<true>, C3_SMEM>(grid1, 256, st, fl, fr, H, W, D, nchunks, invalid, out_left,
                                                        out_right);
            else
                cv64_kernel<SDE_SIDE_RIGHT, OUT_HWD><<<grid, 256, 0, st>>>(fr, fl, H, W, 0, D, D, invalid,
                                                                            out_right, nullptr, nullptr, nullptr);
        } else {
            if (sides & SDE_SIDE_LEFT)
                cv64_kernel<SDE_SIDE_LEFT, OUT_HWD><<<grid, 256, 0, st>>>(fl, fr, H, W, 0, D, D, invalid,
                                                                           out_left, nullptr, nullptr, nullptr);
            if (sides & SDE_SIDE_RIGHT)
                cv64_kernel<SDE_SIDE_RIGHT, OUT_HWD><<<grid, 256, 0, st>>>(fr, fl, H, W, 0, D, D, invalid,
                                                                            out_right, nullptr, nullptr, nullptr);
        }
    } else {
        const int blocks = cdiv((int64_t)H * W, 256);
        if (layout == SDE_LAYOUT_DHW)
            cv_generic_kernel<OUT_DHW><<<blocks, 256, 0, st>>>(fl, fr, H, W, C, 0, D, D, sides, invalid, out_left,
                                                                nullptr, nullptr, nullptr, nullptr);
        else
            cv_generic_kernel<OUT_HWD><<<blocks, 256, 0, st>>>(fl, fr, H, W, C, 0, D, D, sides, invalid, out_left,
                                                                out_right, nullptr, nullptr, nullptr);
    }
    return launch_status();
}
