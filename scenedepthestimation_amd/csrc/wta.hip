// wta.hip -- sde_wta: winner-takes-all over a stored cost volume (gfx950).
//
// Replaces (WHDY/SceneDepthEstimation):
//   WTA1 / WTA                       process_functional.py:96-113 / 76-93
//   WTA_and_SupixelRefinement_kernel process_functional.py:800-837
#include "sde_common.h"

namespace sde {

// WTA over [D][H][W]: one lane per pixel, each d-slice read coalesced along W.
template <int RULE>
__global__ __launch_bounds__(256) void wta_dhw_kernel(const float *__restrict__ vol, int64_t npix, int D,
                                                      float *__restrict__ disp)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    float best;
    int arg;
    if (RULE == SDE_WTA_INIT_D0) { best = vol[p]; arg = 0; }
    else { best = __builtin_inff(); arg = -1; }
    for (int d = (RULE == SDE_WTA_INIT_D0 ? 1 : 0); d < D; d++) {
        const float v = vol[(size_t)d * npix + p];
        if (v < best) { best = v; arg = d; }
    }
    disp[p] = (float)arg;
}

// WTA over [H][W][D]: 16 lanes per pixel (4 pixels per wave), each lane scans a
// strided subset in increasing d, then a (value, index) merge across the 16
// lanes reproduces the sequential scan.
template <int RULE>
__global__ __launch_bounds__(256) void wta_hwd_kernel(const float *__restrict__ vol, int64_t npix, int D,
                                                      float *__restrict__ disp)
{
    const int sub = threadIdx.x & 15;
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool ok = p < npix;
    const float *v = vol + (size_t)(ok ? p : 0) * D;
    float best = __builtin_inff();
    int arg = -1;
    if (ok) {
        for (int d = sub; d < D; d += 16) {
            const float x = v[d];
            if (x < best) { best = x; arg = d; }
        }
    }
    // A lane with arg = -1 holds +inf; a lane with a winner holds a value < +inf,
    // so the plain (value, index) merge never lets -1 win against a real index.
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        argmin_merge(best, arg, ob, oa);
    }
    if (ok && sub == 0) {
        if (RULE == SDE_WTA_INIT_D0) {
            // best = v[0], `best > v[d]` (:805-811): identical to the +inf scan except that
            // "no winner" reads 0 and a NaN at d = 0 is never replaced.
            const float v0 = v[0];
            if (arg < 0 || v0 != v0) arg = 0;
        }
        disp[p] = (float)arg;
    }
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int sde_wta(const float *vol, int H, int W, int D, int layout, int rule, float *disp, void *stream)
{
    if (!vol || !disp || H <= 0 || W <= 0 || D <= 0) return SDE_ERR_ARG;
    if (rule != SDE_WTA_INIT_INF && rule != SDE_WTA_INIT_D0) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t npix = (int64_t)H * W;
    if (layout == SDE_LAYOUT_DHW) {
        const int blocks = cdiv(npix, 256);
        if (rule == SDE_WTA_INIT_INF) wta_dhw_kernel<SDE_WTA_INIT_INF><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
        else wta_dhw_kernel<SDE_WTA_INIT_D0><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
    } else if (layout == SDE_LAYOUT_HWD) {
        const int blocks = cdiv(npix * 16, 256);
        if (rule == SDE_WTA_INIT_INF) wta_hwd_kernel<SDE_WTA_INIT_INF><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
        else wta_hwd_kernel<SDE_WTA_INIT_D0><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
    } else {
        return SDE_ERR_ARG;
    }
    return launch_status();
}
