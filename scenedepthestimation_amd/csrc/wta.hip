// wta.hip -- sde_wta, sde_wta_subpixel: winner-takes-all over a stored cost volume, as the integer winner or
// with the parabola step of subpixel.h applied to it (gfx950).  One kernel per layout; the two entry points are
// its SUBPIXEL = false / true instantiations.
//
// Replaces (WHDY/SceneDepthEstimation):
//   WTA1 / WTA                       process_functional.py:96-113 / 76-93
//   WTA_and_SupixelRefinement_kernel process_functional.py:800-837 (the parabola step switched off there)
#include "subpixel.h"

namespace sde {

// WTA over [D][H][W]: one lane per pixel, each d-slice read coalesced along W.  SUBPIXEL: the winner's two
// neighbours are re-read from the slices the scan has just pulled through the cache.
template <int RULE, bool SUBPIXEL>
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
    if constexpr (SUBPIXEL) {
        float r = (float)arg;
        if (arg > 0 && arg < D - 1) {
            const float cm = vol[(size_t)(arg - 1) * npix + p];
            const float c0 = vol[(size_t)arg * npix + p];
            const float cp = vol[(size_t)(arg + 1) * npix + p];
            r = refine(arg, 0, D, cm, c0, cp);
        }
        disp[p] = r;
    } else {
        disp[p] = (float)arg;
    }
}

// WTA over [H][W][D]: 16 lanes per pixel (4 pixels per wave), each lane scans a
// strided subset in increasing d, then a (value, index) butterfly across the 16
// lanes reproduces the sequential scan and leaves the winner in all of them.
// SUBPIXEL: lanes 0..2 of the pixel then load the costs at winner - 1, winner, winner + 1 in one instruction --
// the pixel's row is in the cache from the scan -- and lane 0 collects them across lanes.
template <int RULE, bool SUBPIXEL>
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
    // best = v[0], `best > v[d]` (:805-811): identical to the +inf scan except that
    // "no winner" reads 0 and a NaN at d = 0 is never replaced.  On the lane that stores; SUBPIXEL: on all 16
    // lanes, before the neighbour loads, which take the winner.
    if (RULE == SDE_WTA_INIT_D0 && (SUBPIXEL || (ok && sub == 0))) {
        const float v0 = v[0];
        if (arg < 0 || v0 != v0) arg = 0;
    }
    if constexpr (SUBPIXEL) {
        const bool inner = ok && arg > 0 && arg < D - 1;
        float c = 0.0f;
        if (inner && sub < 3) c = v[arg - 1 + sub];
        const int base = (threadIdx.x & 63) & ~15;   // the pixel's first lane in the wave
        const float cm = __shfl(c, base, 64);
        const float c0 = __shfl(c, base + 1, 64);
        const float cp = __shfl(c, base + 2, 64);
        if (ok && sub == 0) disp[p] = inner ? refine(arg, 0, D, cm, c0, cp) : (float)arg;
    } else if (ok && sub == 0) {
        disp[p] = (float)arg;
    }
}

template <bool SUBPIXEL>
static int launch_wta(const float *vol, int H, int W, int D, int layout, int rule, float *disp, void *stream)
{
    if (!vol || !disp || H <= 0 || W <= 0 || D <= 0) return SDE_ERR_ARG;
    if (rule != SDE_WTA_INIT_INF && rule != SDE_WTA_INIT_D0) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t npix = (int64_t)H * W;
    if (layout == SDE_LAYOUT_DHW) {
        const int blocks = cdiv(npix, 256);
        if (rule == SDE_WTA_INIT_INF) wta_dhw_kernel<SDE_WTA_INIT_INF, SUBPIXEL><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
        else wta_dhw_kernel<SDE_WTA_INIT_D0, SUBPIXEL><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
    } else if (layout == SDE_LAYOUT_HWD) {
        const int blocks = cdiv(npix * 16, 256);
        if (rule == SDE_WTA_INIT_INF) wta_hwd_kernel<SDE_WTA_INIT_INF, SUBPIXEL><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
        else wta_hwd_kernel<SDE_WTA_INIT_D0, SUBPIXEL><<<blocks, 256, 0, st>>>(vol, npix, D, disp);
    } else {
        return SDE_ERR_ARG;
    }
    return launch_status();
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int sde_wta(const float *vol, int H, int W, int D, int layout, int rule, float *disp, void *stream)
{
    return launch_wta<false>(vol, H, W, D, layout, rule, disp, stream);
}

SDE_EXPORT int sde_wta_subpixel(const float *vol, int H, int W, int D, int layout, int rule, float *disp, void *stream)
{
    return launch_wta<true>(vol, H, W, D, layout, rule, disp, stream);
}
