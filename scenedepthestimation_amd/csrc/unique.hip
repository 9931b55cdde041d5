// unique.hip -- the uniqueness check (gfx950): sdu_wta_unique on a stored volume, and the exact fused form that
// sdu_cv_wta_unique (cv_wta.hip) launches in SDE_CV_EXACT mode, for C != 64 and for ranges wider than one row
// sweep.  Definition: include/sde_unique.h; the certified form is the row sweep's (cv_row.hip).
//
// Build-defined: WHDY/SceneDepthEstimation has no such stage (its guards are is_error_match / LRC,
// process_functional.py:977-1088); this is the absolute-margin counterpart of OpenCV's uniquenessRatio.
//
// Every kernel reads its costs once: the winner and the runner-up outside the winner's neighbourhood come from
// one scan, through the residue-class bookkeeping of unique.h (UqChain).
#include "cv_exact.h"
#include "unique.h"
#include "sde_unique.h"

namespace sde {

// sde_wta's winner from the +inf scan's (best, arg): SDE_WTA_INIT_D0 reads "no winner" as 0 and never replaces a
// NaN at d = 0 (wta.hip); c1 is the winner's cost
template <int RULE>
__device__ __forceinline__ void uq_rule(float &best, int &arg, float v0)
{
    if (RULE == SDE_WTA_INIT_D0 && (arg < 0 || v0 != v0)) {
        arg = 0;
        best = v0;
    }
}

__device__ __forceinline__ void uq_store_volume(int64_t p, int arg, float c1, float c2, float tau,
                                                float *__restrict__ margin, uint8_t *__restrict__ reject,
                                                float *__restrict__ disp)
{
    const bool has = arg >= 0;
    const float m = uq_margin(has, c1, c2);
    const bool rej = has && m < tau;
    if (margin) margin[p] = m;
    if (reject) reject[p] = rej ? 1 : 0;
    if (disp && rej) disp[p] = -1.0f;
}

// [D][H][W]: one lane per pixel, each d-slice read coalesced along W, once; chain u holds d = u (mod 4)
template <int RULE>
__global__ __launch_bounds__(256) void uq_dhw_kernel(const float *__restrict__ vol, int64_t npix, int D, float tau,
                                                     float *__restrict__ margin, uint8_t *__restrict__ reject,
                                                     float *__restrict__ disp)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    UqChain ch[4];
#pragma unroll
    for (int u = 0; u < 4; u++) ch[u].init();
    const float v0 = vol[p];
    for (int d = 0; d < D; d += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (d + u < D) ch[u].take(vol[(size_t)(d + u) * npix + p], d + u);
    }
    float best = ch[0].b1;
    int arg = ch[0].a1;
#pragma unroll
    for (int u = 1; u < 4; u++) argmin_merge(best, arg, ch[u].b1, ch[u].a1);
    uq_rule<RULE>(best, arg, v0);
    float c2 = ch[0].outside(arg);
#pragma unroll
    for (int u = 1; u < 4; u++) c2 = fminf(c2, ch[u].outside(arg));
    uq_store_volume(p, arg, best, c2, tau, margin, reject, disp);
}

// [H][W][D]: wta_hwd_kernel's mapping -- 16 lanes per pixel, lane `sub` scans d = sub, sub + 16, ... in increasing
// d (one chain: its disparities are 16 apart), the (value, index) butterfly gives all 16 lanes the winner, then a
// min butterfly over each lane's cost outside the winner's neighbourhood gives the runner-up
template <int RULE>
__global__ __launch_bounds__(256) void uq_hwd_kernel(const float *__restrict__ vol, int64_t npix, int D, float tau,
                                                     float *__restrict__ margin, uint8_t *__restrict__ reject,
                                                     float *__restrict__ disp)
{
    const int sub = threadIdx.x & 15;
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool ok = p < npix;
    const float *v = vol + (size_t)(ok ? p : 0) * D;
    UqChain ch;
    ch.init();
    if (ok) {
        for (int d = sub; d < D; d += 16) ch.take(v[d], d);
    }
    float best = ch.b1;
    int arg = ch.a1;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        argmin_merge(best, arg, ob, oa);
    }
    uq_rule<RULE>(best, arg, v[0]);
    float c2 = ch.outside(arg);
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) c2 = fminf(c2, __shfl_xor(c2, off, 64));
    if (ok && sub == 0) uq_store_volume(p, arg, best, c2, tau, margin, reject, disp);
}

// the fused forms' outputs: the winner's (min_cost, argmin), the decision, and the masked disparity
__device__ __forceinline__ void uq_store_fused(size_t p, int arg, float c1, float c2, float tau,
                                               float *__restrict__ out_min, int32_t *__restrict__ out_arg,
                                               float *__restrict__ out_disp, uint8_t *__restrict__ out_rej)
{
    const bool has = arg >= 0;
    const bool rej = has && uq_margin(has, c1, c2) < tau;
    if (out_min) out_min[p] = c1;
    if (out_arg) out_arg[p] = arg;
    if (out_disp) out_disp[p] = rej ? -1.0f : (float)arg;
    if (out_rej) out_rej[p] = rej ? 1 : 0;
}

// Exact fused form, C = 64: cv64_kernel<SIDE, OUT_WTA>'s mapping, staging and per-voxel arithmetic (dot64_exact:
// the same bits), with each wave's 16 disparities of a chunk in four chains (d - d0 = u mod 4; chunks and wave
// offsets are multiples of 4).  The four waves' winners merge as there; every wave then takes its chains' cost
// outside the merged winner's neighbourhood, and the minimum over the waves is the runner-up.
template <int SIDE>
__global__ __launch_bounds__(256) void cv64_unique_kernel(const float *__restrict__ own_feat,
                                                          const float *__restrict__ other_feat, int H, int W, int d0,
                                                          int d1, float tau, float *__restrict__ out_min,
                                                          int32_t *__restrict__ out_arg, float *__restrict__ out_disp,
                                                          uint8_t *__restrict__ out_rej)
{
    __shared__ float4 win[CV_ROWS * CV_RSTRIDE];
    __shared__ float sm[CV_WAVES][CV_TX];
    __shared__ int sa[CV_WAVES][CV_TX];
    __shared__ float s2[CV_WAVES][CV_TX];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int y = blockIdx.y;
    const int q0 = blockIdx.x * CV_TX;
    const int q = q0 + lane;
    const bool qok = q < W;

    float own[64];
    {
        const float4 *src = reinterpret_cast<const float4 *>(own_feat + ((size_t)y * W + (qok ? q : 0)) * 64);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const float4 v = src[k];
            own[4 * k + 0] = v.x; own[4 * k + 1] = v.y; own[4 * k + 2] = v.z; own[4 * k + 3] = v.w;
        }
    }
    const float4 *other4 = reinterpret_cast<const float4 *>(other_feat) + (size_t)y * W * 16;

    UqChain ch[4];
#pragma unroll
    for (int u = 0; u < 4; u++) ch[u].init();

    for (int dc = d0; dc < d1; dc += CV_DC) {
        const int dce = min(dc + CV_DC, d1);
        const int rbase = (SIDE == SDE_SIDE_LEFT) ? q0 - (dc + CV_DC - 1) : q0 + dc;
        __syncthreads();   // previous chunk's LDS reads are complete
        for (int idx = threadIdx.x; idx < CV_ROWS * 16; idx += 256) {
            const int lr = idx >> 4, k = idx & 15, g = rbase + lr;
            if (g >= 0 && g < W) win[lr * CV_RSTRIDE + k] = other4[(size_t)g * 16 + k];
        }
        __syncthreads();
        const int ds = dc + wave * CV_DW;
        for (int dd = ds; dd < min(ds + CV_DW, dce); dd += 4) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int d = dd + u;
                if (d < dce) {
                    const int o = (SIDE == SDE_SIDE_LEFT) ? q - d : q + d;
                    const bool valid = (SIDE == SDE_SIDE_LEFT) ? (o >= 0) : (o < W);
                    float cost = -0.0f;
                    if (qok && valid) cost = dot64_exact(own, win, o - rbase);
                    ch[u].take(cost, d);
                }
            }
        }
    }

    float best = ch[0].b1;
    int arg = ch[0].a1;
#pragma unroll
    for (int u = 1; u < 4; u++) argmin_merge(best, arg, ch[u].b1, ch[u].a1);
    sm[wave][lane] = best;
    sa[wave][lane] = arg;
    __syncthreads();
    best = sm[0][lane];
    arg = sa[0][lane];
#pragma unroll
    for (int w = 1; w < CV_WAVES; w++) argmin_merge(best, arg, sm[w][lane], sa[w][lane]);
    float c2 = ch[0].outside(arg);
#pragma unroll
    for (int u = 1; u < 4; u++) c2 = fminf(c2, ch[u].outside(arg));
    s2[wave][lane] = c2;
    __syncthreads();
    if (wave == 0 && qok) {
#pragma unroll
        for (int w = 1; w < CV_WAVES; w++) c2 = fminf(c2, s2[w][lane]);
        uq_store_fused((size_t)y * W + q, arg, best, c2, tau, out_min, out_arg, out_disp, out_rej);
    }
}

// Any channel count: one lane per pixel, cv_generic_kernel's costs (np_neg_dot), four chains
__global__ __launch_bounds__(256) void cv_generic_unique_kernel(const float *__restrict__ fl,
                                                                const float *__restrict__ fr, int H, int W, int C,
                                                                int d0, int d1, int right, float tau,
                                                                float *__restrict__ out_min,
                                                                int32_t *__restrict__ out_arg,
                                                                float *__restrict__ out_disp,
                                                                uint8_t *__restrict__ out_rej)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p % W);
    UqChain ch[4];
#pragma unroll
    for (int u = 0; u < 4; u++) ch[u].init();
    for (int dd = d0; dd < d1; dd += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int d = dd + u;
            if (d < d1) {
                float cost = -0.0f;
                if (right) {
                    if (x + d < W) cost = np_neg_dot(fl + ((size_t)y * W + x + d) * C, fr + ((size_t)y * W + x) * C, C);
                } else if (x >= d) {
                    cost = np_neg_dot(fl + ((size_t)y * W + x) * C, fr + ((size_t)y * W + x - d) * C, C);
                }
                ch[u].take(cost, d);
            }
        }
    }
    float best = ch[0].b1;
    int arg = ch[0].a1;
#pragma unroll
    for (int u = 1; u < 4; u++) argmin_merge(best, arg, ch[u].b1, ch[u].a1);
    float c2 = ch[0].outside(arg);
#pragma unroll
    for (int u = 1; u < 4; u++) c2 = fminf(c2, ch[u].outside(arg));
    uq_store_fused((size_t)p, arg, best, c2, tau, out_min, out_arg, out_disp, out_rej);
}

void launch_cv_unique_exact(bool right, const float *fl, const float *fr, int H, int W, int C, int d0, int d1,
                            float tau, float *disp, float *min_cost, int32_t *argmin, uint8_t *reject,
                            hipStream_t st)
{
    if (C == 64) {
        dim3 grid(cdiv(W, CV_TX), H);
        if (right)
            cv64_unique_kernel<SDE_SIDE_RIGHT><<<grid, 256, 0, st>>>(fr, fl, H, W, d0, d1, tau, min_cost, argmin, disp,
                                                                     reject);
        else
            cv64_unique_kernel<SDE_SIDE_LEFT><<<grid, 256, 0, st>>>(fl, fr, H, W, d0, d1, tau, min_cost, argmin, disp,
                                                                    reject);
    } else {
        cv_generic_unique_kernel<<<cdiv((int64_t)H * W, 256), 256, 0, st>>>(fl, fr, H, W, C, d0, d1, right ? 1 : 0,
                                                                             tau, min_cost, argmin, disp, reject);
    }
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int sdu_wta_unique(const float *vol, int H, int W, int D, int layout, int rule, float tau, float *margin,
                              uint8_t *reject, float *disp, void *stream)
{
    if (!vol || H <= 0 || W <= 0 || D <= 0 || (!margin && !reject && !disp)) return SDE_ERR_ARG;
    if (rule != SDE_WTA_INIT_INF && rule != SDE_WTA_INIT_D0) return SDE_ERR_ARG;
    if (!uq_tau_ok(tau)) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t npix = (int64_t)H * W;
    if (layout == SDE_LAYOUT_DHW) {
        const int blocks = cdiv(npix, 256);
        if (rule == SDE_WTA_INIT_INF)
            uq_dhw_kernel<SDE_WTA_INIT_INF><<<blocks, 256, 0, st>>>(vol, npix, D, tau, margin, reject, disp);
        else
            uq_dhw_kernel<SDE_WTA_INIT_D0><<<blocks, 256, 0, st>>>(vol, npix, D, tau, margin, reject, disp);
    } else if (layout == SDE_LAYOUT_HWD) {
        const int blocks = cdiv(npix * 16, 256);
        if (rule == SDE_WTA_INIT_INF)
            uq_hwd_kernel<SDE_WTA_INIT_INF><<<blocks, 256, 0, st>>>(vol, npix, D, tau, margin, reject, disp);
        else
            uq_hwd_kernel<SDE_WTA_INIT_D0><<<blocks, 256, 0, st>>>(vol, npix, D, tau, margin, reject, disp);
    } else {
        return SDE_ERR_ARG;
    }
    return launch_status();
}
