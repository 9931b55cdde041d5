// cv_exact.h -- the exact cost-volume arithmetic and the kernels both cv_volume.hip (sde_cost_volume) and
// cv_wta.hip (sde_cv_wta*) launch.
//
// Replaces (WHDY/SceneDepthEstimation):
//   compute_cost_volume        process_functional.py:48-73   (CPU path, [D,H,W], -0.0 fill)
//   compute_cost_volume_kernel process_functional.py:120-131 ([H,W,D] L and R, 1.0 fill)
//
// Numerics: every valid voxel is the CPU path's value bit for bit,
//   cost(x,d) = -(0.0f + pairwise8_c(fl[y][x][c] * fr[y][x-d][c]))
// -- products rounded to f32, 8 running f32 accumulators over channel blocks of
// 8, then ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)) (NumPy's pairwise_sum for C=64).
// The library is compiled with -ffp-contract=off so no product is fused.
//
// Mapping (C = 64 fast path): a workgroup is 4 waves on one image row and 64
// consecutive "own" pixels (one per lane, its 64-float feature vector held in
// VGPRs).  The 127 "other" feature rows a 64-disparity chunk touches are staged
// in LDS (272-B padded rows: the 16 lanes of a ds_read_b128 group read 16
// consecutive rows -> 16 distinct bank slots).  Wave w sweeps disparities
// [16w, 16w+16) of each chunk; the fused WTA merges the 4 per-wave first-minima
// by (value, index) at the end, which equals the sequential scan.
#pragma once

#include "sde_common.h"

namespace sde {

constexpr int CV_TX = 64;                    // own pixels per workgroup (= lanes)
constexpr int CV_WAVES = 4;                  // waves per workgroup
constexpr int CV_DC = 64;                    // disparities per LDS chunk
constexpr int CV_DW = CV_DC / CV_WAVES;      // disparities per wave per chunk
constexpr int CV_ROWS = CV_TX + CV_DC - 1;   // other-side rows per chunk

enum { OUT_WTA = 0, OUT_DHW = 1, OUT_HWD = 2 };

// LDS image of the "other" rows: 64 floats + one 16-B pad per row (272 B), so the lanes of a
// ds_read_b128 group, which read the same chunk of consecutive rows, start 4 banks apart
// (conflict-free) and every chunk address is the row base plus an immediate offset.
constexpr int CV_RSTRIDE = 17;     // float4 per LDS row

// The exact cost (Numerics, above) of own[64] (registers) and one padded LDS row.
__device__ __forceinline__ float dot64_exact(const float (&own)[64], const float4 *__restrict__ win, int lr)
{
    float acc[8];
    const float4 *row = win + lr * CV_RSTRIDE;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const float4 a = row[2 * m];
        const float4 b = row[2 * m + 1];
        const float p0 = own[8 * m + 0] * a.x, p1 = own[8 * m + 1] * a.y;
        const float p2 = own[8 * m + 2] * a.z, p3 = own[8 * m + 3] * a.w;
        const float p4 = own[8 * m + 4] * b.x, p5 = own[8 * m + 5] * b.y;
        const float p6 = own[8 * m + 6] * b.z, p7 = own[8 * m + 7] * b.w;
        if (m == 0) {
            acc[0] = p0; acc[1] = p1; acc[2] = p2; acc[3] = p3;
            acc[4] = p4; acc[5] = p5; acc[6] = p6; acc[7] = p7;
        } else {
            acc[0] += p0; acc[1] += p1; acc[2] += p2; acc[3] += p3;
            acc[4] += p4; acc[5] += p5; acc[6] += p6; acc[7] += p7;
        }
    }
    const float res = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    return -(0.0f + res);
}

// The same cost of two 64-float rows in global memory (16-B loads).
__device__ __forceinline__ float dot64_exact_global(const float4 *__restrict__ a, const float4 *__restrict__ b)
{
    float acc[8];
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const float4 a0 = a[2 * m], a1 = a[2 * m + 1], b0 = b[2 * m], b1 = b[2 * m + 1];
        const float p[8] = {a0.x * b0.x, a0.y * b0.y, a0.z * b0.z, a0.w * b0.w,
                            a1.x * b1.x, a1.y * b1.y, a1.z * b1.z, a1.w * b1.w};
#pragma unroll
        for (int jj = 0; jj < 8; jj++) acc[jj] = (m == 0) ? p[jj] : acc[jj] + p[jj];
    }
    const float res = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    return -(0.0f + res);
}

// SIDE_LEFT : own = fl at x,  other = fr at x - d   (L[y][x][d])
// SIDE_RIGHT: own = fr at x', other = fl at x' + d  (R[y][x'][d] = cost(x'+d, d))
template <int SIDE, int OUT>
__global__ __launch_bounds__(256) void cv64_kernel(const float *__restrict__ own_feat,
                                                   const float *__restrict__ other_feat, int H, int W,
                                                   int d0, int d1, int Dvol, float invalid,
                                                   float *__restrict__ out, float *__restrict__ out_min,
                                                   int32_t *__restrict__ out_arg, float *__restrict__ out_disp)
{
    constexpr bool TILE = OUT == OUT_HWD;
    __shared__ float4 win[CV_ROWS * CV_RSTRIDE];
    __shared__ float otile[TILE ? CV_TX * (CV_DC + 1) : 1];

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

    float best = __builtin_inff();
    int arg = -1;

    for (int dc = d0; dc < d1; dc += CV_DC) {
        const int dce = min(dc + CV_DC, d1);
        const int rbase = (SIDE == SDE_SIDE_LEFT) ? q0 - (dc + CV_DC - 1) : q0 + dc;
        __syncthreads();   // previous chunk's LDS reads (win and otile) are complete
        for (int idx = threadIdx.x; idx < CV_ROWS * 16; idx += 256) {
            const int lr = idx >> 4, k = idx & 15, g = rbase + lr;
            if (g >= 0 && g < W) win[lr * CV_RSTRIDE + k] = other4[(size_t)g * 16 + k];
        }
        __syncthreads();
        const int ds = dc + wave * CV_DW;
        const int de = min(ds + CV_DW, dce);
#pragma unroll 2
        for (int d = ds; d < de; d++) {
            const int o = (SIDE == SDE_SIDE_LEFT) ? q - d : q + d;
            const bool valid = (SIDE == SDE_SIDE_LEFT) ? (o >= 0) : (o < W);
            float cost = invalid;
            if (qok && valid) cost = dot64_exact(own, win, o - rbase);
            if (OUT == OUT_WTA) {
                if (cost < best) { best = cost; arg = d; }
            } else if (OUT == OUT_DHW) {
                if (qok) out[((size_t)d * H + y) * W + q] = cost;
            } else {
                otile[lane * (CV_DC + 1) + (d - dc)] = cost;
            }
        }
        if (TILE) {
            __syncthreads();
            const int nd = dce - dc;
            for (int i = wave; i < CV_TX; i += CV_WAVES) {
                if (q0 + i < W && lane < nd)
                    out[((size_t)y * W + q0 + i) * Dvol + dc + lane] = otile[i * (CV_DC + 1) + lane];
            }
        }
    }

    if (OUT == OUT_WTA) {
        __shared__ float sm[CV_WAVES][CV_TX];
        __shared__ int sa[CV_WAVES][CV_TX];
        sm[wave][lane] = best;
        sa[wave][lane] = arg;
        __syncthreads();
        if (wave == 0 && qok) {
#pragma unroll
            for (int w = 1; w < CV_WAVES; w++) argmin_merge(best, arg, sm[w][lane], sa[w][lane]);
            const size_t p = (size_t)y * W + q;
            if (out_min) out_min[p] = best;
            if (out_arg) out_arg[p] = arg;
            if (out_disp) out_disp[p] = (float)arg;
        }
    }
}

// Any channel count: one lane per (pixel, d-range), features read from global
// memory, NumPy's full pairwise recursion.  Correctness path for C != 64.
template <int OUT>
__global__ __launch_bounds__(256) void cv_generic_kernel(const float *__restrict__ fl, const float *__restrict__ fr,
                                                         int H, int W, int C, int d0, int d1, int Dvol,
                                                         int sides, float invalid, float *__restrict__ outl,
                                                         float *__restrict__ outr, float *__restrict__ out_min,
                                                         int32_t *__restrict__ out_arg, float *__restrict__ out_disp)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p % W);
    float best = __builtin_inff();
    int arg = -1;
    for (int d = d0; d < d1; d++) {
        float cost = invalid;
        if (OUT == OUT_WTA && sides == SDE_SIDE_RIGHT) {
            // the right view's scan: cost(x + d, d) for right pixel x
            if (x + d < W) cost = np_neg_dot(fl + ((size_t)y * W + x + d) * C, fr + ((size_t)y * W + x) * C, C);
        } else if (x >= d) {
            cost = np_neg_dot(fl + ((size_t)y * W + x) * C, fr + ((size_t)y * W + x - d) * C, C);
        }
        if (OUT == OUT_WTA) {
            if (cost < best) { best = cost; arg = d; }
        } else if (OUT == OUT_DHW) {
            outl[((size_t)d * H + y) * W + x] = cost;
        } else {
            if (sides & SDE_SIDE_LEFT) outl[((size_t)y * W + x) * Dvol + d] = cost;
        }
        // right volume: R[y][x][d] = cost(x + d, d), computed by its own owner pixel x
        if (OUT == OUT_HWD && (sides & SDE_SIDE_RIGHT)) {
            float cr = invalid;
            if (x + d < W) cr = np_neg_dot(fl + ((size_t)y * W + x + d) * C, fr + ((size_t)y * W + x) * C, C);
            outr[((size_t)y * W + x) * Dvol + d] = cr;
        }
    }
    if (OUT == OUT_WTA) {
        if (out_min) out_min[p] = best;
        if (out_arg) out_arg[p] = arg;
        if (out_disp) out_disp[p] = (float)arg;
    }
}

}  // namespace sde
