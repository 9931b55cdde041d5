// refine.hip -- sub-pixel disparities from the features and the 9x9 bilateral filter (gfx950): sde_cv_subpixel,
// sde_bilateral9.  (Sub-pixel WTA over a stored volume, sde_wta_subpixel, is wta.hip's.)
//
// Replaces (process_functional.py), both switched off in the reference:
//   the parabola step of WTA_and_SupixelRefinement_kernel :813-819 / :830-836 (subpixel.h), here on the exact
//                                                         costs recomputed around a given integer winner
//   Bilateral_Filter_kernel                               :882-974 (call commented out at :1260)
//
// Numerics are stated in include/sde.h down to the rounding.  The library is built with -ffp-contract=off, so
// every operation below is rounded on its own.
#include "subpixel.h"

namespace sde {

// The value sde_cost_volume(..., SDE_LAYOUT_DHW) holds at disparity d for the own pixel (row `own`, column x of
// its view): left view cost(x, d) with the other pixel at x - d, right view cost(x + d, d) with the other pixel at
// x + d; -0.0f where the other pixel is outside the row.  The products commute, so the operand order is free.
// np_neg_dot is NumPy's pairwise recursion for any C (for C = 64 it is cv_exact.h's dot64_exact_global).
template <int SIDE>
__device__ __forceinline__ float cv_value(const float *__restrict__ own, const float *__restrict__ other_row, int x,
                                          int d, int W, int C)
{
    const int o = (SIDE == SDE_SIDE_LEFT) ? x - d : x + d;
    if (o < 0 || o >= W) return -0.0f;
    return np_neg_dot(own, other_row + (size_t)o * C, C);
}

// The value a lane's own row would receive from the lane `N` below it in its row of 16 lanes (DPP row_shr:N, a
// full-rate VALU move); the lowest N lanes of a row keep `v`.
template <int N>
__device__ __forceinline__ float row_shr(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x110 + N, 0xf, 0xf, false));
}

// C = 64: 16 lanes per pixel (4 pixels per wave), lane `sub` holding channels 4 sub .. 4 sub + 3, so every load
// instruction reads whole 256-B feature rows.  cv_exact.h's order -- accumulator j of 8 summed over the channel
// blocks m = 0..7 in turn, then ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)) -- is kept across the lanes: block m sits in
// lanes 2m (accumulators 0..3) and 2m + 1 (4..7), the running sums walk up the row two lanes at a time, and lanes
// 14 / 15 end up with the eight accumulators.  The three costs around the winner share the walk.
template <int SIDE>
__global__ __launch_bounds__(256) void cv_subpixel64_kernel(const float *__restrict__ own_feat,
                                                            const float *__restrict__ other_feat, int H, int W,
                                                            int d0, int d1, const float *disp_in, float *disp_out)
{
    const int sub = threadIdx.x & 15;
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool ok = p < (int64_t)H * W;
    const float v = disp_in[ok ? p : 0];
    int i = 0;
    bool act = false;                                // uniform over the pixel's 16 lanes
    if (ok && v >= (float)d0 && v < (float)d1) {
        i = (int)v;
        act = (float)i == v && i > d0 && i < d1 - 1;
    }
    const int y = (int)((ok ? p : 0) / W), x = (int)((ok ? p : 0) % W);
    const float4 *own4 = reinterpret_cast<const float4 *>(own_feat) + (size_t)(ok ? p : 0) * 16;
    const float4 *row4 = reinterpret_cast<const float4 *>(other_feat) + (size_t)y * W * 16;
    // every lane loads (16-B loads, never split by a predicate): a pixel that is not refined, and a neighbour
    // outside the row, read the own column of the other view instead, and their products are not used
    const float4 a = own4[sub];
    float4 t[3];
    bool valid[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int d = i - 1 + k;
        const int o = (SIDE == SDE_SIDE_LEFT) ? x - d : x + d;
        valid[k] = act && o >= 0 && o < W;
        const float4 b = row4[(size_t)(valid[k] ? o : x) * 16 + sub];
        t[k] = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
    }
    // every lane of the wave takes part in the moves (a lane switched off would hand nothing on)
#pragma unroll
    for (int m = 1; m < 8; m++) {
        const bool mine = (sub >> 1) == m;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float rx = row_shr<2>(t[k].x), ry = row_shr<2>(t[k].y), rz = row_shr<2>(t[k].z),
                        rw = row_shr<2>(t[k].w);
            if (mine) t[k] = make_float4(rx + t[k].x, ry + t[k].y, rz + t[k].z, rw + t[k].w);
        }
    }
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float q = (t[k].x + t[k].y) + (t[k].z + t[k].w);     // lane 14: accumulators 0..3, lane 15: 4..7
        const float res = row_shr<1>(q) + q;
        c[k] = valid[k] ? -(0.0f + res) : -0.0f;
    }
    if (ok && sub == 15) {
        float r = v;
        if (v >= (float)d0 && v < (float)d1 && (float)(int)v == v) r = (float)(int)v;
        if (act) r = refine(i, d0, d1, c[0], c[1], c[2]);
        disp_out[p] = r;
    }
}

// Any channel count, one pixel per lane: a pixel whose input is an integer i in [d0, d1) recomputes the three
// exact costs around i (the neighbouring lanes' rows of the other view overlap and hit L2); any other input is
// copied through.
template <int SIDE>
__global__ __launch_bounds__(256) void cv_subpixel_kernel(const float *__restrict__ own_feat,
                                                          const float *__restrict__ other_feat, int H, int W, int C,
                                                          int d0, int d1, const float *disp_in, float *disp_out)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const float v = disp_in[p];
    float r = v;
    if (v >= (float)d0 && v < (float)d1) {          // false for NaN; d0, d1 < 2^24 are exact in float32
        const int i = (int)v;
        if ((float)i == v) {
            r = (float)i;
            if (i > d0 && i < d1 - 1) {
                const int y = (int)(p / W), x = (int)(p % W);
                const float *own = own_feat + (size_t)p * C;
                const float *row = other_feat + (size_t)y * W * C;
                const float cm = cv_value<SIDE>(own, row, x, i - 1, W, C);
                const float c0 = cv_value<SIDE>(own, row, x, i, W, C);
                const float cp = cv_value<SIDE>(own, row, x, i + 1, W, C);
                r = refine(i, d0, d1, cm, c0, cp);
            }
        }
    }
    disp_out[p] = r;
}

// Bilateral_Filter_kernel for one view: 16 x 16 outputs per workgroup, the 24 x 24 window of intensities and
// disparities in LDS with zeros outside the image (the reference's padded tile), 81 taps per thread in the
// reference's order with float64 running sums.  weights[5..9] (:925-929) are unreachable behind `< 5`.
constexpr int BF_T = 16;              // outputs per workgroup side
constexpr int BF_R = 4;               // window radius
constexpr int BF_S = BF_T + 2 * BF_R; // tile side
constexpr float BF_W0 = (float)0.167747, BF_W1 = (float)0.165145, BF_W2 = (float)0.157581, BF_W3 = (float)0.145735,
                BF_W4 = (float)0.130632;

__global__ __launch_bounds__(256) void bilateral9_kernel(const uint8_t *__restrict__ img, const float *__restrict__ src,
                                                         int H, int W, float *__restrict__ dst)
{
    __shared__ float sdisp[BF_S * BF_S];
    __shared__ uint8_t simg[BF_S * BF_S];
    const int x0 = blockIdx.x * BF_T - BF_R, y0 = blockIdx.y * BF_T - BF_R;
    for (int idx = threadIdx.x; idx < BF_S * BF_S; idx += 256) {
        const int gy = y0 + idx / BF_S, gx = x0 + idx % BF_S;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t g = in ? (size_t)gy * W + gx : 0;
        simg[idx] = in ? img[g] : (uint8_t)0;
        sdisp[idx] = in ? src[g] : 0.0f;
    }
    __syncthreads();
    const int tx = threadIdx.x & (BF_T - 1), ty = threadIdx.x >> 4;
    const int x = x0 + BF_R + tx, y = y0 + BF_R + ty;
    if (y >= H || x >= W) return;
    const int ci = simg[(ty + BF_R) * BF_S + tx + BF_R];
    double wsum = 0.0, dsum = 0.0;
#pragma unroll
    for (int i = 0; i < 2 * BF_R + 1; i++) {
#pragma unroll
        for (int j = 0; j < 2 * BF_R + 1; j++) {
            const int t = (ty + i) * BF_S + tx + j;
            const int m = ci - (int)simg[t];
            const int a = m >= 0 ? m : -m;
            if (a < 5) {
                const float w = a == 0 ? BF_W0 : a == 1 ? BF_W1 : a == 2 ? BF_W2 : a == 3 ? BF_W3 : BF_W4;
                wsum += (double)w;
                dsum += (double)(w * sdisp[t]);
            }
        }
    }
    dst[(size_t)y * W + x] = (float)(dsum / wsum);
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int sde_cv_subpixel(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, int side,
                               const float *disp_in, float *disp_out, void *stream)
{
    if (!fl || !fr || !disp_in || !disp_out || H <= 0 || W <= 0 || C <= 0 || d0 < 0 || d1 <= d0) return SDE_ERR_ARG;
    if (d1 > (1 << 24)) return SDE_ERR_ARG;         // the range test compares against float32(d0), float32(d1)
    if (side != SDE_SIDE_LEFT && side != SDE_SIDE_RIGHT) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    const int64_t npix = (int64_t)H * W;
    if (C == 64) {
        const int blocks = cdiv(npix * 16, 256);
        if (side == SDE_SIDE_LEFT)
            cv_subpixel64_kernel<SDE_SIDE_LEFT><<<blocks, 256, 0, st>>>(fl, fr, H, W, d0, d1, disp_in, disp_out);
        else
            cv_subpixel64_kernel<SDE_SIDE_RIGHT><<<blocks, 256, 0, st>>>(fr, fl, H, W, d0, d1, disp_in, disp_out);
    } else {
        const int blocks = cdiv(npix, 256);
        if (side == SDE_SIDE_LEFT)
            cv_subpixel_kernel<SDE_SIDE_LEFT><<<blocks, 256, 0, st>>>(fl, fr, H, W, C, d0, d1, disp_in, disp_out);
        else
            cv_subpixel_kernel<SDE_SIDE_RIGHT><<<blocks, 256, 0, st>>>(fr, fl, H, W, C, d0, d1, disp_in, disp_out);
    }
    return launch_status();
}

SDE_EXPORT int sde_bilateral9(const uint8_t *img_u8, const float *src, int H, int W, float *dst, void *stream)
{
    if (!img_u8 || !src || !dst || dst == src || H <= 0 || W <= 0) return SDE_ERR_ARG;
    if (H > BF_T * 65535) return SDE_ERR_ARG;       // grid.y
    dim3 grid(cdiv(W, BF_T), cdiv(H, BF_T));
    bilateral9_kernel<<<grid, 256, 0, as_stream(stream)>>>(img_u8, src, H, W, dst);
    return launch_status();
}
