// interp.hip -- interpolation of left-right-flagged pixels (gfx950): sdi_classify, sdi_interpolate.
//
// The definition is stated in include/sde_interp.h.  Every output is a copy of an input value (or that value
// + 0.0f), so any order of evaluation gives the same bytes.  Three kernels:
//
//   interp_classify_kernel  one workgroup per 256 columns of a row, by coverage: each other-view pixel that can
//                           reach the segment marks, in LDS, the few columns its value makes consistent; then one
//                           thread per pixel reads and writes its own byte of the flag map, so cls may alias lrc.
//                           Cost per row: W (1 + (D - 1) / 256) other-view loads (every segment reads the D - 1
//                           pixels beside it, whether or not it holds a flagged pixel) and W (2 max_diff + 3)
//                           compares, against the W D loads of a scan per pixel.
//   interp_bitmap_kernel    one wave per 64 pixels of a row: cls and validity folded into one source bit per pixel
//                           (a wave ballot), two 32-bit words per wave.  Rows are padded to whole 64-bit chunks and
//                           the padding bits are 0, so a scan never needs a column test.
//   interp_fill_kernel      one thread per pixel.  The horizontal searches (every occlusion pixel, the rays (2, 0)
//                           and (-2, 0)) scan the bitmap a word at a time: 32 pixels per load, clz / ctz inside
//                           the word.  The other 14 rays test one bit per step and read disp only at the source.
//                           The median is a rank selection over the 16 ray slots held in registers (a ray without
//                           a source holds 0xffffffff, above every value), no sort and no scratch.
//
// Values are non-negative finite floats, so their order is the order of their bit patterns as unsigned integers.
#include "sde_common.h"
#include "sde_interp.h"

namespace sde {

constexpr uint32_t RAY_NONE = 0xffffffffu;

__device__ __forceinline__ bool interp_valid(float v) { return finite_f32(v) && v >= 0.0f; }   // -0.0f >= 0

__device__ __forceinline__ int interp_cls(uint8_t c) { return c == 1 || c == 2 ? c : 0; }

// One workgroup per 256 columns [c0, c1) of a row, by coverage: the predicate "some dh makes (y, x) consistent"
// depends on (y, x) alone, and other-view pixel xo with a valid value v makes exactly the columns xo + dh (left
// view; xo - dh for the right view) consistent, for the integers dh in [0, D - 1] that pass the definition's own
// float64 compare against v: those lie in [v - max_diff, v + max_diff], and the window scanned is one wider on each
// side than that interval's rounded ends, so no rounding of the ends can lose one.  The threads walk the other-view
// pixels that can reach the segment, xo in [c0 - (D - 1), c1 - 1] (left) or [c0, c1 - 1 + (D - 1)] (right), and set
// a flag per covered column in LDS (every writer stores 1: no atomics); after the barrier a thread reads and
// writes only its own byte of the flag map, so cls may alias lrc (no __restrict__ on either).
__global__ __launch_bounds__(256) void interp_classify_kernel(const float *__restrict__ other, const uint8_t *lrc,
                                                              int H, int W, int D, int right, double max_diff,
                                                              int nseg, uint8_t *cls)
{
    __shared__ uint32_t covered[256];
    const int t = threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)nseg), c0 = (int)(blockIdx.x % (unsigned)nseg) * 256;
    const int c1 = W - c0 > 256 ? c0 + 256 : W;   // c0 <= W - 1; c0 + 256 alone may pass 2^31 - 1
    const float *row = other + (size_t)y * W;
    covered[t] = 0;
    __syncthreads();
    // 64-bit: c1 - 1 + (D - 1) may pass 2^31
    const int64_t reach_lo = right ? c0 : (int64_t)c0 - (D - 1), reach_hi = right ? (int64_t)c1 - 1 + (D - 1) : c1 - 1;
    const int xlo = reach_lo < 0 ? 0 : (int)reach_lo, xhi = reach_hi > W - 1 ? W - 1 : (int)reach_hi;
    for (int64_t xo64 = (int64_t)xlo + t; xo64 <= xhi; xo64 += 256) {   // 64-bit: xhi + 256 may pass 2^31 - 1
        const int xo = (int)xo64;
        const float v = row[xo];
        if (!interp_valid(v)) continue;
        const double a = (double)v - max_diff, b = (double)v + max_diff;   // b >= 0
        if (a > (double)D) continue;
        int lo = a <= 1.0 ? 0 : (int)a - 1;
        int hi = b >= (double)(D - 2) ? D - 1 : (int)b + 1;
        // only the dh that land in [c0, c1): at most 256 steps whatever D and max_diff are, and xo +- dh stays in int
        const int near = right ? xo - (c1 - 1) : c0 - xo, far = right ? xo - c0 : c1 - 1 - xo;
        lo = lo > near ? lo : near;
        hi = hi < far ? hi : far;
        for (int dh = lo; dh <= hi; dh++) {
            const double mn = (double)dh - (double)v;
            if (!(mn > max_diff || mn < -max_diff)) covered[(right ? xo - dh : xo + dh) - c0] = 1;
        }
    }
    __syncthreads();
    if (t < c1 - c0) {
        const size_t p = (size_t)y * W + c0 + t;
        cls[p] = lrc[p] == 1 ? (covered[t] ? 2 : 1) : 0;
    }
}

// wpr: 32-bit words per bitmap row, 2 * ceil(W / 64).
__global__ __launch_bounds__(256) void interp_bitmap_kernel(const float *__restrict__ disp,
                                                            const uint8_t *__restrict__ cls, int H, int W, int nchunk,
                                                            uint32_t *__restrict__ bm)
{
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= (int64_t)H * nchunk) return;   // wave-uniform
    const int y = (int)(wave / nchunk), cx = (int)(wave % nchunk);
    const int64_t x = (int64_t)cx * 64 + lane;   // the last chunk's padding columns may pass 2^31 - 1
    bool src = false;
    if (x < W) {
        const size_t p = (size_t)y * W + x;
        src = interp_cls(cls[p]) == 0 && interp_valid(disp[p]);
    }
    const uint64_t m = __ballot(src);
    if (lane == 0) {
        uint32_t *w = bm + ((size_t)y * nchunk + cx) * 2;
        w[0] = (uint32_t)m;
        w[1] = (uint32_t)(m >> 32);
    }
}

// nearest source column of a bitmap row strictly left / right of x, -1 if there is none
__device__ __forceinline__ int interp_left_of(const uint32_t *__restrict__ row, int x)
{
    int w = x >> 5;
    uint32_t m = row[w] & ((1u << (x & 31)) - 1u);
    while (m == 0 && --w >= 0) m = row[w];
    return m ? w * 32 + 31 - __clz((int)m) : -1;
}

__device__ __forceinline__ int interp_right_of(const uint32_t *__restrict__ row, int x, int wpr)
{
    int w = x >> 5;
    uint32_t m = row[w] & ~((2u << (x & 31)) - 1u);   // x & 31 == 31: 2u << 31 wraps to 0, the mask to 0
    while (m == 0 && ++w < wpr) m = row[w];
    return m ? w * 32 + __ffs((int)m) - 1 : -1;       // padding bits are 0: the column is inside the row
}

__device__ __forceinline__ uint32_t interp_value(const float *__restrict__ disp, size_t q)
{
    return __float_as_uint(disp[q] + 0.0f);   // -0.0 -> +0.0
}

// Ray (A, B): step i is (x + o(A, i), y + o(B, i)); o(+-2, i) = +-i, o(+-1, i) = +-ceil(i / 2) (it moves on odd i),
// o(0, i) = 0.  The coordinate with |.| == 2 moves on every step, so the ray leaves the image and the loop ends.
template <int A, int B>
__device__ __forceinline__ uint32_t interp_ray(const uint32_t *__restrict__ bm, const float *__restrict__ disp, int x,
                                               int y, int H, int W, int wpr)
{
    constexpr int sx = A > 0 ? 1 : (A < 0 ? -1 : 0), sy = B > 0 ? 1 : (B < 0 ? -1 : 0);
    constexpr bool halfx = A == 1 || A == -1, halfy = B == 1 || B == -1;
    if constexpr (B == 0) {
        const uint32_t *row = bm + (size_t)y * wpr;
        const int q = A > 0 ? interp_right_of(row, x, wpr) : interp_left_of(row, x);
        return q < 0 ? RAY_NONE : interp_value(disp, (size_t)y * W + q);
    } else {
        // One step per round.  Loading four steps' words per round, so that a test need not wait for the
        // previous step's load, was measured and not kept: it was slower both on realistic flags and on the
        // single-source map ("Measured": most walks end within a step or two).
        for (int i = 1;; i++) {
            if (!halfx || (i & 1)) x += sx;
            if (!halfy || (i & 1)) y += sy;
            if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return RAY_NONE;
            if ((bm[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u) return interp_value(disp, (size_t)y * W + x);
        }
    }
}

__global__ __launch_bounds__(256) void interp_fill_kernel(const float *__restrict__ disp,
                                                          const uint8_t *__restrict__ cls, int H, int W, int right,
                                                          int wpr, const uint32_t *__restrict__ bm,
                                                          float *__restrict__ out, uint8_t *__restrict__ filled)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int c = interp_cls(cls[p]);
    uint32_t r = RAY_NONE;
    if (c != 0) {
        const int y = (int)(p / W), x = (int)(p % W);
        if (c == 1) {
            const uint32_t *row = bm + (size_t)y * wpr;
            int q = right ? interp_right_of(row, x, wpr) : interp_left_of(row, x);
            if (q < 0) q = right ? interp_left_of(row, x) : interp_right_of(row, x, wpr);
            if (q >= 0) r = interp_value(disp, (size_t)y * W + q);
        } else {
            uint32_t v[16];
#define SDE_RAY(k, a, b) v[k] = interp_ray<a, b>(bm, disp, x, y, H, W, wpr)
            SDE_RAY(0, 2, 0);    SDE_RAY(1, 2, 1);    SDE_RAY(2, 2, 2);    SDE_RAY(3, 1, 2);
            SDE_RAY(4, 0, 2);    SDE_RAY(5, -1, 2);   SDE_RAY(6, -2, 2);   SDE_RAY(7, -2, 1);
            SDE_RAY(8, -2, 0);   SDE_RAY(9, -2, -1);  SDE_RAY(10, -2, -2); SDE_RAY(11, -1, -2);
            SDE_RAY(12, 0, -2);  SDE_RAY(13, 1, -2);  SDE_RAY(14, 2, -2);  SDE_RAY(15, 2, -1);
#undef SDE_RAY
            int n = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) n += v[k] != RAY_NONE;
            // element n / 2 of the n values sorted ascending = element n / 2 of all 16 slots (empty slots sort last):
            // the slot with exactly n / 2 slots before it, ties ordered by slot number
            const int want = n >> 1;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                int rank = 0;
#pragma unroll
                for (int j = 0; j < 16; j++) rank += v[j] < v[k] || (v[j] == v[k] && j < k);
                if (n > 0 && rank == want) r = v[k];
            }
        }
    }
    const bool took = r != RAY_NONE;
    out[p] = took ? __uint_as_float(r) : disp[p];
    if (filled) filled[p] = took ? 1 : 0;
}

static inline bool interp_bad_shape(int H, int W) { return H < 1 || W < 1 || (int64_t)H * W > 2147483647ll; }
static inline bool interp_bad_side(int side) { return side != SDE_SIDE_LEFT && side != SDE_SIDE_RIGHT; }

}  // namespace sde

using namespace sde;

SDE_EXPORT int sdi_classify(const float *disp_other, const uint8_t *lrc, int H, int W, int D, int side,
                            float max_diff, uint8_t *cls, void *stream)
{
    if (!disp_other || !lrc || !cls || interp_bad_shape(H, W) || D < 1 || interp_bad_side(side)) return SDE_ERR_ARG;
    if (!(max_diff >= 0.0f) || max_diff > 3.402823466e38f) return SDE_ERR_ARG;   // negative, NaN, infinite
    const int nseg = cdiv(W, 256);
    interp_classify_kernel<<<(unsigned)((int64_t)H * nseg), 256, 0, as_stream(stream)>>>(
        disp_other, lrc, H, W, D, side == SDE_SIDE_RIGHT, (double)max_diff, nseg, cls);
    return launch_status();
}

SDE_EXPORT int64_t sdi_interpolate_workspace_bytes(int H, int W)
{
    if (interp_bad_shape(H, W)) return 0;
    return (int64_t)H * cdiv(W, 64) * 8;   // one bit per pixel, rows padded to whole 64-bit chunks
}

SDE_EXPORT int sdi_interpolate(const float *disp, const uint8_t *cls, int H, int W, int side, float *out,
                               uint8_t *filled, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!disp || !cls || !out || !workspace || out == disp || interp_bad_shape(H, W) || interp_bad_side(side))
        return SDE_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return SDE_ERR_ARG;
    if (workspace_bytes < sdi_interpolate_workspace_bytes(H, W)) return SDE_ERR_WORKSPACE;
    uint32_t *bm = static_cast<uint32_t *>(workspace);
    hipStream_t st = as_stream(stream);
    const int nchunk = cdiv(W, 64);
    interp_bitmap_kernel<<<cdiv((int64_t)H * nchunk, 4), 256, 0, st>>>(disp, cls, H, W, nchunk, bm);
    interp_fill_kernel<<<cdiv((int64_t)H * W, 256), 256, 0, st>>>(disp, cls, H, W, side == SDE_SIDE_RIGHT,
                                                                  2 * nchunk, bm, out, filled);
    return launch_status();
}
