// geom.hip -- the geometry stage around the matching path (gfx950): sdg_rectify_map, sdg_remap_u8, sdg_reproject.
//
// Replaces, on the device:
//   Calibration/mycalibration.cpp:826-839   initUndistortRectifyMap(..., CV_16SC2, ...) + remap(..., INTER_LINEAR)
//   the GUI's `calculate`                   disparity -> distance
//
// The definitions are stated in include/sde_geom.h down to the rounding.  The library is built with
// -ffp-contract=off, so every float64 operation below is rounded on its own, in the order written.
#include "sde_common.h"
#include "sde_geom.h"

namespace sde {

struct GeomCal { double K[9], dist[8], Minv[9]; };   // sdg_rectify_map's `cal`, by value in the kernel arguments
struct GeomQ { double q[16]; };                      // sdg_reproject's Q

// dword vectors that promise only dword alignment: a map may start on any int32, and [H][W][2] rows of an odd W
// put every other row's first entry off a 16-byte boundary.  gfx950 global loads and stores of 8 and 16 bytes need
// no more than that.
typedef int int4u __attribute__((ext_vector_type(4), aligned(4)));
typedef int int2u __attribute__((ext_vector_type(2), aligned(4)));

constexpr int FRAC = 5, ONE = 1 << FRAC;                // a map coordinate is in 1/32 pixel
constexpr double COORD_LIMIT = 1073741824.0;            // 2^30

__global__ __launch_bounds__(256) void rectify_map_kernel(GeomCal c, int W, int npix, int32_t *__restrict__ map)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const double v = (double)(p / W), u = (double)(p % W);
    const double X = (c.Minv[0] * u + c.Minv[1] * v) + c.Minv[2];
    const double Y = (c.Minv[3] * u + c.Minv[4] * v) + c.Minv[5];
    const double Wd = (c.Minv[6] * u + c.Minv[7] * v) + c.Minv[8];
    const double x = X / Wd, y = Y / Wd;
    const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4], k4 = c.dist[5],
                 k5 = c.dist[6], k6 = c.dist[7];
    const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = (x * kr + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx);
    const double yd = (y * kr + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy;
    const double us = (c.K[0] * xd + c.K[1] * yd) + c.K[2];
    const double vs = c.K[4] * yd + c.K[5];
    const double a = rint(us * (double)ONE), b = rint(vs * (double)ONE);
    // false for NaN and for either infinity
    const bool ok = fabs(a) < COORD_LIMIT && fabs(b) < COORD_LIMIT;
    int2u e;
    e.x = ok ? (int)a : (int)SDG_NO_SAMPLE;
    e.y = ok ? (int)b : (int)SDG_NO_SAMPLE;
    *reinterpret_cast<int2u *>(map + (size_t)p * 2) = e;
}

// One tap.  `ok` drops when a tap the definition reads (non-zero weight) is outside the source.  The offset is
// formed only for a tap that is read and inside (Hs*Ws < 2^30); any other tap loads byte 0 of the source, which
// always exists, and multiplies it by 0 -- so no load sits behind a branch and a thread's sixteen gathers are in
// flight together instead of one L2 round trip after the other.
__device__ __forceinline__ int remap_tap(const uint8_t *__restrict__ src, int Hs, int Ws, int y, int x, int w, bool &ok)
{
    const bool in = (unsigned)x < (unsigned)Ws && (unsigned)y < (unsigned)Hs;
    ok = ok && (w == 0 || in);
    const bool use = w != 0 && in;
    const unsigned off = use ? (unsigned)y * (unsigned)Ws + (unsigned)x : 0u;
    return (use ? w : 0) * (int)src[off];
}

// dst | valid << 8 of one map entry.  x0, y0 are at most 2^26 in magnitude for any int32, so x0 + 1 cannot wrap.
__device__ __forceinline__ unsigned remap_sample(const uint8_t *__restrict__ src, int Hs, int Ws, int a, int b)
{
    const int x0 = a >> FRAC, fx = a & (ONE - 1), y0 = b >> FRAC, fy = b & (ONE - 1);
    bool ok = true;
    const int s = remap_tap(src, Hs, Ws, y0, x0, (ONE - fx) * (ONE - fy), ok)
                + remap_tap(src, Hs, Ws, y0, x0 + 1, fx * (ONE - fy), ok)
                + remap_tap(src, Hs, Ws, y0 + 1, x0, (ONE - fx) * fy, ok)
                + remap_tap(src, Hs, Ws, y0 + 1, x0 + 1, fx * fy, ok);
    return (unsigned)((s + (1 << (2 * FRAC - 1))) >> (2 * FRAC)) | (ok ? 256u : 0u);
}

// The output depends on its map entry alone, so an image is walked as npix pixels in a line rather than by rows:
// thread 0 takes the `head` pixels before dst's first 4-byte boundary, every other thread four pixels from a
// boundary on -- two 16-byte map loads, sixteen byte gathers (a source pair of a few MB stays in L2), one
// dword store -- and the last one the tail, by bytes.  blockIdx.z is the image.
__global__ __launch_bounds__(256) void remap_u8_kernel(const uint8_t *__restrict__ src, int Hs, int Ws,
                                                       const int32_t *__restrict__ map, int npix,
                                                       uint8_t *__restrict__ dst, uint8_t *__restrict__ valid)
{
    const size_t img = blockIdx.z;
    src += img * (size_t)Hs * Ws;
    map += img * (size_t)npix * 2;
    dst += img * (size_t)npix;
    if (valid) valid += img * (size_t)npix;
    const int head = min((int)(-reinterpret_cast<uintptr_t>(dst) & 3), npix);
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int p0 = t == 0 ? 0 : head + 4 * (t - 1);
    if (p0 >= npix) return;
    const int p1 = t == 0 ? head : min(p0 + 4, npix);
    if (t != 0 && p1 - p0 == 4) {
        const int4u m0 = *reinterpret_cast<const int4u *>(map + (size_t)p0 * 2);
        const int4u m1 = *reinterpret_cast<const int4u *>(map + (size_t)p0 * 2 + 4);
        const unsigned r0 = remap_sample(src, Hs, Ws, m0.x, m0.y), r1 = remap_sample(src, Hs, Ws, m0.z, m0.w),
                       r2 = remap_sample(src, Hs, Ws, m1.x, m1.y), r3 = remap_sample(src, Hs, Ws, m1.z, m1.w);
        *reinterpret_cast<uint32_t *>(dst + p0) = (r0 & 255) | (r1 & 255) << 8 | (r2 & 255) << 16 | (r3 & 255) << 24;
        if (valid) {
            // valid need not share dst's alignment
            if ((reinterpret_cast<uintptr_t>(valid + p0) & 3) == 0) {
                *reinterpret_cast<uint32_t *>(valid + p0) = r0 >> 8 | (r1 >> 8) << 8 | (r2 >> 8) << 16 | (r3 >> 8) << 24;
            } else {
                valid[p0] = (uint8_t)(r0 >> 8);
                valid[p0 + 1] = (uint8_t)(r1 >> 8);
                valid[p0 + 2] = (uint8_t)(r2 >> 8);
                valid[p0 + 3] = (uint8_t)(r3 >> 8);
            }
        }
        return;
    }
    for (int p = p0; p < p1; p++) {
        const unsigned r = remap_sample(src, Hs, Ws, map[(size_t)p * 2], map[(size_t)p * 2 + 1]);
        dst[p] = (uint8_t)r;
        if (valid) valid[p] = (uint8_t)(r >> 8);
    }
}

__global__ __launch_bounds__(256) void reproject_kernel(const float *__restrict__ disp, int W, int npix, GeomQ Q,
                                                        float min_disp, float *__restrict__ depth,
                                                        float *__restrict__ xyz)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float df = disp[p];
    float X = 0.0f, Y = 0.0f, Z = 0.0f;
    if (finite_f32(df) && df > min_disp) {
        const double y = (double)(p / W), x = (double)(p % W), d = (double)df;
        const double *q = Q.q;
        const double v0 = ((q[0] * x + q[1] * y) + q[2] * d) + q[3];
        const double v1 = ((q[4] * x + q[5] * y) + q[6] * d) + q[7];
        const double v2 = ((q[8] * x + q[9] * y) + q[10] * d) + q[11];
        const double v3 = ((q[12] * x + q[13] * y) + q[14] * d) + q[15];
        X = (float)(v0 / v3);
        Y = (float)(v1 / v3);
        Z = (float)(v2 / v3);
    }
    if (depth) depth[p] = Z;
    if (xyz) {
        float *o = xyz + (size_t)p * 3;
        o[0] = X;
        o[1] = Y;
        o[2] = Z;
    }
}

static inline bool bad_shape(int H, int W) { return H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30); }

}  // namespace sde

using namespace sde;

SDE_EXPORT int sdg_rectify_map(const double *cal, int H, int W, int32_t *map, void *stream)
{
    if (!cal || !map || bad_shape(H, W)) return SDE_ERR_ARG;
    GeomCal c;
    for (int i = 0; i < 9; i++) c.K[i] = cal[i];
    for (int i = 0; i < 8; i++) c.dist[i] = cal[9 + i];
    for (int i = 0; i < 9; i++) c.Minv[i] = cal[17 + i];
    const int npix = H * W;
    rectify_map_kernel<<<cdiv(npix, 256), 256, 0, as_stream(stream)>>>(c, W, npix, map);
    return launch_status();
}

SDE_EXPORT int sdg_remap_u8(const uint8_t *src, int nimg, int Hs, int Ws, const int32_t *map, int H, int W,
                            uint8_t *dst, uint8_t *valid, void *stream)
{
    if (!src || !map || !dst || nimg < 1 || nimg > 65535 || bad_shape(Hs, Ws) || bad_shape(H, W)) return SDE_ERR_ARG;
    const int npix = H * W;
    // thread 0 for the head and cdiv(npix - head, 4) <= cdiv(npix, 4) threads of four pixels
    dim3 grid(cdiv((int64_t)cdiv(npix, 4) + 1, 256), 1, nimg);
    remap_u8_kernel<<<grid, 256, 0, as_stream(stream)>>>(src, Hs, Ws, map, npix, dst, valid);
    return launch_status();
}

SDE_EXPORT int sdg_reproject(const float *disp, int H, int W, const double *Q, float min_disp, float *depth,
                             float *xyz, void *stream)
{
    if (!disp || !Q || (!depth && !xyz) || bad_shape(H, W)) return SDE_ERR_ARG;
    GeomQ q;
    for (int i = 0; i < 16; i++) q.q[i] = Q[i];
    const int npix = H * W;
    reproject_kernel<<<cdiv(npix, 256), 256, 0, as_stream(stream)>>>(disp, W, npix, q, min_disp, depth, xyz);
    return launch_status();
}
