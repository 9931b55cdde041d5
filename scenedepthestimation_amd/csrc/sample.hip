// sample.hip -- training data from resident stereo scenes, and the bad-pixel score (gfx950).
//
// Replaces the patch preparation (image_patches_prepare/middlebury_*.py: choose a centre with known disparity,
// a positive within half a pixel of its match and a negative 1.5 .. 6 pixels off, cut three patches) and
// error_calculate.py:72-81.  The rules are stated in include/sde.h.
//
//   sde_triplet_centres      per-row counts, then each row's block sums the rows before it and writes its centres
//                            in column order by ballot / popcount: ascending order, no atomics
//   sde_train_sample_gather  one wave per triplet; every lane repeats the (counter-based) draw, so scene and
//                            centre stay wave-uniform, and the wave then copies the 3 P x P patches
//   sde_bad_pixels           one lane per pixel, ballot counts, one integer atomic add per block and word
//
// Doubles are rounded one operation at a time (the library is built with -ffp-contract=off).
#include "sde_common.h"

namespace sde {

constexpr int SM_MAX_LAYERS = 5;
constexpr int SM_NF = 64;

// ---------------------------------------------------------------------------------------------------------
// valid centres
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool centre_ok(const float *__restrict__ dl, const float *__restrict__ dr, int H, int W,
                                          int h, bool zero_invalid, int y, int x)
{
    if (y < h || y >= H - h || x < h || x >= W - h) return false;
    const double d = (double)dl[(size_t)y * W + x];
    if (!__builtin_isfinite(d) || !(d >= 0.0) || (zero_invalid && d == 0.0)) return false;
    if (!(d + (double)h <= (double)x)) return false;
    if (dr) {
        const int xr = (int)((double)x - d);          // h <= x - d <= x: inside the row
        const double r = (double)dr[(size_t)y * W + xr];
        if (!__builtin_isfinite(r) || (zero_invalid && r == 0.0) || !(fabs(r - d) <= 1.0)) return false;
    }
    return true;
}

// sum of v over the block's 256 lanes (v >= 0); every lane gets it
__device__ __forceinline__ int block_sum(int v, int *red)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (threadIdx.x % 64 == 0) red[threadIdx.x / 64] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// block = row: rowcount[y] = the number of centres in row y
__global__ __launch_bounds__(256) void centres_count_kernel(const float *__restrict__ dl, const float *__restrict__ dr,
                                                            int H, int W, int h, int zero_invalid,
                                                            int32_t *__restrict__ rowcount)
{
    __shared__ int red[4];
    const int y = blockIdx.x;
    int n = 0;
    if (y >= h && y < H - h)
        for (int x = threadIdx.x; x < W; x += 256) n += centre_ok(dl, dr, H, W, h, zero_invalid != 0, y, x) ? 1 : 0;
    n = block_sum(n, red);
    if (threadIdx.x == 0) rowcount[y] = n;
}

// block = row: its centres go to centres[sum of the rows before it ...], in column order.  rowcount is the tail
// of the centres buffer, past anything written here.
__global__ __launch_bounds__(256) void centres_write_kernel(const float *__restrict__ dl, const float *__restrict__ dr,
                                                            int H, int W, int h, int zero_invalid,
                                                            const int32_t *rowcount, int32_t *centres,
                                                            int32_t *__restrict__ count)
{
    __shared__ int red[4];
    const int y = blockIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    int before = 0;
    for (int r = threadIdx.x; r < y; r += 256) before += rowcount[r];
    int base = block_sum(before, red);
    if (y >= h && y < H - h) {
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + threadIdx.x;
            const bool ok = x < W && centre_ok(dl, dr, H, W, h, zero_invalid != 0, y, x);
            const unsigned long long m = __ballot(ok);
            __syncthreads();
            if (lane == 0) red[wave] = __popcll(m);
            __syncthreads();
            int off = base;
            for (int w = 0; w < wave; w++) off += red[w];
            if (ok) centres[off + __popcll(m & ((1ull << lane) - 1ull))] = y * W + x;
            base += red[0] + red[1] + red[2] + red[3];
        }
    }
    // rows from H - h on hold no centre: the last row's base is the total
    if (y == H - 1 && threadIdx.x == 0) *count = base;
}

// ---------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter c, key k -> four words
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ double philox_unit(const uint32_t x[4])
{
    return (double)(((uint64_t)x[0] << 21) | (uint64_t)(x[1] >> 11)) * 0x1p-53;
}

// block = 4 waves = 4 triplets
__global__ __launch_bounds__(256) void train_sample_gather_kernel(const int64_t *__restrict__ table, int S, uint32_t N,
                                                                  int B, int P, uint32_t k0, uint32_t k1, uint32_t st0,
                                                                  uint32_t st1, int max_rounds,
                                                                  float *__restrict__ patches, int32_t *__restrict__ idx,
                                                                  int32_t *__restrict__ scene)
{
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + threadIdx.x / 64));
    const int lane = threadIdx.x % 64;
    if (i >= B) return;
    const int h = P / 2;
    uint32_t x[4];

    // centre: the last scene whose first <= g
    philox4x32_10((uint32_t)i, st0, st1, 0u, k0, k1, x);
    const uint32_t g = (uint32_t)(((uint64_t)x[0] * N) >> 32);
    int lo = 0, hi = S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint64_t)table[(size_t)mid * SDE_SCENE_WORDS + 6] <= g) lo = mid;
        else hi = mid;
    }
    const int64_t *row = table + (size_t)lo * SDE_SCENE_WORDS;
    const float *img_l = reinterpret_cast<const float *>(row[0]);
    const float *img_r = reinterpret_cast<const float *>(row[1]);
    const float *disp_l = reinterpret_cast<const float *>(row[2]);
    const int32_t *centres = reinterpret_cast<const int32_t *>(row[3]);
    const int H = (int)row[4], W = (int)row[5];
    const int c = centres[g - (uint32_t)row[6]];
    const int y = c / W, xl = c % W;
    const double rc = (double)xl - (double)disp_l[c];

    int pos = (int)rc;
    for (int r = 0; r < max_rounds; r++) {
        philox4x32_10((uint32_t)i, st0, st1, 1u + r, k0, k1, x);
        const double t = 1.002 * philox_unit(x);
        const double o = -0.501 + t;
        const int p = (int)(rc + o);
        if (p >= h && p < W - h) {
            pos = p;
            break;
        }
    }
    int neg = (pos + 2 >= h && pos + 2 < W - h) ? pos + 2 : pos - 2;
    for (int r = 0; r < max_rounds; r++) {
        philox4x32_10((uint32_t)i, st0, st1, 33u + r, k0, k1, x);
        const double t = 4.5 * philox_unit(x);
        const double dev = 1.5 + t;
        const int n = (x[2] & 1u) ? (int)(rc - dev) : (int)(rc + dev);
        if (n >= h && n < W - h) {
            neg = n;
            break;
        }
    }

    if (lane == 0) {
        if (idx) {
            idx[4 * i + 0] = y;
            idx[4 * i + 1] = xl;
            idx[4 * i + 2] = pos;
            idx[4 * i + 3] = neg;
        }
        if (scene) scene[i] = lo;
    }
    const int pp = P * P;
    for (int e = lane; e < 3 * pp; e += 64) {
        const int which = e / pp, q = e % pp;
        const int yy = y + q / P - h;
        const int xx = (which == 0 ? xl : which == 1 ? pos : neg) + q % P - h;
        const float *img = which == 0 ? img_l : img_r;
        patches[((size_t)which * B + i) * pp + q] =
            (yy >= 0 && yy < H && xx >= 0 && xx < W) ? img[(size_t)yy * W + xx] : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// bad pixels
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bad_pixels_kernel(const float *__restrict__ disp, const float *__restrict__ gt,
                                                         int n, double threshold, uint32_t *__restrict__ counts,
                                                         uint8_t *__restrict__ area)
{
    __shared__ int red[2][4];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;      // the last block may reach past 2^31
    bool eval = false, bad = false;
    if (t < n) {
        const double g = (double)gt[t];
        eval = !(g == (double)INFINITY || g == 0.0);
        bad = eval && fabs((double)disp[t] - g) > threshold;
        if (area) {
            area[3 * (size_t)t + 0] = 0;
            area[3 * (size_t)t + 1] = (eval && !bad) ? 255 : 0;
            area[3 * (size_t)t + 2] = bad ? 255 : 0;
        }
    }
    const unsigned long long me = __ballot(eval), mb = __ballot(bad);
    if (threadIdx.x % 64 == 0) {
        red[0][threadIdx.x / 64] = __popcll(me);
        red[1][threadIdx.x / 64] = __popcll(mb);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (s) atomicAdd(&counts[threadIdx.x], (uint32_t)s);
    }
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int sde_triplet_centres(const float *disp_l, const float *disp_r, int H, int W, int nlayers, int flags,
                                   int32_t *centres, int32_t *count, void *stream)
{
    if (!disp_l || !centres || !count || nlayers < 1 || nlayers > SM_MAX_LAYERS || (flags & ~SDE_ZERO_IS_INVALID))
        return SDE_ERR_ARG;
    const int P = 2 * nlayers + 1;
    if (H < P || W < P + 12 || (int64_t)H * W >= (1ll << 31)) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    int32_t *rowcount = centres + ((int64_t)H * W - H);
    const int zi = (flags & SDE_ZERO_IS_INVALID) ? 1 : 0;
    hipLaunchKernelGGL(centres_count_kernel, dim3(H), dim3(256), 0, st, disp_l, disp_r, H, W, nlayers, zi, rowcount);
    hipLaunchKernelGGL(centres_write_kernel, dim3(H), dim3(256), 0, st, disp_l, disp_r, H, W, nlayers, zi,
                       (const int32_t *)rowcount, centres, count);
    return launch_status();
}

SDE_EXPORT int sde_train_sample_gather(const int64_t *table, int S, int64_t N, int B, int nlayers, uint64_t seed,
                                       uint64_t step, int max_rounds, float *patches, int32_t *idx, int32_t *scene,
                                       void *stream)
{
    if (!table || !patches || S < 1 || N < 1 || N >= (1ll << 31) || B < 1 || nlayers < 1 || nlayers > SM_MAX_LAYERS ||
        max_rounds < 1 || max_rounds > SDE_SAMPLE_MAX_ROUNDS)
        return SDE_ERR_ARG;
    const int P = 2 * nlayers + 1;
    if (3ll * B * P * P * SM_NF >= (1ll << 31)) return SDE_ERR_ARG;      // the limit of every sde_train_* entry point
    hipLaunchKernelGGL(train_sample_gather_kernel, dim3(cdiv(B, 4)), dim3(256), 0, as_stream(stream), table, S,
                       (uint32_t)N, B, P, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step,
                       (uint32_t)(step >> 32), max_rounds, patches, idx, scene);
    return launch_status();
}

SDE_EXPORT int sde_bad_pixels(const float *disp, const float *gt, int H, int W, double threshold, uint32_t *counts,
                              uint8_t *area, void *stream)
{
    if (!disp || !gt || !counts || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31) || !(threshold >= 0.0))
        return SDE_ERR_ARG;
    const int n = H * W;
    hipLaunchKernelGGL(bad_pixels_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), disp, gt, n, threshold,
                       counts, area);
    return launch_status();
}
