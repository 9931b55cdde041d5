// local.hip -- the classical local matcher (gfx950): census / rank transforms, Hamming and SAD+SSD costs, and
// the fused cost + WTA forms that write no volume.
//
// Replaces (local_mathod.py):
//   AD               :13-49      sde_ad_cost, sde_ad_wta
//   Rank_transform   :51-75      sde_rank_transform
//   Census_transform :77-130     sde_census_transform
//   Census_Cost      :132-150    sde_census_cost, sde_census_wta
//   WTA__kernel      :152-165    the fused forms' first strict minimum (SDE_WTA_INIT_D0)
//
// The definitions are stated in include/sde.h.  All arithmetic is integer (the reference's float32 / float64
// values are integers it represents exactly); a cost becomes float32 once, by a round-to-nearest-even convert.
#include "sde_common.h"

namespace sde {

// a pixel outside the image reads as 0
__device__ __forceinline__ int px(const uint8_t *__restrict__ img, int H, int W, int r, int c)
{
    return (r >= 0 && r < H && c >= 0 && c < W) ? (int)img[(size_t)r * W + c] : 0;
}

// ---------------------------------------------------------------------------------------------------------
// transforms: one lane per pixel, images back to back
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void census_kernel(const uint8_t *__restrict__ imgs, int64_t npix_all, int H, int W,
                                                     uint32_t *__restrict__ census)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix_all) return;
    const int64_t hw = (int64_t)H * W;
    const uint8_t *img = imgs + (p / hw) * hw;
    const int q = (int)(p % hw), y = q / W, x = q % W;
    uint32_t w = 0;
    for (int r = y - 3; r < y; r++)
        for (int c = x - 4; c < x; c++) w = (w << 1) | (px(img, H, W, r, c) > px(img, H, W, 2 * y - r, 2 * x - c));
    for (int r = y - 3; r < y; r++) w = (w << 1) | (px(img, H, W, r, x) > px(img, H, W, 2 * y - r, x));
    for (int c = x - 4; c < x; c++) w = (w << 1) | (px(img, H, W, y, c) > px(img, H, W, y, 2 * x - c));
    census[p] = w;
}

__global__ __launch_bounds__(256) void rank_kernel(const uint8_t *__restrict__ imgs, int64_t npix_all, int H, int W,
                                                   uint8_t *__restrict__ rank)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix_all) return;
    const int64_t hw = (int64_t)H * W;
    const uint8_t *img = imgs + (p / hw) * hw;
    const int q = (int)(p % hw), y = q / W, x = q % W;
    const int centre = img[q];
    int n = 0;
    for (int r = y - 3; r <= y + 3; r++)
        for (int c = x - 3; c <= x + 3; c++) n += centre >= px(img, H, W, r, c);
    rank[p] = (uint8_t)n;
}

// ---------------------------------------------------------------------------------------------------------
// volumes (for parity checks and to feed SGM): one lane per voxel, d fastest
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void census_cost_kernel(const uint32_t *__restrict__ cl, const uint32_t *__restrict__ cr,
                                                          int W, int D, int64_t nvox, float invalid,
                                                          float *__restrict__ outl, float *__restrict__ outr)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(v % D);
        const int64_t p = v / D;            // y * W + x
        const int x = (int)(p % W);
        if (outl) outl[v] = x - d >= 0 ? (float)__popc(cl[p] ^ cr[p - d]) : invalid;
        if (outr) outr[v] = x + d < W ? (float)__popc(cl[p + d] ^ cr[p]) : invalid;
    }
}

// the column range of the window at x (the reference's three branches)
__device__ __forceinline__ void ad_columns(int x, int W, int D, int k, int &c0, int &c1)
{
    if (x < D + k) { c0 = x; c1 = x + k; }
    else if (x + k < W - k) { c0 = x - k; c1 = x + k; }
    else { c0 = x - k; c1 = x; }
}

__global__ __launch_bounds__(256) void ad_cost_kernel(const uint8_t *__restrict__ il, const uint8_t *__restrict__ ir,
                                                      int H, int W, int D, int k, int64_t nvox, float invalid,
                                                      float *__restrict__ out)
{
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(v % D);
        const int64_t p = v / D;
        const int x = (int)(p % W), y = (int)(p / W);
        if (x - d < 0) {
            out[v] = invalid;
            continue;
        }
        int c0, c1;
        ad_columns(x, W, D, k, c0, c1);     // W >= D + 2k: c1 < W and c0 - d >= 0
        const int r0 = max(y - k, 0), r1 = min(y + k, H - 1);
        int sum = 0;
        for (int r = r0; r <= r1; r++)
            for (int c = c0; c <= c1; c++) {
                const int df = (int)il[(size_t)r * W + c] - (int)ir[(size_t)r * W + c - d];
                sum += abs(df) + df * df;
            }
        out[v] = (float)sum;
    }
}

// ---------------------------------------------------------------------------------------------------------
// fused Hamming cost + WTA, both views in one pass over a row segment
// ---------------------------------------------------------------------------------------------------------
// One workgroup per (row, segment of CW_TILE columns).  The left census words of columns [x0, x0 + CW_TILE + D - 1)
// and the right ones of [x0 - (D - 1), x0 + CW_TILE) sit in LDS (words outside the row as 0: only voxels inside
// the row are scanned); one lane per pixel loops over d, consecutive lanes read consecutive dwords (no bank
// conflict).  The winner is the unsigned minimum of the key (popcount << 10) | d (popcount <= 19 < 2^22,
// d < 512 < 2^10): the first minimum with no compare/select pair.  d = 0 is always inside the row, so the
// scan never needs the invalid value.
constexpr int CW_TILE = 1024;
constexpr int CW_THREADS = 256;
constexpr int CW_MAXD = 512;

template <bool LEFT, bool RIGHT>
__global__ __launch_bounds__(CW_THREADS) void census_wta_kernel(const uint32_t *__restrict__ cl,
                                                                const uint32_t *__restrict__ cr, int W, int D,
                                                                float *__restrict__ displ, float *__restrict__ minl,
                                                                float *__restrict__ dispr, float *__restrict__ minr)
{
    __shared__ uint32_t sl[CW_TILE + CW_MAXD - 1];   // sl[i] = cl[x0 + i]
    __shared__ uint32_t sr[CW_TILE + CW_MAXD - 1];   // sr[i] = cr[x0 - (D - 1) + i]
    const int x0 = blockIdx.x * CW_TILE;
    const size_t row = (size_t)blockIdx.y * W;
    const int n = CW_TILE + D - 1;
    for (int i = threadIdx.x; i < n; i += CW_THREADS) {
        const int xl = x0 + i, xr = x0 - (D - 1) + i;
        sl[i] = (RIGHT || i < CW_TILE) && xl < W ? cl[row + xl] : 0u;
        sr[i] = xr >= 0 && xr < W ? cr[row + xr] : 0u;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < CW_TILE; p += CW_THREADS) {
        const int x = x0 + p;
        if (x >= W) break;
        const uint32_t wl = sl[p], wr = sr[p + D - 1];
        if (LEFT) {
            const int dn = min(D - 1, x);             // x - d >= 0
            const uint32_t *q = sr + p + D - 1;       // q[-d] = cr[x - d]
            uint32_t key = 0xFFFFFFFFu;
            for (int d = 0; d <= dn; d++) key = min(key, ((uint32_t)__popc(wl ^ q[-d]) << 10) | (uint32_t)d);
            if (displ) displ[row + x] = (float)(key & 1023u);
            if (minl) minl[row + x] = (float)(key >> 10);
        }
        if (RIGHT) {
            const int dn = min(D - 1, W - 1 - x);     // x + d < W
            const uint32_t *q = sl + p;               // q[d] = cl[x + d]
            uint32_t key = 0xFFFFFFFFu;
            for (int d = 0; d <= dn; d++) key = min(key, ((uint32_t)__popc(q[d] ^ wr) << 10) | (uint32_t)d);
            if (dispr) dispr[row + x] = (float)(key & 1023u);
            if (minr) minr[row + x] = (float)(key >> 10);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// fused SAD+SSD cost + WTA
// ---------------------------------------------------------------------------------------------------------
// The window sum is separable: V(y, c, d) = sum over the clipped rows of e(r, c, d), cost(y, x, d) = sum of
// V(y, c, d) over the column range of x.  One workgroup owns AW_ROWS (4 or 8) rows and TX = 256 - 2k output
// columns, i.e. the 256 columns c in [x0 - k, x0 + TX + k) that their windows touch (one per lane).  The rows
// [y0 - k, y0 + AW_ROWS + k) of both images sit in LDS as bytes, rows and columns outside the image as 0 in both
// images, so a row outside the image adds e = 0 and the row clipping needs no branch; columns outside the
// image are only ever read for voxels that no valid window uses (W >= D + 2k).
//   phase 1 (lane = column c): V for AW_DB disparities in registers; the band's first row sums 2k + 1 rows,
//     every later row adds the row that enters and subtracts the row that leaves (a running sum: about
//     (2k + 1 + 2 (AW_ROWS - 1)) / AW_ROWS evaluations of e per voxel instead of 2k + 1).  Left bytes are read
//     once per row and serve the AW_DB disparities; consecutive lanes read consecutive bytes.
//   phase 2 (lane = output pixel x): sums its k + 1 or 2k + 1 values of V from LDS, four disparities per
//     16-byte read (consecutive lanes, consecutive 16-byte slots), and keeps the first strict minimum per row
//     of the band in registers.
// V is double-buffered in LDS, so one barrier per (disparity block, row) separates the phases.  All sums are
// int32 (at most 65 * 65 * 65280 < 2^31); the winner's cost is converted to float32 once.
constexpr int AW_THREADS = 256;
constexpr int AW_ROWS_MAX = 8;
constexpr int AW_DB = 8;                 // disparities per step, a multiple of 4
constexpr int AW_MAXK = SDE_LOCAL_MAX_RADIUS;
constexpr int AW_MAXD = 512;
constexpr int AW_LPITCH = AW_THREADS;
// rows * (left pitch + right pitch) at k = AW_MAXK, D = AW_MAXD
constexpr int AW_MAX_SMEM = (AW_ROWS_MAX + 2 * AW_MAXK) * (AW_LPITCH + ((AW_THREADS + AW_MAXD - 1 + 3) & ~3));

// e = |l - r| + (l - r)^2 = a (a + 1) with a = |l - r| from v_sad_u8 (the operands' upper three bytes are 0)
__device__ __forceinline__ int ad_e(uint32_t l, uint32_t r)
{
    const uint32_t a = __builtin_amdgcn_sad_u8(l, r, 0u);
    return (int)__umul24(a, a + 1u);
}

template <int AW_ROWS>
__global__ __launch_bounds__(AW_THREADS) void ad_wta_kernel(const uint8_t *__restrict__ il, const uint8_t *__restrict__ ir,
                                                            int H, int W, int D, int k, int rpitch,
                                                            float *__restrict__ disp, float *__restrict__ mincost)
{
    extern __shared__ uint8_t smem[];
    __shared__ int4 sv[2][AW_DB / 4][AW_THREADS];    // V of 4 consecutive disparities per 16-B slot
    const int t = threadIdx.x;
    const int TX = AW_THREADS - 2 * k;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * AW_ROWS;
    const int nrow = AW_ROWS + 2 * k;
    uint8_t *ls = smem;                               // ls[rr][j] = il[y0 - k + rr][x0 - k + j], j < 256
    uint8_t *rs = smem + nrow * AW_LPITCH;            // rs[rr][j] = ir[y0 - k + rr][x0 - k - (D - 1) + j], j < 255 + D
    const int rw = AW_THREADS + D - 1;
    for (int rr = 0; rr < nrow; rr++) {
        const int r = y0 - k + rr;
        const bool rin = r >= 0 && r < H;
        const int c = x0 - k + t;
        ls[rr * AW_LPITCH + t] = rin && c >= 0 && c < W ? il[(size_t)r * W + c] : (uint8_t)0;
        for (int j = t; j < rw; j += AW_THREADS) {
            const int cr_ = x0 - k - (D - 1) + j;
            rs[rr * rpitch + j] = rin && cr_ >= 0 && cr_ < W ? ir[(size_t)r * W + cr_] : (uint8_t)0;
        }
    }
    __syncthreads();

    // phase 2's window of this lane's pixel, as indices into sv[..][..][j] (j = c - (x0 - k))
    const int x = x0 + t;
    const bool owner = t < TX && x < W;
    int jlo = 0, jn = 0;
    if (owner) {
        int c0, c1;
        ad_columns(x, W, D, k, c0, c1);
        jlo = c0 - (x0 - k);
        jn = c1 - c0 + 1;
    }
    int best[AW_ROWS], bestd[AW_ROWS];
#pragma unroll
    for (int i = 0; i < AW_ROWS; i++) {
        best[i] = 0x7FFFFFFF;
        bestd[i] = 0;
    }

    int step = 0;
    for (int db = 0; db < D; db += AW_DB) {
        // rs index of the right pixel of (column t, disparity d): t + (D - 1) - d; d >= D repeats D - 1
        int jr[AW_DB];
#pragma unroll
        for (int dd = 0; dd < AW_DB; dd++) jr[dd] = t + (D - 1) - min(db + dd, D - 1);
        int V[AW_DB];
#pragma unroll
        for (int dd = 0; dd < AW_DB; dd++) V[dd] = 0;
        for (int rr = 0; rr <= 2 * k; rr++) {
            const uint32_t l = ls[rr * AW_LPITCH + t];
#pragma unroll
            for (int dd = 0; dd < AW_DB; dd++) V[dd] += ad_e(l, rs[rr * rpitch + jr[dd]]);
        }
#pragma unroll
        for (int i = 0; i < AW_ROWS; i++, step++) {
            if (i > 0) {
                const int ra = i + 2 * k, rb = i - 1;          // the row that enters, the row that leaves
                const uint32_t la = ls[ra * AW_LPITCH + t], lb = ls[rb * AW_LPITCH + t];
#pragma unroll
                for (int dd = 0; dd < AW_DB; dd++)
                    V[dd] += ad_e(la, rs[ra * rpitch + jr[dd]]) - ad_e(lb, rs[rb * rpitch + jr[dd]]);
            }
            int4(*buf)[AW_THREADS] = sv[step & 1];
#pragma unroll
            for (int g = 0; g < AW_DB / 4; g++) buf[g][t] = make_int4(V[4 * g], V[4 * g + 1], V[4 * g + 2], V[4 * g + 3]);
            __syncthreads();
            // the other buffer is written next, after every lane has passed this barrier having finished
            // the reads of the step before
            if (owner) {
                int s[AW_DB];
#pragma unroll
                for (int dd = 0; dd < AW_DB; dd++) s[dd] = 0;
                for (int j = 0; j < jn; j++) {
#pragma unroll
                    for (int g = 0; g < AW_DB / 4; g++) {
                        const int4 v = buf[g][jlo + j];
                        s[4 * g] += v.x;
                        s[4 * g + 1] += v.y;
                        s[4 * g + 2] += v.z;
                        s[4 * g + 3] += v.w;
                    }
                }
#pragma unroll
                for (int dd = 0; dd < AW_DB; dd++) {
                    const int d = db + dd;
                    if (d < D && d <= x && best[i] > s[dd]) {
                        best[i] = s[dd];
                        bestd[i] = d;
                    }
                }
            }
        }
    }
    if (owner) {
#pragma unroll
        for (int i = 0; i < AW_ROWS; i++) {
            const int y = y0 + i;
            if (y < H) {
                if (disp) disp[(size_t)y * W + x] = (float)bestd[i];
                if (mincost) mincost[(size_t)y * W + x] = (float)best[i];
            }
        }
    }
}

static inline bool local_shape_ok(int H, int W, int D) { return H >= 1 && W >= 1 && D >= 1 && D <= 512; }

static inline bool ad_args_ok(int H, int W, int D, int k)
{
    return local_shape_ok(H, W, D) && k >= 0 && k <= SDE_LOCAL_MAX_RADIUS && (int64_t)W >= (int64_t)D + 2 * k;
}

// blocks of a grid-stride launch over n items
static inline int stride_grid(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 1 << 20); }

}  // namespace sde

using namespace sde;

SDE_EXPORT int sde_census_transform(const uint8_t *imgs, int nimg, int H, int W, uint32_t *census, void *stream)
{
    if (!imgs || !census || nimg < 1 || H < 1 || W < 1) return SDE_ERR_ARG;
    const int64_t n = (int64_t)nimg * H * W;
    if ((int64_t)H * W > 0x7FFFFFFF || (n + 255) / 256 > 0x7FFFFFFF) return SDE_ERR_ARG;
    census_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(imgs, n, H, W, census);
    return launch_status();
}

SDE_EXPORT int sde_rank_transform(const uint8_t *imgs, int nimg, int H, int W, uint8_t *rank, void *stream)
{
    if (!imgs || !rank || nimg < 1 || H < 1 || W < 1) return SDE_ERR_ARG;
    const int64_t n = (int64_t)nimg * H * W;
    if ((int64_t)H * W > 0x7FFFFFFF || (n + 255) / 256 > 0x7FFFFFFF) return SDE_ERR_ARG;
    rank_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(imgs, n, H, W, rank);
    return launch_status();
}

SDE_EXPORT int sde_census_cost(const uint32_t *census_l, const uint32_t *census_r, int H, int W, int D, float invalid,
                               float *out_left, float *out_right, void *stream)
{
    if (!census_l || !census_r || (!out_left && !out_right) || !local_shape_ok(H, W, D)) return SDE_ERR_ARG;
    const int64_t nvox = (int64_t)H * W * D;
    census_cost_kernel<<<stride_grid(nvox), 256, 0, as_stream(stream)>>>(census_l, census_r, W, D, nvox, invalid,
                                                                         out_left, out_right);
    return launch_status();
}

SDE_EXPORT int sde_census_wta(const uint32_t *census_l, const uint32_t *census_r, int H, int W, int D, float *disp_l,
                              float *min_l, float *disp_r, float *min_r, void *stream)
{
    if (!census_l || !census_r || (!disp_l && !disp_r) || !local_shape_ok(H, W, D) || H > 65535) return SDE_ERR_ARG;
    // a view is computed when its disparity map is asked for; its min alone is not a request
    if ((min_l && !disp_l) || (min_r && !disp_r)) return SDE_ERR_ARG;
    const dim3 grid(cdiv(W, CW_TILE), H);
    hipStream_t st = as_stream(stream);
    if (disp_l && disp_r)
        census_wta_kernel<true, true><<<grid, CW_THREADS, 0, st>>>(census_l, census_r, W, D, disp_l, min_l, disp_r, min_r);
    else if (disp_l)
        census_wta_kernel<true, false><<<grid, CW_THREADS, 0, st>>>(census_l, census_r, W, D, disp_l, min_l, nullptr, nullptr);
    else
        census_wta_kernel<false, true><<<grid, CW_THREADS, 0, st>>>(census_l, census_r, W, D, nullptr, nullptr, disp_r, min_r);
    return launch_status();
}

SDE_EXPORT int sde_ad_cost(const uint8_t *img_l, const uint8_t *img_r, int H, int W, int D, int radius, float invalid,
                           float *out_left, void *stream)
{
    if (!img_l || !img_r || !out_left || !ad_args_ok(H, W, D, radius)) return SDE_ERR_ARG;
    const int64_t nvox = (int64_t)H * W * D;
    ad_cost_kernel<<<stride_grid(nvox), 256, 0, as_stream(stream)>>>(img_l, img_r, H, W, D, radius, nvox, invalid,
                                                                     out_left);
    return launch_status();
}

SDE_EXPORT int sde_ad_wta(const uint8_t *img_l, const uint8_t *img_r, int H, int W, int D, int radius, float *disp,
                          float *min_cost, void *stream)
{
    if (!img_l || !img_r || !disp || !ad_args_ok(H, W, D, radius)) return SDE_ERR_ARG;
    // rows per workgroup: a band of 8 rows spreads the 2k + 1 rows of its first vertical sum over twice as many
    // outputs as a band of 4, which gives twice as many workgroups; at 1024 x 1024 the short band is the faster
    // one at k = 5 and the long one at k = 10
    const int rows = radius < 8 ? 4 : 8;
    const int TX = AW_THREADS - 2 * radius;
    const int64_t gy = ((int64_t)H + rows - 1) / rows;
    if (gy > 65535) return SDE_ERR_ARG;
    const int rpitch = (AW_THREADS + D - 1 + 3) & ~3;
    const size_t smem = (size_t)(rows + 2 * radius) * (AW_LPITCH + rpitch);
    const dim3 grid(cdiv(W, TX), (unsigned)gy);
    hipStream_t st = as_stream(stream);
    if (rows == 4) {
        ad_wta_kernel<4><<<grid, AW_THREADS, smem, st>>>(img_l, img_r, H, W, D, radius, rpitch, disp, min_cost);
        return launch_status();
    }
    launch_lds_dyn<ad_wta_kernel<8>, AW_MAX_SMEM>(grid, AW_THREADS, smem, st, img_l, img_r, H, W, D, radius, rpitch, disp,
                                                  min_cost);
    return launch_status();
}
