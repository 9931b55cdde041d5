// postprocess.hip -- the GPU path's disparity post-processing (gfx950): left-right check, LRC fill, 5x5 median.
//
// Replaces (process_functional.py):
//   is_error_match_kernel / LRC_kernel :977-1088
//   Median_Filter_kernel               :840-879
#include "sde_common.h"

namespace sde {

// The reference's uint8(v) of a finite v: truncation toward zero, then the low byte of the two's-complement
// integer.  |v| >= 2^63 does not fit the cast; such a double is a multiple of 2^11, so its low byte is 0.
__device__ __forceinline__ int u8cast(double v)
{
    if (v >= 0x1p63 || v <= -0x1p63) return 0;
    return (int)((long long)v & 255);
}

// A pixel whose column value (x - d left, x + d right) is not finite, or whose cast column is >= W, is skipped:
// its flag byte stays as the caller set it, and nothing outside the row is read.
__global__ __launch_bounds__(256) void lr_check_kernel(const float *__restrict__ dl, const float *__restrict__ dr,
                                                       int H, int W, uint8_t *__restrict__ lrcl,
                                                       uint8_t *__restrict__ lrcr)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p % W);
    const double ld = dl[p];
    const double rd = (double)x - ld;
    if (rd >= 0 && rd < (double)__builtin_inf()) {
        const int col = u8cast(rd);
        if (col < W) {
            const double mn = ld - (double)dr[(size_t)y * W + col];
            lrcl[p] = (mn > 1 || mn < -1) ? 1 : 0;
        }
    }
    const double rd2 = dr[p];
    const double ld2 = (double)x + rd2;
    if (ld2 < W && ld2 > -(double)__builtin_inf()) {
        const int col = u8cast(ld2);
        if (col < W) {
            const double mn = rd2 - (double)dl[(size_t)y * W + col];
            lrcr[p] = (mn > 1 || mn < -1) ? 1 : 0;
        }
    }
}

// Left-right consistency without lr_check_kernel's uint8 column cast (which compares against column (x -+ d) & 255:
// the reference's arithmetic, a consistency check only for W <= 256).  The same float64 arithmetic with the column
// taken as the plain truncated integer: a pixel is flagged (1) when its disparity d is negative (no winner), or
// when its counterpart -- x - d in the right map for a left pixel, x + d in the left map for a right pixel -- is
// inside the row and the two disparities differ by more than max_diff; every other pixel gets 0.  Every pixel is
// written (no caller zeroing).  The column is in [0, x] (0 <= d <= x) or [x, W - 1] (d >= 0, x + d < W): never
// outside the row; a NaN disparity fails every compare and gets 0, as in lr_check_kernel.
__global__ __launch_bounds__(256) void lr_consistency_kernel(const float *__restrict__ dl, const float *__restrict__ dr,
                                                             int H, int W, double max_diff,
                                                             uint8_t *__restrict__ lrcl, uint8_t *__restrict__ lrcr)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p % W);
    const size_t row = (size_t)y * W;
    const double ld = dl[p];
    const double xr = (double)x - ld;
    uint8_t fl = 0;
    if (ld < 0) {
        fl = 1;
    } else if (xr >= 0) {
        const double mn = ld - (double)dr[row + (int)xr];
        fl = (mn > max_diff || mn < -max_diff) ? 1 : 0;
    }
    lrcl[p] = fl;
    const double rd = dr[p];
    const double xl = (double)x + rd;
    uint8_t fr = 0;
    if (rd < 0) {
        fr = 1;
    } else if (xl < W) {
        const double mn = rd - (double)dl[row + (int)xl];
        fr = (mn > max_diff || mn < -max_diff) ? 1 : 0;
    }
    lrcr[p] = fr;
}

// LRC_kernel (:1003-1088): every flagged pixel takes the mean of the nearest unflagged
// pixel above, below, to the right and to the left (each only if it exists), summed in
// that order in float64.  The reference walks each direction pixel by pixel, which is
// quadratic in the length of a flagged run; here linear scans find the same four
// pixels.  Pass 1 (wave per column): nearest unflagged row above / below of every
// flagged pixel, parked in the output as two 16-bit row indices (0xFFFF = none).
// Pass 2 (wave per row): nearest unflagged column to the left (sweep left -> right) and
// to the right (sweep right -> left) by wave-wide max-scans over 64-pixel chunks; the
// right sweep, which runs second, has all four neighbours and writes the result.
constexpr uint32_t LRC_NONE = 0xFFFFu;

// inclusive max-scan over the 64 lanes
__device__ __forceinline__ int wave_max_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v = v > t ? v : t;
    }
    return v;
}

// One 64-position chunk of a sweep.  mine: this lane's index along the sweep if its pixel is unflagged, else
// -1; carry: the largest unflagged index of the chunks before (-1 = none).  Returns the nearest unflagged
// index strictly before this lane (-1 = none) and advances carry past the chunk.
__device__ __forceinline__ int lrc_nearest_before(int mine, int &carry)
{
    const int v = wave_max_scan(mine);
    int prev = __shfl_up(v, 1, 64);
    if ((threadIdx.x & 63) == 0) prev = -1;
    const int near = prev > carry ? prev : carry;
    const int last = __builtin_amdgcn_readlane(v, 63);
    carry = last > carry ? last : carry;
    return near;
}

// Pass 1: one wave per column, 64 rows per step, wave-wide max-scans downwards (nearest
// unflagged row above, strictly) and upwards (below), carried across chunks.
__global__ __launch_bounds__(64) void lrc_cols_kernel(const uint8_t *__restrict__ f, int H, int W,
                                                      uint32_t *__restrict__ park)
{
    const int x = blockIdx.x;
    const int lane = threadIdx.x;
    const int nchunk = (H + 63) / 64;
    int carry = -1;
    for (int c = 0; c < nchunk; c++) {             // top -> bottom
        const int y = c * 64 + lane;
        const bool in = y < H;
        const bool flagged = in && f[(size_t)y * W + x] == 1;
        const int up = lrc_nearest_before(in && !flagged ? y : -1, carry);
        if (flagged) park[(size_t)y * W + x] = up < 0 ? LRC_NONE : (uint32_t)up;
    }
    carry = -1;                                    // as H-1-y of the nearest unflagged row below
    for (int c = 0; c < nchunk; c++) {             // bottom -> top
        const int y = H - 1 - (c * 64 + lane);
        const bool in = y >= 0;
        const bool flagged = in && f[(size_t)(in ? y : 0) * W + x] == 1;
        const int dn = lrc_nearest_before(in && !flagged ? H - 1 - y : -1, carry);
        if (flagged) park[(size_t)y * W + x] |= (dn < 0 ? LRC_NONE : (uint32_t)(H - 1 - dn)) << 16;
    }
}

__global__ __launch_bounds__(64) void lrc_rows_kernel(const float *__restrict__ dl, const uint8_t *__restrict__ f,
                                                      int H, int W, float *__restrict__ out)
{
    // nearest unflagged column left of x (LRC_NONE = none): 2 B per column of the row, W <= 65535
    extern __shared__ uint16_t sleft[];
    const int y = blockIdx.x;
    const int lane = threadIdx.x;
    const size_t row = (size_t)y * W;
    const uint32_t *park = reinterpret_cast<const uint32_t *>(out);
    const int nchunk = (W + 63) / 64;
    int carry = -1;
    for (int c = 0; c < nchunk; c++) {             // left -> right
        const int x = c * 64 + lane;
        const bool in = x < W;
        const bool clear = in && f[row + x] != 1;
        // lrc_nearest_before's step written out: here the store sits before the carry's readlane
        const int v = wave_max_scan(clear ? x : -1);
        int prev = __shfl_up(v, 1, 64);
        if (lane == 0) prev = -1;
        const int lft = prev > carry ? prev : carry;
        if (in) sleft[x] = lft < 0 ? (uint16_t)LRC_NONE : (uint16_t)lft;
        const int last = __builtin_amdgcn_readlane(v, 63);
        carry = last > carry ? last : carry;
    }
    __syncthreads();
    carry = -1;                                    // as W-1-x of the nearest unflagged column to the right
    for (int c = 0; c < nchunk; c++) {             // right -> left
        const int x = W - 1 - (c * 64 + lane);
        const bool in = x >= 0;
        const bool flagged = in && f[row + x] == 1;
        const int rr = lrc_nearest_before(in && !flagged ? W - 1 - x : -1, carry);
        if (!in) continue;
        if (!flagged) {
            out[row + x] = dl[row + x];
            continue;
        }
        const uint32_t pk = park[row + x];
        const uint32_t up = pk & 0xFFFFu, down = pk >> 16;
        const int left = sleft[x] == LRC_NONE ? -1 : (int)sleft[x];
        int number = 0;
        double sum = 0.0;
        if (up != LRC_NONE) { number++; sum += dl[(size_t)up * W + x]; }
        if (down != LRC_NONE) { number++; sum += dl[(size_t)down * W + x]; }
        if (rr >= 0) { number++; sum += dl[row + (W - 1 - rr)]; }
        if (left >= 0) { number++; sum += dl[row + left]; }
        out[row + x] = number > 0 ? (float)(sum / number) : dl[row + x];
    }
}

__global__ __launch_bounds__(256) void median5_kernel(const float *__restrict__ src, int H, int W,
                                                      float *__restrict__ dst)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15) + 2;
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4) + 2;
    if (y + 2 >= H || x + 2 >= W) return;
    float w[25];
#pragma unroll
    for (int i = -2; i <= 2; i++)
#pragma unroll
        for (int j = -2; j <= 2; j++) w[(i + 2) * 5 + j + 2] = src[(size_t)(y + i) * W + x + j];
    float cur = 0.0f;
    // partial selection sort to the 13th smallest, same swaps as the reference
    for (int i = 0; i < 13; i++) {
        cur = w[i];
        int ci = i;
        for (int j = i + 1; j < 25; j++)
            if (cur > w[j]) { cur = w[j]; ci = j; }
        w[ci] = w[i];
    }
    dst[(size_t)y * W + x] = cur;
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int sde_lr_check(const float *disp_l, const float *disp_r, int H, int W, uint8_t *lrc_l, uint8_t *lrc_r,
                            void *stream)
{
    if (!disp_l || !disp_r || !lrc_l || !lrc_r || H <= 0 || W <= 0) return SDE_ERR_ARG;
    lr_check_kernel<<<cdiv((int64_t)H * W, 256), 256, 0, as_stream(stream)>>>(disp_l, disp_r, H, W, lrc_l, lrc_r);
    return launch_status();
}

SDE_EXPORT int sde_lr_consistency(const float *disp_l, const float *disp_r, int H, int W, float max_diff,
                                  uint8_t *lrc_l, uint8_t *lrc_r, void *stream)
{
    if (!disp_l || !disp_r || !lrc_l || !lrc_r || H <= 0 || W <= 0 || !(max_diff >= 0.0f)) return SDE_ERR_ARG;
    lr_consistency_kernel<<<cdiv((int64_t)H * W, 256), 256, 0, as_stream(stream)>>>(disp_l, disp_r, H, W,
                                                                                    (double)max_diff, lrc_l, lrc_r);
    return launch_status();
}

SDE_EXPORT int sde_lrc_fill(const float *disp_l, const uint8_t *lrc_l, int H, int W, float *out, void *stream)
{
    if (!disp_l || !lrc_l || !out || H <= 0 || W <= 0) return SDE_ERR_ARG;
    // 16-bit row / column indices (0xFFFF = none); the row pass keeps 2 B per column in LDS (<= 128 KB)
    if (H >= (int)LRC_NONE || W >= (int)LRC_NONE || out == disp_l) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    lrc_cols_kernel<<<W, 64, 0, st>>>(lrc_l, H, W, reinterpret_cast<uint32_t *>(out));
    launch_lds_dyn<lrc_rows_kernel, 2 * LRC_NONE>(H, 64, 2 * (size_t)W, st, disp_l, lrc_l, H, W, out);
    return launch_status();
}

SDE_EXPORT int sde_median5(const float *src, int H, int W, float *dst, void *stream)
{
    if (!src || !dst || H <= 0 || W <= 0) return SDE_ERR_ARG;
    if (H < 5 || W < 5) return SDE_OK;   // no interior pixel
    dim3 grid(cdiv(W - 4, 16), cdiv(H - 4, 16));
    median5_kernel<<<grid, 256, 0, as_stream(stream)>>>(src, H, W, dst);
    return launch_status();
}
