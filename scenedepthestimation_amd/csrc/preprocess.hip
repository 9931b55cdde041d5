// preprocess.hip -- ahead of the tower: NumPy-exact image statistics, then z-normalisation and zero padding.
#include "sde_common.h"
#include <algorithm>

namespace sde {

// Per-image statistics exactly as NumPy computes them for match_single.py:40-41 (float32 image,
// np.mean / np.std over axes (0, 1)): the reduction over both axes of a contiguous 2-D array adds,
// from 0.0f in order, the pairwise sums (numpy pairwise_sum: blocks <= 128 with 8 accumulators,
// larger blocks halved at a multiple of 8) of consecutive 8192-element pieces of the flattened
// image (np.getbufsize()); mean = S / n in float32; std = sqrt(S' / n) with S' the same reduction
// of (x - mean)^2 (float32 ops, no contraction: the library is built with -ffp-contract=off).
// Pinned against NumPy in tests (test_preprocess_u8: bit-identical at every config size).
// Scratch per image: [mean, std, -, -][piece sums][piece sums of squares].
constexpr int NP_PIECE = 8192;

__device__ __forceinline__ float np_val(const uint8_t *img, int64_t i, float mean, bool sq)
{
    const float x = (float)img[i];
    if (!sq) return x;
    const float d = x - mean;
    return d * d;
}

// numpy pairwise_sum of a block of len <= 128 elements at s
__device__ float np_leaf(const uint8_t *img, int64_t s, int len, float mean, bool sq)
{
    if (len < 8) {
        float res = 0.0f;
        for (int i = 0; i < len; i++) res += np_val(img, s + i, mean, sq);
        return res;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = np_val(img, s + j, mean, sq);
    int i = 8;
    for (; i < len - (len % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] += np_val(img, s + i + j, mean, sq);
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < len; i++) res += np_val(img, s + i, mean, sq);
    return res;
}

__device__ __forceinline__ int np_half(int len) { const int n2 = len / 2; return n2 - n2 % 8; }

// One wave per 8192-element piece: its pairwise sum into the image's scratch.  A full piece is a
// perfect tree of 64 blocks of 128 (lane l sums block l; the xor-butterfly adds adjacent subtrees,
// and float addition is commutative); the last, short piece walks numpy's recursion: every lane
// enumerates the blocks in order (lane k % 64 sums block k into LDS), lane 0 adds them up the tree.
// S = 0.0f + v[0] + v[1] + ... in order (np.mean's / np.std's float32 reduction of the piece sums), then the
// quotient: the wave loads the sums into LDS (one round of latency), lane 0 adds them.  NumPy 2.x divides
// the float32 sum by the intp count in float64 and rounds once to float32 (np.mean: ret.dtype.type(ret /
// rcount); _var: true_divide by an intp into a float32 out, and its final ret / rcount), so the quotient
// is formed in fp64 here too.  Below 2^24 pixels this equals the float32 quotient S / (float)n (fp64 has
// more than 2 * 24 + 2 bits: the double rounding is innocuous); above it (float)n would be inexact.
__device__ __forceinline__ float np_stat(const float *__restrict__ v, int npieces, int64_t n, float *buf, int lane)
{
    float q = 0.0f;
    for (int c0 = 0; c0 < npieces; c0 += 256) {   // LDS chunks of 256 sums
        const int m = min(256, npieces - c0);
        for (int c = lane; c < m; c += 64) buf[c] = v[c0 + c];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0)
            for (int c = 0; c < m; c++) q += buf[c];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    q = __shfl(q, 0, 64);
    return (float)((double)q / (double)n);
}

// SQ: the pass over (x - mean)^2, the mean formed here from the first pass's piece sums (the launch of a
// separate statistics kernel saved); block 0 also stores it.
template <bool SQ>
__global__ __launch_bounds__(64) void np_piece_kernel(const uint8_t *__restrict__ imgs, int64_t n, int sstride,
                                                      float *__restrict__ scratch)
{
    const uint8_t *img = imgs + blockIdx.y * n;
    float *st = scratch + (size_t)blockIdx.y * sstride;
    const int npieces = gridDim.x;
    __shared__ float sbuf[256];
    float mean = 0.0f;
    if (SQ) {
        mean = np_stat(st + 4, npieces, n, sbuf, threadIdx.x);
        if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = mean;
    }
    const int lane = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * NP_PIECE;
    const int m = (int)std::min<int64_t>(NP_PIECE, n - c0);
    float sum;
    if (m == NP_PIECE) {
        sum = np_leaf(img, c0 + 128 * lane, 128, mean, SQ);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);
    } else {
        __shared__ float leaf[256];
        {
            int ss[16], sl[16], sp = 0, k = 0;
            ss[0] = 0; sl[0] = m;
            while (sp >= 0) {
                const int s0 = ss[sp], len = sl[sp];
                sp--;
                if (len <= 128) {
                    if ((k & 63) == lane) leaf[k] = np_leaf(img, c0 + s0, len, mean, SQ);
                    k++;
                } else {
                    const int n2 = np_half(len);
                    ss[++sp] = s0 + n2; sl[sp] = len - n2;     // right, visited second
                    ss[++sp] = s0; sl[sp] = n2;                // left first
                }
            }
        }
        __syncthreads();
        sum = 0.0f;
        if (lane == 0) {
            // post-order evaluation of the same tree over the block sums
            int fl[16], fs[16], sp = 0, k = 0;
            float fv[16], ret = 0.0f;
            fl[0] = m; fs[0] = 0;
            while (sp >= 0) {
                const int len = fl[sp];
                if (len <= 128) {
                    ret = leaf[k++];
                    sp--;
                } else if (fs[sp] == 0) {
                    fs[sp] = 1;
                    ++sp; fl[sp] = np_half(len); fs[sp] = 0;
                    continue;
                } else if (fs[sp] == 1) {
                    fv[sp] = ret;
                    fs[sp] = 2;
                    const int n2 = np_half(len);
                    ++sp; fl[sp] = len - n2; fs[sp] = 0;
                    continue;
                } else {
                    ret = fv[sp] + ret;
                    sp--;
                }
                // deliver ret to the parent frame (handled at its next visit)
            }
            sum = ret;
        }
    }
    if (lane == 0) st[4 + (SQ ? npieces : 0) + blockIdx.x] = sum;
}

// (I - mean) / std in float32 (match_single.py:40-41), zero border (process_functional.py:13-19).
constexpr int ZN_PER = 8;   // padded pixels per thread of znorm_pad_kernel

// The std formed here (every block, from the second pass's piece sums: np_stat by its first wave) -- the
// launch of a separate statistics kernel saved; block 0 stores it in the scratch's std word.
__global__ __launch_bounds__(256) void znorm_pad_kernel(const uint8_t *__restrict__ img, int H, int W, int pad,
                                                        float *__restrict__ scratch, int sstride, int npieces,
                                                        float *__restrict__ out)
{
    const int Wp = W + 2 * pad;
    img += (size_t)blockIdx.y * H * W;      // batch: image blockIdx.y
    float *st = scratch + (size_t)blockIdx.y * sstride;
    out += (size_t)blockIdx.y * (H + 2 * pad) * Wp;
    __shared__ float sbuf[256];
    __shared__ float sstd;
    if (threadIdx.x < 64) {
        const float v = sqrtf(np_stat(st + 4 + npieces, npieces, (int64_t)H * W, sbuf, threadIdx.x));
        if (threadIdx.x == 0) {
            sstd = v;
            if (blockIdx.x == 0) st[1] = v;
        }
    }
    __syncthreads();
    const float mean = st[0], stdv = sstd;
    const int64_t np_ = (int64_t)(H + 2 * pad) * Wp;
#pragma unroll
    for (int k = 0; k < ZN_PER; k++) {   // ZN_PER pixels per thread: the block's statistics amortised
        const int64_t i = ((int64_t)blockIdx.x * ZN_PER + k) * blockDim.x + threadIdx.x;
        if (i >= np_) break;
        // the padded image has < 2^31 pixels (checked by sde_preprocess_u8_batch)
        const int ii = (int)i;
        const int y = ii / Wp - pad, x = ii % Wp - pad;
        float v = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) v = ((float)img[(size_t)y * W + x] - mean) / stdv;
        out[i] = v;
    }
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int64_t sde_preprocess_scratch_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return -1;
    const int64_t pieces = ((int64_t)H * W + NP_PIECE - 1) / NP_PIECE;
    return ((4 + 2 * pieces) * 4 + 255) / 256 * 256;
}

SDE_EXPORT int sde_preprocess_u8_batch(const uint8_t *imgs, int nimg, int H, int W, int pad, float *out_pad,
                                       void *scratch, void *stream)
{
    if (!imgs || !out_pad || !scratch || nimg <= 0 || nimg > 65535 || H <= 0 || W <= 0 || pad < 0) return SDE_ERR_ARG;
    const int64_t n = (int64_t)(H + 2 * pad) * (W + 2 * pad);
    if (n >= ((int64_t)1 << 31)) return SDE_ERR_ARG;       // znorm_pad_kernel's 32-bit pixel index
    hipStream_t st = as_stream(stream);
    const int64_t npix = (int64_t)H * W;
    const int pieces = (int)((npix + NP_PIECE - 1) / NP_PIECE);
    const int sstride = (int)(sde_preprocess_scratch_bytes(H, W) / 4);
    float *sc = reinterpret_cast<float *>(scratch);
    np_piece_kernel<false><<<dim3(pieces, nimg), 64, 0, st>>>(imgs, npix, sstride, sc);
    np_piece_kernel<true><<<dim3(pieces, nimg), 64, 0, st>>>(imgs, npix, sstride, sc);
    znorm_pad_kernel<<<dim3((unsigned)cdiv(n, 256 * ZN_PER), nimg), 256, 0, st>>>(imgs, H, W, pad, sc, sstride, pieces,
                                                                                  out_pad);
    return launch_status();
}

SDE_EXPORT int sde_preprocess_u8(const uint8_t *img, int H, int W, int pad, float *out_pad, void *scratch,
                                 void *stream)
{
    return sde_preprocess_u8_batch(img, 1, H, W, pad, out_pad, scratch, stream);
}
