// tower_fp32.h -- SDE_TOWER_FP32, the reference arithmetic.  conv64_mfma_kernel: v_mfma_f32_32x32x2_f32 (exact f32 products, the 157 TF fp32 matrix rate).  512 threads,
// output tile 8 rows x 32 columns, wave w owns output row w (2 accumulators of 32x32); the (8+2) x (32+2) x 64
// input tile (87 KB) stays in LDS for all 9 taps, each tap's 64x64 weight slice is double-buffered; both LDS
// images XOR-swizzled at 8-B granularity.
#pragma once
#include "tower_common.h"

namespace sde {

constexpr int TW_TY = 8;                 // output rows per workgroup (one per wave)
constexpr int TW_TX = 32;                // output cols per workgroup (MFMA N)
constexpr int TW_IY = TW_TY + 2;         // input tile rows
constexpr int TW_IX = TW_TX + 2;         // input tile cols
constexpr int TW_NPIX = TW_IY * TW_IX;   // 340
constexpr size_t TW_SMEM = (size_t)(TW_NPIX * 32 + 2 * NF * 32) * sizeof(float2);

// float2 slot of channel pair `pair` (0..31) of pixel/row `p` in a swizzled 64-float row
__device__ __forceinline__ int pslot(int p, int pair) { return p * 32 + (pair ^ (p & 31)); }

// write channels 4q..4q+3 of row p (a float4) into the swizzled image
__device__ __forceinline__ void put4(float2 *img, int p, int q, float4 v)
{
    const int x = p & 31;
    const int unit = q ^ (x >> 1);
    float4 w = (x & 1) ? make_float4(v.z, v.w, v.x, v.y) : v;
    *reinterpret_cast<float4 *>(img + p * 32 + 2 * unit) = w;
}

// Load the 64x64 weight slice of one tap into registers (16 KB / 512 threads = 2 float4).
__device__ __forceinline__ void load_tap(const float *__restrict__ wk, int tap, float4 (&r)[2])
{
    const float4 *src = reinterpret_cast<const float4 *>(wk + (size_t)tap * NF * NF);
#pragma unroll
    for (int i = 0; i < 2; i++) r[i] = src[threadIdx.x + i * 512];
}

__device__ __forceinline__ void store_tap(float2 *wt, const float4 (&r)[2])
{
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int idx = threadIdx.x + i * 512;   // float4 index: n = idx / 16, q = idx % 16
        put4(wt, idx >> 4, idx & 15, r[i]);
    }
}

// Last-layer extras for the certified cost volume (see cv_tile.h):
// bf16 hi/lo split planes of the output features (x = hi + lo + r, RNE) and
// an upper bound of each pixel's L2 norm.  A lane holds channels
// mt*32 + 8g + 4h + e (e = 0..3) of its pixel in v[mt][4g + e].
__device__ __forceinline__ void emit_split(const float (&v)[2][16], int h, size_t pix, uint16_t *ohi, uint16_t *olo)
{
    typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            bf4 hv, lv;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float x = v[mt][4 * g + e];
                const __bf16 hh = (__bf16)x;
                hv[e] = hh;
                lv[e] = (__bf16)(x - (float)hh);
            }
            const size_t o = pix * NF + mt * 32 + 8 * g + 4 * h;
            *reinterpret_cast<uint2 *>(ohi + o) = __builtin_bit_cast(uint2, hv);
            *reinterpret_cast<uint2 *>(olo + o) = __builtin_bit_cast(uint2, lv);
        }
}

__device__ __forceinline__ void emit_norm(const float (&v)[2][16], int h, size_t pix, float *onrm)
{
    float ss = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) ss += v[0][r] * v[0][r] + v[1][r] * v[1][r];
    ss += __shfl_xor(ss, 32, 64);
    if (h == 0 && pix != (size_t)-1) onrm[pix] = sqrtf(ss) * 1.000004f;   // fp32 rounding bound (64 terms)
}

// FIRST: the input tile is conv1 (Cin = 1) of the padded image, computed here.
// LAST : no ReLU, L2-normalise over the 64 channels before the store.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(512) void conv64_mfma_kernel(const float *__restrict__ in, int Hin, int Win,
                                                          const float *__restrict__ w1blob,
                                                          const float *__restrict__ wkblob,
                                                          float *__restrict__ out, int Hout, int Wout,
                                                          uint16_t *__restrict__ ohi, uint16_t *__restrict__ olo,
                                                          float *__restrict__ onrm)
{
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float2 *tile = smem;                          // TW_NPIX rows x 32 pairs
    float2 *wt0 = smem + TW_NPIX * 32;            // 64 rows x 32 pairs
    float2 *wt1 = wt0 + NF * 32;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tx0 = blockIdx.x * TW_TX;
    const int ty0 = blockIdx.y * TW_TY;
    const float *bias = wkblob;
    const float *wk = wkblob + NF;

    float4 wreg[2];
    load_tap(wk, 0, wreg);

    // ---- input tile -> LDS ------------------------------------------------
    if (!FIRST) {
        // Hin x Win x 64 activations; tile pixel (iy, ix) = in[ty0+iy][tx0+ix]
        for (int idx = tid; idx < TW_NPIX * 16; idx += 512) {
            const int p = idx >> 4, q = idx & 15;
            const int iy = ty0 + p / TW_IX, ix = tx0 + p % TW_IX;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (iy < Hin && ix < Win) v = reinterpret_cast<const float4 *>(in + ((size_t)iy * Win + ix) * NF)[q];
            put4(tile, p, q, v);
        }
    } else {
        // `in` is the padded image (Hin x Win floats); conv1 output has (Hin-2) x (Win-2)
        // pixels.  Tile pixel (iy, ix) = relu(b1 + sum_tap img[ty0+iy+dy][tx0+ix+dx] * w1[tap][n]).
        const float *b1 = w1blob;
        const float *w1 = w1blob + NF;
        const int H1 = Hin - 2, W1 = Win - 2;
        for (int idx = tid; idx < TW_NPIX * 16; idx += 512) {
            const int p = idx >> 4, q = idx & 15;
            const int iy = ty0 + p / TW_IX, ix = tx0 + p % TW_IX;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (iy < H1 && ix < W1) {
                float im[9];
#pragma unroll
                for (int t = 0; t < 9; t++) im[t] = in[(size_t)(iy + t / 3) * Win + ix + t % 3];
                float a[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int n = 4 * q + j;
                    float s = 0.0f;
#pragma unroll
                    for (int t = 0; t < 9; t++) s = fmaf(im[t], w1[t * NF + n], s);
                    s += b1[n];
                    a[j] = s > 0.0f ? s : 0.0f;
                }
                v = make_float4(a[0], a[1], a[2], a[3]);
            }
            put4(tile, p, q, v);
        }
    }
    store_tap(wt0, wreg);
    __syncthreads();

    // ---- 9 taps x 16 k-quads x (2 M-tiles x 2 k-steps) MFMAs ----------------
    floatx16 acc0 = {0}, acc1 = {0};
    const int j = lane & 31;        // output column within the tile (B col / A row)
    const int h = lane >> 5;        // k half: channels 2h, 2h+1 of each k-quad
#pragma unroll 1
    for (int tap = 0; tap < 9; tap++) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        float2 *wt = (tap & 1) ? wt1 : wt0;
        if (tap < 8) load_tap(wk, tap + 1, wreg);
        const int p = (wave + ky) * TW_IX + (j + kx);
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const float2 b = tile[pslot(p, 2 * t + h)];
            const float2 a0 = wt[pslot(j, 2 * t + h)];
            const float2 a1 = wt[pslot(j + 32, 2 * t + h)];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, acc1, 0, 0, 0);
        }
        if (tap < 8) store_tap((tap & 1) ? wt0 : wt1, wreg);
        __syncthreads();
    }

    // ---- epilogue: bias (+ReLU | L2-normalise), float4 stores ---------------
    // lane holds pixel column j, channels n = mt*32 + 8g + 4h + e in acc_mt[4g + e]
    float v[2][16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int n = 8 * (r >> 2) + 4 * h + (r & 3);
        v[0][r] = acc0[r] + bias[n];
        v[1][r] = acc1[r] + bias[32 + n];
    }
    if (!LAST) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            v[0][r] = v[0][r] > 0.0f ? v[0][r] : 0.0f;
            v[1][r] = v[1][r] > 0.0f ? v[1][r] : 0.0f;
        }
    } else {
        float ss = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) ss += v[0][r] * v[0][r] + v[1][r] * v[1][r];
        ss += __shfl_xor(ss, 32, 64);
        const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
#pragma unroll
        for (int r = 0; r < 16; r++) { v[0][r] *= inv; v[1][r] *= inv; }
    }
    const int oy = ty0 + wave, ox = tx0 + j;
    if (oy < Hout && ox < Wout) {
        const size_t pix = (size_t)oy * Wout + ox;
        float *dst = out + pix * NF;
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                *reinterpret_cast<float4 *>(dst + mt * 32 + 8 * g + 4 * h) =
                    make_float4(v[mt][4 * g], v[mt][4 * g + 1], v[mt][4 * g + 2], v[mt][4 * g + 3]);
        if (LAST && ohi) emit_split(v, h, pix, ohi, olo);
    }
    if (LAST && onrm) emit_norm(v, h, oy < Hout && ox < Wout ? (size_t)oy * Wout + ox : (size_t)-1, onrm);
}

}  // namespace sde
