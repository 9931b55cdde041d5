// tower_common.h -- exactly what more than one tower kernel header (fp32, x6p, h16, h16q, wino), or a header
// and the dispatch (tower.hip), uses; whatever one header alone uses lives in that header.
#pragma once
#include "sde_common.h"
#include "tower_blob.h"

namespace sde {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int XP_TY = 16, XP_TX = 32;             // output tile
constexpr int XP_IY = XP_TY + 2, XP_IX = XP_TX + 2;
constexpr int XP_NPIX = XP_IY * XP_IX;            // 612 input pixels per tile
constexpr int XP_UNITS = XP_NPIX * 4;             // (pixel, 4-channel chunk) units per stage
constexpr int XP_STAGERS = 256;                   // threads of the stager waves
constexpr int XP_UPT = (XP_UNITS + XP_STAGERS - 1) / XP_STAGERS;   // units per stager thread (10)
constexpr int XP_WX = XP_IX + 2, XP_WIN = (XP_IY + 2) * XP_WX;   // FIRST: image window of a tile (20 x 36)
constexpr int XP_NCB = LK_NCB;                    // c-blocks per pixel
constexpr int WN_TY = 8, WN_TX = 16;              // outputs per pass of wino_kernel: its launches' tile

// Tiles of a launch over a batch of images of one size: tile t -> image t / tiles_img, then
// row-major 16 x 32 output tiles.  Strides are per image (floats; pixels for the split outputs;
// floats between the images' F16 bound-word arrays).
struct XpBatch {
    int tiles_x, tiles_img, ntiles;
    int64_t in_stride, out_stride, pix_stride;
    int amax_stride;
};

__device__ __forceinline__ void xp_tile(const XpBatch &bt, int t, int &img, int &ty0, int &tx0)
{
    img = t / bt.tiles_img;
    const int tl = t - img * bt.tiles_img;
    ty0 = (tl / bt.tiles_x) * XP_TY;
    tx0 = (tl % bt.tiles_x) * XP_TX;
}

// 2^sigma for a bound: bound * 2^sigma in [2^14, 2^15); a zero, subnormal or non-finite bound gives sigma = 14
__device__ __forceinline__ int xp_sigma(float bound)
{
    int e = 0;   // bound in [2^e, 2^(e+1))
    if (bound >= 1.17549435e-38f && bound <= 3.40282347e38f) e = (int)((__float_as_uint(bound) >> 23) & 255u) - 127;
    return min(max(14 - e, -100), 100);
}

// F16 scalings of one tile (tower_x6p.h, "F16"): s = 2^sigma for the stagers, unscale = 2^-(tau+sigma).
// hdr: the layer blob's F16 header {2^-tau, max_n sum_t |w1[t][n]|, max |b1|, 0}.
__device__ __forceinline__ void xp_scales(bool first, const float *__restrict__ in_amax, const float *__restrict__ hdr,
                                          float &s, float &unscale)
{
    const float m = *in_amax;
    const int sigma = xp_sigma(first ? fmaf(m, hdr[1], hdr[2]) : m);
    s = ldexpf(1.0f, sigma);
    unscale = ldexpf(hdr[0], -sigma);
}

// Split activations (SDE_TOWER_OUT_SPLIT / SDE_TOWER_IN_SPLIT): a layer writes its ReLU outputs already
// scaled and split into the two fp16 parts its reader stages, so the reader's stagers copy them to LDS
// with LDS-DMA and no arithmetic.  The writer cannot know the measured maximum of its outputs before it
// writes them, so its 2^sigma comes from an a-priori bound: |out| <= max|b| + L1 * bound(|input|) (hdr[4],
// hdr[5], rounded up on the host; x 1.001 covers the f16x3 error of the computed outputs) -- bound * 2^sigma
// in [2^14, 2^15), no fp16 overflow.  The bound is looser than the measured maximum by the layer's L1 gain
// only (the input term is the measured bound word), which costs nothing here: values far below the bound
// lose precision only as fp16 subnormals do, an absolute error <= 2^-25 * 2^-sigma = 2^-39 of the bound.
// The writer publishes 2^sigma at its bound word + XP_SCALE_WORD (per image); the reader's unscale is
// 2^-tau / 2^sigma (exact).  Layout of a split activation (per image): 16 planes [cblk32 2][part 2][q 4],
// each [h][w][8 fp16] (16 B per pixel): the same 256 B per pixel as the fp32 [h][w][64].
constexpr int XP_SCALE_WORD = 32;
__device__ __forceinline__ float xp_out_scale(bool first, const float *__restrict__ in_amax,
                                              const float *__restrict__ hdr)
{
    const float m = *in_amax;
    const float bin = first ? fmaf(m, hdr[1], hdr[2]) : m;
    return ldexpf(1.0f, xp_sigma(fmaf(bin, hdr[4], hdr[5]) * 1.001f));
}

// the writer's 2^sigma into out_amax[img * stride + XP_SCALE_WORD] for every image of the launch
// (workgroup 0, wave 0; every workgroup would compute the same value)
__device__ __forceinline__ void xp_publish_scale(bool first, const XpBatch &bt, const float *__restrict__ in_amax,
                                                 const float *__restrict__ hdr, float *__restrict__ out_amax)
{
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    const int nimg = bt.ntiles / bt.tiles_img;
    for (int im = threadIdx.x; im < nimg; im += 64)
        out_amax[im * bt.amax_stride + XP_SCALE_WORD] = xp_out_scale(first, in_amax + im * bt.amax_stride, hdr);
}

// Epilogue stores: buffer descriptors on a per-tile base (wave-uniform), 32-bit per-lane byte
// offsets with an SGPR row offset; a lane outside the output (x >= Wout) gets BUF_OOB, which the
// descriptor's range check drops -- no exec-mask branches, no 64-bit address math per store.
// (Descriptors with an exact record count, whose loads past it return zero: buf_rsrc(base, nrec).)
constexpr uint32_t XP_NREC = 0x40000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t xp_rsrc(const void *base) { return buf_rsrc(base, XP_NREC); }

__device__ __forceinline__ void xp_st4(float4 v, __amdgpu_buffer_rsrc_t r, uint32_t vo, uint32_t so)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, vo, so, 0);
}

// x (already scaled by 2^sigma) split exactly into two fp16 parts: hi = fp16(x) (v_cvt_pk_f16_f32), lo =
// fp16(x - hi) by v_fma_mix{lo,hi}_f16 straight from the packed hi half (x - hi is exact in fp32, so its one
// rounding gives the bits of (fp16)(x - (float)hi); 6 instructions per 4 values instead of 12)
__device__ __forceinline__ void xp_split16s(float4 x, u32x2 &hw, u32x2 &lw)
{
    const f16x2 h01 = {(_Float16)x.x, (_Float16)x.y}, h23 = {(_Float16)x.z, (_Float16)x.w};
    hw = u32x2{__builtin_bit_cast(uint32_t, h01), __builtin_bit_cast(uint32_t, h23)};
    uint32_t l01, l23;
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=&v"(l01) : "v"(x.x), "v"(hw.x));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l01) : "v"(x.y), "v"(hw.x));
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=&v"(l23) : "v"(x.z), "v"(hw.y));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l23) : "v"(x.w), "v"(hw.y));
    lw = u32x2{l01, l23};
}

// a lane pair (rows 2i, 2i + 1 of 16 lanes) trades halves: the even lane ends with both hi parts, the odd with both lo
__device__ __forceinline__ u32x4 xp_pair_parts(u32x2 hw, u32x2 lw)
{
#pragma unroll
    for (int w = 0; w < 2; w++) {
        const auto sw = __builtin_amdgcn_permlane16_swap(hw[w], lw[w], false, false);
        hw[w] = sw[0];
        lw[w] = sw[1];
    }
    return u32x4{hw.x, hw.y, lw.x, lw.y};
}

// the running maximum of a wave's stored outputs into the image's bound word: one atomic per wave and image
__device__ __forceinline__ void xp_flush_amax(uint32_t &amax_run, int &amax_img, int lane, float *out_amax,
                                              int amax_stride)
{
    if (amax_img < 0) return;
    uint32_t a = amax_run;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o, 64));
    if (lane == 0) atomicMax(reinterpret_cast<unsigned int *>(out_amax + amax_img * amax_stride), a);
    amax_run = 0u;
}

constexpr int XP_PIN = 4;   // a stored float4's registers are not rewritten before XP_PIN - 1 more stores issue

}  // namespace sde
