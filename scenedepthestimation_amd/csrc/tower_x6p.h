// tower_x6p.h -- conv64_x6p_kernel (SDE_TOWER_BF16X6; SDE_TOWER_F16X3 | SDE_TOWER_MFMA32) and what it alone uses.
//
// bf16x6: fp32-accurate conv on the bf16 MFMA (v_mfma_f32_32x32x16_bf16).
// Every fp32 operand is split exactly into three bf16 parts, x = x0 + x1 + x2
// (RNE; each residual is exact in f32), and the six partial products with
// i + j <= 2 are accumulated in fp32 (the three dropped ones are < 2^-23 |ab|,
// below one fp32 rounding of the product).  16x the fp32 MFMA rate / 6 terms =
// 2.67x the fp32 matrix peak at fp32-level error.
//
// conv64_x6p_kernel: persistent, one 512-thread workgroup per CU walking 16 x 32
// output tiles, warp-specialised:
// * waves 0-3 (one per SIMD) only issue MFMAs.  Wave w owns output channels
//   32*(w&1)..+31 and output rows 8*(w>>1)..+7 of the tile: 8 accumulators,
//   48 MFMAs per tap.  Weights never touch LDS: they are pre-arranged on the
//   host in A-fragment order [mtile][cblock][tap][part][lane][8] and read
//   straight into VGPRs one tap ahead (L2-resident, 221 KB per layer).
// * waves 4-7 (the "stagers") stream the input: the contraction is cut into
//   16-channel blocks (c-blocks); for one c-block the 18 x 34 input pixels are
//   loaded, split ONCE into bf16 parts and written to LDS as six planes (3 parts
//   x 2 channel halves, 8 bf16 per pixel) so that a B fragment is one contiguous,
//   conflict-free 1-KB ds_read_b128.  Two stage buffers: the stagers fill c-block
//   k+1 (or the next tile's first) while the MFMA waves consume c-block k; one
//   workgroup barrier per c-block.  Keeping the long-latency HBM loads in other
//   waves keeps them out of the MFMA waves' in-order vmcnt.
// Inter-layer activations use a c-block-major layout [4][h][w][16] (IN_CB /
// OUT_CB) so a stage reads contiguous 64-B pixel runs; the last layer writes the
// reference's [h][w][64].
//
// F16 (SDE_TOWER_F16X3): the same kernel with every operand split into TWO fp16
// parts after a power-of-two scaling, x*2^s = h + l (h = fp16(x*2^s), l =
// fp16(x*2^s - h), the residual exact in f32), and the three partial products
// h*h' + h*l' + l*h' on v_mfma_f32_32x32x16_f16.  fp16's 11-bit significand
// makes two parts carry 22 bits: the dropped l*l' term is < 2^-22 |ab| and each
// part's rounding 2^-23 relative -- the error of a few fp32 roundings per
// product, at half the MFMAs of bf16x6.  The scalings keep the parts in fp16's
// normal range without any chance of overflow:
// * weights: 2^tau per layer from the host (max |w| * 2^tau in [2^14, 2^15));
// * activations: 2^sigma per launch from a device word holding an upper bound
//   of |input| (the previous layer's epilogue atomically maxes its ReLU outputs
//   into it; for layer 2 the word holds max |image| and the kernel bounds conv1's
//   output by max|image| * max_n sum_t |w1[t][n]| + max |b1|), so that
//   bound * 2^sigma lies in [2^14, 2^15) < 65504.  Values far below the bound
//   lose relative precision only as fp16 subnormals do: absolute error
//   <= 2^-25 * 2^-sigma, i.e. <= 2^-40 of the layer's largest input.
// The epilogue multiplies the accumulators by 2^-(tau+sigma) (exact).
#pragma once
#include "tower_common.h"

namespace sde {

__device__ __forceinline__ void split3(float x, __bf16 &h, __bf16 &m, __bf16 &l)
{
    h = (__bf16)x;
    const float r1 = x - (float)h;
    m = (__bf16)r1;
    const float r2 = r1 - (float)m;
    l = (__bf16)r2;
}

constexpr int XP_PLANE = XP_NPIX * 16;            // bytes of one (part, channel-half) plane
constexpr int XP_STAGE = 6 * XP_PLANE;            // one c-block stage: 58,752 B
// MFMA wave mapping: each wave owns XP_WROWS output rows x both M-tiles (a pixel's 64 channels in one
// wave, as the last layer's L2 norm wants): 8 accumulators.  (One M-tile of 8 rows per wave was
// measured for the first and middle layers and not kept.)
constexpr int XP_WROWS = 4, XP_MW = 2;
constexpr int XP_ACC = XP_MW * XP_WROWS;          // accumulators per MFMA wave
#define XP_AL(F16) ((F16) ? 2 : 1)                // A fragments requested this many taps ahead
// two stages | FIRST: one image window per stager wave
constexpr size_t XP_BIAS_OFF = (size_t)2 * XP_STAGE + 4 * XP_WIN * sizeof(float);
constexpr size_t XP_SMEM = XP_BIAS_OFF + NF * sizeof(float);     // + the layer's 64 biases

// Split 4 channels and store them into the stage's six planes.
__device__ __forceinline__ void xp_put(char *sb, int u, float4 v)
{
    const int px = u >> 2, chunk = u & 3;
    bf16x4 p0, p1, p2;
    const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        __bf16 a, b, c;
        split3(xs[e], a, b, c);
        p0[e] = a; p1[e] = b; p2[e] = c;
    }
    char *dst = sb + (chunk >> 1) * XP_PLANE + px * 16 + (chunk & 1) * 8;
    *reinterpret_cast<uint2 *>(dst) = __builtin_bit_cast(uint2, p0);
    *reinterpret_cast<uint2 *>(dst + 2 * XP_PLANE) = __builtin_bit_cast(uint2, p1);
    *reinterpret_cast<uint2 *>(dst + 4 * XP_PLANE) = __builtin_bit_cast(uint2, p2);
}

// F16: scale by 2^sigma (s), split into two fp16 parts, store planes (part, channel half).
__device__ __forceinline__ void xp_put16(char *sb, int u, float4 v, float s)
{
    const int px = u >> 2, chunk = u & 3;
    f16x4 p0, p1;
    const float xs[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const _Float16 h = (_Float16)xs[e];
        p0[e] = h;
        p1[e] = (_Float16)(xs[e] - (float)h);
    }
    char *dst = sb + (chunk >> 1) * XP_PLANE + px * 16 + (chunk & 1) * 8;
    *reinterpret_cast<uint2 *>(dst) = __builtin_bit_cast(uint2, p0);
    *reinterpret_cast<uint2 *>(dst + 2 * XP_PLANE) = __builtin_bit_cast(uint2, p1);
}

template <bool F16>
__device__ __forceinline__ void xp_store(char *sb, int u, float4 v, float s)
{
    if (F16) xp_put16(sb, u, v, s);
    else xp_put(sb, u, v);
}

// One stage unit of activations (zero outside the input).
template <bool IN_CB>
__device__ __forceinline__ float4 xp_load(const float *__restrict__ in, int Hin, int Win, int ty0, int tx0, int cb,
                                          int u)
{
    const int px = u >> 2, chunk = u & 3;
    const int iy = px / XP_IX, ix = px - iy * XP_IX;
    const int y = ty0 + iy, x = tx0 + ix;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y < Hin && x < Win) {
        const float4 *in4 = reinterpret_cast<const float4 *>(in);
        const size_t i = IN_CB ? (((size_t)cb * Hin + y) * Win + x) * 4 + chunk : ((size_t)y * Win + x) * 16 + cb * 4 + chunk;
        v = in4[i];   // default cache policy: nontemporal loads / stores measured slower (the next layer
                      // re-reads the outputs from cache; round 2: layer 231 -> 234 / 242 / 250 us)
    }
    return v;
}

// conv1 (Cin = 1, 3x3, bias, ReLU) of the padded image for one stage unit; w = the 9 taps x
// 4 channels of the unit's chunk, b = their biases (a stager thread's chunk is fixed).
// The image values come from the stager wave's LDS window of the tile (win[iy][ix], 20 x 36).
__device__ __forceinline__ float4 xp_conv1(const float *win, int Hin, int Win, const float4 (&w)[9],
                                           float4 b, int ty0, int tx0, int u)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int px = u >> 2;
    const int iy = px / XP_IX, ix = px - iy * XP_IX;
    const int y = ty0 + iy, x = tx0 + ix;
    if (y < Hin - 2 && x < Win - 2) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        const float *wp = win + iy * XP_WX + ix;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const float im = wp[(t / 3) * XP_WX + t % 3];
            s0 = fmaf(im, w[t].x, s0);
            s1 = fmaf(im, w[t].y, s1);
            s2 = fmaf(im, w[t].z, s2);
            s3 = fmaf(im, w[t].w, s3);
        }
        v = make_float4(fmaxf(s0 + b.x, 0.f), fmaxf(s1 + b.y, 0.f), fmaxf(s2 + b.z, 0.f), fmaxf(s3 + b.w, 0.f));
    }
    return v;
}

// Stager waves: fill one stage with c-block cb of tile t.
template <bool FIRST, bool IN_CB, bool F16>
__device__ __forceinline__ void xp_fill(char *sb, const float *__restrict__ in, int Hin, int Win,
                                        const float *__restrict__ w1blob, int t, const XpBatch &bt, int cb, int st,
                                        float s, float *win)
{
    // opaque to the optimiser: stops loop-invariant code motion from hoisting the per-unit
    // address arithmetic of all units out of the tile loop (it would pin ~40 VGPRs that the
    // MFMA waves' accumulators need)
    asm volatile("" : "+v"(st));
    int img, ty0, tx0;
    xp_tile(bt, t, img, ty0, tx0);
    in += img * bt.in_stride;
    if (FIRST) {
        // the tile's image window is already in the wave's LDS window (xp_stager_loop)
        // the thread's chunk is st & 3 for every unit (XP_STAGERS is a multiple of 4)
        const int n0 = cb * 16 + (st & 3) * 4;
        const float4 b = *reinterpret_cast<const float4 *>(w1blob + n0);
        float4 w[9];
#pragma unroll
        for (int t = 0; t < 9; t++) w[t] = *reinterpret_cast<const float4 *>(w1blob + NF + t * NF + n0);
#pragma unroll 2
        for (int i = 0; i < XP_UPT; i++) {
            const int u = st + i * XP_STAGERS;
            if (u < XP_UNITS) xp_store<F16>(sb, u, xp_conv1(win, Hin, Win, w, b, ty0, tx0, u), s);
        }
    } else {
        // two batches of 5 loads in flight (the stagers have time; registers are shared
        // with the MFMA waves' allocation)
        constexpr int HB = (XP_UPT + 1) / 2;
#pragma unroll
        for (int b0 = 0; b0 < XP_UPT; b0 += HB) {
            float4 v[HB];
#pragma unroll
            for (int i = 0; i < HB; i++) {
                const int u = st + (b0 + i) * XP_STAGERS;
                v[i] = u < XP_UNITS ? xp_load<IN_CB>(in, Hin, Win, ty0, tx0, cb, u) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int i = 0; i < HB; i++) {
                const int u = st + (b0 + i) * XP_STAGERS;
                if (u < XP_UNITS) xp_store<F16>(sb, u, v[i], s);
            }
        }
    }
}

// Stager waves' own loop (non-FIRST layers): the pipeline of (tile, c-block) steps the MFMA
// waves consume, one stage ahead, with the HBM loads of step i+2 issued before step i+1's
// units are split and stored -- every load has a whole c-block period to land.  Runs the
// same barriers as the MFMA waves: one per c-block.
template <bool FIRST, bool IN_CB, bool F16>
__device__ __forceinline__ void xp_stager_loop(char *xsm, const float *__restrict__ in, int Hin, int Win,
                                               const XpBatch &bt, int st, const float *__restrict__ in_amax,
                                               const float *__restrict__ hdr, const float *__restrict__ w1blob,
                                               float *win)
{
    const int tile0 = blockIdx.x, gstride = gridDim.x;
    const int nsteps = ((bt.ntiles - 1 - tile0) / gstride + 1) * XP_NCB;
    if (FIRST) {
        // conv1 on the stagers: each step computed from the wave's LDS image window, one stage ahead
        int sc_img = -1;
        float s = 1.0f, unscale = 1.0f;
        // the image window of a tile, loaded into registers 3 steps before its first use (while
        // the previous tile's c-blocks are computed) and written to the wave's LDS window when
        // the tile's first c-block is filled -- the HBM latency stays off the stagers' path
        constexpr int WPL = (XP_WIN + 63) / 64;
        float wv[WPL];
        const int lane = st & 63;
        auto wload = [&](int t) {
            int img, ty0, tx0;
            xp_tile(bt, t, img, ty0, tx0);
            const float *src = in + img * bt.in_stride;
#pragma unroll
            for (int k = 0; k < WPL; k++) {
                const int idx = lane + 64 * k;
                const int iy = idx / XP_WX, ix = idx - iy * XP_WX;
                const int y = ty0 + iy, x = tx0 + ix;
                wv[k] = (idx < XP_WIN && y < Hin && x < Win) ? src[(size_t)y * Win + x] : 0.0f;
            }
        };
        auto fill = [&](int i) {
            const int t = tile0 + (i / XP_NCB) * gstride, im = t / bt.tiles_img, cb = i % XP_NCB;
            if (F16 && im != sc_img) {
                xp_scales(true, in_amax + im * bt.amax_stride, hdr, s, unscale);
                sc_img = im;
            }
            if (cb == 0) {   // a wave's LDS accesses complete in order: no barrier needed
#pragma unroll
                for (int k = 0; k < WPL; k++)
                    if (lane + 64 * k < XP_WIN) win[lane + 64 * k] = wv[k];
                __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the window's LDS writes have landed
                __builtin_amdgcn_wave_barrier();
            }
            xp_fill<true, false, F16>(xsm + (i & 1) * XP_STAGE, in, Hin, Win, w1blob, t, bt, cb, st, s, win);
            if (cb == 1 && t + gstride < bt.ntiles) wload(t + gstride);
        };
        wload(tile0);
        fill(0);
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < nsteps; i++) {
            if (i + 1 < nsteps) fill(i + 1);
            __syncthreads();
        }
        return;
    }
    auto load = [&](float4 (&v)[XP_UPT], int i) {
        const int t = tile0 + (i / XP_NCB) * gstride, cb = i % XP_NCB;
        int img, ty0, tx0;
        xp_tile(bt, t, img, ty0, tx0);
        const float *src = in + img * bt.in_stride;
#pragma unroll
        for (int k = 0; k < XP_UPT; k++) {
            const int u = st + k * XP_STAGERS;
            v[k] = u < XP_UNITS ? xp_load<IN_CB>(src, Hin, Win, ty0, tx0, cb, u) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    int sc_img = -1;
    float s = 1.0f, unscale = 1.0f;
    auto store = [&](const float4 (&v)[XP_UPT], int i) {
        const int im = (tile0 + (i / XP_NCB) * gstride) / bt.tiles_img;
        if (F16 && im != sc_img) {   // the tile's image changed: its bound word (tiles run image-major)
            xp_scales(false, in_amax + im * bt.amax_stride, hdr, s, unscale);
            sc_img = im;
        }
        char *sb = xsm + (i & 1) * XP_STAGE;
#pragma unroll
        for (int k = 0; k < XP_UPT; k++) {
            const int u = st + k * XP_STAGERS;
            if (u < XP_UNITS) xp_store<F16>(sb, u, v[k], s);
        }
    };
    auto sync_step = [&](int) {
        __syncthreads();
    };
    float4 ra[XP_UPT], rb[XP_UPT];
    load(ra, 0);
    store(ra, 0);
    if (nsteps > 1) load(ra, 1);
    __syncthreads();
    // step i: the MFMA waves consume stage i & 1; here step i+1 is stored and step i+2 loaded
#pragma unroll 1
    for (int i = 0; i < nsteps; i += 2) {
        if (i + 2 < nsteps) load(rb, i + 2);
        if (i + 1 < nsteps) store(ra, i + 1);
        sync_step(i);
        if (i + 1 >= nsteps) break;
        if (i + 3 < nsteps) load(ra, i + 3);
        if (i + 2 < nsteps) store(rb, i + 2);
        sync_step(i + 1);
    }
}

struct XpFrag {
    bf16x8 p[3];
};

// A fragments of one (c-block, tap): NP = 3 bf16 parts, or 2 fp16 parts (F16; the blob holds
// [mtile][cblock][tap][part NP][lane][8] for each arithmetic).  Unused parts stay untouched.
template <int NP>
__device__ __forceinline__ XpFrag xp_afrag(const uint4 *__restrict__ wf, int mt, int cb, int tap, int lane)
{
    const uint4 *src = wf + ((size_t)((mt * XP_NCB + cb) * 9 + tap) * NP) * 64 + lane;
    XpFrag f;
#pragma unroll
    for (int q = 0; q < NP; q++) f.p[q] = __builtin_bit_cast(bf16x8, src[q * 64]);
    return f;
}

typedef XpFrag XpB;   // B fragments (three parts; two for F16) of one row-step

template <int NP>
__device__ __forceinline__ XpB xp_bfrag(const char *b)
{
    XpB f;
#pragma unroll
    for (int q = 0; q < NP; q++)
        f.p[q] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(b + 2 * q * XP_PLANE));
    return f;
}

__device__ __forceinline__ floatx16 mfma_h(bf16x8 a, bf16x8 b, floatx16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// One c-block for one MFMA wave: 9 taps x 4 output rows = 36 row-steps; each step's B
// fragment (one input row segment, NP parts) feeds both M-tiles (output channels 0-31 and
// 32-63): 2 x 6 (bf16x6) or 2 x 3 (F16) MFMAs, small terms first, the leading product last.
// B fragments are read RD-1 row-steps ahead (a register ring); sched_barrier fences keep the
// scheduler from hoisting more, which bounds the live registers (8 accumulators = 128 of the
// 256 a wave may hold at 2 waves per SIMD).  A fragments (both M-tiles) are requested AL taps
// ahead.  Rows past the output edge run on zero-filled input and are discarded by the epilogue.
template <bool F16>
__device__ __forceinline__ void xp_cblock(floatx16 (&acc)[XP_ACC], XpFrag (&a)[XP_MW],
                                          XpFrag (&an)[XP_AL(F16)][XP_MW], const uint4 *__restrict__ wf, int mt0,
                                          int cb, int ncb, int lane, const char *sb)
{
    constexpr int NS = 9 * XP_WROWS;
    constexpr int NP = F16 ? 2 : 3;
    constexpr int AL = XP_AL(F16);
    constexpr int RD = 3;   // ring depth: fragments read RD-1 row-steps ahead
    XpB ring[RD];
    auto boff = [&](int s) { return ((s / XP_WROWS / 3 + s % XP_WROWS) * XP_IX + (s / XP_WROWS) % 3) * 16; };
#pragma unroll
    for (int k = 0; k < RD - 1; k++) ring[k] = xp_bfrag<NP>(sb + boff(k));
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int tap = s / XP_WROWS, r = s % XP_WROWS;
        if (r == 0 && tap > 0) {
            // a = A(tap); an[k] = A(tap + 1 + k); request A(tap + AL) (the next c-block's past tap 8)
#pragma unroll
            for (int m = 0; m < XP_MW; m++) {
                a[m] = an[0][m];
#pragma unroll
                for (int k = 0; k + 1 < AL; k++) an[k][m] = an[k + 1][m];
                const int t2 = tap + AL;
                an[AL - 1][m] = t2 < 9 ? xp_afrag<NP>(wf, mt0 + m, cb, t2, lane)
                                            : xp_afrag<NP>(wf, mt0 + m, ncb, t2 - 9, lane);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        const XpB &b = ring[s % RD];
#pragma unroll
        for (int m = 0; m < XP_MW; m++) {
            floatx16 &c = acc[m * XP_WROWS + r];
            if (F16) {
                c = mfma_h(a[m].p[1], b.p[0], c);
                c = mfma_h(a[m].p[0], b.p[1], c);
                c = mfma_h(a[m].p[0], b.p[0], c);
            } else {
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m].p[2], b.p[0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m].p[1], b.p[1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m].p[0], b.p[2], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m].p[1], b.p[0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m].p[0], b.p[1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m].p[0], b.p[0], c, 0, 0, 0);
            }
        }
        if (s + RD - 1 < NS) ring[(s + RD - 1) % RD] = xp_bfrag<NP>(sb + boff(s + RD - 1));
    }
    // hand the c-block boundary over: a = A(next c-block, tap 0)
#pragma unroll
    for (int m = 0; m < XP_MW; m++) {
        a[m] = an[0][m];
#pragma unroll
        for (int k = 0; k + 1 < AL; k++) an[k][m] = an[k + 1][m];
        an[AL - 1][m] = xp_afrag<NP>(wf, mt0 + m, ncb, AL, lane);
    }
}

// Tile epilogue of one MFMA wave (output rows XP_WROWS*g .., M-tiles mt0 ..): bias (+ReLU | L2-normalise),
// stores, and (F16, !LAST) the running maximum of the stored outputs for the image's bound word
// (one atomic per wave and image, xp_flush_amax).  unscale undoes the F16 power-of-two scalings.
template <bool LAST, bool OUT_CB, bool F16>
__device__ __forceinline__ void xp_epilogue(const floatx16 (&acc)[XP_ACC], int lane, int g, int mt0, int img,
                                            int ty0, int tx0, float unscale, const float4 *lbias4,
                                            float *__restrict__ out, int Hout, int Wout, const XpBatch &bt,
                                            uint16_t *__restrict__ ohi, uint16_t *__restrict__ olo,
                                            float *__restrict__ onrm, uint32_t &amax_run, int &amax_img,
                                            float *__restrict__ out_amax)
{
    // ---- epilogue (MFMA waves): bias (+ReLU | L2-normalise) ------------
    // lane holds pixel column j, channels m*32 + 8q + 4h + e in acc[m * XP_WROWS + r][4q + e]
    // opaque copies of the lane coordinates: keep the epilogue's bias loads and
    // addresses inside the loop (hoisted, they would pin registers for the whole kernel)
    int j = lane & 31, h = lane >> 5;
    asm volatile("" : "+v"(j), "+v"(h));
    const int x = tx0 + j;
    const bool xok = x < Wout;
    const int row0 = XP_WROWS * g;   // this wave's first row in the tile
    if (!LAST) {
        // F16: max of this lane's stored outputs of the tile, as float bits (outputs are >= +0
        // after the ReLU, so their bits order like their values: integer max3, no NaN quieting)
        uint32_t amax = 0u;
        float *const outi = out + img * bt.out_stride;
        // OUT_CB: [cblk][h][w][16] -> one descriptor per c-block plane, at the tile's first row;
        // else [h][w][64]
        const uint32_t vo = xok ? (uint32_t)(x * (OUT_CB ? 64 : 256) + 16 * h) : BUF_OOB;
        const size_t HW = (size_t)Hout * Wout;
        // Store-data registers stay untouched for XP_PIN stores ("store-data overwrite"):
        // each stored float4 is pinned live by an empty asm placed after the store XP_PIN - 1 stores
        // later, and the epilogue's last pins carry an s_nop, so no VALU writes a register a dwordx4
        // store still reads within XP_PIN instructions -- the store's issue and its data read are not
        // one event when MFMA waves contend for the VGPR read ports.  _isa_lint.py checks the built
        // code objects for this schedule.
        constexpr int NPIN = XP_MW * 2 * XP_WROWS * 2;
        u32x4 pin[NPIN];
#pragma unroll
        for (int m = 0; m < XP_MW; m++) {
            float4 b4[4];
#pragma unroll
            for (int q = 0; q < 4; q++) b4[q] = lbias4[((mt0 + m) * 32 + 8 * q + 4 * h) >> 2];
#pragma unroll
            for (int qh = 0; qh < 2; qh++) {
                const int cblk = 2 * (mt0 + m) + qh;
                const __amdgpu_buffer_rsrc_t rs = xp_rsrc(OUT_CB ? outi + ((size_t)cblk * HW + (size_t)ty0 * Wout) * 16
                                                                 : outi + (size_t)ty0 * Wout * NF);
#pragma unroll
                for (int r = 0; r < XP_WROWS; r++) {
                    const floatx16 &c = acc[m * XP_WROWS + r];
                    const bool rok = ty0 + row0 + r < Hout;   // wave-uniform
                    const uint32_t so = (uint32_t)((row0 + r) * Wout) * (OUT_CB ? 64u : 256u);
#pragma unroll
                    for (int ql = 0; ql < 2; ql++) {
                        const int q = 2 * qh + ql;
                        const float bq[4] = {b4[q].x, b4[q].y, b4[q].z, b4[q].w};
                        float o4[4];
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            o4[e] = fmaxf((F16 ? fmaf(c[4 * q + e], unscale, bq[e]) : c[4 * q + e] + bq[e]), 0.f);
                        const float4 o = make_float4(o4[0], o4[1], o4[2], o4[3]);
                        const int k = ((m * 2 + qh) * XP_WROWS + r) * 2 + ql;
                        pin[k] = __builtin_bit_cast(u32x4, o);
                        if (rok) {
                            if (F16) {   // the bound before the store: nothing writes o's registers after it
                                amax = max(amax, max(__float_as_uint(o.x), __float_as_uint(o.y)));
                                amax = max(amax, max(__float_as_uint(o.z), __float_as_uint(o.w)));
                            }
                            // byte offset within the descriptor: OUT_CB 32 (q & 1); else ch * 4
                            xp_st4(o, rs, vo + (OUT_CB ? 32u * ql : 4u * ((mt0 + m) * 32 + 8 * q)), so);
                        }
                        if (k >= XP_PIN - 1) asm volatile("" ::"v"(pin[k - (XP_PIN - 1)]));
                    }
                }
            }
        }
#pragma unroll
        for (int k = NPIN - (XP_PIN - 1); k + 1 < NPIN; k++) asm volatile("" ::"v"(pin[k]));
        asm volatile("s_nop 4" ::"v"(pin[NPIN - 1]));
        if (F16) {
            if (!xok) amax = 0u;   // lanes past the output edge stored nothing
            // one atomic per wave and image (flushed when the tiles move to the next
            // image and at the end): every workgroup maxes into the same word
            if (img != amax_img) {
                xp_flush_amax(amax_run, amax_img, lane, out_amax, bt.amax_stride);
                amax_img = img;
            }
            amax_run = max(amax_run, amax);
        }
    } else {
        // a pixel's 64 channels live in this wave (two lanes): wave-local L2 norm.
        // Outputs [h][w][64] (+ bf16 planes, norm bound), descriptors at the tile's first row.
        const size_t pix0 = (size_t)img * bt.pix_stride + (size_t)ty0 * Wout;
        const __amdgpu_buffer_rsrc_t rs = xp_rsrc(out + pix0 * NF);
        const uint32_t vo = xok ? (uint32_t)(x * 256 + 16 * h) : BUF_OOB;
#pragma unroll
        for (int r = 0; r < XP_WROWS; r++) {
            // biased value of channel m*32 + 8q + 4h + e (bias re-read from LDS per use: nothing
            // but the accumulators stays live across the row)
            int hr = h;
            asm volatile("" : "+v"(hr));   // per-row opaque copy: no CSE of bias reads across rows
            auto val4 = [&](int m, int q, float (&t)[4]) {
                const float4 bq4 = lbias4[(m * 32 + 8 * q + 4 * hr) >> 2];
                const float bq[4] = {bq4.x, bq4.y, bq4.z, bq4.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float cv = acc[m * XP_WROWS + r][4 * q + e];
                    t[e] = F16 ? fmaf(cv, unscale, bq[e]) : cv + bq[e];
                }
            };
            float ss = 0.0f;
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float t[4];
                    val4(m, q, t);
#pragma unroll
                    for (int e = 0; e < 4; e++) ss += t[e] * t[e];
                }
            ss += __shfl_xor(ss, 32, 64);
            const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
            float v[2][16];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float t[4];
                    val4(m, q, t);
#pragma unroll
                    for (int e = 0; e < 4; e++) v[m][4 * q + e] = t[e] * inv;
                }
            float s2 = 0.0f;
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int i = 0; i < 16; i++) s2 += v[m][i] * v[m][i];
            s2 += __shfl_xor(s2, 32, 64);
            if (ty0 + row0 + r < Hout) {   // wave-uniform
                const uint32_t rowp = (uint32_t)((row0 + r) * Wout);   // pixels from the tile's first row
#pragma unroll
                for (int m = 0; m < 2; m++)
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        xp_st4(make_float4(v[m][4 * q], v[m][4 * q + 1], v[m][4 * q + 2], v[m][4 * q + 3]),
                               rs, vo + 4u * (m * 32 + 8 * q), rowp * 256u);
                if (ohi) {
                    const __amdgpu_buffer_rsrc_t rh = xp_rsrc(ohi + pix0 * NF), rl = xp_rsrc(olo + pix0 * NF);
                    const uint32_t vo2 = xok ? (uint32_t)(x * 128 + 8 * h) : BUF_OOB;
#pragma unroll
                    for (int m = 0; m < 2; m++)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            bf16x4 hv, lv;
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const float xv = v[m][4 * q + e];
                                const __bf16 hh = (__bf16)xv;
                                hv[e] = hh;
                                lv[e] = (__bf16)(xv - (float)hh);
                            }
                            const uint32_t o2 = vo2 + 2u * (m * 32 + 8 * q);
                            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, hv), rh, o2, rowp * 128u, 0);
                            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, lv), rl, o2, rowp * 128u, 0);
                        }
                }
                // fp32 rounding bound of the 64-term sum
                if (onrm) {
                    const __amdgpu_buffer_rsrc_t rn = xp_rsrc(onrm + pix0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, sqrtf(s2) * 1.000004f), rn,
                                                          (xok && h == 0) ? (uint32_t)(x * 4) : BUF_OOB, rowp * 4u, 0);
                }
            }
        }
    }
}

template <bool FIRST, bool LAST, bool IN_CB, bool OUT_CB, bool F16>
__global__ __launch_bounds__(512) void conv64_x6p_kernel(const float *__restrict__ in, int Hin, int Win,
                                                         const float *__restrict__ w1blob,
                                                         const float *__restrict__ wkblob,
                                                         float *__restrict__ out, int Hout, int Wout,
                                                         uint16_t *__restrict__ ohi, uint16_t *__restrict__ olo,
                                                         float *__restrict__ onrm, XpBatch bt,
                                                         const float *__restrict__ in_amax, float *__restrict__ out_amax)
{
    extern __shared__ __attribute__((aligned(16))) char xsm[];
    // FIRST: the stager wave's image window
    float *win = reinterpret_cast<float *>(xsm + 2 * XP_STAGE) + ((threadIdx.x >> 6) & 3) * XP_WIN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const bool mfma_wave = wave < 4;            // waves 4..7 stage the input
    // MFMA wave: output rows XP_WROWS*g .. +XP_WROWS-1, M-tiles mt0 .. mt0+XP_MW-1
    // wave-uniform by construction; readfirstlane tells the compiler (SGPR row offsets, scalar branches)
    const int g = __builtin_amdgcn_readfirstlane(wave & 3);
    // always 0 (both M-tiles), but kept as an SGPR the compiler does not fold: with a literal 0 it forms the
    // weight and output addresses differently, and the kernel's schedule is the measured one
    const int mt0 = __builtin_amdgcn_readfirstlane(0);
    const int st = tid - XP_STAGERS;            // stager thread index (valid when !mfma_wave)
    constexpr int NP = F16 ? 2 : 3;
    constexpr int AL = XP_AL(F16);
    const float *bias = wkblob;
    const uint4 *wf = reinterpret_cast<const uint4 *>(wkblob + (F16 ? LK_F16 : NF + LK_W));
    // B fragment: plane (part, h), input row XP_WROWS*g + r + ky, pixel j + kx
    const int bbase = (lane >> 5) * XP_PLANE + ((XP_WROWS * g) * XP_IX + (lane & 31)) * 16;

    int tile = blockIdx.x;
    if (tile >= bt.ntiles) return;
    const float *hdr = wkblob + LK_F16 + LK_W;
    // F16 scalings of a tile (per image: each image has its own bound words; re-read only when
    // the tile's image changes -- tiles run image-major)
    int sc_img = -1;
    float sc_s = 1.0f, sc_u = 1.0f;
    auto scales = [&](int t, float &sc, float &usc) {
        if (F16) {
            const int im = t / bt.tiles_img;
            if (im != sc_img) {
                xp_scales(FIRST, in_amax + im * bt.amax_stride, hdr, sc_s, sc_u);
                sc_img = im;
            }
        }
        sc = sc_s;
        usc = sc_u;
    };
    if (!mfma_wave) {
        xp_stager_loop<FIRST, IN_CB, F16>(xsm, in, Hin, Win, bt, st, in_amax, hdr, w1blob, win);
        return;
    }
    float *lbias = reinterpret_cast<float *>(xsm + XP_BIAS_OFF);
    if (wave == 0) lbias[lane] = bias[lane];   // published by the first barrier below
    const float4 *lbias4 = reinterpret_cast<const float4 *>(lbias);
    XpFrag a[XP_MW], an[AL][XP_MW];
#pragma unroll
    for (int m = 0; m < XP_MW; m++) {
        a[m] = xp_afrag<NP>(wf, mt0 + m, 0, 0, lane);
#pragma unroll
        for (int k = 0; k < AL; k++) an[k][m] = xp_afrag<NP>(wf, mt0 + m, 0, 1 + k, lane);
    }
    __syncthreads();

    uint32_t amax_run = 0u;
    int amax_img = -1;
    int cur = 0;
    for (; tile < bt.ntiles; tile += gridDim.x) {
        int img, ty0, tx0;
        xp_tile(bt, tile, img, ty0, tx0);
        floatx16 acc[XP_ACC];
#pragma unroll
        for (int r = 0; r < XP_ACC; r++) acc[r] = floatx16{0};

#pragma unroll 1
        for (int cb = 0; cb < XP_NCB; cb++) {
            const int ncb = (cb + 1) & (XP_NCB - 1);
            xp_cblock<F16>(acc, a, an, wf, mt0, cb, ncb, lane, xsm + cur * XP_STAGE + bbase);
            if (cb == XP_NCB - 1) {
                float unscale = 1.0f;
                if (F16) {
                    float s_unused;
                    scales(tile, s_unused, unscale);
                }
                xp_epilogue<LAST, OUT_CB, F16>(acc, lane, g, mt0, img, ty0, tx0, unscale, lbias4, out, Hout, Wout, bt,
                                               ohi, olo, onrm, amax_run, amax_img, out_amax);
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    if (F16 && !LAST) xp_flush_amax(amax_run, amax_img, lane, out_amax, bt.amax_stride);
}

}  // namespace sde
