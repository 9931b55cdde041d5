// tower_h16s.h -- conv64_h16s_kernel: conv64_h16_kernel's f16x3 arithmetic (tower_h16.h) on 16 x 16 output tiles,
// with the tile outputs stored by the STAGER waves (instantiated in tower_h16s.hip; layers 3..L with fp32
// activations only: the split layouts, the split feature planes and layer 2 stay on conv64_h16_kernel -- layer
// 2's stagers compute conv1 and have no time left for the stores).
//
// Why: in conv64_h16_kernel the MFMA waves' epilogue is 13 % of their cycles with all four matrix cores idle,
// and its cost is the issue of its 32 dwordx4 stores per wave; the stager waves meanwhile
// wait at barriers more than half the time.  Here the MFMA waves only park their raw fp32 accumulators in an
// LDS hand-over buffer (16 ds_write_b128 per wave) and go on with the next tile; the stagers unscale, add the
// bias, ReLU (or L2-normalise) and store while the next tile's MFMAs run.  The hand-over buffer is 64 KB, which a
// 16 x 32 tile's two 78 KB stages leave no room for -- hence the 256-pixel tile (two 42 KB stages).
//
// Mapping: stages, B fragments and the A blob as in conv64_h16_kernel, but MFMA wave g owns 8 output rows
// (8 (g >> 1) ..) x 2 channel quarters (2 (g & 1) + qq) of the tile's one 16-pixel half: 16 accumulators.  It
// loads only its channel half's A fragments -- with every wave loading all four quarters (12 MFMAs per B
// fragment, as conv64_h16_kernel does) the A-fragment traffic per output doubles on the smaller tile and the
// c-block loop slows from 265 to 300 kcycles per layer-image -- so a B fragment feeds 6
// MFMAs and a tap is 8 B fragments.  Every accumulator takes the MFMAs of conv64_h16_kernel in its order
// (c-block 0 taps 0..8, c-block 1 taps 0..8; per tap lo*hi, hi*lo, hi*hi), and every output the same fmaf /
// fmaxf / L2-norm tree: the same bits.
//
// Barrier protocol (two barriers per tile, one per c-block step, as in conv64_h16_kernel; B(i) closes step i,
// tile t is steps 2t and 2t+1):
//   MFMA waves:  step 2t+1 ends with hand-over(t) written, then B(2t+1).
//   stagers:     between B(2t+1) and B(2t+2) -- their iteration 2t+2, after its staging stores and loads are
//                issued -- they read hand-over(t) into registers and store it; __syncthreads' lgkmcnt(0) has
//                the LDS reads complete before B(2t+2).
//   MFMA waves:  write hand-over(t+1) only after B(2t+2) (at the end of step 2t+3): after every read of (t).
//   A workgroup's last tile is drained after the loop (its hand-over was closed by the last barrier).
#pragma once
#ifndef SDE_TOWER_H16S_H   // also a named guard: a probe copy (SDE_H16S_HEADER) must empty tower_h16s.hip's include of this file
#define SDE_TOWER_H16S_H
#include "tower_h16.h"

namespace sde {

struct H16T16 {
    static constexpr int TY = 16, TX = 16, IY = TY + 2, IX = TX + 2, NPIX = IY * IX, UNITS = NPIX * 4;   // 324 input pixels
    static constexpr int UPT = (NPIX + XP_STAGERS / 4 - 1) / (XP_STAGERS / 4);   // 6: h16_unit covers 64 pixels per iteration
    static constexpr int PLANE = 5376, STAGE = 8 * PLANE;                        // 324 x 16 B rounded up to 256 B; 43,008 B
    // hand-over buffer: 64 blocks (tile row R, quarter q) of 1 KB = 64 lanes x 4 fp32
    static constexpr size_t HO_OFF = 2 * (size_t)STAGE, SMEM = HO_OFF + 65536;   // 151,552 B (the biases stay in registers)
    static constexpr bool HANDOFF = true;
    static_assert(PLANE >= NPIX * 16 && PLANE % 256 == 0, "plane size / bank alignment");
    static_assert(SMEM <= 163840, "LDS");
};

// A lane's 16-B slot in a hand-over block: it holds channels 16q + 4 k4 .. +3 of pixel j of the block's row.
// The MFMA waves write with lane = 16 k4 + j (ds_write_b128: 8 contiguous lanes, j in an aligned 8, cover 8
// slots distinct mod 8: every bank of the 128-B window once), the stagers read with lane = 4 j + k4
// (ds_read_b128: each 16-lane group is 4 pixels x 4 k4, slots distinct mod 16) -- both conflict-free -- and a
// stager wave's dwordx4 store of a block is then 1 KB contiguous in the c-block-major output.
__device__ __forceinline__ int h16s_slot(int j, int k4) { return (k4 * 16 + ((j + 4 * k4) & 15)) * 16; }

// One c-block of the 16 x 16 tile for one MFMA wave (8 rows x 2 quarters): 9 taps x 8 rows, each B fragment
// feeding the wave's two quarters (6 MFMAs), B ring of depth 3 as h16_cblock12.  acc[r * 2 + qq].  A ring of three
// taps (slot tap % 3; 9 taps per c-block, so every c-block starts in phase 0): a tap lasts only 48 MFMAs here, so
// tap s requests tap s + 2 into the slot tap s - 1 left; on entry the ring holds taps 0 and 1 of this c-block, on
// exit those of the next.  cbo / ncbo: byte offsets in the A blob of this and the next c-block, each plus the
// wave's channel half (H16_A_HF): a tap's fragments are then h16_afrag's half-tap 2 tap.
constexpr int H16_A_HF = XP_NCB * 9 * 2 * 64 * 16;   // bytes between the two channel halves (M-tiles) of the A blob
template <class T>
__device__ __forceinline__ void h16s_cblock(floatx4 (&acc)[16], H16A (&abuf)[3], __amdgpu_buffer_rsrc_t ra,
                                             uint32_t avoff, int cbo, int ncbo, const char *sb)
{
    constexpr int NT = 9, NB = NT * 8, BRD = H16_RD;
    static_assert(NB % BRD == 0 && NT % 3 == 0, "static ring slots");
    H16B ring[BRD];
#pragma unroll
    for (int k = 0; k < BRD - 1; k++) ring[k] = h16_bfrag_at<T>(sb, k >> 3, k & 7, 0);
#pragma unroll
    for (int s = 0; s < NT; s++) {
        abuf[(s + 2) % 3] = s + 2 < NT ? h16_afrag(ra, avoff, cbo, 2 * (s + 2)) : h16_afrag(ra, avoff, ncbo, 2 * (s + 2 - NT));
        const H16A &a = abuf[s % 3];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int b = s * 8 + r;
            __builtin_amdgcn_sched_barrier(0);
            const H16B &bf = ring[b % BRD];
            if (b + BRD - 1 < NB) {
                const int nb = b + BRD - 1;
                ring[nb % BRD] = h16_bfrag_at<T>(sb, nb >> 3, nb & 7, 0);
            }
#pragma unroll
            for (int qq = 0; qq < 2; qq++) {
                floatx4 &c = acc[r * 2 + qq];
                c = mfma16(a.f[1][qq], bf.hi, c);
                c = mfma16(a.f[0][qq], bf.lo, c);
                c = mfma16(a.f[0][qq], bf.hi, c);
            }
        }
    }
}

// What a wave that stores outputs carries from tile to tile: the image's unscale, the biases of the lane's 16
// channels (16q + 4 k4 + e), the running bound word.
struct H16sOut {
    int sc_img = -1, amax_img = -1;
    float unscale = 1.0f;
    uint32_t amax_run = 0u;
    float4 bias[4];
};

// Four output rows R0 .. R0+3 of tile (img, ty0, tx0) from one stager wave: get(r, q) = the raw accumulator of
// row R0 + r, quarter q whose 4 values are channels 16q + 4 k4 + e of pixel tx0 + j (lane = 4 j + k4: the 4 lanes
// of a pixel are neighbours).  h16_epilogue's arithmetic value by value:
// fmaf(acc, unscale, bias), then ReLU, the integer max into the bound word and the c-block-major (OUT_CB) or
// [h][w][64] store -- or (LAST) the L2 norm in h16_epilogue's summation tree (per lane the running sum over
// (q, e), then (p0 + p1) + (p2 + p3)) and the [h][w][64] features.  Stores as there: per-tile descriptors,
// interior tiles without range selects, stored registers pinned for XP_PIN stores; on edge tiles lanes AND rows
// outside the image take the offset BUF_OOB, so that no store sits behind a branch (the ISA lint reads the
// listing linearly: a store that ends a block must not be followed by another block's VALU writes).
template <class T, bool LAST, bool OUT_CB, typename GET>
__device__ __forceinline__ void h16s_rows_out(H16sOut &o, GET &&get, int lane, int j, int k4, int R0, int img, int ty0,
                                              int tx0, float *__restrict__ out, int Hout, int Wout, const XpBatch &bt,
                                              const float *__restrict__ in_amax, const float *__restrict__ hdr,
                                              float *__restrict__ out_amax)
{
    if (img != o.sc_img) {
        float s_unused;
        xp_scales(false, in_amax + img * bt.amax_stride, hdr, s_unused, o.unscale);
        o.sc_img = img;
    }
    const float unscale = o.unscale;
    asm volatile("" : "+v"(j), "+v"(k4));
    constexpr int NPIN = 16;
    u32x4 pin[NPIN];
    const int x = tx0 + j;
    if (!LAST) {
        uint32_t amax = 0u;
        float *const outi = out + img * bt.out_stride;
        const size_t HW = (size_t)Hout * Wout;
        auto body = [&](auto fullc) {
            constexpr bool FULL = decltype(fullc)::value;
            const bool xok = FULL || x < Wout;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float bq[4] = {o.bias[q].x, o.bias[q].y, o.bias[q].z, o.bias[q].w};
                const __amdgpu_buffer_rsrc_t rs = xp_rsrc(OUT_CB ? outi + ((size_t)q * HW + (size_t)ty0 * Wout) * 16
                                                                 : outi + (size_t)ty0 * Wout * NF);
                const uint32_t vo = xok ? (uint32_t)(OUT_CB ? x * 64 + 16 * k4 : x * 256 + 64 * q + 16 * k4) : BUF_OOB;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const bool rok = FULL || ty0 + R0 + r < Hout;   // wave-uniform
                    const uint32_t so = (uint32_t)((R0 + r) * Wout) * (OUT_CB ? 64u : 256u);
                    const floatx4 c = get(r, q);
                    float o4[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) o4[e] = fmaxf(fmaf(c[e], unscale, bq[e]), 0.f);
                    const float4 ov = make_float4(o4[0], o4[1], o4[2], o4[3]);
                    const int k = q * 4 + r;
                    pin[k] = __builtin_bit_cast(u32x4, ov);
                    // the bound before the store: nothing writes ov's registers after it
                    const uint32_t m = max(max(__float_as_uint(ov.x), __float_as_uint(ov.y)),
                                           max(__float_as_uint(ov.z), __float_as_uint(ov.w)));
                    amax = max(amax, rok && xok ? m : 0u);
                    xp_st4(ov, rs, rok ? vo : BUF_OOB, so);
                    asm volatile("s_nop 2" ::"v"(pin[k >= XP_PIN - 1 ? k - (XP_PIN - 1) : k]) : "memory");   // after each store: >= 9 wait states over XP_PIN stores
                }
            }
#pragma unroll
            for (int k = NPIN - (XP_PIN - 1); k + 1 < NPIN; k++) asm volatile("" ::"v"(pin[k]));
            asm volatile("s_nop 7\n\ts_nop 1" ::"v"(pin[NPIN - 1]) : "memory");
        };
        if (ty0 + T::TY <= Hout && tx0 + T::TX <= Wout) body(std::true_type{});
        else body(std::false_type{});
        // one atomic per wave and image (flushed when the tiles move to the next image and at the end)
        if (img != o.amax_img) {
            xp_flush_amax(o.amax_run, o.amax_img, lane, out_amax, bt.amax_stride);
            o.amax_img = img;
        }
        o.amax_run = max(o.amax_run, amax);
    } else {
        const size_t pix0 = (size_t)img * bt.pix_stride + (size_t)ty0 * Wout;
        const __amdgpu_buffer_rsrc_t rs = xp_rsrc(out + pix0 * NF);
        auto body = [&](auto fullc) {
            constexpr bool FULL = decltype(fullc)::value;
            const bool xok = FULL || x < Wout;
            const uint32_t vo = xok ? (uint32_t)(x * 256 + 16 * k4) : BUF_OOB;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool rok = FULL || ty0 + R0 + r < Hout;
                const uint32_t so = (uint32_t)((R0 + r) * Wout) * 256u;
                float t[4][4];
                float ss = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float bq[4] = {o.bias[q].x, o.bias[q].y, o.bias[q].z, o.bias[q].w};
                    const floatx4 c = get(r, q);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        t[q][e] = fmaf(c[e], unscale, bq[e]);
                        ss += t[q][e] * t[q][e];
                    }
                }
                ss += __shfl_xor(ss, 1, 64);   // p(k4) + p(k4 ^ 1), then + the other pair: h16_epilogue's tree
                ss += __shfl_xor(ss, 2, 64);
                const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float4 ov = make_float4(t[q][0] * inv, t[q][1] * inv, t[q][2] * inv, t[q][3] * inv);
                    const int k = r * 4 + q;
                    pin[k] = __builtin_bit_cast(u32x4, ov);
                    xp_st4(ov, rs, rok ? vo + 64u * q : BUF_OOB, so);
                    asm volatile("s_nop 2" ::"v"(pin[k >= XP_PIN - 1 ? k - (XP_PIN - 1) : k]) : "memory");   // after each store: >= 9 wait states over XP_PIN stores
                }
            }
#pragma unroll
            for (int k = NPIN - (XP_PIN - 1); k + 1 < NPIN; k++) asm volatile("" ::"v"(pin[k]));
            asm volatile("s_nop 7\n\ts_nop 1" ::"v"(pin[NPIN - 1]) : "memory");
        };
        if (ty0 + T::TY <= Hout && tx0 + T::TX <= Wout) body(std::true_type{});
        else body(std::false_type{});
    }
}

// Layers 3..L, f16x3, fp32 activations: IN_CB / OUT_CB c-block-major [cblk16][h][w][16] or [h][w][64]; LAST
// writes the L2-normalised [h][w][64] features.
template <bool LAST, bool IN_CB, bool OUT_CB>
__global__ __launch_bounds__(512) void conv64_h16s_kernel(const float *__restrict__ in, int Hin, int Win,
                                                          const float *__restrict__ wkblob, float *__restrict__ out,
                                                          int Hout, int Wout, XpBatch bt,
                                                          const float *__restrict__ in_amax, float *__restrict__ out_amax)
{
    using T = H16T16;
    extern __shared__ __attribute__((aligned(16))) char hsm[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    int tile = blockIdx.x;
    if (tile >= bt.ntiles) return;
    const float *hdr = wkblob + LK_F16 + LK_W;
    H16sOut os;
    if (wave >= 4) {
        // stager lane 4 j + k4; wave w drains tile rows 4w .. 4w+3
        const int w = __builtin_amdgcn_readfirstlane(wave - 4), j = lane >> 2, k4 = lane & 3;
        const char *hob = hsm + T::HO_OFF + h16s_slot(j, k4);
#pragma unroll
        for (int q = 0; q < 4; q++) os.bias[q] = reinterpret_cast<const float4 *>(wkblob)[4 * q + k4];
        auto drain = [&](int t) {
            int img, ty0, tx0;
            h16_tile<T>(bt, t, img, ty0, tx0);
            auto get = [&](int r, int q) { return *reinterpret_cast<const floatx4 *>(hob + ((4 * w + r) * 4 + q) * 1024); };
            h16s_rows_out<T, LAST, OUT_CB>(os, get, lane, j, k4, 4 * w, img, ty0, tx0, out, Hout, Wout, bt, in_amax, hdr,
                                           out_amax);
        };
        h16_stager_loop<T, IN_CB>(hsm, in, Hin, Win, bt, tid - XP_STAGERS, in_amax, hdr, drain);
        if (!LAST) xp_flush_amax(os.amax_run, os.amax_img, lane, out_amax, bt.amax_stride);
        return;
    }
    const int g = __builtin_amdgcn_readfirstlane(wave);
    const int ch = g & 1, rg = g >> 1;   // the wave's channel half and row group
    const __amdgpu_buffer_rsrc_t ra = xp_rsrc(wkblob + LK_F16);
    // the lane's A-fragment byte offset and B base, as in conv64_h16_kernel
    const uint32_t avoff = (uint32_t)((lane >> 5) * (9 * 2 * 64) + ((lane >> 4) & 1) * 32 + (lane & 15)) * 16u;
    const int bbase = (lane >> 4) * T::PLANE + ((8 * rg) * T::IX + (lane & 15)) * 16;
    // the wave's first hand-over block (row 8 rg, quarter 2 ch) at the lane's slot: lane = 16 k4 + j
    char *how = hsm + T::HO_OFF + ((8 * rg) * 4 + 2 * ch) * 1024 + h16s_slot(lane & 15, lane >> 4);
    const int cbo0 = ch * H16_A_HF, cbo1 = H16_A_CB + ch * H16_A_HF;
    H16A abuf[3];
    abuf[0] = h16_afrag(ra, avoff, cbo0, 0);
    abuf[1] = h16_afrag(ra, avoff, cbo0, 2);
    floatx4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    int cur = 0;
    for (; tile < bt.ntiles; tile += gridDim.x) {
        h16s_cblock<T>(acc, abuf, ra, avoff, cbo0, cbo1, hsm + cur * T::STAGE + bbase);
        __syncthreads();
        cur ^= 1;
        h16s_cblock<T>(acc, abuf, ra, avoff, cbo1, cbo0, hsm + cur * T::STAGE + bbase);
        // park the raw accumulators: acc[r * 2 + qq] -> block (row 8 rg + r, quarter 2 ch + qq)
#pragma unroll
        for (int i = 0; i < 16; i++) *reinterpret_cast<floatx4 *>(how + ((i >> 1) * 4 + (i & 1)) * 1024) = acc[i];
        // the parked accumulators have left the registers before these are zeroed for the next tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        cur ^= 1;
    }
}

}  // namespace sde

#endif  // SDE_TOWER_H16S_H
