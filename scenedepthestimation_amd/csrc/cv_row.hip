// cv_row.hip -- row-sweep certified fused cost volume + WTA (north-star kernel).
//
// Replaces (WHDY/SceneDepthEstimation) compute_cost_volume + WTA1,
// process_functional.py:48-73 + 96-113, fused: the disparity map is bit-identical
// to WTA1(compute_cost_volume(fl, fr, D)) (see cv_cert.h for the
// certificate).  Built with -fno-honor-nans -mno-amdgpu-ieee (see _build.py): the
// per-score max / median / compare run without NaN canonicalisation, so every
// decision that must survive non-finite input is taken on integer bit tests.
#include "cv_cert.h"
#include "unique.h"

#include <algorithm>
#include <type_traits>

namespace sde {

// ---------------------------------------------------------------------------
// Mapping (cv_wta_row2_kernel).
//
// One 512-thread workgroup per image row walks the row in 128-pixel superstrips.  Its eight
// waves have two roles:
//   * waves 0-3 compute.  Wave g owns the 32 left pixels [128 k + 32 g, +32) of superstrip k (one
//     MFMA N-tile): it splits them in registers from fp32 rows prefetched one superstrip ahead,
//     sweeps every 32-pixel right tile of its disparity band itself (12 MFMAs per tile pair), so a
//     pixel's best / runner-up / argmin never leave the wave (no cross-wave merge), and takes the
//     certificate's decision per pixel.
//   * waves 4-7 stage.  The right-feature window of a superstrip (128 + D - 1 pixels, in tiles)
//     lives in an LDS ring of hi / lo fp16 planes; advancing one superstrip retires 4 tiles and
//     admits 4, one per stager: its fp32 loads are issued a superstrip ahead, then split into the
//     planes of the tile's ring slot, with the tile's max squared pixel norm and non-finite flag as
//     whole-wave reductions (no atomics).  Every right pixel is read from HBM once per row, and
//     the kernel's only HBM input is the two fp32 feature maps (no pre-split pass).
// The ring holds the window plus 4 tiles (14 at D = 192, 112 KB): while the compute waves read
// window k, the stagers write window k+1's four new tiles into the slots of the tiles superstrip
// k-1 retired, so one barrier per superstrip orders both directions.  Tiles left of the image are
// zero-filled, so an invalid voxel (x < d) scores exactly +0 = -(-0.0), like the CPU path.
//
// Per pixel, the certificate of cv_cert.h with the bound below: if the
// best fast score beats the runner-up by more than 2 eps, the fast argmax is the exact first
// minimum, and its exact cost is recomputed from the fp32 rows (L2-resident) when requested; every
// other pixel goes to the fix-up list.  Outputs are bit-identical to the exact kernel.
//
// Right view (MIRROR): disp_r = flipW(WTA1(compute_cost_volume(flipW(fr), flipW(fl), D))), i.e. for right pixel
// x' the first minimum over d of cost(x' + d, d) = -(0 + fl[x' + d] . fr[x']), voxels with x' + d >= W the -0.0
// fill.  The kernel runs the sweep above unchanged in mirrored coordinates xm = W - 1 - x: the owning pixels come
// from fr, the staged ring from fl, and "x" in the text above (tiles, band bounds Ta / Tb, score modes, `none`,
// the certificate) is xm.  Only the places that turn a row coordinate into an address map it back (rw_col: the
// ring and owner loads, the winner's exact cost, the pixel index of the outputs, prev_min and the fix-up list,
// whose entries stay true pixel indices), so the partial tile and the partial superstrip of a row sit at the
// low-x end of the true row.  The products commute, so every score and exact cost has the left view's bits on
// the mirrored pair; the bound below is symmetric in its two operands (RW_K |a| |b| + RW_ABS (|a| + |b|)), so no
// constant changes.
// ---------------------------------------------------------------------------
// Arithmetic of the fast scores and their bound (the pre-split tile kernel of cv_tile.h uses bf16
// hi/lo instead): every operand is scaled by 2^RW_S (exact) and split into two fp16 parts, x*2^S =
// h + l + r; the three partial products run on v_mfma_f32_32x32x16_f16, the eight small-term MFMAs
// (l*h', h*l') of a tile before the four leading ones (h*h').  Bound per voxel (a = fl[x],
// b = fr[x-d], Cauchy-Schwarz as in cv_cert.h):
//   split: |r| <= 2^-22 |x| 2^S (fp16 11-bit parts) and the dropped l*l' <= 2^-22 |ab| 2^2S
//          -> 3.001 * 2^-22 * sum|ab|                                         (7.2e-7)
//   accumulation, the conservative per-add model of cv_cert.h (2^-23 of the running
//   sum per product): 128 small-term adds on partial sums <= 2.002 * 2^-11 sum|ab|, then 64
//   leading adds on partial sums <= 1.002 sum|ab|  -> (64 * 1.002 + 0.13) * 2^-23  (7.7e-6)
//   NumPy pairwise order of the exact cost: 10 * 2^-24                        (6.0e-7)
//   -> |s_fast - s_exact| <= RW_K * ||a|| ||b||, RW_K = 1.5e-5 (1.67x margin over 9.0e-6),
// plus 2^-30 (||a|| + ||b||) for parts that fall into fp16's subnormal range (absolute error
// 2^-25 per scaled element, 64 elements).  A pixel is certified only when its norm and the
// window's largest norm are below 2^(15-S) - 1: no part can overflow fp16.
constexpr int RW_S = 8;
constexpr float RW_SCALE = (float)(1 << RW_S);     // 2^RW_S
constexpr float RW_K = 1.5e-5f;
constexpr float RW_ABS = 9.3132257e-10f;           // 2^-30
constexpr float RW_NMAX = 127.0f;                  // norm limit: 127 * 2^8 < 65504
typedef _Float16 rw_f16x8 __attribute__((ext_vector_type(8)));

// the split of one operand (the definition the bound and the CPU model of the tests refer to)
__device__ __forceinline__ void rw_split(float x, _Float16 &h, _Float16 &l)
{
    const float xs = x * RW_SCALE;
    h = (_Float16)xs;
    l = (_Float16)(xs - (float)h);
}

// rw_split's parts of two scaled values x0, x1 (= x * RW_SCALE) at a time, packed (x0's part in the low half):
// hi by one packed convert of the pair, lo = f16(x 2^S - hi) by v_fma_mix{lo,hi} from it (x 2^S - hi is exact
// in fp32: the same bits)
__device__ __forceinline__ void rw_split2(float x0, float x1, uint32_t &hi, uint32_t &lo)
{
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 hh = {(_Float16)x0, (_Float16)x1};
    hi = __builtin_bit_cast(uint32_t, hh);
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=&v"(lo) : "v"(x0), "v"(hi));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(x1), "v"(hi));
}

constexpr int RW_T = 32;          // pixels per tile (= one MFMA N-tile of left pixels)

// the column of the true row that holds sweep coordinate x (0 <= x < W): x itself, W - 1 - x in the mirrored form
template <bool MIRROR>
__device__ __forceinline__ int rw_col(int x, int W)
{
    if constexpr (MIRROR) return W - 1 - x;
    else return x;
}

// one 16-B unit (pixel u>>4, channels 4(u&15)..+3) of ring tile T (zero outside the row)
template <bool MIRROR>
__device__ __forceinline__ float4 rw_load(const float *__restrict__ frrow, int W, int T, int u)
{
    const int xr = T * RW_T + (u >> 4);
    const bool ok = xr >= 0 && xr < W;
    const float4 v = reinterpret_cast<const float4 *>(frrow)[(size_t)rw_col<MIRROR>(ok ? xr : 0, W) * 16 + (u & 15)];
    return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int CTRL>
__device__ __forceinline__ float rw_dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

__device__ __forceinline__ bool rw_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

constexpr int R2_NX = 128;                 // left pixels per superstrip (4 compute waves x 32)
constexpr int R2_NEW = R2_NX / RW_T;       // tiles admitted per superstrip (4)
constexpr int R2_LEAD = 2;                 // scores issued before the next tile's first MFMA (2..8 measured)
// (the paired splits, the norm-based non-finite flags and the merge by permlane32 swaps were each measured against
// the plain form in round 5, DESIGN "Round 5 status")

// one stager lane's 8 units (pixel u >> 4, channels 4 (u & 15) ..) of right tile T: unit u = lane + 64 i
template <bool MIRROR>
__device__ __forceinline__ void r2_load(const float *__restrict__ frrow, int W, int T, int lane, float4 (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = rw_load<MIRROR>(frrow, W, T, lane + 64 * i);
}

// split a loaded tile into ring slot `slot`; its max squared pixel norm and non-finite flag
__device__ __forceinline__ void r2_store(uint4 *ring, unsigned *tmax, unsigned *tbad, int slot, int lane,
                                         const float4 (&v)[8])
{
    unsigned mx = 0u;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int u = lane + 64 * i, px = u >> 4, q = u & 15;
        char *base = reinterpret_cast<char *>(ring + slot * 512 + fx_slot(px, q >> 1)) + 8 * (q & 1);
        const float xs[4] = {v[i].x * RW_SCALE, v[i].y * RW_SCALE, v[i].z * RW_SCALE, v[i].w * RW_SCALE};
        uint32_t hw[2], lw[2];
#pragma unroll
        for (int e = 0; e < 2; e++) rw_split2(xs[2 * e], xs[2 * e + 1], hw[e], lw[e]);
        *reinterpret_cast<uint2 *>(base) = uint2{hw[0], hw[1]};
        *reinterpret_cast<uint2 *>(base + 256 * 16) = uint2{lw[0], lw[1]};
        // the pixel's squared norm: its 16 lanes are one DPP row and sum their squares without LDS
        // round trips -- lane ^ 1, lane ^ 2, then the other quad of the 8 and the other 8 of the row
        // by mirrors (the partial sums are uniform within each quad / 8 by then, so every add is
        // the xor-butterfly's add: the same bits)
        float ss = v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
        ss += rw_dpp<0xB1>(ss);
        ss += rw_dpp<0x4E>(ss);
        ss += rw_dpp<0x141>(ss);
        ss += rw_dpp<0x140>(ss);
        mx = max(mx, __float_as_uint(ss));          // non-negative: bit patterns order as unsigned
        // a non-finite channel makes the pixel's sum of squares non-finite: one test per pixel (the norm
        // bound then fails the certificate as well: NaN / inf bits order above every finite square)
        bad |= rw_nonfinite(ss);
    }
    // whole-wave maximum (every lane holds its rows' pixel norms) and any-non-finite
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
    const bool anybad = __ballot(bad) != 0;
    if (lane == 0) {
        tmax[slot] = mx;
        tbad[slot] = anybad ? 1u : 0u;
    }
}

// prev_min (chunked path, chunks after the first): the previous chunk's exact first-minimum cost per pixel.  A pixel
// whose every exact score here is provably below -prev_min (best fast score + eps, with a factor 2 for the add's
// rounding) has every cost above the previous chunk's minimum, so this chunk cannot win the in-order merge: it
// writes (+inf, -1) and skips the certificate and the fix-up.
// MIRROR: the right view (see the mapping above); fl / fr are the caller's maps in both forms.
// UNIQ: the uniqueness check (include/sde_unique.h) decided in the epilogue -- the sweep is the plain one.  Lane (j, h)'s
// chain tt holds d = dt + j - 4 h - 8 k2 - tt with dt moving by 32 per tile, i.e. one residue class of d modulo 8,
// (x - 4 h - tt) mod 8: the four chains of lane (j, 0) and the four of lane (j, 1) are the eight classes of pixel x,
// so the winner i and i - 1, i + 1 sit in three different chains and each chain's best score outside the three is
// its b2 if its ag is one of them and its b1 otherwise (only the value is used, so ties within a chain are
// harmless).  s2x, the maximum over the eight, is the fast score of the runner-up of the definition; the decision
// and its slack are at `eps` below.  prev_min is not used (one sweep only).
template <bool WANT_MIN, bool MIRROR, bool UNIQ = false>
__global__ __launch_bounds__(512) void cv_wta_row2_kernel(const float *__restrict__ fl, const float *__restrict__ fr,
                                                          int H, int W, int d0, int d1, int tlo0, int nw, int nt,
                                                          float *__restrict__ out_min, int32_t *__restrict__ out_arg,
                                                          float *__restrict__ out_disp, unsigned *__restrict__ counter,
                                                          int32_t *__restrict__ list, const float *__restrict__ prev_min,
                                                          float tau, uint8_t *__restrict__ out_rej)
{
    extern __shared__ __attribute__((aligned(16))) uint4 rsm2[];
    uint4 *ring = rsm2;                                             // [nt][2 planes][32 px][8 chunks]
    unsigned *tmax = reinterpret_cast<unsigned *>(ring + nt * 512);  // [nt] max squared pixel norm (f32 bits)
    unsigned *tbad = tmax + nt;                                     // [nt] any non-finite channel
    const int y = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const float *flrow = (MIRROR ? fr : fl) + (size_t)y * W * 64;   // the owning pixels' row
    const float *frrow = (MIRROR ? fl : fr) + (size_t)y * W * 64;   // the ring's row
    const size_t rowpix = (size_t)y * W;
    const int nss = (W + R2_NX - 1) / R2_NX;
    auto slot_of = [&](int T) { int r = T % nt; return r < 0 ? r + nt : r; };

    if (wave >= 4) {
        // ---------------- stagers ----------------
        const int sw = wave - 4;
        // window 0 (nw tiles, tile tlo0 + t by wave t % 4) and this wave's tile of window 1
        // (nw <= 14: at most 4 prologue tiles per stager, all loads in flight before the first store).
        // The batch loop runs one trip (PB = 4); written flat, the compiler schedules the kernel differently,
        // so it stays a loop until the schedule is re-measured.
        constexpr int PB = 4;                          // tiles per batch
        float4 nv[8];
#pragma unroll
        for (int b = 0; b < 4 / PB; b++) {
            float4 pv[PB][8];
#pragma unroll
            for (int i = 0; i < PB; i++)
                if (sw + 4 * (PB * b + i) < nw) r2_load<MIRROR>(frrow, W, tlo0 + sw + 4 * (PB * b + i), lane, pv[i]);
            if (b == 4 / PB - 1 && nss > 1) r2_load<MIRROR>(frrow, W, tlo0 + nw + sw, lane, nv);
#pragma unroll
            for (int i = 0; i < PB; i++)
                if (sw + 4 * (PB * b + i) < nw) r2_store(ring, tmax, tbad, slot_of(tlo0 + sw + 4 * (PB * b + i)), lane, pv[i]);
        }
        __syncthreads();
        for (int k = 0; k < nss; k++) {
            // window k+1's new tile (loaded a superstrip ago) into the slot superstrip k-1 retired,
            // then the load of window k+2's
            if (k + 1 < nss) {
                const int T = tlo0 + R2_NEW * (k + 1) + nw - R2_NEW + sw;
                r2_store(ring, tmax, tbad, slot_of(T), lane, nv);
                if (k + 2 < nss) r2_load<MIRROR>(frrow, W, T + R2_NEW, lane, nv);
            }
            __syncthreads();
        }
        return;
    }

    // ---------------- compute waves ----------------
    const int grp = wave & 3;                       // pixel group
    float4 lraw[8];
    auto load_left = [&](int kk) {
        const int xx = kk * R2_NX + RW_T * grp + j;
        const float4 *src =
            reinterpret_cast<const float4 *>(flrow) + (size_t)rw_col<MIRROR>(xx < W ? xx : 0, W) * 16 + 2 * h;
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++) { lraw[2 * s2] = src[4 * s2]; lraw[2 * s2 + 1] = src[4 * s2 + 1]; }
    };
    load_left(0);
    __syncthreads();

    for (int k = 0; k < nss; k++) {
        const int tlo = tlo0 + R2_NEW * k;
        const bool more = k + 1 < nss;
        const int xb = k * R2_NX + RW_T * grp;
        const int x = xb + j;
        const bool xok = x < W;
        float best = -__builtin_inff(), second = -__builtin_inff();
        float wcost = -0.0f;   // WANT_MIN: the winner's exact cost (computed before the barrier)
        float s2x = -__builtin_inff();   // UNIQ: the best fast score at |d - arg| >= 2
        int arg = -1;
        float nl = 0.0f;
        unsigned nmax2 = 0u, wbad = 0u;
        bool lbad = false;
        if (xb < W && xb + RW_T - 1 < d0) {
            // every pixel of the group is left of d0: no voxel of the band is in the image (the chunked path's
            // later chunks, disparity shards past the first); the certificate's `none` case writes (-0.0, d0)
            if (more) load_left(k + 1);
        } else if (xb < W) {   // wave-uniform
            rw_f16x8 bh[4], bl[4];
            float ssl = 0.0f;
            // the left split (the MFMAs' B fragments) and the pixel's squared norm
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) {
                const float4 a = lraw[2 * s2], b = lraw[2 * s2 + 1];
                const float v8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                uint32_t hw[4], lw[4];
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    rw_split2(v8[e] * RW_SCALE, v8[e + 1] * RW_SCALE, hw[e / 2], lw[e / 2]);
                    ssl += v8[e] * v8[e];
                    ssl += v8[e + 1] * v8[e + 1];
                }
                bh[s2] = __builtin_bit_cast(rw_f16x8, uint4{hw[0], hw[1], hw[2], hw[3]});
                bl[s2] = __builtin_bit_cast(rw_f16x8, uint4{lw[0], lw[1], lw[2], lw[3]});
            }
            // a non-finite channel makes the sum of squares non-finite (an overflowing sum of finite squares
            // is flagged too: that pixel goes to the exact fix-up, same outputs).  The other half's partial
            // sum by the LDS shuffle: with a permlane32 swap here the build's fix-up counts moved
            // (693 -> 709 at 512 x 2048, same maps) -- the swap's result in lanes 0-31 was not the other
            // half's sum in that schedule, so the norm bound would be wrong; not used
            ssl += __shfl_xor(ssl, 32, 64);
            lbad = rw_nonfinite(ssl);
            nl = sqrtf(ssl) * FX_NORM_UP;
            if (more) load_left(k + 1);

            float b1[4], b2[4];
            int ag[4];
#pragma unroll
            for (int t = 0; t < 4; t++) { b1[t] = -__builtin_inff(); b2[t] = -__builtin_inff(); ag[t] = -1; }
            const int Ta = (xb - d1 + 1 + RW_T * 4096) / RW_T - 4096;
            const int Tb = (xb + 31 - d0 + RW_T * 4096) / RW_T - 4096;
            const int T0 = max(Ta, tlo), T1 = min(Tb, tlo + nw - 1);
            int slot = slot_of(T0);
            {
                // software-pipelined sweep: tile i's 16 scores are interleaved with the 12 MFMAs of
                // tile i + 1 (after two scores that cover the fragment reads' LDS latency: one MFMA,
                // then the VALU of 1-2 scores, per gap -- the MFMA pipe runs while the scores issue).
                // Same scores, same order of score updates: the same outputs.
                // (every T in [T0, T1] is inside the band: Ta / Tb are its exact bounds)
                const int n = T1 - T0 + 1;
                // Fragments are read one step ahead: a tile's hi / lo A fragments (fh, fo) at the start of
                // the step that issues its MFMAs, the step that scores the tile before it.
                rw_f16x8 fh[4], fo[4];
                fx_floatx16 A[2];
                auto nxt = [&](int sl2) { return sl2 + 1 == nt ? 0 : sl2 + 1; };
                auto frag = [&](int sl2, rw_f16x8 (&ah)[4], rw_f16x8 (&al)[4]) {
                    const uint4 *tp = ring + sl2 * 512;
#pragma unroll
                    for (int s2 = 0; s2 < 4; s2++) {
                        const int sl = fx_slot(j, 2 * s2 + h);
                        ah[s2] = __builtin_bit_cast(rw_f16x8, tp[sl]);
                        al[s2] = __builtin_bit_cast(rw_f16x8, tp[256 + sl]);
                    }
                };
                // MFMA m (0..11) of a tile: the small terms first, then the leading products
                auto mfma = [&](int m, fx_floatx16 &acc, const rw_f16x8 (&ah)[4], const rw_f16x8 (&al)[4]) {
                    if (m == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[0], bh[0], fx_floatx16{0}, 0, 0, 0);
                    else if (m < 8) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16((m & 1) ? ah[m >> 1] : al[m >> 1],
                                                                                (m & 1) ? bl[m >> 1] : bh[m >> 1],
                                                                                acc, 0, 0, 0);
                    else acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m - 8], bh[m - 8], acc, 0, 0, 0);
                };
                // MODE 0: a full tile (every voxel in [d0, d1)); 1: only d < d1 can fail (d = dk - tt < d1 <=>
                // dk < d1 + tt: one compare against a per-tt scalar); 3: only d >= d0 can fail (dk >= d0 + tt);
                // 2: both
                auto score1 = [&](const fx_floatx16 &acc, int r, auto mode_c, const int (&dk)[4]) {
                    constexpr int MODE = decltype(mode_c)::value;
                    const int tt = r & 3;
                    const bool in = MODE == 0   ? true
                                    : MODE == 1 ? dk[r >> 2] < d1 + tt
                                    : MODE == 3 ? dk[r >> 2] >= d0 + tt
                                                : (dk[r >> 2] - tt) >= d0 && (dk[r >> 2] - tt) < d1;
                    const float sc = in ? acc[r] : -__builtin_inff();
                    const bool gt = sc > b1[tt];
                    ag[tt] = gt ? dk[r >> 2] : ag[tt];
                    b2[tt] = __builtin_amdgcn_fmed3f(b1[tt], b2[tt], sc);
                    b1[tt] = fmaxf(b1[tt], sc);
                };
                // scores of tile T (accumulators acc, ring slot sl2) interleaved with the MFMAs of the
                // next tile (slot nsl, its fragments read now) into accn; issue = false: the last tile, scores only
                auto step = [&](auto issue_c, int T, int sl2, const fx_floatx16 &acc, int nsl, fx_floatx16 &accn) {
                    constexpr bool issue = decltype(issue_c)::value;
                    if (issue) frag(nsl, fh, fo);
                    nmax2 = max(nmax2, tmax[sl2]);
                    wbad |= tbad[sl2];
                    const int dt = xb - RW_T * T;
                    const bool lowok = dt - 31 >= d0, highok = dt + 31 < d1;   // wave-uniform
                    const int dl = dt + j - 4 * h;
                    int dk[4];
#pragma unroll
                    for (int k2 = 0; k2 < 4; k2++) dk[k2] = dl - 8 * k2;
                    // R2_LEAD scores before the next tile's first MFMA (they cover its fragments' LDS reads), the
                    // other 16 - R2_LEAD spread over the 12 MFMA gaps
                    constexpr int LD = R2_LEAD, RS = 16 - R2_LEAD;
                    auto body = [&](auto mode_c) {
#pragma unroll
                        for (int r = 0; r < LD; r++) score1(acc, r, mode_c, dk);
#pragma unroll
                        for (int m = 0; m < 12; m++) {
                            if (issue) mfma(m, accn, fh, fo);
#pragma unroll
                            for (int r = LD + (RS * m) / 12; r < LD + (RS * (m + 1)) / 12; r++)
                                score1(acc, r, mode_c, dk);
                        }
                    };
                    if (lowok && highok) {
                        asm volatile("");
                        body(std::integral_constant<int, 0>{});
                    } else if (!WANT_MIN && lowok) {   // (WANT_MIN: the two extra bodies spill there)
                        body(std::integral_constant<int, 1>{});
                    } else if (!WANT_MIN && highok) {
                        body(std::integral_constant<int, 3>{});
                    } else {
                        body(std::integral_constant<int, 2>{});
                    }
                };
                if (n > 0) {
                    using yes = std::integral_constant<bool, true>;
                    using no = std::integral_constant<bool, false>;
                    int sa = slot;                              // slot of tile T0 + i2
                    frag(sa, fh, fo);
#pragma unroll
                    for (int m = 0; m < 12; m++) mfma(m, A[0], fh, fo);
                    int i2 = 0;
                    for (; i2 + 3 < n; i2 += 2) {              // two tiles per trip: static accumulator sets
                        const int sb = nxt(sa), sc2 = nxt(sb);
                        step(yes{}, T0 + i2, sa, A[0], sb, A[1]);
                        step(yes{}, T0 + i2 + 1, sb, A[1], sc2, A[0]);
                        sa = sc2;
                    }
                    // the last 1-3 tiles
                    const int sb = nxt(sa), sc2 = nxt(sb);
                    if (i2 + 2 < n) {
                        step(yes{}, T0 + i2, sa, A[0], sb, A[1]);
                        step(yes{}, T0 + i2 + 1, sb, A[1], sc2, A[0]);
                        step(no{}, T0 + i2 + 2, sc2, A[0], sc2, A[1]);
                    } else if (i2 + 1 < n) {
                        step(yes{}, T0 + i2, sa, A[0], sb, A[1]);
                        step(no{}, T0 + i2 + 1, sb, A[1], sb, A[0]);
                    } else {
                        step(no{}, T0 + i2, sa, A[0], sa, A[1]);
                    }
                }
            }
            // a chain that took a score holds d + t >= t >= 0; one that took none still holds -1
#pragma unroll
            for (int t = 0; t < 4; t++) ag[t] = ag[t] >= 0 ? ag[t] - t : -1;
            best = b1[0]; second = b2[0]; arg = ag[0];
#pragma unroll
            for (int t = 1; t < 4; t++) fx_merge(best, arg, second, b1[t], ag[t], b2[t]);
            {
                // lanes 0-31 (the ones that store) take the other half's triple by permlane32 swaps
                auto up = [](uint32_t v) { return __builtin_amdgcn_permlane32_swap(v, v, false, false)[1]; };
                const float bb = __uint_as_float(up(__float_as_uint(best))), ss2 = __uint_as_float(up(__float_as_uint(second)));
                const int aa = (int)up((uint32_t)arg);
                fx_merge(best, arg, second, bb, aa, ss2);
            }
            if constexpr (UNIQ) {
                // both halves take lane j's merged winner, then their four chains' best score outside its
                // neighbourhood (ag already holds disparities; an empty chain holds -1 and -inf twice); lanes 0-31
                // take the maximum over the eight
                const uint32_t lo_arg = __builtin_amdgcn_permlane32_swap((uint32_t)arg, (uint32_t)arg, false, false)[0];
                const int ai = h ? (int)lo_arg : arg;
#pragma unroll
                for (int t = 0; t < 4; t++)
                    s2x = fmaxf(s2x, (ag[t] - ai <= 1 && ai - ag[t] <= 1) ? b2[t] : b1[t]);
                const uint32_t sx = __float_as_uint(s2x);
                s2x = fmaxf(s2x, __uint_as_float(__builtin_amdgcn_permlane32_swap(sx, sx, false, false)[1]));
            }
            if constexpr (WANT_MIN) {
                // the winner's exact cost (used if the pixel certifies), by both lane halves and issued before the
                // barrier: lane (j, h) forms dot64_exact_global's partial sums acc[4h .. 4h+3] (channels 8m + 4h ..
                // 8m + 4h + 3 = float4 2m + h of each operand, all 16 loads in flight) and its half of the final tree,
                // ((acc0 + acc1) + (acc2 + acc3)) or ((acc4 + acc5) + (acc6 + acc7)); a permlane32 swap adds the
                // halves in that order: the same bits as that function's (cv_exact.h), in one round of loads
                const uint32_t lo_arg = __builtin_amdgcn_permlane32_swap((uint32_t)arg, (uint32_t)arg, false, false)[0];
                const int ab = h ? (int)lo_arg : arg;   // the upper half takes lane j's merged arg
                const int xr = x - ab;
                const bool ok = xok && ab >= 0 && xr >= 0;
                // (the two forms written out rather than through rw_col: the left form then compiles to the
                // instructions it had before the mirrored one existed)
                const float4 *la, *ra;
                if constexpr (MIRROR) {
                    la = reinterpret_cast<const float4 *>(flrow + (size_t)(W - 1 - (xok ? x : 0)) * 64) + h;
                    ra = reinterpret_cast<const float4 *>(frrow + (size_t)(W - 1 - (ok ? xr : 0)) * 64) + h;
                } else {
                    la = reinterpret_cast<const float4 *>(flrow + (size_t)(xok ? x : 0) * 64) + h;
                    ra = reinterpret_cast<const float4 *>(frrow + (size_t)(ok ? xr : 0) * 64) + h;
                }
                float4 lv[8], rv[8];
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    lv[m] = la[2 * m];
                    rv[m] = ra[2 * m];
                }
                float a4[4];
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const float p4[4] = {lv[m].x * rv[m].x, lv[m].y * rv[m].y, lv[m].z * rv[m].z, lv[m].w * rv[m].w};
#pragma unroll
                    for (int e = 0; e < 4; e++) a4[e] = m == 0 ? p4[e] : a4[e] + p4[e];
                }
                const float half = (a4[0] + a4[1]) + (a4[2] + a4[3]);
                const float other = __uint_as_float(
                    __builtin_amdgcn_permlane32_swap(__float_as_uint(half), __float_as_uint(half), false, false)[1]);
                wcost = -(0.0f + (half + other));   // lanes 0-31: (lower half) + (upper half)
            }
        }
        // window k+1's new tiles go into the slots superstrip k-1 read (not this window's): one
        // barrier per superstrip orders both directions
        __syncthreads();
        if (xb < W && h == 0 && xok) {
            // scores are scaled by 2^2S (exact): compare against the scaled bound
            const float nr = sqrtf(__uint_as_float(nmax2)) * FX_NORM_UP;
            const float eps = (RW_K * nl * nr + RW_ABS * (nl + nr) + FX_ABS) * (RW_SCALE * RW_SCALE);
            const size_t p = rowpix + rw_col<MIRROR>(x, W);   // the true pixel (outputs, prev_min, list)
            // x < d0: no voxel of the band is inside the image -- every cost is the -0.0 fill, so the scan's
            // first minimum is d0 whatever the features hold
            const bool none = x < d0;
            // certified only when every operand is finite and no fp16 part can overflow (then every score
            // and eps are finite too)
            const bool fin = !lbad && !wbad && nl < RW_NMAX && nr < RW_NMAX;
            // UNIQ.  With S = RW_SCALE^2 and c1, c2 the exact costs of the winner and the runner-up, the exact
            // margin is (c2 - c1) = (s1 - s2) / S over the exact scores; best is within eps of s1 and s2x (a maximum
            // over the same disparities of scores each within eps) within eps of s2, so Mt = best - s2x is within
            // 2 eps of S (c2 - c1).  Roundings: Mt and Mt - S tau in fp32 here, 2^-24 (2 Mt + S tau) in all; the
            // definition's m = fl(c2 - c1) is monotone in c2 - c1 and tau is a float, so m >= tau whenever
            // c2 - c1 >= tau, and m < tau whenever c2 - c1 <= tau (1 - 2^-23): another 2^-23 S tau.  The sum is
            // below 2^-22 (Mt + S tau); the slack takes 2^-21.  A pixel is decided here only if its winner
            // certifies and |Mt - S tau| exceeds 2 eps + slack; s2x = -inf (no d outside the neighbourhood, m =
            // +inf) and tau = 0 (m >= 0: c1 is the minimum) never reject.
            bool rej = false, unsure = false;
            if constexpr (UNIQ) {
                if (none) {
                    rej = tau > 0.0f && d1 - d0 >= 3;   // every cost is the fill: m = +0 (+inf below 3 disparities)
                } else if (tau > 0.0f && s2x != -__builtin_inff()) {
                    const float st = tau * (RW_SCALE * RW_SCALE), mt = best - s2x;
                    const float slack = 2.0f * eps + 4.7683716e-7f * (st + mt);   // 2^-21
                    rej = st - mt > slack;
                    unsure = !rej && !(mt - st > slack);
                }
            }
            if (!none && fin && WANT_MIN && prev_min && best + 2.0f * eps < -prev_min[p] * (RW_SCALE * RW_SCALE)) {
                out_min[p] = __builtin_inff();
                if (out_arg) out_arg[p] = -1;
            } else if (!(UNIQ && unsure) && (none || (fin && (best - second) > 2.0f * eps && arg >= 0))) {
                if (none) arg = d0;
                if (WANT_MIN) {
                    float cost = -0.0f;
                    if (x - arg >= 0) cost = wcost;
                    out_min[p] = cost;
                }
                if (out_arg) out_arg[p] = arg;
                if constexpr (UNIQ) {
                    if (out_disp) out_disp[p] = rej ? -1.0f : (float)arg;
                    if (out_rej) out_rej[p] = rej ? 1 : 0;
                } else {
                    if (out_disp) out_disp[p] = (float)arg;
                }
            } else {
                // near-ties and non-finite operands: the IEEE fix-up kernel's exact scan
                list[atomicAdd(counter, 1u)] = (int32_t)p;
            }
        }
    }
}

// Superstrip 0's window -- right pixels [-(d1 - 1), 127 - d0], first tile tlo0, nw tiles (floor division) --
// and the ring that holds a window plus the R2_NEW tiles being admitted, with its per-tile words
struct RowWindow {
    int tlo0, nw, nt;
    size_t smem;
};

static RowWindow row_window(int d0, int d1)
{
    auto fdiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    RowWindow w;
    w.tlo0 = fdiv(-(d1 - 1), RW_T);
    w.nw = fdiv(R2_NX - 1 - d0, RW_T) - w.tlo0 + 1;
    w.nt = w.nw + R2_NEW;
    w.smem = (size_t)w.nt * 512 * 16 + (size_t)w.nt * 8;
    return w;
}

// the stagers' prologue holds at most 4 tiles each (nw <= 14 + the window-1 tile); ring <= 18 tiles, 144 KB
bool row_cert_supported(int d0, int d1) { return row_window(d0, d1).nw <= 14; }

// mirror: the right view (outputs indexed by right pixel)
void launch_row_cert(const float *fl, const float *fr, int H, int W, int d0, int d1, float *out_min, int32_t *out_arg,
                     float *out_disp, unsigned *counter, int32_t *list, hipStream_t st, const float *prev_min,
                     bool mirror)
{
    constexpr size_t MAX = 150 * 1024;
    const RowWindow w = row_window(d0, d1);
    if (out_min && mirror)
        launch_lds_dyn<cv_wta_row2_kernel<true, true>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0, w.nw, w.nt,
                                                            out_min, out_arg, out_disp, counter, list, prev_min, 0.0f, nullptr);
    else if (out_min)
        launch_lds_dyn<cv_wta_row2_kernel<true, false>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0, w.nw, w.nt,
                                                             out_min, out_arg, out_disp, counter, list, prev_min, 0.0f, nullptr);
    else if (mirror)
        launch_lds_dyn<cv_wta_row2_kernel<false, true>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0, w.nw, w.nt,
                                                             nullptr, out_arg, out_disp, counter, list, nullptr, 0.0f, nullptr);
    else
        launch_lds_dyn<cv_wta_row2_kernel<false, false>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0, w.nw, w.nt,
                                                              nullptr, out_arg, out_disp, counter, list, nullptr, 0.0f, nullptr);
}

void launch_row_cert_unique(const float *fl, const float *fr, int H, int W, int d0, int d1, float tau, float *out_min,
                            int32_t *out_arg, float *out_disp, uint8_t *out_rej, unsigned *counter, int32_t *list,
                            hipStream_t st, bool mirror)
{
    constexpr size_t MAX = 150 * 1024;
    const RowWindow w = row_window(d0, d1);
    if (out_min && mirror)
        launch_lds_dyn<cv_wta_row2_kernel<true, true, true>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0, w.nw,
                                                                  w.nt, out_min, out_arg, out_disp, counter, list,
                                                                  nullptr, tau, out_rej);
    else if (out_min)
        launch_lds_dyn<cv_wta_row2_kernel<true, false, true>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0, w.nw,
                                                                   w.nt, out_min, out_arg, out_disp, counter, list,
                                                                   nullptr, tau, out_rej);
    else if (mirror)
        launch_lds_dyn<cv_wta_row2_kernel<false, true, true>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0, w.nw,
                                                                   w.nt, nullptr, out_arg, out_disp, counter, list,
                                                                   nullptr, tau, out_rej);
    else
        launch_lds_dyn<cv_wta_row2_kernel<false, false, true>, MAX>(H, 512, w.smem, st, fl, fr, H, W, d0, d1, w.tlo0,
                                                                    w.nw, w.nt, nullptr, out_arg, out_disp, counter, list,
                                                                    nullptr, tau, out_rej);
}

}  // namespace sde
