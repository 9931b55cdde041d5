// cv_lr.h -- the L and R cost volumes in one row sweep (cvlr3_kernel, C = 64, [H,W,D]) and its LDS-DMA
// helpers.  Launched by sde_cost_volume (cv_volume.hip) only; the arithmetic is cv_exact.h's.
#pragma once

#include "cv_exact.h"

namespace sde {

// ---------------------------------------------------------------------------
// LDS-DMA helpers of the L/R volume sweep (cvlr3_kernel below): feature rows go from global memory
// straight into padded 272-B LDS rows, without passing through VGPRs.  A buffer descriptor per
// feature row makes out-of-image rows load zeros (cd_desc); one wave-instruction moves 1 KiB
// (cd_dma16); a unit is 32 padded rows = 8.5 instructions, lane s loading chunk s % 17 of row
// s / 17, chunk 16 being the pad (c3_unit); buf_rsrc is the descriptor of the volume
// stores, whose out-of-image rows are dropped by the range check; cd_barrier waits for the LDS
// counter only, so DMA and stores stay in flight across the barrier.
// ---------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int CD_RB = 272;                                // bytes per padded LDS row (17 chunks of 16 B)

__device__ __forceinline__ uint32_t cd_lds(const void *p)
{
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

typedef unsigned cd_u32x4 __attribute__((ext_vector_type(4)));
// raw buffer descriptor of `bytes` bytes at base (SGPRs): loads past the records return zeros
__device__ __forceinline__ cd_u32x4 cd_desc(const void *base, uint32_t bytes)
{
    const uintptr_t b = (uintptr_t)base;
    cd_u32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((uint32_t)b);
    r.y = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) & 0xffffu;
    r.z = __builtin_amdgcn_readfirstlane(bytes);
    r.w = 0x00020000u;
    return r;
}

// one LDS-DMA wave-instruction: 16 B per lane from byte offset voff of the buffer to lds_dst + 16 lane
__device__ __forceinline__ void cd_dma16(cd_u32x4 rs, uint32_t voff, uint32_t lds_dst)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rs), "s"(lds_dst)
                 : "memory");
}

__device__ __forceinline__ void cd_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------
// L and R volumes in one row sweep, two workgroups per CU (C = 64, [H,W,D]) -- the default.
//
// Round 2's cvlr_dma_kernel held the whole CU (155 KB of LDS, 8 waves in lock-step barrier phases):
// its dot loops stopped at every strip boundary while the CU waited (PMC: waves parked 37 % of their
// cycles, VALU busy ~45 %).  Here a 256-thread workgroup (4 waves, one per SIMD) needs 69 KB of
// LDS, so two independent workgroups share each CU and one's barrier phases and exposed loads
// overlap the other's dots.  Workgroup = (row y, 64-disparity chunk dc), 64-pixel strips; the
// exact NumPy-order arithmetic and the two-pixel blocking are round 2's, the mapping is
// per pixel group: wave w, lane (p, h) = (lane & 7, lane >> 3): own pixels u = q0 + 16w + 2p,
// u + 1, disparities e = dc + 8h .. +7; rows o = u+1-e-j, j = 0..8, serve both pixels (the 16
// lanes of a ds_read_b128 group read 12 distinct padded rows in distinct bank slots).
//   * other-side rows: two parity sub-rings of 64 padded rows (272 B) = the strip's two 64-row
//     blocks [q0-dc-64, q0-dc+64); after the strip's dots the older block's slots take the next
//     strip's block by LDS-DMA (that latency is the one the co-resident workgroup covers);
//   * own pixels: LDS-DMA one strip ahead into two parity buffers of 32 padded pixels (coalesced
//     1 KiB pieces; as buffer loads straight into VGPRs the 8-fold re-reads of every line through
//     the texture path cost more than the dots' LDS traffic), copied to VGPRs at the strip start;
//   * every cost lands in a 64 x 65 LDS tile T[d][pixel] of the strip; at the next strip's start
//     each wave reads its 16 L rows (full 256-B runs L[y][x][dc..dc+63]) and the 16 R rows the
//     strip completes (R[y][xr][dc..] = cost(xr + d, d): an R row of the chunk spans at most two
//     strips) into registers; the part an R row got from the previous strip waits in a register
//     carry (16 VGPRs, lane = d; row xr belongs to wave (xr + 3) & 3 in every strip), so every
//     store is a whole 256-B run -- no partial lines; the 32 stores go out in the first four dot
//     rows and drain while the strip computes;
//   * per strip: wait for the DMA, barrier, own pixels -> VGPRs and tile -> registers, barrier,
//     the next own pixels' DMA, dots, barrier, the next rows' DMA.
// Voxels with x >= W are R's invalid fill; strips past the row end compute nothing.
// ---------------------------------------------------------------------------
// cvlr3_kernel's volume stores are nontemporal (cache-policy bits 2; round 3: 0.769 -> 0.756 ms, 1: 0.762)
constexpr int C3_AUX = 2;
constexpr int C3_NX = 64;                                  // own pixels per strip
constexpr int C3_RING = 64;                                // rows per parity sub-ring
constexpr int C3_TS = 65;                                  // tile stride (floats per disparity)
constexpr size_t C3_RING_BYTES = (size_t)2 * C3_RING * CD_RB;           // 34,816 B
constexpr size_t C3_OWN_BYTES = (size_t)2 * 32 * CD_RB;                 // 17,408 B
constexpr size_t C3_TILE_OFF = C3_RING_BYTES + C3_OWN_BYTES + 64 * 4;   // R reads reach 63 floats before T
constexpr size_t C3_SMEM = C3_TILE_OFF + (size_t)(64 * C3_TS + 64) * 4; // ... and 62 past it: 69,376 B

// Instructions [n0, n1) of a unit's nine (a 32-row unit split over two waves): rows gbase + 2i (i = 0..31) of
// a feature row (the buffer) -> 32 padded LDS rows at lds_unit.  Lane s of the 8.5 instructions loads byte
// 256 (gbase + 2i) + 16 (s - 17 i), i = s / 17 (chunk 16, the pad, takes the next row's chunk 0); rows outside
// [0, W) -- negative ones wrap to huge offsets -- are past the records and load zeros, never used.
__device__ __forceinline__ void c3_unit(cd_u32x4 rs, int gbase, uint32_t lds_unit, int lane, int n0, int n1)
{
    // (an opaque lane copy: the offsets are recomputed per issue, a few VALU, instead of being
    // hoisted out of the strip loop into registers the dot loop needs)
    asm volatile("" : "+v"(lane));
    const uint32_t rowoff = (uint32_t)gbase * 256u;
    const uint32_t lb = __builtin_amdgcn_readfirstlane(lds_unit);
#pragma unroll
    for (int n = 0; n < 9; n++) {
        if (n < n0 || n >= n1) continue;
        const int sl = 64 * n + lane;
        const int i = (sl * 3856) >> 16;                // sl / 17 for sl < 544
        if (n < 8 || lane < 32) cd_dma16(rs, rowoff + 16u * sl + 240u * i, lb + 1024u * n);
    }
}

// WR: also the right volume.  Without it (the aggregation path: sde_cbca_lr writes the right volume as the
// aggregated left one's shear) the strips end at the row end and half the stores go.
template <bool WR>
__global__ __launch_bounds__(256, 2) void cvlr3_kernel(const float *__restrict__ fl, const float *__restrict__ fr,
                                                       int H, int W, int D, int nchunks, float invalid,
                                                       float *__restrict__ outl, float *__restrict__ outr)
{
    constexpr int NST = WR ? 32 : 16;                   // emission stores per strip
    extern __shared__ __attribute__((aligned(16))) char c3_sm[];
    const char *ring = c3_sm;
    const char *own = c3_sm + C3_RING_BYTES;
    float *T = reinterpret_cast<float *>(c3_sm + C3_TILE_OFF);
    const uint32_t ring_l = cd_lds(ring), own_l = cd_lds(own);

    const int job = xcd_remap(blockIdx.x, gridDim.x);   // the chunks of a row share an XCD's L2
    const int y = job / nchunks;
    const int dc = (job - y * nchunks) * CV_DC;
    const int nd = min(CV_DC, D - dc);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 7, h = lane >> 3;
    const int e = dc + 8 * h;                           // this lane's first disparity
    const size_t rowvox = (size_t)y * W;
    const cd_u32x4 rs_o = cd_desc(fl + rowvox * 64, (uint32_t)W * 256u);   // own pixels' feature row
    const cd_u32x4 rs_r = cd_desc(fr + rowvox * 64, (uint32_t)W * 256u);   // other side's
    // row y of each volume (the host guarantees 4 W D < BUF_OOB)
    const __amdgpu_buffer_rsrc_t rl = buf_rsrc(outl + rowvox * D, (uint32_t)W * D * 4u);
    const __amdgpu_buffer_rsrc_t rr = buf_rsrc(WR ? outr + rowvox * D : outl, (uint32_t)W * D * 4u);
    // strips: the emission after strip k completes R rows [q0-dc-63, q0-dc] (whatever nd), so
    // the last strip holds x = W-1+dc+63 (left volume only: the last strip holds x = W-1)
    const int nstrips = WR ? (W + dc + 62) / C3_NX + 1 : (W + C3_NX - 1) / C3_NX;

    // a 64-row block of other-side rows at r (a multiple of 64): parity par, instructions [n0, n1)
    auto ring_unit = [&](int r, int par, int n0, int n1) {
        int k0 = (r >> 1) % C3_RING;
        if (k0 < 0) k0 += C3_RING;                      // a multiple of 32: the unit does not wrap
        c3_unit(rs_r, r + par, ring_l + (uint32_t)(par * C3_RING + k0) * CD_RB, lane, n0, n1);
    };
    // own pixels q + par + 2i (i < 32) -> parity buffer par
    auto own_unit = [&](int q, int par, int n0, int n1) {
        c3_unit(rs_o, q + par, own_l + (uint32_t)(par * 32) * CD_RB, lane, n0, n1);
    };

    // Emission of the tile of the strip at qp (lane = disparity dc + lane): L rows x = qp + wave + 4n,
    // R rows xr = qp - dc - 63 + i, i = 4n + wave (complete after this strip: lanes lane >= 63 - i
    // from the tile, the others from the carry), and the carry of the R rows this strip starts
    // (xr + 64, lanes lane <= 62 - i, for the next strip's emission).  Reads outside the tile land
    // in the slack words and are never selected.
    float vl[16], vr[16], cr[16];
#pragma unroll
    for (int n = 0; n < 16; n++) cr[n] = invalid;
    const float *tl = T + lane * C3_TS + wave;
    const float *tr = T + lane * (C3_TS + 1) + wave - 63;
    const uint32_t voff_d = lane < nd ? 4u * lane : BUF_OOB;
    auto emit_load = [&]() {
#pragma unroll
        for (int n = 0; n < 16; n++) {
            vl[n] = tl[4 * n];
            const float t = tr[4 * n];
            vr[n] = lane >= 63 - (4 * n + wave) ? t : cr[n];
            cr[n] = tr[4 * n + 64];
        }
    };
    // stores 8j .. 8j+7 of the 32 (16 L, 16 R runs), issued in the first four dot rows so they
    // drain while the strip computes.  A row outside the image stores with voffset BUF_OOB: the
    // buffer range check compares the voffset with the records (4 W D < BUF_OOB) and drops it, with
    // or without the soffset counted in (row offsets < 2^31: the sum cannot wrap) -- one select per
    // store, no branch.
    auto emit_store = [&](int qp, int j) {
        const int rowstep = 16 * D;                         // 4 rows of the volume, bytes
#pragma unroll
        for (int n = 8 * j; n < 8 * j + 8 && n < NST; n++) {
            if (n < 16) {
                const int x = qp + wave + 4 * n;
                const bool in = x < W;
                const uint32_t so = in ? (uint32_t)(((qp + wave) * D + dc) * 4 + n * rowstep) : 0u;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, vl[n]), rl, in ? voff_d : BUF_OOB, so,
                                                      C3_AUX);
            } else {
                const int xr = qp - dc - 63 + 4 * (n - 16) + wave;
                const bool in = (uint32_t)xr < (uint32_t)W;
                const uint32_t so = in ? (uint32_t)(((qp - dc - 63 + wave) * D + dc) * 4 + (n - 16) * rowstep) : 0u;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, vr[n - 16]), rr, in ? voff_d : BUF_OOB,
                                                      so, C3_AUX);
            }
        }
    };

    // strip 0: rows [-dc-64, 64-dc) (two blocks x two parities, one unit per wave) and own pixels
    ring_unit(-dc - 64 + 64 * (wave >> 1), wave & 1, 0, 9);
    own_unit(0, wave & 1, (wave >> 1) ? 5 : 0, (wave >> 1) ? 9 : 5);

    for (int k = 0; k < nstrips; k++) {
        const int q0 = k * C3_NX;
        const bool more = k + 1 < nstrips;
        const bool compute = q0 + 16 * wave < W;            // wave-uniform
        const int u = q0 + 16 * wave + 2 * p;
        // this strip's rows and own pixels have landed (every wave's DMA, hence the barrier); the
        // previous strip's tile is complete.  Only the own pixels are waited for here --
        // per wave the ops after them are the previous strip's 32 emission stores (none before
        // strip 2) and this strip's 4-5 ring DMA instructions, and vmcnt retires in order -- so the
        // row block's DMA latency overlaps the own copy and the tile reads; the rows are waited for
        // before the second barrier.
        if (k == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (k == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (WR) asm volatile("s_waitcnt vmcnt(36)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
        cd_barrier();
        f32x2 own_a[32], own_b[32];
        if (compute) {
            const f32x4 *sa = reinterpret_cast<const f32x4 *>(own + (size_t)(8 * wave + p) * CD_RB);
            const f32x4 *sb = reinterpret_cast<const f32x4 *>(own + (size_t)(32 + 8 * wave + p) * CD_RB);
#pragma unroll
            for (int c = 0; c < 16; c++) {
                const f32x4 va = sa[c], vb = sb[c];
                own_a[2 * c] = va.xy; own_a[2 * c + 1] = va.zw;
                own_b[2 * c] = vb.xy; own_b[2 * c + 1] = vb.zw;
            }
        }
        if (k > 0) emit_load();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this strip's rows
        cd_barrier();                                       // the own buffers and the tile are free
        if (more) own_unit(q0 + C3_NX, wave & 1, (wave >> 1) ? 5 : 0, (wave >> 1) ? 9 : 5);
        {
            float *Tw = T + (e - dc) * C3_TS + 16 * wave + 2 * p;   // tile column of pixel u (u + 1: +1), disparity e
            const int obase = u + 1 - e;                    // odd: rows j even are odd, j odd even
            const int kb = (obase >> 1) & (C3_RING - 1);
            const bool aok = u < W, bok = u + 1 < W;
            // wave-uniform (lanes past nd compute values that are never stored): no exec masking, so
            // the nine rows are one straight-line block the scheduler can pipeline across
            if (compute) {
                // the 72 (row, 32-byte piece) steps with the pieces two steps ahead in flight
                auto piece = [&](int jj, int mm, f32x4 &a, f32x4 &b) {
                    const int kj = (kb - (jj >> 1)) & (C3_RING - 1);
                    const f32x4 *row = reinterpret_cast<const f32x4 *>(
                        ring + (size_t)(((jj & 1) ? 0 : C3_RING) + kj) * CD_RB);
                    a = row[2 * mm];
                    b = row[2 * mm + 1];
                };
                f32x4 pa[3], pb[3];
                piece(0, 0, pa[0], pb[0]);
                piece(0, 1, pa[1], pb[1]);
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    const int o = obase - j;
                    f32x2 xa[4], xb[4];     // accumulators (0,1) (2,3) (4,5) (6,7)
#pragma unroll
                    for (int m = 0; m < 8; m++) {
                        const int st = 8 * j + m, nx = st + 2;
                        if (nx < 72) piece(nx >> 3, nx & 7, pa[nx % 3], pb[nx % 3]);
                        const f32x4 a = pa[st % 3], b = pb[st % 3];
                        const f32x2 r[4] = {a.xy, a.zw, b.xy, b.zw};
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            if (j <= 7) {
                                const f32x2 pr = own_b[4 * m + t] * r[t];
                                xb[t] = m == 0 ? pr : xb[t] + pr;
                            }
                            if (j >= 1) {
                                const f32x2 pr = own_a[4 * m + t] * r[t];
                                xa[t] = m == 0 ? pr : xa[t] + pr;
                            }
                        }
                    }
                    // the pairwise tree ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)): the first level within
                    // each pixel's channel pairs as single adds, the rest packed across the two pixels
                    // (left to itself, the compiler packed the first level with three moves per add)
                    if (j >= 1 && j <= 7) {
                        f32x2 s[4];
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            float ua, ub;
                            asm("v_add_f32 %0, %1, %2" : "=v"(ua) : "v"(xa[t].x), "v"(xa[t].y));
                            asm("v_add_f32 %0, %1, %2" : "=v"(ub) : "v"(xb[t].x), "v"(xb[t].y));
                            s[t] = f32x2{ua, ub};
                        }
                        const f32x2 sm = f32x2{0.0f, 0.0f} + ((s[0] + s[1]) + (s[2] + s[3]));
                        Tw[j * C3_TS + 1] = (bok && o >= 0) ? -sm.y : invalid;
                        Tw[(j - 1) * C3_TS] = (aok && o >= 0) ? -sm.x : invalid;
                    } else {
                        const f32x2 *x = j == 0 ? xb : xa;
                        float u[4];
#pragma unroll
                        for (int t = 0; t < 4; t++) asm("v_add_f32 %0, %1, %2" : "=v"(u[t]) : "v"(x[t].x), "v"(x[t].y));
                        const float sm = 0.0f + ((u[0] + u[1]) + (u[2] + u[3]));
                        if (j == 0) Tw[1] = (bok && o >= 0) ? -sm : invalid;
                        else Tw[7 * C3_TS] = (aok && o >= 0) ? -sm : invalid;
                    }
                    if (k > 0) emit_store(q0 - C3_NX, j);     // the previous strip's runs
                }
            } else {
                // past the row end: R's invalid fill only
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    Tw[j * C3_TS] = invalid;
                    Tw[j * C3_TS + 1] = invalid;
                    if (k > 0) emit_store(q0 - C3_NX, j);
                }
            }
        }
        // every wave's dots are done: the older row block's slots take the next strip's block
        cd_barrier();
        if (more) ring_unit(q0 + C3_NX - dc, wave & 1, (wave >> 1) ? 5 : 0, (wave >> 1) ? 9 : 5);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    cd_barrier();
    emit_load();
#pragma unroll
    for (int j = 0; j < NST / 8; j++) emit_store((nstrips - 1) * C3_NX, j);
}

}  // namespace sde
