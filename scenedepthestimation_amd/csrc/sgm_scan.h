// sgm_scan.h -- sgm_scan_kernel: one SGM direction over the scanlines of one or two image sides.
//
// Replaces SGM_Interation + the 8 SGM_*_kernel (process_functional.py:265-797; launch order :1166-1203).
//
// SGM recurrence, exactly as the reference computes it (Numba unifies the 1.0
// initialisers with the f32 loads, so the path state is float64):
//   L(p,d) = C(p,d)                                            first pixel / wrap restart
//   L(p,d) = C(p,d) + (min(L'(d), L'(d-1)+P1, L'(d+1)+P1, m'+P2') - m')   otherwise
//   S(p,d) = f32(f64(S(p,d)) + L(p,d));   m = min_d L(p,d)
// with P1 from the previous pixel's penalty channel, P2' read at the previous
// step, out-of-range neighbours (d = 0, D-1) dropped (the reference takes the voxel itself
// there: the same minimum for P1 >= 0; a step with P1 < 0 goes faithful), n-1 pixels per line of n
// (>= 2), and diagonal lines wrapping around the image with a path restart.
//
// Mapping: one wave64 (one workgroup) per scanline and image side, so the line,
// the pixel sequence and the penalty addresses are wave-uniform (scalar loads).
// Lane l owns DPL = ceil(D/64) consecutive disparities d = l*DPL + i in
// registers: d-1 / d+1 cross a lane only at i = 0 / DPL-1 (one DPP wave_shr /
// wave_shl per fp64 half), and min_d is a DPP butterfly (quad_perm, row_ror,
// row_bcast) ending in one readlane -- no LDS round trips on the serial chain.
// Each step's C and S rows (DPL floats per lane, one dwordx{DPL} load each,
// addresses clamped so no load is predicated) are prefetched PF steps ahead in
// a register ring, so HBM latency overlaps the sequential DP.  The left and
// right image sides (the reference's k loop) run in the same launch (grid.y).
//
// The cost and S streams are touched once per pass: nontemporal loads and stores.  Both together:
// 6.44 -> 5.96 ms for the 7-launch pair (either alone measured no change).
#pragma once
#include "sgm_faithful.h"
#include "sgm_wave.h"

namespace sde {

// The directions in the reference launch order (UD, DU, LR, RL, then the four diagonals): step (dr, dc)
// and the penalty channel of P1 (P2 is the next channel; ch is even).
struct SgmDir {
    int dr, dc, ch;
};
constexpr SgmDir kSgmDir[8] = {{+1, 0, 2}, {-1, 0, 0},   {0, +1, 6},  {0, -1, 4},
                               {+1, +1, 10}, {-1, +1, 12}, {+1, -1, 8}, {-1, -1, 14}};

// the same table, one field per array, for a direction known only at run time (one scalar load per field)
struct SgmDirField {
    int v[8];
};
constexpr SgmDirField sgm_dir_field(int SgmDir::*f)
{
    SgmDirField o{};
    for (int i = 0; i < 8; i++) o.v[i] = kSgmDir[i].*f;
    return o;
}
__constant__ SgmDirField c_dir_dr = sgm_dir_field(&SgmDir::dr);
__constant__ SgmDirField c_dir_dc = sgm_dir_field(&SgmDir::dc);
__constant__ SgmDirField c_dir_ch = sgm_dir_field(&SgmDir::ch);

struct SgmSide {
    const float *cv;
    const float *pen;
    float *S;
    float *disp;    // WTA fused into the last direction (sde_sgm_8path_wta_pair), else unused
};

struct PathGeom {
    int dr, dc, ch, H, W, n;    // n: pixels the pass visits per line

    // DIRC >= 0: the direction is a compile-time constant (the walker's steps, wrap tests and the penalty
    // channel fold), else `dir` is read from the table in constant memory
    template <int DIRC>
    __device__ __forceinline__ void init(int dir, int H_, int W_)
    {
        if (DIRC >= 0) {
            dr = kSgmDir[DIRC & 7].dr; dc = kSgmDir[DIRC & 7].dc; ch = kSgmDir[DIRC & 7].ch;
        } else {
            dr = c_dir_dr.v[dir]; dc = c_dir_dc.v[dir]; ch = c_dir_ch.v[dir];
        }
        H = H_; W = W_;
        n = length() - 1 > 2 ? length() - 1 : 2;
    }
    // pixels of a line
    __device__ __forceinline__ int length() const { return (dc != 0 && dr == 0) ? W : H; }
    // The border pixel at which scanline `line` starts (begin) or, walked without its wraps, ends: the
    // end of a direction is the beginning of the opposite one.  Vertical and diagonal lines are named by
    // their column, horizontal ones by their row.
    __device__ __forceinline__ void border(int line, bool begin, int &r, int &c) const
    {
        if (dc == 0) { c = line; r = (dr > 0) == begin ? 0 : H - 1; }
        else if (dr == 0) { r = line; c = (dc > 0) == begin ? 0 : W - 1; }
        else { r = (dr > 0) == begin ? 0 : H - 1; c = line; }
    }
};

// k-th pixel of scanline `line`; restart = first pixel or diagonal wrap.  (The replay of a line in the
// faithful arithmetic, at the end of sgm_scan_kernel.)
__device__ __forceinline__ void path_pixel(const PathGeom &g, int line, int k, int &r, int &c, bool &restart)
{
    restart = (k == 0);
    if (g.dc == 0) {                       // vertical: line = column
        c = line;
        r = g.dr > 0 ? k : g.H - 1 - k;
    } else if (g.dr == 0) {                // horizontal: line = row
        r = line;
        c = g.dc > 0 ? k : g.W - 1 - k;
    } else {                               // diagonal: line = start column, wraps
        r = g.dr > 0 ? k : g.H - 1 - k;
        if (g.dc > 0) {
            c = (int)(((int64_t)line + k) % g.W);
            if (k > 0 && c == 0) restart = true;
        } else {
            int64_t cc = ((int64_t)line - k) % g.W;
            if (cc < 0) cc += g.W;
            c = (int)cc;
            if (k > 0 && c == g.W - 1) restart = true;
        }
    }
}

// Incremental walk along a scanline (wave-uniform scalars; no divisions).  Same
// pixel sequence as path_pixel: diagonal lines wrap around the image with a
// path restart.  Steps past the end of the line are clamped into the image (the
// kernel re-reads valid memory there and stores nothing).
// The pixel index itself advances (one 64-bit scalar add per step, and a
// +-W on a diagonal wrap) and stops at the line's last pixel, instead of clamping (r, c) and
// recomputing r W + c and the previous pixel's index with 64-bit multiplies on every step.  A
// step's predecessor on the path is the previous step's pixel unless the step restarts the path
// (line start, diagonal wrap), which is exactly when the reference's P1 pixel is outside the
// image -- so P1 is carried from the previous step and one 8-byte load per step fetches (P1, P2)
// of the pixel (channels ch, ch + 1; ch even).
struct Walker {
    int r, c;           // r: the line's first row (init only; as a local it swaps a multiply's operands)
    bool restart;
    int left;           // moves left before the line's last pixel
    long long dpx;      // pixel-index step dr W + dc
    size_t px;          // the pixel index r W + c
    __device__ __forceinline__ void init(const PathGeom &g, int line)
    {
        g.border(line, true, r, c);
        restart = true;
        left = min(g.n, g.length()) - 1;
        dpx = (long long)g.dr * g.W + g.dc;
        px = (size_t)r * g.W + c;
    }
    __device__ __forceinline__ void advance(const PathGeom &g)
    {
        // selects, not branches (scalar s_cselect; the step is one basic block)
        const bool mv = left > 0;
        left -= mv ? 1 : 0;
        c += mv ? g.dc : 0;
        px += mv ? dpx : 0;
        restart = false;
        if (g.dr != 0 && g.dc != 0) {
            const bool wr = g.dc > 0 ? c >= g.W : c < 0;
            c = wr ? (g.dc > 0 ? 0 : g.W - 1) : c;
            px = wr ? (g.dc > 0 ? px - g.W : px + g.W) : px;
            restart = wr;
        }
    }
};

template <int N>
struct SgmV {
    typedef float T __attribute__((ext_vector_type(N)));
};

// A cost or a penalty anywhere in the wave that the fast recurrence does not treat as the reference does: NaN or
// +-inf (its minima are the reference's for finite operands only), or a P1 below zero.  The reference's missing
// neighbour at d = 0 and d = D-1 is the voxel itself, so its chain holds L'(d) + P1 there; the fast chain drops
// that term, which is the same minimum only while P1 >= 0.  (P2 may have any sign: m' + P2 is one term in both.)
// c: DPL floats, an array or a vector.
template <int DPL, typename C>
__device__ __forceinline__ bool any_nonfinite(const C &c, float p1, float p2)
{
    bool nf = __builtin_amdgcn_classf(p1, 0x207) | __builtin_amdgcn_classf(p2, 0x207);   // s/qNaN, -inf, +inf
#pragma unroll
    for (int i = 0; i < DPL; i++) nf |= __builtin_amdgcn_classf(c[i], 0x207);
    // p1 is wave-uniform: one scalar compare of its bits -- sign set and not -0.0 (a second class mask would
    // cost every form a register)
    return __builtin_amdgcn_ballot_w64(nf) != 0 || __float_as_uint(p1) > 0x80000000u;
}

// A voxel whose cost and incoming S are both -0.0, anywhere in the wave: the only way a zero's sign reaches S
// (S + L = -0 needs both at -0, and L = C + x is -0 only for C = -0).  Which sign L's zero has there depends on
// the order of the reference's minima over zeros of both signs (left, self, right, m + P2, and one minimum per
// reference lane), which the fast chain (self first, one wave minimum) does not keep -- so the forms that
// accumulate onto a caller's S send such a step to the faithful path.  S the library wrote itself holds no -0.0.
template <int DPL, typename C>
__device__ __forceinline__ bool any_negzero_pair(const C &c, const C &s)
{
    bool nz = false;
#pragma unroll
    for (int i = 0; i < DPL; i++) nz |= __float_as_uint(c[i]) == 0x80000000u && __float_as_uint(s[i]) == 0x80000000u;
    return __builtin_amdgcn_ballot_w64(nz) != 0;
}

// WTA_and_SupixelRefinement_kernel (process_functional.py:800-837) on one pixel whose S values
// are o[i] at d = dbase + i: best = S(0), `best > S(d)` for d = 1.. (== the +inf first-min scan,
// except that "no winner" and a NaN S(0) give 0); lane 63 holds the answer.
template <int DPL>
__device__ __forceinline__ int wta_pixel(const float (&o)[DPL], int dbase, int D)
{
    float best = __builtin_inff();
    int arg = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < DPL; i++)
        if (dbase + i < D && o[i] < best) { best = o[i]; arg = dbase + i; }
    wave_argmin(best, arg);
    const float v0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o[0]), 0));
    return (arg == 0x7fffffff || v0 != v0) ? 0 : arg;
}

// The end of one step's 64-way merge in the fused WTA: the G lanes of the step (a DPP row group)
// hold the merges of their PF partials each; quad_perm, quad_perm, row_half_mirror (and
// row_mirror for G = 16) leave every lane with the G-lane result -- the merge is a total order
// (first-min with index tie-break, no NaN partials), so any order agrees -- and lane q = 0 stores
// the disparity (rule of WTA_and_SupixelRefinement_kernel: "no winner" -> 0) unless px < 0.
template <int G>
__device__ __forceinline__ void wta_block_store(float bv, int ba, int px, int q, float *disp)
{
    static_assert(G == 8 || G == 16, "the fused WTA merge reduces 8 or 16 lanes per step");
    argmin_dpp<0xB1>(bv, ba);                   // quad_perm [1,0,3,2]
    argmin_dpp<0x4E>(bv, ba);                   // quad_perm [2,3,0,1]
    argmin_dpp<0x141>(bv, ba);                  // row_half_mirror: the other quad of the 8
    if (G == 16) argmin_dpp<0x140>(bv, ba);     // row_mirror: the other 8 of the 16
    if (q == 0 && px >= 0) disp[px] = (float)(ba == 0x7fffffff ? 0 : ba);
}

// the destination of the S stores a step must not make (sgm_scan_kernel): one row of the widest lane
// block, rewritten by every wave that needs it, never read.  Aligned explicitly: every line's wave ends
// with one such store, all to these same bytes, and where the row falls within a cache line must not
// depend on what else the object holds.
__device__ __attribute__((aligned(256))) float sgm_dump[64 * 16];

// a slot's DPL costs / S values as ONE vector value: as separate floats, the loop-header phis of
// the elements did not coalesce with the dwordx{DPL} load's register tuple, and the loop latch
// copied them back -- waiting for each slot's load, i.e. draining the prefetch ring
template <int DPL>
struct Slot {
    typename SgmV<DPL>::T c;
    typename SgmV<DPL>::T s;
    float p1, p2;   // this pixel's P1 channel (the NEXT step's P1) and P2
    size_t off;     // voxel offset of (r, c, d = 0)
    int pix;        // pixel index r W + c (the fused WTA's output index; no 64-bit division by D per step)
    bool restart;
};

// VEC: D % DPL == 0, every lane's DPL disparities are all valid or all invalid
// and move as one dwordx{DPL}; otherwise per-element loads with clamped d.
template <int DPL, bool VEC, bool FIRST>
__device__ __forceinline__ void issue(const PathGeom &g, const Walker &w, const SgmSide &sd, int D, int dbase,
                                      Slot<DPL> &sl)
{
    const size_t px = w.px;
    const float2 pp = *reinterpret_cast<const float2 *>(sd.pen + px * 16 + g.ch);
    sl.p1 = pp.x;
    sl.p2 = pp.y;
    sl.restart = w.restart;
    sl.pix = (int)px;
    const size_t off = px * D;
    sl.off = off;
    if (VEC) {
        // wave-uniform row pointers + a 32-bit lane offset: the loads take the SGPR-base form
        const float *cvp = sd.cv + off, *sp = sd.S + off;
        const unsigned lo = (unsigned)(dbase < D ? dbase : 0);
#pragma unroll
        for (int i = 0; i < DPL; i++) sl.c[i] = __builtin_nontemporal_load(cvp + lo + i);
        if (!FIRST)
#pragma unroll
            for (int i = 0; i < DPL; i++) sl.s[i] = __builtin_nontemporal_load(sp + lo + i);
    } else {
#pragma unroll
        for (int i = 0; i < DPL; i++) {
            const int d = dbase + i < D ? dbase + i : D - 1;
            sl.c[i] = sd.cv[off + d];
            if (!FIRST) sl.s[i] = sd.S[off + d];
        }
    }
}

// FIRST: S := f32(0 + L) (S is not read).  DU (direction UD only): also apply direction
// DU in the same pass.  With the penalty channels 0/1 zero -- sgm_penelty_kernel never
// writes them (:134-262) -- and finite costs, DU's recurrence collapses: b = m' exactly,
// so L_DU = C at its first pixel (row H-1) and C + 0.0 elsewhere; the reference adds
// it after UD (launch order :1166-1203), which per voxel is this same sequence.
// WTA (last direction only): the final S of each visited voxel is not stored; the pixel's
// first-min disparity (rule of WTA_and_SupixelRefinement_kernel) goes to sd.disp instead, and
// the pixels this direction never visits (its lines stop one short) take the WTA of the S
// already in memory.
// VMIN: S holds no -0.0 on entry (this library wrote it, or the pass overwrites it): the fast
// recurrence's minima may run on v_min_f64 (see dmin).  Accumulating onto a caller's S keeps the selects.
// sgm.hip's form table lists the combinations that are instantiated.
template <int DPL, int PF, bool VEC, bool FIRST, bool DU, bool WTA, int DC, int DIRC, bool VMIN>
__global__ __launch_bounds__(64) void sgm_scan_kernel(SgmSide s0, SgmSide s1, int H, int W, int D, int dir)
{
    static_assert(!(WTA && (FIRST || DU)), "the fused WTA belongs to the last direction, FIRST and DU to the first");
    static_assert(!(DU && !FIRST && VMIN), "a DU fold that does not overwrite S accumulates onto a caller's S");
    static_assert(!(FIRST && !VMIN), "a pass that overwrites S never meets a caller's -0.0");
    static_assert(DC == 0 || (VEC && VMIN && DC == 64 * DPL), "compile-time D: full lanes, v_min forms only");
    // DC != 0: D == DC == 64 * DPL is a compile-time constant -- every lane's disparities are
    // valid, so the per-disparity range guards and the pixel index's division fold away
    if (DC) D = DC;
    const SgmSide sd = blockIdx.y ? s1 : s0;
    PathGeom g;
    g.init<DIRC>(dir, H, W);
    const int line = blockIdx.x;
    const int lane = threadIdx.x & 63;      // one wave per block: lane < 64 known to the compiler
    const int dbase = lane * DPL;
    const double INF = __builtin_inf();
    // fused WTA: the S values of the last PF steps (wave-private: one wave per block); G = 64 / PF
    // lanes scan one step's pixel.  The scan of a block of PF steps is spread over the next block's
    // steps (one read and compare per step, the G-lane DPP reduction and the store at its last step),
    // so the loop body stays one uniform step: a separate merge block after every PF steps made the
    // compiler rotate the prefetch ring's registers at the loop back-edge and drain it (vmcnt(0)
    // every PF steps).  Values and pixel indices are double-buffered by block parity.
    //
    // Each step parks its 64 DPL S values (+inf past D), value i of lane
    // l at word i IS + l of a row of RS words, and lane (st, q) scans pixel st's disparities
    // DPL (PF q + j) + i, i < DPL, at step j of the next block -- the values lane PF q + j parked --
    // in increasing d with a strict `<` (the reference's sequential scan over its chunk), so only the
    // G-lane DPP merge needs the index tie-break.  Banks (PF = 8): RS = 1 mod 64 puts pixel st's row
    // st banks over, lanes q of a read are 8 banks apart, and IS = 4 mod 64 sends the second word of
    // the compiler's paired `ds_read2_b32` to the other 4 banks of each 8: writes and reads are
    // conflict-free (a [lane][i] row with stride DPL had the pair's words collide: 12.6 M conflict
    // cycles per pair of launches).
    constexpr int IS = 68, RS = ((DPL * IS + 63) / 64) * 64 + 1;
    constexpr int G = 64 / PF;
    __shared__ float wbv[WTA ? 2 * PF * RS : 1];
    __shared__ int wpx[WTA ? 2 * PF : 1];
    __shared__ FaithLds<DPL> flds;

    if (DU && !FIRST) {
        // accumulate + DU fold: S's incoming values cannot be recovered after a folded pass, so a
        // column whose costs are not all finite is found first and runs both directions in the
        // reference's arithmetic (the fold is exact for finite costs only)
        // (and the UD penalties, channels 2/3: the fast recurrence's minima are the reference's
        // for finite operands and P1 >= 0 only; and a voxel with cost and S both -0.0: DU's own L can
        // be -0.0 there, which the fold's C + 0.0 never is)
        bool bad = false;
        for (int r = 0; r < H && !bad; r++) {
            float c[DPL], s[DPL];
            const size_t px = (size_t)r * W + line, off = px * D;
#pragma unroll
            for (int i = 0; i < DPL; i++) {
                c[i] = sd.cv[off + min(dbase + i, D - 1)];
                s[i] = sd.S[off + min(dbase + i, D - 1)];
            }
            bad = any_nonfinite<DPL>(c, sd.pen[px * 16 + 2], sd.pen[px * 16 + 3]) || any_negzero_pair<DPL>(c, s);
        }
        if (bad) {
            faithful_vertical<DPL>(sd.cv, sd.pen, sd.S, H, W, D, line, true, true, flds);
            faithful_vertical<DPL>(sd.cv, sd.pen, sd.S, H, W, D, line, false, true, flds);
            return;
        }
    }

    // Every load is unconditional (steps past the end re-read a clamped pixel):
    // a predicated load would make the ring slot a phi and force an early wait.  (Refilling the
    // ring two adjacent pixels at a time for the horizontal directions measured no gain in round 3
    // and was removed.)
    Slot<DPL> ring[PF];
    Walker ahead;
    ahead.init(g, line);
#pragma unroll
    for (int j = 0; j < PF; j++) {
        issue<DPL, VEC, FIRST>(g, ahead, sd, D, dbase, ring[j]);
        ahead.advance(g);
    }
    // the ring has landed before the loop: otherwise the loop header merges this entry path (the
    // fill's loads in another order, fewer ops after each) with the latch, and the waitcnt pass sizes
    // the first steps' waits for the entry path -- vmcnt(1..3) every PF steps, a drained ring.
    // Except in the first pass (cost loads, S stores, no S loads): there the drained ring is the
    // faster one, 619 against 646 us per launch (profiles/r04/sgm_ab_ring_waits.txt; PF 4 or 6:
    // 634 / 647 us) -- the other six launches gain from the full ring (DU-RL + WTA 670 -> 620 us)
    if (!(FIRST && DU)) __builtin_amdgcn_s_waitcnt(0xF70);          // vmcnt(0)

    double L[DPL];
    double m = 1.0, mP2 = 1.0;
    float p1c = 0.0f;              // the previous step's pixel's P1 channel
    int kf = -1;                   // first step the fast recurrence must not take: the line continues faithfully
    bool redo = false;             // DU fold (FIRST): recompute the column in the faithful arithmetic
#pragma unroll
    for (int i = 0; i < DPL; i++) L[i] = 1.0;

    // fused WTA: this lane's running merge over the previous block (lane (st, q) = (lane / G,
    // lane % G) merges the partials of lanes PF q .. PF q + PF - 1 of step st of that block)
    float mv_b = __builtin_inff();
    int mv_a = 0x7fffffff;
    const int wst = lane / G, wq = lane % G;
    for (int k0 = 0; k0 < g.n; k0 += PF) {
        const int buf = (k0 / PF) & 1;              // this block's partial buffer; buf ^ 1 = the previous block's
#pragma unroll
        for (int j = 0; j < PF; j++) {
            const int k = k0 + j;     // steps k >= n compute on a clamped pixel and store nothing
            const Slot<DPL> &sl = ring[j];
            const float p1f = sl.restart ? 0.0f : p1c;
            // (wave-uniform; into an SGPR for the reason given for p1c below)
            const float p2f = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sl.p2)));
            // read before the slot's refill at the end of this step, into an SGPR: carried as the
            // slot's own VGPR it stayed live across the refill, so the refill took other registers and
            // the loop latch copied every slot's penalty pair back -- waiting for each load in turn,
            // which drained the prefetch ring once per PF steps
            p1c = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sl.p1)));
            if (DU) {
                if (FIRST && !redo) redo = any_nonfinite<DPL>(sl.c, p1f, p2f);
            } else if (kf < 0 && k < g.n &&
                       (any_nonfinite<DPL>(sl.c, p1f, p2f) || (!VMIN && any_negzero_pair<DPL>(sl.c, sl.s)))) {
                // every state so far is finite, and equal to the reference's up to the signs of zeros in L, which
                // no S stored so far depends on; from step k on the line is redone in the reference's exact
                // arithmetic after this loop, which stores nothing more for it
                kf = k;
            }
            const bool keep = DU || kf < 0;
            double Ln[DPL];
            if (sl.restart) {
#pragma unroll
                for (int i = 0; i < DPL; i++) Ln[i] = (double)sl.c[i];
            } else {
                const double p1 = (double)p1f;
                const double lo = dpp_f64<0x138>(L[DPL - 1]);   // wave_shr:1 -> L'(dbase - 1)
                const double hi = dpp_f64<0x130>(L[0]);         // wave_shl:1 -> L'(dbase + DPL)
#pragma unroll
                for (int i = 0; i < DPL; i++) {
                    const int d = dbase + i;
                    double b = L[i];
                    const double left = i > 0 ? L[i - 1] : lo;
                    const double right = i < DPL - 1 ? L[i + 1] : hi;
                    if (DC) {
                        // D = 64 DPL: only lane 0's first and lane 63's last disparity lack a
                        // neighbour -- a select of +inf (min(b, inf) = b) instead of an exec-masked
                        // branch per step
                        b = dmin<VMIN>(b, (i > 0 || d > 0) ? left + p1 : INF);
                        b = dmin<VMIN>(b, (i < DPL - 1 || d < D - 1) ? right + p1 : INF);
                    } else {
                        if (d > 0) b = dmin<VMIN>(b, left + p1);
                        if (d < D - 1) b = dmin<VMIN>(b, right + p1);
                    }
                    b = dmin<VMIN>(b, mP2);
                    Ln[i] = (double)sl.c[i] + (b - m);
                }
            }
            float o[DPL];
#pragma unroll
            for (int i = 0; i < DPL; i++)
                o[i] = FIRST ? (float)(0.0 + Ln[i]) : (float)((double)sl.s[i] + Ln[i]);
            if (DU && k >= H - g.n) {          // UD visits row k; DU visits rows H-n .. H-1
                const bool du_first = (k == H - 1);
#pragma unroll
                for (int i = 0; i < DPL; i++) {
                    const double c = (double)sl.c[i];
                    o[i] = (float)((double)o[i] + (du_first ? c : c + 0.0));
                }
            }
            if (WTA) {
                // this step's S values parked; one piece of the previous block's scan (below), off
                // the recurrence's serial chain
                float *row = wbv + (buf * PF + j) * RS + lane;
#pragma unroll
                for (int i = 0; i < DPL; i++) row[i * IS] = (DC || dbase + i < D) ? o[i] : __builtin_inff();
                if (lane == 0) wpx[buf * PF + j] = (k < g.n && keep) ? sl.pix : -1;
                if (k0 > 0) {
                    const int d0 = DPL * (PF * wq + j);
                    const float *src = wbv + ((buf ^ 1) * PF + wst) * RS + PF * wq + j;
#pragma unroll
                    for (int i = 0; i < DPL; i++) {
                        const float v2 = src[i * IS];
                        if (j == 0 && i == 0) {
                            // the chunk's first value; a NaN S(0) makes the pixel's answer 0
                            const bool w = v2 < __builtin_inff();
                            mv_b = w ? v2 : __builtin_inff();
                            mv_a = w ? d0 : 0x7fffffff;
                            if (wq == 0 && v2 != v2) { mv_b = -__builtin_inff(); mv_a = 0; }
                        } else if (v2 < mv_b) {
                            mv_b = v2;
                            mv_a = d0 + i;
                        }
                    }
                    if (j == PF - 1) wta_block_store<G>(mv_b, mv_a, wpx[(buf ^ 1) * PF + wst], wq, sd.disp);
                }
            } else if (VEC) {
                // every step stores: a step that must not (past the line's end, a line gone faithful)
                // writes the dump row instead.  A store behind a branch left the waitcnt pass unsure
                // how many stores were in flight, so it waited for loads issued 2-3 steps back
                // instead of PF: the prefetch ring was mostly idle.
                float *const sbase = (k < g.n && keep) ? sd.S + sl.off : sgm_dump;
                if (dbase < D) {
#pragma unroll
                    for (int i = 0; i < DPL; i++)
                        __builtin_nontemporal_store(o[i], sbase + (unsigned)dbase + i);
                }
            } else if (k < g.n && keep) {
                {
#pragma unroll
                    for (int i = 0; i < DPL; i++)
                        if (dbase + i < D) sd.S[sl.off + dbase + i] = o[i];
                }
            }
            double mm = INF;
#pragma unroll
            for (int i = 0; i < DPL; i++)
                if (dbase + i < D) mm = dmin<VMIN>(mm, Ln[i]);
            m = wave_min_f64<VMIN>(mm);
            mP2 = m + (double)p2f;
#pragma unroll
            for (int i = 0; i < DPL; i++) L[i] = Ln[i];
            // the slot is refilled after its use (not hoisted above it): its registers are reused,
            // with no moves -- and waits -- at the loop back-edge
            issue<DPL, VEC, FIRST>(g, ahead, sd, D, dbase, ring[j]);
            ahead.advance(g);
        }
    }
    // The parked values and pixel indices cross lanes through LDS: lanes read what other lanes of the
    // wave wrote one block earlier.  Inside the loop a read is always a whole step after the writes it
    // depends on and the compiler does not move LDS accesses of one iteration across another's; here,
    // right after the last writes, the ordering is made explicit (wavefront-scope release/acquire and a
    // wave barrier: no instruction with one wave per workgroup, a scheduling fence only).
    if (WTA && g.n > 0) {
        wave_sync();
        // the last block's scan (its values are in buffer buf_last)
        const int buf = ((g.n - 1) / PF) & 1;
        const float *src = wbv + (buf * PF + wst) * RS + PF * wq;
        float b = __builtin_inff();
        int ba = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < DPL * PF; t++) {
            const float v = src[(t % DPL) * IS + t / DPL];      // d = DPL (PF wq + t / DPL) + t % DPL
            if (v < b) { b = v; ba = DPL * PF * wq + t; }
        }
        if (wq == 0 && src[0] != src[0]) { b = -__builtin_inff(); ba = 0; }
        wta_block_store<G>(b, ba, wpx[buf * PF + wst], wq, sd.disp);
    }
    if (!DU && kf >= 0) {
        // the line again in the reference's exact arithmetic (no prefetch: rare path), storing from
        // step kf on: the replayed finite prefix reproduces the fast steps' state exactly
        double mv[DPL], mpv[DPL];
#pragma unroll
        for (int i = 0; i < DPL; i++) L[i] = mv[i] = mpv[i] = 1.0;
        for (int k = 0; k < g.n; k++) {
            int r, c;
            bool restart;
            path_pixel(g, line, k, r, c, restart);
            const int pr = r - g.dr, pc = c - g.dc;
            const bool pin = pr >= 0 && pr < H && pc >= 0 && pc < W;
            const double p1 = pin ? (double)sd.pen[((size_t)pr * W + pc) * 16 + g.ch] : 0.0;
            const double p2 = (double)sd.pen[((size_t)r * W + c) * 16 + g.ch + 1];
            const size_t off = ((size_t)r * W + c) * D;
            float cc[DPL];
#pragma unroll
            for (int i = 0; i < DPL; i++) cc[i] = sd.cv[off + min(dbase + i, D - 1)];
            double Ln[DPL];
            faithful_step<DPL>(Ln, L, cc, restart, p1, p2, mv, mpv, D, dbase, flds);
            if (k < kf) {
#pragma unroll
                for (int i = 0; i < DPL; i++) L[i] = Ln[i];
                continue;
            }
            float o[DPL];
#pragma unroll
            for (int i = 0; i < DPL; i++) {
                const double s0 = FIRST ? 0.0 : (double)sd.S[off + min(dbase + i, D - 1)];
                o[i] = (float)(s0 + Ln[i]);
                L[i] = Ln[i];
            }
            if (WTA) {
                const int a = wta_pixel<DPL>(o, dbase, D);
                if (lane == 63) sd.disp[off / D] = (float)a;
            } else {
#pragma unroll
                for (int i = 0; i < DPL; i++)
                    if (dbase + i < D) sd.S[off + dbase + i] = o[i];
            }
        }
    }
    if (WTA && g.n < g.length()) {
        // the pixel this direction never visits: the border pixel at the line's end.
        // DU-RL (the reference's last direction) walks rows H-1 .. 1 and never reaches row 0:
        // pixel (0, line) is one of them for every line; other directions map analogously.
        int r0, c0;
        g.border(line, false, r0, c0);
        const size_t off = ((size_t)r0 * W + c0) * D;
        float o[DPL];
#pragma unroll
        for (int i = 0; i < DPL; i++) o[i] = sd.S[off + min(dbase + i, D - 1)];
        const int a = wta_pixel<DPL>(o, dbase, D);
        if (lane == 63) sd.disp[off / D] = (float)a;
    }
    if (FIRST || DU) {
        // rows UD never visits (it stops at row n-1): S := 0 (FIRST), then DU's term
        for (int r = g.n; r < H; r++) {
            const size_t off = ((size_t)r * W + line) * D;
#pragma unroll
            for (int i = 0; i < DPL; i++) {
                const int d = dbase + i;
                if (d < D) {
                    float v = FIRST ? 0.0f : sd.S[off + d];
                    if (DU) {
                        const float cf = sd.cv[off + d];
                        if (FIRST) redo |= (__float_as_uint(cf) & 0x7f800000u) == 0x7f800000u;
                        const double c = (double)cf;
                        v = (float)((double)v + (r == H - 1 ? c : c + 0.0));
                    }
                    sd.S[off + d] = v;
                }
            }
        }
    }
    if (DU && FIRST && __builtin_amdgcn_ballot_w64(redo) != 0) {
        // a non-finite cost (or a UD penalty the fast recurrence must not take) in this column: redo UD
        // (overwrite) and DU (accumulate) in the faithful arithmetic
        faithful_vertical<DPL>(sd.cv, sd.pen, sd.S, H, W, D, line, true, false, flds);
        faithful_vertical<DPL>(sd.cv, sd.pen, sd.S, H, W, D, line, false, true, flds);
    }
}

}  // namespace sde
