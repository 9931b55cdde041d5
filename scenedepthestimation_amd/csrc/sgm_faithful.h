// sgm_faithful.h -- the SGM recurrence in the reference's exact arithmetic: the slow path a scanline takes
// from its first step on that the fast recurrence would not compute as the reference does: a non-finite cost or
// penalty, a P1 below zero, or (accumulating onto a caller's S) a voxel whose cost and S are both -0.0.
//
// The fast recurrence (sgm_scan.h: min chain in any order, one wave-wide minimum, no term for the missing
// neighbour at d = 0 and D-1) equals the reference's for finite costs and penalties of any sign except P1 < 0,
// up to the signs of zeros in L: its minima are then plain minima, L'(d) + P1 >= L'(d) makes the dropped term
// idle, and a zero's sign in L reaches S only where S and the cost are both -0.0.  With NaN / inf in
// the costs the reference's exact arithmetic decides where they propagate (SGM_Interation,
// process_functional.py:265-343): Numba's binary min(a, b) = b if b < a else a (a NaN first
// argument sticks, a NaN second one is ignored), the chain
//   c += min(min(L(d-1) + P1, L(d)), min(L(d+1) + P1, mcP2)) - mc
// with L(d-1) := L(d) at d = 0 and L(d+1) := L(d) at d = D-1, and the minimum kept PER
// reference lane of 4 disparities: min(min(c1, c2), min(c3, c4)), then an xor butterfly
// min(m, shfl_xor(m, k)), k = 1, 2, 4, .. -- with NaN present lanes can end with different
// minima, and each uses its own at the next step.  A line switches to this "faithful" step
// (sticky) at the first such step: the line is replayed from its start in this arithmetic and
// stores from that step on (every S stored before it is the reference's).  Generic D (the reference has D = 128 only): lanes of 4, missing
// disparities of the last lane and padding lanes up to a power of two act as +inf.
#pragma once
#include "sgm_wave.h"

namespace sde {

__device__ __forceinline__ double pymin(double a, double b) { return b < a ? b : a; }

// LDS of the faithful step (wave-private): the step's path costs, then one minimum per reference lane
template <int DPL>
struct FaithLds {
    double L[64 * DPL];
    double v[128];
};

// One SGM_Interation in the reference's exact arithmetic (see above).  mv / mpv: this lane's
// disparities' reference-lane minimum and minimum + P2 from the previous step; updated here.
template <int DPL>
__device__ __forceinline__ void faithful_step(double (&Ln)[DPL], const double (&L)[DPL], const float (&c)[DPL],
                                           bool restart, double p1, double p2, double (&mv)[DPL],
                                           double (&mpv)[DPL], int D, int dbase, FaithLds<DPL> &lds)
{
    const int lane = threadIdx.x & 63;
    if (restart) {
#pragma unroll
        for (int i = 0; i < DPL; i++) Ln[i] = (double)c[i];
    } else {
        const double lo = dpp_f64<0x138>(L[DPL - 1]);   // wave_shr:1 -> L'(dbase - 1)
        const double hi = dpp_f64<0x130>(L[0]);         // wave_shl:1 -> L'(dbase + DPL)
#pragma unroll
        for (int i = 0; i < DPL; i++) {
            const int d = dbase + i;
            const double self = L[i];
            const double lft = d > 0 ? (i > 0 ? L[i - 1] : lo) : self;
            const double rgt = d < D - 1 ? (i < DPL - 1 ? L[i + 1] : hi) : self;
            const double m1 = pymin(lft + p1, self);
            const double m2 = pymin(rgt + p1, mpv[i]);
            Ln[i] = (double)c[i] + (pymin(m1, m2) - mv[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < DPL; i++)
        if (dbase + i < D) lds.L[dbase + i] = Ln[i];
    wave_sync();
    const int nl = (D + 3) / 4;
    int nlp = 1;
    while (nlp < nl) nlp <<= 1;
    double v[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int j = lane + 64 * t;
        double q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = (j < nl && 4 * j + k < D) ? lds.L[4 * j + k] : __builtin_inf();
        v[t] = pymin(pymin(q[0], q[1]), pymin(q[2], q[3]));
    }
    for (int k = 1; k < nlp; k <<= 1) {
        if (k < 64) {
#pragma unroll
            for (int t = 0; t < 2; t++) v[t] = pymin(v[t], __shfl_xor(v[t], k, 64));
        } else {   // lanes j and j ^ 64 live in this lane
            const double a = v[0], b = v[1];
            v[0] = pymin(a, b);
            v[1] = pymin(b, a);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; t++)
        if (lane + 64 * t < nlp) lds.v[lane + 64 * t] = v[t];
    wave_sync();
#pragma unroll
    for (int i = 0; i < DPL; i++) {
        const int d = min(dbase + i, D - 1);
        mv[i] = lds.v[d >> 2];
        mpv[i] = mv[i] + p2;
    }
    wave_sync();     // this step's LDS reads before the next step's writes
}

// One vertical line (column `line`) in the faithful arithmetic, no prefetch: the redo of a
// column whose costs are not all finite after a pass that folded DU into UD (the fold is exact
// for finite costs only).  down: UD (penalty ch 2/3) or DU (ch 0/1); accumulate: S += L,
// else S := f32(0 + L) and the rows the line does not visit are zeroed.
// (The other walk in this arithmetic, a line's replay from its first non-finite step, is the loop at the
// end of sgm_scan_kernel.  One walk on Walker for both was measured and put back: inlined it cost 67 of the
// generic-D kernels SGPR spills, as a call 95, and the call's registers counted against the full-D kernels.)
template <int DPL>
__device__ __noinline__ void faithful_vertical(const float *cv, const float *pen, float *S, int H, int W, int D,
                                               int line, bool down, bool accumulate, FaithLds<DPL> &lds)
{
    const int lane = threadIdx.x & 63, dbase = lane * DPL;
    const int n = H - 1 > 2 ? H - 1 : 2;
    double L[DPL], mv[DPL], mpv[DPL];
#pragma unroll
    for (int i = 0; i < DPL; i++) L[i] = mv[i] = mpv[i] = 1.0;
    for (int k = 0; k < n; k++) {
        const int r = down ? k : H - 1 - k;
        const int pr = down ? r - 1 : r + 1;
        const double p1 = (pr >= 0 && pr < H) ? (double)pen[((size_t)pr * W + line) * 16 + (down ? 2 : 0)] : 0.0;
        const double p2 = (double)pen[((size_t)r * W + line) * 16 + (down ? 3 : 1)];
        const size_t off = ((size_t)r * W + line) * D;
        float c[DPL];
#pragma unroll
        for (int i = 0; i < DPL; i++) c[i] = cv[off + min(dbase + i, D - 1)];
        double Ln[DPL];
        faithful_step<DPL>(Ln, L, c, k == 0, p1, p2, mv, mpv, D, dbase, lds);
#pragma unroll
        for (int i = 0; i < DPL; i++) {
            if (dbase + i < D) {
                const double s0 = accumulate ? (double)S[off + dbase + i] : 0.0;
                S[off + dbase + i] = (float)(s0 + Ln[i]);
            }
            L[i] = Ln[i];
        }
    }
    if (!accumulate)
        for (int r = down ? n : 0; down ? r < H : r < H - n; r++)
#pragma unroll
            for (int i = 0; i < DPL; i++)
                if (dbase + i < D) S[((size_t)r * W + line) * D + dbase + i] = 0.0f;
}

}  // namespace sde
