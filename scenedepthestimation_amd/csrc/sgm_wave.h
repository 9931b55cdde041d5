// sgm_wave.h -- wave64 primitives of the SGM kernels: DPP moves of doubles and ints, the fp64 minimum and its
// wave-wide butterfly, the wave-scope LDS fence, and the (value, index) first-min reduction.  No LDS round
// trips: every cross-lane step is a DPP move (quad_perm, row_ror, row_bcast, wave_shr / wave_shl).
#pragma once
#include "sde_common.h"

namespace sde {

// DPP move of a double (two 32-bit halves); lanes outside ROW_MASK keep `v`.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_f64(double v)
{
    const long long b = __builtin_bit_cast(long long, v);
    int lo = (int)b, hi = (int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// DPP move of a double for reductions whose disabled lanes are never read: no `old` operand, so
// the compiler emits the two v_mov_b32_dpp into fresh registers (dpp_f64's old = v costs two
// v_mov copies per stage).  Lanes outside ROW_MASK hold unspecified values.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_f64_nold(double v)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, ROW_MASK, 0xF, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// DPP move of an int; lanes outside ROW_MASK keep `v`.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp_i32(int v)
{
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xF, false);
}

// t < a ? t : a.  VMIN: one v_min_f64 instead of a compare and two selects.  The two differ
// only when a is NaN or both are zeros of opposite signs.  In the fast recurrence no operand
// is NaN (non-finite costs and penalties take the faithful path), and a zero's sign never
// changes a magnitude downstream (x + -0 = x + +0 for x != 0; comparisons ignore it): it can
// reach S only through S + L with S = -0, and S is never -0 unless the caller's accumulate
// input holds one.  The selects do not give the reference's zero signs either (its chain
// prefers left, self, right, m + P2 on a tie and keeps a minimum per reference lane; this one
// prefers self and has one wave minimum), so the forms that accumulate onto a caller's S send
// a step that could show the difference -- a voxel with S and cost both -0.0 -- to the
// faithful path (any_negzero_pair, sgm_scan.h); they keep the selects, whose result for
// finite operands does not depend on the instruction's handling of zeros.
template <bool VMIN = false>
__device__ __forceinline__ double dmin(double a, double t)
{
    if (VMIN) {
        double r;
        asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(t), "v"(a));
        return r;
    }
    return t < a ? t : a;
}

// min over the 64 lanes, returned wave-uniform.  Only lane 63 is read: stages 1-4 move within
// rows (every lane valid); stage 5 updates rows 1 and 3 from lanes 15 and 47, stage 6 row 3 from
// lane 31 (row 1, valid after stage 5) -- the rows a stage leaves out hold unspecified values
// and never feed lane 63, so the moves need no `old` operand.
template <bool VMIN = false>
__device__ __forceinline__ double wave_min_f64(double v)
{
    v = dmin<VMIN>(v, dpp_f64_nold<0xB1>(v));          // quad_perm [1,0,3,2]
    v = dmin<VMIN>(v, dpp_f64_nold<0x4E>(v));          // quad_perm [2,3,0,1]
    v = dmin<VMIN>(v, dpp_f64_nold<0x124>(v));         // row_ror:4
    v = dmin<VMIN>(v, dpp_f64_nold<0x128>(v));         // row_ror:8   -> every lane holds its row's min
    v = dmin<VMIN>(v, dpp_f64_nold<0x142, 0xA>(v));    // row_bcast:15 -> rows 1, 3
    v = dmin<VMIN>(v, dpp_f64_nold<0x143, 0xC>(v));    // row_bcast:31 -> row 3 holds all four
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// Orders one wave's LDS writes before its later LDS reads (one wave per workgroup: no instruction,
// a scheduling fence only).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One DPP stage of a (value, index) first-min reduction: the lane's pair is merged with the pair the
// move brings in (argmin_merge: strictly smaller, or equal with a lower index -- NaN never wins).
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ void argmin_dpp(float &v, int &a)
{
    const float v2 = __int_as_float(dpp_i32<CTRL, ROW_MASK>(__float_as_int(v)));
    const int a2 = dpp_i32<CTRL, ROW_MASK>(a);
    argmin_merge(v, a, v2, a2);
}

// (min, first argmin) over the 64 lanes, valid in lane 63 (same DPP butterfly as wave_min_f64)
__device__ __forceinline__ void wave_argmin(float &v, int &a)
{
    argmin_dpp<0xB1>(v, a);
    argmin_dpp<0x4E>(v, a);
    argmin_dpp<0x124>(v, a);
    argmin_dpp<0x128>(v, a);
    argmin_dpp<0x142, 0xA>(v, a);
    argmin_dpp<0x143, 0xC>(v, a);
}

}  // namespace sde
