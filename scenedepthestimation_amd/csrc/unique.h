// unique.h -- what the uniqueness check's kernels share (definition: include/sde_unique.h; DESIGN.md
// sec. 3.12): the one-pass runner-up bookkeeping, the decision, and the launchers of unique.hip and cv_row.hip that
// sdu_cv_wta_unique (cv_wta.hip) dispatches to.  Build-defined: the reference has no such stage.
#pragma once

#include "sde_common.h"

namespace sde {

// The runner-up is the smallest cost outside {i - 1, i, i + 1}, and i is known only once the scan is over.  So a
// scan keeps, for a set of disparities of which no two are closer than 3 apart (a residue class of d modulo 4 or
// more, or any subset of one), its smallest cost b1, where it first took it (a1) and its second smallest b2
// (counting duplicates).  At most one member of {i - 1, i, i + 1} is in such a set, so the set's smallest cost
// outside the three is b2 if a1 is one of them and b1 otherwise -- when the excluded member ties with b1 without
// being a1, a1 itself is allowed and has the same value.  NaN never enters (both compares are false).
struct UqChain {
    float b1, b2;
    int a1;
    __device__ __forceinline__ void init()
    {
        b1 = __builtin_inff();
        b2 = __builtin_inff();
        a1 = -1;
    }
    // d ascending within the set: a1 is the set's first minimum
    __device__ __forceinline__ void take(float v, int d)
    {
        if (v < b1) {
            b2 = b1;
            b1 = v;
            a1 = d;
        } else if (v < b2) {
            b2 = v;
        }
    }
    // the set's smallest cost at |d - i| >= 2 (+inf if none; an empty set holds a1 = -1 and b1 = b2 = +inf)
    __device__ __forceinline__ float outside(int i) const { return (a1 - i <= 1 && i - a1 <= 1) ? b2 : b1; }
};

// margin and decision of a pixel whose winner has cost c1 and whose runner-up is c2 (has = false: no winner)
__device__ __forceinline__ float uq_margin(bool has, float c1, float c2)
{
    if (!has) return 0.0f;
    const float m = c2 == c1 ? 0.0f : c2 - c1;
    // NaN only when c1 is NaN (SDE_WTA_INIT_D0 with a NaN at d = 0): the canonical quiet NaN, whatever sign and
    // payload the subtraction's operand order would propagate
    return m != m ? __uint_as_float(0x7fc00000u) : m;
}

// tau: a finite float32 >= 0 (false for NaN)
static inline bool uq_tau_ok(float tau) { return tau >= 0.0f && tau <= 3.4028234663852886e38f; }

// exact fused form (unique.hip): cv64_kernel's costs for C == 64, the generic one-thread-per-pixel form otherwise
void launch_cv_unique_exact(bool right, const float *fl, const float *fr, int H, int W, int C, int d0, int d1,
                            float tau, float *disp, float *min_cost, int32_t *argmin, uint8_t *reject,
                            hipStream_t st);

// the row sweep's uniqueness instantiations (cv_row.hip): as launch_row_cert, plus tau and the reject map
void launch_row_cert_unique(const float *fl, const float *fr, int H, int W, int d0, int d1, float tau, float *out_min,
                            int32_t *out_arg, float *out_disp, uint8_t *out_rej, unsigned *counter, int32_t *list,
                            hipStream_t st, bool mirror);

}  // namespace sde
