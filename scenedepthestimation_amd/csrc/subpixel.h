// subpixel.h -- the parabola step of the sub-pixel disparities (wta.hip: over a stored volume; refine.hip: over
// costs recomputed from the features).  Replaces process_functional.py:813-819 / :830-836.
#pragma once

#include "sde_common.h"

namespace sde {

// Numba's promotion of `index - (c_ - _c)/(2*(_c + c_ - 2*c))` (:818): the difference and the sum of the two
// neighbours are float32, `2*c` is int64 * float32 = float64 and everything after it is float64.  The three
// guards (an interior winner, finite costs, a convex parabola) keep the integer; there is no clamp.
__device__ __forceinline__ float refine(int i, int lo, int hi, float cm, float c0, float cp)
{
    float r = (float)i;
    if (i > lo && i < hi - 1 && finite_f32(cm) && finite_f32(c0) && finite_f32(cp)) {
        const float num = cp - cm;
        const float s = cm + cp;
        const double den = 2.0 * ((double)s - 2.0 * (double)c0);
        if (den > 0.0) r = (float)((double)i - (double)num / den);
    }
    return r;
}

}  // namespace sde
