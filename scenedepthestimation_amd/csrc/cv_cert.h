// cv_cert.h -- the certificate of the fused cost volume + WTA (north-star kernel) and what its two sweeps
// share: the row sweep (cv_row.hip) and the pre-split tile path (cv_tile.h).
//
// Scores s(x,d) = fl[x] . fr[x-d] are computed on the bf16 MFMA (v_mfma_f32_32x32x16_bf16; the row sweep uses
// fp16 parts and its own, tighter constant: see cv_row.hip) with every fp32 operand split into hi + lo parts and
// the three leading partial products (hh, hl, lh) accumulated in fp32.  Rigorous bound for every voxel of a
// pixel (Cauchy-Schwarz on |a|,|b|):
//   |s_fast - s_true| <= (3*2^-16 + 192*2^-23) * sum|a_c b_c|   (split + accumulation)
//   |s_exact - s_true| <= 10*2^-24 * sum|a_c b_c|               (NumPy pairwise order)
//   => |s_fast - s_exact| <= FX_K * sum|a_c b_c| <= FX_K * ||fl[x]||_2 * max_window ||fr||_2
//      (FX_K = 1e-4: 1.4x margin over 7e-5; the per-pixel L2 norms are fp32 sums of
//      squares inflated by FX_NORM_UP = 1 + 4e-6, an upper bound)
// If the best fast score beats the runner-up by more than 2 eps, the exact first-min is provably the fast
// argmax (no other d can tie or win exactly), and its exact cost is computed once (same arithmetic as
// cv64_kernel, cv_exact.h).  Any other pixel (near-ties, NaN/Inf features) goes to a work list that
// cv_wta_fixup_kernel (cv_wta.hip) resolves with the exact scan.  Outputs are therefore bit-identical to
// the exact kernel for every input.
#pragma once

#include "sde_common.h"

namespace sde {

typedef __bf16 fx_bf16x8 __attribute__((ext_vector_type(8)));
typedef float fx_floatx16 __attribute__((ext_vector_type(16)));

constexpr int FX_NX = 64;          // left pixels per workgroup
constexpr float FX_K = 1e-4f;
constexpr float FX_ABS = 1e-30f;   // absolute slack (bf16 subnormal handling)
constexpr float FX_NORM_UP = 1.000004f;

__device__ __forceinline__ int fx_slot(int r, int c8) { return r * 8 + (c8 ^ ((r >> 1) & 7)); }

// merge (best, arg, second) of two disjoint candidate sets, scores in max-domain
__device__ __forceinline__ void fx_merge(float &b, int &a, float &s, float b2, int a2, float s2)
{
    const float ns = fmaxf(fminf(b, b2), fmaxf(s, s2));
    if (b2 > b || (b2 == b && a2 < a)) { b = b2; a = a2; }
    s = ns;
}

// the row-sweep kernel (cv_row.hip): window size limit and launcher (mirror: the right view)
bool row_cert_supported(int d0, int d1);
void launch_row_cert(const float *fl, const float *fr, int H, int W, int d0, int d1, float *out_min, int32_t *out_arg,
                     float *out_disp, unsigned *counter, int32_t *list, hipStream_t st, const float *prev_min = nullptr,
                     bool mirror = false);

}  // namespace sde
