// sgm.hip -- semi-global matching (gfx950): the penalties, the table of sgm_scan_kernel's forms with its
// dispatch, and the sde_sgm_* entry points.
//
// Replaces (process_functional.py):
//   sgm_penelty_kernel                :134-262
//   SGM_Interation + 8 SGM_*_kernel   :265-797  (launch order :1166-1203; the kernel is sgm_scan.h)
#include "sgm_scan.h"

namespace sde {

// One direction over one or two sides.  first: S := f32(0 + L) (no S read); du (direction 0 only):
// direction DU folded into the same pass; wta (direction 7 only): the final S is reduced to the disparity
// map (SgmSide::disp) instead of being stored; vmin: S holds no caller's -0.0 (see dmin).
struct SgmLaunch {
    SgmSide a, b;
    int nsides, H, W, D, dir;
    hipStream_t st;
    bool first, du, wta, vmin;
};

template <int DPL, bool VEC, bool FIRST, bool DU, bool WTA, bool VMIN, int DC, int DIRC>
static void launch_form(const SgmLaunch &L)
{
    constexpr int PF = DPL <= 4 ? 8 : 4;
    const bool horiz = (L.dir == 2 || L.dir == 3);
    const dim3 grid(horiz ? L.H : L.W, L.nsides);
    sgm_scan_kernel<DPL, PF, VEC, FIRST, DU, WTA, DC, DIRC, VMIN><<<grid, 64, 0, L.st>>>(L.a, L.b, L.H, L.W, L.D, L.dir);
}

// A kernel form: what it does, and what it fixes at compile time (dc: D, or 0; dirc: the direction, or -1).
struct ScanForm {
    bool first, du, wta, vmin;
    int dc, dirc;
    void (*launch)(const SgmLaunch &);
};

template <int DPL, bool VEC, bool FIRST, bool DU, bool WTA, bool VMIN, int DC, int DIRC>
constexpr ScanForm form()
{
    return {FIRST, DU, WTA, VMIN, DC, DIRC, launch_form<DPL, VEC, FIRST, DU, WTA, VMIN, DC, DIRC>};
}

// Every kernel that can run is named here once: per DPL, the seven forms for any D and direction (with
// vector loads where DPL divides D, else scalar ones; launch_dpl never asks for <1, false>),
//                             FIRST  DU     WTA    VMIN
template <int DPL, bool VEC>
constexpr ScanForm kForms[7] = {
    form<DPL, VEC, false, false, false, false, 0, -1>(),   // A  accumulate onto a caller's S    any direction
    form<DPL, VEC, false, false, false, true, 0, -1>(),    // B  middle passes                   1..7
    form<DPL, VEC, true, false, false, true, 0, -1>(),     // C  first pass, no fold             0
    form<DPL, VEC, true, true, false, true, 0, -1>(),      // D  first pass + DU fold            0
    form<DPL, VEC, false, true, false, false, 0, -1>(),    // E  accumulate + DU fold            0
    form<DPL, VEC, false, false, true, false, 0, -1>(),    // F  WTA after accumulate            7
    form<DPL, VEC, false, false, true, true, 0, -1>(),     // G  WTA                             7
};
// ... and for D = 64 DPL the v_min forms again with D a compile-time constant, and the direction too where
// the pair path (sgm_pair) launches them.  Form C's direction stays a run-time value.
template <int DPL>
constexpr ScanForm kFormsFullD[9] = {
    form<DPL, true, false, false, false, true, 64 * DPL, 2>(),     // B
    form<DPL, true, false, false, false, true, 64 * DPL, 3>(),
    form<DPL, true, false, false, false, true, 64 * DPL, 4>(),
    form<DPL, true, false, false, false, true, 64 * DPL, 5>(),
    form<DPL, true, false, false, false, true, 64 * DPL, 6>(),
    form<DPL, true, false, false, false, true, 64 * DPL, -1>(),    //    directions 1 and 7
    form<DPL, true, true, false, false, true, 64 * DPL, -1>(),     // C
    form<DPL, true, true, true, false, true, 64 * DPL, 0>(),       // D
    form<DPL, true, false, false, true, true, 64 * DPL, 7>(),      // G
};

// the first form of the list that does what L asks and fixes nothing L contradicts
template <int N>
static bool launch_first_match(const ScanForm (&forms)[N], const SgmLaunch &L)
{
    for (const ScanForm &f : forms) {
        if (f.first == L.first && f.du == L.du && f.wta == L.wta && f.vmin == L.vmin && (f.dc == 0 || f.dc == L.D) &&
            (f.dirc < 0 || f.dirc == L.dir)) {
            f.launch(L);
            return true;
        }
    }
    return false;
}

template <int DPL>
static bool launch_dpl(const SgmLaunch &L)
{
    if (L.D == 64 * DPL && launch_first_match(kFormsFullD<DPL>, L)) return true;
    // (DPL = 1: every D is a multiple -- the scalar-load forms are not instantiated)
    if constexpr (DPL > 1)
        if (L.D % DPL != 0) return launch_first_match(kForms<DPL, false>, L);
    return launch_first_match(kForms<DPL, true>, L);
}

// SDE_ERR_ARG: D beyond 512, or a combination that is no form (no entry point asks for one)
static int launch_scan(const SgmLaunch &L)
{
    bool ok = false;
    switch ((L.D + 63) / 64) {
    case 1: ok = launch_dpl<1>(L); break;
    case 2: ok = launch_dpl<2>(L); break;
    case 3: ok = launch_dpl<3>(L); break;
    case 4: ok = launch_dpl<4>(L); break;
    case 5: ok = launch_dpl<5>(L); break;
    case 6: ok = launch_dpl<6>(L); break;
    case 7: ok = launch_dpl<7>(L); break;
    case 8: ok = launch_dpl<8>(L); break;
    }
    return ok ? SDE_OK : SDE_ERR_ARG;
}

// sgm_penelty_kernel: reduced (P1/lambda, P2/lambda) iff uint64(nb - c) > thr as
// float64, i.e. nb < c or nb > c + thr; channels 0/1 never written (stay 0).
__global__ __launch_bounds__(256) void sgm_penalty_kernel(const uint8_t *__restrict__ img, int H, int W, float fP1,
                                                          float fP2, float rP1, float rP2, double thr,
                                                          float *__restrict__ pen)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p % W);
    const uint64_t c = img[p];
    const int dys[8] = {-1, +1, 0, 0, +1, +1, -1, -1};
    const int dxs[8] = {0, 0, -1, +1, -1, +1, +1, -1};
    const int chs[8] = {2, 2, 4, 6, 8, 10, 12, 14};
    float o[16];
    o[0] = 0.0f;
    o[1] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int yy = y + dys[k], xx = x + dxs[k];
        float a = fP1, b = fP2;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const uint64_t diff = (uint64_t)img[(size_t)yy * W + xx] - c;
            if ((double)diff > thr) { a = rP1; b = rP2; }
        }
        o[chs[k]] = a;
        o[chs[k] + 1] = b;
    }
    float4 *dst = reinterpret_cast<float4 *>(pen + p * 16);
#pragma unroll
    for (int i = 0; i < 4; i++) dst[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int sde_sgm_penalties(const uint8_t *img, int H, int W, double P1, double P2, int64_t threshold,
                                 double lambda, float *pen, void *stream)
{
    if (!img || !pen || H <= 0 || W <= 0 || lambda == 0.0) return SDE_ERR_ARG;
    const int64_t n = (int64_t)H * W;
    sgm_penalty_kernel<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(img, H, W, (float)P1, (float)P2,
                                                                     (float)(P1 / lambda), (float)(P2 / lambda),
                                                                     (double)threshold, pen);
    return launch_status();
}

SDE_EXPORT int sde_sgm_direction(const float *cv, const float *pen, int H, int W, int D, int direction, float *S,
                                 void *stream)
{
    if (!cv || !pen || !S || H < 2 || W < 2 || D <= 0 || D > 512 || direction < 0 || direction > 7)
        return SDE_ERR_ARG;
    const SgmSide a{cv, pen, S, nullptr};
    SgmLaunch L{};
    L.a = L.b = a;
    L.nsides = 1;
    L.H = H; L.W = W; L.D = D; L.dir = direction;
    L.st = as_stream(stream);
    // form A: S is the caller's (it may hold -0.0: no v_min, see dmin)
    L.first = false; L.du = false; L.wta = false; L.vmin = false;
    const int s = launch_scan(L);
    if (s != SDE_OK) return s;
    return launch_status();
}

SDE_EXPORT int sde_sgm_8path(const float *cv, const float *pen, int H, int W, int D, float *S, void *stream)
{
    return sde_sgm_8path_pair(cv, pen, S, nullptr, nullptr, nullptr, H, W, D, SDE_SGM_ACCUMULATE, stream);
}

static int sgm_pair(const float *cv_l, const float *pen_l, float *S_l, float *disp_l, const float *cv_r,
                    const float *pen_r, float *S_r, float *disp_r, int H, int W, int D, int flags, bool wta,
                    hipStream_t st)
{
    if (!cv_l || !pen_l || !S_l || H < 2 || W < 2 || D <= 0 || D > 512 ||
        (flags & ~(SDE_SGM_ACCUMULATE | SDE_SGM_ZERO_DU_PENALTIES)))
        return SDE_ERR_ARG;
    const bool two = cv_r || pen_r || S_r;
    if (two && (!cv_r || !pen_r || !S_r)) return SDE_ERR_ARG;
    if (wta && (!disp_l || (two && !disp_r))) return SDE_ERR_ARG;
    SgmLaunch L{};
    L.a = SgmSide{cv_l, pen_l, S_l, disp_l};
    L.b = two ? SgmSide{cv_r, pen_r, S_r, disp_r} : L.a;
    L.nsides = two ? 2 : 1;
    L.H = H; L.W = W; L.D = D;
    L.st = st;
    const bool fold_du = (flags & SDE_SGM_ZERO_DU_PENALTIES) != 0;
    // the caller's S is accumulated onto (ACCUMULATE): it may hold -0.0 -- no v_min (see dmin)
    const bool overwrite = !(flags & SDE_SGM_ACCUMULATE);
    L.vmin = overwrite;
    for (int dir = 0; dir < 8; dir++) {
        if (dir == 1 && fold_du) continue;      // applied in the UD pass
        L.dir = dir;
        L.first = dir == 0 && overwrite;        // overwrite: form C, with the fold D    (then B, and G if wta)
        L.du = dir == 0 && fold_du;             // accumulate: form A, with the fold E   (then A, and F if wta)
        L.wta = dir == 7 && wta;
        const int s = launch_scan(L);
        if (s != SDE_OK) return s;
    }
    return launch_status();
}

SDE_EXPORT int sde_sgm_8path_pair(const float *cv_l, const float *pen_l, float *S_l, const float *cv_r,
                                  const float *pen_r, float *S_r, int H, int W, int D, int flags, void *stream)
{
    return sgm_pair(cv_l, pen_l, S_l, nullptr, cv_r, pen_r, S_r, nullptr, H, W, D, flags, false, as_stream(stream));
}

SDE_EXPORT int sde_sgm_8path_wta_pair(const float *cv_l, const float *pen_l, float *S_l, float *disp_l,
                                      const float *cv_r, const float *pen_r, float *S_r, float *disp_r, int H, int W,
                                      int D, int flags, void *stream)
{
    return sgm_pair(cv_l, pen_l, S_l, disp_l, cv_r, pen_r, S_r, disp_r, H, W, D, flags, true, as_stream(stream));
}
