// cv_wta.hip -- the fused cost volume + WTA entry points (gfx950): sde_cv_wta*, sde_feature_split, their
// workspace sizes, and sde_argmin_merge.  Replaces (WHDY/SceneDepthEstimation) compute_cost_volume + WTA1,
// process_functional.py:48-73 + 96-113, fused.  Exact mode launches cv_exact.h's kernels; certified mode
// (cv_cert.h) the row sweep of cv_row.hip or the tile path of cv_tile.h, then the exact fix-ups (below).
#include "cv_tile.h"
#include "unique.h"
#include "sde_unique.h"

#include <algorithm>

namespace sde {

// Merge of per-range first minima: the disparity shards of sde_argmin_merge and the chunks of the chunked
// certified CV + WTA (sde_cv_wta, D past one row sweep's LDS window).  Chunk k's exact first-minimum
// (value, index) per pixel at mins / args + k * npix, chunks ordered by d; the pixel's first minimum over
// all of them (strict <: a later chunk wins only with a smaller cost, ties keep the earlier one -- a
// sequential scan over d), written to whichever outputs are requested.
__global__ __launch_bounds__(256) void argmin_chunks_kernel(const float *__restrict__ mins,
                                                            const int32_t *__restrict__ args, int nchunks,
                                                            int64_t npix, float *__restrict__ disp,
                                                            float *__restrict__ out_min, int32_t *__restrict__ out_arg)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    float best = mins[p];
    int arg = args[p];
    for (int k = 1; k < nchunks; k++) {
        const float m = mins[(size_t)k * npix + p];
        if (m < best) { best = m; arg = args[(size_t)k * npix + p]; }
    }
    if (disp) disp[p] = (float)arg;
    if (out_min) out_min[p] = best;
    if (out_arg) out_arg[p] = arg;
}

// Exact resolution of the listed pixels, one 4-wave workgroup per pixel (persistent over the list).
// Wave v takes disparities [d0 + vQ, d0 + (v+1)Q), Q = 8 ceil(D / 32); each of its 8 lane groups of 8
// takes one disparity per iteration, lane jj of a group the products of channels 8m + jj, m = 0..7, in
// order -- dot64_exact_global's partial sum acc[jj] -- and the group's xor butterfly adds the 8 partial
// sums in that function's tree order (adds are commutative: the same bits).  A group scans its
// disparities in increasing d with a strict <, then (value, index) merges over the groups and the waves
// give the sequential first minimum.  All of a wave's iterations are in flight at once up to D = 256 (a
// chunk): one round of loads per pixel instead of a lane's three to four dependent 16-load dots, whose
// 64 lanes each read another pixel's 256 B (64 cache lines per load instruction).
// RIGHT: the right view's scan -- the listed pixel x owns own[p] = fr[p], the other operand is fl at x + d, valid
// iff x + d < W (the load index is clamped, as x - d is in the left form); the same per-disparity arithmetic
// (the products commute) and merge order.  own / other: (fl, fr) for the left view, (fr, fl) for the right.
// UNIQ: the uniqueness check's resolution (include/sde_unique.h).  A lane's disparities are 8 apart (d = d0 + g modulo 8:
// Q and the rounds are multiples of 8), one chain of unique.h, taken by all 8 lanes of the group alike; once the
// winner is merged every lane takes its chain's smallest cost outside the winner's neighbourhood, and the minimum
// over the groups and the waves is the runner-up: i, c1, c2 and the decision of the exact form, from the same scan.
constexpr int FX2_U = 8;   // iterations per round of loads
template <bool RIGHT, bool UNIQ = false>
__global__ __launch_bounds__(256) void cv_wta_fixup_kernel(const float *__restrict__ own,
                                                           const float *__restrict__ other, int W, int d0, int d1, const unsigned *__restrict__ counter,
                                                           const int32_t *__restrict__ list, float *__restrict__ out_min,
                                                           int32_t *__restrict__ out_arg, float *__restrict__ out_disp,
                                                           float tau, uint8_t *__restrict__ out_rej)
{
    __shared__ float wb[4];
    __shared__ int wa[4];
    __shared__ float w2[UNIQ ? 4 : 1];
    const unsigned cnt = *counter;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 3, jj = lane & 7;
    const int Q = (d1 - d0 + 31) / 32 * 8;
    const int dw = d0 + wave * Q, dwe = min(d1, dw + Q);
    for (unsigned e = blockIdx.x; e < cnt; e += gridDim.x) {
        const size_t p = (size_t)list[e];
        const int x = (int)(p % W);
        const size_t rowbase = p - x;
        float av[8];
#pragma unroll
        for (int m = 0; m < 8; m++) av[m] = own[p * 64 + 8 * m + jj];
        float best = __builtin_inff();
        int arg = -1;
        UqChain ch;
        ch.init();
        for (int db = dw; db < dwe; db += 8 * FX2_U) {
            float bv[FX2_U][8];
#pragma unroll
            for (int u = 0; u < FX2_U; u++) {
                const int xr = RIGHT ? x + (db + 8 * u + g) : x - (db + 8 * u + g);
                const float *b = other + (rowbase + (RIGHT ? (xr < W ? xr : W - 1) : (xr >= 0 ? xr : 0))) * 64 + jj;
#pragma unroll
                for (int m = 0; m < 8; m++) bv[u][m] = b[8 * m];
            }
#pragma unroll
            for (int u = 0; u < FX2_U; u++) {
                const int d = db + 8 * u + g;
                float acc = av[0] * bv[u][0];
#pragma unroll
                for (int m = 1; m < 8; m++) acc = acc + av[m] * bv[u][m];
                acc = acc + __shfl_xor(acc, 1, 64);   // (acc0 + acc1), (acc2 + acc3), ...
                acc = acc + __shfl_xor(acc, 2, 64);   // ((acc0 + acc1) + (acc2 + acc3)), ...
                acc = acc + __shfl_xor(acc, 4, 64);
                const float c = (RIGHT ? x + d < W : x - d >= 0) ? -(0.0f + acc) : -0.0f;
                if constexpr (UNIQ) {
                    if (d < dwe) ch.take(c, d);
                } else if (d < dwe && c < best) {
                    best = c;
                    arg = d;
                }
            }
        }
        if constexpr (UNIQ) {
            best = ch.b1;
            arg = ch.a1;
        }
#pragma unroll
        for (int off = 8; off < 64; off <<= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oa = __shfl_xor(arg, off, 64);
            argmin_merge(best, arg, ob, oa);
        }
        if (lane == 0) {
            wb[wave] = best;
            wa[wave] = arg;
        }
        __syncthreads();
        if constexpr (UNIQ) {
            best = wb[0];
            arg = wa[0];
#pragma unroll
            for (int v = 1; v < 4; v++) argmin_merge(best, arg, wb[v], wa[v]);
            float c2 = ch.outside(arg);
#pragma unroll
            for (int off = 8; off < 64; off <<= 1) c2 = fminf(c2, __shfl_xor(c2, off, 64));
            if (lane == 0) w2[wave] = c2;
            __syncthreads();
            if (threadIdx.x == 0) {
                c2 = fminf(fminf(w2[0], w2[1]), fminf(w2[2], w2[3]));
                const bool has = arg >= 0;
                const bool rej = has && uq_margin(has, best, c2) < tau;
                if (out_min) out_min[p] = best;
                if (out_arg) out_arg[p] = arg;
                if (out_disp) out_disp[p] = rej ? -1.0f : (float)arg;
                if (out_rej) out_rej[p] = rej ? 1 : 0;
            }
        } else if (threadIdx.x == 0) {
            best = wb[0];
            arg = wa[0];
#pragma unroll
            for (int v = 1; v < 4; v++) argmin_merge(best, arg, wb[v], wa[v]);
            if (out_min) out_min[p] = best;
            if (out_arg) out_arg[p] = arg;
            if (out_disp) out_disp[p] = (float)arg;
        }
        __syncthreads();
    }
}

}  // namespace sde

using namespace sde;

// certified-mode workspace: [counters 256 B][fix-up list 4*npix], then for sde_cv_wta the (min, arg) planes of
// up to CERT_COUNTERS disparity chunks, 8 B per pixel each: 512*npix covers every K <= 64 (plus two rows of
// 4*npix that earlier layouts used: callers size buffers by the byte counts, which therefore stay).  The fix-up
// count of a call is the sum of the 64 counter words (one per chunk).
constexpr int CERT_COUNTERS = 64;
static int64_t cert_ws_bytes(int H, int W, bool with_chunks)
{
    const int64_t npix = (int64_t)H * W;
    int64_t b = 256 + ((4 * npix + 255) / 256) * 256;
    if (with_chunks) b += 4 * 128 * npix + 2 * ((4 * npix + 255) / 256) * 256;
    return b;
}

// that layout as pointers (K chunk planes of min, then K of arg: in sde_cv_wta's workspace only)
struct CertWs { unsigned *counter; int32_t *list; float *chunk_min; int32_t *chunk_arg; };
static CertWs cert_ws(void *workspace, int H, int W, int K)
{
    char *base = reinterpret_cast<char *>(workspace);
    float *cmin = reinterpret_cast<float *>(base + cert_ws_bytes(H, W, false));
    return {reinterpret_cast<unsigned *>(base), reinterpret_cast<int32_t *>(base + 256), cmin,
            reinterpret_cast<int32_t *>(cmin + (size_t)K * H * W)};
}

SDE_EXPORT int64_t sde_cv_wta_workspace_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return -1;
    return cert_ws_bytes(H, W, true);
}

SDE_EXPORT int64_t sde_cv_wta_split_workspace_bytes(int H, int W)
{
    if (H <= 0 || W <= 0) return -1;
    return cert_ws_bytes(H, W, false);
}

SDE_EXPORT int sde_feature_split(const float *feat, int64_t npix, int C, uint16_t *hi, uint16_t *lo, float *norm,
                                 void *stream)
{
    if (!feat || !hi || !lo || !norm || npix <= 0 || C != 64) return SDE_ERR_ARG;
    feature_split_kernel<<<cdiv(npix * 16, 256), 256, 0, as_stream(stream)>>>(feat, npix, hi, lo, norm);
    return launch_status();
}

SDE_EXPORT int sde_cv_wta_split(const float *fl, const float *fr, const uint16_t *fl_hi, const uint16_t *fl_lo,
                                const float *fl_norm, const uint16_t *fr_hi, const uint16_t *fr_lo,
                                const float *fr_norm, int H, int W, int d0, int d1, float *disp, float *min_cost,
                                int32_t *argmin, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!fl || !fr || !fl_hi || !fl_lo || !fl_norm || !fr_hi || !fr_lo || !fr_norm) return SDE_ERR_ARG;
    if (H <= 0 || W <= 0 || d0 < 0 || d1 <= d0 || (!disp && !min_cost && !argmin)) return SDE_ERR_ARG;
    if (!workspace || workspace_bytes < cert_ws_bytes(H, W, false)) return SDE_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    const CertWs ws = cert_ws(workspace, H, W, 0);
    if (hipMemsetAsync(ws.counter, 0, CERT_COUNTERS * sizeof(unsigned), st) != hipSuccess) return SDE_ERR_LAUNCH;
    cv_wta_cert_kernel<<<cdiv(W, FX_NX) * H, 256, 0, st>>>(
        fl, fr, reinterpret_cast<const uint4 *>(fl_hi), reinterpret_cast<const uint4 *>(fl_lo), fl_norm,
        reinterpret_cast<const uint4 *>(fr_hi), reinterpret_cast<const uint4 *>(fr_lo), fr_norm, H, W, d0, d1,
        min_cost, argmin, disp, ws.counter, ws.list);
    cv_wta_fixup_kernel<false><<<1024, 256, 0, st>>>(fl, fr, W, d0, d1, ws.counter, ws.list, min_cost, argmin, disp,
                                                      0.0f, nullptr);
    return launch_status();
}

// disparities per chunk of the chunked row sweep.  A chunk spans 128 + 256 - 1 right pixels per superstrip, at
// most 13 tiles of 32 whatever its first disparity: every chunk fits the row sweep's ring (row_cert_supported)
constexpr int ROW_CHUNK = 256;

// sde_cv_wta (right = false) and sde_cv_wta_right: the same dispatch, workspace and chunk loop; the right view
// runs the mirrored row sweep, the right-view fix-up and the exact kernels' SDE_SIDE_RIGHT forms
static int cv_wta_view(bool right, const float *fl, const float *fr, int H, int W, int C, int d0, int d1, float *disp,
                       float *min_cost, int32_t *argmin, int mode, void *workspace, int64_t workspace_bytes,
                       void *stream)
{
    if (!fl || !fr || H <= 0 || W <= 0 || C <= 0 || d0 < 0 || d1 <= d0) return SDE_ERR_ARG;
    if (!disp && !min_cost && !argmin) return SDE_ERR_ARG;
    if (mode != SDE_CV_EXACT && mode != SDE_CV_CERTIFIED) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    auto exact64 = [&] {
        dim3 grid(cdiv(W, CV_TX), H);
        if (right)
            cv64_kernel<SDE_SIDE_RIGHT, OUT_WTA><<<grid, 256, 0, st>>>(fr, fl, H, W, d0, d1, 0, -0.0f, nullptr,
                                                                        min_cost, argmin, disp);
        else
            cv64_kernel<SDE_SIDE_LEFT, OUT_WTA><<<grid, 256, 0, st>>>(fl, fr, H, W, d0, d1, 0, -0.0f, nullptr,
                                                                       min_cost, argmin, disp);
    };
    // exact resolution of the pixels a sweep over [a, b) listed
    auto fixup = [&](int a, int b, unsigned *cnt, const int32_t *lst, float *mn, int32_t *ag, float *dp) {
        if (right) cv_wta_fixup_kernel<true><<<1024, 256, 0, st>>>(fr, fl, W, a, b, cnt, lst, mn, ag, dp, 0.0f, nullptr);
        else cv_wta_fixup_kernel<false><<<1024, 256, 0, st>>>(fl, fr, W, a, b, cnt, lst, mn, ag, dp, 0.0f, nullptr);
    };
    if (C == 64 && mode == SDE_CV_CERTIFIED) {
        // The row-sweep kernel straight from the fp32 features (cv_row.hip) + the exact fix-ups of the pixels it
        // lists: one sweep where [d0, d1) fits its ring, else ROW_CHUNK-disparity chunks (e.g. BASELINE config
        // 5, D = 512) and the first minimum over the chunks in d order.  A range of more than CERT_COUNTERS
        // chunks (D > 16384) takes the exact kernel: the certificate's contract is the exact kernel's outputs
        // bit for bit, so only the speed differs, and the zeroed counters report no fix-ups.
        if (!workspace || workspace_bytes < sde_cv_wta_workspace_bytes(H, W)) return SDE_ERR_WORKSPACE;
        const int64_t npix = (int64_t)H * W;
        const int K = cdiv(d1 - d0, ROW_CHUNK);
        const CertWs ws = cert_ws(workspace, H, W, K <= CERT_COUNTERS ? K : 0);
        if (hipMemsetAsync(ws.counter, 0, CERT_COUNTERS * sizeof(unsigned), st) != hipSuccess) return SDE_ERR_LAUNCH;
        if (row_cert_supported(d0, d1)) {
            launch_row_cert(fl, fr, H, W, d0, d1, min_cost, argmin, disp, ws.counter, ws.list, st, nullptr, right);
            fixup(d0, d1, ws.counter, ws.list, min_cost, argmin, disp);
        } else if (K <= CERT_COUNTERS) {
            // each chunk's outputs are the exact kernel's on its range (as for the disparity shards of
            // parallel.py).  Chunk k counts its fix-ups in counter word k; the list is reused: chunk k's fix-ups
            // run before chunk k + 1's sweep
            for (int k = 0; k < K; k++) {
                const int a = d0 + k * ROW_CHUNK, b = std::min(d1, a + ROW_CHUNK);
                float *mk = ws.chunk_min + (size_t)k * npix;
                int32_t *ak = ws.chunk_arg + (size_t)k * npix;
                launch_row_cert(fl, fr, H, W, a, b, mk, ak, nullptr, ws.counter + k, ws.list, st,
                                k > 0 ? mk - npix : nullptr, right);
                fixup(a, b, ws.counter + k, ws.list, mk, ak, nullptr);
            }
            argmin_chunks_kernel<<<cdiv(npix, 256), 256, 0, st>>>(ws.chunk_min, ws.chunk_arg, K, npix, disp, min_cost,
                                                                   argmin);
        } else {
            exact64();
        }
    } else if (C == 64) {
        exact64();
    } else {
        const int blocks = cdiv((int64_t)H * W, 256);
        cv_generic_kernel<OUT_WTA><<<blocks, 256, 0, st>>>(fl, fr, H, W, C, d0, d1, 0,
                                                            right ? SDE_SIDE_RIGHT : SDE_SIDE_LEFT, -0.0f, nullptr,
                                                            nullptr, min_cost, argmin, disp);
    }
    return launch_status();
}

SDE_EXPORT int sde_cv_wta(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, float *disp,
                          float *min_cost, int32_t *argmin, int mode, void *workspace, int64_t workspace_bytes,
                          void *stream)
{
    return cv_wta_view(false, fl, fr, H, W, C, d0, d1, disp, min_cost, argmin, mode, workspace, workspace_bytes,
                       stream);
}

SDE_EXPORT int sde_cv_wta_right(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, float *disp,
                                float *min_cost, int32_t *argmin, int mode, void *workspace, int64_t workspace_bytes,
                                void *stream)
{
    return cv_wta_view(true, fl, fr, H, W, C, d0, d1, disp, min_cost, argmin, mode, workspace, workspace_bytes,
                       stream);
}

// sdu_cv_wta_unique: cv_wta_view's dispatch with the uniqueness check.  Certified mode covers one row sweep
// (row_cert_supported); a wider range takes the exact form, which gives the same bytes, with the counters zeroed --
// the precedent of ranges past CERT_COUNTERS chunks (carrying the runner-up across chunk merges is not built).
SDE_EXPORT int sdu_cv_wta_unique(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, int side,
                                 float tau, float *disp, float *min_cost, int32_t *argmin, uint8_t *reject, int mode,
                                 void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!fl || !fr || H <= 0 || W <= 0 || C <= 0 || d0 < 0 || d1 <= d0) return SDE_ERR_ARG;
    if (!disp && !min_cost && !argmin && !reject) return SDE_ERR_ARG;
    if (mode != SDE_CV_EXACT && mode != SDE_CV_CERTIFIED) return SDE_ERR_ARG;
    if (side != SDE_SIDE_LEFT && side != SDE_SIDE_RIGHT) return SDE_ERR_ARG;
    if (!uq_tau_ok(tau)) return SDE_ERR_ARG;
    const bool right = side == SDE_SIDE_RIGHT;
    hipStream_t st = as_stream(stream);
    if (C == 64 && mode == SDE_CV_CERTIFIED) {
        if (!workspace || workspace_bytes < sde_cv_wta_workspace_bytes(H, W)) return SDE_ERR_WORKSPACE;
        const CertWs ws = cert_ws(workspace, H, W, 0);
        if (hipMemsetAsync(ws.counter, 0, CERT_COUNTERS * sizeof(unsigned), st) != hipSuccess) return SDE_ERR_LAUNCH;
        if (row_cert_supported(d0, d1)) {
            launch_row_cert_unique(fl, fr, H, W, d0, d1, tau, min_cost, argmin, disp, reject, ws.counter, ws.list, st,
                                   right);
            if (right)
                cv_wta_fixup_kernel<true, true><<<1024, 256, 0, st>>>(fr, fl, W, d0, d1, ws.counter, ws.list, min_cost,
                                                                       argmin, disp, tau, reject);
            else
                cv_wta_fixup_kernel<false, true><<<1024, 256, 0, st>>>(fl, fr, W, d0, d1, ws.counter, ws.list, min_cost,
                                                                        argmin, disp, tau, reject);
        } else {
            launch_cv_unique_exact(right, fl, fr, H, W, 64, d0, d1, tau, disp, min_cost, argmin, reject, st);
        }
    } else {
        launch_cv_unique_exact(right, fl, fr, H, W, C, d0, d1, tau, disp, min_cost, argmin, reject, st);
    }
    return launch_status();
}

SDE_EXPORT int sde_argmin_merge(const float *mins, const int32_t *args, int nshards, int64_t npix, float *disp,
                                void *stream)
{
    if (!mins || !args || !disp || nshards <= 0 || npix <= 0) return SDE_ERR_ARG;
    argmin_chunks_kernel<<<cdiv(npix, 256), 256, 0, as_stream(stream)>>>(mins, args, nshards, npix, disp, nullptr,
                                                                         nullptr);
    return launch_status();
}
