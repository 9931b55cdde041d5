// tower_pack.hip -- host-only: packs the tower's HWIO weights into the blob the kernels read (tower_blob.h).
#include "sde.h"
#include "tower_blob.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#define SDE_EXPORT extern "C" __attribute__((visibility("default")))   // as sde_common.h (HIP, not included here)

using namespace sde;

static uint16_t f2bf_rne(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

static float bf2f(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

SDE_EXPORT int64_t sde_tower_packed_floats(int nlayers, int nf)
{
    if (nlayers < 1 || nf != NF) return -1;
    return (int64_t)L1_FLOATS + (int64_t)(nlayers - 1) * LK_FLOATS;
}

SDE_EXPORT int sde_tower_pack_weights(const float *const *hwio, const float *const *biases, int nlayers, int nf,
                                      float *packed)
{
    if (!hwio || !biases || !packed || nlayers < 1 || nf != NF) return SDE_ERR_ARG;
    float *o = packed;
    // layer 1: HWIO [3][3][1][64] is already [tap][n]
    for (int n = 0; n < NF; n++) o[n] = biases[0][n];
    for (int i = 0; i < 9 * NF; i++) o[NF + i] = hwio[0][i];
    o += L1_FLOATS;
    // conv1 output bound terms for the F16 scaling (layer 2 computes conv1)
    float l1 = 0.0f, bmax = 0.0f;
    for (int n = 0; n < NF; n++) {
        double s = 0.0;
        for (int t = 0; t < 9; t++) s += std::fabs((double)hwio[0][t * NF + n]);
        l1 = std::max(l1, (float)(s * (1.0 + 1e-6)));   // rounded up: a bound of the f32 conv1
        bmax = std::max(bmax, std::fabs(biases[0][n]));
    }
    for (int l = 1; l < nlayers; l++) {
        for (int n = 0; n < NF; n++) o[n] = biases[l][n];
        float *w = o + NF;
        uint16_t *pl = reinterpret_cast<uint16_t *>(w + LK_W);
        // F16 parts of W * 2^tau, max |W| * 2^tau in [2^14, 2^15)
        float wmax = 0.0f;
        for (size_t i = 0; i < (size_t)LK_W; i++) wmax = std::max(wmax, std::fabs(hwio[l][i]));
        const int tau = (wmax > 0.0f && std::isfinite(wmax)) ? std::min(std::max(14 - std::ilogb(wmax), -100), 100) : 0;
        _Float16 *ph = reinterpret_cast<_Float16 *>(o + LK_F16);
        float *hdr = o + LK_F16 + LK_W;
        hdr[0] = std::ldexp(1.0f, -tau);
        hdr[1] = l1;
        hdr[2] = bmax;
        hdr[3] = 0.0f;
        {   // this layer's output bound terms (rounded up: bounds of the f32 sums)
            float lk = 0.0f, bk = 0.0f;
            for (int n = 0; n < NF; n++) {
                double s = 0.0;
                for (int i = 0; i < 9 * NF; i++) s += std::fabs((double)hwio[l][(size_t)i * NF + n]);
                lk = std::max(lk, (float)(s * (1.0 + 1e-6)));
                bk = std::max(bk, std::fabs(biases[l][n]));
            }
            hdr[4] = lk;
            hdr[5] = bk;
            hdr[6] = hdr[7] = 0.0f;
        }
        {
            // Winograd U = G g G^T per (n, c) in fp64, scaled by 2^tau_u (max |U| 2^tau_u in [2^14, 2^15)) and
            // split into two fp16 parts (the residual taken in fp64)
            static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
            std::vector<double> U((size_t)16 * NF * NF);
            double umax = 0.0;
            for (int c = 0; c < NF; c++)
                for (int n = 0; n < NF; n++) {
                    double g[3][3];
                    for (int ky = 0; ky < 3; ky++)
                        for (int kx = 0; kx < 3; kx++) g[ky][kx] = hwio[l][((size_t)(ky * 3 + kx) * NF + c) * NF + n];
                    for (int i = 0; i < 4; i++)
                        for (int j = 0; j < 4; j++) {
                            double u = 0.0;
                            for (int ky = 0; ky < 3; ky++)
                                for (int kx = 0; kx < 3; kx++) u += G[i][ky] * g[ky][kx] * G[j][kx];
                            U[((size_t)(4 * i + j) * NF + n) * NF + c] = u;
                            umax = std::max(umax, std::fabs(u));
                        }
                }
            const int tu = (umax > 0.0 && std::isfinite(umax)) ? std::min(std::max(14 - std::ilogb(umax), -100), 100) : 0;
            _Float16 *pu = reinterpret_cast<_Float16 *>(o + LK_WINO);
            float *wh = o + LK_WHDR;
            wh[0] = std::ldexp(1.0f, -tu);
            wh[1] = wh[2] = wh[3] = 0.0f;
            for (int xi = 0; xi < 16; xi++)
                for (int n = 0; n < NF; n++)
                    for (int c = 0; c < NF; c++) {
                        const double x = std::ldexp(U[((size_t)xi * NF + n) * NF + c], tu);
                        const _Float16 h0 = (_Float16)x;
                        const _Float16 parts[2] = {h0, (_Float16)(x - (double)h0)};
                        const int mt = n >> 5, cb = c >> 4, ln = ((c >> 3) & 1) * 32 + (n & 31);
                        for (int q = 0; q < 2; q++)
                            pu[((((size_t)(xi * 2 + mt) * LK_NCB + cb) * 2 + q) * 64 + ln) * 8 + (c & 7)] = parts[q];
                    }
        }
        for (int tap = 0; tap < 9; tap++)
            for (int c = 0; c < NF; c++)
                for (int n = 0; n < NF; n++) {
                    const size_t dsti = ((size_t)tap * NF + n) * NF + c;
                    const float x = hwio[l][((size_t)tap * NF + c) * NF + n];
                    w[dsti] = x;
                    const uint16_t h0 = f2bf_rne(x);
                    const float r1 = x - bf2f(h0);
                    const uint16_t h1 = f2bf_rne(r1);
                    const float r2 = r1 - bf2f(h1);
                    const uint16_t parts[3] = {h0, h1, f2bf_rne(r2)};
                    // A-fragment order [mtile][cblock][tap][part][lane][8] (conv64_x6p_kernel):
                    // lane = (c % 16 >= 8) * 32 + n % 32, element c % 8
                    const int mt = n >> 5, cb = c >> 4, ln = ((c >> 3) & 1) * 32 + (n & 31);
                    for (int q = 0; q < 3; q++)
                        pl[((((size_t)(mt * LK_NCB + cb) * 9 + tap) * 3 + q) * 64 + ln) * 8 + (c & 7)] = parts[q];
                    const float xs = std::ldexp(x, tau);   // the F16 parts, same order with 2 parts
                    const _Float16 f0 = (_Float16)xs;
                    const _Float16 fparts[2] = {f0, (_Float16)(xs - (float)f0)};
                    for (int q = 0; q < 2; q++)
                        ph[((((size_t)(mt * LK_NCB + cb) * 9 + tap) * 2 + q) * 64 + ln) * 8 + (c & 7)] = fparts[q];
                }
        o += LK_FLOATS;
    }
    return SDE_OK;
}
