// tower_fp32.hip -- the instantiations of conv64_mfma_kernel (tower_fp32.h) and their launcher: one launch per image.
#include "tower_fp32.h"
#include "tower_launch.h"
using namespace sde;

void sde::launch_fp32(const TowerLaunch &L)
{
    const dim3 grid2(cdiv(L.wout, TW_TX), cdiv(L.hout, TW_TY));
    const int64_t pix = (int64_t)L.hout * L.wout;
    for (int i = 0; i < L.nimg; i++) {
        const float *ini = L.in + i * L.bt.in_stride;
        float *outi = L.out + i * L.bt.out_stride;
        uint16_t *hi = L.ohi ? L.ohi + i * pix * NF : nullptr, *lo = L.olo ? L.olo + i * pix * NF : nullptr;
        float *nr = L.onrm ? L.onrm + i * pix : nullptr;
#define SDE_CONV(F, L_)                                                                                            \
    launch_lds<conv64_mfma_kernel<F, L_>, TW_SMEM>(grid2, 512, L.st, ini, L.Hin, L.Win, (F) ? L.w1 : nullptr, L.wk, \
                                                   outi, L.hout, L.wout, (L_) ? hi : nullptr, (L_) ? lo : nullptr,  \
                                                   (L_) ? nr : nullptr)
        if (L.first) { if (L.last) SDE_CONV(true, true); else SDE_CONV(true, false); }
        else { if (L.last) SDE_CONV(false, true); else SDE_CONV(false, false); }
#undef SDE_CONV
    }
}
