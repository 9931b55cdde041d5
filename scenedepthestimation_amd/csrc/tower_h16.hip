// tower_h16.hip -- the instantiations of conv64_h16_kernel and conv64_h16q_kernel, and their launcher.  Timing builds
// put a generated probe copy of tower_h16.h first (SDE_H16_HEADER); its guard empties tower_h16q.h's include.
#ifdef SDE_H16_HEADER
#include SDE_H16_HEADER
#endif
#include "tower_h16q.h"
#include "tower_launch.h"
using namespace sde;

void sde::launch_h16(const TowerLaunch &L)
{
    const bool split = L.ohi || L.olo || L.onrm;
    // conv64_h16_kernel<LAST, IN_CB, OUT_CB, SPLIT, ISPL, OSPL, FIRST> (same tiles as conv64_x6p_kernel)
#define SDE_H16(SM, L_, I, O, S, ...)                                                                               \
    launch_lds<conv64_h16_kernel<L_, I, O, S, ##__VA_ARGS__>, SM>(L.grid, 512, L.st, L.in, L.Hin, L.Win, L.wk,       \
                                                                  L.out, L.hout, L.wout, (S) ? L.ohi : nullptr,      \
                                                                  (S) ? L.olo : nullptr, (S) ? L.onrm : nullptr,     \
                                                                  L.bt, L.in_amax, L.out_amax,                       \
                                                                  L.first ? L.w1 : nullptr)
    if (L.first) {   // conv1 on the stagers + conv2
        if (L.out_sp) SDE_H16(H16_SMEM_FIRST, false, false, false, false, false, true, true);
        else if (L.out_cb) SDE_H16(H16_SMEM_FIRST, false, false, true, false, false, false, true);
        else SDE_H16(H16_SMEM_FIRST, false, false, false, false, false, false, true);
    } else if (L.in_sp) {   // split activations in (and out, below the last layer): LDS-DMA stagers
        if (!L.last)   // the 4-wave kernel with resident weights (tower_h16q.h)
            launch_lds<conv64_h16q_kernel, H16_SMEM>(L.grid, 256, L.st, L.in, L.Hin, L.Win, L.wk, L.out, L.hout, L.wout,
                                                     L.bt, L.in_amax, L.out_amax);
        else if (split) SDE_H16(H16_SMEM, true, false, false, true, true, false);
        else SDE_H16(H16_SMEM, true, false, false, false, true, false);
    } else if (L.last) {
        if (split) { if (L.in_cb) SDE_H16(H16_SMEM, true, true, false, true); else SDE_H16(H16_SMEM, true, false, false, true); }
        else { if (L.in_cb) SDE_H16(H16_SMEM, true, true, false, false); else SDE_H16(H16_SMEM, true, false, false, false); }
    } else if (L.in_cb) {
        if (L.out_cb) SDE_H16(H16_SMEM, false, true, true, false); else SDE_H16(H16_SMEM, false, true, false, false);
    } else {
        if (L.out_cb) SDE_H16(H16_SMEM, false, false, true, false); else SDE_H16(H16_SMEM, false, false, false, false);
    }
#undef SDE_H16
}
