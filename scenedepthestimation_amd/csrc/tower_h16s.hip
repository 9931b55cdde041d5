// tower_h16s.hip -- the instantiations of conv64_h16s_kernel and their launcher.  Timing builds put a generated
// probe copy of tower_h16s.h first (SDE_H16S_HEADER, tools/variants/make_phase_header.py).
#ifdef SDE_H16S_HEADER
#include SDE_H16S_HEADER
#endif
#include "tower_h16s.h"
#include "tower_launch.h"
using namespace sde;

void sde::launch_h16s(const TowerLaunch &L)
{
    using T = H16T16;
    // conv64_h16s_kernel<LAST, IN_CB, OUT_CB>
#define SDE_H16S(L_, I, O)                                                                                          \
    launch_lds<conv64_h16s_kernel<L_, I, O>, T::SMEM>(L.grid, 512, L.st, L.in, L.Hin, L.Win, L.wk, L.out, L.hout,    \
                                                      L.wout, L.bt, L.in_amax, L.out_amax)
    if (L.last) {
        if (L.in_cb) SDE_H16S(true, true, false); else SDE_H16S(true, false, false);
    } else if (L.in_cb) {
        if (L.out_cb) SDE_H16S(false, true, true); else SDE_H16S(false, true, false);
    } else {
        if (L.out_cb) SDE_H16S(false, false, true); else SDE_H16S(false, false, false);
    }
#undef SDE_H16S
}
