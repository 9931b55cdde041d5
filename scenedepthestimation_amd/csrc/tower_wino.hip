// tower_wino.hip -- the instantiations of wino_kernel (tower_wino.h) and their launcher.
#include "tower_wino.h"
#include "tower_launch.h"
using namespace sde;

void sde::launch_wino(const TowerLaunch &L)
{
#define SDE_WINO(L_, I, O)                                                                                       \
    launch_lds<wino_kernel<L_, I, O>, WN_SMEM>(L.grid, 512, L.st, L.in, L.Hin, L.Win, L.wk, L.out, L.hout, L.wout, \
                                               L.bt, L.in_amax, L.out_amax)
    if (L.last) { if (L.in_cb) SDE_WINO(true, true, false); else SDE_WINO(true, false, false); }
    else if (L.in_cb) { if (L.out_cb) SDE_WINO(false, true, true); else SDE_WINO(false, true, false); }
    else { if (L.out_cb) SDE_WINO(false, false, true); else SDE_WINO(false, false, false); }
#undef SDE_WINO
}
