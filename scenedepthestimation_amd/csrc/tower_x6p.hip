// tower_x6p.hip -- the instantiations of conv64_x6p_kernel (tower_x6p.h) and their launcher.
#include "tower_x6p.h"
#include "tower_launch.h"
using namespace sde;

void sde::launch_x6p(const TowerLaunch &L)
{
    // conv64_x6p_kernel<FIRST, LAST, IN_CB, OUT_CB, F16>
#define SDE_X6P(F, L_, ...)                                                                                         \
    launch_lds<conv64_x6p_kernel<F, L_, __VA_ARGS__>, XP_SMEM>(L.grid, 512, L.st, L.in, L.Hin, L.Win,                \
                                                               (F) ? L.w1 : nullptr, L.wk, L.out, L.hout, L.wout,    \
                                                               (L_) ? L.ohi : nullptr, (L_) ? L.olo : nullptr,       \
                                                               (L_) ? L.onrm : nullptr, L.bt, L.in_amax, L.out_amax)
#define SDE_X6P_ALL(H)                                                      \
    if (L.first) {                                                          \
        if (L.last) SDE_X6P(true, true, false, false, H);                   \
        else if (L.out_cb) SDE_X6P(true, false, false, true, H);            \
        else SDE_X6P(true, false, false, false, H);                         \
    } else if (L.last) {                                                    \
        if (L.in_cb) SDE_X6P(false, true, true, false, H);                  \
        else SDE_X6P(false, true, false, false, H);                         \
    } else {                                                                \
        if (L.in_cb && L.out_cb) SDE_X6P(false, false, true, true, H);      \
        else if (L.in_cb) SDE_X6P(false, false, true, false, H);            \
        else if (L.out_cb) SDE_X6P(false, false, false, true, H);           \
        else SDE_X6P(false, false, false, false, H);                        \
    }
    if (L.f16) { SDE_X6P_ALL(true) } else { SDE_X6P_ALL(false) }
#undef SDE_X6P_ALL
#undef SDE_X6P
}
