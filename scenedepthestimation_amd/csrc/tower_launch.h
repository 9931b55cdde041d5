// tower_launch.h -- one tower layer launch as a descriptor: tower.hip's launch_layer completes it and picks the
// kernel family, the family's launcher (tower_<family>.hip) picks the instantiation from the layout booleans.
#pragma once
#include "tower_common.h"

namespace sde {

// in: the padded image (first: Hin x Win floats) or Hin x Win x 64 activations; out: hout x wout x 64.  w1 / wk:
// layer 1's and this layer's block of the packed blob.  ohi / olo / onrm (last layer, optional): the features' bf16
// split planes and norm bounds.  in_amax / out_amax (F16X3): the bound words of |input| and of the ReLU outputs.
// Image i of nimg sits at in + i * bt.in_stride, out + i * bt.out_stride, bound words + i * bt.amax_stride; bt's tile
// space is walked by `grid` persistent workgroups (the fp32 kernel: one launch per image on a grid of its own).
// f16: SDE_TOWER_F16X3; first: layer 2, conv1 fused; last: L2-normalised [h][w][64] features.  Activations in / out: c-block-major fp32
// [4][h][w][16] (in_cb / out_cb), split fp16 planes (in_sp / out_sp), else [h][w][64].
struct TowerLaunch {
    const float *in, *w1, *wk, *in_amax;
    float *out, *onrm, *out_amax;
    uint16_t *ohi, *olo;
    int Hin, Win, hout, wout, nimg, grid;
    XpBatch bt;
    hipStream_t st;
    bool f16, first, last, in_cb, out_cb, in_sp, out_sp;
};

// Each names every instantiation of its family once, with its dynamic-LDS size (launch_lds).
__attribute__((visibility("hidden"))) void launch_fp32(const TowerLaunch &L);
__attribute__((visibility("hidden"))) void launch_x6p(const TowerLaunch &L);
__attribute__((visibility("hidden"))) void launch_h16(const TowerLaunch &L);   // conv64_h16_kernel, conv64_h16q_kernel
__attribute__((visibility("hidden"))) void launch_h16s(const TowerLaunch &L);  // conv64_h16s_kernel (16 x 16 tiles)
__attribute__((visibility("hidden"))) void launch_wino(const TowerLaunch &L);

}  // namespace sde
