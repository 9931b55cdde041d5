// tower_blob.h -- the tower's packed-weight blob (tower_pack.hip writes it, every kernel reads it), plain C++:
// layer 1's block of L1_FLOATS floats, then one block of LK_FLOATS floats per layer k >= 2.
#pragma once

namespace sde {

constexpr int NF = 64;                   // feature maps (the reference's num_of_conv_feature_maps)
constexpr int L1_FLOATS = NF + 9 * NF;           // bias + [tap][n]
constexpr int LK_W = 9 * NF * NF;                // one [tap][n][c] plane, elements
constexpr int LK_NCB = NF / 16;                  // 16-channel c-blocks of the A-fragment orders below
// layer k >= 2: bias f32 [64] | W f32 [tap][n][c] | bf16 parts (hi, mid, lo: W = hi+mid+lo) in A-fragment order
// [mtile 2][cblock 4][tap 9][part 3][lane 64][8] for conv64_x6p_kernel | fp16 parts of W * 2^tau (hi, lo)
// [mtile 2][cblock 4][tap 9][part 2][lane 64][8] for the F16 variant | F16 header {2^-tau, conv1 L1 bound,
// max |b1|, 0, L1 bound of this layer (max_n sum_{tap,c} |w|), its max |b|, 0, 0} (the conv1 terms are used
// by layer 2, which computes conv1; the layer's own terms bound its outputs for the split activations)
constexpr int LK_F16 = NF + LK_W + 3 * LK_W / 2;   // float offset of the fp16 parts
constexpr int LK_HDR = 8;                           // F16 header floats
// Winograd F(2x2,3x3) U = G g G^T (tower_wino.h): [xi 16][mtile 2][cblock 4][part 2][lane 64][8] fp16
// after the F16 header, then its own header {2^-tau_u, 0, 0, 0}
constexpr int LK_WINO = LK_F16 + LK_W + LK_HDR;
constexpr int LK_WU = 16 * NF * NF * 2;                // fp16 elements
constexpr int LK_WHDR = LK_WINO + LK_WU / 2;
constexpr int LK_FLOATS = LK_WHDR + 4;

}  // namespace sde
