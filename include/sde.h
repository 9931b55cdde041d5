/*
 * sde.h -- C ABI of the MI355X-native stereo matching path (libsde.so).
 *
 * Drop-in boundary for WHDY/SceneDepthEstimation's matching path.  The
 * reference's boundary is the Python function API of process_functional.py
 * (star-imported by match_single.py:9 / match.py:10); each entry point below
 * names the reference function or Numba kernel it replaces (file:line).
 *
 * Conventions
 *   - every pointer argument except host-side helpers is a DEVICE pointer owned
 *     by the caller; nothing here allocates, frees or synchronises, so every call
 *     is stream-ordered and capturable into a hipGraph;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - feature maps are [H][W][C] float32 (channels-last, the layout
 *     compute_feature returns, process_functional.py:42-43);
 *   - return value: SDE_OK or a negative sde_status; errors are detected before
 *     any launch (argument checks) or right after it (hipGetLastError).
 *   - reentrant: no global state besides the HIP module the loader registers and the
 *     tower's grid cap (sde_set_persistent_grid, a tuning knob that does not change results).
 */
#ifndef SDE_H
#define SDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDE_ABI_VERSION 4

typedef enum {
    SDE_OK = 0,
    SDE_ERR_ARG = -1,         /* bad size / null pointer / unsupported combination */
    SDE_ERR_LAUNCH = -2,      /* hipGetLastError() after a launch */
    SDE_ERR_WORKSPACE = -3,   /* workspace too small */
} sde_status;

typedef enum {
    SDE_LAYOUT_DHW = 0,   /* [D][H][W]: compute_cost_volume / WTA1 (process_functional.py:48,96) */
    SDE_LAYOUT_HWD = 1,   /* [H][W][D]: WTA and the GPU path (process_functional.py:76,120)      */
} sde_layout;

typedef enum {
    SDE_WTA_INIT_INF = 0, /* best=+inf, `v < best`; no winner -> -1 (WTA/WTA1, :83-110)             */
    SDE_WTA_INIT_D0 = 1,  /* best=v[0], `best > v` (WTA_and_SupixelRefinement_kernel, :805-811)      */
} sde_wta_rule;

typedef enum {
    SDE_SIDE_LEFT = 1,    /* L[y][x][d]   = cost(x, d)        (process_functional.py:130) */
    SDE_SIDE_RIGHT = 2,   /* R[y][x-d][d] = cost(x, d)        (process_functional.py:131) */
} sde_side;

/* ABI version (SDE_ABI_VERSION) and a static status string. */
int sde_abi_version(void);
const char *sde_status_string(int status);

/*
 * Cost volume, exact CPU-path numerics: cost(x,d) = -(0.0f + pairwise_sum_c
 * fl[y][x][c]*fr[y][x-d][c]) with NumPy's float32 pairwise order (no FMA).
 *   layout = SDE_LAYOUT_DHW, sides = LEFT, invalid = -0.0f
 *       replaces compute_cost_volume (process_functional.py:48-73), bit-exact;
 *   layout = SDE_LAYOUT_HWD, sides = LEFT|RIGHT, invalid = 1.0f
 *       replaces compute_cost_volume_kernel (process_functional.py:120-131)
 *       including its never-written voxels (:1111-1114).
 * out_left / out_right: D*H*W floats each (the one not requested may be NULL).
 */
int sde_cost_volume(const float *fl, const float *fr, int H, int W, int C, int D, int layout,
                    int sides, float invalid, float *out_left, float *out_right, void *stream);

/*
 * First-minimum over d of an existing volume -> disparity as float32.
 * Replaces WTA1 (process_functional.py:96-113, DHW), WTA (:76-93, HWD) and
 * WTA_and_SupixelRefinement_kernel (:800-837, HWD + SDE_WTA_INIT_D0).
 * A pixel without a winner (all NaN / +inf under INIT_INF) gets -1.0f; the
 * reference asserts there (:89,109) and the Python layer raises.
 */
int sde_wta(const float *vol, int H, int W, int D, int layout, int rule, float *disp, void *stream);

/* sde_cv_wta modes: both give identical (bit-exact) outputs. */
#define SDE_CV_EXACT 0       /* every voxel in NumPy's pairwise order on VALU                                */
#define SDE_CV_CERTIFIED 1   /* f16x3 (row sweep) or bf16x3 MFMA scores + rigorous error bound; pixels whose
                                winner is not certified by a 2*eps gap are resolved by the exact scan
                                (needs workspace) */

/* Workspace bytes sde_cv_wta needs in SDE_CV_CERTIFIED mode (work-list of unresolved pixels). */
int64_t sde_cv_wta_workspace_bytes(int H, int W);

/*
 * Fused cost volume + WTA over the disparity shard [d0, d1) without
 * materialising the volume: WTA1(compute_cost_volume(fl, fr, D)) bit-exact when
 * d0 = 0, d1 = D (process_functional.py:48-73 + :96-113).  Outputs (each
 * optional, NULL to skip): disp (float32 argmin), min_cost (float32 first-min
 * cost, bit-exact) and argmin (int32, -1 if none), [H][W].  Shards merge
 * bit-exactly with sde_argmin_merge (ties -> lower d).  mode: SDE_CV_EXACT or
 * SDE_CV_CERTIFIED (C == 64; other C always run exact).  The workspace's first
 * 256 bytes hold, after the call, 64 uint32 counters whose sum is the number of
 * pixels the certified mode resolved exactly (one per 256-disparity chunk when
 * d1 - d0 exceeds the row sweep's window, e.g. D = 512; word 0 otherwise).
 */
int sde_cv_wta(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, float *disp,
               float *min_cost, int32_t *argmin, int mode, void *workspace, int64_t workspace_bytes,
               void *stream);

/*
 * The right view of sde_cv_wta (additive in ABI 4): fused cost volume + WTA indexed by RIGHT pixel,
 *   disp_r = flipW( WTA1( compute_cost_volume( flipW(fr), flipW(fl), D ) ) )      (d0 = 0, d1 = D)
 * with the reference's own NumPy functions (process_functional.py:48-73 + :96-113) on the mirrored, swapped
 * pair -- the standard right-matcher construction.  Equivalently, for right pixel x', the first minimum over d
 * in [d0, d1) of cost(x'+d, d) = -(0.0f + pairwise_sum_c fl[y][x'+d][c]*fr[y][x'][c]); voxels with x'+d >= W
 * hold the -0.0 fill and take part in the scan (as x < d does in the left view), the comparison is a strict
 * `<` (ties -> lower d), and since the products commute every cost has the left view's bits.  fl / fr are the
 * same left / right feature maps sde_cv_wta takes (not swapped by the caller).  Argument rules, modes (both
 * bit-exact), the workspace (sde_cv_wta_workspace_bytes, same layout and counter words) and the outputs' meaning
 * are sde_cv_wta's; shards over [d0, d1) merge with sde_argmin_merge as for the left view.
 */
int sde_cv_wta_right(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, float *disp,
                     float *min_cost, int32_t *argmin, int mode, void *workspace, int64_t workspace_bytes,
                     void *stream);

/*
 * Split a [npix][64] float32 feature map for SDE_CV_CERTIFIED: hi = bf16_rne(x),
 * lo = bf16_rne(x - hi) (both [npix][64] bf16 bit patterns) and norm[p] >= the
 * pixel's L2 norm.  The tower can emit the same three outputs from its last
 * layer (sde_tower_forward's feat_hi / feat_lo / feat_norm).
 */
int sde_feature_split(const float *feat, int64_t npix, int C, uint16_t *hi, uint16_t *lo, float *norm, void *stream);

/* Workspace bytes for sde_cv_wta_split (work-list of unresolved pixels). */
int64_t sde_cv_wta_split_workspace_bytes(int H, int W);

/*
 * SDE_CV_CERTIFIED on pre-split operands (no split pass): same outputs and
 * bit-exactness as sde_cv_wta.  fl / fr (float32) are read only for the exact
 * resolution of uncertified pixels and for min_cost.
 */
int sde_cv_wta_split(const float *fl, const float *fr, const uint16_t *fl_hi, const uint16_t *fl_lo,
                     const float *fl_norm, const uint16_t *fr_hi, const uint16_t *fr_lo, const float *fr_norm,
                     int H, int W, int d0, int d1, float *disp, float *min_cost, int32_t *argmin, void *workspace,
                     int64_t workspace_bytes, void *stream);

/*
 * Ordered merge of per-shard (min, argmin) pairs: shard s covers a disparity
 * range that precedes shard s+1's; strict `<` keeps the earliest on ties.
 * mins/args: [nshards][npix].  disp: float32 [npix].
 */
int sde_argmin_merge(const float *mins, const int32_t *args, int nshards, int64_t npix, float *disp,
                     void *stream);

/* ---------------------------------------------------------------------- */
/* MC-CNN-fast branch (mc_cnn_brunch.py:31-48; compute_feature's sess.run,   */
/* process_functional.py:11-45).  nlayers 3x3 VALID convs, nf = 64 maps.     */
/* ---------------------------------------------------------------------- */

/* Workgroups of the persistent tower kernels (default 0: one per CU of the device).  A positive value caps
 * the grid -- for a tower sharing the device with other work on CU-masked streams (hipExtStreamCreateWithCUMask),
 * where one workgroup per device CU would leave the last ones waiting for the other stream's CUs.  Process-wide;
 * results do not depend on it. */
int sde_set_persistent_grid(int cus);

/* Tower arithmetic (flags of sde_tower_forward / sde_tower_layer). */
#define SDE_TOWER_FP32 0      /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation            */
#define SDE_TOWER_BF16X6 1    /* fp32 operands split exactly into 3 bf16 parts, the 6 leading partial products
                                 on v_mfma_f32_32x32x16_bf16, fp32 accumulation: fp32-level error, 2.67x rate */
#define SDE_TOWER_F16X3 8     /* operands scaled by powers of two and split exactly into 2 fp16 parts, the 3
                                 leading partial products on v_mfma_f32_32x32x16_f16, fp32 accumulation:
                                 ~2^-22 relative per product (fp32-level), 5.3x the fp32 matrix rate.
                                 The scalings need per-layer bound words: sde_tower_forward keeps them
                                 in its workspace; single layers go through sde_tower_layer_scaled. */
/* sde_tower_layer only, with SDE_TOWER_BF16X6 or SDE_TOWER_F16X3: intermediate activations in the c-block-major
 * layout [nf/16][h][w][16] that sde_tower_forward uses between layers (16-channel blocks
 * contiguous per pixel run).  IN: `in` of a layer >= 3; OUT: `out` of a layer < nlayers. */
/* With SDE_TOWER_F16X3 only: run the 64 -> 64 layers (3..L) with the Winograd F(2x2, 3x3) kernel
 * instead of the direct 3x3 kernel (same arithmetic contract and error class, 2.25x fewer MFMA
 * products, more VALU; slower than the direct kernel at 1024^2 on MI355X -- DESIGN.md 3.2). */
#define SDE_TOWER_WINOGRAD 16
/* With SDE_TOWER_F16X3 only: run the 64 -> 64 layers on the v_mfma_f32_32x32x16_f16 direct kernel instead of
 * the default v_mfma_f32_16x16x32_f16 one (same arithmetic contract). */
#define SDE_TOWER_MFMA32 32
/* With SDE_TOWER_F16X3, not with MFMA32: keep every layer of the v_mfma_f32_16x16x32_f16 path on the 16 x 32-tile
 * kernel.  Without it, layers 3..L with fp32 activations in and out (no IN_SPLIT / OUT_SPLIT, no split feature planes)
 * run the 16 x 16-tile kernel whose stager waves store the outputs; the bits are the same either way, and the
 * flag changes nothing for the layers only the 16 x 32 kernel serves. */
#define SDE_TOWER_TILE32 256
#define SDE_TOWER_IN_CBLOCK 2
#define SDE_TOWER_OUT_CBLOCK 4
/* F16X3 split activations (sde_tower_layer_scaled / sde_tower_layer_batch; what sde_tower_forward uses
 * between the 64->64 layers of the default f16x3 tower): OUT_SPLIT writes a layer's ReLU outputs scaled by
 * 2^sigma and split exactly into two fp16 parts, per image 16 planes [cblk32 2][part 2][quarter 4] of
 * [h][w][8 fp16] (256 B per pixel, as fp32 [h][w][64]), and publishes 2^sigma at out_absmax[32] (per image);
 * IN_SPLIT reads that layout and in_absmax[32] (LDS-DMA staging, no arithmetic).  2^sigma comes from an
 * a-priori bound of the outputs (max |b| + L1 * input bound, no fp16 overflow).  Layers >= 3 (IN) and
 * < nlayers (OUT), a layer between them with both or neither; at most 32 layers, fewer than 2^24 input pixels; bound-word arrays extending >= 33 words past
 * the word passed (batches: amax_stride >= 64 words per image, so no image's scale word lands on the next image's row); not with the CBLOCK flag of the same side, WINOGRAD or MFMA32. */
#define SDE_TOWER_IN_SPLIT 64
#define SDE_TOWER_OUT_SPLIT 128

/* Number of floats of the packed (device-layout) weight blob (fp32 + pre-split bf16 planes). */
int64_t sde_tower_packed_floats(int nlayers, int nf);

/* 1 if this build's sde_tower_forward* pass split activations (SDE_TOWER_OUT_SPLIT / IN_SPLIT layouts) between
 * the default f16x3 tower's 64 -> 64 layers, 0 if they pass c-block-major fp32 (the default build).  Layer-by-layer
 * drivers that must reproduce the forward's bits (the row-band tower of the multi-GPU schemes) follow it. */
int sde_tower_split_act(void);

/*
 * HOST helper: pack TF HWIO weights ([3][3][Cin][nf], `conv{k}/weights:0`) and
 * biases ([nf], `conv{k}/biases:0`) of nlayers layers into `packed` (host memory,
 * sde_tower_packed_floats() floats).  Copy the blob to the device once.
 */
int sde_tower_pack_weights(const float *const *hwio, const float *const *biases, int nlayers, int nf,
                           float *packed);

/* Device workspace bytes needed by sde_tower_forward for an H x W output. */
int64_t sde_tower_workspace_bytes(int H, int W, int nlayers, int nf);

/*
 * img_pad: float32 [(H+2*nlayers)][(W+2*nlayers)] zero-padded normalised image
 * (process_functional.py:13-19).  feat: float32 [H][W][nf], L2-normalised per
 * pixel (mc_cnn_brunch.py:48).  packed: device copy of the packed weights.
 * feat_hi / feat_lo / feat_norm (optional, NULL to skip; nlayers >= 2): the
 * last layer's epilogue also writes the bf16 split planes and per-pixel norm
 * bound that sde_cv_wta_split consumes (same layout as sde_feature_split).
 */
int sde_tower_forward(const float *img_pad, int H, int W, const float *packed, int nlayers, int nf,
                      float *feat, void *workspace, int64_t workspace_bytes, int flags, uint16_t *feat_hi,
                      uint16_t *feat_lo, float *feat_norm, void *stream);

/*
 * sde_tower_forward over nimg images of one size in one set of launches (the
 * split arithmetics tile the whole batch in one persistent grid: fewer launches,
 * less tail imbalance).  img_pad: [nimg][H+2*nlayers][W+2*nlayers]; feat:
 * [nimg][H][W][nf]; feat_hi / feat_lo: [nimg][H][W][nf]; feat_norm: [nimg][H][W].
 * Each image gets the same result as sde_tower_forward on it alone.
 */
int64_t sde_tower_batch_workspace_bytes(int H, int W, int nimg, int nlayers, int nf);
int sde_tower_forward_batch(const float *img_pad, int nimg, int H, int W, const float *packed, int nlayers, int nf,
                            float *feat, void *workspace, int64_t workspace_bytes, int flags, uint16_t *feat_hi,
                            uint16_t *feat_lo, float *feat_norm, void *stream);

/*
 * One layer of the tower as a single kernel launch (for per-layer timing and
 * pipelining): layer == 2 -> conv1+conv2 fused, `in` = padded image Hin x Win
 * floats, out (Hin-4) x (Win-4) x nf; layer in 3..nlayers -> `in` = Hin x Win x
 * nf activations, out (Hin-2) x (Win-2) x nf.  Layer nlayers L2-normalises.
 */
int sde_tower_layer(const float *in, int Hin, int Win, const float *packed, int nlayers, int nf, int layer,
                    float *out, int flags, uint16_t *feat_hi, uint16_t *feat_lo, float *feat_norm, void *stream);

/*
 * sde_tower_layer with the SDE_TOWER_F16X3 bound words (ignored by the other
 * arithmetics): in_absmax -> device float, an upper bound of |input| (layer 2:
 * of |image|; the kernel bounds conv1's output from it); out_absmax -> device
 * float the launch atomically maxes its (non-negative) outputs into, zeroed by
 * the caller (may be NULL for the last layer).
 */
int sde_tower_layer_scaled(const float *in, int Hin, int Win, const float *packed, int nlayers, int nf, int layer,
                           float *out, int flags, uint16_t *feat_hi, uint16_t *feat_lo, float *feat_norm,
                           const float *in_absmax, float *out_absmax, void *stream);

/*
 * sde_tower_layer_scaled over nimg images per launch (no split outputs): image i
 * reads in + i * in_stride, writes out + i * out_stride (floats; the last layer's
 * out_stride must be (Hin-2)*(Win-2)*nf) and uses bound words in_absmax /
 * out_absmax + i * amax_stride.
 */
int sde_tower_layer_batch(const float *in, int nimg, int64_t in_stride, int Hin, int Win, const float *packed,
                          int nlayers, int nf, int layer, float *out, int64_t out_stride, int flags,
                          const float *in_absmax, float *out_absmax, int amax_stride, void *stream);

/* sde_absmax_f32 over nimg arrays of n floats (x + i * n) into absmax[i * absmax_stride]. */
int sde_absmax_f32_batch(const float *x, int nimg, int64_t n, float *absmax, int absmax_stride, void *stream);

/* *absmax = max(*absmax, max |x[i]|) over n floats (float bits compared as integers; *absmax >= +0). */
int sde_absmax_f32(const float *x, int64_t n, float *absmax, void *stream);

/*
 * Preprocess on device (match_single.py:34-43 + process_functional.py:13-19):
 * u8 image -> (I - mean) / std (population std, float32) written into the
 * interior of the zero-padded buffer out_pad [(H+2*pad)][(W+2*pad)] -- bit for bit
 * NumPy's np.mean / np.std over axes (0, 1) of the float32 image (its pairwise
 * float32 reduction order) and the float32 elementwise expression.
 * scratch: sde_preprocess_scratch_bytes(H, W) of device memory per image (the
 * statistics and NumPy's per-8192-element partial sums; no initialisation needed).
 */
int64_t sde_preprocess_scratch_bytes(int H, int W);
int sde_preprocess_u8(const uint8_t *img, int H, int W, int pad, float *out_pad, void *scratch,
                      void *stream);

/* sde_preprocess_u8 over nimg images per launch: imgs [nimg][H][W], out_pad
 * [nimg][H+2*pad][W+2*pad], scratch nimg * sde_preprocess_scratch_bytes(H, W). */
int sde_preprocess_u8_batch(const uint8_t *imgs, int nimg, int H, int W, int pad, float *out_pad, void *scratch,
                            void *stream);

/* ---------------------------------------------------------------------- */
/* Semi-global matching (GPU path of disparity_compute_by_gpu,               */
/* process_functional.py:1093-1267).                                         */
/* ---------------------------------------------------------------------- */

/* sgm_penelty_kernel (process_functional.py:134-262): pen [H][W][16] float32. */
int sde_sgm_penalties(const uint8_t *img, int H, int W, double P1, double P2, int64_t threshold,
                      double lambda, float *pen, void *stream);

/*
 * 8-path SGM for one side (SGM_*_kernel, process_functional.py:265-797, launch
 * order :1166-1203): S [H][W][D] += path costs, direction order UD, DU, LR, RL,
 * UD-LR, DU-LR, UD-RL, DU-RL; fp64 recurrence, float32 S.  The caller zeroes S
 * (the reference uploads np.zeros, :1116-1119).  cv: [H][W][D] with invalid
 * voxels = 1.0 (sde_cost_volume HWD).  Requires H >= 2, W >= 2.
 * pen: [H][W][16], from sde_sgm_penalties or the caller's own: any float32 values.  Finite
 * penalties with P1 >= 0 (P2 of any sign) and finite costs run the fast recurrence; a scanline
 * leaves it for the reference's exact arithmetic (slower, same values as the reference, bit for
 * bit including zero signs) from its first step on with a NaN / inf cost or penalty, a P1 < 0,
 * or -- when S is the caller's -- a voxel whose cost and S are both -0.0.
 */
int sde_sgm_8path(const float *cv, const float *pen, int H, int W, int D, float *S, void *stream);

/*
 * Both image sides of the reference's per-direction k loop (:1166-1203) in one
 * launch per direction (the (cv_r, pen_r, S_r) triple may be all NULL for one
 * side).  flags = 0: S := the 8-path sum starting from zero, so the caller need
 * not zero S and the first direction does not read it (same values as zeroing
 * S then accumulating); SDE_SGM_ACCUMULATE: S += path costs as sde_sgm_8path.
 */
#define SDE_SGM_ACCUMULATE 1
/* The caller asserts that penalty channels 0/1 are zero (sde_sgm_penalties never writes
 * them, as the reference's sgm_penelty_kernel): direction DU then reduces to S += C (+0.0
 * off its first row) for finite costs and is folded into the UD pass (7 passes instead of
 * 8, same values).  A column holding a non-finite cost, a non-finite or negative UD P1 or
 * non-finite UD P2 (channels 2/3) or, with SDE_SGM_ACCUMULATE, a voxel whose cost and S are
 * both -0.0, is detected and recomputed for both directions in the reference's exact
 * arithmetic, so the fold gives the unfolded values for any costs, any S and any penalties
 * in channels 2..15. */
#define SDE_SGM_ZERO_DU_PENALTIES 2
int sde_sgm_8path_pair(const float *cv_l, const float *pen_l, float *S_l, const float *cv_r, const float *pen_r,
                       float *S_r, int H, int W, int D, int flags, void *stream);

/*
 * sde_sgm_8path_pair fused with WTA_and_SupixelRefinement_kernel (process_functional.py:800-837,
 * the same first-min rule as sde_wta(..., SDE_WTA_INIT_D0)): the last direction (DU-RL) reduces
 * each pixel's final S to its disparity in disp [H][W] float32 instead of storing S, so on
 * return S holds the sum of the first seven directions.  disp_r may be NULL only with the
 * right triple.  Same flags and values as sde_sgm_8path_pair followed by sde_wta.
 */
int sde_sgm_8path_wta_pair(const float *cv_l, const float *pen_l, float *S_l, float *disp_l, const float *cv_r,
                           const float *pen_r, float *S_r, float *disp_r, int H, int W, int D, int flags,
                           void *stream);

/* One direction (0..7 in the order above) of sde_sgm_8path. */
int sde_sgm_direction(const float *cv, const float *pen, int H, int W, int D, int direction, float *S,
                      void *stream);

/* ---------------------------------------------------------------------- */
/* Cross-based cost aggregation.  BUILD-DEFINED: the reference has none      */
/* (SURVEY.md sec. 0.3 -- only the buffer name d_cost_volumel_after_aggr,   */
/* process_functional.py:268,347, and an unused timer label, match.py:98);  */
/* the definition is restated on the CPU under oracle/ (parity unpinned vs */
/* the reference, bit-exact vs that restatement).                          */
/* ---------------------------------------------------------------------- */
#define SDE_CBCA_MAX_L1 32

/*
 * Cross arms of an f32 image (row pitch in elements, e.g. the z-normalised
 * interior of the tower's padded input): for left/right/up/down the largest
 * k <= L1-1 with |I(p) - I(p + j*dir)| < tau for all 1 <= j <= k inside the
 * image.  arms u32 [H][W] = l | r<<8 | u<<16 | d<<24.
 */
int sde_cbca_arms(const float *img, int64_t pitch, int H, int W, int L1, float tau, uint32_t *arms, void *stream);

/*
 * Definition v2 (round 4; the CPU restatement under oracle/ states it in full): volumes are
 * aggregated in LEFT coordinates (a right-referenced volume through
 * R(y,x',d) = L(y,x'+d,d)); voxels whose right-image pixel is outside the
 * image pass through unchanged; support arms = min(left-image arm, right-image
 * arm); fp64 prefix chains restart per segment of SDE_CBCA_SEG positions at
 * kS - (L1 - 1); the mean multiplies by the correctly rounded fp64 1/count.
 * Consequence: the aggregation of R = shear(L) is shear(aggregation of L).
 */
#define SDE_CBCA_SEG 256

/* Workspace of the aggregation entry points (a column-major copy of the left
 * image's arms for the vertical pass): 4 * W * roundup(H, 4) bytes (ABI 3 asked
 * for 8 *: larger buffers stay valid). */
size_t sde_cbca_workspace_bytes(int H, int W);

/*
 * iters x (horizontal pass, vertical pass) on an [H][W][D] volume, in place
 * in cv (tmp: same size, scratch).  side SDE_SIDE_LEFT: left-referenced volume,
 * the other pixel is x - d (arms_ref = left image arms, arms_other = right);
 * SDE_SIDE_RIGHT: x + d (arms_ref = right image, arms_other = left; done as a
 * rotation into left coordinates, the aggregation, and the rotation back).
 * L1 as given to sde_cbca_arms (arms must not exceed L1 - 1).
 */
int sde_cbca(float *cv, float *tmp, const uint32_t *arms_ref, const uint32_t *arms_other, int H, int W, int D,
             int side, int L1, int iters, void *ws, size_t ws_bytes, void *stream);

/*
 * sde_cbca on both volumes of a pair (same results as sde_cbca(cv_l, tmp_l,
 * arms_l, arms_r, SDE_SIDE_LEFT) and sde_cbca(cv_r, tmp_r, arms_r, arms_l,
 * SDE_SIDE_RIGHT)) for any two volumes; the four buffers must be distinct.
 * Build-defined like sde_cbca: the reference only names the aggregated
 * volumes d_cost_volumel/r_after_aggr (process_functional.py:268,347).
 */
int sde_cbca_pair(float *cv_l, float *tmp_l, float *cv_r, float *tmp_r, const uint32_t *arms_l,
                  const uint32_t *arms_r, int H, int W, int D, int L1, int iters, void *ws, size_t ws_bytes,
                  void *stream);

/*
 * The GPU path's pair (d_cost_volumel/r_after_aggr, process_functional.py:268,
 * 347): cv_l aggregated in place (tmp: scratch), then every valid voxel of cv_r
 * set to its shear, cv_r(y,x',d) = cv_l(y,x'+d,d) for x'+d < W (the others are
 * left as they are).  Equals sde_cbca_pair whenever cv_r's valid voxels are
 * the shear of cv_l's -- as sde_cost_volume(..., SDE_LAYOUT_HWD) writes them --
 * at half its traffic: one volume aggregated, one shear.
 */
int sde_cbca_lr(float *cv_l, float *cv_r, float *tmp, const uint32_t *arms_l, const uint32_t *arms_r, int H, int W,
                int D, int L1, int iters, void *ws, size_t ws_bytes, void *stream);
/* sde_cbca* shape limits (32-bit offsets, refused with SDE_ERR_ARG): D <= 512,
 * (5R + 5) * 4*W*D < 2^31 with R = 13 (L1 <= 14), 15 (L1 <= 16) or 31, and
 * 4 * roundup(H, 4) * W < 2^31. */

/* The fp64 reciprocals the aggregation multiplies by, out[i] = 1/(i+1) as the
 * kernels compute it (the tests check them against the IEEE quotient). */
int sde_cbca_reciprocals(double *out, int n, void *stream);

/*
 * is_error_match_kernel (process_functional.py:977-1000): lrc_l / lrc_r u8 [H][W], caller-zeroed.  In float64,
 * with col = the reference's uint8 cast of c (truncation toward zero, then the low byte of the two's-complement
 * integer; 0 for |c| >= 2^63, whose low byte is 0):
 *   left  pixel, d = disp_l[y][x], c = x - d: if 0 <= c < +inf and col < W, lrc_l = |d - disp_r[y][col]| > 1
 *   right pixel, d = disp_r[y][x], c = x + d: if -inf < c < W  and col < W, lrc_r = |d - disp_l[y][col]| > 1
 * Every other pixel is skipped: its byte stays as the caller set it.  That covers a NaN or infinite c, and for
 * W < 256 a cast column past the row (a left -1 at x = W - 1 gives column W, a right -1 at x = 0 column 255; -1
 * is what sde_wta's SDE_WTA_INIT_INF writes for "no winner").  Never reads outside the row, and the result is
 * defined for every float input.
 */
int sde_lr_check(const float *disp_l, const float *disp_r, int H, int W, uint8_t *lrc_l, uint8_t *lrc_r,
                 void *stream);

/*
 * Left-right consistency without sde_lr_check's uint8 column cast (the reference indexes column (x -+ d) & 255,
 * which checks consistency only for W <= 256).  The same float64 arithmetic with the column taken as the plain
 * truncated integer; lrc_l / lrc_r u8 [H][W], every pixel written (no zeroing needed), max_diff >= 0:
 *   lrc_l = 1 iff d = disp_l[y][x] < 0, or x - d >= 0 and |d - disp_r[y][(int)(x-d)]| > max_diff; else 0
 *   lrc_r = 1 iff d = disp_r[y][x] < 0, or x + d <  W and |d - disp_l[y][(int)(x+d)]| > max_diff; else 0
 * Never reads outside the row.  For W <= 256, non-negative disparities and max_diff = 1 it equals sde_lr_check
 * on zeroed buffers.  Composes with sde_cv_wta / sde_cv_wta_right, sde_lrc_fill and sde_median5.
 */
int sde_lr_consistency(const float *disp_l, const float *disp_r, int H, int W, float max_diff, uint8_t *lrc_l,
                       uint8_t *lrc_r, void *stream);

/* LRC_kernel left output (process_functional.py:1003-1088).  Two linear scans instead of
 * the reference's per-pixel walks; `out` doubles as scratch, so out != disp_l.  Requires
 * H < 65535 and W < 65535 (16-bit row / column indices; the row pass keeps 2 B per column in LDS). */
int sde_lrc_fill(const float *disp_l, const uint8_t *lrc_l, int H, int W, float *out, void *stream);

/* Median_Filter_kernel (process_functional.py:840-879): 5x5 median of src into the interior of dst. */
int sde_median5(const float *src, int H, int W, float *dst, void *stream);

/* ---------------------------------------------------------------------- */
/* Sub-pixel disparities and the 9x9 bilateral filter: the two stages the    */
/* reference carries switched off (process_functional.py:813-819, :830-836;  */
/* :882-974 with its call commented out at :1260).  Additive in ABI 4.      */
/* ---------------------------------------------------------------------- */
/*
 * The parabola step refine(i, lo, hi, c-, c0, c+): i the integer winner, c-, c0, c+ the float32 costs at i - 1,
 * i, i + 1.  The result is float32(i) unless lo < i < hi - 1, the three costs are finite and den > 0; then, with
 * Numba's promotion of `index - (c_ - _c)/(2*(_c + c_ - 2*c))` (:818) and every operation rounded to nearest on
 * its own (nothing fused):
 *   num = float32(c+ - c-);  s = float32(c- + c+);          float32 subtraction and addition
 *   den = 2.0 * ((double)s - 2.0 * (double)c0);             float64
 *   result = float32((double)i - (double)num / den)         float64 division and subtraction, one rounding
 * The three guards are the only departures from the reference's dead code, which would produce inf or NaN
 * without them.  There is no clamp: with costs a few ulps apart the offset can exceed 0.5 (costs [2, c+5u, c, c, 3]
 * at c = 1, u = ulp(c) give 2.625).
 */

/*
 * sde_wta followed by the parabola step on the stored volume: i is exactly sde_wta's winner for the same
 * (layout, rule), lo = 0, hi = D, and the three costs are read from the volume as they stand.  A pixel without a
 * winner keeps -1.0f.  Argument checks are sde_wta's.
 */
int sde_wta_subpixel(const float *vol, int H, int W, int D, int layout, int rule, float *disp, void *stream);

/*
 * The parabola step for the fused cost volume + WTA (sde_cv_wta / sde_cv_wta_right), which store no volume: a
 * pixel of disp_in that is not an integer in [d0, d1) is copied through bit for bit (-1 and NaN included);
 * otherwise i is that integer, lo = d0, hi = d1 and the three costs are the values
 * sde_cost_volume(..., SDE_LAYOUT_DHW) holds, recomputed in its exact arithmetic:
 *   side = SDE_SIDE_LEFT:  x - d >= 0 ? cost(x, d)     : -0.0f
 *   side = SDE_SIDE_RIGHT: x + d <  W ? cost(x + d, d) : -0.0f      (sde_cv_wta_right's indexing)
 * So on sde_cv_wta's map over [0, D) it equals sde_wta_subpixel of the stored DHW volume, by bytes.  fl / fr:
 * the [H][W][C] maps sde_cv_wta takes; disp_out == disp_in is allowed (each pixel reads only itself).
 * SDE_ERR_ARG: a null pointer, H, W or C < 1, d0 < 0, d1 <= d0, d1 > 2^24, side not exactly one of the two.
 */
int sde_cv_subpixel(const float *fl, const float *fr, int H, int W, int C, int d0, int d1, int side,
                    const float *disp_in, float *disp_out, void *stream);

/*
 * Bilateral_Filter_kernel (process_functional.py:882-974) for one view: img_u8 / src / dst [H][W], dst != src,
 * every pixel of dst written.  For pixel (y, x), with wsum = dsum = 0.0 in float64 and for i = -4..4 (outer),
 * j = -4..4 (inner): I' = img[y+i][x+j], d' = src[y+i][x+j], both 0 outside the image (the reference's
 * zero-padded tile); a = |int(img[y][x]) - int(I')|; if a < 5: w = float32(weights[a]) with the reference's
 * literals 0.167747, 0.165145, 0.157581, 0.145735, 0.130632 (:920-924; entries 5..9 are unreachable),
 * wsum += (double)w, dsum += (double)float32(w * d').  dst = float32(dsum / wsum).  The sequential order is part
 * of the definition; the centre tap always counts, so wsum > 0; non-finite disparities propagate as the
 * arithmetic says.  The reference's staging overrun (`id + 512 < 596`, :939) touches no value that is read and is
 * not reproduced.  H <= 16 * 65535.
 */
int sde_bilateral9(const uint8_t *img_u8, const float *src, int H, int W, float *dst, void *stream);

/* ---------------------------------------------------------------------- */
/* Local matcher (local_mathod.py): SAD+SSD, rank and census.  It needs no   */
/* weights: two uint8 images in, disparity maps out.  Additive in ABI 4.    */
/* ---------------------------------------------------------------------- */
/*
 * Images are uint8 [H][W] (the reference reads cv2.IMREAD_GRAYSCALE and casts to float32: every value is an
 * integer 0..255, so integer arithmetic reproduces its float arithmetic exactly); a pixel outside the image
 * reads as 0.  Volumes are float32 [H][W][D] (SDE_LAYOUT_HWD, what sde_sgm_8path* takes), disparities
 * float32 [H][W].  Limits of every entry point: H, W >= 1, 1 <= D <= 512; null or misordered arguments
 * return SDE_ERR_ARG before any launch.
 *
 * SDE_LOCAL_INVALID: the float32 nearest the reference's literal 999999999999 (AD / Census_Cost fill,
 * :49,150) = 999999995904, bits 0x5368d4a5.
 *
 * Census (Census_transform, :77-130): a 19-bit word built most-significant bit first --
 *   for r in y-3..y-1 (outer), c in x-4..x-1 (inner): append I(r,c) > I(2y-r, 2x-c);
 *   for r in y-3..y-1:                                append I(r,x) > I(2y-r, x);
 *   for c in x-4..x-1:                                append I(y,c) > I(y, 2x-c).
 * Not symmetric under a horizontal flip (the right view below cannot be built by flipping the images).
 *
 * Rank (Rank_transform, :51-75): the number of (r,c) in the 7x7 window around (y,x), centre included, with
 * I(y,x) >= I(r,c): 1..49, stored as uint8.
 *
 * Hamming cost (Census_Cost, :132-150), left view:  L(y,x,d)  = popcount(cl[y][x] ^ cr[y][x-d]) for x-d >= 0,
 * else `invalid`.  Right view (the standard construction, as sde_cost_volume's right side):
 *                                                   R(y,x',d) = popcount(cl[y][x'+d] ^ cr[y][x']) for x'+d < W,
 * else `invalid`; so R(y,x',d) == L(y,x'+d,d) on valid voxels.
 *
 * SAD+SSD cost (AD, :13-49), radius k (the script's -k), 0 <= k <= SDE_LOCAL_MAX_RADIUS:
 *   e(r,c,d) = |l(r,c) - r_img(r,c-d)| + (l(r,c) - r_img(r,c-d))^2 as a signed integer;
 *   rows max(y-k,0) .. min(y+k,H-1); columns by the reference's three branches:
 *       x <  D+k                   [x,   x+k]
 *       x >= D+k and x+k < W-k     [x-k, x+k]
 *       otherwise                  [x-k, x]
 *   cost(y,x,d) = float32(sum of e), rounded to nearest even from the exact integer, for x-d >= 0, else
 *   `invalid` (Numba accumulates in float64, exact here, and stores float32: the same bits).  The first
 *   branch reads column x+k, which the reference reads out of bounds when W < D+2k: the entry points
 *   REQUIRE W >= D + 2k (SDE_ERR_ARG otherwise).  The largest sum is 65^2 * 65280 < 2^31.
 *
 * WTA (WTA__kernel, :152-165): best = c(0); for d = 1..D-1 take d if best > c(d) -- the first strict
 * minimum, the rule of SDE_WTA_INIT_D0.  d = 0 is always valid and every real cost is below `invalid`, so
 * the fused forms never return an invalid voxel and do not depend on `invalid`.
 *
 * Rank+SAD (the script's commented chain :203-204) is sde_ad_* on the two rank images, with the SIGNED
 * difference.  The reference would subtract uint32 arrays there and Numba's unsigned arithmetic wraps; that
 * wrap is not reproduced -- parity unpinned for this chain.
 */
#define SDE_LOCAL_MAX_RADIUS 32
#define SDE_LOCAL_INVALID 999999995904.0f

/* imgs: [nimg][H][W] (e.g. the left and right image back to back), census / rank: [nimg][H][W]. */
int sde_census_transform(const uint8_t *imgs, int nimg, int H, int W, uint32_t *census, void *stream);
int sde_rank_transform(const uint8_t *imgs, int nimg, int H, int W, uint8_t *rank, void *stream);

/* The Hamming volumes; either output may be NULL, not both. */
int sde_census_cost(const uint32_t *census_l, const uint32_t *census_r, int H, int W, int D, float invalid,
                    float *out_left, float *out_right, void *stream);

/*
 * Hamming cost + WTA of both views in one pass, no volume written: disp_* the first minimum over d as float32,
 * min_* (optional) the winner's cost as float32.  At least one of disp_l / disp_r; a view's min needs its disp.
 * Equals sde_wta(sde_census_cost(...), SDE_LAYOUT_HWD, SDE_WTA_INIT_D0) per view.  H <= 65535.
 */
int sde_census_wta(const uint32_t *census_l, const uint32_t *census_r, int H, int W, int D, float *disp_l,
                   float *min_l, float *disp_r, float *min_r, void *stream);

/* The SAD+SSD volume (left view; the reference defines no right view for its one-sided windows). */
int sde_ad_cost(const uint8_t *img_l, const uint8_t *img_r, int H, int W, int D, int radius, float invalid,
                float *out_left, void *stream);

/* SAD+SSD cost + WTA, no volume written: disp, and min_cost (optional) the winner's cost as float32.
 * Equals sde_wta(sde_ad_cost(...), SDE_LAYOUT_HWD, SDE_WTA_INIT_D0).  H <= 4 * 65535. */
int sde_ad_wta(const uint8_t *img_l, const uint8_t *img_r, int H, int W, int D, int radius, float *disp,
               float *min_cost, void *stream);

/* ---------------------------------------------------------------------- */
/* Training of the MC-CNN-fast branch (train.py:71-99, mc_cnn_brunch.py:31-48):  */
/* hinge loss over (left, positive, negative) patch triplets, momentum SGD.    */
/* Additive in ABI 4.                                                       */
/* ---------------------------------------------------------------------- */
/*
 * Limits of every entry point: nf == 64, 1 <= nlayers <= 5, B >= 1 and 3*B*P*P*64 < 2^31 with the patch side
 * P = 2*nlayers + 1 (32-bit offsets); anything else, a null pointer or a short workspace returns SDE_ERR_ARG
 * before any launch (the size queries return -1).  fp32 storage, fp32 FMA accumulation.
 *
 * Parameter blob (also the layout of gradients and momentum velocity): float32, the reference's variable order
 * and HWIO layout -- w1 [3][3][1][nf], b1 [nf], w2 [3][3][nf][nf], b2 [nf], ...
 *
 * Definition.  N = 3B patches, left / positive / negative back to back, each through the same tower:
 *   conv        out[y][x][co] = b[co] + sum in[y+ky][x+kx][ci] * w[ky][kx][ci][co]   (VALID), ReLU on all but the last
 *   normalise   y = x * r,  r = 1/sqrt(max(sum x^2, 1e-12))
 *   h_i = margin - (l_i.p_i - l_i.n_i),  loss = mean_i max(0, h_i)
 * and backward: ReLU gradient [z > 0]; normalise dx = r * (g - y * (y.g)) where sum x^2 >= 1e-12, else 1e6 * g;
 * a_i = [h_i > 0] / B, dl_i = a_i * (n_i - p_i), dp_i = -a_i * l_i, dn_i = a_i * l_i; weight and bias
 * gradients summed over all 3B patches.  No floating-point atomics and a reduction order that depends on the
 * shape alone: the same inputs give the same bytes.
 */
int64_t sde_train_param_floats(int nlayers, int nf);
int64_t sde_train_workspace_bytes(int B, int nlayers, int nf);

/* img_l / img_r: float32 [H][W] normalised images; idx: int32 [B][4] = (y, x_left, x_pos, x_neg) patch centres;
 * patches: float32 [3][B][P][P] (left, positive, negative).  A pixel outside the image reads 0 (the tower's
 * zero padding). */
int sde_train_gather(const float *img_l, const float *img_r, int H, int W, const int32_t *idx, int B, int nlayers,
                     float *patches, void *stream);

/* Forward + backward.  loss: float32 [1 + B] = the mean, then every h_i.  grads: the blob layout, every element
 * written; NULL = forward only.  ws: sde_train_workspace_bytes(B, nlayers, nf), 16-byte aligned like params (SDE_ERR_ARG otherwise);
 * it keeps the activations for sde_train_export_activations. */
int sde_train_loss_grad(const float *patches, int B, const float *params, int nlayers, int nf, float margin,
                        float *loss, float *grads, void *ws, int64_t ws_bytes, void *stream);

/* Copy what the last sde_train_loss_grad on ws kept for `layer` (1-based) to out [3B][h][w][nf]: the post-ReLU
 * output of a layer < nlayers (h = w = P - 2*layer), the normalised features [3B][nf] for layer == nlayers. */
int sde_train_export_activations(const void *ws, int B, int nlayers, int nf, int layer, float *out, void *stream);

/* TF's MomentumOptimizer (non-Nesterov), one fp32 rounding per operation:
 * v = fl(fl(beta * v) + g); p = fl(p - fl(lr * v)).  n floats each. */
int sde_train_momentum(float *params, float *velocity, const float *grads, int64_t n, float lr, float beta,
                       void *stream);

/* ---------------------------------------------------------------------- */
/* Training from resident stereo scenes (image_patches_prepare/*.py) and   */
/* the bad-pixel rate (error_calculate.py).  Additive in ABI 4.            */
/* ---------------------------------------------------------------------- */
#define SDE_ZERO_IS_INVALID 1       /* sde_triplet_centres flag: a disparity of 0 marks an unknown pixel */
#define SDE_SCENE_WORDS 8           /* int64 words per scene in the table of sde_train_sample_gather */
#define SDE_SAMPLE_MAX_ROUNDS 32

/*
 * The valid patch centres of one scene.  h = nlayers, P = 2h + 1.  Pixel (y, x) with d = disp_l[y][x] is a
 * centre iff (every comparison on the values widened to double)
 *   d is finite, d >= 0 and, with SDE_ZERO_IS_INVALID, d != 0;
 *   h <= y < H - h and h <= x < W - h;   d + h <= x;
 *   with disp_r (may be NULL): r = disp_r[y][trunc(x - d)] is finite (with the flag, r != 0) and |r - d| <= 1.
 * centres: int32, capacity H*W; on return its first *count entries hold y*W + x in ascending order.  The last
 * H entries are used as scratch (per-row counts; no centre can land there: count <= (H-2)(W-2) <= H*W - H);
 * nothing else is written.  count: one device int32.  Two launches, no atomics: the same maps give the same
 * bytes.  SDE_ERR_ARG before any launch: H < P, W < P + 12, H*W >= 2^31, nlayers outside 1..5, unknown flag
 * bits, a null disp_l / centres / count.
 */
int sde_triplet_centres(const float *disp_l, const float *disp_r, int H, int W, int nlayers, int flags,
                        int32_t *centres, int32_t *count, void *stream);

/*
 * Draw B triplets from S resident scenes and gather their patches, in one launch.
 * table: device int64 [S][SDE_SCENE_WORDS] = {img_l, img_r, disp_l, centres (device addresses), H, W, first,
 * count}; img_* float32 [H][W] normalised images, disp_l the map sde_triplet_centres read, centres / count its
 * result, first = the sum of count over the scenes before this one, N = the sum over all.  The library checks
 * the scalars (S >= 1, 1 <= N < 2^31, B and nlayers as above, 1 <= max_rounds <= SDE_SAMPLE_MAX_ROUNDS, non-null
 * table and patches) and TRUSTS THE TABLE: a table that does not describe live buffers of those sizes is the
 * caller's error.
 *
 * Triplet i: Philox4x32-10 with key (seed lo, seed hi) and counter (i, step lo, step hi, tag) gives x0..x3;
 * U = ((x0 << 21) | (x1 >> 11)) * 2^-53 in double.
 *   centre    tag 0: g = (x0 * N) >> 32 (64-bit product); scene s has first_s <= g < first_s + count_s;
 *             (y, x) from centres_s[g - first_s]; rc = (double)x - (double)disp_l_s[y][x]
 *   positive  round r < max_rounds, tag 1 + r: pos = trunc(rc + (-0.501 + 1.002 * U)), accepted iff
 *             h <= pos < W_s - h; no round accepted: pos = trunc(rc)
 *   negative  round r, tag 33 + r: dev = 1.5 + 4.5 * U, neg = trunc(rc - dev) if x2 & 1 else trunc(rc + dev),
 *             same test; no round accepted: neg = pos + 2 if that is accepted, else pos - 2
 * every double operation rounded on its own.  patches: float32 [3][B][P][P] as sde_train_gather writes them
 * from (y, x, pos, neg), a pixel outside the image reading 0; idx (optional): int32 [B][4] = (y, x, pos, neg);
 * scene (optional): int32 [B].  The result depends on (seed, step, i, table) alone.
 */
int sde_train_sample_gather(const int64_t *table, int S, int64_t N, int B, int nlayers, uint64_t seed, uint64_t step,
                            int max_rounds, float *patches, int32_t *idx, int32_t *scene, void *stream);

/*
 * error_calculate.py:72-81.  A pixel whose gt is +inf or 0 is skipped; any other is evaluated, and bad iff
 * |(double)disp - (double)gt| > threshold (a NaN gt is evaluated and never bad).  counts: uint32 [2] =
 * (evaluated, bad), ADDED to what the words hold (integer atomics, one per block and word: exact, order-free;
 * the caller zeroes them and keeps the sum below 2^32).  area (optional): uint8 [H][W][3], every byte written:
 * skipped 0,0,0; good 0,255,0; bad 0,0,255.  SDE_ERR_ARG: H or W < 1, H*W >= 2^31, a threshold that is negative
 * or NaN, a null disp / gt / counts.
 */
int sde_bad_pixels(const float *disp, const float *gt, int H, int W, double threshold, uint32_t *counts,
                   uint8_t *area, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDE_H */
