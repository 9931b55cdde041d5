// tower.hip -- MC-CNN-fast Siamese branch on the MFMA units (gfx950).
//
// Replaces mc_cnn_brunch.py:31-48 (Net.construct) + :70-92 (conv) as run by
// compute_feature (process_functional.py:21-39): nlayers x [3x3 VALID conv,
// bias, ReLU] (no ReLU on the last), then tf.nn.l2_normalize over channels.
// Layers 2..n are implicit GEMMs: out[n][pixel] = sum over (tap, c) of
// W[tap][n][c] * in[pixel + tap][c], M = 64 output maps, K = 9 taps x 64 maps.
// Layer 1 (Cin = 1, 9 MACs per output) is computed on VALU straight into layer
// 2's input staging, so its output never touches HBM; the last layer's epilogue
// L2-normalises each pixel (and can emit the certified cost volume's bf16 split
// planes and norm bounds).
//
// This file: the C ABI, the argument rules and the dispatch; the kernels live one family per header, each
// instantiated in its own tower_<family>.hip behind a launcher (tower_launch.h; file map in DESIGN.md 3.2).
#include "tower_launch.h"
#include <algorithm>
#include <atomic>

namespace sde {

// max |x| over n floats, atomically maxed (as float bits) into *amax (F16 tower scaling):
// float4 grid-stride loads, one atomic per workgroup.
__global__ __launch_bounds__(256) void absmax_kernel(const float *__restrict__ x, int64_t n, float *__restrict__ amax,
                                                     int amax_stride)
{
    x += blockIdx.y * n;        // batch: image blockIdx.y -> amax[blockIdx.y * amax_stride]
    amax += blockIdx.y * amax_stride;
    float m = 0.0f;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    const int64_t head = std::min<int64_t>(n, (16 - (reinterpret_cast<uintptr_t>(x) & 15)) / 4 & 3);
    if (tid < head) m = fabsf(x[tid]);
    const float4 *x4 = reinterpret_cast<const float4 *>(x + head);
    const int64_t n4 = (n - head) / 4;
    for (int64_t i = tid; i < n4; i += nt) {
        const float4 v = x4[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    for (int64_t i = head + 4 * n4 + tid; i < n; i += nt) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicMax(reinterpret_cast<unsigned int *>(amax),
                  __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// nlayers == 1: conv1 + L2 normalisation only (no ReLU on the last layer).
__global__ __launch_bounds__(256) void conv1_only_kernel(const float *__restrict__ img, int Hin, int Win,
                                                         const float *__restrict__ w1blob, float *__restrict__ out)
{
    const int Ho = Hin - 2, Wo = Win - 2;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)Ho * Wo) return;
    const int y = (int)(p / Wo), x = (int)(p % Wo);
    const float *b1 = w1blob, *w1 = w1blob + NF;
    float im[9];
    for (int t = 0; t < 9; t++) im[t] = img[(size_t)(y + t / 3) * Win + x + t % 3];
    float v[NF];
    float ss = 0.0f;
    for (int n = 0; n < NF; n++) {
        float s = 0.0f;
        for (int t = 0; t < 9; t++) s = fmaf(im[t], w1[t * NF + n], s);
        v[n] = s + b1[n];
        ss += v[n] * v[n];
    }
    const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
    for (int n = 0; n < NF; n++) out[p * NF + n] = v[n] * inv;
}

}  // namespace sde

using namespace sde;

static constexpr int64_t TOWER_AMAX_BYTES = 256;   // 64 bound words (nlayers <= 64)

SDE_EXPORT int64_t sde_tower_batch_workspace_bytes(int H, int W, int nimg, int nlayers, int nf)
{
    if (H <= 0 || W <= 0 || nimg <= 0 || nlayers < 1 || nf != NF) return -1;
    if (nlayers == 1) return 0;
    // two ping-pong activation buffers sized for layer 2's output (nimg images each), then the
    // F16X3 bound words (64 per image)
    const int64_t h2 = H + 2 * (nlayers - 2), w2 = W + 2 * (nlayers - 2);
    return (nlayers > 2 ? 2 * nimg * h2 * w2 * NF * (int64_t)sizeof(float) : 0) + nimg * TOWER_AMAX_BYTES;
}

SDE_EXPORT int64_t sde_tower_workspace_bytes(int H, int W, int nlayers, int nf)
{
    return sde_tower_batch_workspace_bytes(H, W, 1, nlayers, nf);
}

// Persistent tower grids: one workgroup per CU (160 KB of LDS each), or g_grid_cus workgroups when set
// (sde_set_persistent_grid: the tower sharing the device with other work on CU-masked streams, where a
// workgroup per device CU would leave the last ones waiting for CUs the other stream holds).
static std::atomic<int> g_grid_cus{0};

static int cu_count()
{
    const int cus = device_cus();
    const int g = g_grid_cus.load(std::memory_order_relaxed);
    return g > 0 ? std::min(g, cus) : cus;
}

// The tile space of a batch launch (tw x th output tiles, image-major) and the persistent grid that walks it
static int xp_batch(XpBatch &bt, int tw, int th, int hout, int wout, int nimg)
{
    bt.tiles_x = cdiv(wout, tw);
    bt.tiles_img = bt.tiles_x * cdiv(hout, th);
    bt.ntiles = bt.tiles_img * nimg;
    bt.pix_stride = (int64_t)hout * wout;
    return std::min(bt.ntiles, cu_count());
}

// One launch: layer == 2 -> conv1+conv2 fused from the padded image (Hin x Win floats);
// layer > 2 -> one 64->64 conv on Hin x Win x 64 activations.  Output (Hin-4|Hin-2) x ... x 64.
// The caller sets L's pointers, Hin, Win, nimg, bt's three strides, the stream and the four layout booleans.
static void launch_layer(TowerLaunch L, const float *packed, int nlayers, int layer, int flags)
{
    L.first = (layer == 2);
    L.last = (layer == nlayers);
    L.f16 = (flags & SDE_TOWER_F16X3) != 0;
    const bool x6 = L.f16 || (flags & SDE_TOWER_BF16X6) != 0;
    const bool h16 = L.f16 && !(flags & SDE_TOWER_MFMA32);   // v_mfma_f32_16x16x32_f16 (tower_h16.h)
    L.w1 = packed;
    L.wk = packed + L1_FLOATS + (int64_t)(layer - 2) * LK_FLOATS;
    L.hout = L.Hin - (L.first ? 4 : 2);
    L.wout = L.Win - (L.first ? 4 : 2);
    // the Winograd kernel's input / output descriptors span a whole image with 32-bit record
    // counts and offsets (tower_wino.h): planes of 4 GiB or more take the direct kernel, which
    // rebases its descriptors per tile (same f16x3 arithmetic, fp32-level error either way)
    const bool wino_fits = (int64_t)L.Hin * L.Win * 256 < ((int64_t)1 << 32) &&
                           (int64_t)L.hout * L.wout * 256 < ((int64_t)1 << 32);
    const bool wino = L.f16 && layer >= 3 && !L.ohi && !L.onrm && (flags & SDE_TOWER_WINOGRAD) && wino_fits;
    // the 16x16x32 kernels: layers 3..L run 16 x 16 tiles with the stores on the stager waves (tower_h16s.h) where
    // the activations are fp32 and no split feature planes are asked for, unless SDE_TOWER_TILE32 keeps the 16 x 32
    // kernel; layer 2 always runs the 16 x 32 kernel (its stagers compute conv1: +9 % with the stores on top)
    const bool h16k = !wino && h16 && (layer >= 3 || !L.last);
    const bool h16s = h16k && !L.first && !(flags & SDE_TOWER_TILE32) && !L.in_sp && !L.out_sp && !L.ohi && !L.onrm;
    L.grid = xp_batch(L.bt, wino ? WN_TX : h16s ? 16 : XP_TX, wino ? WN_TY : XP_TY, L.hout, L.wout, L.nimg);
    if (wino) launch_wino(L);
    else if (h16s) launch_h16s(L);
    else if (h16k) launch_h16(L);
    else if (x6) launch_x6p(L);
    else launch_fp32(L);
}

// split activations (SDE_TOWER_IN_SPLIT / OUT_SPLIT): the scale word sits at bound word + XP_SCALE_WORD (so
// the bound-word arrays hold 64 words per image and a tower at most 32 layers), and a plane's bytes
// (h w 16) times 8 fit the 32-bit buffer offsets
static constexpr int64_t SPLIT_MAX_PIX = (int64_t)1 << 24;
#ifndef SDE_SPLIT_ACT
// 1: sde_tower_forward* pass split activations between the f16x3 64->64 layers (conv64_h16q_kernel in the
// middle); 0 (the default): fp32 c-blocks.  Same time within 0.5 % on MI355X (the tower is
// power-capped, and the split path moves the fp16 split from the stagers into the MFMA waves' epilogue);
// ops.TOWER_SPLIT_ACT mirrors this for the layer-by-layer drivers.
#define SDE_SPLIT_ACT 0
#endif
static bool split_ok(int nlayers, int64_t pix) { return nlayers <= XP_SCALE_WORD && pix < SPLIT_MAX_PIX; }
// the kernels that exist: layer 2 may write split planes; a middle layer reads them iff it writes them; the
// last layer may read them
static bool split_pairing_ok(bool in_sp, bool out_sp, int layer, int nlayers, int Hin, int Win)
{
    if (!in_sp && !out_sp) return true;
    // the pixel limit applies to the split plane itself: the input plane for IN_SPLIT, the output plane (what the
    // forward checks for layer 2's split outputs, h2 * w2) for OUT_SPLIT
    const int sh = layer == 2 ? 4 : 2;
    if ((in_sp && !split_ok(nlayers, (int64_t)Hin * Win)) || (out_sp && !split_ok(nlayers, (int64_t)(Hin - sh) * (Win - sh))))
        return false;
    if ((in_sp && layer == 2) || (out_sp && layer == nlayers)) return false;
    return layer == 2 || layer == nlayers || in_sp == out_sp;
}

SDE_EXPORT int sde_tower_split_act(void) { return SDE_SPLIT_ACT; }

static bool tower_flags_ok(int flags, bool layer_api)
{
    if (flags & (SDE_TOWER_IN_SPLIT | SDE_TOWER_OUT_SPLIT)) {   // F16X3 on the 16x16x32 kernel (layer API only)
        if (!layer_api || !(flags & SDE_TOWER_F16X3) || (flags & (SDE_TOWER_WINOGRAD | SDE_TOWER_MFMA32))) return false;
        if ((flags & SDE_TOWER_IN_SPLIT && flags & SDE_TOWER_IN_CBLOCK) ||
            (flags & SDE_TOWER_OUT_SPLIT && flags & SDE_TOWER_OUT_CBLOCK)) return false;
        flags &= ~(SDE_TOWER_IN_SPLIT | SDE_TOWER_OUT_SPLIT);
    }
    if (flags & SDE_TOWER_TILE32) {   // F16X3 on the 16x16x32 kernels: their tile (a no-op where only the 16 x 32 kernel exists)
        if (!(flags & SDE_TOWER_F16X3) || (flags & SDE_TOWER_MFMA32)) return false;
        flags &= ~SDE_TOWER_TILE32;
    }
    if (flags & (SDE_TOWER_WINOGRAD | SDE_TOWER_MFMA32)) {   // F16X3 only: the 64 -> 64 layers' kernel choice
        if (!(flags & SDE_TOWER_F16X3) || (flags & SDE_TOWER_WINOGRAD && flags & SDE_TOWER_MFMA32)) return false;
        flags &= ~(SDE_TOWER_WINOGRAD | SDE_TOWER_MFMA32);
    }
    const int prec = flags & (SDE_TOWER_BF16X6 | SDE_TOWER_F16X3);
    if (prec == (SDE_TOWER_BF16X6 | SDE_TOWER_F16X3)) return false;
    const int layout = SDE_TOWER_IN_CBLOCK | SDE_TOWER_OUT_CBLOCK;
    if (!layer_api) return (flags & ~(SDE_TOWER_BF16X6 | SDE_TOWER_F16X3)) == 0;
    if (flags & ~(SDE_TOWER_BF16X6 | SDE_TOWER_F16X3 | layout)) return false;
    return !((flags & layout) && prec == 0);
}

// Sets L's layout booleans from the flags, then the checks sde_tower_layer_scaled and sde_tower_layer_batch share.
static bool layer_set_layout_and_check(TowerLaunch &L, const float *packed, int nlayers, int nf, int layer, int flags)
{
    L.in_cb = (flags & SDE_TOWER_IN_CBLOCK) != 0, L.out_cb = (flags & SDE_TOWER_OUT_CBLOCK) != 0;
    L.in_sp = (flags & SDE_TOWER_IN_SPLIT) != 0, L.out_sp = (flags & SDE_TOWER_OUT_SPLIT) != 0;
    if (!L.in || !packed || !L.out || nf != NF || nlayers < 2 || layer < 2 || layer > nlayers) return false;
    if (L.Hin < (layer == 2 ? 5 : 3) || L.Win < (layer == 2 ? 5 : 3)) return false;
    if (!tower_flags_ok(flags, true)) return false;
    if ((L.in_cb && layer == 2) || (L.out_cb && layer == nlayers)) return false;
    if ((flags & SDE_TOWER_F16X3) && (!L.in_amax || (layer < nlayers && !L.out_amax))) return false;
    return split_pairing_ok(L.in_sp, L.out_sp, layer, nlayers, L.Hin, L.Win);
}

SDE_EXPORT int sde_tower_layer_scaled(const float *in, int Hin, int Win, const float *packed, int nlayers, int nf,
                                      int layer, float *out, int flags, uint16_t *feat_hi, uint16_t *feat_lo,
                                      float *feat_norm, const float *in_absmax, float *out_absmax, void *stream)
{
    TowerLaunch L{};
    L.in = in, L.Hin = Hin, L.Win = Win, L.out = out, L.nimg = 1, L.st = as_stream(stream);
    L.ohi = feat_hi, L.olo = feat_lo, L.onrm = feat_norm, L.in_amax = in_absmax, L.out_amax = out_absmax;
    if (!layer_set_layout_and_check(L, packed, nlayers, nf, layer, flags) || (feat_hi != nullptr) != (feat_lo != nullptr))
        return SDE_ERR_ARG;
    launch_layer(L, packed, nlayers, layer, flags);
    return launch_status();
}

SDE_EXPORT int sde_tower_layer_batch(const float *in, int nimg, int64_t in_stride, int Hin, int Win,
                                     const float *packed, int nlayers, int nf, int layer, float *out,
                                     int64_t out_stride, int flags, const float *in_absmax, float *out_absmax,
                                     int amax_stride, void *stream)
{
    TowerLaunch L{};
    L.in = in, L.Hin = Hin, L.Win = Win, L.out = out, L.nimg = nimg, L.st = as_stream(stream);
    L.in_amax = in_absmax, L.out_amax = out_absmax;
    L.bt.in_stride = in_stride, L.bt.out_stride = out_stride, L.bt.amax_stride = amax_stride;
    if (!layer_set_layout_and_check(L, packed, nlayers, nf, layer, flags) || nimg <= 0) return SDE_ERR_ARG;
    const int64_t hout = Hin - (layer == 2 ? 4 : 2), wout = Win - (layer == 2 ? 4 : 2);
    const int64_t in_need = layer == 2 ? (int64_t)Hin * Win : (int64_t)Hin * Win * NF;
    if (nimg > 1 && (in_stride < in_need || out_stride < hout * wout * NF ||
                     (layer == nlayers && out_stride != hout * wout * NF))) return SDE_ERR_ARG;
    if ((flags & SDE_TOWER_F16X3) && nimg > 1 && amax_stride < 1) return SDE_ERR_ARG;
    // split activations: a layer's scale word sits 32 words past its bound word, which is column <= 31 of the
    // image's row; rows of fewer than 64 words would put image i's scale word on image i + 1's bound words
    if ((L.in_sp || L.out_sp) && nimg > 1 && amax_stride < (int)(TOWER_AMAX_BYTES / sizeof(float)))
        return SDE_ERR_ARG;
    launch_layer(L, packed, nlayers, layer, flags);
    return launch_status();
}

SDE_EXPORT int sde_tower_layer(const float *in, int Hin, int Win, const float *packed, int nlayers, int nf, int layer,
                               float *out, int flags, uint16_t *feat_hi, uint16_t *feat_lo, float *feat_norm,
                               void *stream)
{
    if (flags & SDE_TOWER_F16X3) return SDE_ERR_ARG;   // needs the bound words: sde_tower_layer_scaled
    return sde_tower_layer_scaled(in, Hin, Win, packed, nlayers, nf, layer, out, flags, feat_hi, feat_lo, feat_norm,
                                  nullptr, nullptr, stream);
}

SDE_EXPORT int sde_set_persistent_grid(int cus)
{
    if (cus < 0) return SDE_ERR_ARG;
    g_grid_cus.store(cus, std::memory_order_relaxed);
    return SDE_OK;
}

SDE_EXPORT int sde_absmax_f32(const float *x, int64_t n, float *absmax, void *stream)
{
    return sde_absmax_f32_batch(x, 1, n, absmax, 0, stream);
}

SDE_EXPORT int sde_absmax_f32_batch(const float *x, int nimg, int64_t n, float *absmax, int absmax_stride, void *stream)
{
    if (!absmax || n < 0 || nimg <= 0 || nimg > 65535 || absmax_stride < 0) return SDE_ERR_ARG;
    if (n == 0) return SDE_OK;
    if (!x) return SDE_ERR_ARG;
    const int blocks = (int)std::min<int64_t>(std::max(1, 256 / nimg), cdiv(n, 256 * 16));
    absmax_kernel<<<dim3(blocks, nimg), 256, 0, as_stream(stream)>>>(x, n, absmax, absmax_stride);
    return launch_status();
}

SDE_EXPORT int sde_tower_forward_batch(const float *img_pad, int nimg, int H, int W, const float *packed, int nlayers,
                                       int nf, float *feat, void *workspace, int64_t workspace_bytes, int flags,
                                       uint16_t *feat_hi, uint16_t *feat_lo, float *feat_norm, void *stream)
{
    if ((feat_hi != nullptr) != (feat_lo != nullptr)) return SDE_ERR_ARG;
    if (nlayers == 1 && (feat_hi || feat_norm)) return SDE_ERR_ARG;
    if (!img_pad || !packed || !feat || H <= 0 || W <= 0 || nimg <= 0 || nlayers < 1 || nf != NF) return SDE_ERR_ARG;
    if (!tower_flags_ok(flags, false)) return SDE_ERR_ARG;
    const int64_t need = sde_tower_batch_workspace_bytes(H, W, nimg, nlayers, nf);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SDE_ERR_WORKSPACE;
    hipStream_t st = as_stream(stream);
    const int Hp = H + 2 * nlayers, Wp = W + 2 * nlayers;
    const int64_t img_stride = (int64_t)Hp * Wp, feat_stride = (int64_t)H * W * NF;
    if (nlayers == 1) {
        for (int i = 0; i < nimg; i++)
            conv1_only_kernel<<<cdiv((int64_t)H * W, 256), 256, 0, st>>>(img_pad + i * img_stride, Hp, Wp, packed,
                                                                         feat + i * feat_stride);
        return launch_status();
    }
    float *buf[2] = {nullptr, nullptr};
    const int64_t h2 = H + 2 * (nlayers - 2), w2 = W + 2 * (nlayers - 2);
    const int64_t act_stride = h2 * w2 * NF;   // per image, sized for layer 2's output
    if (nlayers > 2) {
        buf[0] = reinterpret_cast<float *>(workspace);
        buf[1] = buf[0] + nimg * act_stride;
    }
    // F16X3 bound words: amax[i * 64 + l - 2] bounds |input of layer l| of image i
    float *amax = reinterpret_cast<float *>(static_cast<char *>(workspace) +
                                            (nlayers > 2 ? 2 * nimg * act_stride * 4 : 0));
    constexpr int AS = (int)(TOWER_AMAX_BYTES / 4);
    const bool f16 = (flags & SDE_TOWER_F16X3) != 0;
    if (f16) {
        if (nlayers > AS) return SDE_ERR_ARG;
        if (hipMemsetAsync(amax, 0, nimg * TOWER_AMAX_BYTES, st) != hipSuccess) return SDE_ERR_LAUNCH;
        // one launch for the batch: per-image bound words amax[i * AS]
        const int blocks = (int)std::min<int64_t>(std::max<int64_t>(1, 256 / nimg), cdiv(img_stride, 256 * 16));
        absmax_kernel<<<dim3(blocks, nimg), 256, 0, st>>>(img_pad, img_stride, amax, AS);
    }
    int hin = Hp, win = Wp;
    // intermediate activations: f16x3 on the 16x16x32 kernel -- split (scaled fp16 parts, staged by LDS-DMA);
    // the other split paths -- c-block-major fp32
    const bool sp = SDE_SPLIT_ACT && f16 && !(flags & (SDE_TOWER_WINOGRAD | SDE_TOWER_MFMA32)) && nlayers > 2 &&
                    split_ok(nlayers, h2 * w2);
    const bool cbl = !sp && (flags & (SDE_TOWER_BF16X6 | SDE_TOWER_F16X3)) != 0;
    TowerLaunch L{};
    L.ohi = feat_hi, L.olo = feat_lo, L.onrm = feat_norm, L.nimg = nimg, L.bt.amax_stride = AS, L.st = st;
    // layer l: the image (l == 2) or buf[(l & 1) ^ 1] -> buf[l & 1] or the features (l == nlayers)
    for (int l = 2; l <= nlayers; l++) {
        const bool first = l == 2, last = l == nlayers;
        L.in = first ? img_pad : buf[(l & 1) ^ 1], L.Hin = hin, L.Win = win, L.out = last ? feat : buf[l & 1];
        L.bt.in_stride = first ? img_stride : act_stride, L.bt.out_stride = last ? feat_stride : act_stride;
        L.in_amax = amax + (l - 2), L.out_amax = amax + (l - 1);
        L.in_cb = cbl && !first, L.out_cb = cbl && !last, L.in_sp = sp && !first, L.out_sp = sp && !last;
        launch_layer(L, packed, nlayers, l, flags);
        hin -= first ? 4 : 2, win -= first ? 4 : 2;
    }
    return launch_status();
}

SDE_EXPORT int sde_tower_forward(const float *img_pad, int H, int W, const float *packed, int nlayers, int nf,
                                 float *feat, void *workspace, int64_t workspace_bytes, int flags, uint16_t *feat_hi,
                                 uint16_t *feat_lo, float *feat_norm, void *stream)
{
    return sde_tower_forward_batch(img_pad, 1, H, W, packed, nlayers, nf, feat, workspace, workspace_bytes, flags,
                                   feat_hi, feat_lo, feat_norm, stream);
}
