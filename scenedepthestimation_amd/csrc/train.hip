// train.hip -- one MC-CNN-fast training step on the device (gfx950): patch gather, forward pass keeping the
// activations, hinge loss, backward pass and the momentum update.
//
// Replaces (train.py:71-99, mc_cnn_brunch.py:31-48): three weight-sharing towers over left / positive /
// negative 11x11 patches, loss = mean(max(0, margin - l.p + l.n)), MomentumOptimizer.  The definition of every
// quantity is stated in include/sde.h.
//
// Layouts.  N = 3B patches (left, positive, negative back to back), P = 2L + 1, s_k = P - 2k the side of layer
// k's output.  Activations are channels-last [N][s_k][s_k][64]; layers 1..L-1 keep their post-ReLU output (its
// sign is the ReLU mask), layer L keeps z [N][64] and the normalised y [N][64].  A conv layer's three passes
// are 64 x 64 register-tiled fp32 FMA products over LDS tiles:
//   forward        out[m][co] = b[co] + sum_tap in[m + tap][ci] * w[tap][ci][co]          (64 pixels per block)
//   backward data  din[m][ci] = [act > 0] * sum_tap dout[m - tap][co] * w[tap][ci][co]    (64 pixels per block)
//   backward wts   dw[tap][ci][co] = sum_m in[m + tap][ci] * dout[m][co]                  (one (chunk, tap) per block)
// The weight gradient's sum over pixels is cut into at most 128 chunks whose bounds depend on the shape alone;
// every block writes its partial sum and a second kernel adds the chunks in index order: no floating-point
// atomics, one fixed order, identical bytes on every run.
#include "sde_common.h"

namespace sde {

constexpr int TR_NF = 64;
constexpr int TR_MAX_LAYERS = 5;
constexpr int TR_MAX_CHUNKS = 128;
constexpr int TR_MIN_CHUNK = 256;      // pixels
constexpr int TR_SUB = 32;             // pixels per LDS step of the weight-gradient kernel
constexpr int TR_LDA = 68;             // LDS row pitch of the 64 x 64 tiles (floats): rows 4 banks apart, 16 B aligned

static inline int64_t tr_w_floats(int layer, int nf) { return 9ll * (layer == 1 ? 1 : nf) * nf; }

// float offset of layer k's weights in the parameter blob (its biases follow them)
static inline int64_t tr_param_offset(int layer, int nf)
{
    return layer == 1 ? 0 : (9ll * nf + nf) + (int64_t)(layer - 2) * (9ll * nf * nf + nf);
}

struct TrainLayout {
    int N, L, P;
    int side[TR_MAX_LAYERS + 1];        // side[k] = P - 2k
    int64_t act[TR_MAX_LAYERS + 1];     // float offsets: act[k], 1 <= k < L
    int64_t z, y, ss, dbuf[2], partial, total;
    int chunk[TR_MAX_LAYERS + 1], nchunks[TR_MAX_LAYERS + 1];
};

static inline int64_t up64(int64_t v) { return (v + 63) / 64 * 64; }

// false: unsupported shape, or offsets past what the kernels index with (32-bit)
static bool train_layout(int64_t B, int L, int nf, TrainLayout &t)
{
    if (nf != TR_NF || L < 1 || L > TR_MAX_LAYERS || B < 1) return false;
    const int P = 2 * L + 1;
    if (3 * B * P * P * TR_NF >= (1ll << 31)) return false;
    t.N = (int)(3 * B);
    t.L = L;
    t.P = P;
    int64_t off = 0, maxpart = 0;
    for (int k = 0; k <= L; k++) t.side[k] = P - 2 * k;
    for (int k = 1; k <= L; k++) {
        t.act[k] = off;
        if (k < L) off += up64((int64_t)t.N * t.side[k] * t.side[k] * TR_NF);
        const int64_t pix = (int64_t)t.N * t.side[k] * t.side[k];
        int64_t c = (pix + TR_MAX_CHUNKS - 1) / TR_MAX_CHUNKS;
        c = (c + TR_SUB - 1) / TR_SUB * TR_SUB;
        if (c < TR_MIN_CHUNK) c = TR_MIN_CHUNK;
        t.chunk[k] = (int)c;
        t.nchunks[k] = (int)((pix + c - 1) / c);
        const int64_t part = t.nchunks[k] * (tr_w_floats(k, nf) + nf);
        if (part > maxpart) maxpart = part;
    }
    t.z = off;  off += up64((int64_t)t.N * TR_NF);
    t.y = off;  off += up64((int64_t)t.N * TR_NF);
    t.ss = off; off += up64(t.N);
    const int64_t dsz = up64((int64_t)t.N * t.side[1] * t.side[1] * TR_NF);
    t.dbuf[0] = off; off += dsz;
    t.dbuf[1] = off; off += dsz;
    t.partial = off; off += up64(maxpart);
    t.total = off;
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// gather: one lane per patch pixel; a pixel outside the image reads 0
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void train_gather_kernel(const float *__restrict__ img_l, const float *__restrict__ img_r,
                                                           int H, int W, const int32_t *__restrict__ idx, int B, int P,
                                                           float *__restrict__ patches)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int pp = P * P;
    if (t >= 3 * B * pp) return;
    const int which = t / (B * pp), rem = t % (B * pp);
    const int b = rem / pp, q = rem % pp;
    const int r = P / 2;
    const long long y = (long long)idx[4 * b] + q / P - r;
    const long long x = (long long)idx[4 * b + 1 + which] + q % P - r;
    const float *img = which == 0 ? img_l : img_r;
    patches[t] = (y >= 0 && y < H && x >= 0 && x < W) ? img[(size_t)y * W + x] : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------
// layer 1 (one input channel): forward and weight gradient on plain lanes, 9 products per output
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void train_conv1_fwd_kernel(const float *__restrict__ patches, const float *__restrict__ w,
                                                              const float *__restrict__ bias, float *__restrict__ out,
                                                              int npix, int P, int relu)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = t / TR_NF, co = t % TR_NF;
    if (m >= npix) return;
    const int so = P - 2;
    const int n = m / (so * so), q = m % (so * so), y = q / so, x = q % so;
    const float *in = patches + ((size_t)n * P + y) * P + x;
    float acc = bias[co];
#pragma unroll
    for (int ky = 0; ky < 3; ky++)
#pragma unroll
        for (int kx = 0; kx < 3; kx++) acc = __builtin_fmaf(in[ky * P + kx], w[(ky * 3 + kx) * TR_NF + co], acc);
    out[(size_t)m * TR_NF + co] = relu ? fmaxf(acc, 0.0f) : acc;
}

// block = chunk; lane (co, g): group g sums taps g, g+4, g+8 (group 3: taps 3, 7 and the bias) over the chunk
__global__ __launch_bounds__(256) void train_conv1_wgrad_kernel(const float *__restrict__ patches,
                                                                const float *__restrict__ dout, int npix, int P, int chunk,
                                                                float *__restrict__ partial)
{
    const int co = threadIdx.x % TR_NF, g = threadIdx.x / TR_NF;
    const int so = P - 2;
    const int m0 = blockIdx.x * chunk, m1 = min(m0 + chunk, npix);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int m = m0; m < m1; m++) {
        const int n = m / (so * so), q = m % (so * so), y = q / so, x = q % so;
        const float *in = patches + ((size_t)n * P + y) * P + x;
        const float d = dout[(size_t)m * TR_NF + co];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int tap = g + 4 * j;
            if (tap < 9) acc[j] = __builtin_fmaf(in[(tap / 3) * P + tap % 3], d, acc[j]);
            else if (tap == 11) acc[j] += d;
        }
    }
    float *out = partial + (size_t)blockIdx.x * (9 * TR_NF + TR_NF);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int tap = g + 4 * j;
        if (tap < 9) out[tap * TR_NF + co] = acc[j];
        else if (tap == 11) out[9 * TR_NF + co] = acc[j];
    }
}

// ---------------------------------------------------------------------------------------------------------
// 64 -> 64 layers: forward (BWD = false) and backward data (BWD = true).  Block = 64 output pixels x 64
// channels, lane = 4 pixels (tp + 16 i) x 4 channels (4 tc ..), one LDS tile pair per tap.
//   forward:  so = the layer's output side, source side so + 2, source pixel (y + ky, x + kx), B[ci][co] = w
//   backward: so = the layer's input side,  source side so - 2, source pixel (y - ky, x - kx) or zero,
//             B[co][ci] = w transposed; the result is multiplied by [mask_src > 0]
// ---------------------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void train_conv64_kernel(const float *__restrict__ src, const float *__restrict__ w,
                                                           const float *__restrict__ bias,
                                                           const float *__restrict__ mask_src, float *__restrict__ out,
                                                           int npix, int so, int relu)
{
    __shared__ __attribute__((aligned(16))) float As[64 * TR_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[64 * TR_LDA];
    const int t = threadIdx.x, tc = t % 16, tp = t / 16;
    const int si = BWD ? so - 2 : so + 2;
    const int tile0 = blockIdx.x * 64;

    // the four rows this lane stages (and computes): tile row tp + 16 j
    int rn[4], ry[4], rx[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int m = tile0 + tp + 16 * j;
        if (m < npix) {
            rn[j] = m / (so * so);
            const int q = m % (so * so);
            ry[j] = q / so;
            rx[j] = q % so;
        } else {
            rn[j] = -1; ry[j] = 0; rx[j] = 0;
        }
    }

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[i][c] = BWD ? 0.0f : bias[4 * tc + c];

    for (int tap = 0; tap < 9; tap++) {
        const int ky = tap / 3, kx = tap % 3;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int yy = BWD ? ry[j] - ky : ry[j] + ky, xx = BWD ? rx[j] - kx : rx[j] + kx;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (rn[j] >= 0 && yy >= 0 && yy < si && xx >= 0 && xx < si)
                v = *reinterpret_cast<const float4 *>(src + (((size_t)rn[j] * si + yy) * si + xx) * TR_NF + 4 * tc);
            *reinterpret_cast<float4 *>(&As[(tp + 16 * j) * TR_LDA + 4 * tc]) = v;
        }
        const float *wt = w + (size_t)tap * TR_NF * TR_NF;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int ci = tp + 16 * j;
            const float4 v = *reinterpret_cast<const float4 *>(wt + ci * TR_NF + 4 * tc);
            if (BWD) {
                Bs[(4 * tc + 0) * TR_LDA + ci] = v.x;
                Bs[(4 * tc + 1) * TR_LDA + ci] = v.y;
                Bs[(4 * tc + 2) * TR_LDA + ci] = v.z;
                Bs[(4 * tc + 3) * TR_LDA + ci] = v.w;
            } else {
                *reinterpret_cast<float4 *>(&Bs[ci * TR_LDA + 4 * tc]) = v;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 64; k += 4) {
            float4 a[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = *reinterpret_cast<const float4 *>(&As[(tp + 16 * i) * TR_LDA + k]);
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const float4 b = *reinterpret_cast<const float4 *>(&Bs[(k + kk) * TR_LDA + 4 * tc]);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float av = kk == 0 ? a[i].x : kk == 1 ? a[i].y : kk == 2 ? a[i].z : a[i].w;
                    acc[i][0] = __builtin_fmaf(av, b.x, acc[i][0]);
                    acc[i][1] = __builtin_fmaf(av, b.y, acc[i][1]);
                    acc[i][2] = __builtin_fmaf(av, b.z, acc[i][2]);
                    acc[i][3] = __builtin_fmaf(av, b.w, acc[i][3]);
                }
            }
        }
    }

#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = tile0 + tp + 16 * i;
        if (m >= npix) continue;
        float *o = out + (size_t)m * TR_NF + 4 * tc;
        if (BWD) {
            const float *ms = mask_src + (size_t)m * TR_NF + 4 * tc;
#pragma unroll
            for (int c = 0; c < 4; c++) o[c] = ms[c] > 0.0f ? acc[i][c] : 0.0f;
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) o[c] = relu ? fmaxf(acc[i][c], 0.0f) : acc[i][c];
        }
    }
}

// weight gradient of a 64 -> 64 layer: block (chunk, tap), lane = 4 ci x 4 co, TR_SUB pixels per LDS step.
// The tap-0 block also sums the bias gradient (lanes 0..63, pixel order).
__global__ __launch_bounds__(256) void train_conv64_wgrad_kernel(const float *__restrict__ in, const float *__restrict__ dout,
                                                                 int npix, int so, int chunk, float *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float As[TR_SUB * TR_NF];
    __shared__ __attribute__((aligned(16))) float Ds[TR_SUB * TR_NF];
    const int t = threadIdx.x, tc = t % 16, tp = t / 16;
    const int tap = blockIdx.y, ky = tap / 3, kx = tap % 3;
    const int si = so + 2;
    const int m0 = blockIdx.x * chunk, m1 = min(m0 + chunk, npix);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[i][c] = 0.0f;
    float bacc = 0.0f;

    for (int s0 = m0; s0 < m1; s0 += TR_SUB) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int p = tp + 16 * j, m = s0 + p;
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = a;
            if (m < m1) {
                const int n = m / (so * so), q = m % (so * so), y = q / so, x = q % so;
                a = *reinterpret_cast<const float4 *>(in + (((size_t)n * si + y + ky) * si + x + kx) * TR_NF + 4 * tc);
                d = *reinterpret_cast<const float4 *>(dout + (size_t)m * TR_NF + 4 * tc);
            }
            *reinterpret_cast<float4 *>(&As[p * TR_NF + 4 * tc]) = a;
            *reinterpret_cast<float4 *>(&Ds[p * TR_NF + 4 * tc]) = d;
        }
        __syncthreads();
#pragma unroll 8
        for (int p = 0; p < TR_SUB; p++) {
            const float4 a = *reinterpret_cast<const float4 *>(&As[p * TR_NF + 4 * tp]);
            const float4 d = *reinterpret_cast<const float4 *>(&Ds[p * TR_NF + 4 * tc]);
            const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                acc[i][0] = __builtin_fmaf(av[i], d.x, acc[i][0]);
                acc[i][1] = __builtin_fmaf(av[i], d.y, acc[i][1]);
                acc[i][2] = __builtin_fmaf(av[i], d.z, acc[i][2]);
                acc[i][3] = __builtin_fmaf(av[i], d.w, acc[i][3]);
            }
        }
        if (tap == 0 && t < TR_NF)
            for (int p = 0; p < TR_SUB; p++) bacc += Ds[p * TR_NF + t];
    }

    float *outp = partial + (size_t)blockIdx.x * (9 * TR_NF * TR_NF + TR_NF);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) outp[((size_t)tap * TR_NF + 4 * tp + i) * TR_NF + 4 * tc + c] = acc[i][c];
    if (tap == 0 && t < TR_NF) outp[9 * TR_NF * TR_NF + t] = bacc;
}

// grads[e] = sum over chunks, in chunk order, of partial[chunk][e]
__global__ __launch_bounds__(256) void train_reduce_kernel(const float *__restrict__ partial, int nchunks, int n,
                                                           float *__restrict__ grads)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float s = partial[e];
    for (int c = 1; c < nchunks; c++) s += partial[(size_t)c * n + e];
    grads[e] = s;
}

// ---------------------------------------------------------------------------------------------------------
// loss: one wave per triplet (lane = channel).  Butterfly sums: every lane holds the same, order-fixed total.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float l2norm_bwd(float g, float y, float r, float ss)
{
    const float yg = wave_sum(y * g);
    return ss >= 1e-12f ? r * (g - y * yg) : 1e6f * g;
}

__global__ __launch_bounds__(256) void train_loss_kernel(const float *__restrict__ z, int B, float margin,
                                                         float *__restrict__ y, float *__restrict__ ssq,
                                                         float *__restrict__ loss, float *__restrict__ dz)
{
    const int i = blockIdx.x * 4 + threadIdx.x / 64, c = threadIdx.x % 64;
    if (i >= B) return;
    float zz[3], yy[3], ss[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        zz[k] = z[((size_t)k * B + i) * TR_NF + c];
        ss[k] = wave_sum(zz[k] * zz[k]);
        r[k] = 1.0f / sqrtf(fmaxf(ss[k], 1e-12f));
        yy[k] = zz[k] * r[k];
        y[((size_t)k * B + i) * TR_NF + c] = yy[k];
        if (c == 0) ssq[k * B + i] = ss[k];
    }
    const float pos = wave_sum(yy[0] * yy[1]), neg = wave_sum(yy[0] * yy[2]);
    const float h = margin - (pos - neg);
    if (c == 0) loss[1 + i] = h;
    if (!dz) return;
    const float a = h > 0.0f ? 1.0f / (float)B : 0.0f;
    const float g[3] = {a * (yy[2] - yy[1]), -(a * yy[0]), a * yy[0]};
#pragma unroll
    for (int k = 0; k < 3; k++) dz[((size_t)k * B + i) * TR_NF + c] = l2norm_bwd(g[k], yy[k], r[k], ss[k]);
}

// loss[0] = (sum_i max(0, h_i)) / B: lane-strided partial sums in index order, then a fixed tree
__global__ __launch_bounds__(256) void train_loss_mean_kernel(float *__restrict__ loss, int B)
{
    __shared__ float red[256];
    float s = 0.0f;
    for (int i = threadIdx.x; i < B; i += 256) s += fmaxf(loss[1 + i], 0.0f);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0] / (float)B;
}

// TF's non-Nesterov momentum, one fp32 rounding per operation (the library is built without contraction)
__global__ __launch_bounds__(256) void train_momentum_kernel(float *__restrict__ p, float *__restrict__ v,
                                                             const float *__restrict__ g, int64_t n, float lr, float beta)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float bv = beta * v[i];
    const float nv = bv + g[i];
    const float step = lr * nv;
    v[i] = nv;
    p[i] = p[i] - step;
}

}  // namespace sde

using namespace sde;

SDE_EXPORT int64_t sde_train_param_floats(int nlayers, int nf)
{
    if (nf != TR_NF || nlayers < 1 || nlayers > TR_MAX_LAYERS) return -1;
    return tr_param_offset(nlayers, nf) + tr_w_floats(nlayers, nf) + nf;
}

SDE_EXPORT int64_t sde_train_workspace_bytes(int B, int nlayers, int nf)
{
    TrainLayout t;
    if (!train_layout(B, nlayers, nf, t)) return -1;
    return t.total * (int64_t)sizeof(float);
}

SDE_EXPORT int sde_train_gather(const float *img_l, const float *img_r, int H, int W, const int32_t *idx, int B,
                                int nlayers, float *patches, void *stream)
{
    TrainLayout t;
    if (!img_l || !img_r || !idx || !patches || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31) ||
        !train_layout(B, nlayers, TR_NF, t))
        return SDE_ERR_ARG;
    const int n = t.N * t.P * t.P;
    hipLaunchKernelGGL(train_gather_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), img_l, img_r, H, W,
                       idx, B, t.P, patches);
    return launch_status();
}

SDE_EXPORT int sde_train_loss_grad(const float *patches, int B, const float *params, int nlayers, int nf, float margin,
                                   float *loss, float *grads, void *ws, int64_t ws_bytes, void *stream)
{
    TrainLayout t;
    if (!patches || !params || !loss || !ws || !train_layout(B, nlayers, nf, t)) return SDE_ERR_ARG;
    // params and ws are read with 16-byte loads (patches, loss and grads by single floats only)
    if (((uintptr_t)params & 15) || ((uintptr_t)ws & 15)) return SDE_ERR_ARG;
    if (ws_bytes < t.total * (int64_t)sizeof(float)) return SDE_ERR_ARG;
    hipStream_t st = as_stream(stream);
    float *w = static_cast<float *>(ws);
    const int L = t.L, N = t.N;
    auto pix = [&](int k) { return N * t.side[k] * t.side[k]; };
    auto wk = [&](int k) { return params + tr_param_offset(k, nf); };
    auto bk = [&](int k) { return wk(k) + tr_w_floats(k, nf); };
    auto actk = [&](int k) { return k == L ? w + t.z : w + t.act[k]; };

    // forward
    hipLaunchKernelGGL(train_conv1_fwd_kernel, dim3(cdiv((int64_t)pix(1) * TR_NF, 256)), dim3(256), 0, st, patches,
                       wk(1), bk(1), actk(1), pix(1), t.P, (int)(L > 1));
    for (int k = 2; k <= L; k++)
        hipLaunchKernelGGL(train_conv64_kernel<false>, dim3(cdiv(pix(k), 64)), dim3(256), 0, st, actk(k - 1), wk(k),
                           bk(k), (const float *)nullptr, actk(k), pix(k), t.side[k], (int)(k < L));
    float *dz = grads ? w + t.dbuf[L & 1] : nullptr;
    hipLaunchKernelGGL(train_loss_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, w + t.z, B, margin, w + t.y, w + t.ss,
                       loss, dz);
    hipLaunchKernelGGL(train_loss_mean_kernel, dim3(1), dim3(256), 0, st, loss, B);
    if (!grads) return launch_status();

    // backward
    float *partial = w + t.partial;
    for (int k = L; k >= 1; k--) {
        const float *dout = w + t.dbuf[k & 1];
        const int nparam = (int)(tr_w_floats(k, nf) + nf);
        if (k == 1)
            hipLaunchKernelGGL(train_conv1_wgrad_kernel, dim3(t.nchunks[1]), dim3(256), 0, st, patches, dout, pix(1), t.P,
                               t.chunk[1], partial);
        else
            hipLaunchKernelGGL(train_conv64_wgrad_kernel, dim3(t.nchunks[k], 9), dim3(256), 0, st, actk(k - 1), dout,
                               pix(k), t.side[k], t.chunk[k], partial);
        hipLaunchKernelGGL(train_reduce_kernel, dim3(cdiv(nparam, 256)), dim3(256), 0, st, partial, t.nchunks[k], nparam,
                           grads + tr_param_offset(k, nf));
        if (k > 1)
            hipLaunchKernelGGL(train_conv64_kernel<true>, dim3(cdiv(pix(k - 1), 64)), dim3(256), 0, st, dout, wk(k),
                               (const float *)nullptr, actk(k - 1), w + t.dbuf[(k - 1) & 1], pix(k - 1), t.side[k - 1], 0);
    }
    return launch_status();
}

SDE_EXPORT int sde_train_export_activations(const void *ws, int B, int nlayers, int nf, int layer, float *out,
                                            void *stream)
{
    TrainLayout t;
    if (!ws || !out || !train_layout(B, nlayers, nf, t) || layer < 1 || layer > nlayers) return SDE_ERR_ARG;
    const float *w = static_cast<const float *>(ws);
    const float *src = layer == nlayers ? w + t.y : w + t.act[layer];
    const size_t n = (size_t)t.N * t.side[layer] * t.side[layer] * TR_NF;
    if (hipMemcpyAsync(out, src, n * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)) != hipSuccess)
        return SDE_ERR_LAUNCH;
    return SDE_OK;
}

SDE_EXPORT int sde_train_momentum(float *params, float *velocity, const float *grads, int64_t n, float lr, float beta,
                                  void *stream)
{
    if (!params || !velocity || !grads || n < 1 || n >= (1ll << 31) * 256) return SDE_ERR_ARG;
    hipLaunchKernelGGL(train_momentum_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), params, velocity,
                       grads, n, lr, beta);
    return launch_status();
}
