// speckle.hip -- speckle removal by connected-component labelling (gfx950): sdf_speckle.
//
// The definition is stated in include/sde_filter.h.  The result is a function of the partition of the image into
// regions alone, so any order of discovery gives the same bytes; sizes are integer counts added with integer
// atomics.  Four launches (three when the image is one tile), none of which has a workgroup wait for another:
//
//   1 speckle_tile_kernel   a 64 x 16 tile in LDS: union-find over the links inside the tile, then
//                           labels[p] = global index of p's tile-local root (-1 for an invalid pixel) and
//                           counts[p] = size of the tile-local component if p is its root, else 0.
//   2 speckle_seam_kernel   one thread per pixel pair across a tile seam: lock-free union of the two roots, unless
//                           the previous pair of the seam and launch 1 have made the link already.
//   3 speckle_flatten_kernel every tile-local root that is not a global root finds its global root, adds its
//                           count to that root's and points itself at it.
//   4 speckle_apply_kernel  root = labels[labels[p]], n = counts[root]; out, mask, sizes.
//
// Labels only ever decrease and a pixel's label is the index of a pixel of its own region that is not above its
// own, so every chain of labels ends, at the least index of what has been joined so far, and `find` terminates
// whatever other threads do meanwhile.  A union retries only when its own atomicMin met a word that another
// union had lowered in between; the words are bounded below, so the retries are too.
//
// Visibility: in launches 2 and 3 a word of `labels` (and in 3 a global root's word of `counts`) may be written
// by another workgroup of the same launch; those words are read and written with agent-scope atomics only.
// Plain loads read what an earlier launch finished.
#include "sde_common.h"
#include "sde_filter.h"

namespace sde {

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));   // dword-aligned: rows of an odd W
typedef int int4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int TW = 64, TH = 16, TPIX = TW * TH;   // the tile of launch 1: 256 threads of four pixels in a row

__device__ __forceinline__ bool speckle_valid(float v)
{
    return (__float_as_uint(v) & 0x7fffffffu) < 0x7f800000u && v >= 0.0f;   // finite, and -0.0f >= 0
}

__device__ __forceinline__ bool speckle_link(float a, float b, float max_diff)
{
    return speckle_valid(a) && speckle_valid(b) && fabsf(a - b) <= max_diff;
}

// ---- the tile-local forest, in LDS (workgroup scope) ----
__device__ __forceinline__ int lds_find(int *L, int a)
{
    for (;;) {
        const int p = __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == a) return a;
        a = p;
    }
}

__device__ __forceinline__ void lds_union(int *L, int a, int b)
{
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == b) return;   // b was still a root: joined
        b = old;                // another union lowered it first: join a with where it pointed
    }
}

// ---- the global forest (agent scope) ----
__device__ __forceinline__ int agent_load(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int agent_find(const int *L, int a)
{
    for (;;) {
        const int p = agent_load(L + a);
        if (p == a) return a;
        a = p;
    }
}

__device__ __forceinline__ void agent_union(int *L, int a, int b)
{
    for (;;) {
        a = agent_find(L, a);
        b = agent_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == b) return;
        b = old;
    }
}

__global__ __launch_bounds__(256) void speckle_tile_kernel(const float *__restrict__ disp, int H, int W, int ntx,
                                                           float max_diff, int *__restrict__ labels,
                                                           int *__restrict__ counts)
{
    __shared__ float val[TPIX];
    __shared__ int lab[TPIX];
    __shared__ int cnt[TPIX];
    const int t = threadIdx.x, r = t >> 4, c = (t & 15) * 4, i = r * TW + c;
    const int x0 = (int)(blockIdx.x % (unsigned)ntx) * TW, y0 = (int)(blockIdx.x / (unsigned)ntx) * TH;
    const int gy = y0 + r, gx = x0 + c;
    const bool row_in = gy < H, all_in = row_in && gx + 3 < W;
    const size_t g = (size_t)gy * W + gx;   // formed for every thread, used only where the pixel is in the image

    // a pixel outside the image is a NaN: invalid, so it links to nothing
    float v[4];
    if (all_in) {
        const float4u q = *reinterpret_cast<const float4u *>(disp + g);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = row_in && gx + k < W ? disp[g + k] : __uint_as_float(0x7fc00000u);
    }
    // links to the right inside the thread's four pixels: a run starts with its first pixel's label
    bool right[4];
    int l = i;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        right[k] = k < 3 && speckle_link(v[k], v[k + 1], max_diff);
        if (k > 0 && !right[k - 1]) l = i + k;
        val[i + k] = v[k];
        lab[i + k] = l;
        cnt[i + k] = 0;
    }
    __syncthreads();

    if (c + 4 < TW && speckle_link(v[3], val[i + 4], max_diff)) lds_union(lab, i + 3, i + 4);
    if (r + 1 < TH) {
        float b[4];
        bool down[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            b[k] = val[i + TW + k];
            down[k] = speckle_link(v[k], b[k], max_diff);
            // the square k-1, k over the two rows is closed by its other three sides: this link adds nothing
            const bool closed = k > 0 && right[k - 1] && down[k - 1] && speckle_link(b[k - 1], b[k], max_diff);
            if (down[k] && !closed) lds_union(lab, i + k, i + TW + k);
        }
    }
    __syncthreads();

    // roots, and one LDS add per run of equal roots among the four pixels
    int root[4];
#pragma unroll
    for (int k = 0; k < 4; k++) root[k] = speckle_valid(v[k]) ? lds_find(lab, i + k) : -1;
    int run = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (root[k] >= 0) run++;
        if (run > 0 && (k == 3 || root[k + 1] != root[k])) {
            atomicAdd(&cnt[root[k]], run);
            run = 0;
        }
    }
    __syncthreads();

    int gl[4], gc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        gl[k] = root[k] < 0 ? -1 : (int)((size_t)(y0 + root[k] / TW) * W + (x0 + root[k] % TW));
        gc[k] = root[k] == i + k ? cnt[i + k] : 0;
    }
    if (all_in) {
        int4u a, n;
        a.x = gl[0]; a.y = gl[1]; a.z = gl[2]; a.w = gl[3];
        n.x = gc[0]; n.y = gc[1]; n.z = gc[2]; n.w = gc[3];
        *reinterpret_cast<int4u *>(labels + g) = a;
        *reinterpret_cast<int4u *>(counts + g) = n;
    } else if (row_in) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (gx + k < W) {
                labels[g + k] = gl[k];
                counts[g + k] = gc[k];
            }
    }
}

// Seam pair s: the first nh are the pairs (y - 1, x), (y, x) over the horizontal seams y = TH, 2 TH, ..., the
// rest the pairs (y, x - 1), (y, x) over the vertical seams x = TW, 2 TW, ...
__global__ __launch_bounds__(256) void speckle_seam_kernel(const float *__restrict__ disp, int H, int W,
                                                           int64_t nh, int64_t nseam, float max_diff, int *labels)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseam) return;
    // `back` steps to the previous pair of the same seam where that pair lies between the same two tiles
    size_t a, b, back;
    if (s < nh) {
        const int64_t y = (s / W + 1) * TH, x = s % W;
        b = (size_t)y * W + x;
        a = b - W;
        back = x % TW != 0 ? 1 : 0;
    } else {
        const int64_t u = s - nh, x = (u / H + 1) * TW, y = u % H;
        b = (size_t)y * W + x;
        a = b - 1;
        back = y % TH != 0 ? (size_t)W : 0;
    }
    const float da = disp[a], db = disp[b], pa = disp[a - back], pb = disp[b - back];
    if (!speckle_link(da, db, max_diff)) return;
    // The square of this pair and the previous one is closed by its other three sides: the previous pair's link,
    // made by its own thread or closed in its turn (the first pair between two tiles always unions), and two links
    // inside the tiles, which launch 1 made.  A constant map then costs one union per tile seam, not one per pixel.
    if (back != 0 && speckle_link(pa, pb, max_diff) && speckle_link(pa, da, max_diff) && speckle_link(pb, db, max_diff))
        return;
    agent_union(labels, (int)a, (int)b);
}

__global__ __launch_bounds__(256) void speckle_flatten_kernel(int64_t npix, int *labels, int *counts)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int l = agent_load(labels + p);
    if (l < 0 || l == p) return;   // invalid, or a global root: others add to its count, it reads nothing
    // not a global root, so nobody adds to this word in this launch
    const int n = counts[p];
    if (n == 0) return;            // not a tile-local root: its label is one, and stays
    const int root = agent_find(labels, l);
    atomicAdd(counts + root, n);
    __hip_atomic_store(labels + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// disp and out may be the same array: a thread reads only the pixel it writes.
__global__ __launch_bounds__(256) void speckle_apply_kernel(const float *disp, int64_t npix, int max_size, float fill,
                                                            const int *__restrict__ labels,
                                                            const int *__restrict__ counts, float *out,
                                                            uint8_t *__restrict__ mask, int32_t *__restrict__ sizes)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float d = disp[p];
    const int l = labels[p];
    int n = 0;
    if (l >= 0) n = counts[labels[l]];   // pixel -> tile-local root -> global root (a root points at itself)
    const bool gone = l >= 0 && n <= max_size;
    out[p] = gone ? fill : d;
    if (mask) mask[p] = gone ? 1 : 0;
    if (sizes) sizes[p] = n;
}

static inline bool speckle_bad_shape(int H, int W) { return H < 1 || W < 1 || (int64_t)H * W > 2147483647ll; }

}  // namespace sde

using namespace sde;

SDE_EXPORT int64_t sdf_speckle_workspace_bytes(int H, int W)
{
    if (speckle_bad_shape(H, W)) return 0;
    return (int64_t)H * W * 8;   // labels int32 [H][W], counts int32 [H][W]
}

SDE_EXPORT int sdf_speckle(const float *disp, int H, int W, int max_size, float max_diff, float fill, float *out,
                           uint8_t *mask, int32_t *sizes, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!disp || !out || !workspace || speckle_bad_shape(H, W) || max_size < 0) return SDE_ERR_ARG;
    if (!(max_diff >= 0.0f) || max_diff > 3.402823466e38f) return SDE_ERR_ARG;   // negative, NaN, infinite
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return SDE_ERR_ARG;
    if (workspace_bytes < sdf_speckle_workspace_bytes(H, W)) return SDE_ERR_WORKSPACE;
    const int64_t npix = (int64_t)H * W;
    int *labels = static_cast<int *>(workspace), *counts = labels + npix;
    hipStream_t st = as_stream(stream);
    const int ntx = cdiv(W, TW), nty = cdiv(H, TH);
    speckle_tile_kernel<<<(unsigned)((int64_t)ntx * nty), 256, 0, st>>>(disp, H, W, ntx, max_diff, labels, counts);
    const int64_t nh = (int64_t)(nty - 1) * W, nseam = nh + (int64_t)(ntx - 1) * H;
    if (nseam > 0)
        speckle_seam_kernel<<<cdiv(nseam, 256), 256, 0, st>>>(disp, H, W, nh, nseam, max_diff, labels);
    speckle_flatten_kernel<<<cdiv(npix, 256), 256, 0, st>>>(npix, labels, counts);
    speckle_apply_kernel<<<cdiv(npix, 256), 256, 0, st>>>(disp, npix, max_size, fill, labels, counts, out, mask,
                                                           sizes);
    return launch_status();
}
