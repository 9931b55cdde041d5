// cv_tile.h -- the pre-split tile path of the certified fused cost volume + WTA (sde_feature_split and
// sde_cv_wta_split, cv_wta.hip).  The certificate and FX_K are cv_cert.h's, the winner's exact cost cv_exact.h's.
//
// Mapping: workgroup = 4 waves on one row and 64 left pixels (2 N-tiles of 32);
// the right-feature window of a <=128-disparity chunk (<= 6 M-tiles of 32
// pixels) arrives pre-split as hi/lo bf16 planes (written by the tower's last
// epilogue or feature_split_kernel) and is staged into LDS by LDS-DMA
// (global_load_lds, swizzle applied to the source address); wave w owns N-tile
// w&1 and every other M-tile; the left operand lives in registers (hi/lo).
// Blocks are remapped so all blocks of a row run on one XCD (its L2 serves the
// overlapping windows).
#pragma once

#include "cv_cert.h"
#include "cv_exact.h"

namespace sde {

constexpr int FX_DCH = 128;        // disparities per window chunk
constexpr int FX_NT = 6;           // max M-tiles per chunk: ceil((128 + 63) / 32)
constexpr int FX_WIN = FX_NT * 32; // window pixels

__device__ __forceinline__ void fx_split(float x, __bf16 &h, __bf16 &l)
{
    h = (__bf16)x;
    l = (__bf16)(x - (float)h);
}

// Split of a feature map for the certified path: x = hi + lo + r with hi =
// bf16_rne(x), lo = bf16_rne(x - hi) (|r| <= 2^-16 |x|), plus an upper bound of
// each pixel's L2 norm (fp32 sum of 64 squares, relative error <= 64*2^-24,
// inflated by (1 + 4e-6)).  16 lanes per pixel, one float4 each.
__global__ __launch_bounds__(256) void feature_split_kernel(const float *__restrict__ f, int64_t npix,
                                                            uint16_t *__restrict__ hi, uint16_t *__restrict__ lo,
                                                            float *__restrict__ nrm)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = idx < npix * 16;
    const float4 v = ok ? reinterpret_cast<const float4 *>(f)[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    float ss = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    ss += __shfl_xor(ss, 4, 64);
    ss += __shfl_xor(ss, 8, 64);
    if (!ok) return;
    __bf16 h0, h1, h2, h3, l0, l1, l2, l3;
    fx_split(v.x, h0, l0); fx_split(v.y, h1, l1); fx_split(v.z, h2, l2); fx_split(v.w, h3, l3);
    typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
    const bf4 hv = {h0, h1, h2, h3}, lv = {l0, l1, l2, l3};
    reinterpret_cast<uint2 *>(hi)[idx] = __builtin_bit_cast(uint2, hv);
    reinterpret_cast<uint2 *>(lo)[idx] = __builtin_bit_cast(uint2, lv);
    if ((idx & 15) == 0) nrm[idx >> 4] = sqrtf(ss) * FX_NORM_UP;
}

// Certified fast kernel on pre-split operands.  One workgroup per (row,
// 64-pixel strip), <= 128-disparity chunks (window <= 6 M-tiles = 192 pixels,
// 48 KB of hi/lo planes in LDS -> 3 workgroups per CU).  The window is staged
// by LDS-DMA (global_load_lds_dwordx4: no VGPRs, no VALU): each wave-instruction
// fills 1 KB of the swizzled image linearly, so the swizzle is applied to the
// per-lane SOURCE chunk.  Invalid voxels (x - d < 0: exact cost -0.0) are
// forced to score +0 in the edge-tile path.
__global__ __launch_bounds__(256) void cv_wta_cert_kernel(const float *__restrict__ fl, const float *__restrict__ fr,
                                                          const uint4 *__restrict__ lhi, const uint4 *__restrict__ llo,
                                                          const float *__restrict__ lnrm,
                                                          const uint4 *__restrict__ rhi, const uint4 *__restrict__ rlo,
                                                          const float *__restrict__ rnrm, int H, int W, int d0, int d1,
                                                          float *__restrict__ out_min, int32_t *__restrict__ out_arg,
                                                          float *__restrict__ out_disp, unsigned *__restrict__ counter,
                                                          int32_t *__restrict__ list)
{
    __shared__ uint4 pl[2 * FX_WIN * 8];            // [plane][pixel][8 chunks], swizzled
    __shared__ float mb[4][64];
    __shared__ int ma[4][64];
    __shared__ float ms[4][64];
    __shared__ unsigned nmax_bits;

    const int nbx = (W + FX_NX - 1) / FX_NX;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int y = lb / nbx;
    const int x0 = (lb % nbx) * FX_NX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = wave & 1, mpar = wave >> 1;
    const int j = lane & 31, h = lane >> 5;
    const int x = x0 + 32 * n + j;
    const bool xok = x < W;
    const size_t rowpix = (size_t)y * W;
    if (tid == 0) nmax_bits = 0u;

    // left operand: 16-B chunks 2s+h of this lane's pixel (channels 16s+8h..+7)
    fx_bf16x8 bh[4], bl[4];
    {
        const size_t pc = (rowpix + (xok ? x : 0)) * 8;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            bh[s] = __builtin_bit_cast(fx_bf16x8, lhi[pc + 2 * s + h]);
            bl[s] = __builtin_bit_cast(fx_bf16x8, llo[pc + 2 * s + h]);
        }
    }
    const float nl = lnrm[rowpix + (xok ? x : 0)];

    float b1[4], b2[4];
    int ag[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { b1[t] = -__builtin_inff(); b2[t] = -__builtin_inff(); ag[t] = -1; }

    for (int dc0 = d0; dc0 < d1; dc0 += FX_DCH) {
        const int dc1 = min(dc0 + FX_DCH, d1);
        const int nt = (dc1 - dc0 + 63 + 31) / 32;
        const int rb = x0 + FX_NX - dc0 - 32 * nt;     // right pixel of window row 0
        __syncthreads();                               // previous chunk's plane reads are done
        // LDS-DMA: 2 planes x nt*32 pixels x 8 chunks = nt*8 KB; 1 KB (8 pixels) per wave-instruction
        const int ninst = nt * 4 * 2;                  // per plane nt*4 instructions
        for (int ii = wave; ii < ninst; ii += 4) {
            const int plane = ii / (nt * 4);
            const int slot = (ii - plane * nt * 4) * 64 + lane;   // 16-B slot within the plane image
            const int r = slot >> 3, cs = slot & 7;
            const int c8 = cs ^ ((r >> 1) & 7);                  // source chunk for this LDS slot
            const int xr = min(max(rb + r, 0), W - 1);
            const uint4 *src = (plane ? rlo : rhi) + (rowpix + xr) * 8 + c8;
            __builtin_amdgcn_global_load_lds((const void *)src,
                                             (__attribute__((address_space(3))) void *)(pl + plane * FX_WIN * 8 +
                                                                                        (ii - plane * nt * 4) * 64),
                                             16, 0, 0);
        }
        // window norm bound: max over its pixels
        {
            float nm = 0.0f;
            for (int r = tid; r < nt * 32; r += 256) {
                const int xr = rb + r;
                if (xr >= 0 && xr < W) nm = fmaxf(nm, rnrm[rowpix + xr]);
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) nm = fmaxf(nm, __shfl_xor(nm, o, 64));
            if (lane == 0) atomicMax(&nmax_bits, __float_as_uint(nm));   // non-negative: uint order
        }
        __syncthreads();                               // drains the DMA (vmcnt(0)) and publishes it

        const int xbase = x0 + 32 * n;
        for (int m = mpar; m < nt; m += 2) {
            const int dt = xbase - (rb + 32 * m);
            const int dlo = dt - 31, dhi = dt + 31;
            if (dhi < dc0 || dlo >= dc1) continue;     // wave-uniform
            fx_floatx16 acc = {0};
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int sl = fx_slot(32 * m + j, 2 * s + h);
                const fx_bf16x8 ah = __builtin_bit_cast(fx_bf16x8, pl[sl]);
                const fx_bf16x8 al = __builtin_bit_cast(fx_bf16x8, pl[FX_WIN * 8 + sl]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[s], acc, 0, 0, 0);
            }
            const int dl = dt + j - 4 * h;             // d of register r is dl - ((r&3) + 8(r>>2))
            const int xrl = rb + 32 * m + 4 * h;       // right pixel of register r is xrl + ((r&3) + 8(r>>2))
            if (dlo >= dc0 && dhi < dc1 && rb + 32 * m >= 0) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int t = r & 3;
                    const int d = dl - ((r & 3) + 8 * (r >> 2));
                    const float sc = acc[r];
                    const bool gt = sc > b1[t];
                    ag[t] = gt ? d : ag[t];
                    b2[t] = __builtin_amdgcn_fmed3f(b1[t], b2[t], sc);
                    b1[t] = fmaxf(b1[t], sc);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int t = r & 3;
                    const int ri = (r & 3) + 8 * (r >> 2);
                    const int d = dl - ri;
                    float sc = (xrl + ri < 0) ? 0.0f : acc[r];          // x < d: exact cost -0.0
                    sc = (d >= dc0 && d < dc1) ? sc : -__builtin_inff();
                    const bool gt = sc > b1[t];
                    ag[t] = gt ? d : ag[t];
                    b2[t] = __builtin_amdgcn_fmed3f(b1[t], b2[t], sc);
                    b1[t] = fmaxf(b1[t], sc);
                }
            }
        }
    }

    float best = b1[0], second = b2[0];
    int arg = ag[0];
#pragma unroll
    for (int t = 1; t < 4; t++) fx_merge(best, arg, second, b1[t], ag[t], b2[t]);
    {
        const float bb = __shfl_xor(best, 32, 64), ss = __shfl_xor(second, 32, 64);
        const int aa = __shfl_xor(arg, 32, 64);
        fx_merge(best, arg, second, bb, aa, ss);
    }
    mb[wave][lane] = best;
    ma[wave][lane] = arg;
    ms[wave][lane] = second;
    __syncthreads();
    if (wave < 2 && h == 0 && xok) {
        fx_merge(best, arg, second, mb[wave + 2][lane], ma[wave + 2][lane], ms[wave + 2][lane]);
        const float eps = FX_K * nl * __uint_as_float(nmax_bits) + FX_ABS;
        const size_t p = rowpix + x;
        if ((best - second) > 2.0f * eps && arg >= 0) {
            if (out_min) {
                float cost = -0.0f;
                if (x - arg >= 0)   // exact cost of the winner: NumPy pairwise order, as cv64_kernel
                    cost = dot64_exact_global(reinterpret_cast<const float4 *>(fl + p * 64),
                                              reinterpret_cast<const float4 *>(fr + (p - arg) * 64));
                out_min[p] = cost;
            }
            if (out_arg) out_arg[p] = arg;
            if (out_disp) out_disp[p] = (float)arg;
        } else {
            const unsigned e = atomicAdd(counter, 1u);
            list[e] = (int32_t)p;
        }
    }
}

}  // namespace sde
