"""Write the phase-probe headers of the two 16x16x32 tower kernels: the PRODUCT tower_h16.h / tower_h16s.h with
per-phase s_memtime stamps injected by exact-text anchors, so the probes never drift from the product code (a
moved anchor is an assertion here, not a stale copy).  Every wave's lane 0 writes 4 floats to
out[32 blockIdx.x + 4 wave ..] at the end: MFMA waves (c-block loop, epilogue or hand-over write, barrier), stagers
(staging work, barrier, drain of the hand-over buffer).  Timing-only: wrong outputs in tile-0 rows.
  tools/_var/tower_h16_phase.h    conv64_h16_kernel (16 x 32 tiles):   -DSDE_H16_HEADER  on tower_h16.hip
  tools/_var/tower_h16s_phase.h   conv64_h16s_kernel (16 x 16 tiles):  -DSDE_H16S_HEADER on tower_h16s.hip
usage: python tools/variants/make_phase_header.py
       bash tools/build_file_variant.sh tower_h16s.hip phase_s -DSDE_H16S_HEADER='"'$PWD/tools/_var/tower_h16s_phase.h'"'
       bash tools/build_file_variant.sh tower_h16.hip phase -DSDE_H16_HEADER='"'$PWD/tools/_var/tower_h16_phase.h'"'
       python tools/tower_phase.py tools/_var/libsde_phase_s.so tools/_var/libsde_phase.so@t32"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "scenedepthestimation_amd", "csrc")
src = open(os.path.join(CSRC, "tower_h16.h")).read()
src_s = open(os.path.join(CSRC, "tower_h16s.h")).read()


def rep(s, old, new):
    assert old in s, old[:70]
    return s.replace(old, new, 1)


helpers = '''__device__ float *h16_probe_out;
__device__ __forceinline__ uint64_t h16_stamp()
{
    const uint64_t t = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    return t;
}
__device__ __forceinline__ void h16_stamp_out(float *out, int wave, int lane, const uint64_t (&ph)[4])
{
    if (lane == 0)
        for (int k = 0; k < 4; k++) out[32 * blockIdx.x + 4 * wave + k] = (float)ph[k];
}

'''
# ---- tower_h16.h: the stager loop both kernels share (h16_stager_loop; layer 3 is what the probe runs), and
# conv64_h16_kernel's MFMA waves
STAGE_STEP = '''        if (2 * i + 2 < nh) store(ra, 2 * i + 2);
        if (2 * i + 4 < nh) load(ra, 2 * i + 4);
        if (2 * i + 3 < nh) store(rb, 2 * i + 3);
        if (2 * i + 5 < nh) load(rb, 2 * i + 5);
'''
s = rep(src, "namespace sde {\n", "namespace sde {\n" + helpers)
s = rep(s, '''#pragma unroll 1
    for (int i = 0; i < nsteps; i++) {
''' + STAGE_STEP + '''        if (T::HANDOFF && i >= 2 && !(i & 1)) drain(tile0 + ((i - 2) >> 1) * gstride);
        __syncthreads();
    }
    if (T::HANDOFF) drain(tile0 + ((nsteps - 2) >> 1) * gstride);
}''', '''    uint64_t ph[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int i = 0; i < nsteps; i++) {
        const uint64_t t0 = h16_stamp();
''' + STAGE_STEP + '''        const uint64_t t1 = h16_stamp();
        if (T::HANDOFF && i >= 2 && !(i & 1)) drain(tile0 + ((i - 2) >> 1) * gstride);
        const uint64_t t2 = h16_stamp();
        __syncthreads();
        const uint64_t t3 = h16_stamp();
        ph[0] += t1 - t0;
        ph[1] += t3 - t2;
        ph[2] += t2 - t1;
    }
    const uint64_t t4 = h16_stamp();
    if (T::HANDOFF) drain(tile0 + ((nsteps - 2) >> 1) * gstride);
    ph[2] += h16_stamp() - t4;
    h16_stamp_out(h16_probe_out, (st >> 6) + 4, st & 63, ph);
}''')
s = rep(s, '''    if (wave >= 4) {
        auto nodrain = [](int) {};''', '''    h16_probe_out = out;
    if (wave >= 4) {
        auto nodrain = [](int) {};''')
s = rep(s, '''        auto cstep = [&](int cb) {
''', '''        auto cstep = [&](int cb) {
            const uint64_t ta = h16_stamp();
''')
s = rep(s, '''            if (cb == H16_NCB - 1) {
                if (img != sc_img) {''', '''            const uint64_t tb = h16_stamp();
            if (cb == H16_NCB - 1) {
                if (img != sc_img) {''')
s = rep(s, '''            __syncthreads();
            cur ^= 1;
        };''', '''            const uint64_t tc = h16_stamp();
            __syncthreads();
            const uint64_t td = h16_stamp();
            pht[0] += tb - ta;
            pht[1] += tc - tb;
            pht[2] += td - tc;
            cur ^= 1;
        };''')
s = rep(s, '''    int sc_img = -1;
    float sc_u = 1.0f, sc_o = 1.0f;''', '''    uint64_t pht[4] = {0, 0, 0, 0};
    int sc_img = -1;
    float sc_u = 1.0f, sc_o = 1.0f;''')
s = rep(s, '''    if (!LAST) xp_flush_amax(amax_run, amax_img, lane, out_amax, bt.amax_stride);
}''', '''    if (!LAST) xp_flush_amax(amax_run, amax_img, lane, out_amax, bt.amax_stride);
    h16_stamp_out(out, g, lane, pht);
}''')
os.makedirs(os.path.join(ROOT, "tools", "_var"), exist_ok=True)
open(os.path.join(ROOT, "tools", "_var", "tower_h16_phase.h"), "w").write(s)
print("wrote tools/_var/tower_h16_phase.h")
# variant: the stagers skip their loads and splits (barriers only) -- how much of the MFMA waves' loop excess is
# the stagers' issue on the shared SIMDs
s2 = rep(s, "        const uint64_t t0 = h16_stamp();\n" + STAGE_STEP, "        const uint64_t t0 = h16_stamp();\n")
open(os.path.join(ROOT, "tools", "_var", "tower_h16_phase_nostage.h"), "w").write(s2)
print("wrote tools/_var/tower_h16_phase_nostage.h")

# ---- tower_h16s.h: conv64_h16s_kernel's MFMA waves, behind the stamped tower_h16.h (whose named guard empties
# tower_h16s.h's include of the product header)
t = rep(src_s, '''    if (wave >= 4) {
        // stager lane 4 j + k4''', '''    h16_probe_out = out;
    if (wave >= 4) {
        // stager lane 4 j + k4''')
t = rep(t, '''    int cur = 0;
    for (; tile < bt.ntiles; tile += gridDim.x) {
        h16s_cblock<T>(acc, abuf, ra, avoff, cbo0, cbo1, hsm + cur * T::STAGE + bbase);
        __syncthreads();
        cur ^= 1;
        h16s_cblock<T>(acc, abuf, ra, avoff, cbo1, cbo0, hsm + cur * T::STAGE + bbase);
''', '''    int cur = 0;
    uint64_t pht[4] = {0, 0, 0, 0};
    for (; tile < bt.ntiles; tile += gridDim.x) {
        const uint64_t ta = h16_stamp();
        h16s_cblock<T>(acc, abuf, ra, avoff, cbo0, cbo1, hsm + cur * T::STAGE + bbase);
        const uint64_t tb = h16_stamp();
        __syncthreads();
        const uint64_t tc = h16_stamp();
        cur ^= 1;
        h16s_cblock<T>(acc, abuf, ra, avoff, cbo1, cbo0, hsm + cur * T::STAGE + bbase);
        const uint64_t td = h16_stamp();
''')
t = rep(t, '''        for (int i = 0; i < 16; i++) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        cur ^= 1;
    }
''', '''        for (int i = 0; i < 16; i++) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        const uint64_t te = h16_stamp();
        __syncthreads();
        pht[0] += (tb - ta) + (td - tc);
        pht[1] += te - td;
        pht[2] += (tc - tb) + (h16_stamp() - te);
        cur ^= 1;
    }
    h16_stamp_out(out, g, lane, pht);
''')
open(os.path.join(ROOT, "tools", "_var", "tower_h16s_phase.h"), "w").write(s + t)
print("wrote tools/_var/tower_h16s_phase.h")
