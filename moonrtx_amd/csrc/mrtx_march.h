// mrtx_march.h -- the march core of libmoonrt.so's gfx950 kernels, shared by the translation units that march rays through the
// height field: mrtx_kernels.hip (camera and path stage) and mrtx_terrain.hip (terrain queries).
//
// Device-side only, every function __forceinline__: the correctly rounded math, the DEM fetch (dem_march), a march's segments
// with their skip intervals (seg_setup .. march_segment, march), the bisection (refine), the hit vertex and the light sample.
// The rule: this header holds the march core and what BOTH translation units use; what one of them alone uses stays in that
// file, and so does every __device__ variable (a header would give each translation unit a copy of its own).
//
// Arithmetic follows the spec of DESIGN.md section 3 operation by operation: explicit fmaf, build with -ffp-contract=off,
// correctly rounded / and sqrt (hipcc default), own polynomial atan/sin/cos.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_device.h"

// The cold constants are read-only for the whole launch: address them through the constant address space so the
// (wave-uniform) reads become scalar loads (s_load_*) instead of per-lane vector loads.
#define CF(f) ((const __attribute__((address_space(4))) FrameCold*)(f).cold)

#ifndef MRTX_TRIAL_BATCH
#define MRTX_TRIAL_BATCH 1     // steps fetched together in the trial segment.  Round 4 (8 waves per SIMD, VALU issue 0.65): 1 step
#endif                         // 16.20 ms against 16.34 with 2 -- the 64 continuation rays are incoherent, a speculated second step is
                               // mostly thrown away; the coherent marches keep MRTX_STEP_BATCH = 2 (1: 16.64 ms, 3: 16.68)

namespace mrtx {

__device__ constexpr float kPi = 3.14159274101257324f;
__device__ constexpr float kHalfPi = 1.57079637050628662f;
__device__ constexpr float kInv255 = 0.003921568859368563f;

// -DMRTX_PROF (tools/build_variant.sh prof -DMRTX_PROF): s_memtime section timers, summed per wave into g_prof
// (mrtx_kernels.hip, with the launch code that reads it back).
// A measurement build only; the shipped library never defines it.
#ifdef MRTX_PROF
#ifdef MRTX_PROF_FULLIV       // this measurement build uses the timers' slots for its own counts
#define PROF_BEGIN(i)
#define PROF_END(i)
#else
#define PROF_BEGIN(i) const unsigned long long _pt##i = __builtin_readcyclecounter()
#define PROF_END(i) cnt[i] += (uint32_t)(__builtin_readcyclecounter() - _pt##i)
#endif
#else
#define PROF_BEGIN(i)
#define PROF_END(i)
#endif

enum { ST_PRIMARY = 0, ST_HITS, ST_SHADOW, ST_HEIGHT, ST_COLOUR, ST_BG, ST_FETCH, ST_MIP, ST_BOUNCE, ST_SUNHIT, ST_N };

// atan(q) ~= q * P(q^2) on [0,1], |err| <= 1.3e-7
__device__ __forceinline__ float atan_poly(float q) {
    const float s = q * q;
    float p = -0.004054343327879906f;
    p = fmaf(p, s, 0.02186218835413456f);
    p = fmaf(p, s, -0.05591127648949623f);
    p = fmaf(p, s, 0.0964212492108345f);
    p = fmaf(p, s, -0.1390860229730606f);
    p = fmaf(p, s, 0.19946560263633728f);
    p = fmaf(p, s, -0.33329859375953674f);
    p = fmaf(p, s, 0.9999993443489075f);
    return p * q;
}

// Correctly rounded sqrt for x in [2^-96, 2^96]: the raw v_sqrt_f32 (<= 1 ulp) plus the +-1 ulp residual
// test LLVM uses, without the denormal pre-scaling and class checks the general expansion carries
// (callers clamp x into the domain; tests compare against the host's IEEE sqrtf bit for bit).
__device__ __forceinline__ float sqrt_cr(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = __uint_as_float(__float_as_uint(s) - 1u);
    const float s_up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_dn = fmaf(-s_dn, s, x);
    const float r_up = fmaf(-s_up, s, x);
    s = r_dn <= 0.0f ? s_dn : s;
    s = r_up > 0.0f ? s_up : s;
    return s;
}

// Correctly rounded 1/x for every NORMAL x whose reciprocal is normal (|x| in [2^-126, 2^126)): v_rcp_f32 (<= 1 ulp) + one Newton
// step with an exact fma residual -- 3 VALU instead of the 10 of the general division expansion (v_div_scale x 2, v_rcp, four fmas,
// v_div_fmas, v_div_fixup), which exists to survive operands and quotients at the ends of the exponent range.  Equality with the
// IEEE quotient 1.0f / x is not argued, it is CHECKED: mrtx_probe_cr() compares the two on the device for EVERY normal float of
// either sign (2^32 bit patterns, under a second; profiles/r04_probe_cr.txt): 0 mismatches for exponents -126 .. 125, all of them
// where 1/x is subnormal or x = 0 (tests/test_gpu_parity.py::test_domain_restricted_reciprocal_and_sqrt_are_ieee_exact).
// sqrt_cr() likewise: 0 mismatches for x = 0 and exponents -104 .. 127.  Callers keep their arguments inside these domains (each
// call site says why); the oracle uses the C compiler's IEEE division and sqrtf throughout.
#ifndef MRTX_RCP_STEPS
#define MRTX_RCP_STEPS 1      // measured exhaustively: ONE step is already exact wherever x and 1/x are normal (profiles/r04_probe_cr.txt)
#endif
#ifndef MRTX_FAST_CR
#define MRTX_FAST_CR 1      // 0 = the compiler's IEEE expansions everywhere (A/B switch; the results are the same bits)
#endif
template <int STEPS = 2>
__device__ __forceinline__ float rcp_nr(float x) {
    float y = __builtin_amdgcn_rcpf(x);
#pragma unroll
    for (int i = 0; i < STEPS; i++) { const float e = fmaf(-x, y, 1.0f); y = fmaf(e, y, y); }
    return y;
}
__device__ __forceinline__ float rcp_cr(float x) {
#if MRTX_FAST_CR
    return rcp_nr<MRTX_RCP_STEPS>(x);
#else
    return 1.0f / x;
#endif
}
// sqrt for the shading code: sqrt_cr where the argument is inside its domain (or exactly zero, which it returns as zero)
__device__ __forceinline__ float sqrt_sh(float x) {
#if MRTX_FAST_CR
    return sqrt_cr(x);
#else
    return sqrtf(x);
#endif
}

// (a, b, c) -> lat = atan2(c, rho), lon = atan2(a, b), rho = sqrt(max(a^2+b^2, 1e-28)).  The two min/max
// ratios share ONE correctly rounded reciprocal (a v_div_scale/v_rcp/fma/v_div_fixup chain is ~12 VALU);
// min/max instead of compare+select keeps VCC hazards (s_nop) out of the loop.
__device__ __forceinline__ void latlon(float a, float b, float c, float rho2, float& lat, float& lon) {
    const float rho = sqrt_cr(fmaxf(rho2, 1.0e-28f));
    const float aa = fabsf(a), ab = fabsf(b), ac = fabsf(c);
    const float m1 = fmaxf(rho, ac), n1 = fminf(rho, ac);
    const float m2 = fmaxf(ab, aa), n2 = fminf(ab, aa);
    const float den = fmaxf(m1 * m2, 1.0e-37f);
    const float t = rcp_cr(den);            // den in [1e-37, ~1e7]: normal, reciprocal normal
    float r1 = atan_poly(n1 * (t * m2));
    float r2 = atan_poly(n2 * (t * m1));
    r1 = ac >= rho ? kHalfPi - r1 : r1;
    r2 = aa >= ab ? kHalfPi - r2 : r2;
    r2 = b < 0.0f ? kPi - r2 : r2;
    lat = copysignf(r1, c);
    lon = copysignf(r2, a);
}

// cos / sin of 2*pi*u, u in [0,1): quadrant split + polynomials on [0, pi/2)
__device__ __forceinline__ void sincos_turn(float u, float& cs, float& sn) {
    const float t4 = u * 4.0f;
    const float qf = floorf(t4);
    const float a = (t4 - qf) * kHalfPi;
    const float a2 = a * a;
    float sp = 2.590481244624243e-06f;
    sp = fmaf(sp, a2, -0.00019800894369836897f);
    sp = fmaf(sp, a2, 0.008332899771630764f);
    sp = fmaf(sp, a2, -0.16666647791862488f);
    sp = fmaf(sp, a2, 1.0f);
    const float s1 = sp * a;
    float cp = 2.3153859729063697e-05f;
    cp = fmaf(cp, a2, -0.001385370153002441f);
    cp = fmaf(cp, a2, 0.04166358336806297f);
    cp = fmaf(cp, a2, -0.4999990463256836f);
    cp = fmaf(cp, a2, 0.9999999403953552f);
    const float c1 = cp;
    const int qi = (int)qf;
    cs = qi == 0 ? c1 : (qi == 1 ? -s1 : (qi == 2 ? -c1 : s1));
    sn = qi == 0 ? s1 : (qi == 1 ? c1 : (qi == 2 ? -s1 : -c1));
}

__device__ __forceinline__ float lerp2(float e00, float e01, float e10, float e11, float fr, float fc) {
    const float top = fmaf(fc, e01 - e00, e00);
    const float bot = fmaf(fc, e11 - e10, e10);
    return fmaf(fr, bot - top, top);
}

// Bilinear taps, floor() form of renderer_navigation.py:581-588: r0 = floor(row), c0 = floor(col); rows r0 and
// r0+1 clamp to [0,h-1], columns c0 and c0+1 wrap into [0,w).
//
// The DEM lives in HBM PADDED by two texels on every side (rows -2,-1 = row 0, rows h,h+1 = row h-1, columns
// -2,-1 = columns w-2,w-1, columns w,w+1 = columns 0,1; pitch = w+4), so a bilinear evaluation -- on the march
// path, where floor() lands in [-1,h-1] x [-1,w-1], and one texel either side of it for the normal -- is two
// unconditional 8-byte loads: no clamp, no wrap, no seam branch.
struct __attribute__((packed, aligned(8))) Quad { float a, b, c, d; };
struct __attribute__((packed, aligned(8))) UQuad { uint32_t a, b, c, d; };

template <bool WIDE>
__device__ __forceinline__ float dem_march(const FrameC& f, float rowf, float colf) {
    const float rfl = floorf(rowf), cfl = floorf(colf);
    const float fr = rowf - rfl, fc = colf - cfl;
    // padded index of (r0, c0) = (r0+2)*pitch + (c0+2); both factors < 2^24 -> one v_mad_u32_u24.  A single
    // unsigned min keeps any garbage (NaN position) inside the array; it never bites for a valid (lat, lon).
    const uint32_t r0p = (uint32_t)((int)rfl + 2), c0p = (uint32_t)((int)cfl + 2);
    const uint32_t idx = min(__umul24(r0p, (uint32_t)f.dem_pitch) + c0p, f.dem_maxidx);
    const char* base = reinterpret_cast<const char*>(f.dem);
    // row-pair layout: element (r, c) = (D[r][c], D[r+1][c]); elements (r0, c0) and (r0, c0+1) are adjacent, so the
    // whole 2x2 footprint is ONE 16-byte load -- half the gather instructions and L1 tag look-ups of two row loads
    // (tried and retired, DESIGN.md section 4.18: two 8-byte loads from a plain float32 DEM, 14.82 ms against 14.03; non-temporal loads
    // for the incoherent marches, path stage 6.85 ms against 5.4 -- the lines ARE reused)
    Quad q;
    if (WIDE) q = *reinterpret_cast<const Quad*>(base + ((uint64_t)idx << 3));
    else q = *reinterpret_cast<const Quad*>(base + (idx << 3));
    return lerp2(q.a, q.c, q.b, q.d, fr, fc);
}

// ---- D2/D3: the march.
// Texel coordinates are smooth along a ray, while the exact (lat, lon) -> (row, col) costs ~65 VALU (sqrt,
// reciprocal, two degree-15 polynomials, octant logic) and this kernel is VALU-issue bound.  Per SEG_N-step
// segment the exact coordinates are evaluated at the segment's start, middle and end only; the steps in
// between use the quadratic through those three (|error| <= ~1e-3 row / 7e-3 column texels for rho >= 0.2 R,
// i.e. the float32 resolution of the coordinate itself).  Segments that touch the polar cap or straddle
// the +/-180 seam evaluate every step exactly.  DEM evaluations, hit tests and counters are unchanged.
constexpr int SEG_N = 16;
struct Seg {
    float sa, ra, r1, r2, ca, c1, c2;
    int jlo, jhi;   // steps of this segment that can possibly be at/below the surface (see seg_setup)
#ifdef MRTX_PROF_FULLIV
    int why;        // measurement only: why the max-mip gave no interval (1 rows, 2 columns, 3 map edge; 0 = it did)
#endif
    bool exact;
};
// per-march constants of r^2(s) = q0 + 2 b s + a s^2
struct RayQ { float q0, b, a; };

__device__ __forceinline__ void exact_rowcol(const FrameC& f, float pa, float pb, float pc, float& rowf, float& colf,
                                             float& rho2) {
    rho2 = fmaf(pb, pb, pa * pa);
    float lat, lon;
    latlon(pa, pb, pc, rho2, lat, lon);
    rowf = fmaf(lat, f.gd.row_scale, f.gd.row_off);
    colf = fmaf(lon, f.gd.col_scale, f.gd.col_off);
}

// Anchors + quadratic of one segment, and the RESULT-PRESERVING skip interval:
// the max-mip (64x64-texel cell maxima, ~1 MB, cache resident) bounds D over the footprint of the three
// anchors (+1 texel for the bilinear tap and the quadratic's bulge): D <= Dmax there.  A step can only be at or
// below the surface if r^2(s) <= (R Dmax)^2; r^2(s) is a parabola in s, so those steps form one interval
// [jlo, jhi] (widened by a step each side and by 1e-5 in the bound, which dwarfs every rounding involved,
// so approximate v_sqrt/v_rcp are fine here).  Steps outside it cannot hit and are not evaluated; the ray's
// termination test is monotone, so it is enough to apply it at evaluated steps and at the segment end.
// seg_setup in two phases: seg_anchors = the anchors, the quadratic and WHERE the max-mip is to be read; seg_interval = the skip interval from the cells.
#ifndef MRTX_TAP_COLS
#define MRTX_TAP_COLS 4       // a footprint of up to MRTX_TAP_COLS cells along the columns still gets its skip interval (see seg_anchors)
#endif
struct MipTap { uint32_t off; bool usable, two_r, two_c; int ncol; };
__device__ __forceinline__ void seg_anchors(const FrameC& f, float oa, float ob, float oc, float da, float db, float dc,
                                            int ka, float rowA, float colA, float q2A, Seg& sg,
                                            float& rowB, float& colB, float& q2B, MipTap& tap) {
    const float sm = (float)(ka + SEG_N / 2) * f.step, sb = (float)(ka + SEG_N) * f.step;
    float rM, cM, q2M;
    exact_rowcol(f, fmaf(sm, da, oa), fmaf(sm, db, ob), fmaf(sm, dc, oc), rM, cM, q2M);
    exact_rowcol(f, fmaf(sb, da, oa), fmaf(sb, db, ob), fmaf(sb, dc, oc), rowB, colB, q2B);
    const float hw = 0.5f * f.gd.wf;
    const float qmin = fminf(q2A, fminf(q2M, q2B));
    sg.exact = (fabsf(cM - colA) > hw) || (fabsf(colB - colA) > hw) || (qmin < f.polar_rho2);
    sg.sa = (float)ka * f.step;
    sg.ra = rowA; sg.ca = colA;
    sg.r2 = (fmaf(-2.0f, rM, rowA) + rowB) * 0.0078125f;
    sg.r1 = fmaf(-16.0f, sg.r2, (rowB - rowA) * 0.0625f);
    sg.c2 = (fmaf(-2.0f, cM, colA) + colB) * 0.0078125f;
    sg.c1 = fmaf(-16.0f, sg.c2, (colB - colA) * 0.0625f);

    sg.jlo = 1; sg.jhi = SEG_N;
    tap.usable = false; tap.two_r = tap.two_c = false; tap.off = 0u; tap.ncol = 1;
    if (f.mip != nullptr) {
        const int i0 = ((int)floorf(fminf(rowA, fminf(rM, rowB))) - 1) >> f.mip_shift;
        const int i1 = ((int)floorf(fmaxf(rowA, fmaxf(rM, rowB))) + 2) >> f.mip_shift;
        const int j0 = ((int)floorf(fminf(colA, fminf(cM, colB))) - 1) >> f.mip_shift;
        const int j1 = ((int)floorf(fmaxf(colA, fmaxf(cM, colB))) + 2) >> f.mip_shift;
        // Columns shrink with cos(latitude): a ray that travels east-west at 30 degrees of latitude already covers more columns in
        // 16 steps than a cell is wide, and round 4 found 23 % of all camera and shadow segments of the cfg3 frame WITHOUT a skip
        // interval for that reason alone.  Up to four cells along the columns are therefore allowed (a second 16-byte load).
        tap.usable = !sg.exact & (i1 - i0 <= 1) & (j1 - j0 <= MRTX_TAP_COLS - 1) & (i0 >= -1) & (i1 <= f.mip_h) & (j0 >= -1) &
                     (j1 <= f.mip_w);
        tap.two_r = i1 > i0; tap.two_c = j1 > j0; tap.ncol = j1 - j0 + 1;
#ifdef MRTX_PROF_FULLIV
        sg.why = sg.exact ? 4 : (i1 - i0 > 1) ? 1 : (j1 - j0 > MRTX_TAP_COLS - 1) ? 2 : tap.usable ? 0 : 3;
#endif
        // the mip is stored in row pairs as well (element (i, j) = (m[i][j], m[i+1][j])): one 16-byte load brings the
        // 2x2 cells at (i0, j0); the ones the footprint does not reach are ignored, so the bound is the old one
        tap.off = tap.usable ? ((uint32_t)((i0 + 1) * f.mip_pitch + j0 + 1) << 3) : 0u;
    }
}
__device__ __forceinline__ Quad mip_fetch(const FrameC& f, const MipTap& tap) {
    return *reinterpret_cast<const Quad*>(reinterpret_cast<const char*>(f.mip) + tap.off);
}
template <bool STATS>
__device__ __forceinline__ void seg_interval(const FrameC& f, const RayQ& rq, Seg& sg, const MipTap& tap, const Quad& q,
                                             uint32_t* cnt, float dmax_more = 0.0f) {
    const float dmax = fmaxf(fmaxf(fmaxf(q.a, tap.two_r ? q.b : q.a), fmaxf(tap.two_c ? q.c : q.a, (tap.two_r & tap.two_c) ? q.d : q.a)), dmax_more);
    if (STATS) cnt[ST_MIP] += 4;
    const float rd = f.Rf * dmax;
    const float T = (rd * rd) * 1.00001f;
    const float disc = fmaf(rq.b, rq.b, -rq.a * (rq.q0 - T));
    if (disc < 0.0f) {
        sg.jlo = SEG_N + 1; sg.jhi = SEG_N;      // the whole segment stays above Dmax
    } else {
        const float sq = __builtin_amdgcn_sqrtf(disc), inva = __builtin_amdgcn_rcpf(rq.a);
        const float u1 = fminf(fmaxf(((-rq.b - sq) * inva - sg.sa) * f.inv_step, -4.0f), 64.0f);
        const float u2 = fminf(fmaxf(((-rq.b + sq) * inva - sg.sa) * f.inv_step, -4.0f), 64.0f);
        sg.jlo = min(SEG_N + 1, max(1, (int)floorf(u1) - 1));
        sg.jhi = min(SEG_N, (int)ceilf(u2) + 1);
    }
}
template <bool STATS>
__device__ __forceinline__ void seg_setup(const FrameC& f, float oa, float ob, float oc, float da, float db, float dc,
                                          const RayQ& rq, int ka, float rowA, float colA, float q2A, Seg& sg,
                                          float& rowB, float& colB, float& q2B, uint32_t* cnt) {
    MipTap tap;
    seg_anchors(f, oa, ob, oc, da, db, dc, ka, rowA, colA, q2A, sg, rowB, colB, q2B, tap);
    if (tap.usable) {
        const Quad q = mip_fetch(f, tap);
        float more = 0.0f;       // D > 0 everywhere: zero is neutral for the maximum
#pragma unroll
        for (int c = 2; c < MRTX_TAP_COLS; c += 2) {      // columns j0 + c (and j0 + c + 1): the next two cells of the same row pair
            if (tap.ncol > c) {
                const Quad q2 = *reinterpret_cast<const Quad*>(reinterpret_cast<const char*>(f.mip) + tap.off + 8u * (uint32_t)c);
                more = fmaxf(more, fmaxf(q2.a, tap.two_r ? q2.b : q2.a));
                if (tap.ncol > c + 1) more = fmaxf(more, fmaxf(q2.c, tap.two_r ? q2.d : q2.c));
                if (STATS) cnt[ST_MIP] += 4;
            }
        }
        seg_interval<STATS>(f, rq, sg, tap, q, cnt, more);
    }
}

// is the point at or below the displaced surface?  r^2 <= (R * D(row, col))^2
// EXACTABLE = false: the caller knows (by ballot) that no lane of the wave is in an exact-fallback segment.
// The quadratic needs no clamp: a non-seam, non-polar segment keeps (row, col) >= 0.5 texel inside
// [-1, h) x [-1, w), and dem_march()'s unsigned index clamp keeps even a NaN inside the allocation.
template <bool WIDE, bool EXACTABLE>
__device__ __forceinline__ bool below_seg(const FrameC& f, const Seg& sg, float sk, float pa, float pb, float pc,
                                          float r2) {
    const float u = (sk - sg.sa) * f.inv_step;
    float rowf = fmaf(u, fmaf(u, sg.r2, sg.r1), sg.ra);
    float colf = fmaf(u, fmaf(u, sg.c2, sg.c1), sg.ca);
    if (EXACTABLE && sg.exact) {
        float q2;
        exact_rowcol(f, pa, pb, pc, rowf, colf, q2);
    }
    const float surf = f.Rf * dem_march<WIDE>(f, rowf, colf);
    return r2 <= surf * surf;
}

// The steps jlo..jhi of one segment, per lane.  Branch-free body: the DEM is sampled even on the step that
// turns out to lie outside (its result is discarded), so the only control flow is the loop-back on the
// ballot of lanes still stepping.
//
// The kernel is bound by DEPENDENT-LOAD LATENCY (each round trip ~1-2 k cycles under load, five waves per SIMD
// to hide it), so the plain-quadratic variant evaluates MRTX_STEP_BATCH consecutive steps per iteration: all
// their DEM loads are issued back to back, then the steps are tested in march order and everything after the
// first terminating one is discarded.  Same evaluations, same order, same result; a few wasted fetches.
// Measured at cfg3: batch 1 15.19 ms, 2 14.83, 4 16.57 (+11 % fetches), 8 18.55.
#ifndef MRTX_STEP_BATCH
#define MRTX_STEP_BATCH 2
#endif
#ifndef MRTX_SHADOW_BATCH
#define MRTX_SHADOW_BATCH MRTX_STEP_BATCH     // the first vertex's shadow march in render_kernel<MODE 2> (A/B: 1 / 2 / 3)
#endif
#ifndef MRTX_STEP_BATCH_BOUNCE
#define MRTX_STEP_BATCH_BOUNCE 1
#endif
// BOUNDED (shadow rays only; mrtx_sight_*): the ray also ends before the first step with s_k >= smax, the
// segment's far end.  Every other caller leaves it false and compiles to the code it always had.
template <bool WIDE, bool PRIMARY, bool STATS, bool EXACTABLE, int BATCH, bool BOUNDED = false>
__device__ __forceinline__ void step_loop_from(const FrameC& f, float oa, float ob, float oc, float da, float db, float dc,
                                               float smax, const Seg& sg, int ka, int j, bool more, bool& go, bool& hit,
                                               float& sk_out, uint32_t* cnt) {
    if (EXACTABLE || BATCH == 1) {
        while (more) {
            const int k = ka + j;
            const float sk = (float)k * f.step;
            const float pa = fmaf(sk, da, oa), pb = fmaf(sk, db, ob), pc = fmaf(sk, dc, oc);
            const float r2 = fmaf(pc, pc, fmaf(pb, pb, pa * pa));
            const bool in = (PRIMARY ? (sk <= smax) : (r2 <= f.R2f)) & (!BOUNDED || sk < smax) & (k <= f.kmax);
            const bool bel = below_seg<WIDE, EXACTABLE>(f, sg, sk, pa, pb, pc, r2);
            if (STATS) { cnt[ST_HEIGHT] += in ? 1u : 0u; cnt[ST_FETCH]++; }
#ifdef MRTX_PROF
            cnt[11] += 1;                                    // wave-level step iterations
            cnt[12] += (uint32_t)__popcll(__ballot(true));   // lanes evaluating in them
#endif
            hit = in & bel;
            go = in & !bel;
            sk_out = sk;
            j++;
            more = go & (j <= sg.jhi);
        }
    } else {
        constexpr int B = BATCH;
        while (more) {
            float surf[B];
#pragma unroll
            for (int i = 0; i < B; i++) {
                // steps past jhi are evaluated at the segment's last step instead (inside the quadratic's range)
                const float u = ((float)(ka + min(j + i, SEG_N)) * f.step - sg.sa) * f.inv_step;   // as below_seg()
                const float rowf = fmaf(u, fmaf(u, sg.r2, sg.r1), sg.ra);
                const float colf = fmaf(u, fmaf(u, sg.c2, sg.c1), sg.ca);
                surf[i] = f.Rf * dem_march<WIDE>(f, rowf, colf);
            }
#ifdef MRTX_PROF
            cnt[11] += 1;
            cnt[12] += (uint32_t)__popcll(__ballot(true));
#endif
            bool act = true;
#pragma unroll
            for (int i = 0; i < B; i++) {
                const int k = ka + j + i;
                const float sk = (float)k * f.step;
                const float pa = fmaf(sk, da, oa), pb = fmaf(sk, db, ob), pc = fmaf(sk, dc, oc);
                const float r2 = fmaf(pc, pc, fmaf(pb, pb, pa * pa));
                const bool in = (PRIMARY ? (sk <= smax) : (r2 <= f.R2f)) & (!BOUNDED || sk < smax) & (k <= f.kmax);
                const bool bel = r2 <= surf[i] * surf[i];
                if (STATS) { cnt[ST_HEIGHT] += (act & in) ? 1u : 0u; cnt[ST_FETCH] += act ? 1u : 0u; }   // speculative fetches are not credited
                hit = act ? (in & bel) : hit;
                go = act ? (in & !bel) : go;
                sk_out = act ? sk : sk_out;
                act = act & go & (j + i + 1 <= sg.jhi);
            }
            j += B;
            more = act;
        }
    }
}

template <bool WIDE, bool PRIMARY, bool STATS, bool EXACTABLE, int BATCH, bool BOUNDED = false>
__device__ __forceinline__ void step_loop(const FrameC& f, float oa, float ob, float oc, float da, float db, float dc,
                                          float smax, const Seg& sg, int ka, bool& go, bool& hit, float& sk_out,
                                          uint32_t* cnt) {
    step_loop_from<WIDE, PRIMARY, STATS, EXACTABLE, BATCH, BOUNDED>(f, oa, ob, oc, da, db, dc, smax, sg, ka, sg.jlo, sg.jlo <= sg.jhi,
                                                                       go, hit, sk_out, cnt);
}

// STATS builds only: the spec counts a DEM evaluation at every step that is still inside; add the skipped ones.
template <bool PRIMARY, bool BOUNDED = false>
__device__ __forceinline__ uint32_t count_in_steps(const FrameC& f, float oa, float ob, float oc, float da, float db,
                                                   float dc, float smax, int ka, int j_from, int j_to) {
    uint32_t n = 0;
    for (int j = j_from; j <= j_to; j++) {
        const int k = ka + j;
        const float sk = (float)k * f.step;
        const float pa = fmaf(sk, da, oa), pb = fmaf(sk, db, ob), pc = fmaf(sk, dc, oc);
        const float r2 = fmaf(pc, pc, fmaf(pb, pb, pa * pa));
        const bool in = (PRIMARY ? (sk <= smax) : (r2 <= f.R2f)) & (!BOUNDED || sk < smax) & (k <= f.kmax);
        if (!in) break;
        n++;
    }
    return n;
}

// Per-ray march state between segments: the ray, the coefficients of r^2(s) and the exact texel coordinates at the
// start of the next segment (step ka).
struct MarchState {
    float oa, ob, oc, da, db, dc;
    RayQ rq;
    float rowA, colA, q2A;
    int ka;
    int kend;   // no step beyond this one can be at/below the surface (horizon_kend); kmax when nothing is known
};

// RESULT-PRESERVING end of a shadow / continuation march: once an ASCENDING ray (b = o.d >= 0, so r^2(s) grows
// monotonically) is above everything its remaining ground track can reach, no later step can be at/below the surface,
// and the march can stop there instead of stepping -- or setting up empty segments -- until it leaves the bounding sphere.
// "Everything it can reach" comes from the HORIZON MIP: cells of Cc = 8 fine-mip cells (512 texels at cfg 3), each holding
// the maximum of D over the cell DILATED by Cc texels on every side (rows clamp, columns wrap), so one look-up at the
// ray's origin bounds D over any ground track that stays within Cc texels of it.  The track's extent is bounded from the
// chord to the sphere exit L: it subtends phi <= 1.03 L / r0 at the centre (the ray stays above its origin radius r0), at most
// phi * h/pi rows and asin(sin phi / cos(lat_max)) * w/2pi <= 1.05 phi / (cos(lat0) - phi) * w/2pi columns; the test needs
// both (+4 texels for taps and the quadratic's bulge) inside Cc, otherwise nothing is cut.  Then the last step that can
// matter is where r^2(s) reaches (R Dc)^2 (1 + 1e-5).  Approximate v_sqrt / v_rcp are fine: every bound is padded.
// Radiance, hits and the spec counters are unchanged (MRTX_F_NO_SKIP switches this off together with the max-mip).
// the horizon-mip cell of a march origin at texel (rowA, colA): one look-up serves every ray that starts there
__device__ __forceinline__ float horizon_cell(const FrameC& f, float rowA, float colA) {
    int i = (int)floorf(rowA) >> CF(f)->hm_shift, j = (int)floorf(colA) >> CF(f)->hm_shift;
    i = max(0, min(i, CF(f)->hm_h - 1)); j = max(0, min(j, CF(f)->hm_w - 1));
    return CF(f)->hmip[i * CF(f)->hm_w + j];
}
// PRE: the caller has fetched horizon_cell(f, m.rowA, m.colA) already (`cell_pre`): same bound, no load here
template <bool PRE = false>
__device__ __forceinline__ int horizon_kend(const FrameC& f, const MarchState& m, float cell_pre = 0.0f) {
    int kend = f.kmax;
    const float* hm = CF(f)->hmip;
    if (hm != nullptr && m.rq.b >= 0.0f) {
        const float a = m.rq.a, b = m.rq.b, q0 = m.rq.q0;
        const float c = f.R2f - q0;                        // >= 0: the origin is inside the bounding sphere
        const float L = c * __builtin_amdgcn_rcpf(b + __builtin_amdgcn_sqrtf(fmaf(a, c, b * b)) + 1.0e-30f) * 1.02f;
        const float inv_cos = __builtin_amdgcn_sqrtf(q0 * __builtin_amdgcn_rcpf(fmaxf(m.q2A, 1.0e-30f)));   // r0 / rho0
        const float phi = L * __builtin_amdgcn_rsqf(q0) * 1.03f;   // 2 asin(L / 2 r0) <= 1.003 L / r0 for L <= r0 / 4; r(s) >= r0
        const float den = 1.0f - phi * inv_cos;            // cos(lat0) - phi, in units of cos(lat0)
        const float drow = fmaf(phi, CF(f)->hm_krow, 4.0f);
        const float dcol = fmaf(phi * CF(f)->hm_kcol, inv_cos * __builtin_amdgcn_rcpf(fmaxf(den, 0.25f)), 4.0f);
        const float cell = CF(f)->hm_cell;
        if ((c >= 0.0f) & (phi <= 0.25f) & (den >= 0.5f) & (drow <= cell) & (dcol <= cell)) {
            const float rd = f.Rf * (PRE ? cell_pre : horizon_cell(f, m.rowA, m.colA));
            const float d = (rd * rd) * 1.00001f - q0;
            if (d <= 0.0f) kend = 0;
            else {
                const float sc = d * __builtin_amdgcn_rcpf(b + __builtin_amdgcn_sqrtf(fmaf(a, d, b * b))) * 1.001f;
                kend = min(f.kmax, (int)(sc * f.inv_step) + 2);
            }
        }
    }
    return kend;
}
// horizon_kend() asked again from the start of segment m.ka (texel coordinates m.rowA / m.colA, rho^2 = m.q2A): the parabola's
// coefficients moved to that point.  Steps are counted from there; f.kmax = nothing known.
#ifndef MRTX_HORIZON_RETRY
#define MRTX_HORIZON_RETRY 2     // bit 0: render_kernel's shadow marches (measured: +0.55 ms, the test runs for the whole wave), bit 1: path_kernel (-0.13 ms)
#endif
__device__ __forceinline__ int horizon_retry(const FrameC& f, const MarchState& m) {
    const float s = (float)m.ka * f.step;
    MarchState t;
    t.rq.a = m.rq.a;
    t.rq.b = fmaf(m.rq.a, s, m.rq.b);
    t.rq.q0 = fmaf(s, fmaf(s, m.rq.a, m.rq.b + m.rq.b), m.rq.q0);
    t.q2A = m.q2A; t.rowA = m.rowA; t.colA = m.colA;
    return horizon_kend(f, t);
}
// STATS builds: the steps the spec evaluates after a march was cut at kend (every step while the ray is inside)
template <bool BOUNDED = false>
__device__ __forceinline__ uint32_t steps_after(const FrameC& f, const MarchState& m, int k_from, float smax = 0.0f) {
    uint32_t n = 0;
    for (int k = k_from; k <= f.kmax; k++) {
        const float sk = (float)k * f.step;
        const float pa = fmaf(sk, m.da, m.oa), pb = fmaf(sk, m.db, m.ob), pc = fmaf(sk, m.dc, m.oc);
        if (!(fmaf(pc, pc, fmaf(pb, pb, pa * pa)) <= f.R2f)) break;
        if (BOUNDED && !(sk < smax)) break;
        n++;
    }
    return n;
}

// Start of a march: exact coordinates at the origin, r^2(s) coefficients; returns `go` (false: the march is over before
// its first step).
// ... with the exact texel coordinates of the origin already known (m.rowA, m.colA)
// LAZY_KEND (path_kernel): the horizon bound is left open (m.kend = -1) and looked up by the first segment set-up, in the
// same memory round as that segment's max-mip fetch, instead of costing a round of its own here.
template <bool PRIMARY, bool STATS, bool LAZY_KEND = false, bool PRE_CELL = false, bool BOUNDED = false>
__device__ __forceinline__ bool march_begin_at(const FrameC& f, float oa, float ob, float oc, float da, float db, float dc,
                                               MarchState& m, uint32_t* cnt, float cell_pre = 0.0f, float smax = 0.0f) {
    m.oa = oa; m.ob = ob; m.oc = oc; m.da = da; m.db = db; m.dc = dc;
    m.q2A = fmaf(ob, ob, oa * oa);
    m.rq.q0 = fmaf(oc, oc, m.q2A);
    m.rq.b = fmaf(oc, dc, fmaf(ob, db, oa * da));
    m.rq.a = fmaf(dc, dc, fmaf(db, db, da * da));
    m.ka = 0;
    bool go = true;
    if (!PRIMARY) {
        // The skip below relies on "once outside, always outside".  r^2(s) is convex, so that holds from the first
        // step that is inside -- but an origin lifted by scene_epsilon off a D = 1 texel can sit just outside R and head
        // inward: the march ends at step 1 (spec), and must not resume where the parabola dips back inside.
        const float s1 = f.step;
        const float pa = fmaf(s1, da, oa), pb = fmaf(s1, db, ob), pc = fmaf(s1, dc, oc);
        go = fmaf(pc, pc, fmaf(pb, pb, pa * pa)) <= f.R2f;
        if (BOUNDED) go = go && s1 < smax;
        if (LAZY_KEND) {
            m.kend = -1;
        } else {
            m.kend = horizon_kend<PRE_CELL>(f, m, cell_pre);
            if (go && m.kend < 1) {          // already above everything in reach: no step can hit
                if (STATS) cnt[ST_HEIGHT] += steps_after<BOUNDED>(f, m, 1, smax);
                go = false;
            }
        }
    } else {
        m.kend = f.kmax;
    }
    return go;
}
template <bool PRIMARY, bool STATS, bool LAZY_KEND = false, bool BOUNDED = false>
__device__ __forceinline__ bool march_begin(const FrameC& f, float oa, float ob, float oc, float da, float db, float dc,
                                            MarchState& m, uint32_t* cnt, float smax = 0.0f) {
    float q2;
    exact_rowcol(f, oa, ob, oc, m.rowA, m.colA, q2);
    return march_begin_at<PRIMARY, STATS, LAZY_KEND, false, BOUNDED>(f, oa, ob, oc, da, db, dc, m, cnt, 0.0f, smax);
}

// End of a segment whose steps are through: a ray that is still marching (`go`) may have ended inside the skipped tail, or
// is cut by its horizon bound; the march state moves on to the next segment.
template <bool PRIMARY, bool STATS, bool BOUNDED = false>
__device__ __forceinline__ void segment_tail(const FrameC& f, MarchState& m, float smax, const Seg& sg, bool& go, float rowB,
                                             float colB, float q2B, uint32_t* cnt) {
    const float oa = m.oa, ob = m.ob, oc = m.oc, da = m.da, db = m.db, dc = m.dc;
    const int ka = m.ka;
    if (go) {
        // still marching after the last evaluated step: did the ray end inside the skipped tail?
        if (STATS) cnt[ST_HEIGHT] += count_in_steps<PRIMARY, BOUNDED>(f, oa, ob, oc, da, db, dc, smax, ka, max(sg.jhi + 1, 1), SEG_N);
        const int k = ka + SEG_N;
        const float sk = (float)k * f.step;
        const float pa = fmaf(sk, da, oa), pb = fmaf(sk, db, ob), pc = fmaf(sk, dc, oc);
        go = (PRIMARY ? (sk <= smax) : (fmaf(pc, pc, fmaf(pb, pb, pa * pa)) <= f.R2f)) & (!BOUNDED || sk < smax) & (k < f.kmax);
        if (!PRIMARY && go && k >= m.kend) {           // cut by the horizon bound: the rest of the ray is above the terrain
            if (STATS) cnt[ST_HEIGHT] += steps_after<BOUNDED>(f, m, k + 1, smax);
            go = false;
        }
    }
    m.ka = ka + SEG_N; m.rowA = rowB; m.colA = colB; m.q2A = q2B;
}

// Camera rays: the FIRST step of the skip interval [jlo, jhi] that the medium max-mip cannot prove above the surface (jhi + 1 when it
// proves them all).  A camera ray descends onto the terrain and its march ends at the first step at or below it, so only the front of
// the interval matters: the steps are tested in march order, four per memory round, and a lane stops at its first inconclusive one.
// The test itself only has to be CONSERVATIVE, not the spec's arithmetic: the step's texel position from the segment's quadratic at
// u = j (the spec's u differs by < 3e-4, a thousandth of a texel; a cell's maximum covers two texels more than its own rows and
// columns on the low side and one more than a bilinear tap needs on the high side, mip_build_kernel), r^2 from the ray's parabola
// (its terms are ~R^2 each and s reaches 2R: good to ~1e-6 relative, a tenth of the comparison's 1e-5 margin -- the margin seg_interval
// has relied on since round 1; the evaluation's own r^2 is as close to the true value).  Result-preserving like every other skip.
#ifndef MRTX_PMASK_Q
#define MRTX_PMASK_Q 4        // tests per memory round in render_kernel's marches (cfg3: 2 -> 14.0 ms, 3 -> 13.9, 4 -> 13.75, 6 -> 13.9)
#endif
#ifndef MRTX_PATH_MASK_Q
#define MRTX_PATH_MASK_Q 8    // ... and in path_kernel, which is bound by its dependent memory rounds (4 -> 4.84 ms, 6 -> 4.75, 8 -> 4.64, 16 -> 6.4: spills)
#endif
// ... and the mirror image for shadow and continuation rays, which LEAVE the terrain: their first steps are close to the surface,
// the later ones far above it, so the interval is cut from its END -- the steps are tested backwards from jhi and a lane stops at
// the first one the medium mip cannot prove above the surface: that is the new jhi (jlo - 1 when every step is proven above).
template <bool STATS, int Q>
__device__ __forceinline__ int last_kept_step(const FrameC& f, const MarchState& m, const Seg& sg, uint32_t* cnt) {
    const float* m2 = CF(f)->mip2;
    const int pitch = CF(f)->m2_pitch, sh = CF(f)->m2_shift;
    const uint32_t maxidx = (uint32_t)((CF(f)->m2_h + 2) * pitch - 1);
    const float two_b = m.rq.b + m.rq.b;
    int j = sg.jhi;
    int last = sg.jhi;
    bool open = (sg.jlo <= sg.jhi) & !sg.exact;
    if (open) last = sg.jlo - 1;
    while (open) {
        float mv[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const float u = (float)max(j - q, sg.jlo);
            const float rowf = fmaf(u, fmaf(u, sg.r2, sg.r1), sg.ra), colf = fmaf(u, fmaf(u, sg.c2, sg.c1), sg.ca);
            const int i = (int)floorf(rowf) >> sh, c = (int)floorf(colf) >> sh;
            mv[q] = m2[min((uint32_t)((i + 1) * pitch + c + 1), maxidx)];
        }
        bool found = false;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int jj = j - q;
            const float sk = fmaf((float)max(jj, sg.jlo), f.step, sg.sa);
            const float r2 = fmaf(sk, fmaf(sk, m.rq.a, two_b), m.rq.q0);
            const float rd = f.Rf * mv[q];
            const bool kept = !(r2 > (rd * rd) * 1.00001f);
            if (STATS) cnt[ST_MIP] += (!found && jj >= sg.jlo) ? 1u : 0u;
            if (!found && jj >= sg.jlo && kept) { last = jj; found = true; }
        }
        j -= Q;
        open = !found && j >= sg.jlo;
    }
    return last;
}
template <bool STATS, int Q>
__device__ __forceinline__ int first_kept_step(const FrameC& f, const MarchState& m, const Seg& sg, uint32_t* cnt) {
    const float* m2 = CF(f)->mip2;
    const int pitch = CF(f)->m2_pitch, sh = CF(f)->m2_shift;
    const uint32_t maxidx = (uint32_t)((CF(f)->m2_h + 2) * pitch - 1);
    const float two_b = m.rq.b + m.rq.b;
    int j = sg.jlo;
    int first = sg.jlo;
    bool open = (sg.jlo <= sg.jhi) & !sg.exact;
    if (open) first = sg.jhi + 1;
    while (open) {
        float mv[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const float u = (float)min(j + q, sg.jhi);
            const float rowf = fmaf(u, fmaf(u, sg.r2, sg.r1), sg.ra), colf = fmaf(u, fmaf(u, sg.c2, sg.c1), sg.ca);
            const int i = (int)floorf(rowf) >> sh, c = (int)floorf(colf) >> sh;
            mv[q] = m2[min((uint32_t)((i + 1) * pitch + c + 1), maxidx)];      // one-cell border; the clamp never bites for a valid segment
        }
        bool found = false;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int jj = j + q;
            const float sk = fmaf((float)min(jj, sg.jhi), f.step, sg.sa);
            const float r2 = fmaf(sk, fmaf(sk, m.rq.a, two_b), m.rq.q0);
            const float rd = f.Rf * mv[q];
            const bool kept = !(r2 > (rd * rd) * 1.00001f);
            if (STATS) cnt[ST_MIP] += (!found && jj <= sg.jhi) ? 1u : 0u;
            if (!found && jj <= sg.jhi && kept) { first = jj; found = true; }
        }
        j += Q;
        open = !found && j <= sg.jhi;
    }
    return first;
}
// The part of march_segment() before the steps: the late horizon bound, anchors + skip interval, the cuts of the interval.  Returns false
// when the march ended before this segment (`go` is false then); rowB / colB / q2B are the segment's far anchor, for segment_tail().
template <bool PRIMARY, bool STATS, int SCAN, bool BOUNDED>
__device__ __forceinline__ bool segment_head(const FrameC& f, MarchState& m, float smax, Seg& sg, bool& go, float& rowB, float& colB,
                                             float& q2B, uint32_t* cnt) {
    const float oa = m.oa, ob = m.ob, oc = m.oc, da = m.da, db = m.db, dc = m.dc;
    const int ka = m.ka;
    if (!PRIMARY && (MRTX_HORIZON_RETRY & 1) != 0 && ka > 0 && m.kend >= f.kmax) {
        // The horizon bound was out of reach at the ray's origin (its ground track to the sphere exit is longer than the horizon
        // cell's dilation: low rays, and any east-west ray at high latitude, where columns shrink).  The ray has climbed since:
        // asked again from HERE, the remaining track is shorter and the bound may apply.
        const int ke = horizon_retry(f, m);
        if (ke < 1) {                        // above everything in reach already: the march ends before this segment
            if (STATS) cnt[ST_HEIGHT] += steps_after<BOUNDED>(f, m, ka + 1, smax);
            go = false;
            return false;
        }
        m.kend = min(f.kmax, ka + ke);       // ke == kmax: still unknown
    }
    PROF_BEGIN(6);
    seg_setup<STATS>(f, oa, ob, oc, da, db, dc, m.rq, ka, m.rowA, m.colA, m.q2A, sg, rowB, colB, q2B, cnt);
#ifdef MRTX_PROF_FULLIV   // measurement only: how many lanes get NO skip interval from the max-mip (footprint over more than 2 x 2 cells, or a true full interval)
    { const bool full = (sg.jlo == 1) & (sg.jhi == SEG_N) & !sg.exact;
      cnt[13] += (uint32_t)__popcll(__ballot(full)); cnt[14] += (uint32_t)__popcll(__ballot(sg.exact));
      cnt[5] += (uint32_t)__popcll(__ballot(full && sg.why == 1)); cnt[6] += (uint32_t)__popcll(__ballot(full && sg.why == 2));
      cnt[7] += (uint32_t)__popcll(__ballot(full && sg.why == 3)); }
#endif
    if (!PRIMARY) sg.jhi = max(min(sg.jhi, m.kend - ka), sg.jlo - 1);   // steps beyond kend cannot be at/below the surface
    // the medium max-mip cuts the interval once more (first_kept_step / last_kept_step above): camera rays from the front, shadow rays
    // from the end; MRTX_SEG_MASK bits 2 / 1 switch the two off (A/B)
    if (SCAN == 1 && (MRTX_SEG_MASK & 4) != 0 && CF(f)->mip2 != nullptr) sg.jlo = first_kept_step<STATS, MRTX_PMASK_Q>(f, m, sg, cnt);
    if (SCAN == 2 && (MRTX_SEG_MASK & 2) != 0 && CF(f)->mip2 != nullptr) sg.jhi = last_kept_step<STATS, MRTX_PMASK_Q>(f, m, sg, cnt);
    if (SCAN == 3 && (MRTX_SEG_MASK & 1) != 0 && CF(f)->mip2 != nullptr) sg.jhi = last_kept_step<STATS, MRTX_PMASK_Q>(f, m, sg, cnt);   // A/B: the trial segment
    PROF_END(6);
    return true;
}
// ONE 16-step segment of a march (the lanes that call it are still marching): anchors + skip interval, the steps
// that can be at/below the surface, the termination test at the segment end.  `hit` / `sk_hit` are set by the step
// that lands at/below the surface, `go` says whether the ray continues with the next segment.
template <bool WIDE, bool PRIMARY, bool STATS, int BATCH, int SCAN = PRIMARY ? 1 : 0, bool BOUNDED = false>
__device__ __forceinline__ void march_segment(const FrameC& f, MarchState& m, float smax, Seg& sg, bool& go, bool& hit,
                                              float& sk_hit, uint32_t* cnt) {
    const float oa = m.oa, ob = m.ob, oc = m.oc, da = m.da, db = m.db, dc = m.dc;
    const int ka = m.ka;
    float rowB, colB, q2B;
    if (!segment_head<PRIMARY, STATS, SCAN, BOUNDED>(f, m, smax, sg, go, rowB, colB, q2B, cnt)) return;
    PROF_BEGIN(7);
    if (STATS) cnt[ST_HEIGHT] += count_in_steps<PRIMARY, BOUNDED>(f, oa, ob, oc, da, db, dc, smax, ka, 1, sg.jlo - 1);
    if (__ballot(sg.exact) != 0ull)
        step_loop<WIDE, PRIMARY, STATS, true, 1, BOUNDED>(f, oa, ob, oc, da, db, dc, smax, sg, ka, go, hit, sk_hit, cnt);
    else
        step_loop<WIDE, PRIMARY, STATS, false, BATCH, BOUNDED>(f, oa, ob, oc, da, db, dc, smax, sg, ka, go, hit, sk_hit, cnt);
    PROF_END(7);
#ifdef MRTX_PROF
#if !defined(MRTX_PROF_TRIAL) && !defined(MRTX_PROF_FULLIV)
    cnt[8] += 1;                                     // wave-level segments
    cnt[9] += (uint32_t)__popcll(__ballot(true));    // lanes alive in them
    cnt[PRIMARY ? 13 : 14] += (__ballot(sg.jlo <= sg.jhi) == 0ull) ? 1u : 0u;   // wave-level segments nobody steps in
    cnt[15] += PRIMARY ? 1u : 0u;
#endif
#ifdef MRTX_PROF_FULLIV
    cnt[8] += 1; cnt[9] += (uint32_t)__popcll(__ballot(true));
#endif
#endif
    segment_tail<PRIMARY, STATS, BOUNDED>(f, m, smax, sg, go, rowB, colB, q2B, cnt);
}

// ---- The trial segment's steps, dealt out over the wave (render_kernel<MODE 2>).
// The trial segment is the first segment (ka = 0) of the 64 continuation rays of a wave.  Its rays are incoherent: a few grazing ones
// keep all their steps while most have none or one, and the serial loop (step_loop_from, one step per iteration) runs for as long as
// the longest lane.  A step's evaluation is a pure function of the ray, the segment's quadratic and the step number, and the loop
// carries nothing from step to step but "stop at the first step that is outside or at/below the surface" -- so the pending steps of
// all lanes are laid out as ONE work list (a ray's steps contiguous, rays in lane order), the list is evaluated 64 items at a time by
// the 64 lanes, and two ballots per window give every ray its first terminating item.  Same arithmetic per step (the expressions of step_loop_from / below_seg with sa = 0), same
// first terminating step, same counters: items past a ray's terminating step are speculative fetches inside the segment's range, like
// the second step of MRTX_STEP_BATCH 2, and are not credited.  Not a skip: it stays on under MRTX_F_NO_SKIP.
//
// Called by ALL 64 lanes of the wave in wave-uniform control flow (`live`: this lane has a trial segment set up).  Exchange through
// LDS: three 16-byte slots per lane for a ray's state (`st`: slot-major like the parking slots, which are free during the trial) and
// one spare 32-bit word per lane (`ctl`, stride four words; see below).
#ifndef MRTX_TRIAL_WIDE
#define MRTX_TRIAL_WIDE 1       // 0 = the serial loop (A/B switch; the results are the same bits)
#endif
#ifndef MRTX_TRIAL_WIDE_K
#define MRTX_TRIAL_WIDE_K 5     // serial iterations before the pending steps are counted: the first ones still have most lanes at work
                                // (render_kernel at cfg3: 0 -> 13.61 ms, 1 -> 13.33, 2 -> 13.00, 3 -> 12.85-12.91, 4 -> 12.86-12.95, 5 -> 12.86, 6 -> 12.94;
                                // the serial loop 13.05-13.15)
#endif
#ifndef MRTX_TRIAL_WIDE_MIN
#define MRTX_TRIAL_WIDE_MIN 2   // go wide when the longest lane has this many more steps pending than full rounds would take
#endif
typedef float xch4 __attribute__((ext_vector_type(4)));
// one wave per workgroup: its LDS instructions execute in order; what is needed is that the compiler keeps them in order too
__device__ __forceinline__ void xch_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// one step of a ka = 0, non-primary segment: step_loop_from's `in` and below_seg's `bel`, expression by expression
template <bool WIDE>
__device__ __forceinline__ void trial_step(const FrameC& f, float ra, float r1, float r2, float ca, float c1, float c2, float oa,
                                           float ob, float oc, float da, float db, float dc, int k, bool& in, bool& bel) {
    const float sk = (float)k * f.step;
    const float pa = fmaf(sk, da, oa), pb = fmaf(sk, db, ob), pc = fmaf(sk, dc, oc);
    const float q = fmaf(pc, pc, fmaf(pb, pb, pa * pa));
    in = (q <= f.R2f) & (k <= f.kmax);
    const float u = (sk - 0.0f) * f.inv_step;          // sg.sa = (float)0 * step
    const float rowf = fmaf(u, fmaf(u, r2, r1), ra);
    const float colf = fmaf(u, fmaf(u, c2, c1), ca);
    const float surf = f.Rf * dem_march<WIDE>(f, rowf, colf);
    bel = q <= surf * surf;
}
template <bool WIDE, bool STATS>
__device__ __forceinline__ void trial_steps_wide(const FrameC& f, const MarchState& m, const Seg& sg, bool live, xch4* st,
                                                 uint32_t* ctl, bool& go, bool& hit, float& sk_out, uint32_t* cnt) {
    if (__ballot(live && sg.exact) != 0ull) {      // a lane in an exact-fallback segment: the wave keeps the serial loop
        if (live) step_loop<WIDE, false, STATS, true, 1>(f, m.oa, m.ob, m.oc, m.da, m.db, m.dc, 0.0f, sg, 0, go, hit, sk_out, cnt);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const int jhi = live ? sg.jhi : 0;
    int j = live ? sg.jlo : 1;
    bool pend = j <= jhi;
#pragma unroll
    for (int it = 0; it < MRTX_TRIAL_WIDE_K; it++) {
        if (pend) {
            bool in, bel;
            trial_step<WIDE>(f, sg.ra, sg.r1, sg.r2, sg.ca, sg.c1, sg.c2, m.oa, m.ob, m.oc, m.da, m.db, m.dc, j, in, bel);
            if (STATS) { cnt[ST_HEIGHT] += in ? 1u : 0u; cnt[ST_FETCH]++; }
#ifdef MRTX_PROF
            cnt[11] += 1;
#endif
            hit = in & bel; go = in & !bel; sk_out = (float)j * f.step;
            j++;
            pend = go & (j <= jhi);
        }
    }
    // every lane's place in the work list: an exclusive prefix sum of the pending counts (at most SEG_N = 16: five ballots), their
    // total and their maximum
    uint32_t n, start, W, nmax;
    auto deal = [&]() {
        n = pend ? (uint32_t)(jhi - j + 1) : 0u;
        start = 0u; W = 0u; nmax = 0u;
        bool top = true;
#pragma unroll
        for (int b = 4; b >= 0; b--) {
            const bool bit = ((n >> b) & 1u) != 0u;
            const uint64_t mk = __ballot(bit);
            start += __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u)) << b;
            W += (uint32_t)__popcll(mk) << b;
            if (__ballot(top && bit) != 0ull) { nmax |= 1u << b; top = top && bit; }
        }
    };
    deal();
    if (W == 0u) return;
    if (((int)nmax - MRTX_TRIAL_WIDE_MIN) * 64 <= (int)W) {      // too few stragglers for a round's bookkeeping to pay
        step_loop_from<WIDE, false, STATS, false, 1>(f, m.oa, m.ob, m.oc, m.da, m.db, m.dc, 0.0f, sg, 0, j, pend, go, hit, sk_out, cnt);
        return;
    }
    // The list is cut into windows of 64 items.  Published once: every ray's state and (start, first pending step) under the ray's NUMBER
    // among the rays with steps pending, and a bitmap of the list positions where a ray's steps begin -- the number of bits at or below
    // an item's position is the number of the ray it belongs to.
    const uint64_t rays = __ballot(n > 0u);
    const uint32_t c = __builtin_amdgcn_mbcnt_hi((uint32_t)(rays >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rays, 0u));
    uint16_t* const c16 = reinterpret_cast<uint16_t*>(ctl);     // spare word i = ctl[4 i]; words 0-31: the bitmap, 32-63: 64 16-bit entries
    if (lane < 32u) ctl[lane * 4u] = 0u;
    xch_order();
    if (n > 0u) {
        const xch4 a = {sg.ra, sg.r1, sg.r2, sg.ca}, b = {sg.c1, sg.c2, m.oa, m.ob}, cc = {m.oc, m.da, m.db, m.dc};
        st[c] = a; st[64u + c] = b; st[128u + c] = cc;
        c16[(32u + (c >> 1)) * 8u + (c & 1u)] = (uint16_t)(start | ((uint32_t)j << 10));
        __hip_atomic_fetch_or(&ctl[(start >> 5) * 4u], 1u << (start & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    xch_order();
    const uint64_t lanes_le = (2ull << lane) - 1ull;
    uint32_t before = 0u;                                       // rays that begin below this window
    for (uint32_t base = 0u;; base += 64u) {
        const uint32_t h0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ctl[(base >> 5) * 4u]);
        const uint32_t h1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ctl[((base >> 5) + 1u) * 4u]);
        const uint64_t heads = ((uint64_t)h1 << 32) | h0;
        const uint32_t ci = (before + (uint32_t)__popcll(heads & lanes_le) - 1u) & 63u;      // window 0 begins with a ray: never negative
        const uint32_t t = base + lane;
        const uint32_t sj = c16[(32u + (ci >> 1)) * 8u + (ci & 1u)];
        const int jj = min((int)((sj >> 10) + (t - (sj & 1023u))), SEG_N);           // items past the end of the list stay inside the segment
#ifdef MRTX_PROF_TRIAL
        if (lane == 0u) { cnt[8] += 1u; cnt[9] += min(W - base, 64u); }              // wave-level: windows and the items in them
#endif
        const xch4 a = st[ci], b = st[64u + ci], cc = st[128u + ci];
        bool in, bel;
        trial_step<WIDE>(f, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, cc.x, cc.y, cc.z, cc.w, jj, in, bel);
        const uint64_t term = __ballot((t < W) & !(in & !bel)), inside = __ballot(in);
        if (pend && start < base + 64u) {
            // this ray's items in the window are the list positions [p0, p1): its first terminating one, if any
            const uint32_t p0 = start > base ? start - base : 0u, p1 = min(start + n - base, 64u);
            const uint64_t mine = term & ~((1ull << p0) - 1ull) & (p1 >= 64u ? ~0ull : (1ull << p1) - 1ull);
            if (mine != 0ull) {
                const uint32_t p = (uint32_t)__ffsll((long long)mine) - 1u;
                const int jt = j + (int)(base + p - start);
                hit = ((inside >> p) & 1ull) != 0ull;       // terminated inside: at or below the surface
                go = false;
                sk_out = (float)jt * f.step;
                if (STATS) { cnt[ST_FETCH] += (uint32_t)(jt - j + 1); cnt[ST_HEIGHT] += (uint32_t)(jt - j) + (hit ? 1u : 0u); }
                pend = false;
            } else if (start + n <= base + 64u) {           // through all its steps: inside and above the surface at each
                if (STATS) { cnt[ST_FETCH] += n; cnt[ST_HEIGHT] += n; }
                pend = false;
            }
        }
        if (__ballot(pend) == 0ull) break;
        before += (uint32_t)__popc(h0) + (uint32_t)__popc(h1);
    }
}

// Coarse march s_k = k*step, k = 1, 2, ...; returns true and s_k at the first sample at/below the surface.
// PRIMARY: stop when s_k > smax (left the bounding sphere); shadow rays: stop when r^2 > R^2.
// A lane drops out of the exec mask when it hits or leaves, and the wave leaves the loop when no lane is still
// marching.  f.kmax is a multiple of SEG_N.  BOUNDED (shadow rays): the steps end before s_k >= smax as well.
template <bool WIDE, bool PRIMARY, bool STATS, int BATCH, int SCAN = PRIMARY ? 1 : 0, bool BOUNDED = false>
__device__ __forceinline__ bool march(const FrameC& f, float oa, float ob, float oc, float da, float db, float dc,
                                      float smax, Seg& sg, float& sk_hit, uint32_t* cnt) {
    MarchState m;
    bool hit = false;
    bool go = march_begin<PRIMARY, STATS, false, BOUNDED>(f, oa, ob, oc, da, db, dc, m, cnt, smax);
    while (go) march_segment<WIDE, PRIMARY, STATS, BATCH, SCAN, BOUNDED>(f, m, smax, sg, go, hit, sk_hit, cnt);
    return hit;
}

// D3 refinement: nbis bisections of (lo, hi) on below().  (Two levels per round -- the three mid-points evaluated
// together, 3 dependent rounds instead of 5 -- measured no faster: 13.90 vs 13.85 ms.)
template <bool WIDE>
__device__ __forceinline__ void refine(const FrameC& f, const Seg& sg, float oa, float ob, float oc, float da, float db,
                                       float dc, float& lo, float& hi) {
    auto below = [&](float s) {
        const float ma = fmaf(s, da, oa), mb = fmaf(s, db, ob), mc = fmaf(s, dc, oc);
        return below_seg<WIDE, true>(f, sg, s, ma, mb, mc, fmaf(mc, mc, fmaf(mb, mb, ma * ma)));
    };
    for (int i = 0; i < f.nbis; i++) {
        const float mid = 0.5f * (lo + hi);
        const bool bel = below(mid);
        hi = bel ? mid : hi;
        lo = bel ? lo : mid;
    }
}

struct Vertex {
    float pa, pb, pc;      // surface point (moon frame)
    float na, nb, nc;      // unit normal
    float al0, al1, al2;   // reflectance
};

// Duff et al., "Building an Orthonormal Basis, Revisited"
__device__ __forceinline__ void duff_basis(float na, float nb, float nc, float& b1a, float& b1b, float& b1c, float& b2a,
                                           float& b2b, float& b2c) {
    const float sg = nc >= 0.0f ? 1.0f : -1.0f;
    const float aa = -rcp_cr(sg + nc);       // |sg + nc| in [1, 2]; -(1/x) == (-1)/x bit for bit
    const float bb = (na * nb) * aa;
    b1a = fmaf(sg, (na * na) * aa, 1.0f); b1b = sg * bb; b1c = -sg * na;
    b2a = bb; b2b = fmaf(nb * nb, aa, sg); b2c = -nb;
}

// surface point -> normal (central differences of D one texel either side of it) and albedo (D4)
template <bool STATS, bool WIDE>
__device__ __forceinline__ void hit_vertex(const FrameC& f, float ha, float hb, float hc, Vertex& v, uint32_t* cnt) {
    const float rho2 = fmaf(hb, hb, ha * ha);
    const float r2 = fmaf(hc, hc, rho2);
    const float rho = sqrt_sh(rho2);         // only used through rhoc = max(rho, 1e-6): a rho2 below 2^-104 cannot matter
    const float r = sqrt_sh(r2);             // r2 ~ R^2
    float lat, lon;
    latlon(ha, hb, hc, rho2, lat, lon);
    const float rowf = fmaf(lat, f.gd.row_scale, f.gd.row_off);
    const float colf = fmaf(lon, f.gd.col_scale, f.gd.col_off);
    // the two-texel border makes the +-1 texel taps plain two-load evaluations as well
    const float dn = dem_march<WIDE>(f, rowf - 1.0f, colf);
    const float ds = dem_march<WIDE>(f, rowf + 1.0f, colf);
    const float de = dem_march<WIDE>(f, rowf, colf + 1.0f);
    const float dw = dem_march<WIDE>(f, rowf, colf - 1.0f);
    if (STATS) { cnt[ST_HEIGHT] += 4; cnt[ST_FETCH] += 4; }
    const float dlat = (dn - ds) * CF(f)->dlat_scale;
    const float dlon = (de - dw) * CF(f)->dlon_scale;
    const float rhoc = rho > 1.0e-6f ? rho : 1.0e-6f;
    const float inv_r = rcp_cr(r), inv_rho = rcp_cr(rhoc);   // r ~ R, rhoc in [1e-6, R]
    const float sphi = hc * inv_r, cphi = rhoc * inv_r;
    const float slam = ha * inv_rho, clam = hb * inv_rho;
    const float glat = (f.Rf * inv_r) * dlat;
    const float glon = (f.Rf * inv_rho) * dlon;
    const float na = fmaf(-glon, clam, fmaf(glat, sphi * slam, ha * inv_r));
    const float nb = fmaf(glon, slam, fmaf(glat, sphi * clam, hb * inv_r));
    const float nc = fmaf(-glat, cphi, hc * inv_r);
    const float inv_nl = rcp_cr(sqrt_sh(fmaf(nc, nc, fmaf(nb, nb, na * na))));   // |n|^2 >= ~1 (unit radial part + gradient)
    v.pa = ha; v.pb = hb; v.pc = hc;
    v.na = na * inv_nl; v.nb = nb * inv_nl; v.nc = nc * inv_nl;
    if (CF(f)->color) {  // D4: bilinear RGBA8
        const float rc = fmaf(lat, CF(f)->gc.row_scale, CF(f)->gc.row_off);
        const float cc = fmaf(lon, CF(f)->gc.col_scale, CF(f)->gc.col_off);
        GridC gcl;   // scalar-load the colour grid constants (member-wise: no copy constructor across address spaces)
        gcl.h = CF(f)->gc.h; gcl.w = CF(f)->gc.w; gcl.row_scale = CF(f)->gc.row_scale; gcl.row_off = CF(f)->gc.row_off;
        gcl.col_scale = CF(f)->gc.col_scale; gcl.col_off = CF(f)->gc.col_off; gcl.wf = CF(f)->gc.wf;
        // row-pair layout as for the DEM (color_pair_kernel): element (r, c) = (T[max(r,0)][wrap(c)], T[min(r+1,h-1)][wrap(c)])
        // for r in [-1, h-1], c in [-2, w+1]: the 2x2 RGBA8 footprint is one 16-byte load instead of four gathers
        const float rfl = floorf(rc), cfl = floorf(cc);
        int32_t r0 = (int32_t)rfl, c0 = (int32_t)cfl;
        r0 = r0 < -1 ? -1 : (r0 > gcl.h - 1 ? gcl.h - 1 : r0);
        c0 = c0 < -2 ? -2 : (c0 > gcl.w ? gcl.w : c0);
        const float tfr = rc - rfl, tfc = cc - cfl;
        const uint64_t ci = (uint64_t)(uint32_t)(r0 + 1) * (uint64_t)(uint32_t)(gcl.w + 4) + (uint64_t)(uint32_t)(c0 + 2);
        const UQuad cq = *reinterpret_cast<const UQuad*>(reinterpret_cast<const char*>(CF(f)->color) + (ci << 3));
        const uint32_t p00 = cq.a, p10 = cq.b, p01 = cq.c, p11 = cq.d;
        v.al0 = lerp2((float)(p00 & 255u), (float)(p01 & 255u), (float)(p10 & 255u), (float)(p11 & 255u), tfr, tfc) * kInv255;
        v.al1 = lerp2((float)((p00 >> 8) & 255u), (float)((p01 >> 8) & 255u), (float)((p10 >> 8) & 255u),
                      (float)((p11 >> 8) & 255u), tfr, tfc) * kInv255;
        v.al2 = lerp2((float)((p00 >> 16) & 255u), (float)((p01 >> 16) & 255u), (float)((p10 >> 16) & 255u),
                      (float)((p11 >> 16) & 255u), tfr, tfc) * kInv255;
        if (STATS) cnt[ST_COLOUR]++;
    } else {
        v.al0 = CF(f)->const_albedo[0]; v.al1 = CF(f)->const_albedo[1]; v.al2 = CF(f)->const_albedo[2];
    }
}

// D5's light constants (Lb, rL2, rad2) as light_sample and illum_mu read them: the frame's cold block (every render kernel,
// illum_kernel: scalar loads where the code uses them), or one epoch's, held in registers (illum_series_kernel)
struct FrameLight {
    const FrameC& f;
    __device__ __forceinline__ float Lb(int i) const { return CF(f)->Lb[i]; }
    __device__ __forceinline__ float rL2() const { return CF(f)->rL2; }
    __device__ __forceinline__ float rad2() const { return CF(f)->rad2; }
};
struct EpochLight {
    float lb[3], rl2, r2;
    __device__ __forceinline__ float Lb(int i) const { return lb[i]; }
    __device__ __forceinline__ float rL2() const { return rl2; }
    __device__ __forceinline__ float rad2() const { return r2; }
};

// D5: one sample of the spherical light from a vertex: the shadow ray (origin lifted by scene_epsilon, direction
// uniform in the cone the light subtends) and what it carries if it arrives, radiance * solid angle / pi * cos(theta_i);
// false when the sampled direction lies below the surface (no shadow ray, no contribution).
template <class L>
__device__ __forceinline__ bool light_sample(const FrameC& f, const L& lt, const Vertex& v, float u2, float u3, float& oa,
                                             float& ob, float& oc, float& wa, float& wb, float& wc, float& carried) {
    const float eps = CF(f)->scene_eps;
    oa = fmaf(eps, v.na, v.pa); ob = fmaf(eps, v.nb, v.pb); oc = fmaf(eps, v.nc, v.pc);
    const float ta = lt.Lb(0) - oa, tb = lt.Lb(1) - ob, tc = lt.Lb(2) - oc;
    const float d2 = fmaf(tc, tc, fmaf(tb, tb, ta * ta));
    const float inv_dist = rcp_cr(sqrt_sh(d2));   // distance to the light: ~2e4 R
    const float la = ta * inv_dist, lb = tb * inv_dist, lc = tc * inv_dist;
    float sin2 = lt.rL2() * (inv_dist * inv_dist);
    if (sin2 > 1.0f) sin2 = 1.0f;
    const float cosmax = sqrt_sh(1.0f - sin2);     // 0 or >= 2^-24
    const float omc = sin2 / (1.0f + cosmax);
    const float av = u2 * omc;
    const float cost = 1.0f - av;
    const float sint = sqrt_sh(av * (2.0f - av));  // 0 (u2 = 0 or a point light) or >= ~2^-24 * omc
    float cph, sph;
    sincos_turn(u3, cph, sph);
    float b1a, b1b, b1c, b2a, b2b, b2c;
    duff_basis(la, lb, lc, b1a, b1b, b1c, b2a, b2b, b2c);
    const float ca = sint * cph, sa = sint * sph;
    wa = fmaf(cost, la, fmaf(sa, b2a, ca * b1a));
    wb = fmaf(cost, lb, fmaf(sa, b2b, ca * b1b));
    wc = fmaf(cost, lc, fmaf(sa, b2c, ca * b1c));
    const float cosi = fmaf(v.nc, wc, fmaf(v.nb, wb, v.na * wa));
    carried = (lt.rad2() * omc) * cosi;
    return cosi > 0.0f;
}
// the frame's light (every caller but illum_series_kernel)
__device__ __forceinline__ bool light_sample(const FrameC& f, const Vertex& v, float u2, float u3, float& oa, float& ob,
                                             float& oc, float& wa, float& wb, float& wc, float& carried) {
    return light_sample(f, FrameLight{f}, v, u2, u3, oa, ob, oc, wa, wb, wc, carried);
}

}  // namespace mrtx
