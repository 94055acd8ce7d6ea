// mrtx_terrain.hip -- gfx950 kernels of the terrain-query stage: what the Sun, the Earth and the terrain itself do at points of
// the surface, marched through the same height field as the camera's rays (the march core, mrtx_march.h).
//
//   illum_kernel, illum_series_kernel       Sun illumination of nodes and points, one frame or a series of epochs
//   horizon_kernel, horizon_raised_kernel   terrain horizon profiles, from the ground or from a mast (3.8, 3.15)
//   horizon_sun_kernel                      the Sun's visible fraction per epoch against a horizon, and its statistics (3.8)
//   horizon_windows_kernel                  joint Sun / Earth windows (3.15)
//   horizon_mask_kernel                     the joint predicate as bits: drive masks (3.19)
//   power_budget_kernel                     energy-storage need and state of charge (3.17)
//   occultation_kernel                      the Earth's occultation of the Sun (3.18)
//   passes_full_kernel, passes_summary_kernel, passes_list_kernel   orbiter passes against the horizons (3.27)
//   thermal_kernel                          regolith temperatures and subsurface columns (3.9, 3.11, 3.16, 3.18)
//   view_hits_kernel, view_share_kernel, scatter_flux_kernel   terrain-scattered sunlight and infrared (3.11)
//   sight_kernel                            line of sight, viewsheds, mast heights (3.12)
// and their launch wrappers (called from mrtx_api.hip).
//
// Own translation unit: an edit here recompiles none of the camera and path kernels of mrtx_kernels.hip, and the other way
// round.  The kernels stay in namespace mrtx, so their names are what they were.  Build flags as there (-ffp-contract=off,
// correctly rounded /).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "mrtx_device.h"
#include "mrtx_march.h"

namespace mrtx {

// ------------------------------------------------------------------------------------------------
// Sun illumination of the terrain (DESIGN.md sections 3.6 and 4.8): per node of a lat/lon band or a point list, the vertex
// of the camera path's first hit (hit_vertex at p = R D(node) u) and n_sun light samples of the fixed table marched like its
// shadow ray (light_sample + march, the body of direct_light with the visibility kept apart from what a sample carries).
// One wave = 64/n adjacent nodes x n samples in adjacent lanes (render_kernel's idea: the lanes march from nearly one point in
// nearly one direction).  Tried and retired (DESIGN.md sections 4.8 and 4.18; profiles/illum_a_summary.md): lane = node, the samples
// in a loop -- the same bits, the whole-Moon map 8.7 ms against 4.6.
// (sum over the n lanes of a node, the pairwise order of tree_sum<n>) for a run-time n
__device__ __forceinline__ float group_sum(float v, int n) {
    for (int m = 1; m < n; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// The counters of the terrain kernels: each lane counts into its own zeroed cnt[ST_N]; at the end the wave's sums of four of
// them -- `first` (ST_SHADOW, or ST_BOUNCE for view rays), ST_HEIGHT, ST_FETCH, ST_MIP -- go to the stats block from lane 0.
template <bool STATS>
__device__ __forceinline__ void stage_flush(const FrameC& f, const uint32_t* cnt, int first, int lane) {
    if (!STATS) return;
    const int which[4] = {first, ST_HEIGHT, ST_FETCH, ST_MIP};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t c = cnt[which[i]];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) c += __shfl_xor(c, m, 64);
        if (lane == 0) atomicAdd(&CF(f)->stats[which[i]], (unsigned long long)c);
    }
}
// A point's local frame from its table entries, U = u, E = (c_lon, -s_lon, 0) from ct = (s_lon, c_lon) and
// N = (-s_lat s_lon, -s_lat c_lon, c_lat), and the lifted origin o = fmaf(scene_eps, n, p) of its vertex v (light_sample's)
struct PointFrame {
    float ua, ub, uc, Na, Nb, Nc, oa, ob, oc;
    float2 ct;
};
__device__ __forceinline__ PointFrame point_frame(const FrameC& f, const IllumC& g, int row, int col, const Vertex& v) {
    const float2 rt = reinterpret_cast<const float2*>(g.rtab)[g.points ? col : row];   // (s_lat, c_lat)
    const float2 ct = reinterpret_cast<const float2*>(g.ctab)[col];                    // (s_lon, c_lon)
    const float eps = CF(f)->scene_eps;
    return {rt.y * ct.x, rt.y * ct.y, rt.x, -(rt.x * ct.x), -(rt.x * ct.y), rt.y,
            fmaf(eps, v.na, v.pa), fmaf(eps, v.nb, v.pb), fmaf(eps, v.nc, v.pc), ct};
}
// the node's surface vertex and D (what every sample of the node shares)
template <bool STATS, bool WIDE>
__device__ __forceinline__ float illum_vertex(const FrameC& f, const IllumC& g, int row, int col, Vertex& v, uint32_t* cnt) {
    const float2 rt = reinterpret_cast<const float2*>(g.rtab)[g.points ? col : row];
    const float2 ct = reinterpret_cast<const float2*>(g.ctab)[col];
    const float ua = rt.y * ct.x, ub = rt.y * ct.y, uc = rt.x;     // (cos lat sin lon, cos lat cos lon, sin lat)
    float lat, lon;
    latlon(ua, ub, uc, fmaf(ub, ub, ua * ua), lat, lon);
    const float D = dem_march<WIDE>(f, fmaf(lat, f.gd.row_scale, f.gd.row_off), fmaf(lon, f.gd.col_scale, f.gd.col_off));
    if (STATS) { cnt[ST_HEIGHT]++; cnt[ST_FETCH]++; }
    const float rD = f.Rf * D;
    hit_vertex<STATS, WIDE>(f, rD * ua, rD * ub, rD * uc, v, cnt);
    return D;
}
// mu = n . l toward the light centre, l formed as light_sample forms it from the lifted origin
template <class L>
__device__ __forceinline__ float illum_mu(const FrameC& f, const L& lt, const Vertex& v) {
    const float eps = CF(f)->scene_eps;
    const float oa = fmaf(eps, v.na, v.pa), ob = fmaf(eps, v.nb, v.pb), oc = fmaf(eps, v.nc, v.pc);
    const float ta = lt.Lb(0) - oa, tb = lt.Lb(1) - ob, tc = lt.Lb(2) - oc;
    const float inv_dist = rcp_cr(sqrt_sh(fmaf(tc, tc, fmaf(tb, tb, ta * ta))));
    return fmaf(v.nc, tc * inv_dist, fmaf(v.nb, tb * inv_dist, v.na * (ta * inv_dist)));
}
// one light sample: true if it arrives (cos > 0 and the shadow ray escapes); `carried` = what it carries then
template <bool STATS, bool WIDE, class L>
__device__ __forceinline__ bool illum_sample(const FrameC& f, const L& lt, const Vertex& v, float u2, float u3, float& carried,
                                             uint32_t* cnt) {
    float oa, ob, oc, wa, wb, wc;
    if (!light_sample(f, lt, v, u2, u3, oa, ob, oc, wa, wb, wc, carried)) return false;
    if (STATS) cnt[ST_SHADOW]++;
    Seg ssg;
    float sk_occ;
    return !march<WIDE, false, STATS, MRTX_STEP_BATCH, 2>(f, oa, ob, oc, wa, wb, wc, 0.0f, ssg, sk_occ, cnt);
}

template <bool STATS, bool WIDE>
__global__ void __launch_bounds__(64) illum_kernel(const FrameC f, const IllumC g) {
    const int lane = threadIdx.x;
    const int n = g.n_sun;
    const int s = lane & (n - 1), p = lane >> g.n_log2;
    // the wave's node block: PW x PH nodes in raster order
    const int pw = 1 << g.pw_log2;
    const int wx = (int)(blockIdx.x % (unsigned)g.waves_x), wy = (int)(blockIdx.x / (unsigned)g.waves_x);
    const int col = wx * pw + (p & (pw - 1));
    const int row = wy * ((64 >> g.n_log2) >> g.pw_log2) + (p >> g.pw_log2);
    const bool in = row < g.rows && col < g.cols;
    uint32_t cnt_store[STATS ? ST_N : 1] = {};
    uint32_t* const cnt = STATS ? cnt_store : nullptr;
    float lit = 0.0f, irr = 0.0f, mu = 0.0f, D = 0.0f;
    if (in) {
        Vertex v;
        D = illum_vertex<STATS, WIDE>(f, g, row, col, v, cnt);
        mu = illum_mu(f, FrameLight{f}, v);
        const float2* sun = reinterpret_cast<const float2*>(g.sun);
        const float2 us = sun[s];
        float carried;
        if (illum_sample<STATS, WIDE>(f, FrameLight{f}, v, us.x, us.y, carried, cnt)) { lit = 1.0f; irr = carried; }
    }
    lit = group_sum(lit, n);    // a count: exact
    irr = group_sum(irr, n);
    const float inv_n = 1.0f / (float)n;   // a power of two: the scalings below are exact
    if (in && s == 0)
        reinterpret_cast<float4*>(g.out)[(int64_t)row * g.cols + col] = make_float4(lit * inv_n, irr * inv_n, mu, D);
    stage_flush<STATS>(f, cnt, ST_SHADOW, lane);
}

// Sun illumination over many dates (DESIGN.md sections 3.7 and 4.9): entry (point, j) of a series is illum_kernel's output at
// the point under epoch first[point] + j, whose light constants come from a table instead of the cold block.  One wave = 64/n
// (point, epoch) pairs x n samples in adjacent lanes, laid out as illum_kernel's node block with points as rows and the
// epochs of a window as columns: 64/n consecutive epochs of one point (the Sun moves ~0.085 deg in 10 minutes, a third of
// its radius: the lanes march from one origin in nearly one direction), or several points when the window is shorter.
template <bool STATS, bool WIDE>
__global__ void __launch_bounds__(64) illum_series_kernel(const FrameC f, const IllumSeriesC q) {
    const IllumC& g = q.g;
    const int lane = threadIdx.x;
    const int n = g.n_sun;
    const int s = lane & (n - 1), p = lane >> g.n_log2;
    const int pw = 1 << g.pw_log2;
    const int wx = (int)(blockIdx.x % (unsigned)g.waves_x), wy = (int)(blockIdx.x / (unsigned)g.waves_x);
    const int j = wx * pw + (p & (pw - 1));                                         // epoch within the window
    const int pt = wy * ((64 >> g.n_log2) >> g.pw_log2) + (p >> g.pw_log2);         // point
    const bool in = pt < g.rows && j < g.cols;
    uint32_t cnt_store[STATS ? ST_N : 1] = {};
    uint32_t* const cnt = STATS ? cnt_store : nullptr;
    float lit = 0.0f, irr = 0.0f, mu = 0.0f, D = 0.0f;
    if (in) {
        const int64_t k = (int64_t)(q.first ? q.first[pt] : 0) + j;
        const float4 l0 = reinterpret_cast<const float4*>(q.lights)[2 * k];
        const float4 l1 = reinterpret_cast<const float4*>(q.lights)[2 * k + 1];
        const EpochLight lt{{l0.x, l0.y, l0.z}, l0.w, l1.x};
        Vertex v;
        D = illum_vertex<STATS, WIDE>(f, g, pt, pt, v, cnt);      // g.points = 1: both tables indexed by the point
        mu = illum_mu(f, lt, v);
        const float2 us = reinterpret_cast<const float2*>(g.sun)[s];
        float carried;
        if (illum_sample<STATS, WIDE>(f, lt, v, us.x, us.y, carried, cnt)) { lit = 1.0f; irr = carried; }
    }
    lit = group_sum(lit, n);    // a count: exact
    irr = group_sum(irr, n);
    const float inv_n = 1.0f / (float)n;   // a power of two: the scalings below are exact
    if (in && s == 0)
        reinterpret_cast<float4*>(g.out)[(int64_t)pt * g.cols + j] = make_float4(lit * inv_n, irr * inv_n, mu, D);
    stage_flush<STATS>(f, cnt, ST_SHADOW, lane);
}

// Terrain horizons (DESIGN.md sections 3.8 and 4.10): per (point, azimuth) a bisection over the elevation whose n_bis probes
// are each exactly an illumination sample's visibility decision -- n . d > 0 and the shadow march from the lifted origin
// escapes (light_sample's origin, illum_sample's march).  Lane = (point, azimuth), point-major: one wave = 64 consecutive
// azimuths of one point (64 / n_az points when n_az < 64), so the 64 lanes leave one origin.  Steep probes end after a few
// steps; the last probes graze the horizon and run the length of the bounding shell.
// RAISED (DESIGN.md sections 3.15 and 4.16, horizon_raised_kernel): point pt marches from sight_end(p, hs[pt]).  hs == 0 is
// the plain probe, bit for bit; hs > 0 drops the facet test (a mast top sees below its facet's plane) and, when the raised
// origin lies outside the bounding sphere, marches from where the probe enters it, as sight_probe does (clear when it heads
// away from the sphere or misses it).  RAISED = false compiles to the kernel as it was.
__device__ __forceinline__ void sight_end(const PointFrame& p, float hs, float& Pa, float& Pb, float& Pc);
template <bool STATS, bool WIDE, bool RAISED>
__device__ __forceinline__ void horizon_body(const FrameC& f, const HorizonC& h, const float* hs_tab) {
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * 64 + lane;
    const int n_az = 1 << h.az_log2;
    const int pt = (int)(gid >> h.az_log2), az = (int)(gid & (int64_t)(n_az - 1));
    const bool in = pt < h.g.rows;
    uint32_t cnt_store[STATS ? ST_N : 1] = {};
    uint32_t* const cnt = STATS ? cnt_store : nullptr;
    if (in) {
        Vertex v;
        (void)illum_vertex<STATS, WIDE>(f, h.g, pt, pt, v, cnt);    // g.points = 1: both tables indexed by the point
        const PointFrame p = point_frame(f, h.g, pt, pt, v);
        float cp, sp;
        sincos_turn((float)az * (1.0f / (float)n_az), cp, sp);     // a / n_az: exact
        const float ha = fmaf(cp, p.Na, sp * p.ct.y), hb = fmaf(cp, p.Nb, -(sp * p.ct.x)), hc = cp * p.Nc;
        // the march origin: the lifted origin, or the mast top above it; q0 > R^2: that one lies outside the bounding sphere
        const float hs = RAISED ? hs_tab[pt] : 0.0f;
        const bool up = RAISED && hs > 0.0f;
        float Oa = p.oa, Ob = p.ob, Oc = p.oc;
        if (up) sight_end(p, hs, Oa, Ob, Oc);
        const float q0 = RAISED ? fmaf(Oc, Oc, fmaf(Ob, Ob, Oa * Oa)) : 0.0f;
        const bool outside = up && q0 > f.R2f;
        float lo = 0.0f, hi = 1.0f;
        for (int i = 0; i < h.n_bis; i++) {
            const float mid = 0.5f * (lo + hi);                     // dyadic, at most 24 fraction bits: exact
            float ce, se;
            sincos_turn((mid - 0.5f) * 0.5f, ce, se);               // e in (-1/4, 1/4) turn: quadrants -1 and 0
            const float da = fmaf(se, p.ua, ce * ha), db = fmaf(se, p.ub, ce * hb), dc = fmaf(se, p.uc, ce * hc);
            bool clear = false;
            if (up || fmaf(v.nc, dc, fmaf(v.nb, db, v.na * da)) > 0.0f) {
                if (STATS) cnt[ST_SHADOW]++;
                float oa = Oa, ob = Ob, oc = Oc;
                bool meets = true;
                if (outside) {
                    const float b = fmaf(Oc, dc, fmaf(Ob, db, Oa * da));
                    const float c = q0 - f.R2f;
                    const float disc = fmaf(b, b, -c);
                    meets = b < 0.0f && disc >= 0.0f;              // heads for the sphere and meets it
                    if (meets) {
                        const float s_in = c / (sqrtf(disc) - b);   // the nearer root of s^2 + 2 b s + c, without cancellation
                        oa = fmaf(s_in, da, Oa); ob = fmaf(s_in, db, Ob); oc = fmaf(s_in, dc, Oc);
                    }
                }
                clear = true;
                if (meets) {
                    Seg ssg;
                    float sk_occ;
                    clear = !march<WIDE, false, STATS, MRTX_STEP_BATCH, 2>(f, oa, ob, oc, da, db, dc, 0.0f, ssg, sk_occ, cnt);
                }
            }
            hi = clear ? mid : hi;
            lo = clear ? lo : mid;
        }
        h.out[gid] = (hi - 0.5f) * 180.0f;
    }
    stage_flush<STATS>(f, cnt, ST_SHADOW, lane);
}
template <bool STATS, bool WIDE>
__global__ void __launch_bounds__(64) horizon_kernel(const FrameC f, const HorizonC h) {
    horizon_body<STATS, WIDE, false>(f, h, nullptr);
}
template <bool STATS, bool WIDE>
__global__ void __launch_bounds__(64) horizon_raised_kernel(const FrameC f, const HorizonRaisedC q) {
    horizon_body<STATS, WIDE, true>(f, q.h, q.hs);
}

// The visible share of the light's disc above a point's horizon, from the epoch's (Lb.xyz, rL2) l0,
// the point's frame p (its lifted origin, U, N and E) and its horizon row hz of n_az samples.  (la, lb, lc): the unit
// direction to the light centre as light_sample forms it (illum_mu's l).
__device__ __forceinline__ float disc_fraction(const float4 l0, const PointFrame& p, const float* hz, int n_az, float& la,
                                               float& lb, float& lc) {
    constexpr float kDeg = 57.2957795130823209f, kInvTurn = 0.159154943091895336f, kInvPi = 0.318309886183790672f;
    const float ta = l0.x - p.oa, tb = l0.y - p.ob, tc = l0.z - p.oc;
    const float inv_dist = rcp_cr(sqrt_sh(fmaf(tc, tc, fmaf(tb, tb, ta * ta))));
    la = ta * inv_dist; lb = tb * inv_dist; lc = tc * inv_dist;
    const float xu = fmaf(p.uc, lc, fmaf(p.ub, lb, p.ua * la));
    const float xn = fmaf(p.Nc, lc, fmaf(p.Nb, lb, p.Na * la));
    const float xe = fmaf(-p.ct.x, lb, p.ct.y * la);
    const float es = atan2f(xu, sqrtf(fmaf(xe, xe, xn * xn))) * kDeg;
    float ph = atan2f(xe, xn) * kInvTurn;                   // turns from north through east, [-1/2, 1/2]
    ph = ph < 0.0f ? ph + 1.0f : ph;
    const float x = ph * (float)n_az;
    const float x0 = floorf(x);
    const float w = x - x0;
    const int i0 = (int)x0 & (n_az - 1), i1 = (i0 + 1) & (n_az - 1);
    const float h0 = hz[i0], h1 = hz[i1];
    const float hh = fmaf(w, h1 - h0, h0);
    const float alpha = asinf(fminf(1.0f, sqrtf(l0.w) * inv_dist)) * kDeg;
    float fr = 0.0f;
    if (alpha > 0.0f) {
        const float r = (hh - es) / alpha;
        if (r <= -1.0f) fr = 1.0f;
        else if (r < 1.0f) fr = fminf(1.0f, fmaxf(0.0f, (acosf(r) - r * sqrtf(1.0f - r * r)) * kInvPi));
    } else {
        fr = es > hh ? 1.0f : 0.0f;
    }
    return fr;
}

// The share g of a source's disc that a body's disc leaves uncovered, from the epoch's (Lb.xyz, rL2)
// of the source ls and of the body lb and the point's frame p (its lifted origin).  Both unit directions and both angular
// radii (radians) as disc_fraction forms them; the separation from atan2f of |a x b| and a . b (acosf of the dot product keeps
// no digit at a third of a degree); then the planar two-disc rule.  In the lens the half-angles acos(x) and acos(y) are taken as
// atan2f(K, x's numerator) and atan2f(K, y's numerator), K = 2 sep alpha_s sin = the square root of the four-factor product:
// the same angles, but formed from the factored gap, so that they go to 0 at a contact as fast as the gap does (acosf of the
// quotient keeps half the digits there, and the area is a difference of terms (alpha_b / alpha_s)^2 = 13 solar discs large).
__device__ __forceinline__ float occult_fraction(const float4 ls, const float4 lb, const PointFrame& p) {
    const float sa = ls.x - p.oa, sb = ls.y - p.ob, sc = ls.z - p.oc;
    const float inv_s = rcp_cr(sqrt_sh(fmaf(sc, sc, fmaf(sb, sb, sa * sa))));
    const float ax = sa * inv_s, ay = sb * inv_s, az = sc * inv_s;
    const float ta = lb.x - p.oa, tb = lb.y - p.ob, tc = lb.z - p.oc;
    const float inv_b = rcp_cr(sqrt_sh(fmaf(tc, tc, fmaf(tb, tb, ta * ta))));
    const float bx = ta * inv_b, by = tb * inv_b, bz = tc * inv_b;
    const float as = asinf(fminf(1.0f, sqrtf(ls.w) * inv_s));
    const float ab = asinf(fminf(1.0f, sqrtf(lb.w) * inv_b));
    const float cx = fmaf(ay, bz, -(az * by)), cy = fmaf(az, bx, -(ax * bz)), cz = fmaf(ax, by, -(ay * bx));
    const float sep = atan2f(sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx))), fmaf(az, bz, fmaf(ay, by, ax * bx)));
    if (!(as > 0.0f)) return sep > ab ? 1.0f : 0.0f;               // a point source: a step
    if (sep >= as + ab) return 1.0f;                                // apart
    if (ab >= as) { if (sep <= ab - as) return 0.0f; }              // total
    else if (sep <= as - ab) { const float r = ab / as; return 1.0f - r * r; }     // annular
    const float K = sqrtf(fmaxf(0.0f, ((as + ab - sep) * (sep + as - ab)) * ((sep - as + ab) * (sep + as + ab))));
    const float s2 = sep * sep, as2 = as * as, ab2 = ab * ab;
    const float d2 = as2 - ab2;
    const float A = fmaf(as2, atan2f(K, s2 + d2), ab2 * atan2f(K, s2 - d2)) - 0.5f * K;
    return fminf(1.0f, fmaxf(0.0f, 1.0f - A / (kPi * as2)));
}

// Runs of set epochs, followed by the epoch walkers (horizon_sun_kernel, horizon_windows_kernel, occultation_kernel) across
// their 64-epoch chunks, lane = epoch.  occultation_kernel calls run_ending_here and wave_max and keeps what it carries in
// plain variables: with EpochRuns its year SUMMARY measured 2 % slower (profiles/epoch_walk_helpers.md).
// the run of set epochs that ends at this lane's epoch (0 if it is not set): back to the nearest unset epoch of the chunk, or
// through the chunk's start into the run `cur` carried in.  set holds no lane past the last epoch.
__device__ __forceinline__ int run_ending_here(unsigned long long set, int lane, bool in, int cur) {
    const unsigned long long below = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const unsigned long long brk = ~set & below;
    const int run = brk ? lane - (63 - __clzll((long long)brk)) : lane + 1 + cur;
    return in ? run : 0;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = max(v, __shfl_xor(v, s, 64));
    return v;
}
// What a walker carries from chunk to chunk for one mask, all of it wave-uniform: `cur`, the run that reaches the previous
// chunk's last epoch (it continues into the next chunk); `best`, the longest run so far; `first`, the first epoch of the
// earliest run of that length (longest_first only; -1 while there is none).  `last` is the chunk's last valid lane.
struct EpochRuns {
    int cur = 0, best = 0, first = -1;
    __device__ __forceinline__ int step(unsigned long long set, int lane, bool in, int last) {
        const int run = run_ending_here(set, lane, in, cur);
        cur = __shfl(run, last, 64);
        return run;
    }
    __device__ __forceinline__ void longest(unsigned long long set, int lane, bool in, int last) {
        best = max(best, wave_max(step(set, lane, in, last)));
    }
    // a later run of the same length does not replace the first: the lowest lane that ends a run of mx ends the earliest
    __device__ __forceinline__ void longest_first(unsigned long long set, int lane, bool in, int last, int k0) {
        const int run = step(set, lane, in, last);
        const int mx = wave_max(run);
        if (mx > best) {
            const unsigned long long at = __ballot(run == mx);
            best = mx;
            first = k0 + (int)__builtin_ctzll(at) - mx + 1;
        }
    }
};

// The Sun against a horizon (DESIGN.md sections 3.9 and 4.10): per (point, epoch) the share of the light's disc above the
// point's horizon, interpolated at the light's azimuth.  One wave = one point; it walks the epochs 64 at a time (lane = epoch),
// so the point's vertex is formed once and its horizon row stays in L1.  FULL writes every fraction; SUMMARY reduces them in
// the wave: the sum in float64 (per lane over its epochs k = lane mod 64 in order, then the xor butterfly), the two counts, and
// the longest run of dark epochs carried from chunk to chunk (the run that reaches a chunk's last epoch continues into the next).
template <bool WIDE>
__global__ void __launch_bounds__(64) horizon_sun_kernel(const FrameC f, const HorizonSunC q) {
    const int lane = threadIdx.x;
    const int pt = (int)blockIdx.x;
    const int n_az = 1 << q.az_log2;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const lights = reinterpret_cast<const float4*>(q.lights);
    double sum = 0.0;
    uint32_t n_lit = 0, n_full = 0;
    EpochRuns dark;             // the runs of dark epochs
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < q.m;
        float fr = 0.0f;
        if (in) {
            float la, lb, lc;
            fr = disc_fraction(lights[2 * (int64_t)k], p, hz, n_az, la, lb, lc);
            if (q.mode == 0) q.out[(int64_t)pt * q.m + k] = fr;
        }
        if (q.mode != 0) {
            sum += (double)fr;
            n_lit += (in && fr > 0.0f) ? 1u : 0u;
            n_full += (in && fr == 1.0f) ? 1u : 0u;
            dark.longest(__ballot(in && fr == 0.0f), lane, in, min(64, q.m - k0) - 1);
        }
    }
    if (q.mode != 0) {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            sum += __shfl_xor(sum, s, 64);
            n_lit += __shfl_xor(n_lit, s, 64);
            n_full += __shfl_xor(n_full, s, 64);
        }
        if (lane == 0) {
            const double inv_m = 1.0 / (double)q.m;
            reinterpret_cast<float4*>(q.out)[pt] =
                make_float4((float)(sum * inv_m), (float)((double)n_lit * inv_m), (float)((double)n_full * inv_m), (float)dark.best);
        }
    }
}

// Joint windows of two bodies against one set of horizons (DESIGN.md sections 3.15 and 4.16): horizon_sun_kernel's walk -- one
// wave per point, the epochs 64 at a time, the vertex and frame once, the horizon row in L1 -- with disc_fraction evaluated for
// both epoch tables and three masks (ok_a, ok_b, both) reduced in the wave: their counts from the ballots' popcounts, and four
// runs (!ok_a, !ok_b, both, !both) by horizon_sun_kernel's scheme, the run that reaches a chunk's end carried into the next.
// Everything carried is wave-uniform; the first epoch of the longest `both` run is kept with it (a later run of the same length
// does not replace it).  No atomics, no LDS; lane 0 stores the point's two float4.
template <bool WIDE>
__global__ void __launch_bounds__(64) horizon_windows_kernel(const FrameC f, const HorizonWindowsC q) {
    const int lane = threadIdx.x;
    const int pt = (int)blockIdx.x;
    const int n_az = 1 << q.az_log2;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const la4 = reinterpret_cast<const float4*>(q.lights_a);
    const float4* const lb4 = reinterpret_cast<const float4*>(q.lights_b);
    uint32_t n_a = 0, n_b = 0, n_ab = 0;                    // wave-uniform counts
    EpochRuns no_a, no_b, ab, no_ab;                        // the runs of !ok_a, !ok_b, both, !both
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < q.m;
        bool ok_a = false, ok_b = false;
        if (in) {
            float la, lb, lc;
            ok_a = disc_fraction(la4[2 * (int64_t)k], p, hz, n_az, la, lb, lc) >= q.min_a;
            ok_b = disc_fraction(lb4[2 * (int64_t)k], p, hz, n_az, la, lb, lc) >= q.min_b;
        }
        const unsigned long long ma = __ballot(ok_a), mb = __ballot(ok_b), valid = __ballot(in);
        const unsigned long long mab = ma & mb;
        n_a += (uint32_t)__popcll(ma); n_b += (uint32_t)__popcll(mb); n_ab += (uint32_t)__popcll(mab);
        const int last = min(64, q.m - k0) - 1;
        no_a.longest(valid & ~ma, lane, in, last);
        no_b.longest(valid & ~mb, lane, in, last);
        ab.longest_first(mab, lane, in, last, k0);
        no_ab.longest(valid & ~mab, lane, in, last);
    }
    if (lane == 0) {
        const double md = (double)q.m;                      // shares are (float)(count / (double)m): a division, as specified
        float4* const o = reinterpret_cast<float4*>(q.out) + 2 * (int64_t)pt;
        o[0] = make_float4((float)((double)n_a / md), (float)no_a.best, (float)((double)n_b / md), (float)no_b.best);
        o[1] = make_float4((float)((double)n_ab / md), (float)ab.best, (float)ab.first, (float)no_ab.best);
    }
}

// Drive masks (DESIGN.md sections 3.19 and 4.22): horizon_windows_kernel's walk -- one wave per point, the epochs 64 at a time,
// the vertex and frame once, the horizon row in L1 -- with the joint predicate kept, not reduced: the chunk's ballot of
// ok_a && ok_b is the chunk's word (bit = lane = epoch & 63; the lanes past the last epoch vote 0), stored by lane 0.  Without a
// second table the bit is ok_a.  Nothing is carried from chunk to chunk; no atomics, no LDS.
template <bool WIDE>
__global__ void __launch_bounds__(64) horizon_mask_kernel(const FrameC f, const HorizonMaskC q) {
    const int lane = threadIdx.x;
    const int pt = (int)blockIdx.x;
    const int n_az = 1 << q.az_log2;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const la4 = reinterpret_cast<const float4*>(q.lights_a);
    const float4* const lb4 = reinterpret_cast<const float4*>(q.lights_b);
    unsigned long long* const row = q.out + (int64_t)pt * ((q.m + 63) >> 6);
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        bool ok = false;
        if (k < q.m) {
            float la, lb, lc;
            ok = disc_fraction(la4[2 * (int64_t)k], p, hz, n_az, la, lb, lc) >= q.min_a;
            if (lb4) ok = (disc_fraction(lb4[2 * (int64_t)k], p, hz, n_az, la, lb, lc) >= q.min_b) && ok;
        }
        const unsigned long long word = __ballot(ok);
        if (lane == 0) row[k0 >> 6] = word;
    }
}

// Site power budgets (DESIGN.md sections 3.17 and 4.19): horizon_windows_kernel's walk -- one wave per point, the epochs 64 at
// a time, the vertex and frame once, the horizon row in L1 -- with disc_fraction turned into integer counts of generated energy
// G_k (the panel's cosine factor from the same xu, xn, xe) and, with the host's counts of the load L_k, e_k = G_k - L_k.  FULL
// stores G_k.  SUMMARY reduces e in int64, so no result depends on the order of a reduction: per chunk an inclusive add scan
// (the running balance S), an exclusive scan of its peak (value and index, the later index on equal values), the wave's
// largest drawdown peak - S (its lowest lane from a ballot, kept only when strictly greater than the one held), and an
// inclusive scan of the clamp functions x -> min(hi, max(lo, x + a)) (closed under composition), which each lane applies to
// the carried state of charge.  Everything carried is wave-uniform and read from the chunk's last valid lane.  A lane past the
// last epoch holds e = 0 and no peak, no drawdown and no count: its clamp (0, 0, capacity) is the identity on a state of charge.
// Plain shuffles; no atomics, no LDS; lane 0 stores the point's four 16-byte pairs.
__device__ __forceinline__ long long ll_min(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long ll_max(long long a, long long b) { return a > b ? a : b; }
template <bool WIDE>
__global__ void __launch_bounds__(64) power_budget_kernel(const FrameC f, const PowerC q) {
    constexpr long long kLowest = -0x7fffffffffffffffll - 1;
    const int lane = threadIdx.x;
    const int pt = (int)blockIdx.x;
    const int n_az = 1 << q.az_log2;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const lights = reinterpret_cast<const float4*>(q.lights);
    const long long cap = q.capacity;
    long long sum_g = 0, unmet = 0, min_s = 0x7fffffffffffffffll;   // per lane, reduced at the end
    uint32_t n_unmet = 0;                                           // wave-uniform
    long long S_c = 0, pk_c = 0, s_c = q.initial, D = 0;            // the carries: balance, its peak, state of charge; the drawdown
    int pki_c = -1, d_first = -1, d_last = -1;
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < q.m;
        int G = 0, L = 0;
        if (in) {
            float la, lb, lc;
            const float fr = disc_fraction(lights[2 * (int64_t)k], p, hz, n_az, la, lb, lc);
            float c = 1.0f;
            if (q.panel != 0) {                                     // wave-uniform; xu, xn, xe as disc_fraction forms them
                const float xu = fmaf(p.uc, lc, fmaf(p.ub, lb, p.ua * la));
                const float xn = fmaf(p.Nc, lc, fmaf(p.Nb, lb, p.Na * la));
                const float xe = fmaf(-p.ct.x, lb, p.ct.y * la);
                c = q.panel == 1 ? fmaxf(0.0f, fmaf(q.nU, xu, fmaf(q.nN, xn, q.nE * xe)))
                                 : fminf(1.0f, sqrtf(fmaf(xe, xe, xn * xn)));
            }
            const float g = (q.gen[k] * fr) * c;
            G = (int)rintf(g * q.scale);
            if (q.mode == 0) reinterpret_cast<int32_t*>(q.out)[(int64_t)pt * q.m + k] = G;
            else L = q.load[k];
        }
        if (q.mode == 0) continue;
        const long long e = (long long)G - (long long)L;
        sum_g += (long long)G;
        // the balance after each epoch
        long long S = e;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const long long t = __shfl_up(S, s, 64);
            if (lane >= s) S += t;
        }
        S += S_c;
        // its peak up to and including each epoch (ps, pi), then up to the epoch before (xs, xi) with the carried peak
        long long ps = in ? S : kLowest;
        int pi = k;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const long long ts = __shfl_up(ps, s, 64);
            const int ti = __shfl_up(pi, s, 64);
            if (lane >= s && ts > ps) { ps = ts; pi = ti; }         // the earlier one only when strictly greater
        }
        long long xs = __shfl_up(ps, 1, 64);
        int xi = __shfl_up(pi, 1, 64);
        if (lane == 0 || pk_c > xs) { xs = pk_c; xi = pki_c; }
        const long long d = in ? xs - S : -1;
        long long mx = d;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) mx = ll_max(mx, __shfl_xor(mx, s, 64));
        if (mx > D) {                                               // wave-uniform; the lowest lane at mx: the earliest end
            const int jl = (int)__builtin_ctzll(__ballot(d == mx));
            D = mx;
            d_last = k0 + jl;
            d_first = __shfl(xi, jl, 64) + 1;
        }
        // the clamps of epochs k0 .. k composed: (fa, flo, fhi)
        long long fa = e, flo = 0, fhi = cap;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const long long ta = __shfl_up(fa, s, 64), tlo = __shfl_up(flo, s, 64), thi = __shfl_up(fhi, s, 64);
            if (lane >= s) {                                        // this lane's function after the earlier lanes'
                const long long nlo = ll_min(fhi, ll_max(flo, tlo + fa)), nhi = ll_min(fhi, ll_max(flo, thi + fa));
                fa += ta; flo = nlo; fhi = nhi;
            }
        }
        const long long sk = ll_min(fhi, ll_max(flo, s_c + fa));
        long long sp = __shfl_up(sk, 1, 64);
        if (lane == 0) sp = s_c;
        const long long t = sp + e;
        const bool miss = in && t < 0;
        if (in) min_s = ll_min(min_s, sk);
        if (miss) unmet -= t;
        n_unmet += (uint32_t)__popcll(__ballot(miss));
        const int last = min(64, q.m - k0) - 1;
        S_c = __shfl(S, last, 64);
        s_c = __shfl(sk, last, 64);
        const long long ls = __shfl(ps, last, 64);
        const int li = __shfl(pi, last, 64);
        if (!(pk_c > ls)) { pk_c = ls; pki_c = li; }
    }
    if (q.mode != 0) {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            sum_g += __shfl_xor(sum_g, s, 64);
            unmet += __shfl_xor(unmet, s, 64);
            min_s = ll_min(min_s, __shfl_xor(min_s, s, 64));
        }
        if (lane == 0) {
            longlong2* const o = reinterpret_cast<longlong2*>(q.out) + 4 * (int64_t)pt;
            o[0] = make_longlong2(sum_g, S_c);
            o[1] = make_longlong2(D, (long long)d_first);
            o[2] = make_longlong2((long long)d_last, min_s);
            o[3] = make_longlong2((long long)n_unmet, unmet);
        }
    }
}

// The Earth's occultation of the Sun (DESIGN.md sections 3.18 and 4.20): horizon_windows_kernel's walk -- one wave per point,
// the epochs 64 at a time with lane = epoch, the vertex and frame once -- with occult_fraction in place of disc_fraction and no
// horizon.  A lane whose epoch the host did not mark takes g = 1 without forming anything: the value it would have computed
// (the host's float64 test keeps a margin float32 cannot bridge).  FULL stores g.  SUMMARY: the float64 sum per lane in epoch
// order and the minimum, reduced at the end; the counts of g < 1 and g == 0 from the ballots; their runs by run_ending_here /
// wave_max, the earliest longest g < 1 run kept with its first epoch; and the number of maximal g < 1 runs, a set epoch whose
// predecessor is unset, lane 0's predecessor being the carried last bit of the chunk before.  Everything carried is
// wave-uniform.  No atomics, no LDS; lane 0 stores the point's two float4.
template <bool WIDE>
__global__ void __launch_bounds__(64) occultation_kernel(const FrameC f, const OccultC q) {
    const int lane = threadIdx.x;
    const int pt = (int)blockIdx.x;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    const float4* const src = reinterpret_cast<const float4*>(q.src);
    const float4* const body = reinterpret_cast<const float4*>(q.body);
    double sum = 0.0;                                       // per lane, reduced at the end
    float g_min = 1.0f;
    uint32_t n_part = 0, n_tot = 0, n_runs = 0;             // wave-uniform counts
    int cur_p = 0, cur_t = 0, best_p = 0, best_t = 0, first_p = -1;
    unsigned long long prev = 0;                            // the g < 1 bit of the previous chunk's last epoch
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < q.m;
        float g = 1.0f;
        if (in) {
            if (q.mark[k] != 0) g = occult_fraction(src[2 * (int64_t)k], body[2 * (int64_t)k], p);
            if (q.mode == 0) q.out[(int64_t)pt * q.m + k] = g;
        }
        if (q.mode == 0) continue;
        sum += in ? (double)g : 0.0;
        g_min = fminf(g_min, g);
        const unsigned long long mp = __ballot(in && g < 1.0f), mt = __ballot(in && g == 0.0f);
        n_part += (uint32_t)__popcll(mp); n_tot += (uint32_t)__popcll(mt);
        const int last = min(64, q.m - k0) - 1;
        const int rp = run_ending_here(mp, lane, in, cur_p);
        const int rt = run_ending_here(mt, lane, in, cur_t);
        cur_p = __shfl(rp, last, 64); cur_t = __shfl(rt, last, 64);
        best_t = max(best_t, wave_max(rt));
        const int mx = wave_max(rp);
        if (mx > best_p) {                                  // wave-uniform; the lowest lane that ends a run of mx: the earliest
            const unsigned long long at = __ballot(rp == mx);
            best_p = mx;
            first_p = k0 + (int)__builtin_ctzll(at) - mx + 1;
        }
        n_runs += (uint32_t)__popcll(mp & ~((mp << 1) | prev));
        prev = (mp >> last) & 1ull;
    }
    if (q.mode != 0) {
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            sum += __shfl_xor(sum, s, 64);
            g_min = fminf(g_min, __shfl_xor(g_min, s, 64));
        }
        if (lane == 0) {
            const double md = (double)q.m;
            float4* const o = reinterpret_cast<float4*>(q.out) + 2 * (int64_t)pt;
            o[0] = make_float4((float)(sum * (1.0 / md)), g_min, (float)((double)n_part / md), (float)((double)n_tot / md));
            o[1] = make_float4((float)best_p, (float)first_p, (float)best_t, (float)n_runs);
        }
    }
}

// Orbiter passes (DESIGN.md sections 3.27 and 4.33): a satellite at X (body axes, scene units) seen from the raised end P of a
// point -- its range, elevation es and azimuth, and its margin g = es - max(horizon at that azimuth, the elevation mask).  The
// unit direction, es, the azimuth in turns and the interpolated horizon are disc_fraction's operations restated for a point
// source (in view iff g > 0, its rule es > hh), so that function stays as it is.
struct SatLook {
    float es, az, range, g;     // degrees, degrees in [0, 360), scene units, degrees
};
__device__ __forceinline__ SatLook sat_look(const float4 X, float Pa, float Pb, float Pc, const PointFrame& p, const float* hz,
                                            int n_az, float min_elev) {
    constexpr float kDeg = 57.2957795130823209f, kInvTurn = 0.159154943091895336f;
    const float ta = X.x - Pa, tb = X.y - Pb, tc = X.z - Pc;
    const float dist = sqrt_sh(fmaf(tc, tc, fmaf(tb, tb, ta * ta)));
    const float inv_dist = rcp_cr(dist);
    const float la = ta * inv_dist, lb = tb * inv_dist, lc = tc * inv_dist;
    const float xu = fmaf(p.uc, lc, fmaf(p.ub, lb, p.ua * la));
    const float xn = fmaf(p.Nc, lc, fmaf(p.Nb, lb, p.Na * la));
    const float xe = fmaf(-p.ct.x, lb, p.ct.y * la);
    const float es = atan2f(xu, sqrtf(fmaf(xe, xe, xn * xn))) * kDeg;
    float ph = atan2f(xe, xn) * kInvTurn;                   // turns from north through east, [-1/2, 1/2]
    ph = ph < 0.0f ? ph + 1.0f : ph;
    const float x = ph * (float)n_az;
    const float x0 = floorf(x);
    const float w = x - x0;
    const int i0 = (int)x0 & (n_az - 1), i1 = (i0 + 1) & (n_az - 1);
    const float h0 = hz[i0], h1 = hz[i1];
    const float hh = fmaf(w, h1 - h0, h0);
    const float az = ph * 360.0f;                           // ph + 1 may round to a whole turn: north
    return {es, az >= 360.0f ? 0.0f : az, dist, es - fmaxf(hh, min_elev)};
}

// The pointing table and the coverage of a constellation: horizon_windows_kernel's walk -- one wave per point, the epochs 64 at
// a time with lane = epoch, the vertex, the frame and the raised origin once, the horizon row in L1 -- with a loop over the
// satellites inside each chunk.  FULL stores (es, azimuth, range in metres, g) per (satellite, epoch).
template <bool WIDE>
__global__ void __launch_bounds__(64) passes_full_kernel(const FrameC f, const PassesC q) {
    const int lane = threadIdx.x;
    const int pt = (int)blockIdx.x;
    const int n_az = 1 << q.az_log2;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    float Pa, Pb, Pc;
    sight_end(p, q.hs[pt], Pa, Pb, Pc);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const sat = reinterpret_cast<const float4*>(q.sat);
    float4* const out = reinterpret_cast<float4*>(q.out) + (int64_t)pt * q.n_sat * q.m;
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        if (k < q.m)
            for (int s = 0; s < q.n_sat; s++) {
                const SatLook l = sat_look(sat[s * q.m + k], Pa, Pb, Pc, p, hz, n_az, q.min_elev);
                out[(int64_t)s * q.m + k] = make_float4(l.es, l.az, l.range * q.range_scale, l.g);
            }
    }
}

// SUMMARY: per chunk each lane counts the satellites in view at its epoch, c_k, and keeps the greatest es among them; the
// ballots of c_k >= 1 and c_k >= 2 give the shares, the runs of c_k == 0 and c_k >= 1 go through EpochRuns (the earliest longest
// contact kept with its first epoch), and the contacts are counted as occultation_kernel counts its eclipses: a set epoch whose
// predecessor is unset, lane 0's predecessor being the carried last bit of the chunk before.  Everything carried is wave-uniform;
// the sum of c_k and the greatest es are reduced at the end.  No atomics, no LDS; lane 0 stores the point's two float4.
template <bool WIDE>
__global__ void __launch_bounds__(64) passes_summary_kernel(const FrameC f, const PassesC q) {
    const int lane = threadIdx.x;
    const int pt = (int)blockIdx.x;
    const int n_az = 1 << q.az_log2;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    float Pa, Pb, Pc;
    sight_end(p, q.hs[pt], Pa, Pb, Pc);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const sat = reinterpret_cast<const float4*>(q.sat);
    uint32_t n_any = 0, n_two = 0, n_runs = 0;              // wave-uniform counts
    uint32_t sum_c = 0;                                     // per lane, reduced at the end (n_sat * m <= 2^24)
    float e_max = -90.0f;                                   // per lane, reduced at the end
    EpochRuns outage, contact;                              // the runs of c_k == 0 and of c_k >= 1
    unsigned long long prev = 0;                            // the c_k >= 1 bit of the previous chunk's last epoch
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < q.m;
        uint32_t c = 0;
        if (in)
            for (int s = 0; s < q.n_sat; s++) {
                const SatLook l = sat_look(sat[s * q.m + k], Pa, Pb, Pc, p, hz, n_az, q.min_elev);
                if (l.g > 0.0f) { c++; e_max = fmaxf(e_max, l.es); }
            }
        sum_c += c;
        const unsigned long long m1 = __ballot(c >= 1u), m2 = __ballot(c >= 2u), valid = __ballot(in);
        n_any += (uint32_t)__popcll(m1); n_two += (uint32_t)__popcll(m2);
        const int last = min(64, q.m - k0) - 1;
        outage.longest(valid & ~m1, lane, in, last);
        contact.longest_first(m1, lane, in, last, k0);
        n_runs += (uint32_t)__popcll(m1 & ~((m1 << 1) | prev));
        prev = (m1 >> last) & 1ull;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        sum_c += __shfl_xor(sum_c, s, 64);
        e_max = fmaxf(e_max, __shfl_xor(e_max, s, 64));
    }
    if (lane == 0) {
        const double md = (double)q.m;
        float4* const o = reinterpret_cast<float4*>(q.out) + 2 * (int64_t)pt;
        o[0] = make_float4((float)((double)n_any / md), (float)outage.best, (float)contact.best, (float)contact.first);
        o[1] = make_float4((float)n_runs, e_max, (float)((double)sum_c / md), (float)((double)n_two / md));
    }
}

// LIST: one wave per (point, satellite), the epochs 64 at a time with lane = epoch.  FILL = false counts the passes -- the set
// epochs whose predecessor is unset, as above -- and lane 0 stores the count.  FILL = true recomputes the same margins and writes
// record base[point, satellite] + (passes ended so far) from the lane that ends the pass.  Per chunk: the ballot of the starts
// keys a segmented scan (plain shuffles) of the greatest es with its earliest epoch and of the least range, so the lane that
// ends a pass holds them from the pass's start in this chunk on; a pass that came in through the chunk's start joins them with
// what is carried.  Carried, all wave-uniform and read from the chunk's last valid lane: the in-view bit and the margin of the
// last epoch (the rise at lane 0 needs it), the open pass's first epoch, rise_frac, greatest es with its epoch and least range,
// and the passes ended so far.  The margin of the epoch after a lane's own comes by shuffle from the lane above; the top
// lane's comes from the next chunk, which is evaluated one iteration ahead (a single lane evaluating epoch k0 + 64 would cost the
// wave a whole evaluation more per chunk).  No atomics, no LDS, nothing between workgroups; the records' order is the prefix
// sums', so two runs write the same bytes.
struct PassLane {
    float g, es, range;
    bool in;
};
template <bool WIDE, bool FILL>
__global__ void __launch_bounds__(64) passes_list_kernel(const FrameC f, const PassesC q) {
    const int lane = threadIdx.x;
    const int pt = (int)(blockIdx.x / (unsigned)q.n_sat), s = (int)(blockIdx.x % (unsigned)q.n_sat);
    const int n_az = 1 << q.az_log2;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    float Pa, Pb, Pc;
    sight_end(p, q.hs[pt], Pa, Pb, Pc);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const sat = reinterpret_cast<const float4*>(q.sat) + s * q.m;
    auto eval = [&](int k0) -> PassLane {
        const int k = k0 + lane;
        PassLane r{0.0f, -INFINITY, INFINITY, k < q.m};
        if (r.in) {
            const SatLook l = sat_look(sat[k], Pa, Pb, Pc, p, hz, n_az, q.min_elev);
            r.g = l.g; r.es = l.es; r.range = l.range;
        }
        return r;
    };
    unsigned long long prev = 0;                            // the in-view bit of the previous chunk's last epoch
    if constexpr (!FILL) {
        uint32_t n_pass = 0;
        for (int k0 = 0; k0 < q.m; k0 += 64) {
            const PassLane c = eval(k0);
            const unsigned long long mv = __ballot(c.in && c.g > 0.0f);
            n_pass += (uint32_t)__popcll(mv & ~((mv << 1) | prev));
            prev = (mv >> (min(64, q.m - k0) - 1)) & 1ull;
        }
        if (lane == 0) q.counts[blockIdx.x] = n_pass;
        return;
    }
    PassRec* const rec = reinterpret_cast<PassRec*>(q.out) + q.base[blockIdx.x];
    const unsigned long long below = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);     // lanes 0 .. lane
    uint32_t n_done = 0;
    float g_last = 0.0f;                                    // the margin of the previous chunk's last epoch
    int c_first = 0, c_at = 0;                              // the pass that reaches the previous chunk's last epoch
    float c_rise = 0.0f, c_emax = 0.0f, c_rmin = 0.0f;
    PassLane cur = eval(0);
    for (int k0 = 0; k0 < q.m; k0 += 64) {
        const int k = k0 + lane;
        const bool more = k0 + 64 < q.m;                    // wave-uniform
        const PassLane nxt = more ? eval(k0 + 64) : PassLane{0.0f, -INFINITY, INFINITY, false};
        const int last = min(64, q.m - k0) - 1;
        const bool view = cur.in && cur.g > 0.0f;
        const unsigned long long mv = __ballot(view);
        const unsigned long long next_bit = (more && __shfl(nxt.g, 0, 64) > 0.0f) ? 1ull : 0ull;
        const unsigned long long st = mv & ~((mv << 1) | prev);
        const unsigned long long en = mv & ~((mv >> 1) | (next_bit << 63));
        // the margins of the epochs before and after this lane's
        float g_prev = __shfl_up(cur.g, 1, 64), g_next = __shfl_down(cur.g, 1, 64);
        const float g_top = __shfl(nxt.g, 0, 64);
        if (lane == 0) g_prev = g_last;
        if (lane == 63) g_next = g_top;
        const float rise = k == 0 ? 0.0f : cur.g / (cur.g - g_prev);
        const float setf = k == q.m - 1 ? 0.0f : cur.g / (cur.g - g_next);
        // the segment of this lane: from the nearest start at or below it, or from the chunk's start
        const unsigned long long hb = st & below;
        const int head = hb ? 63 - __clzll((long long)hb) : 0;
        float e = view ? cur.es : -INFINITY, r = view ? cur.range : INFINITY;
        int at = k;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float te = __shfl_up(e, d, 64), tr = __shfl_up(r, d, 64);
            const int ta = __shfl_up(at, d, 64);
            if (lane - d >= head) {
                if (te >= e) { e = te; at = ta; }           // the earlier epoch on equal elevations
                r = fminf(r, tr);
            }
        }
        int first = k0 + head;
        float rf = __shfl(rise, head, 64);
        if (!hb) {                                          // the pass came in through the chunk's start
            first = c_first; rf = c_rise;
            if (c_emax >= e) { e = c_emax; at = c_at; }
            r = fminf(r, c_rmin);
        }
        if ((en >> lane) & 1ull) {
            PassRec o;
            o.point = pt; o.sat = s; o.first = first; o.count = k - first + 1; o.max_at = at;
            o.flags = (first == 0 ? 1u : 0u) | (k == q.m - 1 ? 2u : 0u);
            o.rise_frac = rf; o.set_frac = setf; o.max_elev_deg = e; o.min_range_m = r * q.range_scale;
            rec[n_done + (uint32_t)__popcll(en & (below >> 1))] = o;
        }
        n_done += (uint32_t)__popcll(en);
        prev = (mv >> last) & 1ull;
        g_last = __shfl(cur.g, last, 64);
        c_first = __shfl(first, last, 64); c_rise = __shfl(rf, last, 64);
        c_emax = __shfl(e, last, 64); c_at = __shfl(at, last, 64); c_rmin = __shfl(r, last, 64);
        cur = nxt;
    }
}

// Regolith surface temperatures (DESIGN.md sections 3.10 and 4.11).  One lane = one point: its vertex and local frame are
// formed once, then per epoch the absorbed flux (the disc fraction of horizon_sun_kernel, illum_mu's mu, the albedo law) and
// n_sub explicit steps of its heat-conduction column.  The column's temperatures are float64 registers (a deep node moves by
// a few ulp of float32 per step, so float32 state would round its change away); the rates of a step are float32.  The layer
// tables are the kernel arguments' (wave-uniform, scalar loads); the node loops are unrolled to MRTX_THERMAL_NODES with a
// wave-uniform bound, so every index is a constant and the column never leaves the registers.  Lanes past the last point
// repeat it and store nothing.
// EXT (section 3.11, mrtx_thermal_scatter): the same column with two additions -- an extra absorbed flux q.xflux[pt][k] added
// to Q_abs in every epoch (spin-up and the start included), and mode 3 (EXITANCE), which records per epoch the reflected
// sunlight M_vis = A(theta) S f max(mu, 0) and the emission eps sigma T0^4 after the epoch's steps.  EXT = false is the
// mrtx_thermal kernel unchanged.
// COL (section 3.16, mrtx_thermal_column; EXT's column, modes 4 and 5 only): what the column holds below the surface.  COL = 1
// (COLUMN) stores (float)T_i of every node after each recorded epoch's steps.  COL = 2 (VOLATILE) keeps per node a float64 sum
// of the free sublimation rate E((float)T_i), evaluated once per recorded epoch, and a float32 maximum: 3 registers per node
// beside the column's own, and the point's n_nodes (mean E, T_max) pairs at the end.  COL = 0 is the kernel of modes 0-3,
// its machine code unchanged.
// After each epoch's steps the column is checked once (not per step, which would cost a share of the step itself): a node
// that is not finite or lies outside [20, 450] K, the range the step bound and the heat capacity were checked on, counts
// that (point, epoch) in q.caps[1]; the host then refuses the call's results (sections 3.10, 3.11).
// COLX = COL + 4 (section 3.18, mrtx_thermal_occulted; EXT's column and its modes, COL = COLX & 3): the disc fraction of
// every epoch, spin-up included, times occult_fraction's g for the far source and the body of q.occ_src / q.occ_body at the
// point's own vertex.  The epoch is wave-uniform, so its mark is a scalar branch: an unmarked epoch costs one scalar load.
// The flag rides in the third template argument so that the instantiations without it (COLX = 0, 1, 2) keep their names and
// their machine code (tools/asm_same.py).
template <bool WIDE, bool EXT, int COLX = 0>
__global__ void __launch_bounds__(64) thermal_kernel(const FrameC f, const ThermalC q) {
    constexpr int COL = COLX & 3;
    constexpr bool OCC = (COLX & 4) != 0;
    static_assert(COL == 0 || EXT, "the subsurface modes run EXT's column");
    static_assert(!OCC || EXT, "the occulted column runs EXT's column");
    constexpr int NN = MRTX_THERMAL_NODES;
    constexpr float kDeg = 57.2957795130823209f;
    const int lane = threadIdx.x;
    const int pt0 = (int)blockIdx.x * 64 + lane;
    const bool in = pt0 < q.g.rows;
    const int pt = in ? pt0 : q.g.rows - 1;
    const int n_az = 1 << q.az_log2;
    const int n = q.n_nodes;
    Vertex v;
    (void)illum_vertex<false, WIDE>(f, q.g, pt, pt, v, nullptr);
    const PointFrame p = point_frame(f, q.g, pt, pt, v);
    const float* const hz = q.horizon + ((int64_t)pt << q.az_log2);
    const float4* const lights = reinterpret_cast<const float4*>(q.lights);
    // Q_abs of epoch k: (1 - A(theta)) S_k f max(mu, 0), exactly 0 when f == 0 or mu <= 0; EXT: mv = A(theta) S_k f max(mu, 0)
    auto sunlit = [&](int k, float& mv) -> float {
        float la, lb, lc;
        float fr = disc_fraction(lights[2 * (int64_t)k], p, hz, n_az, la, lb, lc);
        if constexpr (OCC) {
            if (q.occ_mark[k] != 0)                                      // wave-uniform
                fr = fr * occult_fraction(reinterpret_cast<const float4*>(q.occ_src)[2 * (int64_t)k],
                                          reinterpret_cast<const float4*>(q.occ_body)[2 * (int64_t)k], p);
        }
        const float mu = fmaf(v.nc, lc, fmaf(v.nb, lb, v.na * la));      // illum_mu's expression
        if (!(fr > 0.0f) || !(mu > 0.0f)) { mv = 0.0f; return 0.0f; }
        const float th = acosf(fminf(mu, 1.0f)) * kDeg;
        const float x = th * (1.0f / 45.0f), y = th * (1.0f / 90.0f);
        const float y2 = y * y, y4 = y2 * y2;
        const float A = fmaf(q.alb[2], y4 * y4, fmaf(q.alb[1], x * x * x, q.alb[0]));
        if constexpr (EXT) mv = ((A * q.flux[k]) * fr) * mu;
        return (((1.0f - A) * q.flux[k]) * fr) * mu;
    };
    // what drives the surface in epoch k: Q_abs, plus EXT's extra flux
    auto absorbed = [&](int k, float& mv) -> float {
        const float qa = sunlit(k, mv);
        if constexpr (EXT) return q.xflux ? qa + q.xflux[(int64_t)pt * q.m + k] : qa;
        return qa;
    };
    float mv = 0.0f;
    if constexpr (COL == 0) {
        if (q.mode == 2) {
            if (in)
                for (int k = 0; k < q.m; k++) q.out[(int64_t)pt * q.m + k] = absorbed(k, mv);
            return;
        }
    }
    // the uniform start: ((<Q_abs> over the spin-up epochs + Q) / (eps sigma))^(1/4)
    double qs = 0.0;
    for (int k = 0; k < q.n_spin; k++) qs += (double)absorbed(k, mv);
    const double t_init = sqrt(sqrt(((q.n_spin > 0 ? qs / (double)q.n_spin : 0.0) + (double)q.q_geo) / (double)q.es));
    auto kof = [&](int i, double t) -> float {        // k_i(T) in float32
        const float tf = (float)t;
        return q.kc[i] * fmaf(q.chi3, tf * tf * tf, 1.0f);
    };
    // below node i0 the steady profile carrying Q upward from temperature `top` at node i0 (left as it is):
    // k_{i+1/2} (T_{i+1} - T_i) / dz_i = Q, the step of each link in float32 by six fixed-point passes, the last link by the
    // bottom rule
    auto geotherm = [&](double* T, int i0, double top) {
#pragma unroll
        for (int i = 0; i < NN - 1; i++) {
            const double ti = i == i0 ? top : T[i];
            if (i >= i0 && i < n - 2) {
                const float tf = (float)ti, ki = kof(i, ti);
                float d = 0.0f;
                for (int r = 0; r < 6; r++) {
                    const float t = tf + d;
                    d = q.qdz[i] / (0.5f * (ki + q.kc[i + 1] * fmaf(q.chi3, t * t * t, 1.0f)));
                }
                T[i + 1] = ti + (double)d;
            } else if (i >= i0 && i == n - 2) {
                T[i + 1] = ti + (double)(q.qdz[i] / kof(i, ti));
            }
        }
    };
    double T[NN];
#pragma unroll
    for (int i = 0; i < NN; i++) T[i] = t_init;
    geotherm(T, 0, t_init);
    uint32_t caps = 0, out_of_range = 0;
    double ref_sum = 0.0, sum_s = 0.0, sum_b = 0.0;
    float t_max = -INFINITY, t_min = INFINITY;
    int in_block = 0, blocks = 0;
    const int m_rec = q.m - q.n_spin;
    double e_sum[COL == 2 ? NN : 1];        // VOLATILE: the left fold of E((float)T_i) and the maximum of (float)T_i per node
    float n_max[COL == 2 ? NN : 1];
    if constexpr (COL == 2) {
#pragma unroll
        for (int i = 0; i < NN; i++) { e_sum[i] = 0.0; n_max[i] = -INFINITY; }
    }
    for (int k = 0; k < q.m; k++) {
        const float qa = absorbed(k, mv);
        for (int s = 0; s < q.n_sub; s++) {
            // 1. interior nodes from the old values; link i's flux k_{i+1/2} (T_{i+1} - T_i) / dz_i, k of node i carried
            float k_lo = kof(0, T[0]), k_hi = kof(1, T[1]);
            float g_lo = ((k_lo + k_hi) * q.hdz[0]) * (float)(T[1] - T[0]);
#pragma unroll
            for (int i = 1; i < NN - 1; i++) {
                if (i < n - 1) {
                    k_lo = k_hi;
                    k_hi = kof(i + 1, T[i + 1]);
                    const float g_hi = ((k_lo + k_hi) * q.hdz[i]) * (float)(T[i + 1] - T[i]);
                    const float tf = (float)T[i];
                    const float c = fmaf(fmaf(fmaf(fmaf(q.c[4], tf, q.c[3]), tf, q.c[2]), tf, q.c[1]), tf, q.c[0]);
                    T[i] += (double)((q.a[i] * (g_hi - g_lo)) * rcp_cr(c));
                    g_lo = g_hi;
                }
            }
            // 2. the surface: eps sigma T0^4 = Q_abs + k_{1/2}(T0) (T1 - T0) / dz0, Newton from the previous T0
            const float t1 = (float)T[1];
            const float k1 = kof(1, T[1]);
            float t0 = (float)T[0];
            int it = 0;
            for (; it < 30; it++) {
                const float t2 = t0 * t0, t3 = t2 * t0;
                const float kh = 0.5f * (q.kc[0] * fmaf(q.chi3, t3, 1.0f) + k1);
                const float d = t1 - t0;
                const float gv = (q.es * t3) * t0 - qa - (kh * d) * q.inv_dz0;
                const float gd = (4.0f * q.es) * t3 + (kh - ((1.5f * q.kc[0]) * q.chi3) * t2 * d) * q.inv_dz0;
                const float dt = gv / gd;
                t0 -= dt;
                if (fabsf(dt) < 1.0e-3f) break;
            }
            caps += it == 30 ? 1u : 0u;
            T[0] = (double)t0;
            // 3. the bottom: T_{N-1} = T_{N-2} + Q dz_{N-2} / k_{N-2}(T_{N-2})
#pragma unroll
            for (int i = 2; i < NN; i++)
                if (i == n - 1) T[i] = T[i - 1] + (double)(q.qdz[i - 1] / kof(i - 1, T[i - 1]));
        }
        // |T - 235| <= 215 is false for NaN and +-inf as well
        bool bad = false;
#pragma unroll
        for (int i = 0; i < NN; i++)
            if (i < n) bad = bad || !(fabs(T[i] - 235.0) <= 215.0);
        out_of_range += bad ? 1u : 0u;
        const float ts = (float)T[0];
        if (k < q.n_spin) {
            if (blocks < q.n_reset) {
                double tr = 0.0;
#pragma unroll
                for (int i = 0; i < NN; i++) tr = i == q.ref ? T[i] : tr;
                ref_sum += tr;
                if (++in_block == q.block) {
                    const double mean = ref_sum / (double)q.block;
                    geotherm(T, q.ref, mean);
                    ref_sum = 0.0;
                    in_block = 0;
                    blocks++;
                }
            }
        } else if constexpr (COL == 0) {
            double tb = 0.0;
#pragma unroll
            for (int i = 2; i < NN; i++) tb = i == n - 1 ? T[i] : tb;
            t_max = fmaxf(t_max, ts);
            t_min = fminf(t_min, ts);
            sum_s += (double)ts;
            sum_b += tb;
            if (in && q.mode == 0) q.out[(int64_t)pt * m_rec + (k - q.n_spin)] = ts;
            if constexpr (EXT) {
                if (in && q.mode == 3)
                    reinterpret_cast<float2*>(q.out)[(int64_t)pt * m_rec + (k - q.n_spin)] =
                        make_float2(mv, q.es * ((ts * ts) * (ts * ts)));
            }
        } else if constexpr (COL == 1) {
            // node i of recorded epoch k - n_spin: at most 2^31 outputs per call, so the index needs 64 bits
            float* const o = q.out + ((int64_t)pt * m_rec + (k - q.n_spin)) * n;
#pragma unroll
            for (int i = 0; i < NN; i++)
                if (in && i < n) o[i] = (float)T[i];
        } else {
            // E at the float32-rounded temperature (what COLUMN stores): x = b0 - b1 / T + b2 ln T + b3 T, once per epoch
#pragma unroll
            for (int i = 0; i < NN; i++) {
                if (i < n) {
                    const float tf = (float)T[i];
                    const double td = (double)tf;
                    const double x = fma(q.vb[3], td, fma(q.vb[2], log(td), q.vb[0] - q.vb[1] / td));
                    e_sum[i] = e_sum[i] + exp(x);
                    n_max[i] = fmaxf(n_max[i], tf);
                }
            }
        }
    }
    if constexpr (COL == 0) {
        if (in && q.mode == 1) {
            const double inv = 1.0 / (double)m_rec;
            reinterpret_cast<float4*>(q.out)[pt] = make_float4(t_max, t_min, (float)(sum_s * inv), (float)(sum_b * inv));
        }
    }
    if constexpr (COL == 2) {
        double2* const o = reinterpret_cast<double2*>(q.out) + (int64_t)pt * n;
#pragma unroll
        for (int i = 0; i < NN; i++)
            if (in && i < n) o[i] = make_double2(e_sum[i] / (double)m_rec, (double)n_max[i]);
    }
    caps = in ? caps : 0u;
    out_of_range = in ? out_of_range : 0u;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        caps += __shfl_xor(caps, s, 64);
        out_of_range += __shfl_xor(out_of_range, s, 64);
    }
    if (lane == 0 && caps) atomicAdd(q.caps, (unsigned long long)caps);
    if (lane == 0 && out_of_range) atomicAdd(q.caps + 1, (unsigned long long)out_of_range);
}

// What terrain a point sees (DESIGN.md sections 3.11 and 4.12): per point K fixed cosine-weighted directions fed through
// continue_path's mapping (sqrt_sh, sincos_turn, duff_basis) from the lifted origin, each marched and refined exactly as a
// path's continuation ray, to the (lat, lon) of its first terrain hit or NaN when it leaves the bounding sphere.  One lane =
// one (point, j), point-major: every lane forms its point's vertex (5 DEM taps) and marches one ray.  Measured 3-4x faster
// than one lane per point looping over j (4.12): a lane's rays differ in length, so the loop left most lanes of a wave idle.
// view_share_kernel then counts each point's hits.
template <bool WIDE, bool STATS>
__global__ void __launch_bounds__(64) view_hits_kernel(const FrameC f, const ViewC q) {
    constexpr float kDeg = 57.2957795130823209f;
    const int lane = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * 64 + lane;
    uint32_t cnt_store[STATS ? ST_N : 1] = {};
    uint32_t* const cnt = STATS ? cnt_store : nullptr;
    if (gid < (int64_t)q.g.rows * q.K) {
        const int pt = (int)(gid / q.K), j = (int)(gid % q.K);
        Vertex v;
        (void)illum_vertex<STATS, WIDE>(f, q.g, pt, pt, v, cnt);    // g.points = 1: both tables indexed by the point
        float b1a, b1b, b1c, b2a, b2b, b2c;
        duff_basis(v.na, v.nb, v.nc, b1a, b1b, b1c, b2a, b2b, b2c);
        const PointFrame p = point_frame(f, q.g, pt, pt, v);
        const float2 uh = reinterpret_cast<const float2*>(q.dirs)[j];
        const float rr = sqrt_sh(uh.x), zz = sqrt_sh(1.0f - uh.x);
        float cph, sph;
        sincos_turn(uh.y, cph, sph);
        const float xx = rr * cph, yy = rr * sph;
        const float da = fmaf(zz, v.na, fmaf(yy, b2a, xx * b1a));
        const float db = fmaf(zz, v.nb, fmaf(yy, b2b, xx * b1b));
        const float dc = fmaf(zz, v.nc, fmaf(yy, b2c, xx * b1c));
        if (STATS) cnt[ST_BOUNCE]++;
        Seg sg;
        float hi = 0.0f;
        float2 o = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        if (march<WIDE, false, STATS, MRTX_STEP_BATCH>(f, p.oa, p.ob, p.oc, da, db, dc, 0.0f, sg, hi, cnt)) {
            const int bk = (int)rintf(hi * f.inv_step);
            float lo = (float)(bk - 1) * f.step;
            refine<WIDE>(f, sg, p.oa, p.ob, p.oc, da, db, dc, lo, hi);
            if (STATS) { cnt[ST_HEIGHT] += (uint32_t)f.nbis; cnt[ST_FETCH] += (uint32_t)f.nbis; }
            const float ha = fmaf(lo, da, p.oa), hb = fmaf(lo, db, p.ob), hc = fmaf(lo, dc, p.oc);
            float lat, lon;
            latlon(ha, hb, hc, fmaf(hb, hb, ha * ha), lat, lon);
            o = make_float2(lat * kDeg, lon * kDeg);
        }
        reinterpret_cast<float2*>(q.out)[gid] = o;
    }
    stage_flush<STATS>(f, cnt, ST_BOUNCE, lane);
}

// The terrain share of each point: its hits (non-NaN latitudes) over K, exact for a power of two.  One lane per point.
__global__ void __launch_bounds__(64) view_share_kernel(const ViewC q) {
    const int pt = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (pt >= q.g.rows) return;
    const float2* const row = reinterpret_cast<const float2*>(q.out) + (int64_t)pt * q.K;
    int n_hit = 0;
    for (int j = 0; j < q.K; j++) n_hit += row[j].x == row[j].x ? 1 : 0;
    q.out[2 * (int64_t)q.g.rows * q.K + pt] = (float)n_hit / (float)q.K;
}

// The gather of section 3.11: Q_sec[p][k] = (1/K) sum over j = 0, 1, ..., K - 1 with idx[p][j] >= 0, in that order, of
// ((1 - A_h) M_vis + eps M_ir) of hit idx[p][j] at epoch k, each term and each partial sum rounded to float32 (no fused
// multiply-add).  Lane = epoch: one block = 64 consecutive epochs of one target, so the hit's row is read contiguously and the
// index row is wave-uniform (scalar loads).
__global__ void __launch_bounds__(64) scatter_flux_kernel(const ScatterC q) {
    const int64_t b = blockIdx.x;
    const int p = (int)(b / q.chunks);
    const int k = (int)(b % q.chunks) * 64 + (int)threadIdx.x;
    if (k >= q.m) return;
    const int32_t* const ix = q.idx + (int64_t)p * q.K;
    const float2* const ex = reinterpret_cast<const float2*>(q.ex);
    float s = 0.0f;
    for (int j = 0; j < q.K; j++) {
        const int h = ix[j];
        if (h >= 0) {
            const float2 e = ex[(int64_t)h * q.m + k];
            const float t = q.omah * e.x, u = q.eps * e.y;
            s = s + (t + u);
        }
    }
    q.out[(int64_t)p * q.m + k] = s * q.inv_k;
}

// Terrain line of sight (DESIGN.md sections 3.12 and 4.13).  One probe: does the raised target end T see the raised observer
// end O?  The march starts at the lower end (|P|^2 in float32; the target on a tie) and heads for the other one, so a swap of
// the two ends marches the same ray (O - T == -(T - O) exactly); it is a shadow ray's march -- steps, skip intervals,
// horizon-mip cut, below test -- that also ends before the first step with s_k >= L.  A lower end outside the bounding sphere
// marches from where the segment enters the sphere, or not at all when the segment misses it.  true: clear.
template <bool STATS, bool WIDE>
__device__ __forceinline__ bool sight_probe(const FrameC& f, float Ta, float Tb, float Tc, float Oa, float Ob, float Oc,
                                            uint32_t* cnt) {
    if (STATS) cnt[ST_SHADOW]++;
    const float rT = fmaf(Tc, Tc, fmaf(Tb, Tb, Ta * Ta)), rO = fmaf(Oc, Oc, fmaf(Ob, Ob, Oa * Oa));
    const bool from_t = rT <= rO;
    float oa = from_t ? Ta : Oa, ob = from_t ? Tb : Ob, oc = from_t ? Tc : Oc;
    const float ta = from_t ? Oa - Ta : Ta - Oa, tb = from_t ? Ob - Tb : Tb - Ob, tc = from_t ? Oc - Tc : Tc - Oc;
    const float L2 = fmaf(tc, tc, fmaf(tb, tb, ta * ta));
    if (!(L2 > 0.0f)) return true;                          // the two ends coincide
    const float L = sqrt_sh(L2);
    const float inv = rcp_cr(L);
    const float da = ta * inv, db = tb * inv, dc = tc * inv;
    float smax = L;
    const float q0 = from_t ? rT : rO;
    if (q0 > f.R2f) {                                       // the lower end lies outside the bounding sphere
        const float b = fmaf(oc, dc, fmaf(ob, db, oa * da));
        const float c = q0 - f.R2f;
        const float disc = fmaf(b, b, -c);
        if (!(b < 0.0f) || !(disc >= 0.0f)) return true;   // heads away from the sphere, or misses it
        const float s_in = c / (sqrtf(disc) - b);           // the nearer root of s^2 + 2 b s + c, without cancellation
        if (!(s_in < L)) return true;                       // the segment ends before the sphere
        oa = fmaf(s_in, da, oa); ob = fmaf(s_in, db, ob); oc = fmaf(s_in, dc, oc);
        smax = L - s_in;
    }
    Seg ssg;
    float sk_occ;
    return !march<WIDE, false, STATS, MRTX_STEP_BATCH, 2, true>(f, oa, ob, oc, da, db, dc, smax, ssg, sk_occ, cnt);
}

// the raised end of a point: P = fmaf(hs, u, o), o its lifted origin
__device__ __forceinline__ void sight_end(const PointFrame& p, float hs, float& Pa, float& Pb, float& Pc) {
    Pa = fmaf(hs, p.ua, p.oa);
    Pb = fmaf(hs, p.ub, p.ob);
    Pc = fmaf(hs, p.uc, p.oc);
}

// Per target the extra mast height (metres) at which it sees the observer: 0 if it does at its own height, otherwise a
// bisection over t in [0, 1] of the mast t * mast_max (n_bis - 1 probes after the one at t = 1), +inf when even mast_max
// is blocked.  Lane = target; a wave = 64 neighbouring nodes of one row (or 64 consecutive points), so with one observer its
// rays leave nearby points for one end point.  The observer's vertex is formed per lane with the target's own code.
template <bool STATS, bool WIDE>
__global__ void __launch_bounds__(64) sight_kernel(const FrameC f, const SightC q) {
    const int lane = threadIdx.x;
    const int row = (int)(blockIdx.x / (unsigned)q.waves_x);
    const int col = (int)(blockIdx.x % (unsigned)q.waves_x) * 64 + lane;
    const bool in = row < q.g.rows && col < q.g.cols;
    uint32_t cnt_store[STATS ? ST_N : 1] = {};
    uint32_t* const cnt = STATS ? cnt_store : nullptr;
    if (in) {
        Vertex vt, vo;
        (void)illum_vertex<STATS, WIDE>(f, q.g, row, col, vt, cnt);
        const int oi = q.n_obs == 1 ? 0 : col;
        (void)illum_vertex<STATS, WIDE>(f, q.obs, oi, oi, vo, cnt);   // obs.points = 1: both tables indexed by the observer
        const PointFrame pt = point_frame(f, q.g, row, col, vt), po = point_frame(f, q.obs, oi, oi, vo);
        float Oa, Ob, Oc;
        sight_end(po, q.obs_hs[oi], Oa, Ob, Oc);
        // the target raised by target_h + t * mast_max metres
        auto probe = [&](float t) {
            const float hs = (float)((q.target_h_m + (double)t * q.mast_max_m) / q.radius_m * q.R);
            float Ta, Tb, Tc;
            sight_end(pt, hs, Ta, Tb, Tc);
            return sight_probe<STATS, WIDE>(f, Ta, Tb, Tc, Oa, Ob, Oc, cnt);
        };
        float m = 0.0f;
        if (!probe(0.0f)) {
            m = __builtin_inff();
            if (q.n_bis > 0 && probe(1.0f)) {
                float lo = 0.0f, hi = 1.0f;
                for (int i = 1; i < q.n_bis; i++) {
                    const float mid = 0.5f * (lo + hi);             // dyadic, at most 23 fraction bits: exact
                    const bool clear = probe(mid);
                    hi = clear ? mid : hi;
                    lo = clear ? lo : mid;
                }
                m = (float)((double)hi * q.mast_max_m);
            }
        }
        q.out[(int64_t)row * q.g.cols + col] = m;
    }
    stage_flush<STATS>(f, cnt, ST_SHADOW, lane);
}

}  // namespace mrtx

// ------------------------------------------------------------------------------------------------
// launch wrappers (called from mrtx_api.hip)
extern "C++" {
// Runs launch(a, b) with a and b as std::integral_constant<bool>, so that the lambda can name the kernel instantiation it
// launches (kernel<a(), b()>): the four instantiations a pair of run-time flags such as (stats, wide) selects.
template <class L>
static void pick2(bool a, bool b, L&& launch) {
    if (a) { if (b) launch(std::true_type{}, std::true_type{}); else launch(std::true_type{}, std::false_type{}); }
    else { if (b) launch(std::false_type{}, std::true_type{}); else launch(std::false_type{}, std::false_type{}); }
}

// The Sun illumination stage (illum_kernel): one wave per block of nodes -- 64 / n_sun nodes in a
// PW x PH block, PW as render_geometry picks it for as many pixels.  g.rows x g.cols nodes; g.pw_log2 and g.waves_x are set here.
hipError_t mrtx_launch_illum(const FrameC& f, IllumC g, bool stats, hipStream_t st) {
    if (g.n_sun < 1 || g.n_sun > 64 || (g.n_sun & (g.n_sun - 1)) || g.rows < 1 || g.cols < 1) return hipErrorInvalidValue;
    g.n_log2 = 0;
    while ((1 << g.n_log2) < g.n_sun) g.n_log2++;
    const int P = 64 >> g.n_log2;
    int PW = P >= 32 ? 8 : P >= 8 ? 4 : P >= 2 ? 2 : 1;
    if (g.rows == 1) PW = P;                    // a point list (or a one-row band): the nodes side by side
    g.pw_log2 = PW == 64 ? 6 : PW == 32 ? 5 : PW == 16 ? 4 : PW == 8 ? 3 : PW == 4 ? 2 : PW == 2 ? 1 : 0;
    const int PH = P / PW;
    g.waves_x = (g.cols + PW - 1) / PW;
    const uint64_t waves = (uint64_t)g.waves_x * (uint64_t)((g.rows + PH - 1) / PH);
    if (waves > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)waves), block(64);
    pick2(stats, f.dem_wide != 0, [&](auto s, auto w) {
        hipLaunchKernelGGL((mrtx::illum_kernel<s(), w()>), grid, block, 0, st, f, g);
    });
    return hipGetLastError();
}

// The series (illum_series_kernel): the node block of mrtx_launch_illum with points as rows and a window's epochs as columns,
// PW = 64 / n_sun epochs wide, narrowed to the window (the least power of two >= count) so that a wave holds several points
// when the window is short.  g.rows points x g.cols epochs; g.n_log2, g.pw_log2 and g.waves_x are set here.
hipError_t mrtx_launch_illum_series(const FrameC& f, IllumSeriesC q, bool stats, hipStream_t st) {
    IllumC& g = q.g;
    if (g.n_sun < 1 || g.n_sun > 64 || (g.n_sun & (g.n_sun - 1)) || g.rows < 1 || g.cols < 1 || !g.points || !q.lights)
        return hipErrorInvalidValue;
    g.n_log2 = 0;
    while ((1 << g.n_log2) < g.n_sun) g.n_log2++;
    const int P = 64 >> g.n_log2;
    int PW = P;
    while (PW > 1 && PW / 2 >= g.cols) PW /= 2;
    g.pw_log2 = 0;
    while ((1 << g.pw_log2) < PW) g.pw_log2++;
    const int PH = P / PW;
    g.waves_x = (g.cols + PW - 1) / PW;
    const uint64_t waves = (uint64_t)g.waves_x * (uint64_t)((g.rows + PH - 1) / PH);
    if (waves > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)waves), block(64);
    pick2(stats, f.dem_wide != 0, [&](auto s, auto w) {
        hipLaunchKernelGGL((mrtx::illum_series_kernel<s(), w()>), grid, block, 0, st, f, q);
    });
    return hipGetLastError();
}

// Terrain horizons (horizon_kernel): lane = (point, azimuth), point-major, 64 lanes per wave.  h.g.rows points.
hipError_t mrtx_launch_horizon(const FrameC& f, HorizonC h, bool stats, hipStream_t st) {
    if (h.g.rows < 1 || h.az_log2 < 2 || h.az_log2 > 12 || h.n_bis < 1 || h.n_bis > 24 || !h.g.points || !h.out)
        return hipErrorInvalidValue;
    const uint64_t lanes = (uint64_t)h.g.rows << h.az_log2;
    if (lanes > (1ull << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((lanes + 63) / 64)), block(64);
    pick2(stats, f.dem_wide != 0, [&](auto s, auto w) {
        hipLaunchKernelGGL((mrtx::horizon_kernel<s(), w()>), grid, block, 0, st, f, h);
    });
    return hipGetLastError();
}

// The Sun against a horizon (horizon_sun_kernel): one wave per point.
hipError_t mrtx_launch_horizon_sun(const FrameC& f, HorizonSunC q, hipStream_t st) {
    if (q.g.rows < 1 || q.az_log2 < 2 || q.az_log2 > 12 || q.m < 1 || (q.mode != 0 && q.mode != 1) || !q.g.points || !q.horizon ||
        !q.lights || !q.out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)q.g.rows), block(64);
    if (f.dem_wide) hipLaunchKernelGGL((mrtx::horizon_sun_kernel<true>), grid, block, 0, st, f, q);
    else hipLaunchKernelGGL((mrtx::horizon_sun_kernel<false>), grid, block, 0, st, f, q);
    return hipGetLastError();
}

// Raised horizons (horizon_raised_kernel): mrtx_launch_horizon's lane mapping, with the per-point raise table q.hs.
hipError_t mrtx_launch_horizon_raised(const FrameC& f, HorizonRaisedC q, bool stats, hipStream_t st) {
    const HorizonC& h = q.h;
    if (h.g.rows < 1 || h.az_log2 < 2 || h.az_log2 > 12 || h.n_bis < 1 || h.n_bis > 24 || !h.g.points || !h.out || !q.hs)
        return hipErrorInvalidValue;
    const uint64_t lanes = (uint64_t)h.g.rows << h.az_log2;
    if (lanes > (1ull << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((lanes + 63) / 64)), block(64);
    pick2(stats, f.dem_wide != 0, [&](auto s, auto w) {
        hipLaunchKernelGGL((mrtx::horizon_raised_kernel<s(), w()>), grid, block, 0, st, f, q);
    });
    return hipGetLastError();
}

// Joint windows (horizon_windows_kernel): one wave per point.
hipError_t mrtx_launch_horizon_windows(const FrameC& f, HorizonWindowsC q, hipStream_t st) {
    if (q.g.rows < 1 || q.az_log2 < 2 || q.az_log2 > 12 || q.m < 1 || q.m > (1 << 24) || !q.g.points || !q.horizon ||
        !q.lights_a || !q.lights_b || !q.out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)q.g.rows), block(64);
    if (f.dem_wide) hipLaunchKernelGGL((mrtx::horizon_windows_kernel<true>), grid, block, 0, st, f, q);
    else hipLaunchKernelGGL((mrtx::horizon_windows_kernel<false>), grid, block, 0, st, f, q);
    return hipGetLastError();
}

// Drive masks (horizon_mask_kernel): one wave per point.
hipError_t mrtx_launch_horizon_mask(const FrameC& f, HorizonMaskC q, hipStream_t st) {
    if (q.g.rows < 1 || q.az_log2 < 2 || q.az_log2 > 12 || q.m < 1 || q.m > (1 << 24) || !q.g.points || !q.horizon ||
        !q.lights_a || !q.out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)q.g.rows), block(64);
    if (f.dem_wide) hipLaunchKernelGGL((mrtx::horizon_mask_kernel<true>), grid, block, 0, st, f, q);
    else hipLaunchKernelGGL((mrtx::horizon_mask_kernel<false>), grid, block, 0, st, f, q);
    return hipGetLastError();
}

// Site power budgets (power_budget_kernel): one wave per point.
hipError_t mrtx_launch_power_budget(const FrameC& f, PowerC q, hipStream_t st) {
    if (q.g.rows < 1 || q.az_log2 < 2 || q.az_log2 > 12 || q.m < 1 || q.m > (1 << 24) || (q.mode != 0 && q.mode != 1) ||
        q.panel < 0 || q.panel > 2 || q.initial < 0 || q.initial > q.capacity || q.capacity > (1ll << 52) || !q.g.points ||
        !q.horizon || !q.lights || !q.gen || !q.load || !q.out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)q.g.rows), block(64);
    if (f.dem_wide) hipLaunchKernelGGL((mrtx::power_budget_kernel<true>), grid, block, 0, st, f, q);
    else hipLaunchKernelGGL((mrtx::power_budget_kernel<false>), grid, block, 0, st, f, q);
    return hipGetLastError();
}

// The Earth's occultation of the Sun (occultation_kernel): one wave per point.
hipError_t mrtx_launch_occultation(const FrameC& f, OccultC q, hipStream_t st) {
    if (q.g.rows < 1 || q.m < 1 || q.m > (1 << 24) || (q.mode != 0 && q.mode != 1) || !q.g.points || !q.src || !q.body || !q.mark ||
        !q.out)
        return hipErrorInvalidValue;
    if (q.mode == 0 && (int64_t)q.g.rows * q.m > (int64_t)1 << 31) return hipErrorInvalidValue;
    if (q.mode == 1 && ((uintptr_t)q.out & 15)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)q.g.rows), block(64);
    if (f.dem_wide) hipLaunchKernelGGL((mrtx::occultation_kernel<true>), grid, block, 0, st, f, q);
    else hipLaunchKernelGGL((mrtx::occultation_kernel<false>), grid, block, 0, st, f, q);
    return hipGetLastError();
}

// Orbiter passes (passes_full_kernel, passes_summary_kernel: one wave per point; passes_list_kernel: one wave per (point,
// satellite)).  mode: MRTX_PASSES_FULL / SUMMARY, 2 = LIST's count, 3 = LIST's fill.
hipError_t mrtx_launch_passes(const FrameC& f, PassesC q, int mode, hipStream_t st) {
    if (q.g.rows < 1 || q.az_log2 < 2 || q.az_log2 > 12 || q.m < 1 || q.n_sat < 1 || q.n_sat > 256 ||
        (int64_t)q.n_sat * q.m > (int64_t)1 << 24 || mode < 0 || mode > 3 || !q.g.points || !q.horizon || !q.hs || !q.sat)
        return hipErrorInvalidValue;
    if (mode == 0 && (!q.out || ((uintptr_t)q.out & 15) || (int64_t)q.g.rows * q.n_sat * q.m > (int64_t)1 << 27)) return hipErrorInvalidValue;
    if (mode == 1 && (!q.out || ((uintptr_t)q.out & 15))) return hipErrorInvalidValue;
    if (mode >= 2 && (int64_t)q.g.rows * q.n_sat > (int64_t)1 << 27) return hipErrorInvalidValue;
    if (mode == 2 && !q.counts) return hipErrorInvalidValue;
    if (mode == 3 && (!q.out || ((uintptr_t)q.out & 7) || !q.base)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(mode >= 2 ? q.g.rows * q.n_sat : q.g.rows)), block(64);
    pick2(mode & 1, f.dem_wide != 0, [&](auto odd, auto w) {
        if (mode < 2) {
            if constexpr (odd()) hipLaunchKernelGGL((mrtx::passes_summary_kernel<w()>), grid, block, 0, st, f, q);
            else hipLaunchKernelGGL((mrtx::passes_full_kernel<w()>), grid, block, 0, st, f, q);
        } else {
            hipLaunchKernelGGL((mrtx::passes_list_kernel<w(), odd()>), grid, block, 0, st, f, q);
        }
    });
    return hipGetLastError();
}

// Terrain line of sight (sight_kernel): one lane per target, q.g.rows rows of q.g.cols targets, 64 targets of a row per wave.
hipError_t mrtx_launch_sight(const FrameC& f, SightC q, bool stats, hipStream_t st) {
    if (q.g.rows < 1 || q.g.cols < 1 || q.n_bis < 0 || q.n_bis > 24 || (q.n_obs != 1 && q.n_obs != q.g.cols) || !q.g.rtab ||
        !q.g.ctab || !q.obs.rtab || !q.obs.ctab || !q.obs_hs || !q.out || !q.obs.points)
        return hipErrorInvalidValue;
    if ((uint64_t)q.g.rows * (uint64_t)q.g.cols > (1ull << 31)) return hipErrorInvalidValue;
    q.waves_x = (q.g.cols + 63) / 64;
    const uint64_t waves = (uint64_t)q.g.rows * (uint64_t)q.waves_x;
    if (waves > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)waves), block(64);
    pick2(stats, f.dem_wide != 0, [&](auto s, auto w) {
        hipLaunchKernelGGL((mrtx::sight_kernel<s(), w()>), grid, block, 0, st, f, q);
    });
    return hipGetLastError();
}

// The thermal column under occultation (thermal_kernel<.., COL + 4>; called by mrtx_launch_thermal, which made the checks).
static hipError_t mrtx_launch_thermal_occulted(const FrameC& f, const ThermalC& q, dim3 grid, hipStream_t st) {
    const dim3 block(64);
    pick2(f.dem_wide != 0, q.mode >= 4, [&](auto w, auto c) {
        if (!c()) hipLaunchKernelGGL((mrtx::thermal_kernel<w(), true, 4>), grid, block, 0, st, f, q);
        else if (q.mode == 4) hipLaunchKernelGGL((mrtx::thermal_kernel<w(), true, 5>), grid, block, 0, st, f, q);
        else hipLaunchKernelGGL((mrtx::thermal_kernel<w(), true, 6>), grid, block, 0, st, f, q);
    });
    return hipGetLastError();
}

// Regolith surface temperatures (thermal_kernel): one lane per point, 64 per wave.  ext: the same column with an extra
// absorbed flux and the EXITANCE mode 3 (mrtx_thermal_scatter, section 3.11), and the subsurface modes 4 (COLUMN) and
// 5 (VOLATILE) of mrtx_thermal_column (section 3.16), which have instantiations of their own.
hipError_t mrtx_launch_thermal(const FrameC& f, const ThermalC& q, bool ext, hipStream_t st) {
    if (q.g.rows < 1 || q.az_log2 < 2 || q.az_log2 > 12 || q.m < 1 || q.mode < 0 || q.mode > (ext ? 5 : 2) || q.n_nodes < 3 ||
        q.n_nodes > MRTX_THERMAL_NODES || q.n_sub < 1 || q.block < 1 || q.n_spin < 0 || q.n_reset < 0 || q.ref < 0 ||
        q.ref >= q.n_nodes - 1 || (q.mode != 2 && q.n_spin >= q.m) || !q.g.points || !q.horizon || !q.lights || !q.flux ||
        !q.out || !q.caps)
        return hipErrorInvalidValue;
    if (q.mode == 4 && (int64_t)q.g.rows * (q.m - q.n_spin) * q.n_nodes > (int64_t)1 << 31) return hipErrorInvalidValue;
    if (q.mode == 5 && ((uintptr_t)q.out & 7)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((q.g.rows + 63) / 64)), block(64);
    if (q.occ_mark || q.occ_src || q.occ_body) {            // mrtx_thermal_occulted with tables: kernels of their own
        if (!ext || !q.occ_mark || !q.occ_src || !q.occ_body) return hipErrorInvalidValue;
        return mrtx_launch_thermal_occulted(f, q, grid, st);
    }
    if (q.mode >= 4)
        pick2(f.dem_wide != 0, q.mode == 5, [&](auto w, auto v) {
            hipLaunchKernelGGL((mrtx::thermal_kernel<w(), true, v() ? 2 : 1>), grid, block, 0, st, f, q);
        });
    else
        pick2(f.dem_wide != 0, ext, [&](auto w, auto e) {
            hipLaunchKernelGGL((mrtx::thermal_kernel<w(), e()>), grid, block, 0, st, f, q);
        });
    return hipGetLastError();
}

// View samples (view_hits_kernel): one lane per (point, j), 64 per wave; then the shares (view_share_kernel).
hipError_t mrtx_launch_view_hits(const FrameC& f, const ViewC& q, bool stats, hipStream_t st) {
    if (q.g.rows < 1 || q.K < 16 || q.K > 1024 || (q.K & (q.K - 1)) || !q.g.points || !q.dirs || !q.out ||
        (int64_t)q.g.rows * q.K > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((int64_t)q.g.rows * q.K + 63) / 64)), block(64);
    pick2(stats, f.dem_wide != 0, [&](auto s, auto w) {
        hipLaunchKernelGGL((mrtx::view_hits_kernel<w(), s()>), grid, block, 0, st, f, q);
    });
    hipLaunchKernelGGL(mrtx::view_share_kernel, dim3((unsigned)((q.g.rows + 63) / 64)), block, 0, st, q);
    return hipGetLastError();
}

// The gather (scatter_flux_kernel): one block of 64 lanes per (target, 64 epochs).
hipError_t mrtx_launch_scatter_flux(const ScatterC& q, hipStream_t st) {
    if (q.n < 1 || q.K < 1 || q.m < 1 || q.chunks != (q.m + 63) / 64 || !q.idx || !q.ex || !q.out) return hipErrorInvalidValue;
    const int64_t blocks = (int64_t)q.n * q.chunks;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx::scatter_flux_kernel, dim3((unsigned)blocks), dim3(64), 0, st, q);
    return hipGetLastError();
}
}
