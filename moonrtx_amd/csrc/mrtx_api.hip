// mrtx_api.hip -- host side of libmoonrt.so: the C ABI declared in include/moonrt.h, but for the calls that work on a lattice
// of nodes and its tables (regions, zonal statistics, proximity, outlines, contours, depressions, bowls), whose host side is
// mrtx_lattice_api.hip.  What the two units share (the context, the refusal, the staging path) is declared in mrtx_host.h and
// defined here.
//
// The context keeps the scene the way the reference describes it to its renderer object (float64
// camera / moon frame / light / Sun disk, moon_renderer.py:570-650 and :824-871) and derives the
// float32 per-launch constant block (FrameC) from it right before every launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "mrtx_host.h"

using namespace mrtx_host;

hipError_t mrtx_launch_render(const FrameC& f, int S, bool stats, int mode, bool overlay, const PathQ* pq, hipStream_t st);
uint64_t mrtx_path_chunks(const FrameC& f, int S, uint32_t* grid_a, int* njobs_log2);
int mrtx_path_waves(bool stats, bool wide, int* out);
hipError_t mrtx_launch_paths(const FrameC& f, const PathQ& pq, int S, bool stats, int n_waves, hipStream_t st);
hipError_t mrtx_launch_resolve_linear(const float* accum, float* out, int64_t npix, uint32_t ns, hipStream_t st);
hipError_t mrtx_launch_resolve_rgba8(const float* accum, uint32_t* out, int64_t npix, uint32_t ns, float expo,
                                     const float* T8, const uint32_t* overlay, hipStream_t st);
hipError_t mrtx_launch_resolve_rgb16(const float* accum, uint16_t* out, int64_t npix, uint32_t ns, float expo,
                                     const float* T16, hipStream_t st);
hipError_t mrtx_launch_pack(const float* accum, const float* hits, void* dst, int W, int H, int tw, int th,
                            int tiles_x, int n_tiles, int rank, int world, int slot0, int slots, const int32_t* list, int shift,
                            int with_hits, hipStream_t st);
hipError_t mrtx_launch_unpack(float* accum, float* hits, const void* src, int W, int H, int tw, int th,
                              int tiles_x, int n_tiles, int src_rank, int world, int slots, const int32_t* list, int shift,
                              int with_hits, hipStream_t st);
hipError_t mrtx_launch_unpack_all(float* accum, float* hits, const void* const* srcs, int W, int H, int tw, int th, int tiles_x,
                                  int n_tiles, int self, int world, int slots, const int32_t* list_all, int shift, int with_hits,
                                  hipStream_t st);
hipError_t mrtx_launch_zero_tiles(float* accum, float* hits, const int32_t* tiles, int n, int W, int H, int tw, int th,
                                  int tiles_x, int shift, hipStream_t st);
hipError_t mrtx_launch_ldem(const int16_t* src, float* dst, int h, int w, int d, unsigned int* max_bits,
                            hipStream_t st);
hipError_t mrtx_launch_synth_ldem(int16_t* dst, int h, int w, uint32_t seed, hipStream_t st);
hipError_t mrtx_launch_synth_color(uint32_t* dst, int h, int w, uint32_t seed, hipStream_t st);
hipError_t mrtx_launch_probe_latlon(const float* a, const float* b, const float* c, float* lat, float* lon, int n,
                                    hipStream_t st);
hipError_t mrtx_launch_pad_dem(const float* src, float* dst, int h, int w, hipStream_t st);
hipError_t mrtx_launch_mip(const float* dem_padded, int h, int w, float* mip, int mh, int mw, int shift, hipStream_t st);
hipError_t mrtx_launch_color_pairs(const uint32_t* src, void* dst, int h, int w, hipStream_t st);
hipError_t mrtx_launch_mip_pairs(const float* mip, float* out_pairs, int rows, int pitch, hipStream_t st);
hipError_t mrtx_launch_hmip(const float* mip, int mh, int mw, int shift, float* out, int hh, int hw, int hshift, int h, int w,
                            hipStream_t st);
hipError_t mrtx_launch_probe_stream(const void* src, int64_t n_pairs, float* out, hipStream_t st);
hipError_t mrtx_launch_probe_cr(uint32_t lo, uint64_t n, int which, unsigned long long* out2, hipStream_t st);
hipError_t mrtx_launch_illum(const FrameC& f, IllumC g, bool stats, hipStream_t st);
hipError_t mrtx_launch_illum_series(const FrameC& f, IllumSeriesC q, bool stats, hipStream_t st);
hipError_t mrtx_launch_horizon(const FrameC& f, HorizonC h, bool stats, hipStream_t st);
hipError_t mrtx_launch_horizon_sun(const FrameC& f, HorizonSunC q, hipStream_t st);
hipError_t mrtx_launch_horizon_raised(const FrameC& f, HorizonRaisedC q, bool stats, hipStream_t st);
hipError_t mrtx_launch_horizon_windows(const FrameC& f, HorizonWindowsC q, hipStream_t st);
hipError_t mrtx_launch_passes(const FrameC& f, PassesC q, int mode, hipStream_t st);
hipError_t mrtx_launch_occultation(const FrameC& f, OccultC q, hipStream_t st);
hipError_t mrtx_launch_power_budget(const FrameC& f, PowerC q, hipStream_t st);
hipError_t mrtx_launch_sight(const FrameC& f, SightC q, bool stats, hipStream_t st);
hipError_t mrtx_launch_thermal(const FrameC& f, const ThermalC& q, bool ext, hipStream_t st);
hipError_t mrtx_launch_view_hits(const FrameC& f, const ViewC& q, bool stats, hipStream_t st);
hipError_t mrtx_launch_scatter_flux(const ScatterC& q, hipStream_t st);
hipError_t mrtx_launch_horizon_mask(const FrameC& f, HorizonMaskC q, hipStream_t st);
hipError_t mrtx_launch_relief(const ReliefC& q, int tile, hipStream_t st);
hipError_t mrtx_launch_relief_share(const ShareC& q, hipStream_t st);
size_t mrtx_relief_tile_lds(int th, int tw, int ri, int rj);

// Host -> device copies that feed kernels of this context go through the context's OWN stream (hipStreamNonBlocking: the null
// stream does not order it) and are waited for before the host buffer is released, so copy and consumer are ordered by the
// stream itself.  (Introduced in round 3 on suspicion while a one-off fuzz mismatch was open; round 4 showed that mismatch to
// be a changed INPUT -- one word of the caller's colour-map array decremented by one before the upload,
// profiles/r04_seed601_case49.md -- so this is plain hygiene, not a fix of anything observed.)
static hipError_t h2d(mrtx_ctx* c, void* dst, const void* src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

namespace {

// Streams and events are POOLED per device and never destroyed while the process lives (MOONRT_POOL_STREAMS=0 switches back to
// create / destroy per context).  A context is cheap and short-lived in the tests (hundreds per process); the pool saves two
// runtime calls per object and, more to the point, keeps the HIP runtime's completion threads from ever working on a stream or
// event whose owner has gone (round 4: the harness's input guard caught a word of a host array being decremented by one while
// only the runtime's own threads could have been writing, profiles/r04_seed601_case49.md).
struct StreamPool {
    std::mutex mu;
    std::vector<hipStream_t> streams[16];
    std::vector<hipEvent_t> events[16];
};
StreamPool& pool() { static StreamPool* p = new StreamPool(); return *p; }     // leaked on purpose: outlives every context
// MOONRT_POOL_STREAMS: unset / 1 = pool both (default), 0 = neither, 2 = streams only, 3 = events only (the last two: diagnosis)
int pool_mode() { static const int m = std::getenv("MOONRT_POOL_STREAMS") ? std::atoi(std::getenv("MOONRT_POOL_STREAMS")) : 1; return m; }
bool pool_streams() { return pool_mode() == 1 || pool_mode() == 2; }
bool pool_events() { return pool_mode() == 1 || pool_mode() == 3; }

hipError_t get_stream(int dev, hipStream_t* out) {
    if (pool_streams() && dev >= 0 && dev < 16) {
        std::lock_guard<std::mutex> g(pool().mu);
        auto& v = pool().streams[dev];
        if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void put_stream(int dev, hipStream_t st) {
    if (!st) return;
    if (pool_streams() && dev >= 0 && dev < 16) { std::lock_guard<std::mutex> g(pool().mu); pool().streams[dev].push_back(st); }
    else (void)hipStreamDestroy(st);
}
hipError_t get_event(int dev, hipEvent_t* out) {
    if (pool_events() && dev >= 0 && dev < 16) {
        std::lock_guard<std::mutex> g(pool().mu);
        auto& v = pool().events[dev];
        if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
    }
    return hipEventCreate(out);
}
void put_event(int dev, hipEvent_t ev) {
    if (!ev) return;
    if (pool_events() && dev >= 0 && dev < 16) { std::lock_guard<std::mutex> g(pool().mu); pool().events[dev].push_back(ev); }
    else (void)hipEventDestroy(ev);
}

const double kPiD = 3.14159265358979323846;

void unit3(double v[3]) {
    const double l = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
}
void cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
uint32_t mix32h(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU;
    x ^= x >> 15; x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
void set_grid(GridC& g, int h, int w) {
    g.h = h; g.w = w;
    g.row_scale = (float)(-(double)h / kPiD);
    g.row_off = (float)(0.5 * (double)h - 0.5);
    g.col_scale = (float)((double)w / (2.0 * kPiD));
    g.col_off = (float)(0.5 * (double)w - 0.5);
    g.wf = (float)w;
}

// moon frame rows: east-90, lon-0, north.  u = north pole, v = longitude-0 direction
// (moon_renderer.py:621, :844-845; renderer_navigation.py:47-53)
static void moon_rows(const double u[3], const double v[3], double M[3][3]) {
    double ez[3] = {u[0], u[1], u[2]}, v0[3], ex[3];
    unit3(ez);
    const double dp = (v[0] * ez[0] + v[1] * ez[1]) + v[2] * ez[2];
    for (int i = 0; i < 3; i++) v0[i] = v[i] - dp * ez[i];
    unit3(v0);
    cross(ez, v0, ex);
    for (int j = 0; j < 3; j++) { M[0][j] = ex[j]; M[1][j] = v0[j]; M[2][j] = ez[j]; }
}
// D5's light constants: the light centre in the moon frame relative to the Moon centre, radius^2 and 2 x radiance.  build_frame
// and the per-epoch table of mrtx_illum_series both form them here, so that a series epoch and a set_light / set_moon_frame
// date give the same bits.
static void light_consts(const double M[3][3], const double center[3], const double pos[3], double radius, double radiance,
                         float Lb[3], float& rL2, float& rad2) {
    double lr[3];
    for (int i = 0; i < 3; i++) lr[i] = pos[i] - center[i];
    for (int i = 0; i < 3; i++) Lb[i] = (float)((M[i][0] * lr[0] + M[i][1] * lr[1]) + M[i][2] * lr[2]);
    rL2 = (float)(radius * radius);
    rad2 = (float)(2.0 * radiance);
}

// Scene (float64) -> per-launch constants.  DESIGN.md section 3.1 lists every formula; the oracle
// derives the same block on its own and tests compare the two float for float.
void build_frame(const mrtx_ctx* c, FrameC& f, FrameCold& k) {
    std::memset(&f, 0, sizeof f);
    std::memset(&k, 0, sizeof k);
    f.W = c->cfg.width; f.H = c->cfg.height;
    double wv[3], uv[3], vv[3];
    for (int i = 0; i < 3; i++) wv[i] = c->target[i] - c->eye[i];
    unit3(wv);
    cross(wv, c->up, uv); unit3(uv);
    cross(uv, wv, vv);
    const double th = std::tan(c->vfov * kPiD / 360.0);
    const double aspect = (double)f.W / (double)f.H;
    for (int i = 0; i < 3; i++) {
        k.Wd[i] = (float)wv[i];
        k.Ux[i] = (float)(uv[i] * (th * aspect));
        k.Vy[i] = (float)(vv[i] * th);
        k.oc[i] = c->eye[i] - c->center[i];
        k.centerf[i] = (float)c->center[i];
        k.eyef[i] = (float)c->eye[i];
    }
    k.two_over_w = (float)(2.0 / (double)f.W);
    k.two_over_h = (float)(2.0 / (double)f.H);
    k.cq = ((k.oc[0] * k.oc[0] + k.oc[1] * k.oc[1]) + k.oc[2] * k.oc[2]) - c->radius * c->radius;
    moon_rows(c->u, c->v, k.M);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) k.Mf[i][j] = (float)k.M[i][j];
    f.Rf = (float)c->radius;
    f.R2f = f.Rf * f.Rf;
    light_consts(k.M, c->center, c->light_pos, c->light_radius, c->light_radiance, k.Lb, k.rL2, k.rad2);
    k.sun_on = c->sun_radius > 0.0 ? 1 : 0;
    double sr[3];
    for (int i = 0; i < 3; i++) { sr[i] = c->sun_pos[i] - c->eye[i]; k.sc[i] = (float)sr[i]; }
    k.sun_cq = (float)(((sr[0] * sr[0] + sr[1] * sr[1]) + sr[2] * sr[2]) - c->sun_radius * c->sun_radius);
    k.sun_rad = (float)c->sun_radiance;
    {
        double sm[3];
        for (int i = 0; i < 3; i++) sm[i] = c->sun_pos[i] - c->center[i];
        for (int i = 0; i < 3; i++) k.Sb[i] = (float)((k.M[i][0] * sm[0] + k.M[i][1] * sm[1]) + k.M[i][2] * sm[2]);
        k.sun_r2 = (float)(c->sun_radius * c->sun_radius);
    }
    f.step = c->prm.marching_step;
    k.eps = c->prm.marching_step_eps;
    k.scene_eps = c->prm.scene_epsilon;
    f.nbis = 0;
    for (double wdt = (double)f.step; wdt > (double)k.eps && f.nbis < 24; wdt *= 0.5) f.nbis++;
    f.kmax = (((int)(2.0 * c->radius / (double)f.step) + 8) + 15) & ~15;   // multiple of the 16-step segment
    f.inv_step = 1.0f / f.step;
    f.polar_rho2 = (float)(0.04 * c->radius * c->radius);
    f.row_hi = std::nextafterf((float)c->dem_h, 0.0f);
    f.col_hi = std::nextafterf((float)c->dem_w, 0.0f);
    set_grid(f.gd, c->dem_h, c->dem_w);
    k.dlat_scale = (float)((double)c->dem_h / (2.0 * kPiD));
    k.dlon_scale = (float)((double)c->dem_w / (4.0 * kPiD));
    if (c->color) set_grid(k.gc, c->color_h, c->color_w);
    if (c->bg) {
        k.bg_h = c->bg_h; k.bg_w = c->bg_w;
        k.bg_row_scale = (float)(-(double)c->bg_h / kPiD);
        k.bg_row_off = (float)(0.5 * (double)c->bg_h);
        k.bg_col_scale = (float)((double)c->bg_w / (2.0 * kPiD));
        k.bg_col_off = (float)(0.5 * (double)c->bg_w);
    }
    k.key0 = mix32h(c->prm.seed ^ 0x9E3779B9u);
    k.path_seg_min = c->prm.path_seg_min; k.path_seg_max = c->prm.path_seg_max < 1 ? 1 : c->prm.path_seg_max;
    for (int i = 0; i < 3; i++) k.const_albedo[i] = c->prm.const_albedo[i];
    f.dem = c->dem; k.color = c->color; k.bg = c->bg;
    k.hmip = (c->prm.flags & MRTX_F_NO_SKIP) ? nullptr : c->hmip; k.hm_h = c->hm_h; k.hm_w = c->hm_w; k.hm_shift = c->hm_shift;
    k.hm_cell = (float)(1 << c->hm_shift);
    k.mip2 = (c->prm.flags & MRTX_F_NO_SKIP) ? nullptr : c->mip2; k.m2_pitch = c->m2_w + 2; k.m2_h = c->m2_h; k.m2_w = c->m2_w; k.m2_shift = c->m2_shift;
    k.hm_krow = (float)((double)c->dem_h / kPiD);
    k.hm_kcol = (float)(1.05 * (double)c->dem_w / (2.0 * kPiD));
    f.mip = c->mip; f.mip_pitch = c->mip_w + 2; f.mip_h = c->mip_h; f.mip_w = c->mip_w; f.mip_shift = c->mip_shift;
    f.dem_pitch = c->dem_w + 4;
    f.dem_maxidx = (uint32_t)((uint64_t)(c->dem_h + 4) * (uint64_t)(c->dem_w + 4) - 2);   // elements idx and idx+1 are read
    f.dem_wide = ((uint64_t)(c->dem_h + 4) * (uint64_t)(c->dem_w + 4) * MRTX_DEM_ELEM_BYTES > 0xFFFFFFFFull) ? 1 : 0;
    f.tile_w = c->cfg.tile_w; f.tile_h = c->cfg.tile_h;
    f.tiles_x = c->tiles_x; f.tiles_y = c->tiles_y; f.tile_shift = c->tile_shift;
    f.rank = c->cfg.rank; f.world = c->cfg.world; f.n_local_tiles = c->n_local;
    k.accum = c->accum; k.hits = c->hits; k.stats = c->stats_dev; k.stats_paths = c->stats_dev + 16;
    f.tile_list = nullptr; f.n_active = c->n_local;
}

// D11: (re)build the device copy of the overlay capsules (relative to the Moon centre) and their per-tile bins.
// A capsule is binned into every local tile its bounding sphere can project into (conservative: perspective
// stretch factor 1 + tan^2, +2 px), so the kernel's nearest-hit search over a bin equals the search over all.
int build_capsule_bins(mrtx_ctx* c) {
    const size_t n = c->caps_host.size() / 12;
    c->caps_off_host.assign((size_t)c->n_local + 1, 0);
    if (n == 0) return MRTX_OK;
    const int W = c->cfg.width, H = c->cfg.height;
    double wv[3], uv[3], vv[3];
    for (int i = 0; i < 3; i++) wv[i] = c->target[i] - c->eye[i];
    unit3(wv);
    cross(wv, c->up, uv); unit3(uv);
    cross(uv, wv, vv);
    const double th = std::tan(c->vfov * kPiD / 360.0), aspect = (double)W / (double)H;
    std::vector<float> rel(n * 12);
    std::vector<std::vector<int32_t>> bins((size_t)c->n_local);
    for (size_t k = 0; k < n; k++) {
        const float* p = &c->caps_host[12 * k];
        float* q = &rel[12 * k];
        for (int i = 0; i < 3; i++) {
            q[i] = (float)((double)p[i] - c->center[i]);
            q[4 + i] = (float)((double)p[4 + i] - c->center[i]);
        }
        q[3] = p[3]; q[7] = 0.0f; q[8] = p[8]; q[9] = p[9]; q[10] = p[10]; q[11] = 0.0f;
        double m[3], half = 0.0;
        for (int i = 0; i < 3; i++) { m[i] = 0.5 * ((double)p[i] + (double)p[4 + i]) - c->eye[i]; const double d = (double)p[4 + i] - (double)p[i]; half += d * d; }
        const double rho = 0.5 * std::sqrt(half) + (double)p[3];
        const double z = (m[0] * wv[0] + m[1] * wv[1]) + m[2] * wv[2];
        if (z + rho <= 1.0e-9) continue;                       // entirely behind the eye
        int tx0 = 0, tx1 = c->tiles_x - 1, ty0 = 0, ty1 = c->tiles_y - 1;
        if (z - rho > 1.0e-6) {
            const double x = (m[0] * uv[0] + m[1] * uv[1]) + m[2] * uv[2], y = (m[0] * vv[0] + m[1] * vv[1]) + m[2] * vv[2];
            const double tx = x / z, ty = y / z;               // tangents of the view angles
            const double px = (tx / (th * aspect) + 1.0) * 0.5 * W, py = (1.0 - ty / th) * 0.5 * H;
            const double pr = rho / (z - rho) / th * (0.5 * H) * (1.0 + tx * tx + ty * ty) * 1.05 + 2.0;
            const double fx0 = std::floor((px - pr) / c->cfg.tile_w), fx1 = std::floor((px + pr) / c->cfg.tile_w);
            const double fy0 = std::floor((py - pr) / c->cfg.tile_h), fy1 = std::floor((py + pr) / c->cfg.tile_h);
            if (fx1 < 0 || fy1 < 0 || fx0 > c->tiles_x - 1 || fy0 > c->tiles_y - 1) continue;
            tx0 = (int)std::fmax(fx0, 0.0); tx1 = (int)std::fmin(fx1, (double)c->tiles_x - 1);
            ty0 = (int)std::fmax(fy0, 0.0); ty1 = (int)std::fmin(fy1, (double)c->tiles_y - 1);
        }
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) {
                const int t = mrtx_tile_id(tx, ty, c->tiles_x, c->tile_shift);
                if (t % c->cfg.world == c->cfg.rank) bins[(size_t)(t / c->cfg.world)].push_back((int32_t)k);
            }
    }
    std::vector<int32_t> idx;
    for (int lt = 0; lt < c->n_local; lt++) {
        c->caps_off_host[(size_t)lt] = (int32_t)idx.size();
        idx.insert(idx.end(), bins[(size_t)lt].begin(), bins[(size_t)lt].end());
    }
    c->caps_off_host[(size_t)c->n_local] = (int32_t)idx.size();
    if (c->caps_dev_n < n) {
        if (c->caps_dev) { HIPCHK(c, hipFree(c->caps_dev)); c->caps_dev = nullptr; }
        HIPCHK(c, hipMalloc((void**)&c->caps_dev, n * 12 * sizeof(float)));
        c->caps_dev_n = n;
    }
    if (!c->caps_off_dev) HIPCHK(c, hipMalloc((void**)&c->caps_off_dev, ((size_t)c->n_local + 1) * sizeof(int32_t)));
    if (c->caps_idx_cap < idx.size() + 1) {
        if (c->caps_idx_dev) { HIPCHK(c, hipFree(c->caps_idx_dev)); c->caps_idx_dev = nullptr; }
        c->caps_idx_cap = idx.size() * 2 + 64;
        HIPCHK(c, hipMalloc((void**)&c->caps_idx_dev, c->caps_idx_cap * sizeof(int32_t)));
    }
    HIPCHK(c, h2d(c, c->caps_dev, rel.data(), n * 12 * sizeof(float)));
    HIPCHK(c, h2d(c, c->caps_off_dev, c->caps_off_host.data(), c->caps_off_host.size() * sizeof(int32_t)));
    if (!idx.empty()) HIPCHK(c, h2d(c, c->caps_idx_dev, idx.data(), idx.size() * sizeof(int32_t)));
    return MRTX_OK;
}

// Host-side sky cull (exact): with no environment texture a pixel whose samples all miss the Moon's bounding
// sphere and the Sun disk is identically zero (radiance, coverage and hit record).  A tile is kept unless the
// cone of its view directions (tile-centre direction, half-angle = largest corner angle + 5 % + 1e-4 rad, pixel
// extents included so every jittered sample is inside) is disjoint from both objects' cones as seen from the eye.
// Returns the local tile indices to render and the number of pixels culled.
// With an environment texture bound nothing is culled, but the classification still pays: the tiles that can only see
// the sky go to the END of the list (n_front = how many can see more), so that the deferred-path pipeline -- buffers sized
// per wave-job, persistent waves walking every group of blocks -- is set up for the Moon's tiles only and the sky gets one
// plain launch (cfg3 with the reference's star map: 8 100 tiles, 3 056 of them with the Moon in view).
void cull_tiles(const mrtx_ctx* c, int rank, std::vector<int32_t>& keep, uint64_t& culled_px, int* n_front = nullptr) {
    keep.clear(); culled_px = 0;
    std::vector<int32_t> sky;
    const int n_local = (c->n_tiles - rank + c->cfg.world - 1) / c->cfg.world;
    const bool own = rank == c->cfg.rank;   // overlay bins exist for the own tiles only (gather_layout() switches off with overlays)
    const int W = c->cfg.width, H = c->cfg.height;
    double wv[3], uv[3], vv[3];
    for (int i = 0; i < 3; i++) wv[i] = c->target[i] - c->eye[i];
    unit3(wv);
    cross(wv, c->up, uv); unit3(uv);
    cross(uv, wv, vv);
    const double th = std::tan(c->vfov * kPiD / 360.0), aspect = (double)W / (double)H;
    struct Cone { double ax[3]; double half; bool all; bool on; };
    Cone cones[2];
    const double* centres[2] = {c->center, c->sun_pos};
    const double radii[2] = {c->radius, c->sun_radius};
    for (int k = 0; k < 2; k++) {
        Cone& cn = cones[k];
        cn.on = radii[k] > 0.0; cn.all = false; cn.half = 0.0;
        double d[3] = {centres[k][0] - c->eye[0], centres[k][1] - c->eye[1], centres[k][2] - c->eye[2]};
        const double dist = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (!cn.on) continue;
        if (dist <= radii[k] * 1.0001) { cn.all = true; continue; }
        for (int i = 0; i < 3; i++) cn.ax[i] = d[i] / dist;
        cn.half = std::asin(radii[k] / dist);
    }
    const bool everything = cones[0].all || cones[1].all;
    const bool sky_rendered = c->bg != nullptr;
    auto dir = [&](double px, double py, double o[3]) {
        const double sx = px * 2.0 / W - 1.0, sy = 1.0 - py * 2.0 / H;
        for (int i = 0; i < 3; i++) o[i] = wv[i] + sx * (uv[i] * (th * aspect)) + sy * (vv[i] * th);
        unit3(o);
    };
    auto ang = [](const double a[3], const double b[3]) {
        double dp = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
        dp = dp > 1.0 ? 1.0 : (dp < -1.0 ? -1.0 : dp);
        return std::acos(dp);
    };
    // Longest first: a pixel on the limb marches ~20x longer than one at the disc centre, and a launch ends with its
    // slowest late wave, so tiles on the limb ring (0.85 .. 1 of the disc's angular radius) go to the FRONT of the
    // list; raster order is kept inside both classes (neighbouring tiles share DEM lines in L2 / Infinity Cache).
    std::vector<int32_t> ring;
    const bool sort_ring = !(c->prm.flags & MRTX_F_NO_SORT) && cones[0].on && !cones[0].all;
    for (int lt = 0; lt < n_local; lt++) {
        const int t = lt * c->cfg.world + rank;
        int ttx, tty;
        mrtx_tile_xy(t, c->tiles_x, c->tile_shift, ttx, tty);
        const int x0 = ttx * c->cfg.tile_w, y0 = tty * c->cfg.tile_h;
        const int x1 = x0 + c->cfg.tile_w < W ? x0 + c->cfg.tile_w : W, y1 = y0 + c->cfg.tile_h < H ? y0 + c->cfg.tile_h : H;
        bool need = everything;
        if (!need) {
            double d0[3], dc[3];
            dir(0.5 * (x0 + x1), 0.5 * (y0 + y1), d0);
            double gamma = 0.0;
            const double cx[4] = {(double)x0, (double)x1, (double)x0, (double)x1}, cy[4] = {(double)y0, (double)y0, (double)y1, (double)y1};
            for (int k = 0; k < 4; k++) { dir(cx[k], cy[k], dc); const double a = ang(d0, dc); gamma = a > gamma ? a : gamma; }
            gamma = gamma * 1.05 + 1.0e-4;
            for (int k = 0; k < 2; k++)
                if (cones[k].on && ang(d0, cones[k].ax) <= cones[k].half + gamma) need = true;
        }
        if (!need && own && !c->caps_off_host.empty() && c->caps_off_host[(size_t)lt + 1] > c->caps_off_host[(size_t)lt]) need = true;   // overlay tubes here
        if (need) {
            bool on_ring = false;
            if (sort_ring) {
                double d0[3];
                dir(0.5 * (x0 + x1), 0.5 * (y0 + y1), d0);
                const double rho = ang(d0, cones[0].ax) / cones[0].half;
                on_ring = rho >= 0.85 && rho <= 1.05;
            }
            (on_ring ? ring : keep).push_back(lt);
        } else if (sky_rendered) {
            sky.push_back(lt);
        } else {
            culled_px += (uint64_t)(x1 - x0) * (uint64_t)(y1 - y0);
        }
    }
    keep.insert(keep.begin(), ring.begin(), ring.end());
    if (n_front) *n_front = (int)keep.size();
    keep.insert(keep.end(), sky.begin(), sky.end());
}

int check_vec(const double* p) {
    if (!p) return 0;
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(p[i])) return 0;
    return 1;
}

}  // namespace

// ---- What the host units share (mrtx_host.h): defined here, used by mrtx_lattice_api.hip as well ---------------------------
int mrtx_host::fail(mrtx_ctx* c, int code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

bool mrtx_host::spans_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

// grow one of the stage's device buffers to at least `bytes`
int mrtx_host::stage_buffer(mrtx_ctx* c, float*& p, size_t& cap, size_t bytes) {
    if (bytes > cap) {
        if (p) { HIPCHK(c, hipFree(p)); p = nullptr; cap = 0; }
        HIPCHK(c, hipMalloc((void**)&p, bytes));
        cap = bytes;
    }
    return MRTX_OK;
}

// The launch's tables in one device block, c->illum_tab: each segment at an offset rounded up to 16 bytes (the float4 loads
// of the epoch lights), copied straight from the caller's memory, which must stay put until stage_finish.  dev[i] = segment
// i's device address.  Called after stage_out, so that every buffer is grown before the first copy is queued.
int mrtx_host::stage_tables(mrtx_ctx* c, std::initializer_list<HostSeg> segs, float** dev) {
    size_t words = 0;
    for (const HostSeg& s : segs) words += (s.n + 3) & ~(size_t)3;
    const int rc = stage_buffer(c, c->illum_tab, c->illum_tab_bytes, std::max(words * 4, (size_t)16));
    if (rc != MRTX_OK) return rc;
    float* d = c->illum_tab;
    for (const HostSeg& s : segs) {
        if (s.n) HIPCHK(c, hipMemcpyAsync(d, s.p, s.n * 4, hipMemcpyHostToDevice, c->stream));
        *dev++ = d;
        d += (s.n + 3) & ~(size_t)3;
    }
    return MRTX_OK;
}

// where the launch writes: the caller's dev_out, or else c->illum_out grown to `bytes` (read back by stage_finish)
int mrtx_host::stage_out(mrtx_ctx* c, void*& dev_out, size_t bytes) {
    if (dev_out) return MRTX_OK;
    const int rc = stage_buffer(c, c->illum_out, c->illum_out_bytes, bytes);
    dev_out = c->illum_out;
    return rc;
}

// right before the launch: the cold block (if any) and zeroed counters (if asked) queued, then the start event
int mrtx_host::stage_start(mrtx_ctx* c, const FrameCold* cold, bool zero) {
    if (cold) HIPCHK(c, hipMemcpyAsync(c->illum_cold, cold, sizeof *cold, hipMemcpyHostToDevice, c->stream));
    if (zero) HIPCHK(c, hipMemsetAsync(c->illum_stats, 0, 16 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    return MRTX_OK;
}

// right after the launch: the end event, wait, time, read back, counters (rays: reported as shadow_rays or bounce_rays)
int mrtx_host::stage_finish(mrtx_ctx* c, const void* dev_out, float* host_out, size_t out_bytes, MrtxStats* out, StageRays rays) {
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));     // also: the pageable tables are no longer read
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (host_out) HIPCHK(c, hipMemcpy(host_out, dev_out, out_bytes, hipMemcpyDeviceToHost));
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->kernel_ms = ms;
        out->launches = 1;
        if (rays != kNoRays) {
            unsigned long long h[16];
            HIPCHK(c, hipMemcpy(h, c->illum_stats, sizeof h, hipMemcpyDeviceToHost));
            (rays == kBounceRays ? out->bounce_rays : out->shadow_rays) = h[rays];
            out->height_samples = h[3]; out->dem_fetches = h[6]; out->mip_fetches = h[7];
        }
    }
    return MRTX_OK;
}

extern "C" {

int mrtx_abi_version(void) { return MRTX_ABI_VERSION; }

int mrtx_get_config(mrtx_ctx* c, MrtxConfig* out) {
    if (!c || !out) return MRTX_E_INVALID;
    *out = c->cfg;      // mrtx_create filled the defaults in
    return MRTX_OK;
}

void mrtx_default_params(MrtxParams* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->scene_epsilon = 1.0e-4f;      // moon_renderer.py:99
    p->marching_step = 5.0e-3f;      // :100
    p->marching_step_eps = 3.0e-4f;  // :101
    p->tonemap_exposure = 0.9f;      // :598
    p->tonemap_gamma = 2.2f;
    p->path_seg_min = 2; p->path_seg_max = 4;  // :583
    p->spp_per_launch = 64; p->max_spp = 64;   // :130
    p->seed = 1;
    p->const_albedo[0] = p->const_albedo[1] = p->const_albedo[2] = 75.0f / 255.0f;  // lut[128], gamma 2.2
    p->flags = 0;   // production kernels; MRTX_F_COUNT_STATS selects the counting instantiations (2-3x slower)
}

int mrtx_create(const MrtxConfig* cfg, mrtx_ctx** out) {
    if (!cfg || !out) return MRTX_E_INVALID;
    *out = nullptr;
    if (cfg->width < 1 || cfg->height < 1 || cfg->width > 32768 || cfg->height > 32768) return MRTX_E_INVALID;
    if (cfg->world < 1 || cfg->rank < 0 || cfg->rank >= cfg->world) return MRTX_E_INVALID;
    mrtx_ctx* c = new (std::nothrow) mrtx_ctx();
    if (!c) return MRTX_E_NOMEM;
    c->cfg = *cfg;
    // default tile: 16 x 16 on one GPU -- the sky cull and the limb-first launch order work at tile granularity, and the finer
    // tile keeps ~2 % of cfg3's waves (all-sky pixel blocks along the limb) off the GPU: 23.7 ms against 24.2 with 32 x 32 (direct
    // frame 12.7 / 13.2; gpurun_out/r3m/tile1.log), and for two ranks (slowest rank 12.28 / 12.49 ms); 32 x 32 from four ranks up
    // (world 4: 6.41 against 6.60 ms, world 8: 3.51 against 3.76: a rank's lattice of small tiles loses L2 locality)
    const int dflt = c->cfg.world > 2 ? 32 : 16;
    if (c->cfg.tile_w <= 0) c->cfg.tile_w = dflt;
    if (c->cfg.tile_h <= 0) c->cfg.tile_h = dflt;
    if ((c->cfg.tile_w & 15) || (c->cfg.tile_h & 15)) { delete c; return MRTX_E_INVALID; }
    mrtx_default_params(&c->prm);
    {   // tuning knobs of the deferred path stage (measurement aid; the defaults are what bench.py times)
        const char* e;
        if ((e = std::getenv("MOONRT_PATH_REFILL")) && std::atoi(e) >= -64 && std::atoi(e) <= 64) c->path_refill = std::atoi(e);
        if ((e = std::getenv("MOONRT_PATH_SEGMIN")) && std::atoi(e) >= -64 && std::atoi(e) <= 64) c->path_segmin = std::atoi(e);
        if ((e = std::getenv("MOONRT_PATH_HITMIN")) && std::atoi(e) >= -64 && std::atoi(e) <= 64) c->path_hitmin = std::atoi(e);
        if ((e = std::getenv("MOONRT_PATH_NSUB")) && std::atoi(e) >= 1 && std::atoi(e) <= 16) c->path_nsub = std::atoi(e);
        if ((e = std::getenv("MOONRT_PATH_GRP")) && std::atoi(e) >= 0 && std::atoi(e) <= 5) c->path_grp_log2 = std::atoi(e);   // + njobs_log2 (<= 1) <= 6: 64 chunks per group
        if ((e = std::getenv("MOONRT_PATH_MAX_GB")) && std::atof(e) > 0.0) { c->path_budget_bytes = (uint64_t)(std::atof(e) * 1073741824.0); c->path_budget_env = true; }
        if ((e = std::getenv("MOONRT_PATH_WAVES")) && std::atoi(e) >= 8 * c->path_nsub) c->path_waves_env = std::atoi(e) / 8 * 8;   // every work counter needs a consumer (read after MOONRT_PATH_NSUB)
        if ((e = std::getenv("MOONRT_PATH_QUEUE_MIN")) && std::atof(e) >= 0.0) c->path_queue_min = (uint64_t)std::atof(e);
        if ((e = std::getenv("MOONRT_TEST_PATH_NOMEM")) && std::atoi(e) == 1) c->path_alloc_fail_test = true;
        if ((e = std::getenv("MOONRT_PATH_OVERLAP")) && std::atoi(e) >= 0 && std::atoi(e) <= 64) c->path_overlap = std::atoi(e) == 1 ? 0 : std::atoi(e);
        if ((e = std::getenv("MOONRT_PATH_OVERLAP_WAVES")) && std::atoi(e) >= 8 * c->path_nsub) c->path_overlap_waves = std::atoi(e) / 8 * 8;
    }
    c->tiles_x = (cfg->width + c->cfg.tile_w - 1) / c->cfg.tile_w;
    c->tiles_y = (cfg->height + c->cfg.tile_h - 1) / c->cfg.tile_h;
    c->n_tiles = c->tiles_x * c->tiles_y;
    c->tile_shift = mrtx_tile_shift(cfg->world);
    c->slots = (c->n_tiles + cfg->world - 1) / cfg->world;
    c->n_local = (c->n_tiles - cfg->rank + cfg->world - 1) / cfg->world;
    *out = c;  // from here on the caller can read mrtx_last_error and must destroy
    const size_t fb = (size_t)cfg->width * cfg->height * 16;
    HIPCHK(c, hipSetDevice(cfg->device));
    HIPCHK(c, get_stream(cfg->device, &c->stream));
    HIPCHK(c, get_event(cfg->device, &c->ev0));
    HIPCHK(c, get_event(cfg->device, &c->ev1));
    HIPCHK(c, hipMalloc((void**)&c->accum, fb));
    HIPCHK(c, hipMalloc((void**)&c->hits, fb));
    HIPCHK(c, hipMalloc(&c->scratch, fb));
    HIPCHK(c, hipMalloc((void**)&c->stats_dev, 32 * sizeof(unsigned long long)));   // [0..15] render_kernel (+ watchdog), [16..31] path_kernel
    HIPCHK(c, hipMalloc((void**)&c->cold_dev, sizeof(FrameCold)));
    HIPCHK(c, hipMalloc((void**)&c->tile_list_dev, (size_t)(c->n_local > 0 ? c->n_local : 1) * sizeof(int32_t)));
    HIPCHK(c, hipMemsetAsync(c->accum, 0, fb, c->stream));
    HIPCHK(c, hipMemsetAsync(c->hits, 0, fb, c->stream));
    HIPCHK(c, hipMemsetAsync(c->stats_dev, 0, 32 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MRTX_OK;
}

void mrtx_destroy(mrtx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->accum) (void)hipFree(c->accum);
    if (c->hits) (void)hipFree(c->hits);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->tone8_dev) (void)hipFree(c->tone8_dev);
    if (c->tone16_dev) (void)hipFree(c->tone16_dev);
    if (c->stats_dev) (void)hipFree(c->stats_dev);
    if (c->cold_dev) (void)hipFree(c->cold_dev);
    if (c->caps_dev) (void)hipFree(c->caps_dev);
    if (c->caps_off_dev) (void)hipFree(c->caps_off_dev);
    if (c->caps_idx_dev) (void)hipFree(c->caps_idx_dev);
    if (c->tile_list_dev) (void)hipFree(c->tile_list_dev);
    if (c->act_dev) (void)hipFree(c->act_dev);
    if (c->stale_dev) (void)hipFree(c->stale_dev);
    if (c->path_rec) (void)hipFree(c->path_rec);
    if (c->path_meta) (void)hipFree(c->path_meta);
    if (c->path_npaths) (void)hipFree(c->path_npaths);
    if (c->path_ctr) (void)hipFree(c->path_ctr);
    if (c->wd_host) (void)hipHostFree(c->wd_host);
    for (hipEvent_t e : c->evs) put_event(c->cfg.device, e);
    if (c->dem) (void)hipFree(c->dem);
    if (c->mip) (void)hipFree(c->mip);
    if (c->hmip) (void)hipFree(c->hmip);
    if (c->mip2) (void)hipFree(c->mip2);
    if (c->color) (void)hipFree(c->color);
    if (c->bg) (void)hipFree(c->bg);
    if (c->overlay) (void)hipFree(c->overlay);
    if (c->illum_cold) (void)hipFree(c->illum_cold);
    if (c->illum_stats) (void)hipFree(c->illum_stats);
    if (c->illum_tab) (void)hipFree(c->illum_tab);
    if (c->illum_out) (void)hipFree(c->illum_out);
    if (c->trav_buf) (void)hipFree(c->trav_buf);
    if (c->stream2) { (void)hipStreamSynchronize(c->stream2); put_stream(c->cfg.device, c->stream2); }
    put_event(c->cfg.device, c->ov_done[0]); put_event(c->cfg.device, c->ov_done[1]); put_event(c->cfg.device, c->ov_join);
    put_event(c->cfg.device, c->ev0);
    put_event(c->cfg.device, c->ev1);
    put_stream(c->cfg.device, c->stream);      // synchronised above
    delete c;
}

const char* mrtx_last_error(mrtx_ctx* c) { return c ? c->err.c_str() : "null context"; }

// The context keeps its own PADDED copy of the DEM (see dem_march() in mrtx_march.h).
static int ingest_dem(mrtx_ctx* c, const float* dev_src, int32_t h, int32_t w) {
    if (c->dem) { HIPCHK(c, hipFree(c->dem)); }
    c->dem = nullptr; c->dem_h = c->dem_w = 0;
    const size_t bytes = (size_t)(h + 4) * (size_t)(w + 4) * MRTX_DEM_ELEM_BYTES;
    HIPCHK(c, hipMalloc((void**)&c->dem, bytes));
    HIPCHK(c, mrtx_launch_pad_dem(dev_src, c->dem, h, w, c->stream));
    if (c->mip) { HIPCHK(c, hipFree(c->mip)); }
    c->mip = nullptr; c->mip_shift = 0;   // (re)built by mrtx_render for the march step in force
    if (c->hmip) { HIPCHK(c, hipFree(c->hmip)); }
    c->hmip = nullptr;
    if (c->mip2) { HIPCHK(c, hipFree(c->mip2)); }
    c->mip2 = nullptr;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dem_h = h; c->dem_w = w;
    return MRTX_OK;
}
// The max-mip cell must cover a whole 16-step segment (plus tap margins) so that a segment's footprint touches at
// most 2 x 2 cells: cell = 2^shift >= 16*step/texel + 3.5, clamped to [16, 1024] texels.
static int ensure_mip(mrtx_ctx* c) {
    const double texel = std::fmin(kPiD * c->radius / (double)c->dem_h, 2.0 * kPiD * c->radius / (double)c->dem_w);
    const double span = 16.0 * (double)c->prm.marching_step / texel + 3.5;   // + the (-1, +2) tap margins of seg_setup
    int shift = 4;
    while ((1 << shift) < span && shift < 10) shift++;
    if (c->mip && c->mip_shift == shift) return MRTX_OK;
    if (c->mip) { HIPCHK(c, hipFree(c->mip)); }
    c->mip = nullptr;
    if (c->hmip) { HIPCHK(c, hipFree(c->hmip)); }
    c->hmip = nullptr;
    if (c->mip2) { HIPCHK(c, hipFree(c->mip2)); }
    c->mip2 = nullptr;
    const int cell = 1 << shift;
    c->mip_h = (c->dem_h + cell - 1) / cell; c->mip_w = (c->dem_w + cell - 1) / cell;
    const size_t cells = (size_t)(c->mip_h + 2) * (c->mip_w + 2);
    float* plain = nullptr;
    HIPCHK(c, hipMalloc((void**)&plain, cells * sizeof(float)));
    hipError_t e = hipMalloc((void**)&c->mip, (cells + 1) * 2 * sizeof(float));   // row pairs + one element of slack for the 16-byte load
    if (e == hipSuccess) e = mrtx_launch_mip(c->dem, c->dem_h, c->dem_w, plain, c->mip_h, c->mip_w, shift, c->stream);
    if (e == hipSuccess) e = mrtx_launch_mip_pairs(plain, c->mip, c->mip_h + 2, c->mip_w + 2, c->stream);
    c->hm_shift = shift + 3;
    c->hm_h = (c->dem_h + (cell << 3) - 1) / (cell << 3); c->hm_w = (c->dem_w + (cell << 3) - 1) / (cell << 3);
    if (e == hipSuccess) e = hipMalloc((void**)&c->hmip, (size_t)c->hm_h * c->hm_w * sizeof(float));
    if (e == hipSuccess) e = mrtx_launch_hmip(plain, c->mip_h, c->mip_w, shift, c->hmip, c->hm_h, c->hm_w, c->hm_shift, c->dem_h, c->dem_w, c->stream);
    // medium max-mip: the same cell maxima (dilated by the two-texel tap border) at a quarter of the cell size -- 16 texels at cfg3,
    // 17 MB: what path_kernel tests the steps of a segment against before it fetches the DEM for them
    c->m2_shift = shift - MRTX_M2_DELTA < 2 ? 2 : shift - MRTX_M2_DELTA;
    if ((MRTX_PATH_MIP2 | MRTX_SEG_MASK) != 0) {
        const int c2 = 1 << c->m2_shift;
        c->m2_h = (c->dem_h + c2 - 1) / c2; c->m2_w = (c->dem_w + c2 - 1) / c2;
        if (e == hipSuccess) e = hipMalloc((void**)&c->mip2, (size_t)(c->m2_h + 2) * (size_t)(c->m2_w + 2) * sizeof(float));
        if (e == hipSuccess) e = mrtx_launch_mip(c->dem, c->dem_h, c->dem_w, c->mip2, c->m2_h, c->m2_w, c->m2_shift, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(plain);
    HIPCHK(c, e);
    c->mip_shift = shift;
    return MRTX_OK;
}

int mrtx_upload_dem(mrtx_ctx* c, const float* host, int32_t h, int32_t w) {
    if (!c) return MRTX_E_INVALID;
    if (!host || h < 2 || w < 2) return fail(c, MRTX_E_INVALID, "DEM must be a float32 (h>=2, w>=2) array");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    float* stage = nullptr;
    const size_t bytes = (size_t)h * w * sizeof(float);
    HIPCHK(c, hipMalloc((void**)&stage, bytes));
    hipError_t e = h2d(c, stage, host, bytes);
    int rc = e == hipSuccess ? ingest_dem(c, stage, h, w) : fail(c, MRTX_E_DEVICE, "hipMemcpy H2D: %s", hipGetErrorString(e));
    (void)hipFree(stage);
    return rc;
}
int mrtx_bind_dem_device(mrtx_ctx* c, const void* dev, int32_t h, int32_t w) {
    if (!c) return MRTX_E_INVALID;
    if (!dev || h < 2 || w < 2) return fail(c, MRTX_E_INVALID, "bad device DEM");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return ingest_dem(c, (const float*)dev, h, w);
}
// The context keeps the colour map in ROW PAIRS (color_pair_kernel): 8 bytes per texel, (h+1) x (w+4) elements + slack.
static int ingest_color(mrtx_ctx* c, const void* dev_src, int32_t h, int32_t w) {
    if (c->color) { HIPCHK(c, hipFree(c->color)); }
    c->color = nullptr; c->color_h = c->color_w = 0;
    if (!dev_src) return MRTX_OK;
    const size_t elems = (size_t)(h + 1) * (size_t)(w + 4) + 1;
    HIPCHK(c, hipMalloc((void**)&c->color, elems * 8));
    HIPCHK(c, mrtx_launch_color_pairs((const uint32_t*)dev_src, c->color, h, w, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->color_h = h; c->color_w = w;
    return MRTX_OK;
}
int mrtx_upload_color(mrtx_ctx* c, const uint8_t* rgba, int32_t h, int32_t w) {
    if (!c) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!rgba) return ingest_color(c, nullptr, 0, 0);
    if (h < 2 || w < 2) return fail(c, MRTX_E_INVALID, "colour texture must be (h>=2, w>=2, 4) uint8");
    const size_t bytes = (size_t)h * w * 4;
    void* tmp = nullptr;
    HIPCHK(c, hipMalloc(&tmp, bytes));
    hipError_t e = h2d(c, tmp, rgba, bytes);
    int rc = MRTX_OK;
    if (e == hipSuccess) rc = ingest_color(c, tmp, h, w);
    (void)hipFree(tmp);
    HIPCHK(c, e);
    return rc;
}
int mrtx_bind_color_device(mrtx_ctx* c, const void* dev, int32_t h, int32_t w) {
    if (!c) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (dev && (h < 2 || w < 2)) return fail(c, MRTX_E_INVALID, "bad device colour texture");
    return ingest_color(c, dev, h, w);   // the caller's buffer is read once; the context keeps its own row-pair copy
}
int mrtx_upload_background(mrtx_ctx* c, const uint8_t* rgba, int32_t h, int32_t w) {
    if (!c) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->bg) { HIPCHK(c, hipFree(c->bg)); }
    c->bg = nullptr; c->bg_h = c->bg_w = 0;
    c->scene_version++;
    if (!rgba) return MRTX_OK;
    if (h < 1 || w < 1) return fail(c, MRTX_E_INVALID, "background must be (h>=1, w>=1, 4) uint8");
    const size_t bytes = (size_t)h * w * 4;
    HIPCHK(c, hipMalloc((void**)&c->bg, bytes));
    HIPCHK(c, h2d(c, c->bg, rgba, bytes));
    c->bg_h = h; c->bg_w = w;
    c->scene_version++;
    return MRTX_OK;
}

int mrtx_upload_overlay(mrtx_ctx* c, const uint8_t* rgba, int32_t h, int32_t w) {
    if (!c) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!rgba) {
        if (c->overlay) { HIPCHK(c, hipFree(c->overlay)); }
        c->overlay = nullptr;
        return MRTX_OK;
    }
    if (h != c->cfg.height || w != c->cfg.width) return fail(c, MRTX_E_INVALID, "the overlay texture must match the frame (%d x %d)", c->cfg.width, c->cfg.height);
    const size_t bytes = (size_t)h * w * 4;
    if (!c->overlay) HIPCHK(c, hipMalloc((void**)&c->overlay, bytes));
    HIPCHK(c, h2d(c, c->overlay, rgba, bytes));
    return MRTX_OK;
}

int mrtx_set_params(mrtx_ctx* c, const MrtxParams* p) {
    if (!c || !p) return MRTX_E_INVALID;
    const uint32_t S = p->spp_per_launch;
    if (S == 0 || S > 64 || (S & (S - 1))) return fail(c, MRTX_E_INVALID, "spp_per_launch must be 1,2,4,...,64");
    if (!(p->marching_step > 0.0f) || !(p->marching_step_eps > 0.0f) || !(p->scene_epsilon >= 0.0f))
        return fail(c, MRTX_E_INVALID, "marching_step, marching_step_eps must be > 0 and scene_epsilon >= 0");
    if (!(p->tonemap_gamma > 0.0f)) return fail(c, MRTX_E_INVALID, "tonemap_gamma must be > 0");
    if (S != c->prm.spp_per_launch && c->blocks_done != 0)
        return fail(c, MRTX_E_STATE, "spp_per_launch cannot change inside an accumulation cycle; reset first");
    if (p->flags != c->prm.flags) c->scene_version++;   // MRTX_F_NO_CULL changes the cull and the gather layout
    c->prm = *p;
    return MRTX_OK;
}

int mrtx_set_camera(mrtx_ctx* c, const double eye[3], const double target[3], const double up[3], double vfov) {
    if (!c) return MRTX_E_INVALID;
    if (!check_vec(eye) || !check_vec(target) || !check_vec(up) || !(vfov > 0.0 && vfov < 180.0))
        return fail(c, MRTX_E_INVALID, "bad camera");
    double w[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]}, x[3];
    cross(w, up, x);
    if (!((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2] > 0.0)) return fail(c, MRTX_E_INVALID, "camera up is parallel to the view axis");
    for (int i = 0; i < 3; i++) { c->eye[i] = eye[i]; c->target[i] = target[i]; c->up[i] = up[i]; }
    c->vfov = vfov;
    c->scene_version++;
    return MRTX_OK;
}
int mrtx_set_moon_frame(mrtx_ctx* c, const double center[3], double radius, const double u[3], const double v[3]) {
    if (!c) return MRTX_E_INVALID;
    if (!check_vec(center) || !check_vec(u) || !check_vec(v) || !(radius > 0.0)) return fail(c, MRTX_E_INVALID, "bad moon frame");
    double x[3];
    cross(u, v, x);
    if (!((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2] > 0.0)) return fail(c, MRTX_E_INVALID, "moon u and v are parallel");
    for (int i = 0; i < 3; i++) { c->center[i] = center[i]; c->u[i] = u[i]; c->v[i] = v[i]; }
    c->radius = radius;
    c->moon_set = true;
    c->scene_version++;
    return MRTX_OK;
}
int mrtx_set_light(mrtx_ctx* c, const double pos[3], double radius, double radiance) {
    if (!c) return MRTX_E_INVALID;
    if (!check_vec(pos) || !(radius >= 0.0) || !(radiance >= 0.0)) return fail(c, MRTX_E_INVALID, "bad light");
    for (int i = 0; i < 3; i++) c->light_pos[i] = pos[i];
    c->light_radius = radius; c->light_radiance = radiance;
    c->light_set = true;
    return MRTX_OK;
}
int mrtx_set_sun_disk(mrtx_ctx* c, const double pos[3], double radius, double radiance) {
    if (!c) return MRTX_E_INVALID;
    if (!check_vec(pos) || !std::isfinite(radius) || !(radiance >= 0.0)) return fail(c, MRTX_E_INVALID, "bad sun disk");
    for (int i = 0; i < 3; i++) c->sun_pos[i] = pos[i];
    c->sun_radius = radius; c->sun_radiance = radiance;
    c->scene_version++;
    return MRTX_OK;
}

int mrtx_set_capsules(mrtx_ctx* c, const float* caps12, int32_t n) {
    if (!c || n < 0 || (n > 0 && !caps12)) return MRTX_E_INVALID;
    for (int64_t i = 0; i < (int64_t)n * 12; i++)
        if (!std::isfinite(caps12[i])) return fail(c, MRTX_E_INVALID, "non-finite value in capsule %lld", (long long)(i / 12));
    c->caps_host.assign(caps12, caps12 + (size_t)n * 12);
    c->scene_version++;
    return MRTX_OK;
}

int mrtx_reset_accum(mrtx_ctx* c) {
    if (!c) return MRTX_E_INVALID;
    c->blocks_done = 0;
    c->path_nomem_chunks = 0;            // a new accumulation cycle may try the hand-over allocation again
    return MRTX_OK;
}

static int gather_layout(mrtx_ctx* c);
// slots [a, b) of part `part` of `n_parts` over n entries: contiguous, sizes differ by at most one
static void part_range(int n, int part, int n_parts, int& a, int& b) {
    a = (int)((int64_t)n * part / n_parts);
    b = (int)((int64_t)n * (part + 1) / n_parts);
}

int mrtx_render(mrtx_ctx* c, int32_t n_blocks, MrtxStats* out) { return mrtx_render_part(c, n_blocks, 0, 1, out); }

int mrtx_render_part(mrtx_ctx* c, int32_t n_blocks, int32_t part, int32_t n_parts, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (n_blocks < 1) return fail(c, MRTX_E_INVALID, "n_blocks must be >= 1");
    if (n_parts < 1 || part < 0 || part >= n_parts) return fail(c, MRTX_E_INVALID, "bad part %d of %d", part, n_parts);
    if (n_parts > 1 && (c->prm.flags & MRTX_F_NO_CULL)) return fail(c, MRTX_E_STATE, "parts need the tile list (MRTX_F_NO_CULL is set)");
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!(c->prm.flags & MRTX_F_NO_SKIP)) { const int rc_ = ensure_mip(c); if (rc_ != MRTX_OK) return rc_; }
    if (c->caps_version != c->scene_version) {   // overlay bins follow the camera / moon frame / capsule list
        const int rc_ = build_capsule_bins(c);
        if (rc_ != MRTX_OK) return rc_;
        c->caps_version = c->scene_version;
        c->cull_version = 0;   // the sky cull depends on the bins
    }
    FrameC f;
    FrameCold cold;
    std::memset(&cold, 0, sizeof cold);      // padding included: the block is compared bytewise below
    build_frame(c, f, cold);
    f.cold = c->cold_dev;
    cold.caps = c->caps_dev; cold.caps_off = c->caps_off_dev; cold.caps_idx = c->caps_idx_dev;
    cold.n_caps = (int32_t)(c->caps_host.size() / 12);
    if (!c->cold_valid || std::memcmp(&cold, &c->cold_uploaded, sizeof cold) != 0) {
        std::memcpy(&c->cold_uploaded, &cold, sizeof cold);
        HIPCHK(c, hipMemcpyAsync(c->cold_dev, &c->cold_uploaded, sizeof cold, hipMemcpyHostToDevice, c->stream));
        c->cold_valid = true;
    }
    f.first_block = c->blocks_done;
    f.n_blocks = (uint32_t)n_blocks;
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    if (c->prm.flags & MRTX_F_FORCE_WIDE) f.dem_wide = 1;
    if (c->prm.flags & MRTX_F_NO_SKIP) f.mip = nullptr;   // (build_frame leaves the horizon mip out as well)
    uint64_t culled_px = 0;
    if (c->tile_dirty.size() != (size_t)c->n_local) c->tile_dirty.assign((size_t)c->n_local, 0);
    const bool overlay = !c->caps_host.empty();
    bool culling = false;
    if (!(c->prm.flags & MRTX_F_NO_CULL)) {
        if (c->cull_version != c->scene_version) {
            cull_tiles(c, c->cfg.rank, c->keep_cached, c->culled_px_cached, &c->keep_front_cached);
            c->cull_version = c->scene_version;
        }
        culled_px = c->culled_px_cached;
        culling = true;   // the list also carries the launch ORDER, so it is used even when it holds every tile
    }
    const std::vector<int32_t>& keep = c->keep_cached;
    int moon_n = -1;                     // leading tiles of this launch's list that can see more than sky (-1: no split known)
    if (culling) {
        if (keep != c->keep_uploaded) {
            if (!keep.empty()) {
                HIPCHK(c, hipMemcpyAsync(c->tile_list_dev, keep.data(), keep.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));   // `keep` is pageable host memory
            }
            c->keep_uploaded = keep;
        }
        int pa = 0, pb = (int)keep.size();
        if (n_parts > 1) {   // cut where the shard parts cut: at slot numbers of the COMMON (longest) list
            const int rc_ = gather_layout(c);
            if (rc_ != MRTX_OK) return rc_;
            if (!c->act_on) return fail(c, MRTX_E_STATE, "parts need the active gather layout (mrtx_shard_parts)");
            part_range(c->act_slots, part, n_parts, pa, pb);
            pa = std::min(pa, (int)keep.size()); pb = std::min(pb, (int)keep.size());
        }
        f.tile_list = c->tile_list_dev + pa;
        f.n_active = pb - pa;
        if (c->bg != nullptr) moon_n = std::max(0, std::min(pb, c->keep_front_cached) - pa);
        // culled tiles are all-zero by construction: clear only if an earlier view rendered into one of them
        std::vector<uint8_t> kept((size_t)c->n_local, 0);
        for (int32_t lt : keep) kept[(size_t)lt] = 1;
        bool stale = false;
        for (int lt = 0; lt < c->n_local && !stale; lt++) stale = c->tile_dirty[(size_t)lt] && !kept[(size_t)lt];
        if (stale) {
            const size_t fb = (size_t)c->cfg.width * c->cfg.height * 16;
            HIPCHK(c, hipMemsetAsync(c->accum, 0, fb, c->stream));
            HIPCHK(c, hipMemsetAsync(c->hits, 0, fb, c->stream));
            c->tile_dirty.assign((size_t)c->n_local, 0);
        }
        for (int32_t lt : keep) c->tile_dirty[(size_t)lt] = 1;
    } else {
        culled_px = 0;
        c->tile_dirty.assign((size_t)c->n_local, 1);
    }
    if (stats) HIPCHK(c, hipMemsetAsync(c->stats_dev, 0, 32 * sizeof(unsigned long long), c->stream));
    // D6 (path_seg_max > 1): by default the path continues in path_kernel behind a queue (mode 2);
    // MRTX_F_INWAVE_PATHS keeps it inside the render wave (mode 1) -- same result bit for bit, slower.
    const int S = (int)c->prm.spp_per_launch;
    int mode = c->prm.path_seg_max > 1 ? ((c->prm.flags & MRTX_F_INWAVE_PATHS) ? 1 : 2) : 0;
    if (mode == 2) {
        const uint64_t tiles = f.tile_list ? (uint64_t)(moon_n >= 0 ? moon_n : f.n_active) : (uint64_t)c->n_local;
        if (tiles * (uint64_t)(f.tile_w * f.tile_h) * (uint64_t)S * (uint64_t)n_blocks < c->path_queue_min) mode = 1;
    }
    // With an environment map the sky-only tiles at the end of the list get a launch of their own (render_kernel<MODE 3>: a
    // sample is its environment texel): a small kernel at full occupancy, and the path pipeline is set up for the rest only.
    FrameC fsky = f;
    bool have_sky = false;
    if (moon_n >= 0 && moon_n < f.n_active) {
        fsky.tile_list = f.tile_list + moon_n; fsky.n_active = f.n_active - moon_n;
        fsky.first_block = c->blocks_done; fsky.n_blocks = (uint32_t)n_blocks;
        f.n_active = moon_n;
        have_sky = true;
    }
    // Deferred paths need hand-over buffers and a 24-bit step count per record.  When either is not to be had, the frame is
    // rendered with the paths inside the render wave instead (mode 1: no buffers, the same frame bit for bit, slower) -- a
    // render call does not fail where an identical result exists.  Said once per context on stderr.
    std::vector<FrameC> fs;
    std::vector<PathQ> pqs;
    int n_sub = 1;
    bool overlap = false;                // path stage of sub-part i beside the render kernel of sub-part i + 1 (MOONRT_PATH_OVERLAP)
    auto fall_back = [&](const char* why) {
        if (!c->path_fallback_said) {
            std::fprintf(stderr, "libmoonrt: %s -- frames of this size keep their paths inside the render wave (same result, slower); "
                                 "retried after mrtx_reset_accum or when a frame needs less\n", why);
            c->path_fallback_said = true;
        }
        mode = 1;
    };
    if (mode == 2 && f.kmax >= (1 << 24)) fall_back("marching_step is too small for the 24-bit step count of a hand-over record");
    if (mode == 2) {
    // The hand-over buffers are sized for the worst case (64 bytes for each of the 64 lanes of every wave-job of the
    // launch: 12 GB for the whole-disc cfg3 frame, 129 GB for a cfg4 frame whose every pixel is on the Moon).  A frame
    // that needs more than path_budget_bytes is rendered in SUB-PARTS of its tile list, one after the other through the
    // same buffers: render(sub) -> paths(sub) -> resolve(sub); sub-parts cover disjoint pixels.
    // ... and never more than half of what the device has free right now (unless MOONRT_PATH_MAX_GB says otherwise): a second
    // context, a torch process or a 34 GB cfg4 DEM on the same GPU must not turn the fixed budget into an allocation failure
    uint64_t budget = c->path_budget_bytes;
    const uint64_t full_chunks = mrtx_path_chunks(f, S, nullptr, nullptr);
    if (!c->path_budget_env && full_chunks > c->path_cap) {      // asked only when the buffers have to grow (a driver call: not per frame)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const uint64_t held = (uint64_t)c->path_cap * (uint64_t)c->path_sets * 64ull * MRTX_PATH_REC_BYTES;   // what this context already holds counts as free
            budget = std::min<uint64_t>(budget, std::max<uint64_t>(1ull << 28, ((uint64_t)free_b + held) / 2));
        } else {
            (void)hipGetLastError();
        }
    }
    const uint64_t cap_chunks = std::max<uint64_t>(std::max<uint64_t>(4096, budget / (64ull * MRTX_PATH_REC_BYTES)), c->path_cap);
    n_sub = 1;
    {
        const uint64_t full = full_chunks;
        if (full > cap_chunks && f.tile_list != nullptr) n_sub = (int)std::min<uint64_t>((uint64_t)f.n_active, (full + cap_chunks - 1) / cap_chunks);
    }
    overlap = c->path_overlap > 1 && f.tile_list != nullptr && f.n_active >= 8 * c->path_overlap && !stats;
    if (overlap) n_sub = std::max(n_sub, c->path_overlap);
    const int sets = overlap ? 2 : 1;
    fs.assign((size_t)n_sub, f);
    pqs.assign((size_t)n_sub, PathQ());
    uint64_t chunks = 0;
    for (int s = 0; s < n_sub; s++) {
        int a_, b_;
        part_range(f.n_active, s, n_sub, a_, b_);
        if (n_sub > 1) { fs[(size_t)s].tile_list = f.tile_list + a_; fs[(size_t)s].n_active = b_ - a_; }
        std::memset(&pqs[(size_t)s], 0, sizeof(PathQ));
        chunks = std::max(chunks, mrtx_path_chunks(fs[(size_t)s], S, &pqs[(size_t)s].grid_a, &pqs[(size_t)s].njobs_log2));
    }
    if (chunks * 64ull > 0xFFFFFFFFull) {
        fall_back("the frame holds more wave-jobs than one deferred-path launch can index");
    } else if (chunks > c->path_cap && c->path_nomem_chunks != 0 && chunks >= c->path_nomem_chunks) {
        mode = 1;      // an allocation of this size failed before: do not free and retry three multi-gigabyte hipMallocs per frame
    } else if (chunks > c->path_cap || sets > c->path_sets) {
        if (c->path_rec) { HIPCHK(c, hipFree(c->path_rec)); c->path_rec = nullptr; }
        if (c->path_meta) { HIPCHK(c, hipFree(c->path_meta)); c->path_meta = nullptr; }
        if (c->path_npaths) { HIPCHK(c, hipFree(c->path_npaths)); c->path_npaths = nullptr; }
        c->path_cap = 0;
        if (c->path_alloc_fail_test ||
            hipMalloc((void**)&c->path_rec, (size_t)sets * (size_t)chunks * 64 * MRTX_PATH_REC_BYTES) != hipSuccess ||
            hipMalloc((void**)&c->path_meta, (size_t)sets * (size_t)chunks * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void**)&c->path_npaths, (size_t)sets * ((size_t)chunks + 64)) != hipSuccess) {
            (void)hipGetLastError();                                    // clear the allocation error: the frame is still rendered
            if (c->path_rec) { (void)hipFree(c->path_rec); c->path_rec = nullptr; }
            if (c->path_meta) { (void)hipFree(c->path_meta); c->path_meta = nullptr; }
            if (c->path_npaths) { (void)hipFree(c->path_npaths); c->path_npaths = nullptr; }
            c->path_nomem_chunks = chunks;                              // latched until less is needed or mrtx_reset_accum
            fall_back("no device memory for the hand-over records");
        } else {
            c->path_cap = chunks;
            c->path_sets = sets;
            c->path_nomem_chunks = 0;
        }
    }
    const size_t n = (size_t)c->path_cap * 64;
    if (mode == 2 && !c->path_ctr) HIPCHK(c, hipMalloc((void**)&c->path_ctr, 2 * 8 * 16 * sizeof(uint32_t)));
    for (int s = 0; mode == 2 && s < n_sub; s++) {
        PathQ& pq = pqs[(size_t)s];
        const size_t set = overlap ? (size_t)(s & 1) : 0;     // ping-pong: sub-part s hands over through buffer set s % 2
        pq.ray0 = reinterpret_cast<float4*>(reinterpret_cast<char*>(c->path_rec) + set * n * MRTX_PATH_REC_BYTES); pq.ray1 = pq.ray0 + n; pq.ray2 = pq.ray1 + n;
        pq.c4 = pq.ray2 + n;
        pq.lane_of = reinterpret_cast<uint32_t*>(reinterpret_cast<float*>(pq.c4) + 3 * n);     // 12 bytes per sample
        pq.npaths = c->path_npaths + set * ((size_t)c->path_cap + 64);
        pq.meta = c->path_meta + set * (size_t)c->path_cap;
        pq.counters = c->path_ctr + set * 8 * 16; pq.n_sub = c->path_nsub; pq.grp_log2 = c->path_grp_log2;
        pq.n_chunks = (uint32_t)((uint64_t)pq.grid_a << pq.njobs_log2);
        pq.s_log2 = 0;
        while ((1 << pq.s_log2) < S) pq.s_log2++;
        { const int P = 64 / S; const int PW = P >= 32 ? 8 : P >= 8 ? 4 : P >= 2 ? 2 : 1; pq.pw_log2 = PW == 8 ? 3 : PW == 4 ? 2 : PW == 2 ? 1 : 0; }
        pq.refill_min = c->path_refill; pq.seg_min = c->path_segmin; pq.rare_min = c->path_hitmin;
    }
    }
    double primary_ms = 0.0, paths_ms = 0.0;
    uint32_t launches = 0;
    if (mode != 2) {
        // one launch per block of S samples (round 4: a kernel that knows it traces ONE block keeps nothing alive from block to
        // block -- 25 to 48 VGPRs less, see render_kernel; a launch costs ~10 us, a block of a 4K frame milliseconds)
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        for (int32_t b = 0; b < n_blocks; b++) {
            FrameC fb = f, fsb = fsky;
            fb.first_block = fsb.first_block = c->blocks_done + (uint32_t)b;
            fb.n_blocks = fsb.n_blocks = 1;
            if (f.n_active > 0 || !f.tile_list) HIPCHK(c, mrtx_launch_render(fb, S, stats, mode, overlay, nullptr, c->stream));
            if (have_sky) HIPCHK(c, mrtx_launch_render(fsb, S, stats, 3, false, nullptr, c->stream));
        }
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        primary_ms = ms;
        launches = (((f.n_active > 0 || !f.tile_list) ? 1u : 0u) + (have_sky ? 1u : 0u)) * (uint32_t)n_blocks;
    } else {
        const int wi = (stats ? 2 : 0) + (f.dem_wide ? 1 : 0);
        if (c->path_waves[wi] == 0) {
            int nw = 0;
            if (mrtx_path_waves(stats, f.dem_wide != 0, &nw) != 0 || nw < 8) return fail(c, MRTX_E_DEVICE, "cannot size the path_kernel launch");
            c->path_waves[wi] = nw;
        }
        const int nw = c->path_waves_env ? c->path_waves_env : c->path_waves[wi];
        const size_t n_ev = (size_t)n_blocks * (size_t)n_sub * 3;
        while (c->evs.size() < n_ev) { hipEvent_t e; HIPCHK(c, get_event(c->cfg.device, &e)); c->evs.push_back(e); }
        if (overlap) {
            if (!c->stream2) HIPCHK(c, get_stream(c->cfg.device, &c->stream2));
            for (int i = 0; i < 2; i++) if (!c->ov_done[i]) HIPCHK(c, get_event(c->cfg.device, &c->ov_done[i]));
            if (!c->ov_join) HIPCHK(c, get_event(c->cfg.device, &c->ov_join));
        }
        size_t ov_idx = 0;                 // sub-part launches so far in this call (overlap: which buffer set / which `done` event)
        for (int32_t b = 0; b < n_blocks && f.n_active > 0; b++) {
            for (int s = 0; s < n_sub; s++) {
                hipEvent_t* ev = &c->evs[((size_t)b * (size_t)n_sub + (size_t)s) * 3];
                FrameC fb = fs[(size_t)s];
                fb.first_block = c->blocks_done + (uint32_t)b;
                fb.n_blocks = 1;
                PathQ& pq = pqs[(size_t)s];
                pq.gs_base = fb.first_block * (uint32_t)S;
                if (overlap) {
                    // render(i) on the context's stream, paths(i) + resolve(i) on stream2 beside render(i + 1); buffer set i % 2 is
                    // free again when paths(i - 2) has finished
                    const int set = s & 1;
                    if (ov_idx >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ov_done[set], 0));
                    HIPCHK(c, hipMemsetAsync(pq.meta, 0, (size_t)pq.n_chunks * sizeof(uint32_t), c->stream));
                    HIPCHK(c, hipMemsetAsync(pq.npaths, 0, (size_t)pq.n_chunks, c->stream));
                    HIPCHK(c, hipMemsetAsync(pq.counters, 0, 8 * 16 * sizeof(uint32_t), c->stream));
                    HIPCHK(c, hipEventRecord(ev[0], c->stream));
                    HIPCHK(c, mrtx_launch_render(fb, S, stats, 2, overlay, &pq, c->stream));
                    HIPCHK(c, hipEventRecord(ev[1], c->stream));
                    HIPCHK(c, hipStreamWaitEvent(c->stream2, ev[1], 0));
                    const bool last = (b == n_blocks - 1) && (s == n_sub - 1);
                    HIPCHK(c, mrtx_launch_paths(fb, pq, S, stats, last ? nw : std::min(nw, c->path_overlap_waves), c->stream2));
                    HIPCHK(c, hipEventRecord(c->ov_done[set], c->stream2));
                    HIPCHK(c, hipEventRecord(ev[2], c->stream2));
                    ov_idx++;
                    continue;
                }
                HIPCHK(c, hipMemsetAsync(pq.meta, 0, (size_t)pq.n_chunks * sizeof(uint32_t), c->stream));
                HIPCHK(c, hipMemsetAsync(pq.npaths, 0, (size_t)pq.n_chunks, c->stream));
                HIPCHK(c, hipMemsetAsync(pq.counters, 0, 8 * 16 * sizeof(uint32_t), c->stream));
                HIPCHK(c, hipEventRecord(ev[0], c->stream));
                HIPCHK(c, mrtx_launch_render(fb, S, stats, 2, overlay, &pq, c->stream));
                HIPCHK(c, hipEventRecord(ev[1], c->stream));
                HIPCHK(c, mrtx_launch_paths(fb, pq, S, stats, nw, c->stream));
                HIPCHK(c, hipEventRecord(ev[2], c->stream));
            }
        }
        if (overlap && ov_idx > 0) {       // the context's stream goes on (sky tiles, watchdog read-back) when stream2 has drained
            HIPCHK(c, hipEventRecord(c->ov_join, c->stream2));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ov_join, 0));
        }
        if (have_sky) {   // nothing but the environment can be seen from these tiles: no paths, no records
            HIPCHK(c, hipEventRecord(c->ev0, c->stream));
            for (int32_t b = 0; b < n_blocks; b++) {
                FrameC fsb = fsky;
                fsb.first_block = c->blocks_done + (uint32_t)b; fsb.n_blocks = 1;
                HIPCHK(c, mrtx_launch_render(fsb, S, stats, 3, false, nullptr, c->stream));
            }
            HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        }
        // path_kernel's watchdog (stats[15]): a wave gave up after 2^24 iterations -- the frame is incomplete.  Read through
        // pinned memory on the stream, so that the one synchronisation below covers it (no second blocking copy per call).
        if (!c->wd_host) HIPCHK(c, hipHostMalloc((void**)&c->wd_host, sizeof(unsigned long long), hipHostMallocDefault));
        HIPCHK(c, hipMemcpyAsync(c->wd_host, c->stats_dev + 15, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        {
            const unsigned long long wd = *c->wd_host;
            if (wd != 0) {
                HIPCHK(c, hipMemset(c->stats_dev + 15, 0, sizeof wd));
                return fail(c, MRTX_E_DEVICE, "path_kernel watchdog: %llu wave(s) did not finish their paths", wd);
            }
        }
        if (have_sky) {
            float a = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&a, c->ev0, c->ev1));
            primary_ms += a;
        }
        const size_t n_launched = f.n_active > 0 ? (size_t)n_blocks * (size_t)n_sub : 0;
        if (overlap && n_launched > 0) {
            // the two stages run side by side: primary_ms = first render start .. last render end, paths_ms = what of the path
            // stage is still running after that (the EXPOSED part)
            float a = 0.0f, p = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&a, c->evs[0], c->evs[(n_launched - 1) * 3 + 1]));
            HIPCHK(c, hipEventElapsedTime(&p, c->evs[(n_launched - 1) * 3 + 1], c->evs[(n_launched - 1) * 3 + 2]));
            primary_ms += a; paths_ms += p;
        }
        for (size_t i = 0; !overlap && i < n_launched; i++) {
            float a = 0.0f, p = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&a, c->evs[i * 3], c->evs[i * 3 + 1]));
            HIPCHK(c, hipEventElapsedTime(&p, c->evs[i * 3 + 1], c->evs[i * 3 + 2]));
            primary_ms += a; paths_ms += p;
        }
        launches = (f.n_active > 0 ? 3u * (uint32_t)n_blocks * (uint32_t)n_sub : 0u) + (have_sky ? (uint32_t)n_blocks : 0u);
    }
    if (part == n_parts - 1) c->blocks_done += (uint32_t)n_blocks;
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->kernel_ms = primary_ms + paths_ms;
        out->primary_ms = primary_ms;
        out->paths_ms = paths_ms;
        out->launches = launches;
        if (stats) {
            unsigned long long h[32];
            HIPCHK(c, hipMemcpy(h, c->stats_dev, sizeof h, hipMemcpyDeviceToHost));
            out->camera_height_samples = h[3]; out->camera_dem_fetches = h[6]; out->camera_mip_fetches = h[7];
            out->camera_colour_fetches = h[4]; out->camera_background_fetches = h[5];
            for (int i = 0; i < 15; i++) h[i] += h[16 + i];          // totals = render_kernel's + path_kernel's
            out->primary_rays = h[0] + (part == 0 ? culled_px : 0) * (uint64_t)c->prm.spp_per_launch * (uint64_t)n_blocks;
            out->primary_hits = h[1]; out->shadow_rays = h[2];
            out->height_samples = h[3]; out->colour_fetches = h[4]; out->background_fetches = h[5];
            out->dem_fetches = h[6]; out->mip_fetches = h[7]; out->bounce_rays = h[8]; out->bounce_sun_hits = h[9];
        }
    }
    return MRTX_OK;
}

// ---- Sun illumination of the terrain ------------------------------------------------------------
static bool illum_n_ok(int32_t n) { return n >= 1 && n <= 64 && (n & (n - 1)) == 0; }

int mrtx_illum_sun_samples(int32_t n, float* out2) {
    if (!illum_n_ok(n) || !out2) return MRTX_E_INVALID;
    for (int32_t i = 0; i < n; i++) {
        if (n == 1) { out2[0] = 0.0f; out2[1] = 0.0f; break; }     // the Sun's centre: a point-light terminator
        const double t = (double)i * 0.6180339887498949;
        out2[2 * i] = (float)(((double)i + 0.5) / (double)n);
        out2[2 * i + 1] = (float)(t - std::floor(t));
    }
    return MRTX_OK;
}

// (sin, cos) of an angle in degrees: float64, rounded once each
static void illum_sc(double deg, float* sc) {
    const double r = deg * (kPiD / 180.0);
    sc[0] = (float)std::sin(r);
    sc[1] = (float)std::cos(r);
}

// ---- What every terrain query shares: its tables and frame (staging, output and finish: "What the host units share") --------
// The band of a lat/lon map (MrtxIllumGrid, or MrtxSightGrid's targets) checked and as the stage's tables: rtab = the rows'
// (sin lat, cos lat), ctab = the columns' (sin lon, cos lon).  The illumination grid's n_sun is checked among them.
extern "C++" template <class G>
static int grid_tables(mrtx_ctx* c, const G* g, std::vector<float>& rtab, std::vector<float>& ctab) {
    if (!std::isfinite(g->lat_north) || !std::isfinite(g->lat_south) || !(g->lat_north > g->lat_south) || g->lat_north > 90.0 ||
        g->lat_south < -90.0)
        return fail(c, MRTX_E_INVALID, "latitudes must satisfy 90 >= lat_north > lat_south >= -90");
    if (!std::isfinite(g->lon_west) || !std::isfinite(g->lon_east) || !(g->lon_east > g->lon_west) || std::fabs(g->lon_west) > 1e6 ||
        std::fabs(g->lon_east) > 1e6)
        return fail(c, MRTX_E_INVALID, "longitudes must be finite with lon_west < lon_east");
    if (g->h < 1 || g->w < 1) return fail(c, MRTX_E_INVALID, "empty grid (%d x %d)", g->h, g->w);
    if (g->row_begin < 0 || g->row_end > g->h || g->row_begin >= g->row_end)
        return fail(c, MRTX_E_INVALID, "bad band [%d, %d) of %d rows", g->row_begin, g->row_end, g->h);
    if constexpr (std::is_same<G, MrtxIllumGrid>::value)
        if (!illum_n_ok(g->n_sun)) return fail(c, MRTX_E_INVALID, "n_sun must be 1, 2, 4, ..., 64 (got %d)", g->n_sun);
    if ((int64_t)(g->row_end - g->row_begin) * (int64_t)g->w > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a band holds at most 2^31 nodes: split the map into more bands");
    const int rows = g->row_end - g->row_begin;
    rtab.assign((size_t)rows * 2, 0.0f);
    ctab.assign((size_t)g->w * 2, 0.0f);
    const double dlat = (g->lat_north - g->lat_south) / (double)g->h, dlon = (g->lon_east - g->lon_west) / (double)g->w;
    for (int i = 0; i < rows; i++) illum_sc(g->lat_north - ((double)(g->row_begin + i) + 0.5) * dlat, &rtab[(size_t)i * 2]);
    for (int j = 0; j < g->w; j++) illum_sc(g->lon_west + ((double)j + 0.5) * dlon, &ctab[(size_t)j * 2]);
    return MRTX_OK;
}

// A point list checked and as the stage's tables: rtab = n (sin lat, cos lat) pairs, ctab = n (sin lon, cos lon) pairs
static int point_tables(mrtx_ctx* c, const double* latlon, int32_t n, std::vector<float>& rtab, std::vector<float>& ctab) {
    rtab.assign((size_t)n * 2, 0.0f);
    ctab.assign((size_t)n * 2, 0.0f);
    for (int32_t i = 0; i < n; i++) {
        const double la = latlon[2 * (size_t)i], lo = latlon[2 * (size_t)i + 1];
        if (!std::isfinite(la) || !std::isfinite(lo) || la > 90.0 || la < -90.0 || std::fabs(lo) > 1e6)
            return fail(c, MRTX_E_INVALID, "point %d: latitude must lie in [-90, 90] and longitude be finite", i);
        illum_sc(la, &rtab[(size_t)i * 2]);
        illum_sc(lo, &ctab[(size_t)i * 2]);
    }
    return MRTX_OK;
}

// The frame of a terrain launch: the context's DEM and march parameters (and the horizon mip when the launch marches), the
// stage's own cold block and counters.  sky: the single-epoch illumination calls, which also read the context's Moon frame
// and light.  Called after every argument check.
static int stage_frame(mrtx_ctx* c, FrameC& f, FrameCold& cold, bool march, bool sky = false) {
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    if (sky && !c->moon_set) return fail(c, MRTX_E_STATE, "no moon frame: call mrtx_set_moon_frame first");
    if (sky && !c->light_set) return fail(c, MRTX_E_STATE, "no light: call mrtx_set_light first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (march && !(c->prm.flags & MRTX_F_NO_SKIP)) { const int rc_ = ensure_mip(c); if (rc_ != MRTX_OK) return rc_; }
    std::memset(&cold, 0, sizeof cold);
    build_frame(c, f, cold);
    if (!c->illum_cold) HIPCHK(c, hipMalloc((void**)&c->illum_cold, sizeof(FrameCold)));
    if (!c->illum_stats) HIPCHK(c, hipMalloc((void**)&c->illum_stats, 16 * sizeof(unsigned long long)));
    cold.accum = nullptr; cold.hits = nullptr; cold.stats = c->illum_stats; cold.stats_paths = nullptr;
    f.cold = c->illum_cold;
    if (c->prm.flags & MRTX_F_FORCE_WIDE) f.dem_wide = 1;
    if (c->prm.flags & MRTX_F_NO_SKIP) f.mip = nullptr;   // (build_frame leaves the horizon mip out as well)
    return MRTX_OK;
}

// ---- Sun illumination: maps, points and series ---------------------------------------------------------------------------
// Everything after the argument checks: state, tables, one launch into `dev_out`, counters.  rtab / ctab: n_r and n_c
// (sin, cos) pairs.  A series (mrtx_illum_series) passes `lights`, 8 floats per epoch, and `first` (per point, or null): then
// rows = points, cols = the window's length, and the context's own light and Moon frame are not used.
static int illum_run(mrtx_ctx* c, const std::vector<float>& rtab, const std::vector<float>& ctab, int rows, int cols, bool points,
                     int n_sun, void* dev_out, float* host_out, MrtxStats* out, const std::vector<float>* lights = nullptr,
                     const int32_t* first = nullptr) {
    FrameC f;
    FrameCold cold;
    int rc = stage_frame(c, f, cold, true, !lights);
    if (rc != MRTX_OK) return rc;
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    float sun[128];
    mrtx_illum_sun_samples(n_sun, sun);
    const size_t out_bytes = (size_t)rows * (size_t)cols * 16;
    float* d[5];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK ||
        (rc = stage_tables(c, {{sun, 2 * (size_t)n_sun}, rtab, ctab,
                               {lights ? lights->data() : nullptr, lights ? lights->size() : 0}, {first, first ? (size_t)rows : 0}},
                           d)) != MRTX_OK)
        return rc;
    IllumC g;
    std::memset(&g, 0, sizeof g);
    g.sun = d[0]; g.rtab = d[1]; g.ctab = d[2];
    g.out = (float*)dev_out; g.rows = rows; g.cols = cols; g.points = points ? 1 : 0; g.n_sun = n_sun;
    if ((rc = stage_start(c, &cold, stats)) != MRTX_OK) return rc;
    if (lights) {
        IllumSeriesC q;
        q.g = g;
        q.lights = d[3];
        q.first = first ? reinterpret_cast<const int32_t*>(d[4]) : nullptr;
        HIPCHK(c, mrtx_launch_illum_series(f, q, stats, c->stream));
    } else {
        HIPCHK(c, mrtx_launch_illum(f, g, stats, c->stream));
    }
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_illum_grid(mrtx_ctx* c, const MrtxIllumGrid* g, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!g) return fail(c, MRTX_E_INVALID, "null grid");
    std::vector<float> rtab, ctab;
    const int rc = grid_tables(c, g, rtab, ctab);
    if (rc != MRTX_OK) return rc;
    if (!dev_out && !host_out) return fail(c, MRTX_E_INVALID, "no output buffer");
    return illum_run(c, rtab, ctab, g->row_end - g->row_begin, g->w, false, g->n_sun, dev_out, host_out, out);
}

int mrtx_illum_points(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_sun, float* host_out4, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (n < 1) return fail(c, MRTX_E_INVALID, "n must be >= 1 (got %d)", n);
    if (!latlon || !host_out4) return fail(c, MRTX_E_INVALID, "null point list or output");
    if (!illum_n_ok(n_sun)) return fail(c, MRTX_E_INVALID, "n_sun must be 1, 2, 4, ..., 64 (got %d)", n_sun);
    std::vector<float> rtab, ctab;
    const int rc = point_tables(c, latlon, n, rtab, ctab);
    if (rc != MRTX_OK) return rc;
    return illum_run(c, rtab, ctab, 1, n, true, n_sun, nullptr, host_out4, out);
}

// per epoch what build_frame forms from mrtx_set_light + mrtx_set_moon_frame, after the checks those two make: 8 floats per
// epoch, (Lb.xyz, rL2), (rad2, 0, 0, 0)
static int epoch_lights(mrtx_ctx* c, const MrtxIllumEpoch* ep, int32_t n_epochs, std::vector<float>& lights) {
    lights.assign((size_t)n_epochs * 8, 0.0f);
    for (int32_t k = 0; k < n_epochs; k++) {
        const MrtxIllumEpoch& e = ep[k];
        if (!check_vec(e.light_pos) || !std::isfinite(e.light_radius) || !std::isfinite(e.light_radiance) ||
            !(e.light_radius >= 0.0) || !(e.light_radiance >= 0.0))
            return fail(c, MRTX_E_INVALID, "epoch %d: bad light", k);
        if (!check_vec(e.center) || !check_vec(e.u) || !check_vec(e.v)) return fail(c, MRTX_E_INVALID, "epoch %d: bad moon frame", k);
        double x[3];
        cross(e.u, e.v, x);
        if (!((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2] > 0.0)) return fail(c, MRTX_E_INVALID, "epoch %d: moon u and v are parallel", k);
        double M[3][3];
        moon_rows(e.u, e.v, M);
        float* l = &lights[(size_t)k * 8];
        light_consts(M, e.center, e.light_pos, e.light_radius, e.light_radiance, l, l[3], l[4]);
    }
    return MRTX_OK;
}

int mrtx_illum_series(mrtx_ctx* c, const double* latlon, int32_t n_points, const MrtxIllumEpoch* ep, int32_t n_epochs,
                      const int32_t* first, int32_t count, int32_t n_sun, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !ep) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    if (!dev_out && !host_out) return fail(c, MRTX_E_INVALID, "no output buffer");
    if (n_points < 1 || n_epochs < 1 || count < 1)
        return fail(c, MRTX_E_INVALID, "n_points, n_epochs and count must be >= 1 (got %d, %d, %d)", n_points, n_epochs, count);
    if (!illum_n_ok(n_sun)) return fail(c, MRTX_E_INVALID, "n_sun must be 1, 2, 4, ..., 64 (got %d)", n_sun);
    if ((int64_t)n_points * (int64_t)count > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a series holds at most 2^31 outputs: split the points into more calls");
    for (int32_t p = 0; p < n_points; p++) {
        const int64_t f0 = first ? (int64_t)first[p] : 0;
        if (f0 < 0 || f0 + count > n_epochs)
            return fail(c, MRTX_E_INVALID, "point %d: window [%lld, %lld) runs outside the %d epochs", p, (long long)f0,
                        (long long)(f0 + count), n_epochs);
    }
    std::vector<float> rtab, ctab, lights;
    int rc = point_tables(c, latlon, n_points, rtab, ctab);
    if (rc != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, ep, n_epochs, lights)) != MRTX_OK) return rc;
    return illum_run(c, rtab, ctab, n_points, count, true, n_sun, dev_out, host_out, out, &lights, first);
}

// ---- Terrain horizons and the Sun against them (DESIGN.md sections 3.8 and 3.9) --------------------------------------------
static bool horizon_az_ok(int32_t n_az) { return n_az >= 4 && n_az <= 4096 && (n_az & (n_az - 1)) == 0; }
static int log2_of(int32_t n) { int l = 0; while ((1 << l) < n) l++; return l; }

// the horizon and output arguments of mrtx_horizon_sun and the thermal calls: where each lives, and the horizons' size
static int horizon_args(mrtx_ctx* c, const void* dev_horizon, const float* host_horizon, int32_t n, int32_t n_az,
                        const void* dev_out, const float* host_out) {
    if ((dev_horizon == nullptr) == (host_horizon == nullptr))
        return fail(c, MRTX_E_INVALID, "give exactly one of dev_horizon and host_horizon");
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if ((int64_t)n * (int64_t)n_az > (int64_t)1 << 31) return fail(c, MRTX_E_INVALID, "at most 2^31 horizon samples per call");
    return MRTX_OK;
}

// every entry of a host horizon table an elevation in [-90, 90] degrees (a device table is not scanned)
static int horizon_entries(mrtx_ctx* c, const float* host_horizon, int32_t n, int32_t n_az) {
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    for (size_t i = 0; i < nh; i++)
        if (!(host_horizon[i] >= -90.0f && host_horizon[i] <= 90.0f))
            return fail(c, MRTX_E_INVALID, "horizon entry %zu is not an elevation in [-90, 90] degrees", i);
    return MRTX_OK;
}

int mrtx_horizon_points(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, int32_t n_bis, void* dev_out, float* host_out,
                        MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon) return fail(c, MRTX_E_INVALID, "null point list");
    if (n < 1) return fail(c, MRTX_E_INVALID, "n must be >= 1 (got %d)", n);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (n_bis < 1 || n_bis > 24) return fail(c, MRTX_E_INVALID, "n_bis must lie in [1, 24] (got %d)", n_bis);
    if ((int64_t)n * (int64_t)n_az > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a call holds at most 2^31 outputs: split the points into more calls");
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    std::vector<float> rtab, ctab;
    int rc = point_tables(c, latlon, n, rtab, ctab);
    if (rc != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, true)) != MRTX_OK) return rc;
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    const size_t out_bytes = (size_t)n * (size_t)n_az * sizeof(float);
    float* d[2];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK || (rc = stage_tables(c, {rtab, ctab}, d)) != MRTX_OK) return rc;
    HorizonC h;
    std::memset(&h, 0, sizeof h);
    h.g.rtab = d[0]; h.g.ctab = d[1];
    h.g.rows = n; h.g.cols = n; h.g.points = 1;
    h.out = (float*)dev_out; h.az_log2 = log2_of(n_az); h.n_bis = n_bis;
    if ((rc = stage_start(c, &cold, stats)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_horizon(f, h, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_horizon_sun(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon, const float* host_horizon,
                     const MrtxIllumEpoch* epochs, int32_t m, int32_t mode, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    if (n < 1 || m < 1) return fail(c, MRTX_E_INVALID, "n and m must be >= 1 (got %d, %d)", n, m);
    // the kernel's epoch loop and the dark run (a float count, exact up to 2^24) stay exact below this
    if (m > (1 << 24)) return fail(c, MRTX_E_INVALID, "at most 2^24 epochs per call (got %d)", m);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (mode != 0 && mode != 1) return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL) or 1 (SUMMARY) (got %d)", mode);
    int rc = horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, host_out);
    if (rc != MRTX_OK) return rc;
    if (mode == 0 && (int64_t)n * (int64_t)m > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "FULL holds at most 2^31 outputs per call: split the points into more calls");
    if ((rc = horizon_entries(c, host_horizon, n, n_az)) != MRTX_OK) return rc;
    std::vector<float> rtab, ctab, lights;
    if ((rc = point_tables(c, latlon, n, rtab, ctab)) != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, epochs, m, lights)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    const size_t out_bytes = mode == 0 ? (size_t)n * (size_t)m * sizeof(float) : (size_t)n * 16;
    float* d[4];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK ||
        (rc = stage_tables(c, {rtab, ctab, lights, {host_horizon, nh}}, d)) != MRTX_OK)
        return rc;
    HorizonSunC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.lights = d[2];
    q.horizon = host_horizon ? d[3] : (const float*)dev_horizon;
    q.out = (float*)dev_out; q.az_log2 = log2_of(n_az); q.m = m; q.mode = mode;
    if ((rc = stage_start(c, &cold, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_horizon_sun(f, q, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays);
}

// ---- Mast-height horizons and joint windows --------------------------------------------------------
int mrtx_horizon_raised(mrtx_ctx* c, const double* latlon, const double* height_m, double radius_m, int32_t n, int32_t n_az,
                        int32_t n_bis, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !height_m) return fail(c, MRTX_E_INVALID, "null point list or height list");
    if (n < 1) return fail(c, MRTX_E_INVALID, "n must be >= 1 (got %d)", n);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (n_bis < 1 || n_bis > 24) return fail(c, MRTX_E_INVALID, "n_bis must lie in [1, 24] (got %d)", n_bis);
    if (!std::isfinite(radius_m) || !(radius_m > 0.0)) return fail(c, MRTX_E_INVALID, "radius_m must be finite and > 0");
    if ((int64_t)n * (int64_t)n_az > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a call holds at most 2^31 outputs: split the points into more calls");
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    std::vector<float> hs((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const double h = height_m[i];
        if (!std::isfinite(h) || h < 0.0 || h > 1e4) return fail(c, MRTX_E_INVALID, "point %d: height must lie in [0, 1e4] m", i);
        hs[(size_t)i] = (float)(h / radius_m * c->radius);
        if (!std::isfinite(hs[(size_t)i])) return fail(c, MRTX_E_INVALID, "point %d: height / radius_m is out of range", i);
    }
    std::vector<float> rtab, ctab;
    int rc = point_tables(c, latlon, n, rtab, ctab);
    if (rc != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, true)) != MRTX_OK) return rc;
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    const size_t out_bytes = (size_t)n * (size_t)n_az * sizeof(float);
    float* d[3];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK || (rc = stage_tables(c, {rtab, ctab, hs}, d)) != MRTX_OK) return rc;
    HorizonRaisedC q;
    std::memset(&q, 0, sizeof q);
    q.h.g.rtab = d[0]; q.h.g.ctab = d[1];
    q.h.g.rows = n; q.h.g.cols = n; q.h.g.points = 1;
    q.h.out = (float*)dev_out; q.h.az_log2 = log2_of(n_az); q.h.n_bis = n_bis;
    q.hs = d[2];
    if ((rc = stage_start(c, &cold, stats)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_horizon_raised(f, q, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_horizon_windows(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                         const float* host_horizon, const MrtxIllumEpoch* epochs_a, const MrtxIllumEpoch* epochs_b, int32_t m,
                         double min_a, double min_b, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs_a || !epochs_b) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    if (n < 1 || m < 1) return fail(c, MRTX_E_INVALID, "n and m must be >= 1 (got %d, %d)", n, m);
    // the runs and the start index are float counts, exact up to 2^24
    if (m > (1 << 24)) return fail(c, MRTX_E_INVALID, "at most 2^24 epochs per call (got %d)", m);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (!(min_a > 0.0 && min_a <= 1.0) || !(min_b > 0.0 && min_b <= 1.0))
        return fail(c, MRTX_E_INVALID, "min_a and min_b must lie in (0, 1]");
    if (!((float)min_a > 0.0f) || !((float)min_b > 0.0f))
        return fail(c, MRTX_E_INVALID, "min_a and min_b must be positive as float32");
    int rc = horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, host_out);
    if (rc != MRTX_OK) return rc;
    if (dev_out && ((uintptr_t)dev_out & 15)) return fail(c, MRTX_E_INVALID, "dev_out must be 16-byte aligned");
    if ((rc = horizon_entries(c, host_horizon, n, n_az)) != MRTX_OK) return rc;
    std::vector<float> rtab, ctab, lights_a, lights_b;
    if ((rc = point_tables(c, latlon, n, rtab, ctab)) != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, epochs_a, m, lights_a)) != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, epochs_b, m, lights_b)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    const size_t out_bytes = (size_t)n * 32;
    float* d[5];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK ||
        (rc = stage_tables(c, {rtab, ctab, lights_a, lights_b, {host_horizon, nh}}, d)) != MRTX_OK)
        return rc;
    HorizonWindowsC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.lights_a = d[2]; q.lights_b = d[3];
    q.horizon = host_horizon ? d[4] : (const float*)dev_horizon;
    q.out = (float*)dev_out; q.min_a = (float)min_a; q.min_b = (float)min_b; q.az_log2 = log2_of(n_az); q.m = m;
    if ((rc = stage_start(c, &cold, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_horizon_windows(f, q, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays);
}

// ---- Drive masks: mrtx_horizon_windows' predicate kept as bits -------------------------------------
int mrtx_horizon_mask(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                      const float* host_horizon, const MrtxIllumEpoch* epochs_a, const MrtxIllumEpoch* epochs_b, int32_t m,
                      double min_a, double min_b, void* dev_out, uint64_t* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs_a) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    if (n < 1 || m < 1) return fail(c, MRTX_E_INVALID, "n and m must be >= 1 (got %d, %d)", n, m);
    if (m > (1 << 24)) return fail(c, MRTX_E_INVALID, "at most 2^24 epochs per call (got %d)", m);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (!epochs_b) min_b = 1.0;        // ignored without a second table
    if (!(min_a > 0.0 && min_a <= 1.0) || !(min_b > 0.0 && min_b <= 1.0))
        return fail(c, MRTX_E_INVALID, "min_a and min_b must lie in (0, 1]");
    if (!((float)min_a > 0.0f) || !((float)min_b > 0.0f))
        return fail(c, MRTX_E_INVALID, "min_a and min_b must be positive as float32");
    int rc = horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, reinterpret_cast<const float*>(host_out));
    if (rc != MRTX_OK) return rc;
    if (dev_out && ((uintptr_t)dev_out & 7)) return fail(c, MRTX_E_INVALID, "dev_out must be 8-byte aligned");
    if ((rc = horizon_entries(c, host_horizon, n, n_az)) != MRTX_OK) return rc;
    std::vector<float> rtab, ctab, lights_a, lights_b;
    if ((rc = point_tables(c, latlon, n, rtab, ctab)) != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, epochs_a, m, lights_a)) != MRTX_OK) return rc;
    if (epochs_b && (rc = epoch_lights(c, epochs_b, m, lights_b)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    const size_t out_bytes = (size_t)n * (size_t)((m + 63) / 64) * 8;
    float* d[5];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK ||
        (rc = stage_tables(c, {rtab, ctab, lights_a, lights_b, {host_horizon, nh}}, d)) != MRTX_OK)
        return rc;
    HorizonMaskC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.lights_a = d[2]; q.lights_b = epochs_b ? d[3] : nullptr;
    q.horizon = host_horizon ? d[4] : (const float*)dev_horizon;
    q.out = (unsigned long long*)dev_out; q.min_a = (float)min_a; q.min_b = (float)min_b; q.az_log2 = log2_of(n_az); q.m = m;
    if ((rc = stage_start(c, &cold, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_horizon_mask(f, q, c->stream));
    return stage_finish(c, dev_out, reinterpret_cast<float*>(host_out), out_bytes, out, kNoRays);
}

// ---- The Earth's occultation of the Sun ------------------------------------------------------------
// The two epoch tables of mrtx_occultation and mrtx_thermal_occulted: epoch_lights' checks and constants for both, the
// geometry the two-disc rule stands on, and per epoch the float64 mark "some point inside the bounding sphere may see the
// discs overlap".  With Rb the bounding sphere (the Moon's radius and the vertex lift, plus a thousandth), d the centre
// distances and r the radii: the centre's separation, less both bodies' largest parallax asin(Rb / d), against the sum of the
// largest angular radii asin(r / (d - Rb)) widened by 1 % and 1e-4 rad -- a hundred times what float32 directions can move.
static int occult_tables(mrtx_ctx* c, const MrtxIllumEpoch* src, const MrtxIllumEpoch* body, int32_t m, std::vector<float>& ls,
                         std::vector<float>& lb, std::vector<float>& marks) {
    int rc;
    if ((rc = epoch_lights(c, src, m, ls)) != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, body, m, lb)) != MRTX_OK) return rc;
    const double Rb = 1.001 * c->radius + std::fabs((double)c->prm.scene_epsilon);
    marks.assign((size_t)m, 0.0f);
    int32_t* const mk = reinterpret_cast<int32_t*>(marks.data());
    for (int32_t k = 0; k < m; k++) {
        double a[3], b[3];
        for (int i = 0; i < 3; i++) { a[i] = src[k].light_pos[i] - src[k].center[i]; b[i] = body[k].light_pos[i] - body[k].center[i]; }
        const double ds = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
        const double db = std::sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
        const double rs = src[k].light_radius, rb = body[k].light_radius;
        if (!(rb > 0.0)) return fail(c, MRTX_E_INVALID, "epoch %d: the body's radius must be > 0", k);
        if (!(db > Rb + rb))
            return fail(c, MRTX_E_INVALID, "epoch %d: the body reaches into the Moon's bounding sphere (centre %g away, radius %g)",
                        k, db, rb);
        if (!(db + Rb < ds - Rb))
            return fail(c, MRTX_E_INVALID, "epoch %d: the body (%g away) is not nearer than the source (%g) from every point", k, db,
                        ds);
        double x[3];
        cross(a, b, x);
        const double sep = std::atan2(std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
        const double reach = std::asin(std::min(1.0, rs / (ds - Rb))) + std::asin(std::min(1.0, rb / (db - Rb)));
        mk[k] = sep - std::asin(Rb / ds) - std::asin(Rb / db) <= 1.01 * reach + 1e-4 ? 1 : 0;
    }
    return MRTX_OK;
}

int mrtx_occultation(mrtx_ctx* c, const double* latlon, int32_t n, const MrtxIllumEpoch* epochs_source,
                     const MrtxIllumEpoch* epochs_body, int32_t m, int32_t mode, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs_source || !epochs_body) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    if (n < 1 || m < 1) return fail(c, MRTX_E_INVALID, "n and m must be >= 1 (got %d, %d)", n, m);
    // the runs, the start index and the run count are float counts, exact up to 2^24
    if (m > (1 << 24)) return fail(c, MRTX_E_INVALID, "at most 2^24 epochs per call (got %d)", m);
    if (mode != 0 && mode != 1) return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL) or 1 (SUMMARY) (got %d)", mode);
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if (mode == 1 && dev_out && ((uintptr_t)dev_out & 15)) return fail(c, MRTX_E_INVALID, "dev_out must be 16-byte aligned");
    if (mode == 0 && (int64_t)n * (int64_t)m > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "FULL holds at most 2^31 outputs per call: split the points into more calls");
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    std::vector<float> rtab, ctab, ls, lb, marks;
    int rc;
    if ((rc = point_tables(c, latlon, n, rtab, ctab)) != MRTX_OK) return rc;
    if ((rc = occult_tables(c, epochs_source, epochs_body, m, ls, lb, marks)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const size_t out_bytes = mode == 0 ? (size_t)n * (size_t)m * sizeof(float) : (size_t)n * 32;
    float* d[5];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK || (rc = stage_tables(c, {rtab, ctab, ls, lb, marks}, d)) != MRTX_OK)
        return rc;
    OccultC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.src = d[2]; q.body = d[3]; q.mark = reinterpret_cast<const int32_t*>(d[4]);
    q.out = (float*)dev_out; q.m = m; q.mode = mode;
    if ((rc = stage_start(c, &cold, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_occultation(f, q, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays);
}

// ---- Orbiter passes: relay contact windows against terrain horizons -------------------------------
static_assert(sizeof(MrtxPasses) == 32, "MrtxPasses is 32 bytes");
static_assert(sizeof(MrtxPass) == 40 && sizeof(PassRec) == sizeof(MrtxPass) && alignof(PassRec) == 4, "MrtxPass is 40 bytes");

int mrtx_horizon_passes(mrtx_ctx* c, const MrtxPasses* k, const double* latlon, const double* height_m, int32_t n, int32_t n_az,
                        const void* dev_horizon, const float* host_horizon, const double* sat_pos_m, void* dev_out, void* host_out,
                        uint64_t pass_cap, uint64_t* n_passes, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!k) return fail(c, MRTX_E_INVALID, "null passes block");
    if (!latlon || !sat_pos_m) return fail(c, MRTX_E_INVALID, "null point list or position table");
    if (k->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    if (k->mode != MRTX_PASSES_FULL && k->mode != MRTX_PASSES_SUMMARY && k->mode != MRTX_PASSES_LIST)
        return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL), 1 (SUMMARY) or 2 (LIST) (got %d)", k->mode);
    if (n < 1) return fail(c, MRTX_E_INVALID, "n must be >= 1 (got %d)", n);
    if (k->n_sat < 1 || k->n_sat > 256) return fail(c, MRTX_E_INVALID, "n_sat must lie in [1, 256] (got %d)", k->n_sat);
    // the runs, the indices and the sum of c_k are float counts, exact up to 2^24
    if (k->m < 1 || k->m > (1 << 24) || (int64_t)k->n_sat * (int64_t)k->m > (int64_t)1 << 24)
        return fail(c, MRTX_E_INVALID, "m must be >= 1 and n_sat * m at most 2^24 (got %d x %d)", k->n_sat, k->m);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (!std::isfinite(k->radius_m) || !(k->radius_m > 0.0)) return fail(c, MRTX_E_INVALID, "radius_m must be finite and > 0");
    if (!(k->min_elev_deg >= -90.0 && k->min_elev_deg < 90.0)) return fail(c, MRTX_E_INVALID, "min_elev_deg must lie in [-90, 90)");
    const bool list = k->mode == MRTX_PASSES_LIST;
    const int S = k->n_sat, m = k->m;
    if ((dev_horizon == nullptr) == (host_horizon == nullptr))
        return fail(c, MRTX_E_INVALID, "give exactly one of dev_horizon and host_horizon");
    if ((int64_t)n * (int64_t)n_az > (int64_t)1 << 31) return fail(c, MRTX_E_INVALID, "at most 2^31 horizon samples per call");
    if (dev_out && host_out) return fail(c, MRTX_E_INVALID, "give at most one of dev_out and host_out");
    const bool has_out = dev_out || host_out;
    if (!list && !has_out) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if (list && !n_passes) return fail(c, MRTX_E_INVALID, "null n_passes");
    if (list && !has_out && pass_cap) return fail(c, MRTX_E_INVALID, "without a table pass_cap must be 0 (got %llu)", (unsigned long long)pass_cap);
    if (dev_out && ((uintptr_t)dev_out & (list ? 7 : 15)))
        return fail(c, MRTX_E_INVALID, "dev_out must be %d-byte aligned", list ? 8 : 16);
    if (k->mode == MRTX_PASSES_FULL && (int64_t)n * S * m > (int64_t)1 << 27)
        return fail(c, MRTX_E_INVALID, "FULL holds at most 2^27 outputs per call: split the points into more calls");
    if (list && (int64_t)n * S > (int64_t)1 << 27)
        return fail(c, MRTX_E_INVALID, "LIST holds at most 2^27 (point, satellite) pairs per call: split the points into more calls");
    int rc;
    if ((rc = horizon_entries(c, host_horizon, n, n_az)) != MRTX_OK) return rc;
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    std::vector<float> hs((size_t)n, 0.0f);
    double hs_max = 0.0;
    for (int32_t i = 0; height_m && i < n; i++) {
        const double h = height_m[i];
        if (!std::isfinite(h) || h < 0.0 || h > 1e4) return fail(c, MRTX_E_INVALID, "point %d: height must lie in [0, 1e4] m", i);
        hs[(size_t)i] = (float)(h / k->radius_m * c->radius);
        if (!std::isfinite(hs[(size_t)i])) return fail(c, MRTX_E_INVALID, "point %d: height / radius_m is out of range", i);
        hs_max = std::max(hs_max, (double)hs[(size_t)i]);
    }
    // the satellites' table: one float4 per (satellite, epoch), outside mrtx_occultation's bounding sphere plus the largest raise
    const double Rb = 1.001 * c->radius + std::fabs((double)c->prm.scene_epsilon) + hs_max;
    std::vector<float> sat((size_t)S * (size_t)m * 4, 0.0f);
    for (size_t i = 0; i < (size_t)S * (size_t)m; i++) {
        double r2 = 0.0;
        for (int j = 0; j < 3; j++) {
            const double x = sat_pos_m[3 * i + j];
            const float xf = (float)(x / k->radius_m * c->radius);
            if (!std::isfinite(x) || !std::isfinite(xf))
                return fail(c, MRTX_E_INVALID, "satellite %zu, epoch %zu: the position is not finite", i / (size_t)m, i % (size_t)m);
            sat[4 * i + j] = xf;
            r2 += (double)xf * (double)xf;
        }
        if (!(std::sqrt(r2) > Rb))
            return fail(c, MRTX_E_INVALID, "satellite %zu, epoch %zu: the position lies within the Moon's bounding sphere (%g of %g)",
                        i / (size_t)m, i % (size_t)m, std::sqrt(r2), Rb);
    }
    std::vector<float> rtab, ctab;
    if ((rc = point_tables(c, latlon, n, rtab, ctab)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    const size_t pairs = (size_t)n * (size_t)S;
    const size_t out_bytes = k->mode == MRTX_PASSES_FULL ? pairs * (size_t)m * 16 : (size_t)n * 32;
    float* d[5];
    if (!list && (rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK) return rc;
    // LIST: the counts, then the prefix sums (8-byte aligned), in the work buffer
    const size_t base_at = (pairs * 4 + 15) & ~(size_t)15;
    if (list && (rc = stage_buffer(c, c->trav_buf, c->trav_bytes, base_at + pairs * 8)) != MRTX_OK) return rc;
    if ((rc = stage_tables(c, {rtab, ctab, hs, sat, {host_horizon, nh}}, d)) != MRTX_OK) return rc;
    PassesC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.hs = d[2]; q.sat = d[3];
    q.horizon = host_horizon ? d[4] : (const float*)dev_horizon;
    q.min_elev = (float)k->min_elev_deg; q.range_scale = (float)(k->radius_m / c->radius);
    q.az_log2 = log2_of(n_az); q.m = m; q.n_sat = S;
    if (!list) {
        q.out = dev_out;
        if ((rc = stage_start(c, &cold, false)) != MRTX_OK) return rc;
        HIPCHK(c, mrtx_launch_passes(f, q, k->mode, c->stream));
        return stage_finish(c, dev_out, static_cast<float*>(host_out), out_bytes, out, kNoRays);
    }
    char* const tb = reinterpret_cast<char*>(c->trav_buf);
    q.counts = reinterpret_cast<uint32_t*>(tb);
    q.base = reinterpret_cast<const unsigned long long*>(tb + base_at);
    if ((rc = stage_start(c, &cold, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_passes(f, q, 2, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // also: the pageable tables are no longer read
    std::vector<uint32_t> counts(pairs);
    HIPCHK(c, hipMemcpy(counts.data(), q.counts, pairs * 4, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> base(pairs);
    uint64_t total = 0;
    for (size_t i = 0; i < pairs; i++) { base[i] = total; total += counts[i]; }
    uint32_t launches = 1;
    const bool fits = total <= pass_cap;
    const size_t list_bytes = sizeof(MrtxPass) * (size_t)total;
    if (has_out && fits && total) {
        if (host_out) {
            if ((rc = stage_buffer(c, c->illum_out, c->illum_out_bytes, list_bytes)) != MRTX_OK) return rc;
            dev_out = c->illum_out;
        }
        q.out = dev_out;
        HIPCHK(c, hipMemcpyAsync(tb + base_at, base.data(), pairs * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, mrtx_launch_passes(f, q, 3, c->stream));
        launches = 2;
    }
    const bool filled = launches == 2;
    if ((rc = stage_finish(c, dev_out, filled ? static_cast<float*>(host_out) : nullptr, list_bytes, out, kNoRays)) != MRTX_OK) return rc;
    if (out) out->launches = launches;
    *n_passes = total;
    if (has_out && !fits)
        return fail(c, MRTX_E_INVALID, "the table is too small: %llu passes are needed (pass_cap = %llu)", (unsigned long long)total,
                    (unsigned long long)pass_cap);
    return MRTX_OK;
}

// ---- Site power budgets ----------------------------------------------------------------------------
int mrtx_power_budget(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon, const float* host_horizon,
                      const MrtxIllumEpoch* epochs, const double* gen_w, const double* load_w, int32_t m,
                      const MrtxPowerModel* model, int32_t mode, void* dev_out, void* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    if (!gen_w || !load_w || !model) return fail(c, MRTX_E_INVALID, "null generation table, load table or power model");
    if (n < 1 || m < 1) return fail(c, MRTX_E_INVALID, "n and m must be >= 1 (got %d, %d)", n, m);
    // 2^24 epochs of at most 2^28 counts: every sum stays within 2^52
    if (m > (1 << 24)) return fail(c, MRTX_E_INVALID, "at most 2^24 epochs per call (got %d)", m);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (mode != 0 && mode != 1) return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL) or 1 (SUMMARY) (got %d)", mode);
    int rc = horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, (const float*)host_out);
    if (rc != MRTX_OK) return rc;
    if (mode == 1 && dev_out && ((uintptr_t)dev_out & 15)) return fail(c, MRTX_E_INVALID, "dev_out must be 16-byte aligned");
    if (mode == 0 && (int64_t)n * (int64_t)m > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "FULL holds at most 2^31 outputs per call: split the points into more calls");
    if (model->panel < 0 || model->panel > 2)
        return fail(c, MRTX_E_INVALID, "panel must be 0 (TRACK), 1 (FIXED) or 2 (AZIMUTH) (got %d)", model->panel);
    float nrm[3] = {0.0f, 0.0f, 1.0f};
    if (model->panel == 1) {
        const double* e = model->normal_enu;
        const double len = std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        if (!check_vec(e) || !std::isfinite(len) || !(len > 0.0)) return fail(c, MRTX_E_INVALID, "normal_enu must be finite and not zero");
        for (int i = 0; i < 3; i++) nrm[i] = (float)(e[i] / len);
    }
    if (model->cpw_log2 < -20 || model->cpw_log2 > 20)
        return fail(c, MRTX_E_INVALID, "cpw_log2 must lie in [-20, 20] (got %d)", model->cpw_log2);
    if (model->capacity < 0 || model->capacity > ((int64_t)1 << 52))
        return fail(c, MRTX_E_INVALID, "capacity must lie in [0, 2^52] counts");
    if (model->initial < 0 || model->initial > model->capacity) return fail(c, MRTX_E_INVALID, "initial must lie in [0, capacity]");
    const float scale = std::ldexp(1.0f, model->cpw_log2);
    std::vector<float> gen((size_t)m);
    std::vector<int32_t> load((size_t)m);
    for (int32_t k = 0; k < m; k++) {
        const float g = (float)gen_w[k] * scale, l = (float)load_w[k] * scale;      // a power of two: exact
        if (!std::isfinite(gen_w[k]) || !(gen_w[k] >= 0.0) || !(g <= 268435456.0f))
            return fail(c, MRTX_E_INVALID, "gen_w[%d] must be finite, >= 0 and at most 2^28 counts", k);
        if (!std::isfinite(load_w[k]) || !(load_w[k] >= 0.0) || !(l <= 268435456.0f))
            return fail(c, MRTX_E_INVALID, "load_w[%d] must be finite, >= 0 and at most 2^28 counts", k);
        gen[(size_t)k] = (float)gen_w[k];
        load[(size_t)k] = (int32_t)std::nearbyint(l);       // round to nearest even, the kernel's rintf
    }
    if ((rc = horizon_entries(c, host_horizon, n, n_az)) != MRTX_OK) return rc;
    std::vector<float> rtab, ctab, lights;
    if ((rc = point_tables(c, latlon, n, rtab, ctab)) != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, epochs, m, lights)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    const size_t out_bytes = mode == 0 ? (size_t)n * (size_t)m * sizeof(int32_t) : (size_t)n * 64;
    float* d[6];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK ||
        (rc = stage_tables(c, {rtab, ctab, lights, gen, {load.data(), load.size()}, {host_horizon, nh}}, d)) != MRTX_OK)
        return rc;
    PowerC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.lights = d[2]; q.gen = d[3]; q.load = reinterpret_cast<const int32_t*>(d[4]);
    q.horizon = host_horizon ? d[5] : (const float*)dev_horizon;
    q.out = dev_out; q.capacity = model->capacity; q.initial = model->initial; q.scale = scale;
    q.nE = nrm[0]; q.nN = nrm[1]; q.nU = nrm[2];
    q.panel = model->panel; q.az_log2 = log2_of(n_az); q.m = m; q.mode = mode;
    if ((rc = stage_start(c, &cold, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_power_budget(f, q, c->stream));
    return stage_finish(c, dev_out, (float*)host_out, out_bytes, out, kNoRays);
}

// ---- Terrain line of sight -------------------------------------------------------------------------
static bool sight_height_ok(double h) { return std::isfinite(h) && h >= 0.0 && h <= 1e9; }
static bool sight_latlon_ok(double la, double lo) { return std::isfinite(la) && std::isfinite(lo) && std::fabs(la) <= 90.0 && std::fabs(lo) <= 1e6; }

// the checks every sight call shares
static int sight_check(mrtx_ctx* c, double target_h_m, double mast_max_m, double radius_m, int32_t n_bis, const void* dev_out,
                       const float* host_out) {
    if (!sight_height_ok(target_h_m)) return fail(c, MRTX_E_INVALID, "target height must lie in [0, 1e9] m");
    if (!std::isfinite(mast_max_m) || mast_max_m < 0.0 || mast_max_m > 1e9 || (n_bis > 0 && !(mast_max_m > 0.0)))
        return fail(c, MRTX_E_INVALID, "mast_max_m must lie in [0, 1e9] m, and be > 0 when n_bis > 0");
    if (!std::isfinite(radius_m) || !(radius_m > 0.0)) return fail(c, MRTX_E_INVALID, "radius_m must be finite and > 0");
    if (n_bis < 0 || n_bis > 24) return fail(c, MRTX_E_INVALID, "n_bis must lie in [0, 24] (got %d)", n_bis);
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    return MRTX_OK;
}

// Everything after the argument checks: the targets' tables (trt, tct: rows x cols nodes, or a point list), the observers'
// tables and raised heights (scene units), one launch into the output, counters.
static int sight_run(mrtx_ctx* c, const std::vector<float>& trt, const std::vector<float>& tct, int rows, int cols, bool points,
                     const std::vector<float>& ort, const std::vector<float>& oct, const std::vector<double>& obs_h_m,
                     double target_h_m, double mast_max_m, double radius_m, int32_t n_bis, void* dev_out, float* host_out,
                     MrtxStats* out) {
    FrameC f;
    FrameCold cold;
    int rc;
    if ((rc = stage_frame(c, f, cold, true)) != MRTX_OK) return rc;
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    const int n_obs = (int)obs_h_m.size();
    std::vector<float> hs((size_t)n_obs);
    for (int i = 0; i < n_obs; i++) hs[(size_t)i] = (float)(obs_h_m[(size_t)i] / radius_m * c->radius);
    const size_t out_bytes = (size_t)rows * (size_t)cols * sizeof(float);
    float* d[5];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK || (rc = stage_tables(c, {trt, tct, ort, oct, hs}, d)) != MRTX_OK)
        return rc;
    SightC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = rows; q.g.cols = cols; q.g.points = points ? 1 : 0;
    q.obs.rtab = d[2]; q.obs.ctab = d[3];
    q.obs.rows = n_obs; q.obs.cols = n_obs; q.obs.points = 1;
    q.obs_hs = d[4];
    q.out = (float*)dev_out;
    q.target_h_m = target_h_m; q.mast_max_m = mast_max_m; q.radius_m = radius_m; q.R = c->radius;
    q.n_obs = n_obs; q.n_bis = n_bis;
    if ((rc = stage_start(c, &cold, stats)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_sight(f, q, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_sight_grid(mrtx_ctx* c, const MrtxSightGrid* g, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!g) return fail(c, MRTX_E_INVALID, "null grid");
    if (!sight_latlon_ok(g->obs_lat, g->obs_lon))
        return fail(c, MRTX_E_INVALID, "observer: latitude must lie in [-90, 90] and longitude be finite");
    if (!sight_height_ok(g->obs_h_m)) return fail(c, MRTX_E_INVALID, "observer height must lie in [0, 1e9] m");
    int rc = sight_check(c, g->target_h_m, g->mast_max_m, g->radius_m, g->n_bis, dev_out, host_out);
    if (rc != MRTX_OK) return rc;
    std::vector<float> trt, tct, ort, oct;
    if ((rc = grid_tables(c, g, trt, tct)) != MRTX_OK) return rc;
    const double ll[2] = {g->obs_lat, g->obs_lon};
    if ((rc = point_tables(c, ll, 1, ort, oct)) != MRTX_OK) return rc;
    return sight_run(c, trt, tct, g->row_end - g->row_begin, g->w, false, ort, oct, std::vector<double>(1, g->obs_h_m),
                     g->target_h_m, g->mast_max_m, g->radius_m, g->n_bis, dev_out, host_out, out);
}

int mrtx_sight_points(mrtx_ctx* c, const double* target_latlon, int32_t n, const double* observer_llh, int32_t n_observers,
                      double target_h_m, double mast_max_m, double radius_m, int32_t n_bis, void* dev_out, float* host_out,
                      MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!target_latlon || !observer_llh) return fail(c, MRTX_E_INVALID, "null target or observer list");
    if (n < 1) return fail(c, MRTX_E_INVALID, "n must be >= 1 (got %d)", n);
    if (n_observers != 1 && n_observers != n)
        return fail(c, MRTX_E_INVALID, "n_observers must be 1 or n (got %d for n = %d)", n_observers, n);
    int rc = sight_check(c, target_h_m, mast_max_m, radius_m, n_bis, dev_out, host_out);
    if (rc != MRTX_OK) return rc;
    std::vector<float> trt, tct, ort, oct;
    if ((rc = point_tables(c, target_latlon, n, trt, tct)) != MRTX_OK) return rc;
    std::vector<double> oll((size_t)n_observers * 2), oh((size_t)n_observers);
    for (int32_t i = 0; i < n_observers; i++) {
        const double* o = observer_llh + 3 * (size_t)i;
        if (!sight_latlon_ok(o[0], o[1]))
            return fail(c, MRTX_E_INVALID, "observer %d: latitude must lie in [-90, 90] and longitude be finite", i);
        if (!sight_height_ok(o[2])) return fail(c, MRTX_E_INVALID, "observer %d: height must lie in [0, 1e9] m", i);
        oll[2 * (size_t)i] = o[0]; oll[2 * (size_t)i + 1] = o[1]; oh[(size_t)i] = o[2];
    }
    if ((rc = point_tables(c, oll.data(), n_observers, ort, oct)) != MRTX_OK) return rc;
    return sight_run(c, trt, tct, 1, n, true, ort, oct, oh, target_h_m, mast_max_m, radius_m, n_bis, dev_out, host_out, out);
}

// ---- Least-cost traverses ---------------------------------------------------------------------------
// The checks that need no DEM: the effort model, the window's own numbers, the node count
static int traverse_params(mrtx_ctx* c, const MrtxTraverse* t) {
    if (t->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    if (t->rows < 1 || t->cols < 1) return fail(c, MRTX_E_INVALID, "empty window (%d x %d)", t->rows, t->cols);
    if ((int64_t)t->rows * (int64_t)t->cols > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a window holds at most 2^31 nodes (got %d x %d)", t->rows, t->cols);
    if (t->stride < 1) return fail(c, MRTX_E_INVALID, "stride must be >= 1 (got %d)", t->stride);
    if (t->row0 < 0 || t->col0 < 0) return fail(c, MRTX_E_INVALID, "row0 and col0 must be >= 0");
    if (t->wrap != 0 && t->wrap != 1) return fail(c, MRTX_E_INVALID, "wrap must be 0 or 1 (got %d)", t->wrap);
    if (t->wrap && t->cols < 3) return fail(c, MRTX_E_INVALID, "a wrapped window needs cols >= 3 (got %d)", t->cols);
    if (!std::isfinite(t->radius_m) || !(t->radius_m > 0.0) || !std::isfinite((float)t->radius_m))
        return fail(c, MRTX_E_INVALID, "radius_m must be finite and > 0 (also as a float32)");
    if (!((float)t->max_grade > 0.0f)) return fail(c, MRTX_E_INVALID, "max_grade must be > 0 (as a float32; +inf: no limit)");
    if (!std::isfinite(t->climb_cost) || !(t->climb_cost >= 0.0) || !std::isfinite((float)t->climb_cost) ||
        !std::isfinite(t->descent_cost) || !(t->descent_cost >= 0.0) || !std::isfinite((float)t->descent_cost))
        return fail(c, MRTX_E_INVALID, "climb_cost and descent_cost must be finite and >= 0 (also as float32)");
    return MRTX_OK;
}

// The checks against the DEM's shape (H, W), then the rows x 3 lengths into out3 (each finite and > 0 as a float32)
static int traverse_window(mrtx_ctx* c, const MrtxTraverse* t, int32_t H, int32_t W, float* out3) {
    if (H < 2 || W < 2) return fail(c, MRTX_E_INVALID, "the DEM must be at least 2 x 2 (got %d x %d)", H, W);
    if (t->row0 + (int64_t)(t->rows - 1) * t->stride >= H)
        return fail(c, MRTX_E_INVALID, "the window's last row %lld lies outside the DEM's %d rows",
                    (long long)(t->row0 + (int64_t)(t->rows - 1) * t->stride), H);
    if (t->col0 >= W) return fail(c, MRTX_E_INVALID, "col0 = %d lies outside the DEM's %d columns", t->col0, W);
    if (t->wrap && (int64_t)t->cols * t->stride != W)
        return fail(c, MRTX_E_INVALID, "wrap = 1 needs cols x stride == W (%lld != %d)", (long long)t->cols * t->stride, W);
    if (!t->wrap && (int64_t)(t->cols - 1) * t->stride >= W)
        return fail(c, MRTX_E_INVALID, "the window's columns repeat: (cols - 1) x stride must be < W = %d", W);
    const double dphi = (double)t->stride * kPiD / (double)H, dlam = (double)t->stride * 2.0 * kPiD / (double)W;
    const double sl = std::sin(0.5 * dlam), sp = std::sin(0.5 * dphi);
    for (int32_t i = 0; i < t->rows; i++) {
        const double r = (double)t->row0 + (double)i * t->stride;
        const double p1 = 0.5 * kPiD - (r + 0.5) * (kPiD / (double)H), p2 = p1 - dphi;
        const double c1 = std::cos(p1), c2 = std::cos(p2);
        const double hav[3] = {c1 * c1 * sl * sl, sp * sp, sp * sp + c1 * c2 * sl * sl};     // haversines of the three edges
        for (int k = 0; k < 3; k++) {
            const bool last = i == t->rows - 1 && k > 0;
            const float L = last ? 0.0f : (float)(2.0 * t->radius_m * std::asin(std::sqrt(std::min(hav[k], 1.0))));
            if (!last && !(std::isfinite(L) && L > 0.0f))
                return fail(c, MRTX_E_INVALID, "row %d: edge length %d is %g, not a finite positive float32", i, k, (double)L);
            if (out3) out3[3 * (size_t)i + k] = L;
        }
    }
    return MRTX_OK;
}

int mrtx_traverse_lengths(const MrtxTraverse* t, int32_t dem_h, int32_t dem_w, float* out3) {
    if (!t || !out3) return MRTX_E_INVALID;
    const int rc = traverse_params(nullptr, t);
    return rc != MRTX_OK ? rc : traverse_window(nullptr, t, dem_h, dem_w, out3);
}

// The caller's device tables: the costs are read and written as 64-bit atomics (8-byte aligned), the penalties as floats
// (4-byte aligned); no two of them may overlap (the kernels read the penalties while they write costs and codes)
static int traverse_dev_buffers(mrtx_ctx* c, const MrtxTraverse* t, const void* dev_penalty, const void* dev_cost,
                                const void* dev_pred) {
    const size_t N = (size_t)t->rows * (size_t)t->cols;
    if (dev_cost && (reinterpret_cast<uintptr_t>(dev_cost) & 7))
        return fail(c, MRTX_E_INVALID, "dev_cost must be 8-byte aligned (float64, read and written atomically)");
    if (dev_penalty && (reinterpret_cast<uintptr_t>(dev_penalty) & 3))
        return fail(c, MRTX_E_INVALID, "dev_penalty must be 4-byte aligned (float32)");
    if (spans_overlap(dev_cost, 8 * N, dev_pred, N) || spans_overlap(dev_penalty, 4 * N, dev_cost, 8 * N) ||
        spans_overlap(dev_penalty, 4 * N, dev_pred, N))
        return fail(c, MRTX_E_INVALID, "dev_penalty, dev_cost and dev_pred must not overlap");
    return MRTX_OK;
}

static bool traverse_penalty_ok(float p) { return (p >= 1e-3f && p <= 1e6f) || p == INFINITY; }

// a host penalty table is refused at its first bad entry (a device table's bad entries are counted by the init kernel)
static int traverse_host_penalty(mrtx_ctx* c, const float* host_penalty, size_t N) {
    if (host_penalty)
        for (size_t n = 0; n < N; n++)
            if (!traverse_penalty_ok(host_penalty[n]))
                return fail(c, MRTX_E_INVALID, "penalty %zu must be finite in [1e-3, 1e6] or +inf (got %g)", n, (double)host_penalty[n]);
    return MRTX_OK;
}

// MOONRT_TRAVERSE_TILE: the tile edge, 8, 16 or 32 (the same field in every case)
static int traverse_tile_edge(mrtx_ctx* c, int& TS) {
    TS = 32;
    if (const char* e = std::getenv("MOONRT_TRAVERSE_TILE")) {
        TS = std::atoi(e);
        if (TS != 8 && TS != 16 && TS != 32) return fail(c, MRTX_E_INVALID, "MOONRT_TRAVERSE_TILE must be 8, 16 or 32 (got %s)", e);
    }
    return MRTX_OK;
}

// The sources of a field with starts of type S: each inside the window and with a start that start_rule(k, s) accepts (it
// fails with the field's own text), then sorted by node and duplicates reduced to their smallest start
extern "C++" template <class S, class Rule>
static int traverse_sources(mrtx_ctx* c, const MrtxTraverse* t, const int32_t* src_ij, const S* src_start, int32_t n_src,
                            Rule start_rule, std::vector<int64_t>& sn, std::vector<S>& sc) {
    if (n_src < 1 || !src_ij) return fail(c, MRTX_E_INVALID, "need n_src >= 1 sources (got %d)", n_src);
    std::vector<std::pair<int64_t, S>> src((size_t)n_src);
    for (int32_t k = 0; k < n_src; k++) {
        const int32_t i = src_ij[2 * (size_t)k], j = src_ij[2 * (size_t)k + 1];
        const S s = src_start ? src_start[k] : S(0);
        if (i < 0 || i >= t->rows || j < 0 || j >= t->cols)
            return fail(c, MRTX_E_INVALID, "source %d: node (%d, %d) lies outside the %d x %d window", k, i, j, t->rows, t->cols);
        const int rc = start_rule(k, s);
        if (rc != MRTX_OK) return rc;
        src[(size_t)k] = {(int64_t)i * t->cols + j, s + S(0)};      // -0 made +0: the kernels order costs by their bits
    }
    std::sort(src.begin(), src.end());
    for (const auto& e : src)
        if (sn.empty() || sn.back() != e.first) { sn.push_back(e.first); sc.push_back(e.second); }
    return MRTX_OK;
}

// the DEM and the window of a traverse block: all that mrtx_traverse_heights needs of it
static void traverse_fill_window(const mrtx_ctx* c, const FrameC& f, const MrtxTraverse* t, TraverseC& g) {
    g.dem = f.dem; g.dem_pitch = f.dem_pitch; g.dem_w = c->dem_w;
    g.row0 = t->row0; g.col0 = t->col0; g.rows = t->rows; g.cols = t->cols; g.stride = t->stride; g.wrap = t->wrap;
}

// A field's block Q (TraverseC, or one that holds it) and its three launch steps
static TraverseC& traverse_block(TraverseC& q) { return q; }
static TraverseC& traverse_block(TraverseTimedC& q) { return q.t; }
extern "C++" template <class Q>
struct TraverseSteps {
    hipError_t (*init)(const Q&, hipStream_t);
    hipError_t (*relax)(const Q&, hipStream_t);
    hipError_t (*pred)(const Q&, hipStream_t);
};

// the relaxation launches one batch at a time; the change counter of the batch's last launch is read after each batch
static const int kTraverseBatch = 8;

// What mrtx_traverse and mrtx_traverse_timed share, from the sources on; their own argument checks come before it.  q: the
// field's zeroed block; S: the type of a start and of a value (8 bytes); extra: one more host table (or none) for stage_tables;
// set_field(values, starts, extra's device copy) fills what is the field's own in q.  trav_buf holds the values and the
// codes the caller wants on the host, then the two tile-flag arrays.
extern "C++" template <class Q, class S, class Rule, class Field>
static int traverse_run(mrtx_ctx* c, const MrtxTraverse* t, Q& q, const TraverseSteps<Q>& steps, const int32_t* src_ij,
                        const S* src_start, int32_t n_src, Rule start_rule, const void* dev_penalty, const float* host_penalty,
                        HostSeg extra, void* dev_val, S* host_val, void* dev_pred, uint8_t* host_pred, Field set_field,
                        uint64_t* tile_visits, MrtxStats* out) {
    static_assert(sizeof(S) == 8, "values and starts are 64-bit");
    std::vector<int64_t> sn;
    std::vector<S> sc;
    int rc = traverse_sources(c, t, src_ij, src_start, n_src, start_rule, sn, sc);
    if (rc != MRTX_OK) return rc;
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    std::vector<float> len((size_t)t->rows * 3);
    if ((rc = traverse_window(c, t, c->dem_h, c->dem_w, len.data())) != MRTX_OK) return rc;
    const size_t N = (size_t)t->rows * (size_t)t->cols;
    if ((rc = traverse_host_penalty(c, host_penalty, N)) != MRTX_OK) return rc;
    int TS;
    if ((rc = traverse_tile_edge(c, TS)) != MRTX_OK) return rc;
    // ---- device work from here
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const int tiles_x = (t->cols + TS - 1) / TS, tiles_y = (t->rows + TS - 1) / TS;
    const size_t tiles = (size_t)tiles_x * (size_t)tiles_y;
    const size_t val_b = host_val ? N * 8 : 0, pred_b = host_pred ? (N + 15) & ~(size_t)15 : 0;
    if ((rc = stage_buffer(c, c->trav_buf, c->trav_bytes, val_b + pred_b + 2 * tiles * 4)) != MRTX_OK) return rc;
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    void* d_val = host_val ? tb : dev_val;
    uint8_t* d_pred = host_pred ? reinterpret_cast<uint8_t*>(tb + val_b) : static_cast<uint8_t*>(dev_pred);
    uint32_t* flags = reinterpret_cast<uint32_t*>(tb + val_b + pred_b);
    const size_t np = host_penalty ? N : 0;
    float* d[5];
    if ((rc = stage_tables(c, {len, {sn.data(), 2 * sn.size()}, {sc.data(), 2 * sc.size()}, {host_penalty, np}, extra}, d)) != MRTX_OK)
        return rc;
    TraverseC& g = traverse_block(q);
    traverse_fill_window(c, f, t, g);
    g.len = d[0];
    g.src_node = reinterpret_cast<const int64_t*>(d[1]);
    g.n_src = (int32_t)sn.size();
    g.pen = host_penalty ? d[3] : static_cast<const float*>(dev_penalty);
    g.pred = d_pred;
    g.rm = (float)t->radius_m; g.gmax = (float)t->max_grade; g.a_up = (float)t->climb_cost; g.a_dn = (float)t->descent_cost;
    g.tile = TS; g.tiles_x = tiles_x; g.tiles_y = tiles_y;
    g.visits = c->illum_stats;                                       // [0] tile visits, [1] bad device penalties
    g.changed = reinterpret_cast<uint32_t*>(c->illum_stats + 2);     // kTraverseBatch per-launch change counters
    set_field(d_val, d[2], d[4]);
    uint32_t* fa = flags;
    uint32_t* fb = flags + tiles;
    HIPCHK(c, hipMemsetAsync(flags, 0, 2 * tiles * 4, c->stream));
    if ((rc = stage_start(c, nullptr, true)) != MRTX_OK) return rc;
    g.flag_in = fa;
    HIPCHK(c, steps.init(q, c->stream));
    unsigned long long cnt[2] = {0, 0};
    if (dev_penalty) {
        HIPCHK(c, hipMemcpyAsync(cnt, c->illum_stats, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (cnt[1])
            return fail(c, MRTX_E_INVALID, "%llu entries of the device penalty table are not finite in [1e-3, 1e6] or +inf", cnt[1]);
    }
    // no launch cap: every store strictly lowers a value, and the fixed point is reached after finitely many of them
    // (DESIGN.md section 4.14 for the costs, 4.22 for the arrival ticks)
    uint32_t launches = 0;
    for (;;) {
        HIPCHK(c, hipMemsetAsync(g.changed, 0, kTraverseBatch * sizeof(uint32_t), c->stream));
        for (int s = 0; s < kTraverseBatch; s++) {
            g.flag_in = fa; g.flag_out = fb; g.slot = s;
            HIPCHK(c, steps.relax(q, c->stream));
            std::swap(fa, fb);
            launches++;
        }
        uint32_t last = 0;
        HIPCHK(c, hipMemcpyAsync(&last, g.changed + (kTraverseBatch - 1), sizeof last, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (last == 0) break;       // a whole launch lowered nothing: every later one is empty too
    }
    HIPCHK(c, steps.pred(q, c->stream));
    // finish: time, the 64-bit and uint8 read-backs, the counters
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (host_val) HIPCHK(c, hipMemcpy(host_val, d_val, N * 8, hipMemcpyDeviceToHost));
    if (host_pred) HIPCHK(c, hipMemcpy(host_pred, d_pred, N, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(cnt, c->illum_stats, sizeof cnt, hipMemcpyDeviceToHost));
    if (tile_visits) *tile_visits = cnt[0];
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->kernel_ms = ms;
        out->launches = launches;
    }
    return MRTX_OK;
}

int mrtx_traverse(mrtx_ctx* c, const MrtxTraverse* t, const int32_t* src_ij, const double* src_cost, int32_t n_src,
                  const void* dev_penalty, const float* host_penalty, void* dev_cost, double* host_cost, void* dev_pred,
                  uint8_t* host_pred, uint64_t* tile_visits, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!t) return fail(c, MRTX_E_INVALID, "null window");
    int rc = traverse_params(c, t);
    if (rc != MRTX_OK) return rc;
    if (dev_penalty && host_penalty) return fail(c, MRTX_E_INVALID, "give at most one of dev_penalty and host_penalty");
    if ((dev_cost == nullptr) == (host_cost == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_cost and host_cost");
    if ((dev_pred == nullptr) == (host_pred == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_pred and host_pred");
    if ((rc = traverse_dev_buffers(c, t, dev_penalty, dev_cost, dev_pred)) != MRTX_OK) return rc;
    TraverseC q;
    std::memset(&q, 0, sizeof q);
    const TraverseSteps<TraverseC> steps = {mrtx_launch_traverse_init, mrtx_launch_traverse_relax, mrtx_launch_traverse_pred};
    return traverse_run(
        c, t, q, steps, src_ij, src_cost, n_src,
        [&](int32_t k, double s) {
            return std::isfinite(s) && s >= 0.0 ? MRTX_OK : fail(c, MRTX_E_INVALID, "source %d: start cost must be finite and >= 0", k);
        },
        dev_penalty, host_penalty, HostSeg(nullptr, 0), dev_cost, host_cost, dev_pred, host_pred,
        [&](void* val, const float* start, const float*) {
            q.d = static_cast<double*>(val);
            q.src_cost = reinterpret_cast<const double*>(start);
        },
        tile_visits, out);
}

// ---- Timed traverses: earliest arrival under per-node drive windows --------------------------------
int mrtx_traverse_timed(mrtx_ctx* c, const MrtxTraverse* t, const MrtxTraverseTimed* tt, const int32_t* src_ij,
                        const uint64_t* src_tick, int32_t n_src, const void* dev_penalty, const float* host_penalty,
                        const void* dev_avail, const uint64_t* host_avail, void* dev_arrival, uint64_t* host_arrival,
                        void* dev_pred, uint8_t* host_pred, uint64_t* tile_visits, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!t) return fail(c, MRTX_E_INVALID, "null window");
    if (!tt) return fail(c, MRTX_E_INVALID, "null tick scales");
    int rc = traverse_params(c, t);
    if (rc != MRTX_OK) return rc;
    if (tt->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    if (!std::isfinite(tt->ticks_per_cost) || !(tt->ticks_per_cost > 0.0))
        return fail(c, MRTX_E_INVALID, "ticks_per_cost must be finite and > 0");
    if (tt->ticks_per_epoch < 1) return fail(c, MRTX_E_INVALID, "ticks_per_epoch must be >= 1 (got %d)", tt->ticks_per_epoch);
    const bool table = dev_avail || host_avail;
    if (table && (tt->n_epochs < 1 || tt->n_epochs > (1 << 24)))
        return fail(c, MRTX_E_INVALID, "n_epochs must lie in [1, 2^24] (got %d)", tt->n_epochs);
    if (dev_penalty && host_penalty) return fail(c, MRTX_E_INVALID, "give at most one of dev_penalty and host_penalty");
    if (dev_avail && host_avail) return fail(c, MRTX_E_INVALID, "give at most one of dev_avail and host_avail");
    if ((dev_arrival == nullptr) == (host_arrival == nullptr))
        return fail(c, MRTX_E_INVALID, "give exactly one of dev_arrival and host_arrival");
    if ((dev_pred == nullptr) == (host_pred == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_pred and host_pred");
    if (dev_arrival && (reinterpret_cast<uintptr_t>(dev_arrival) & 7))
        return fail(c, MRTX_E_INVALID, "dev_arrival must be 8-byte aligned (uint64, read and written atomically)");
    if ((rc = traverse_dev_buffers(c, t, dev_penalty, dev_arrival, dev_pred)) != MRTX_OK) return rc;
    const size_t N = (size_t)t->rows * (size_t)t->cols;
    const size_t W64 = table ? ((size_t)tt->n_epochs + 63) / 64 : 0;
    if (dev_avail && (reinterpret_cast<uintptr_t>(dev_avail) & 7)) return fail(c, MRTX_E_INVALID, "dev_avail must be 8-byte aligned");
    if (spans_overlap(dev_avail, 8 * N * W64, dev_arrival, 8 * N) || spans_overlap(dev_avail, 8 * N * W64, dev_pred, N) ||
        spans_overlap(dev_avail, 8 * N * W64, dev_penalty, 4 * N))
        return fail(c, MRTX_E_INVALID, "dev_avail must not overlap dev_penalty, dev_arrival or dev_pred");
    // a start tick lies inside the table; without one it leaves room for 2^31 edges of 2^31 ticks below UINT64_MAX
    const uint64_t tick_end = table ? (uint64_t)tt->n_epochs * (uint64_t)tt->ticks_per_epoch : (uint64_t)1 << 62;
    TraverseTimedC q;
    std::memset(&q, 0, sizeof q);
    const TraverseSteps<TraverseTimedC> steps = {mrtx_launch_timed_init, mrtx_launch_timed_relax, mrtx_launch_timed_pred};
    return traverse_run(
        c, t, q, steps, src_ij, src_tick, n_src,
        [&](int32_t k, uint64_t s) {
            return s < tick_end ? MRTX_OK
                                : fail(c, MRTX_E_INVALID, "source %d: start tick %llu must be below %llu", k, (unsigned long long)s,
                                       (unsigned long long)tick_end);
        },
        dev_penalty, host_penalty, HostSeg(host_avail, host_avail ? 2 * N * W64 : 0), dev_arrival, host_arrival, dev_pred, host_pred,
        [&](void* val, const float* start, const float* avail) {
            q.arr = static_cast<unsigned long long*>(val);
            q.src_tick = reinterpret_cast<const unsigned long long*>(start);
            q.avail = host_avail ? reinterpret_cast<const unsigned long long*>(avail) : static_cast<const unsigned long long*>(dev_avail);
            q.tpc = tt->ticks_per_cost; q.tpe = tt->ticks_per_epoch;
            q.n_epochs = table ? tt->n_epochs : 0; q.w64 = (int32_t)W64;
        },
        tile_visits, out);
}

// The window's node heights D (rows x cols float32), gathered on the device: what a route's heights are read from
int mrtx_traverse_heights(mrtx_ctx* c, const MrtxTraverse* t, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!t) return fail(c, MRTX_E_INVALID, "null window");
    int rc = traverse_params(c, t);
    if (rc != MRTX_OK) return rc;
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if (dev_out && (reinterpret_cast<uintptr_t>(dev_out) & 3)) return fail(c, MRTX_E_INVALID, "dev_out must be 4-byte aligned");
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    if ((rc = traverse_window(c, t, c->dem_h, c->dem_w, nullptr)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const size_t bytes = (size_t)t->rows * (size_t)t->cols * sizeof(float);
    if ((rc = stage_out(c, dev_out, bytes)) != MRTX_OK) return rc;
    TraverseC q;
    std::memset(&q, 0, sizeof q);
    traverse_fill_window(c, f, t, q);
    if ((rc = stage_start(c, nullptr, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_traverse_heights(q, static_cast<float*>(dev_out), c->stream));
    return stage_finish(c, dev_out, host_out, bytes, out, kNoRays);
}

// ---- Terrain relief: slope, roughness, landing hazard -------------------------------------------
// The checks that need no DEM: the window's own numbers, the footprint, the node count, the radius
static int relief_params(mrtx_ctx* c, const MrtxRelief* r) {
    if (r->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    if (r->rows < 1 || r->cols < 1) return fail(c, MRTX_E_INVALID, "empty window (%d x %d)", r->rows, r->cols);
    if ((int64_t)r->rows * (int64_t)r->cols > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a window holds at most 2^31 nodes (got %d x %d)", r->rows, r->cols);
    if (r->stride < 1) return fail(c, MRTX_E_INVALID, "stride must be >= 1 (got %d)", r->stride);
    if (r->row0 < 0 || r->col0 < 0) return fail(c, MRTX_E_INVALID, "row0 and col0 must be >= 0");
    if (r->ri < 1 || r->ri > 32 || r->rj < 1 || r->rj > 32)
        return fail(c, MRTX_E_INVALID, "the footprint's ri and rj must lie in 1 .. 32 (got %d, %d)", r->ri, r->rj);
    if (!std::isfinite(r->radius_m) || !(r->radius_m > 0.0) || !std::isfinite((float)r->radius_m))
        return fail(c, MRTX_E_INVALID, "radius_m must be finite and > 0 (also as a float32)");
    return MRTX_OK;
}

// The checks against the DEM's shape (H, W), then the rows x 2 scales (kx, ky) into out2 (each finite and > 0)
static int relief_window(mrtx_ctx* c, const MrtxRelief* r, int32_t H, int32_t W, double* out2) {
    if (H < 2 || W < 2) return fail(c, MRTX_E_INVALID, "the DEM must be at least 2 x 2 (got %d x %d)", H, W);
    if (r->row0 + (int64_t)(r->rows - 1) * r->stride >= H)
        return fail(c, MRTX_E_INVALID, "the window's last row %lld lies outside the DEM's %d rows",
                    (long long)(r->row0 + (int64_t)(r->rows - 1) * r->stride), H);
    if (r->col0 >= W) return fail(c, MRTX_E_INVALID, "col0 = %d lies outside the DEM's %d columns", r->col0, W);
    if ((int64_t)(r->cols - 1) * r->stride >= W)
        return fail(c, MRTX_E_INVALID, "the window's columns repeat: (cols - 1) x stride must be < W = %d", W);
    if ((int64_t)(2 * r->rj + 1) * r->stride > W)
        return fail(c, MRTX_E_INVALID, "the footprint goes round the circle: (2 rj + 1) x stride must be <= W = %d", W);
    const double dphi = (double)r->stride * kPiD / (double)H, dlam = (double)r->stride * 2.0 * kPiD / (double)W;
    for (int32_t i = 0; i < r->rows; i++) {
        const double row = (double)r->row0 + (double)i * r->stride;
        const double lat = 0.5 * kPiD - (row + 0.5) * (kPiD / (double)H);
        const double kx = r->radius_m / (r->radius_m * std::cos(lat) * dlam), ky = r->radius_m / (r->radius_m * dphi);
        if (!(std::isfinite(kx) && kx > 0.0 && std::isfinite(ky) && ky > 0.0))
            return fail(c, MRTX_E_INVALID, "row %d: the scales (%g, %g) are not finite and positive", i, kx, ky);
        if (out2) { out2[2 * (size_t)i] = kx; out2[2 * (size_t)i + 1] = ky; }
    }
    return MRTX_OK;
}

int mrtx_relief_scales(const MrtxRelief* r, int32_t dem_h, int32_t dem_w, double* out2) {
    if (!r || !out2) return MRTX_E_INVALID;
    const int rc = relief_params(nullptr, r);
    return rc != MRTX_OK ? rc : relief_window(nullptr, r, dem_h, dem_w, out2);
}

// Q(r) = r (r + 1)(2 r + 1) / 3 = the sum of d^2 over d = -r .. r, an exact integer
static int64_t relief_q(int64_t r) { return r * (r + 1) * (2 * r + 1) / 3; }

int mrtx_relief(mrtx_ctx* c, const MrtxRelief* r, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!r) return fail(c, MRTX_E_INVALID, "null window");
    int rc = relief_params(c, r);
    if (rc != MRTX_OK) return rc;
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if (dev_out && (reinterpret_cast<uintptr_t>(dev_out) & 15)) return fail(c, MRTX_E_INVALID, "dev_out must be 16-byte aligned (float4)");
    // MOONRT_RELIEF_TILE: the nodes a workgroup stages, 16 (16 x 16), 32 (32 x 32) or 64 (64 rows x 16 columns), or 0 = the
    // kernel that reads every footprint straight from global memory; the same bits in every case
    int tile = r->ri > 4 ? 32 : 16;
    if (const char* e = std::getenv("MOONRT_RELIEF_TILE")) {
        tile = std::atoi(e);
        if ((tile != 0 || std::strcmp(e, "0") != 0) && tile != 16 && tile != 32 && tile != 64)
            return fail(c, MRTX_E_INVALID, "MOONRT_RELIEF_TILE must be 0, 16, 32 or 64 (got %s)", e);
    }
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    std::vector<double> scale((size_t)r->rows * 2);
    if ((rc = relief_window(c, r, c->dem_h, c->dem_w, scale.data())) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    const size_t bytes = (size_t)r->rows * (size_t)r->cols * 16;
    float* d[1];
    if ((rc = stage_out(c, dev_out, bytes)) != MRTX_OK || (rc = stage_tables(c, {{scale.data(), 2 * scale.size()}}, d)) != MRTX_OK)
        return rc;
    ReliefC q;
    std::memset(&q, 0, sizeof q);
    q.dem = f.dem; q.dem_pitch = f.dem_pitch; q.dem_h = c->dem_h; q.dem_w = c->dem_w;
    q.row0 = r->row0; q.col0 = r->col0; q.rows = r->rows; q.cols = r->cols; q.stride = r->stride; q.ri = r->ri; q.rj = r->rj;
    q.scale = reinterpret_cast<const double*>(d[0]);
    const int64_t nj = 2 * r->rj + 1, ni = 2 * r->ri + 1;
    q.inv_n = 1.0 / (double)(ni * nj);
    q.inv_xj = 1.0 / (double)(ni * relief_q(r->rj));
    q.inv_xi = 1.0 / (double)(nj * relief_q(r->ri));
    q.rm = (float)r->radius_m;
    q.out = static_cast<float4*>(dev_out);
    q.fetches = stats ? c->illum_stats + 6 : nullptr;
    if ((rc = stage_start(c, nullptr, stats)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_relief(q, tile, c->stream));
    return stage_finish(c, dev_out, host_out, bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_relief_share(mrtx_ctx* c, const MrtxReliefShare* s, const void* dev_relief, const float* host_relief, void* dev_out,
                      float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!s) return fail(c, MRTX_E_INVALID, "null share");
    if (s->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    if (s->rows < 1 || s->cols < 1) return fail(c, MRTX_E_INVALID, "empty map (%d x %d)", s->rows, s->cols);
    if ((int64_t)s->rows * (int64_t)s->cols > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a map holds at most 2^31 nodes (got %d x %d)", s->rows, s->cols);
    if (s->Ri < 0 || s->Ri > 1024 || s->Rj < 0 || s->Rj > 1024)
        return fail(c, MRTX_E_INVALID, "the box's Ri and Rj must lie in 0 .. 1024 (got %d, %d)", s->Ri, s->Rj);
    if (s->wrap != 0 && s->wrap != 1) return fail(c, MRTX_E_INVALID, "wrap must be 0 or 1 (got %d)", s->wrap);
    if (s->wrap && s->cols < 3) return fail(c, MRTX_E_INVALID, "a wrapped map needs cols >= 3 (got %d)", s->cols);
    if (!(s->grade_max >= 0.0) || !(s->rms_max >= 0.0)) return fail(c, MRTX_E_INVALID, "grade_max and rms_max must be >= 0 (+inf: no limit)");
    if ((dev_relief == nullptr) == (host_relief == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_relief and host_relief");
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if (dev_relief && (reinterpret_cast<uintptr_t>(dev_relief) & 15)) return fail(c, MRTX_E_INVALID, "dev_relief must be 16-byte aligned (float4)");
    if (dev_out && (reinterpret_cast<uintptr_t>(dev_out) & 3)) return fail(c, MRTX_E_INVALID, "dev_out must be 4-byte aligned (float32)");
    const size_t N = (size_t)s->rows * (size_t)s->cols;
    if (spans_overlap(dev_relief, 16 * N, dev_out, 4 * N)) return fail(c, MRTX_E_INVALID, "dev_relief and dev_out must not overlap");
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc;
    float* d[1] = {nullptr};
    if ((rc = stage_out(c, dev_out, 4 * N)) != MRTX_OK || (rc = stage_buffer(c, c->trav_buf, c->trav_bytes, 4 * N)) != MRTX_OK ||
        (rc = stage_tables(c, {{host_relief, host_relief ? 4 * N : 0}}, d)) != MRTX_OK)
        return rc;
    ShareC q;
    std::memset(&q, 0, sizeof q);
    q.relief = host_relief ? reinterpret_cast<const float4*>(d[0]) : static_cast<const float4*>(dev_relief);
    q.sat = reinterpret_cast<uint32_t*>(c->trav_buf);
    q.out = static_cast<float*>(dev_out);
    q.rows = s->rows; q.cols = s->cols; q.Ri = s->Ri; q.Rj = s->Rj; q.wrap = s->wrap;
    q.gmax = (float)s->grade_max; q.smax = (float)s->rms_max;
    if ((rc = stage_start(c, nullptr, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_relief_share(q, c->stream));
    if ((rc = stage_finish(c, dev_out, host_out, 4 * N, out, kNoRays)) != MRTX_OK) return rc;
    if (out) out->launches = 3;
    return MRTX_OK;
}

// ---- Regolith surface temperatures ---------------------------------------------------------------
static double thermal_c(const MrtxThermalModel& md, double T) {
    return md.c[0] + T * (md.c[1] + T * (md.c[2] + T * (md.c[3] + T * md.c[4])));
}

// the model's checks; on success the step bound Delta_max at F = 1/2 (section 3.10) is in *dmax
static int thermal_model_ok(mrtx_ctx* c, const MrtxThermalModel& md, int32_t m, int32_t mode, double* dmax) {
    const int n = md.n_nodes;
    if (n < 3 || n > MRTX_THERMAL_MAX_NODES)
        return fail(c, MRTX_E_INVALID, "n_nodes must lie in [3, %d] (got %d)", MRTX_THERMAL_MAX_NODES, n);
    for (int i = 0; i < n; i++) {
        if (!(std::isfinite(md.rho[i]) && md.rho[i] > 0.0) || !(std::isfinite(md.kc[i]) && md.kc[i] > 0.0) ||
            (i < n - 1 && !(std::isfinite(md.dz[i]) && md.dz[i] > 0.0)))
            return fail(c, MRTX_E_INVALID, "node %d: dz, rho and kc must be finite and positive", i);
    }
    bool fin = std::isfinite(md.chi) && std::isfinite(md.emissivity) && std::isfinite(md.sigma) && std::isfinite(md.q_geo);
    for (int i = 0; i < 5; i++) fin = fin && std::isfinite(md.c[i]);
    for (int i = 0; i < 3; i++) fin = fin && std::isfinite(md.albedo[i]);
    if (!fin) return fail(c, MRTX_E_INVALID, "the model's constants must be finite");
    if (!(md.chi >= 0.0) || !(md.emissivity > 0.0) || !(md.sigma > 0.0) || !(md.q_geo >= 0.0) || !(md.albedo[0] >= 0.0) ||
        !(md.albedo[0] < 1.0))
        return fail(c, MRTX_E_INVALID, "need chi >= 0, emissivity > 0, sigma > 0, q_geo >= 0 and 0 <= A0 < 1");
    // A(theta) must be a reflectance at every incidence (a law above 1 at grazing incidence would absorb a negative flux)
    for (int t = 0; t <= 900; t++) {
        const double th = 0.1 * t, x = th / 45.0, y = th / 90.0, y2 = y * y, y4 = y2 * y2;
        const double A = md.albedo[0] + md.albedo[1] * x * x * x + md.albedo[2] * y4 * y4;
        if (!(A >= 0.0 && A <= 1.0))
            return fail(c, MRTX_E_INVALID, "the albedo A(theta) = %g at theta = %.1f deg lies outside [0, 1]", A, th);
    }
    // a never-lit column settles on the geothermal floor (q_geo / (eps sigma))^(1/4), which must lie inside [20, 450] K too
    const double q_floor = md.emissivity * md.sigma * (20.0 * 20.0 * 20.0 * 20.0);
    if (!(md.q_geo >= q_floor))
        return fail(c, MRTX_E_INVALID,
                    "q_geo = %g W/m^2 puts the geothermal floor (q_geo / (eps sigma))^(1/4) at %.2f K, below 20 K: need q_geo >= "
                    "eps sigma 20^4 = %g W/m^2", md.q_geo, std::pow(md.q_geo / (md.emissivity * md.sigma), 0.25), q_floor);
    if (!(std::isfinite(md.spacing_s) && md.spacing_s > 0.0)) return fail(c, MRTX_E_INVALID, "spacing_s must be positive");
    if (md.n_sub < 1) return fail(c, MRTX_E_INVALID, "n_sub must be >= 1 (got %d)", md.n_sub);
    if (md.block < 1) return fail(c, MRTX_E_INVALID, "block must be >= 1 (got %d)", md.block);
    if (md.n_spin < 0 || (mode != 2 && md.n_spin >= m))
        return fail(c, MRTX_E_INVALID, "n_spin must lie in [0, m) (got %d for m = %d)", md.n_spin, m);
    if (md.n_reset < 0 || (int64_t)md.n_reset * md.block > md.n_spin)
        return fail(c, MRTX_E_INVALID, "need 0 <= n_reset and n_reset * block <= n_spin");
    if (md.ref_node < 1 || md.ref_node > n - 2) return fail(c, MRTX_E_INVALID, "ref_node must lie in [1, n_nodes - 2]");
    // Delta_max = 1/2 min_i rho_i min(dz_{i-1}, dz_i)^2 min_{T in [20, 450] K, 1 K grid} c(T) / k_i(T) over the interior nodes
    double best = INFINITY;
    for (int T = 20; T <= 450; T++) {
        const double cT = thermal_c(md, (double)T), r = (double)T / 350.0;
        if (!(cT > 0.0)) return fail(c, MRTX_E_INVALID, "the heat capacity must be positive on [20, 450] K");
        for (int i = 1; i < n - 1; i++) {
            const double dz = std::min(md.dz[i - 1], md.dz[i]);
            best = std::min(best, md.rho[i] * dz * dz * cT / (md.kc[i] * (1.0 + md.chi * r * r * r)));
        }
    }
    *dmax = 0.5 * best;
    if (!(md.spacing_s / md.n_sub <= *dmax))
        return fail(c, MRTX_E_INVALID, "spacing_s / n_sub = %g s exceeds the stable step %g s", md.spacing_s / md.n_sub, *dmax);
    return MRTX_OK;
}

// the sublimation law of VOLATILE (section 3.16): finite, strictly increasing on [20, 450] K (the 1 K grid, as
// thermal_model_ok scans c(T)), and exp(x) finite at the top of the range
static int volatile_ok(mrtx_ctx* c, const MrtxVolatile& sp) {
    const double* b = sp.b;
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(b[i])) return fail(c, MRTX_E_INVALID, "the species' coefficient b[%d] must be finite", i);
    for (int T = 20; T <= 450; T++) {
        const double t = (double)T;
        if (!(b[1] / (t * t) + b[2] / t + b[3] > 0.0))
            return fail(c, MRTX_E_INVALID, "the species' law must increase on [20, 450] K: d ln E / dT <= 0 at %d K", T);
    }
    const double x_top = std::fma(b[3], 450.0, std::fma(b[2], std::log(450.0), b[0] - b[1] / 450.0));
    if (!(x_top <= 700.0))
        return fail(c, MRTX_E_INVALID, "the species' ln E(450 K) = %g exceeds 700: exp would overflow", x_top);
    return MRTX_OK;
}

// what each entry point accepts: mrtx_thermal modes 0-2; mrtx_thermal_scatter (section 3.11) also mode 3 EXITANCE and the
// extra flux table, exactly one of dev_extra and host_extra or neither, with at least n x m entries; mrtx_thermal_column
// (section 3.16) also modes 4 COLUMN and 5 VOLATILE, the latter with a species
enum ThermalEntry { kThermal = 0, kThermalScatter = 1, kThermalColumn = 2 };

static int thermal_run(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                       const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux, int32_t m,
                       const MrtxThermalModel* model, int32_t mode, void* dev_out, void* host_out, MrtxStats* out,
                       ThermalEntry entry, const void* dev_extra, const float* host_extra, int64_t extra_len,
                       const MrtxVolatile* species, const MrtxIllumEpoch* occ_source = nullptr,
                       const MrtxIllumEpoch* occ_body = nullptr) {
    const bool ext = entry != kThermal;
    if (!c) return MRTX_E_INVALID;
    if ((occ_source == nullptr) != (occ_body == nullptr))
        return fail(c, MRTX_E_INVALID, "give both occultation tables or neither");
    if (!latlon || !epochs || !flux || !model) return fail(c, MRTX_E_INVALID, "null point list, epoch table, flux or model");
    if (n < 1 || m < 1) return fail(c, MRTX_E_INVALID, "n and m must be >= 1 (got %d, %d)", n, m);
    if (m > (1 << 24)) return fail(c, MRTX_E_INVALID, "at most 2^24 epochs per call (got %d)", m);
    if (!horizon_az_ok(n_az)) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    if (entry == kThermal && (mode < 0 || mode > 2))
        return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL), 1 (SUMMARY) or 2 (FLUX) (got %d)", mode);
    if (entry == kThermalScatter && (mode < 0 || mode > 3))
        return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL), 1 (SUMMARY), 2 (FLUX) or 3 (EXITANCE) (got %d)", mode);
    if (entry == kThermalColumn && (mode < 0 || mode > 5))
        return fail(c, MRTX_E_INVALID,
                    "mode must be 0 (FULL), 1 (SUMMARY), 2 (FLUX), 3 (EXITANCE), 4 (COLUMN) or 5 (VOLATILE) (got %d)", mode);
    if ((mode == 5) != (species != nullptr))
        return fail(c, MRTX_E_INVALID, "a species is required in mode 5 (VOLATILE) and must be null in every other mode");
    if (species) { const int rc_ = volatile_ok(c, *species); if (rc_ != MRTX_OK) return rc_; }
    if (mode == 5 && ((uintptr_t)dev_out & 7))
        return fail(c, MRTX_E_INVALID, "VOLATILE writes float64 pairs: dev_out must be 8-byte aligned");
    if (dev_extra && host_extra) return fail(c, MRTX_E_INVALID, "give at most one of dev_extra and host_extra");
    const bool have_extra = dev_extra || host_extra;
    if (have_extra && extra_len < (int64_t)n * (int64_t)m)
        return fail(c, MRTX_E_INVALID, "the extra-flux table holds %lld entries, fewer than n x m = %lld", (long long)extra_len,
                    (long long)n * (long long)m);
    double x_max = 0.0;         // the largest host extra flux: it joins the radiative-equilibrium check below
    if (host_extra) {
        const size_t ne = (size_t)n * (size_t)m;
        for (size_t i = 0; i < ne; i++) {
            if (!(std::isfinite(host_extra[i]) && host_extra[i] >= 0.0f))
                return fail(c, MRTX_E_INVALID, "extra-flux entry %zu must be finite and >= 0 (got %g)", i, (double)host_extra[i]);
            x_max = std::max(x_max, (double)host_extra[i]);
        }
    }
    int rc = horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, static_cast<const float*>(host_out));
    if (rc != MRTX_OK) return rc;
    const MrtxThermalModel& md = *model;
    double dmax = 0.0;
    if ((rc = thermal_model_ok(c, md, m, mode, &dmax)) != MRTX_OK) return rc;
    // outputs per point; VOLATILE's are float64
    const int64_t width = mode == 0 ? (int64_t)m - md.n_spin : mode == 2 ? (int64_t)m : mode == 3 ? 2 * ((int64_t)m - md.n_spin) :
                          mode == 4 ? ((int64_t)m - md.n_spin) * md.n_nodes : mode == 5 ? 2 * (int64_t)md.n_nodes : 4;
    if ((int64_t)n * width > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a call holds at most 2^31 outputs: split the points into more calls");
    double s_max = 0.0;
    for (int32_t k = 0; k < m; k++) {
        if (!std::isfinite(flux[k]) || !(flux[k] >= 0.0))
            return fail(c, MRTX_E_INVALID, "epoch %d: the solar flux must be finite and >= 0 (got %g)", k, flux[k]);
        s_max = std::max(s_max, flux[k]);
    }
    // the hottest the surface can get, radiative equilibrium under the largest absorbed flux (a host extra table's largest
    // entry added; a device table is not scanned), must stay inside the range the step bound covers
    double a_max = 0.0;
    for (int t = 0; t <= 900; t++) {
        const double th = 0.1 * t, x = th / 45.0, y = th / 90.0, y2 = y * y, y4 = y2 * y2;
        const double A = md.albedo[0] + md.albedo[1] * x * x * x + md.albedo[2] * y4 * y4;
        a_max = std::max(a_max, (1.0 - A) * std::cos(th * (M_PI / 180.0)));
    }
    if (mode != 2) {
        const double t_eq = std::pow((a_max * s_max + x_max + md.q_geo) / (md.emissivity * md.sigma), 0.25);
        if (!(t_eq <= 450.0))
            return fail(c, MRTX_E_INVALID, "the radiative-equilibrium temperature %.1f K exceeds 450 K, the model's range", t_eq);
    }
    if ((rc = horizon_entries(c, host_horizon, n, n_az)) != MRTX_OK) return rc;
    std::vector<float> rtab, ctab, lights;
    if ((rc = point_tables(c, latlon, n, rtab, ctab)) != MRTX_OK) return rc;
    if ((rc = epoch_lights(c, epochs, m, lights)) != MRTX_OK) return rc;
    std::vector<float> occ_s, occ_b, occ_m;     // section 3.18: empty segments without the tables
    if (occ_source && (rc = occult_tables(c, occ_source, occ_body, m, occ_s, occ_b, occ_m)) != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, false)) != MRTX_OK) return rc;
    std::vector<float> fl((size_t)m);
    for (int32_t k = 0; k < m; k++) fl[k] = (float)flux[k];
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    const size_t nx = host_extra ? (size_t)n * (size_t)m : 0;
    const size_t out_bytes = (size_t)n * (size_t)width * (mode == 5 ? sizeof(double) : sizeof(float));
    float* d[9];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK ||
        (rc = stage_tables(c, {rtab, ctab, lights, fl, {host_horizon, nh}, {host_extra, nx}, occ_s, occ_b, occ_m}, d)) != MRTX_OK)
        return rc;
    ThermalC q;
    std::memset(&q, 0, sizeof q);
    if (occ_source) { q.occ_src = d[6]; q.occ_body = d[7]; q.occ_mark = reinterpret_cast<const int32_t*>(d[8]); }
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.horizon = host_horizon ? d[4] : (const float*)dev_horizon;
    q.lights = d[2]; q.flux = d[3]; q.out = (float*)dev_out; q.caps = c->illum_stats;
    q.xflux = host_extra ? d[5] : (const float*)dev_extra;
    q.az_log2 = log2_of(n_az); q.m = m; q.mode = mode;
    if (species) for (int i = 0; i < 4; i++) q.vb[i] = species->b[i];
    const int nn = md.n_nodes;
    q.n_nodes = nn; q.n_sub = md.n_sub; q.n_spin = md.n_spin; q.block = md.block; q.n_reset = md.n_reset; q.ref = md.ref_node;
    const double delta = md.spacing_s / md.n_sub;
    q.es = (float)(md.emissivity * md.sigma);
    q.q_geo = (float)md.q_geo;
    q.chi3 = (float)(md.chi / (350.0 * 350.0 * 350.0));
    for (int i = 0; i < 5; i++) q.c[i] = (float)md.c[i];
    for (int i = 0; i < 3; i++) q.alb[i] = (float)md.albedo[i];
    q.inv_dz0 = (float)(1.0 / md.dz[0]);
    for (int i = 0; i < nn; i++) {
        q.kc[i] = (float)md.kc[i];
        if (i < nn - 1) q.hdz[i] = (float)(0.5 / md.dz[i]);
        if (i < nn - 1) q.qdz[i] = (float)(md.q_geo * md.dz[i]);
        if (i > 0 && i < nn - 1) q.a[i] = (float)(delta * 2.0 / (md.rho[i] * (md.dz[i - 1] + md.dz[i])));
    }
    if ((rc = stage_start(c, &cold, true)) != MRTX_OK) return rc;      // the counters: q.caps
    HIPCHK(c, mrtx_launch_thermal(f, q, ext, c->stream));
    if ((rc = stage_finish(c, dev_out, static_cast<float*>(host_out), out_bytes, out, kNoRays)) != MRTX_OK) return rc;
    unsigned long long cnt[2] = {0, 0};      // Newton cap hits, (point, epoch)s whose column left [20, 450] K
    HIPCHK(c, hipMemcpy(cnt, c->illum_stats, sizeof cnt, hipMemcpyDeviceToHost));
    if (out) out->reserved = cnt[0] > 0xffffffffull ? 0xffffffffu : (uint32_t)cnt[0];
    if (cnt[1])
        return fail(c, MRTX_E_INVALID,
                    "the column left the model's range [20, 450] K (or became non-finite) after the steps of %llu (point, epoch)s: "
                    "the output is not valid (an extra flux too large for the step, or a transient past the step bound)",
                    cnt[1]);
    return MRTX_OK;
}

int mrtx_thermal(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon, const float* host_horizon,
                 const MrtxIllumEpoch* epochs, const double* flux, int32_t m, const MrtxThermalModel* model, int32_t mode,
                 void* dev_out, float* host_out, MrtxStats* out) {
    return thermal_run(c, latlon, n, n_az, dev_horizon, host_horizon, epochs, flux, m, model, mode, dev_out, host_out, out,
                       kThermal, nullptr, nullptr, 0, nullptr);
}

int mrtx_thermal_scatter(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                         const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux, int32_t m,
                         const MrtxThermalModel* model, int32_t mode, const void* dev_extra, const float* host_extra,
                         int64_t extra_len, void* dev_out, float* host_out, MrtxStats* out) {
    return thermal_run(c, latlon, n, n_az, dev_horizon, host_horizon, epochs, flux, m, model, mode, dev_out, host_out, out,
                       kThermalScatter, dev_extra, host_extra, extra_len, nullptr);
}

// ---- Subsurface temperature columns and volatile loss rates --------------------------------------
int mrtx_thermal_column(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                        const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux, int32_t m,
                        const MrtxThermalModel* model, int32_t mode, const void* dev_extra, const float* host_extra,
                        int64_t extra_len, const MrtxVolatile* species, void* dev_out, void* host_out, MrtxStats* out) {
    return thermal_run(c, latlon, n, n_az, dev_horizon, host_horizon, epochs, flux, m, model, mode, dev_out, host_out, out,
                       kThermalColumn, dev_extra, host_extra, extra_len, species);
}

// ---- The thermal column under the Earth's occultation of the Sun ----------------------------------
int mrtx_thermal_occulted(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                          const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux, int32_t m,
                          const MrtxThermalModel* model, int32_t mode, const void* dev_extra, const float* host_extra,
                          int64_t extra_len, const MrtxVolatile* species, const MrtxIllumEpoch* occ_source,
                          const MrtxIllumEpoch* occ_body, void* dev_out, void* host_out, MrtxStats* out) {
    return thermal_run(c, latlon, n, n_az, dev_horizon, host_horizon, epochs, flux, m, model, mode, dev_out, host_out, out,
                       kThermalColumn, dev_extra, host_extra, extra_len, species, occ_source, occ_body);
}

// ---- Terrain-scattered sunlight and infrared -------------------------------------------------------
static bool view_k_ok(int32_t k) { return k >= 16 && k <= 1024 && (k & (k - 1)) == 0; }

int mrtx_view_dir_samples(int32_t k, float* out2) {
    if (!view_k_ok(k) || !out2) return MRTX_E_INVALID;
    for (int32_t j = 0; j < k; j++) {
        const double t = (double)j * 0.6180339887498949;
        out2[2 * j] = (float)(((double)j + 0.5) / (double)k);
        out2[2 * j + 1] = (float)(t - std::floor(t));
    }
    return MRTX_OK;
}

int mrtx_view_hits(mrtx_ctx* c, const double* latlon, int32_t n, int32_t k, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon) return fail(c, MRTX_E_INVALID, "null point list");
    if (n < 1) return fail(c, MRTX_E_INVALID, "n must be >= 1 (got %d)", n);
    if (!view_k_ok(k)) return fail(c, MRTX_E_INVALID, "K must be 16, 32, ..., 1024 (got %d)", k);
    if ((int64_t)n * (2 * (int64_t)k + 1) > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a call holds at most 2^31 outputs: split the points into more calls");
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    std::vector<float> rtab, ctab, dirs((size_t)k * 2);
    int rc = point_tables(c, latlon, n, rtab, ctab);
    if (rc != MRTX_OK) return rc;
    FrameC f;
    FrameCold cold;
    if ((rc = stage_frame(c, f, cold, true)) != MRTX_OK) return rc;
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    mrtx_view_dir_samples(k, dirs.data());
    const size_t out_bytes = (size_t)n * (2 * (size_t)k + 1) * sizeof(float);
    float* d[3];
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK || (rc = stage_tables(c, {rtab, ctab, dirs}, d)) != MRTX_OK) return rc;
    ViewC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.dirs = d[2];
    q.out = (float*)dev_out; q.K = k;
    if ((rc = stage_start(c, &cold, stats)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_view_hits(f, q, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kBounceRays : kNoRays);
}

int mrtx_scatter_flux(mrtx_ctx* c, const int32_t* index, int32_t n, int32_t k, const void* dev_exitance,
                      const float* host_exitance, int64_t exitance_len, int32_t n_hits, int32_t m, double albedo_h,
                      double emissivity, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!index) return fail(c, MRTX_E_INVALID, "null index table");
    if (n < 1 || m < 1 || n_hits < 0) return fail(c, MRTX_E_INVALID, "need n >= 1, m >= 1 and n_hits >= 0 (got %d, %d, %d)", n, m, n_hits);
    if (!view_k_ok(k)) return fail(c, MRTX_E_INVALID, "K must be 16, 32, ..., 1024 (got %d)", k);
    if (!(std::isfinite(albedo_h) && albedo_h >= 0.0 && albedo_h < 1.0))
        return fail(c, MRTX_E_INVALID, "the hemispherical albedo must be finite and in [0, 1) (got %g)", albedo_h);
    if (!(std::isfinite(emissivity) && emissivity > 0.0 && emissivity <= 1.0))
        return fail(c, MRTX_E_INVALID, "the emissivity must be finite and in (0, 1] (got %g)", emissivity);
    if ((dev_exitance == nullptr) == (host_exitance == nullptr))
        return fail(c, MRTX_E_INVALID, "give exactly one of dev_exitance and host_exitance");
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if ((int64_t)n * (int64_t)m > (int64_t)1 << 31 || (int64_t)n_hits * (int64_t)m > (int64_t)1 << 30)
        return fail(c, MRTX_E_INVALID, "a call holds at most 2^31 outputs and 2^30 exitance pairs: split the targets");
    if (exitance_len < 2 * (int64_t)n_hits * (int64_t)m)
        return fail(c, MRTX_E_INVALID, "the exitance table holds %lld floats, fewer than n_hits x m x 2 = %lld",
                    (long long)exitance_len, 2 * (long long)n_hits * (long long)m);
    const size_t ni = (size_t)n * (size_t)k;
    for (size_t i = 0; i < ni; i++)
        if (index[i] < -1 || index[i] >= n_hits)
            return fail(c, MRTX_E_INVALID, "index entry %zu = %d lies outside the hit list [0, %d) (-1: sky)", i, index[i], n_hits);
    const size_t ne = host_exitance ? (size_t)n_hits * (size_t)m * 2 : 0;
    for (size_t i = 0; i < ne; i++)
        if (!(std::isfinite(host_exitance[i]) && host_exitance[i] >= 0.0f))
            return fail(c, MRTX_E_INVALID, "exitance entry %zu must be finite and >= 0", i);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t out_bytes = (size_t)n * (size_t)m * sizeof(float);
    float* d[2];
    int rc;
    if ((rc = stage_out(c, dev_out, out_bytes)) != MRTX_OK ||
        (rc = stage_tables(c, {{index, ni}, {host_exitance, ne}}, d)) != MRTX_OK)
        return rc;
    ScatterC q;
    std::memset(&q, 0, sizeof q);
    q.idx = reinterpret_cast<const int32_t*>(d[0]);
    q.ex = host_exitance ? d[1] : (const float*)dev_exitance;   // (n_hits = 0: never read, but not null)
    q.out = (float*)dev_out;
    q.n = n; q.K = k; q.m = m; q.chunks = (m + 63) / 64;
    q.omah = (float)(1.0 - albedo_h); q.eps = (float)emissivity; q.inv_k = (float)(1.0 / k);
    if ((rc = stage_start(c, nullptr, false)) != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_scatter_flux(q, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays);
}

int mrtx_samples_done(mrtx_ctx* c, uint32_t* out) {
    if (!c || !out) return MRTX_E_INVALID;
    *out = c->blocks_done * c->prm.spp_per_launch;
    return MRTX_OK;
}

// Thresholds of the exact "Gamma" post-process: T[0] = 0 (never read as a threshold),
// T[j] = (float)pow((j - 0.5) / n, gamma) for j = 1..n, float64 on the host, rounded once; n + 1 entries on the device,
// rebuilt when tonemap_gamma changes.  Level = #{j : exposure * mean >= T[j]} = round(n * (exposure * mean)^(1/gamma)).
static int tone_table(mrtx_ctx* c, int n, float** dev, float* built_for) {
    if (*dev && *built_for == c->prm.tonemap_gamma) return MRTX_OK;
    std::vector<float> T((size_t)n + 1);
    const double g = (double)c->prm.tonemap_gamma;
    T[0] = 0.0f;
    for (int j = 1; j <= n; j++) T[(size_t)j] = (float)pow(((double)j - 0.5) / (double)n, g);
    if (!*dev) HIPCHK(c, hipMalloc((void**)dev, T.size() * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(*dev, T.data(), T.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // T is a local
    *built_for = c->prm.tonemap_gamma;
    return MRTX_OK;
}

int mrtx_read_linear(mrtx_ctx* c, float* out) {
    if (!c || !out) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int64_t npix = (int64_t)c->cfg.width * c->cfg.height;
    HIPCHK(c, mrtx_launch_resolve_linear(c->accum, (float*)c->scratch, npix, c->blocks_done * c->prm.spp_per_launch, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->scratch, (size_t)npix * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MRTX_OK;
}
int mrtx_read_rgba8(mrtx_ctx* c, uint8_t* out) {
    if (!c || !out) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int64_t npix = (int64_t)c->cfg.width * c->cfg.height;
    const int rc = tone_table(c, 255, &c->tone8_dev, &c->tone8_gamma);
    if (rc != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_resolve_rgba8(c->accum, (uint32_t*)c->scratch, npix, c->blocks_done * c->prm.spp_per_launch,
                                        c->prm.tonemap_exposure, c->tone8_dev, c->overlay, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->scratch, (size_t)npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MRTX_OK;
}
int mrtx_read_rgb16(mrtx_ctx* c, uint16_t* out) {
    if (!c || !out) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int64_t npix = (int64_t)c->cfg.width * c->cfg.height;
    const int rc = tone_table(c, 65535, &c->tone16_dev, &c->tone16_gamma);
    if (rc != MRTX_OK) return rc;
    HIPCHK(c, mrtx_launch_resolve_rgb16(c->accum, (uint16_t*)c->scratch, npix, c->blocks_done * c->prm.spp_per_launch,
                                        c->prm.tonemap_exposure, c->tone16_dev, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->scratch, (size_t)npix * 6, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MRTX_OK;
}
int mrtx_read_hits(mrtx_ctx* c, float* out) {
    if (!c || !out) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t bytes = (size_t)c->cfg.width * c->cfg.height * 16;
    HIPCHK(c, hipMemcpyAsync(out, c->hits, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MRTX_OK;
}

int mrtx_read_hit(mrtx_ctx* c, int32_t x, int32_t y, float out[4]) {
    if (!c || !out) return MRTX_E_INVALID;
    if (x < 0 || y < 0 || x >= c->cfg.width || y >= c->cfg.height) return fail(c, MRTX_E_INVALID, "pixel (%d, %d) outside the frame", x, y);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(out, c->hits + 4 * ((size_t)y * (size_t)c->cfg.width + (size_t)x), 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MRTX_OK;
}

// The layout both ends of the gather use for the scene as it stands: active tiles only while the sky cull is in force
// (no environment map, no overlay geometry, culling not disabled), the full layout otherwise.  Every rank derives
// every rank's list from its own copy of the scene -- identical on all ranks by contract -- so nothing is negotiated.
static int gather_layout(mrtx_ctx* c) {
    if (c->act_version == c->scene_version) return MRTX_OK;
    c->act_on = false;
    c->act_slots = c->slots;
    const bool can = c->cfg.world > 1 && !(c->prm.flags & MRTX_F_NO_CULL) && c->bg == nullptr && c->caps_host.empty();
    if (can) {
        c->act_lists.assign((size_t)c->cfg.world, std::vector<int32_t>());
        int longest = 0;
        uint64_t px = 0;
        for (int r = 0; r < c->cfg.world; r++) {
            cull_tiles(c, r, c->act_lists[(size_t)r], px);
            longest = std::max(longest, (int)c->act_lists[(size_t)r].size());
        }
        if (longest < c->slots) { c->act_on = true; c->act_slots = longest; }
    }
    c->act_version = c->scene_version;
    return MRTX_OK;
}
static int upload_layout(mrtx_ctx* c) {
    if (!c->act_on || c->act_uploaded_version == c->act_version) return MRTX_OK;
    const size_t n = (size_t)c->cfg.world * (size_t)std::max(1, c->act_slots);
    std::vector<int32_t> flat(n, -1);
    for (int r = 0; r < c->cfg.world; r++)
        std::copy(c->act_lists[(size_t)r].begin(), c->act_lists[(size_t)r].end(), flat.begin() + (size_t)r * (size_t)c->act_slots);
    if (c->act_dev_cap < n) {
        if (c->act_dev) { HIPCHK(c, hipFree(c->act_dev)); c->act_dev = nullptr; }
        HIPCHK(c, hipMalloc((void**)&c->act_dev, n * sizeof(int32_t)));
        c->act_dev_cap = n;
    }
    HIPCHK(c, h2d(c, c->act_dev, flat.data(), n * sizeof(int32_t)));
    c->act_uploaded_version = c->act_version;
    return MRTX_OK;
}
static const int32_t* layout_list(const mrtx_ctx* c, int rank) {
    return c->act_on ? c->act_dev + (size_t)rank * (size_t)c->act_slots : nullptr;
}
// root: tiles of other ranks that still hold an earlier view's data and are sky now must read as zero
static int clear_stale_peer_tiles(mrtx_ctx* c) {
    if (c->peer_written.size() != (size_t)c->n_tiles) c->peer_written.assign((size_t)c->n_tiles, 0);
    if (!c->act_on) return MRTX_OK;
    std::vector<uint8_t> active((size_t)c->n_tiles, 0);
    for (int r = 0; r < c->cfg.world; r++)
        for (int32_t lt : c->act_lists[(size_t)r]) active[(size_t)lt * (size_t)c->cfg.world + (size_t)r] = 1;
    std::vector<int32_t> stale;
    for (int t = 0; t < c->n_tiles; t++)
        if (t % c->cfg.world != c->cfg.rank && c->peer_written[(size_t)t] && !active[(size_t)t]) { stale.push_back(t); c->peer_written[(size_t)t] = 0; }
    if (stale.empty()) return MRTX_OK;
    if (c->stale_cap < stale.size()) {
        if (c->stale_dev) { HIPCHK(c, hipFree(c->stale_dev)); c->stale_dev = nullptr; }
        HIPCHK(c, hipMalloc((void**)&c->stale_dev, (size_t)c->n_tiles * sizeof(int32_t)));
        c->stale_cap = (size_t)c->n_tiles;
    }
    HIPCHK(c, h2d(c, c->stale_dev, stale.data(), stale.size() * sizeof(int32_t)));
    HIPCHK(c, mrtx_launch_zero_tiles(c->accum, c->hits, c->stale_dev, (int)stale.size(), c->cfg.width, c->cfg.height,
                                     c->cfg.tile_w, c->cfg.tile_h, c->tiles_x, c->tile_shift, c->stream));
    return MRTX_OK;
}
static void mark_peer_written(mrtx_ctx* c, int src_rank) {
    if (c->peer_written.size() != (size_t)c->n_tiles) c->peer_written.assign((size_t)c->n_tiles, 0);
    if (c->act_on) {
        for (int32_t lt : c->act_lists[(size_t)src_rank]) c->peer_written[(size_t)lt * (size_t)c->cfg.world + (size_t)src_rank] = 1;
    } else {
        for (int t = src_rank; t < c->n_tiles; t += c->cfg.world) c->peer_written[(size_t)t] = 1;
    }
}

int mrtx_set_gather_hits(mrtx_ctx* c, int32_t on) {
    if (!c) return MRTX_E_INVALID;
    c->gather_hits = on != 0;
    return MRTX_OK;
}
int mrtx_shard_bytes(mrtx_ctx* c, int32_t rank, uint64_t* out) {
    if (!c || !out || rank < 0 || rank >= c->cfg.world) return MRTX_E_INVALID;
    *out = (uint64_t)c->slots * c->cfg.tile_w * c->cfg.tile_h * (c->gather_hits ? 32ull : 16ull);  // equal for every rank (padded): the upper bound
    return MRTX_OK;
}
int mrtx_shard_bytes_active(mrtx_ctx* c, uint64_t* out) {
    if (!c || !out) return MRTX_E_INVALID;
    const int rc = gather_layout(c);
    if (rc != MRTX_OK) return rc;
    *out = (uint64_t)c->act_slots * c->cfg.tile_w * c->cfg.tile_h * (c->gather_hits ? 32ull : 16ull);
    return MRTX_OK;
}
int mrtx_pack_shard(mrtx_ctx* c, void* dev_dst, void* hip_stream) { return mrtx_pack_part(c, dev_dst, 0, 1, nullptr, nullptr, hip_stream); }

// Part `part` of `n_parts` of the shard: the slots whose tiles mrtx_render_part(.., part, n_parts) rendered (own
// tiles first come first; the padding up to the common slot count goes with the last part).
int mrtx_pack_part(mrtx_ctx* c, void* dev_dst, int32_t part, int32_t n_parts, uint64_t* byte_off, uint64_t* byte_len,
                   void* hip_stream) {
    if (!c || !dev_dst || n_parts < 1 || part < 0 || part >= n_parts) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = gather_layout(c);
    if (rc == MRTX_OK) rc = upload_layout(c);
    if (rc != MRTX_OK) return rc;
    if (n_parts > 1 && !c->act_on) return fail(c, MRTX_E_STATE, "the shard moves in parts only in the active layout (mrtx_shard_parts)");
    // every rank cuts at the SAME slot numbers (parts of the longest list), so part k of every peer lands at one offset
    int a, b;
    part_range(c->act_slots, part, n_parts, a, b);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(c, mrtx_launch_pack(c->accum, c->hits, dev_dst, c->cfg.width, c->cfg.height, c->cfg.tile_w, c->cfg.tile_h,
                               c->tiles_x, c->n_tiles, c->cfg.rank, c->cfg.world, a, b - a, layout_list(c, c->cfg.rank),
                               c->tile_shift, c->gather_hits ? 1 : 0, st));
    const uint64_t slot_bytes = (uint64_t)c->cfg.tile_w * c->cfg.tile_h * (c->gather_hits ? 32ull : 16ull);
    if (byte_off) *byte_off = (uint64_t)a * slot_bytes;
    if (byte_len) *byte_len = (uint64_t)(b - a) * slot_bytes;
    if (!hip_stream) HIPCHK(c, hipStreamSynchronize(st));
    return MRTX_OK;
}
// How many parts the exchange may use for the scene as it stands (1 when the full layout is in force), and which
// render part produces the tiles of shard part k: shard parts cut the COMMON slot range, render parts must cover them.
int mrtx_shard_parts(mrtx_ctx* c, int32_t wanted, int32_t* out) {
    if (!c || !out || wanted < 1) return MRTX_E_INVALID;
    const int rc = gather_layout(c);
    if (rc != MRTX_OK) return rc;
    *out = (c->act_on && c->act_slots >= wanted) ? wanted : 1;
    return MRTX_OK;
}
int mrtx_unpack_shard(mrtx_ctx* c, int32_t src_rank, const void* dev_src, void* hip_stream) {
    if (!c || !dev_src || src_rank < 0 || src_rank >= c->cfg.world) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = gather_layout(c);
    if (rc == MRTX_OK) rc = upload_layout(c);
    if (rc == MRTX_OK) rc = clear_stale_peer_tiles(c);
    if (rc != MRTX_OK) return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (hip_stream) HIPCHK(c, hipStreamSynchronize(c->stream));   // the stale-tile clear ran on the context's stream
    HIPCHK(c, mrtx_launch_unpack(c->accum, c->hits, dev_src, c->cfg.width, c->cfg.height, c->cfg.tile_w,
                                 c->cfg.tile_h, c->tiles_x, c->n_tiles, src_rank, c->cfg.world, c->act_slots,
                                 layout_list(c, src_rank), c->tile_shift, c->gather_hits ? 1 : 0, st));
    mark_peer_written(c, src_rank);
    if (!hip_stream) HIPCHK(c, hipStreamSynchronize(st));
    return MRTX_OK;
}

int mrtx_unpack_all(mrtx_ctx* c, const void* const* dev_srcs, int32_t n) {
    if (!c || !dev_srcs || n != c->cfg.world) return MRTX_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = gather_layout(c);
    if (rc == MRTX_OK) rc = upload_layout(c);
    if (rc == MRTX_OK) rc = clear_stale_peer_tiles(c);
    if (rc != MRTX_OK) return rc;
    for (int r = 0; r < n; r++)
        if (r != c->cfg.rank && !dev_srcs[r]) return fail(c, MRTX_E_INVALID, "missing shard of rank %d", r);
    if (n <= 16) {      // one launch for all peers (pointers by value in the kernel arguments)
        HIPCHK(c, mrtx_launch_unpack_all(c->accum, c->hits, dev_srcs, c->cfg.width, c->cfg.height, c->cfg.tile_w, c->cfg.tile_h,
                                         c->tiles_x, c->n_tiles, c->cfg.rank, c->cfg.world, c->act_slots,
                                         c->act_on ? c->act_dev : nullptr, c->tile_shift, c->gather_hits ? 1 : 0, c->stream));
        for (int r = 0; r < n; r++)
            if (r != c->cfg.rank) mark_peer_written(c, r);
    } else {
        for (int r = 0; r < n; r++) {
            if (r == c->cfg.rank) continue;
            HIPCHK(c, mrtx_launch_unpack(c->accum, c->hits, dev_srcs[r], c->cfg.width, c->cfg.height, c->cfg.tile_w,
                                         c->cfg.tile_h, c->tiles_x, c->n_tiles, r, c->cfg.world, c->act_slots,
                                         layout_list(c, r), c->tile_shift, c->gather_hits ? 1 : 0, c->stream));
            mark_peer_written(c, r);
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MRTX_OK;
}

int mrtx_device_ptr(mrtx_ctx* c, int32_t which, void** out, uint64_t* bytes) {
    if (!c || !out) return MRTX_E_INVALID;
    const uint64_t fb = (uint64_t)c->cfg.width * c->cfg.height * 16;
    switch (which) {
        case MRTX_BUF_ACCUM: *out = c->accum; if (bytes) *bytes = fb; break;
        case MRTX_BUF_HITS: *out = c->hits; if (bytes) *bytes = fb; break;
        case MRTX_BUF_DEM: *out = c->dem; if (bytes) *bytes = c->dem ? (uint64_t)(c->dem_h + 4) * (c->dem_w + 4) * MRTX_DEM_ELEM_BYTES : 0; break;
        case MRTX_BUF_COLOR: *out = c->color; if (bytes) *bytes = c->color ? ((uint64_t)(c->color_h + 1) * (c->color_w + 4) + 1) * 8 : 0; break;
        // the march's skip structures (ensure_mip): null until the first marching call has built them for the step in force
        case MRTX_BUF_MIP: *out = c->mip; if (bytes) *bytes = c->mip ? (uint64_t)(c->mip_h + 2) * (c->mip_w + 2) * 8 : 0; break;   // without the slack element
        case MRTX_BUF_MIP2: *out = c->mip2; if (bytes) *bytes = c->mip2 ? (uint64_t)(c->m2_h + 2) * (c->m2_w + 2) * 4 : 0; break;
        case MRTX_BUF_HMIP: *out = c->hmip; if (bytes) *bytes = c->hmip ? (uint64_t)c->hm_h * c->hm_w * 4 : 0; break;
        default: return fail(c, MRTX_E_INVALID, "unknown buffer id %d", which);
    }
    return MRTX_OK;
}

int mrtx_mip_info(mrtx_ctx* c, int32_t out[9]) {
    if (!c || !out) return MRTX_E_INVALID;
    for (int i = 0; i < 9; i++) out[i] = 0;
    if (!c->mip) return MRTX_OK;      // nothing built (yet, or since the last DEM upload)
    out[0] = c->mip_shift; out[1] = c->mip_h; out[2] = c->mip_w;
    if (c->mip2) { out[3] = c->m2_shift; out[4] = c->m2_h; out[5] = c->m2_w; }
    if (c->hmip) { out[6] = c->hm_shift; out[7] = c->hm_h; out[8] = c->hm_w; }
    return MRTX_OK;
}

// ---- context-free helpers ---------------------------------------------------------------------
static int efail(char* err, int32_t n, const char* what, hipError_t e) {
    if (err && n > 0) snprintf(err, (size_t)n, "%s: %s", what, hipGetErrorString(e));
    return MRTX_E_DEVICE;
}
#define HIPCHK2(call)                                       \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return efail(err, err_len, #call, e_); \
    } while (0)

int mrtx_dem_from_ldem(int32_t device, const void* src, int32_t h, int32_t w, int32_t d, void* dst,
                       float* radius_scale, char* err, int32_t err_len) {
    if (!src || !dst || h < 1 || w < 1 || d < 1 || d > 64) return MRTX_E_INVALID;
    HIPCHK2(hipSetDevice(device));
    unsigned int* mb = nullptr;
    HIPCHK2(hipMalloc((void**)&mb, sizeof(unsigned int)));
    HIPCHK2(hipMemset(mb, 0, sizeof(unsigned int)));
    hipError_t e = mrtx_launch_ldem((const int16_t*)src, (float*)dst, h, w, d, mb, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned int bits = 0;
    if (e == hipSuccess) e = hipMemcpy(&bits, mb, sizeof bits, hipMemcpyDeviceToHost);
    (void)hipFree(mb);
    if (e != hipSuccess) return efail(err, err_len, "ldem kernels", e);
    if (radius_scale) std::memcpy(radius_scale, &bits, sizeof(float));
    return MRTX_OK;
}
int mrtx_synth_ldem(int32_t device, void* dst, int32_t h, int32_t w, uint32_t seed, char* err, int32_t err_len) {
    if (!dst || h < 1 || w < 1) return MRTX_E_INVALID;
    HIPCHK2(hipSetDevice(device));
    HIPCHK2(mrtx_launch_synth_ldem((int16_t*)dst, h, w, seed, nullptr));
    HIPCHK2(hipDeviceSynchronize());
    return MRTX_OK;
}
int mrtx_synth_color(int32_t device, void* dst, int32_t h, int32_t w, uint32_t seed, char* err, int32_t err_len) {
    if (!dst || h < 1 || w < 1) return MRTX_E_INVALID;
    HIPCHK2(hipSetDevice(device));
    HIPCHK2(mrtx_launch_synth_color((uint32_t*)dst, h, w, seed, nullptr));
    HIPCHK2(hipDeviceSynchronize());
    return MRTX_OK;
}
int mrtx_dev_alloc(int32_t device, uint64_t bytes, void** out) {
    if (!out || bytes == 0) return MRTX_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MRTX_E_DEVICE;
    return hipMalloc(out, (size_t)bytes) == hipSuccess ? MRTX_OK : MRTX_E_NOMEM;
}
int mrtx_dev_free(int32_t device, void* p) {
    if (hipSetDevice(device) != hipSuccess) return MRTX_E_DEVICE;
    return hipFree(p) == hipSuccess ? MRTX_OK : MRTX_E_DEVICE;
}
int mrtx_dev_download(int32_t device, void* host_dst, const void* dev_src, uint64_t bytes) {
    if (!host_dst || !dev_src) return MRTX_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MRTX_E_DEVICE;
    return hipMemcpy(host_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess ? MRTX_OK : MRTX_E_DEVICE;
}
int mrtx_dev_upload(int32_t device, void* dev_dst, const void* host_src, uint64_t bytes) {
    if (!dev_dst || !host_src) return MRTX_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MRTX_E_DEVICE;
    return hipMemcpy(dev_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice) == hipSuccess ? MRTX_OK : MRTX_E_DEVICE;
}
int mrtx_probe_stream(int32_t device, uint64_t bytes, int32_t repeats) {
    if (bytes < 1024 || repeats < 1) return MRTX_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MRTX_E_DEVICE;
    void* buf = nullptr; float* out = nullptr;
    int rc = MRTX_OK;
    if (hipMalloc(&buf, (size_t)bytes) != hipSuccess || hipMalloc((void**)&out, 4) != hipSuccess) rc = MRTX_E_NOMEM;
    if (rc == MRTX_OK && hipMemset(buf, 1, (size_t)bytes) != hipSuccess) rc = MRTX_E_DEVICE;
    for (int i = 0; i < repeats && rc == MRTX_OK; i++)
        if (mrtx_launch_probe_stream(buf, (int64_t)(bytes / 8), out, nullptr) != hipSuccess) rc = MRTX_E_DEVICE;
    if (rc == MRTX_OK && hipDeviceSynchronize() != hipSuccess) rc = MRTX_E_DEVICE;
    if (buf) (void)hipFree(buf);
    if (out) (void)hipFree(out);
    return rc;
}
int mrtx_probe_cr(int32_t device, int32_t which, uint32_t lo_bits, uint64_t n, uint64_t* mismatches, uint32_t* first_bad_bits) {
    if (which < 0 || which > 2 || n == 0 || !mismatches) return MRTX_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MRTX_E_DEVICE;
    unsigned long long* d = nullptr;
    unsigned long long h[2] = {0ull, ~0ull};
    int rc = MRTX_OK;
    if (hipMalloc((void**)&d, sizeof h) != hipSuccess) return MRTX_E_NOMEM;
    if (hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess ||
        mrtx_launch_probe_cr(lo_bits, n, which, d, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess)
        rc = MRTX_E_DEVICE;
    (void)hipFree(d);
    *mismatches = h[0];
    if (first_bad_bits) *first_bad_bits = h[1] == ~0ull ? 0u : (uint32_t)(h[1] - 1ull);
    return rc;
}
int mrtx_probe_latlon(int32_t device, const float* a, const float* b, const float* c, float* lat, float* lon,
                      int32_t n) {
    if (!a || !b || !c || !lat || !lon || n < 1) return MRTX_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return MRTX_E_DEVICE;
    float* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const float* in[3] = {a, b, c};
    const size_t bytes = (size_t)n * sizeof(float);
    int rc = MRTX_OK;
    for (int i = 0; i < 5 && rc == MRTX_OK; i++)
        if (hipMalloc((void**)&d[i], bytes) != hipSuccess) rc = MRTX_E_NOMEM;
    for (int i = 0; i < 3 && rc == MRTX_OK; i++)
        if (hipMemcpy(d[i], in[i], bytes, hipMemcpyHostToDevice) != hipSuccess) rc = MRTX_E_DEVICE;
    if (rc == MRTX_OK && (mrtx_launch_probe_latlon(d[0], d[1], d[2], d[3], d[4], n, nullptr) != hipSuccess ||
                          hipMemcpy(lat, d[3], bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                          hipMemcpy(lon, d[4], bytes, hipMemcpyDeviceToHost) != hipSuccess))
        rc = MRTX_E_DEVICE;
    for (int i = 0; i < 5; i++)
        if (d[i]) (void)hipFree(d[i]);
    return rc;
}

}  // extern "C"
