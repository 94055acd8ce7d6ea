// mrtx_terrain_api.hip -- host side of the terrain calls of libmoonrt.so.  First the queries that march
// the DEM or read horizons at points and maps of the Moon: mrtx_illum_*, mrtx_horizon_*, mrtx_occultation, mrtx_power_budget,
// mrtx_sight_*, mrtx_thermal*, mrtx_view_* and mrtx_scatter_flux.  Then the calls that work on a window of the DEM's texel
// lattice: mrtx_traverse* and mrtx_relief*.  Their kernels lie in mrtx_terrain.hip, mrtx_traverse.hip and mrtx_relief.hip; the
// context, the scene's frame and the staging, launch and read-back path are mrtx_api.hip's (mrtx_host.h).  No device code.
//
// A query reads: its own checks, its own tables, stage_query, its launch-block fields, stage_start / launch / stage_finish.  The
// checks are calls of the small functions below, inline and in the order in which the call refuses: an argument set with two
// defects is refused for the first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "mrtx_host.h"
#include "mrtx_pairs.h"

using namespace mrtx_host;

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

namespace {

// ---- The vocabulary of the queries' argument checks: each returns MRTX_OK or the code of fail() with its text.  one_of and
// at_most_one are mrtx_host.h's.  A call whose text differs by a word keeps its own (DESIGN.md section 4.35 lists them) -----------
int count_ok(mrtx_ctx* c, int32_t n) {
    if (n < 1) return fail(c, MRTX_E_INVALID, "n must be >= 1 (got %d)", n);
    return MRTX_OK;
}

// n points over m epochs: the kernels' runs, indices and sums over the epochs are float counts, exact up to 2^24
int counts_ok(mrtx_ctx* c, int32_t n, int32_t m) {
    if (n < 1 || m < 1) return fail(c, MRTX_E_INVALID, "n and m must be >= 1 (got %d, %d)", n, m);
    if (m > (1 << 24)) return fail(c, MRTX_E_INVALID, "at most 2^24 epochs per call (got %d)", m);
    return MRTX_OK;
}

int az_ok(mrtx_ctx* c, int32_t n_az) {
    if (n_az < 4 || n_az > 4096 || (n_az & (n_az - 1)) != 0) return fail(c, MRTX_E_INVALID, "n_az must be 4, 8, ..., 4096 (got %d)", n_az);
    return MRTX_OK;
}
int log2_of(int32_t n) { int l = 0; while ((1 << l) < n) l++; return l; }

// the mode of the calls that give every epoch or a summary per point
int mode_ok(mrtx_ctx* c, int32_t mode) {
    if (mode != 0 && mode != 1) return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL) or 1 (SUMMARY) (got %d)", mode);
    return MRTX_OK;
}

int bis_ok(mrtx_ctx* c, int32_t n_bis, int least) {
    if (n_bis < least || n_bis > 24) return fail(c, MRTX_E_INVALID, "n_bis must lie in [%d, 24] (got %d)", least, n_bis);
    return MRTX_OK;
}

// the 32-bit indices of an output table, and of a horizon table
int outputs_fit(mrtx_ctx* c, int64_t outputs) {
    if (outputs > (int64_t)1 << 31) return fail(c, MRTX_E_INVALID, "a call holds at most 2^31 outputs: split the points into more calls");
    return MRTX_OK;
}
int full_fits(mrtx_ctx* c, int32_t mode, int32_t n, int32_t m) {
    if (mode == 0 && (int64_t)n * (int64_t)m > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "FULL holds at most 2^31 outputs per call: split the points into more calls");
    return MRTX_OK;
}
int samples_fit(mrtx_ctx* c, int32_t n, int32_t n_az) {
    if ((int64_t)n * (int64_t)n_az > (int64_t)1 << 31) return fail(c, MRTX_E_INVALID, "at most 2^31 horizon samples per call");
    return MRTX_OK;
}

// a caller's device output (or none) that the kernel writes 8 or 16 bytes at a time
int out_aligned(mrtx_ctx* c, const void* dev_out, unsigned bytes) {
    if (reinterpret_cast<uintptr_t>(dev_out) & (bytes - 1)) return fail(c, MRTX_E_INVALID, "dev_out must be %u-byte aligned", bytes);
    return MRTX_OK;
}

// the lit shares two bodies must reach
int shares_ok(mrtx_ctx* c, double min_a, double min_b) {
    if (!(min_a > 0.0 && min_a <= 1.0) || !(min_b > 0.0 && min_b <= 1.0))
        return fail(c, MRTX_E_INVALID, "min_a and min_b must lie in (0, 1]");
    if (!((float)min_a > 0.0f) || !((float)min_b > 0.0f)) return fail(c, MRTX_E_INVALID, "min_a and min_b must be positive as float32");
    return MRTX_OK;
}

int radius_ok(mrtx_ctx* c, double radius_m) {
    if (!std::isfinite(radius_m) || !(radius_m > 0.0)) return fail(c, MRTX_E_INVALID, "radius_m must be finite and > 0");
    return MRTX_OK;
}

// The mast heights of n points (metres; null: none) as the kernels' table: each (float)(height / radius_m * R), scene units
int mast_table(mrtx_ctx* c, const double* height_m, int32_t n, double radius_m, std::vector<float>& hs) {
    hs.assign((size_t)n, 0.0f);
    for (int32_t i = 0; height_m && i < n; i++) {
        const double h = height_m[i];
        if (!std::isfinite(h) || h < 0.0 || h > 1e4) return fail(c, MRTX_E_INVALID, "point %d: height must lie in [0, 1e4] m", i);
        hs[(size_t)i] = (float)(h / radius_m * c->radius);
        if (!std::isfinite(hs[(size_t)i])) return fail(c, MRTX_E_INVALID, "point %d: height / radius_m is out of range", i);
    }
    return MRTX_OK;
}

// the horizon table of a launch: where the host's copy was staged, or else where the caller put it on the device
const float* horizon_at(const float* host, const float* staged, const void* dev) { return host ? staged : static_cast<const float*>(dev); }

bool counting(const mrtx_ctx* c) { return (c->prm.flags & MRTX_F_COUNT_STATS) != 0; }

}  // namespace

extern "C" {

// ---- Sun illumination of the terrain ------------------------------------------------------------
static bool illum_n_ok(int32_t n) { return n >= 1 && n <= 64 && (n & (n - 1)) == 0; }
static int sun_ok(mrtx_ctx* c, int32_t n_sun) {
    if (!illum_n_ok(n_sun)) return fail(c, MRTX_E_INVALID, "n_sun must be 1, 2, 4, ..., 64 (got %d)", n_sun);
    return MRTX_OK;
}

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
    if constexpr (std::is_same<G, MrtxIllumGrid>::value) CHK(sun_ok(c, g->n_sun));
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
    if (march && !(c->prm.flags & MRTX_F_NO_SKIP)) CHK(ensure_mip(c));
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

// What a query does between its last check and its launch block.  The frame comes first: it holds the state's refusal.  Then the
// output, and only then the tables (mrtx_host.h: every buffer is grown before the first copy is queued); rtab and ctab are the
// first two of them, the rest is the call's own, at s.d[2] onwards.  The launch block q is zeroed, and its grid g gets the two
// tables and rows x cols nodes: a point list of n points is n, n, true.
struct QueryStage {
    FrameC f;
    FrameCold cold;
    float* d[10];       // (the most a call stages is 9 tables)
};
extern "C++" template <class Q>
static int stage_query(mrtx_ctx* c, QueryStage& s, bool march, int rows, int cols, bool points, void*& dev_out, size_t out_bytes,
                       std::initializer_list<HostSeg> tables, Q& q, IllumC& g) {
    CHK(stage_frame(c, s.f, s.cold, march));
    CHK(stage_out(c, dev_out, out_bytes));
    CHK(stage_tables(c, tables, s.d));
    std::memset(&q, 0, sizeof q);
    g.rtab = s.d[0]; g.ctab = s.d[1];
    g.rows = rows; g.cols = cols; g.points = points ? 1 : 0;
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
    CHK(stage_frame(c, f, cold, true, !lights));
    const bool stats = counting(c);
    float sun[128];
    mrtx_illum_sun_samples(n_sun, sun);
    const size_t out_bytes = (size_t)rows * (size_t)cols * 16;
    float* d[5];
    CHK(stage_out(c, dev_out, out_bytes));
    CHK(stage_tables(c, {{sun, 2 * (size_t)n_sun}, rtab, ctab, {lights ? lights->data() : nullptr, lights ? lights->size() : 0},
                         {first, first ? (size_t)rows : 0}}, d));
    IllumC g;
    std::memset(&g, 0, sizeof g);
    g.sun = d[0]; g.rtab = d[1]; g.ctab = d[2];
    g.out = (float*)dev_out; g.rows = rows; g.cols = cols; g.points = points ? 1 : 0; g.n_sun = n_sun;
    CHK(stage_start(c, &cold, stats));
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
    CHK(grid_tables(c, g, rtab, ctab));
    if (!dev_out && !host_out) return fail(c, MRTX_E_INVALID, "no output buffer");
    return illum_run(c, rtab, ctab, g->row_end - g->row_begin, g->w, false, g->n_sun, dev_out, host_out, out);
}

int mrtx_illum_points(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_sun, float* host_out4, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    CHK(count_ok(c, n));
    if (!latlon || !host_out4) return fail(c, MRTX_E_INVALID, "null point list or output");
    CHK(sun_ok(c, n_sun));
    std::vector<float> rtab, ctab;
    CHK(point_tables(c, latlon, n, rtab, ctab));
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
    CHK(sun_ok(c, n_sun));
    if ((int64_t)n_points * (int64_t)count > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a series holds at most 2^31 outputs: split the points into more calls");
    for (int32_t p = 0; p < n_points; p++) {
        const int64_t f0 = first ? (int64_t)first[p] : 0;
        if (f0 < 0 || f0 + count > n_epochs)
            return fail(c, MRTX_E_INVALID, "point %d: window [%lld, %lld) runs outside the %d epochs", p, (long long)f0,
                        (long long)(f0 + count), n_epochs);
    }
    std::vector<float> rtab, ctab, lights;
    CHK(point_tables(c, latlon, n_points, rtab, ctab));
    CHK(epoch_lights(c, ep, n_epochs, lights));
    return illum_run(c, rtab, ctab, n_points, count, true, n_sun, dev_out, host_out, out, &lights, first);
}

// ---- Terrain horizons and the Sun against them (DESIGN.md sections 3.8 and 3.9) --------------------------------------------
// the horizon and output arguments of the calls that read horizons: where each lives, and the horizons' size
static int horizon_args(mrtx_ctx* c, const void* dev_horizon, const float* host_horizon, int32_t n, int32_t n_az,
                        const void* dev_out, const void* host_out) {
    CHK(one_of(c, dev_horizon, host_horizon, "horizon"));
    CHK(one_of(c, dev_out, host_out, "out"));
    return samples_fit(c, n, n_az);
}

// every entry of a host horizon table an elevation in [-90, 90] degrees (a device table is not scanned)
static int horizon_entries(mrtx_ctx* c, const float* host_horizon, int32_t n, int32_t n_az) {
    const size_t nh = host_horizon ? (size_t)n * (size_t)n_az : 0;
    for (size_t i = 0; i < nh; i++)
        if (!(host_horizon[i] >= -90.0f && host_horizon[i] <= 90.0f))
            return fail(c, MRTX_E_INVALID, "horizon entry %zu is not an elevation in [-90, 90] degrees", i);
    return MRTX_OK;
}

// a host horizon table as the launch's last table (a device table: an empty one); horizon_at picks the kernel's address
static HostSeg horizon_seg(const float* host_horizon, int32_t n, int32_t n_az) {
    return {host_horizon, host_horizon ? (size_t)n * (size_t)n_az : 0};
}

int mrtx_horizon_points(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, int32_t n_bis, void* dev_out, float* host_out,
                        MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon) return fail(c, MRTX_E_INVALID, "null point list");
    CHK(count_ok(c, n));
    CHK(az_ok(c, n_az));
    CHK(bis_ok(c, n_bis, 1));
    CHK(outputs_fit(c, (int64_t)n * (int64_t)n_az));
    CHK(one_of(c, dev_out, host_out, "out"));
    std::vector<float> rtab, ctab;
    CHK(point_tables(c, latlon, n, rtab, ctab));
    const bool stats = counting(c);
    const size_t out_bytes = (size_t)n * (size_t)n_az * sizeof(float);
    QueryStage s;
    HorizonC h;
    CHK(stage_query(c, s, true, n, n, true, dev_out, out_bytes, {rtab, ctab}, h, h.g));
    h.out = (float*)dev_out; h.az_log2 = log2_of(n_az); h.n_bis = n_bis;
    CHK(stage_start(c, &s.cold, stats));
    HIPCHK(c, mrtx_launch_horizon(s.f, h, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_horizon_sun(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon, const float* host_horizon,
                     const MrtxIllumEpoch* epochs, int32_t m, int32_t mode, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    CHK(counts_ok(c, n, m));
    CHK(az_ok(c, n_az));
    CHK(mode_ok(c, mode));
    CHK(horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, host_out));
    CHK(full_fits(c, mode, n, m));
    CHK(horizon_entries(c, host_horizon, n, n_az));
    std::vector<float> rtab, ctab, lights;
    CHK(point_tables(c, latlon, n, rtab, ctab));
    CHK(epoch_lights(c, epochs, m, lights));
    const size_t out_bytes = mode == 0 ? (size_t)n * (size_t)m * sizeof(float) : (size_t)n * 16;
    QueryStage s;
    HorizonSunC q;
    CHK(stage_query(c, s, false, n, n, true, dev_out, out_bytes, {rtab, ctab, lights, horizon_seg(host_horizon, n, n_az)}, q, q.g));
    q.lights = s.d[2];
    q.horizon = horizon_at(host_horizon, s.d[3], dev_horizon);
    q.out = (float*)dev_out; q.az_log2 = log2_of(n_az); q.m = m; q.mode = mode;
    CHK(stage_start(c, &s.cold, false));
    HIPCHK(c, mrtx_launch_horizon_sun(s.f, q, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays);
}

// ---- Mast-height horizons and joint windows --------------------------------------------------------
int mrtx_horizon_raised(mrtx_ctx* c, const double* latlon, const double* height_m, double radius_m, int32_t n, int32_t n_az,
                        int32_t n_bis, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !height_m) return fail(c, MRTX_E_INVALID, "null point list or height list");
    CHK(count_ok(c, n));
    CHK(az_ok(c, n_az));
    CHK(bis_ok(c, n_bis, 1));
    CHK(radius_ok(c, radius_m));
    CHK(outputs_fit(c, (int64_t)n * (int64_t)n_az));
    CHK(one_of(c, dev_out, host_out, "out"));
    std::vector<float> hs, rtab, ctab;
    CHK(mast_table(c, height_m, n, radius_m, hs));
    CHK(point_tables(c, latlon, n, rtab, ctab));
    const bool stats = counting(c);
    const size_t out_bytes = (size_t)n * (size_t)n_az * sizeof(float);
    QueryStage s;
    HorizonRaisedC q;
    CHK(stage_query(c, s, true, n, n, true, dev_out, out_bytes, {rtab, ctab, hs}, q, q.h.g));
    q.h.out = (float*)dev_out; q.h.az_log2 = log2_of(n_az); q.h.n_bis = n_bis;
    q.hs = s.d[2];
    CHK(stage_start(c, &s.cold, stats));
    HIPCHK(c, mrtx_launch_horizon_raised(s.f, q, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_horizon_windows(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                         const float* host_horizon, const MrtxIllumEpoch* epochs_a, const MrtxIllumEpoch* epochs_b, int32_t m,
                         double min_a, double min_b, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs_a || !epochs_b) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    CHK(counts_ok(c, n, m));
    CHK(az_ok(c, n_az));
    CHK(shares_ok(c, min_a, min_b));
    CHK(horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, host_out));
    CHK(out_aligned(c, dev_out, 16));
    CHK(horizon_entries(c, host_horizon, n, n_az));
    std::vector<float> rtab, ctab, lights_a, lights_b;
    CHK(point_tables(c, latlon, n, rtab, ctab));
    CHK(epoch_lights(c, epochs_a, m, lights_a));
    CHK(epoch_lights(c, epochs_b, m, lights_b));
    const size_t out_bytes = (size_t)n * 32;
    QueryStage s;
    HorizonWindowsC q;
    CHK(stage_query(c, s, false, n, n, true, dev_out, out_bytes,
                    {rtab, ctab, lights_a, lights_b, horizon_seg(host_horizon, n, n_az)}, q, q.g));
    q.lights_a = s.d[2]; q.lights_b = s.d[3];
    q.horizon = horizon_at(host_horizon, s.d[4], dev_horizon);
    q.out = (float*)dev_out; q.min_a = (float)min_a; q.min_b = (float)min_b; q.az_log2 = log2_of(n_az); q.m = m;
    CHK(stage_start(c, &s.cold, false));
    HIPCHK(c, mrtx_launch_horizon_windows(s.f, q, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays);
}

// ---- Drive masks: mrtx_horizon_windows' predicate kept as bits -------------------------------------
int mrtx_horizon_mask(mrtx_ctx* c, const double* latlon, int32_t n, int32_t n_az, const void* dev_horizon,
                      const float* host_horizon, const MrtxIllumEpoch* epochs_a, const MrtxIllumEpoch* epochs_b, int32_t m,
                      double min_a, double min_b, void* dev_out, uint64_t* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!latlon || !epochs_a) return fail(c, MRTX_E_INVALID, "null point list or epoch table");
    CHK(counts_ok(c, n, m));
    CHK(az_ok(c, n_az));
    if (!epochs_b) min_b = 1.0;        // ignored without a second table
    CHK(shares_ok(c, min_a, min_b));
    CHK(horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, host_out));
    CHK(out_aligned(c, dev_out, 8));
    CHK(horizon_entries(c, host_horizon, n, n_az));
    std::vector<float> rtab, ctab, lights_a, lights_b;
    CHK(point_tables(c, latlon, n, rtab, ctab));
    CHK(epoch_lights(c, epochs_a, m, lights_a));
    if (epochs_b) CHK(epoch_lights(c, epochs_b, m, lights_b));
    const size_t out_bytes = (size_t)n * (size_t)((m + 63) / 64) * 8;
    QueryStage s;
    HorizonMaskC q;
    CHK(stage_query(c, s, false, n, n, true, dev_out, out_bytes,
                    {rtab, ctab, lights_a, lights_b, horizon_seg(host_horizon, n, n_az)}, q, q.g));
    q.lights_a = s.d[2]; q.lights_b = epochs_b ? s.d[3] : nullptr;
    q.horizon = horizon_at(host_horizon, s.d[4], dev_horizon);
    q.out = (unsigned long long*)dev_out; q.min_a = (float)min_a; q.min_b = (float)min_b; q.az_log2 = log2_of(n_az); q.m = m;
    CHK(stage_start(c, &s.cold, false));
    HIPCHK(c, mrtx_launch_horizon_mask(s.f, q, c->stream));
    return stage_finish(c, dev_out, reinterpret_cast<float*>(host_out), out_bytes, out, kNoRays);
}

// ---- Joint availability of mask rows: pairs of horizon_mask's rows, reduced on the device -------------
static_assert(sizeof(MrtxMaskPairs) == 48 && sizeof(PairRec) == 16 && sizeof(PairCell) == 8 && sizeof(PairBox) == 24 &&
              sizeof(PairPick) == 16, "the pair blocks");

// a host position table is refused at its first bad coordinate (a device table's are counted by the box kernel)
static int pair_positions_ok(mrtx_ctx* c, const int32_t* host_pos, size_t n, const char* name) {
    for (size_t k = 0; host_pos && k < 3 * n; k++)
        if (host_pos[k] < -MRTX_PAIRS_CMAX || host_pos[k] > MRTX_PAIRS_CMAX)
            return fail(c, MRTX_E_INVALID, "coordinate %zu of row %zu of %s must lie in -2^29 .. 2^29 (got %d)", k % 3, k / 3, name,
                        host_pos[k]);
    return MRTX_OK;
}

int mrtx_mask_pairs(mrtx_ctx* c, const MrtxMaskPairs* p, const void* dev_a, const uint64_t* host_a, const void* dev_b,
                    const uint64_t* host_b, const void* dev_base, const uint64_t* host_base, const void* dev_pos_a,
                    const int32_t* host_pos_a, const void* dev_pos_b, const int32_t* host_pos_b, void* dev_out, void* host_out,
                    uint64_t* pairs, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!p) return fail(c, MRTX_E_INVALID, "null pairs block");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    if (p->m < 1 || p->m > (1 << 24)) return fail(c, MRTX_E_INVALID, "m must lie in 1 .. 2^24 (got %d)", p->m);
    if (p->n_a < 1 || p->n_a > (1 << 24)) return fail(c, MRTX_E_INVALID, "n_a must lie in 1 .. 2^24 (got %d)", p->n_a);
    if (p->n_b < 0 || p->n_b > (1 << 24)) return fail(c, MRTX_E_INVALID, "n_b must lie in 0 .. 2^24 (got %d)", p->n_b);
    if (p->mode != MRTX_PAIRS_ROWS && p->mode != MRTX_PAIRS_BEST && p->mode != MRTX_PAIRS_TABLE)
        return fail(c, MRTX_E_INVALID, "mode must be MRTX_PAIRS_ROWS, MRTX_PAIRS_BEST or MRTX_PAIRS_TABLE (got %d)", p->mode);
    const bool rows = p->mode == MRTX_PAIRS_ROWS, best = p->mode == MRTX_PAIRS_BEST;
    if (!rows && p->op != MRTX_PAIRS_ANY && p->op != MRTX_PAIRS_BOTH)
        return fail(c, MRTX_E_INVALID, "op must be MRTX_PAIRS_ANY or MRTX_PAIRS_BOTH (got %d)", p->op);
    if (best && p->rank != MRTX_PAIRS_BY_COUNT && p->rank != MRTX_PAIRS_BY_GAP)
        return fail(c, MRTX_E_INVALID, "rank must be MRTX_PAIRS_BY_COUNT or MRTX_PAIRS_BY_GAP (got %d)", p->rank);
    CHK(one_of(c, dev_a, host_a, "a"));
    CHK(at_most_one(c, dev_b, host_b, "b"));
    CHK(at_most_one(c, dev_base, host_base, "base"));
    CHK(at_most_one(c, dev_pos_a, host_pos_a, "pos_a"));
    CHK(at_most_one(c, dev_pos_b, host_pos_b, "pos_b"));
    CHK(one_of(c, dev_out, host_out, "out"));
    const bool has_b = dev_b || host_b, has_pa = dev_pos_a || host_pos_a, has_pb = dev_pos_b || host_pos_b;
    if (has_b != (p->n_b > 0)) return fail(c, MRTX_E_INVALID, "give a B table iff n_b > 0 (n_b == 0: B is A itself)");
    if (rows && (has_b || has_pa || has_pb)) return fail(c, MRTX_E_INVALID, "MRTX_PAIRS_ROWS takes no B table and no positions");
    if (has_pb != (has_pa && has_b)) return fail(c, MRTX_E_INVALID, "give pos_b iff pos_a is given and B is not A");
    const int32_t w64 = (p->m + 63) / 64, n_b = has_b ? p->n_b : p->n_a;
    if ((int64_t)p->n_a * w64 >= (int64_t)1 << 31 || (int64_t)n_b * w64 >= (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a table holds fewer than 2^31 words (got %d and %d rows of %d)", p->n_a, n_b, w64);
    if (p->mode == MRTX_PAIRS_TABLE && (int64_t)p->n_a * n_b > (int64_t)1 << 28)
        return fail(c, MRTX_E_INVALID, "MRTX_PAIRS_TABLE holds at most 2^28 pairs (got %d x %d)", p->n_a, n_b);
    CHK(aligned(c, dev_a, 8, "dev_a", "uint64"));
    CHK(aligned(c, dev_b, 8, "dev_b", "uint64"));
    CHK(aligned(c, dev_base, 8, "dev_base", "uint64"));
    CHK(aligned(c, dev_pos_a, 4, "dev_pos_a", "int32"));
    CHK(aligned(c, dev_pos_b, 4, "dev_pos_b", "int32"));
    CHK(aligned(c, dev_out, 8, "dev_out", "records"));
    const size_t a_words = (size_t)p->n_a * (size_t)w64, b_words = has_b ? (size_t)n_b * (size_t)w64 : 0;
    const size_t out_bytes = p->mode == MRTX_PAIRS_TABLE ? sizeof(PairCell) * (size_t)p->n_a * (size_t)n_b : sizeof(PairRec) * (size_t)p->n_a;
    if (spans_overlap(dev_out, out_bytes, dev_a, 8 * a_words) || spans_overlap(dev_out, out_bytes, dev_b, 8 * b_words) ||
        spans_overlap(dev_out, out_bytes, dev_base, 8 * (size_t)w64) || spans_overlap(dev_out, out_bytes, dev_pos_a, 12 * (size_t)p->n_a) ||
        spans_overlap(dev_out, out_bytes, dev_pos_b, 12 * (size_t)n_b))
        return fail(c, MRTX_E_INVALID, "dev_out must not overlap a device input");
    // MOONRT_PAIRS=brute: every tile pair is looked at, the yardstick of the pruned walk; the same bytes and the same pairs
    bool prune = true;
    CHK(variant(c, "MOONRT_PAIRS", "prune", "brute", &prune));
    CHK(pair_positions_ok(c, host_pos_a, (size_t)p->n_a, "pos_a"));
    CHK(pair_positions_ok(c, host_pos_b, (size_t)n_b, "pos_b"));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const PairsLayout at = pairs_layout(p->n_a, n_b, !rows, best, has_pa);
    float* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    CHK(stage_out(c, dev_out, out_bytes));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, at.end));
    CHK(stage_tables(c, {{host_a, host_a ? 2 * a_words : 0}, {host_b, host_b ? 2 * b_words : 0},
                         {host_base, host_base ? 2 * (size_t)w64 : 0}, {host_pos_a, host_pos_a ? 3 * (size_t)p->n_a : 0},
                         {host_pos_b, host_pos_b ? 3 * (size_t)n_b : 0}}, d));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    PairsC q;
    std::memset(&q, 0, sizeof q);
    q.a = static_cast<const unsigned long long*>(host_a ? d[0] : dev_a);
    q.b = has_b ? static_cast<const unsigned long long*>(host_b ? d[1] : dev_b) : q.a;
    q.base = static_cast<const unsigned long long*>(host_base ? d[2] : dev_base);
    q.pos_a = static_cast<const int32_t*>(host_pos_a ? d[3] : dev_pos_a);
    q.pos_b = has_b ? static_cast<const int32_t*>(host_pos_b ? d[4] : dev_pos_b) : q.pos_a;
    q.out = dev_out;
    q.part = reinterpret_cast<PairPick*>(tb + at.part_at);
    q.box_a = reinterpret_cast<PairBox*>(tb + at.box_a_at);
    q.box_b = reinterpret_cast<PairBox*>(tb + at.box_b_at);
    q.pairs = reinterpret_cast<unsigned long long*>(tb);
    q.bad = reinterpret_cast<uint32_t*>(tb + 8);
    q.d2_min = has_pa ? p->d2_min : 0; q.d2_max = has_pa ? p->d2_max : ~0ull;
    q.n_a = p->n_a; q.n_b = n_b; q.m = p->m; q.w64 = w64;
    q.op_and = !rows && p->op == MRTX_PAIRS_BOTH; q.mode = p->mode; q.by_gap = best && p->rank == MRTX_PAIRS_BY_GAP; q.self = !has_b;
    q.splits = at.splits;
    uint32_t launches = 0;
    unsigned long long head[2] = {0, 0};                    // pairs, bad
    HIPCHK(c, hipMemsetAsync(tb, 0, 32, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_mask_pairs(q, prune, c->stream, &launches));
    CHK(stage_finish(c, nullptr, nullptr, 0, out, kNoRays));
    if (out) out->launches = launches;
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    if ((uint32_t)head[1])
        return fail(c, MRTX_E_INVALID, "%u coordinates of the device position tables lie outside -2^29 .. 2^29", (uint32_t)head[1]);
    if (host_out) HIPCHK(c, hipMemcpy(host_out, dev_out, out_bytes, hipMemcpyDeviceToHost));
    if (pairs) *pairs = rows ? (uint64_t)p->n_a : head[0];
    return MRTX_OK;
}

// ---- The Earth's occultation of the Sun ------------------------------------------------------------
// The two epoch tables of mrtx_occultation and mrtx_thermal_occulted: epoch_lights' checks and constants for both, the
// geometry the two-disc rule stands on, and per epoch the float64 mark "some point inside the bounding sphere may see the
// discs overlap".  With Rb the bounding sphere (the Moon's radius and the vertex lift, plus a thousandth), d the centre
// distances and r the radii: the centre's separation, less both bodies' largest parallax asin(Rb / d), against the sum of the
// largest angular radii asin(r / (d - Rb)) widened by 1 % and 1e-4 rad -- a hundred times what float32 directions can move.
static int occult_tables(mrtx_ctx* c, const MrtxIllumEpoch* src, const MrtxIllumEpoch* body, int32_t m, std::vector<float>& ls,
                         std::vector<float>& lb, std::vector<float>& marks) {
    CHK(epoch_lights(c, src, m, ls));
    CHK(epoch_lights(c, body, m, lb));
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
    CHK(counts_ok(c, n, m));
    CHK(mode_ok(c, mode));
    CHK(one_of(c, dev_out, host_out, "out"));
    if (mode == 1) CHK(out_aligned(c, dev_out, 16));
    CHK(full_fits(c, mode, n, m));
    // the state's refusal before the tables: theirs are measured against the Moon the context holds
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    std::vector<float> rtab, ctab, ls, lb, marks;
    CHK(point_tables(c, latlon, n, rtab, ctab));
    CHK(occult_tables(c, epochs_source, epochs_body, m, ls, lb, marks));
    const size_t out_bytes = mode == 0 ? (size_t)n * (size_t)m * sizeof(float) : (size_t)n * 32;
    QueryStage s;
    OccultC q;
    CHK(stage_query(c, s, false, n, n, true, dev_out, out_bytes, {rtab, ctab, ls, lb, marks}, q, q.g));
    q.src = s.d[2]; q.body = s.d[3]; q.mark = reinterpret_cast<const int32_t*>(s.d[4]);
    q.out = (float*)dev_out; q.m = m; q.mode = mode;
    CHK(stage_start(c, &s.cold, false));
    HIPCHK(c, mrtx_launch_occultation(s.f, q, c->stream));
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
    CHK(count_ok(c, n));
    if (k->n_sat < 1 || k->n_sat > 256) return fail(c, MRTX_E_INVALID, "n_sat must lie in [1, 256] (got %d)", k->n_sat);
    // the runs, the indices and the sum of c_k are float counts, exact up to 2^24
    if (k->m < 1 || k->m > (1 << 24) || (int64_t)k->n_sat * (int64_t)k->m > (int64_t)1 << 24)
        return fail(c, MRTX_E_INVALID, "m must be >= 1 and n_sat * m at most 2^24 (got %d x %d)", k->n_sat, k->m);
    CHK(az_ok(c, n_az));
    CHK(radius_ok(c, k->radius_m));
    if (!(k->min_elev_deg >= -90.0 && k->min_elev_deg < 90.0)) return fail(c, MRTX_E_INVALID, "min_elev_deg must lie in [-90, 90)");
    const bool list = k->mode == MRTX_PASSES_LIST;
    const int S = k->n_sat, m = k->m;
    CHK(one_of(c, dev_horizon, host_horizon, "horizon"));
    CHK(samples_fit(c, n, n_az));
    CHK(at_most_one(c, dev_out, host_out, "out"));
    const bool has_out = dev_out || host_out;
    if (!list) CHK(one_of(c, dev_out, host_out, "out"));
    if (list && !n_passes) return fail(c, MRTX_E_INVALID, "null n_passes");
    if (list && !has_out && pass_cap) return fail(c, MRTX_E_INVALID, "without a table pass_cap must be 0 (got %llu)", (unsigned long long)pass_cap);
    CHK(out_aligned(c, dev_out, list ? 8 : 16));
    if (k->mode == MRTX_PASSES_FULL && (int64_t)n * S * m > (int64_t)1 << 27)
        return fail(c, MRTX_E_INVALID, "FULL holds at most 2^27 outputs per call: split the points into more calls");
    if (list && (int64_t)n * S > (int64_t)1 << 27)
        return fail(c, MRTX_E_INVALID, "LIST holds at most 2^27 (point, satellite) pairs per call: split the points into more calls");
    CHK(horizon_entries(c, host_horizon, n, n_az));
    // the state's refusal before the tables: theirs are measured against the Moon the context holds
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    std::vector<float> hs;
    CHK(mast_table(c, height_m, n, k->radius_m, hs));
    const double hs_max = *std::max_element(hs.begin(), hs.end());
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
    CHK(point_tables(c, latlon, n, rtab, ctab));
    // not stage_query: LIST has no output yet, but a work buffer to grow before the tables are copied
    FrameC f;
    FrameCold cold;
    CHK(stage_frame(c, f, cold, false));
    const size_t pairs = (size_t)n * (size_t)S;
    const size_t out_bytes = k->mode == MRTX_PASSES_FULL ? pairs * (size_t)m * 16 : (size_t)n * 32;
    float* d[5];
    if (!list) CHK(stage_out(c, dev_out, out_bytes));
    // LIST: the counts, then the prefix sums (8-byte aligned), in the work buffer
    const size_t base_at = (pairs * 4 + 15) & ~(size_t)15;
    if (list) CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, base_at + pairs * 8));
    CHK(stage_tables(c, {rtab, ctab, hs, sat, horizon_seg(host_horizon, n, n_az)}, d));
    PassesC q;
    std::memset(&q, 0, sizeof q);
    q.g.rtab = d[0]; q.g.ctab = d[1];
    q.g.rows = n; q.g.cols = n; q.g.points = 1;
    q.hs = d[2]; q.sat = d[3];
    q.horizon = horizon_at(host_horizon, d[4], dev_horizon);
    q.min_elev = (float)k->min_elev_deg; q.range_scale = (float)(k->radius_m / c->radius);
    q.az_log2 = log2_of(n_az); q.m = m; q.n_sat = S;
    if (!list) {
        q.out = dev_out;
        CHK(stage_start(c, &cold, false));
        HIPCHK(c, mrtx_launch_passes(f, q, k->mode, c->stream));
        return stage_finish(c, dev_out, static_cast<float*>(host_out), out_bytes, out, kNoRays);
    }
    char* const tb = reinterpret_cast<char*>(c->trav_buf);
    q.counts = reinterpret_cast<uint32_t*>(tb);
    q.base = reinterpret_cast<const unsigned long long*>(tb + base_at);
    CHK(stage_start(c, &cold, false));
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
            CHK(stage_buffer(c, c->illum_out, c->illum_out_bytes, list_bytes));
            dev_out = c->illum_out;
        }
        q.out = dev_out;
        HIPCHK(c, hipMemcpyAsync(tb + base_at, base.data(), pairs * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, mrtx_launch_passes(f, q, 3, c->stream));
        launches = 2;
    }
    const bool filled = launches == 2;
    CHK(stage_finish(c, dev_out, filled ? static_cast<float*>(host_out) : nullptr, list_bytes, out, kNoRays));
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
    CHK(counts_ok(c, n, m));       // 2^24 epochs of at most 2^28 counts: every sum stays within 2^52
    CHK(az_ok(c, n_az));
    CHK(mode_ok(c, mode));
    CHK(horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, host_out));
    if (mode == 1) CHK(out_aligned(c, dev_out, 16));
    CHK(full_fits(c, mode, n, m));
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
    CHK(horizon_entries(c, host_horizon, n, n_az));
    std::vector<float> rtab, ctab, lights;
    CHK(point_tables(c, latlon, n, rtab, ctab));
    CHK(epoch_lights(c, epochs, m, lights));
    const size_t out_bytes = mode == 0 ? (size_t)n * (size_t)m * sizeof(int32_t) : (size_t)n * 64;
    QueryStage s;
    PowerC q;
    CHK(stage_query(c, s, false, n, n, true, dev_out, out_bytes,
                    {rtab, ctab, lights, gen, {load.data(), load.size()}, horizon_seg(host_horizon, n, n_az)}, q, q.g));
    q.lights = s.d[2]; q.gen = s.d[3]; q.load = reinterpret_cast<const int32_t*>(s.d[4]);
    q.horizon = horizon_at(host_horizon, s.d[5], dev_horizon);
    q.out = dev_out; q.capacity = model->capacity; q.initial = model->initial; q.scale = scale;
    q.nE = nrm[0]; q.nN = nrm[1]; q.nU = nrm[2];
    q.panel = model->panel; q.az_log2 = log2_of(n_az); q.m = m; q.mode = mode;
    CHK(stage_start(c, &s.cold, false));
    HIPCHK(c, mrtx_launch_power_budget(s.f, q, c->stream));
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
    CHK(radius_ok(c, radius_m));
    CHK(bis_ok(c, n_bis, 0));
    return one_of(c, dev_out, host_out, "out");
}

// Everything after the argument checks: the targets' tables (trt, tct: rows x cols nodes, or a point list), the observers'
// tables and raised heights (scene units), one launch into the output, counters.
static int sight_run(mrtx_ctx* c, const std::vector<float>& trt, const std::vector<float>& tct, int rows, int cols, bool points,
                     const std::vector<float>& ort, const std::vector<float>& oct, const std::vector<double>& obs_h_m,
                     double target_h_m, double mast_max_m, double radius_m, int32_t n_bis, void* dev_out, float* host_out,
                     MrtxStats* out) {
    const bool stats = counting(c);
    const int n_obs = (int)obs_h_m.size();
    std::vector<float> hs((size_t)n_obs);
    for (int i = 0; i < n_obs; i++) hs[(size_t)i] = (float)(obs_h_m[(size_t)i] / radius_m * c->radius);
    const size_t out_bytes = (size_t)rows * (size_t)cols * sizeof(float);
    QueryStage s;
    SightC q;
    CHK(stage_query(c, s, true, rows, cols, points, dev_out, out_bytes, {trt, tct, ort, oct, hs}, q, q.g));
    q.obs.rtab = s.d[2]; q.obs.ctab = s.d[3];
    q.obs.rows = n_obs; q.obs.cols = n_obs; q.obs.points = 1;
    q.obs_hs = s.d[4];
    q.out = (float*)dev_out;
    q.target_h_m = target_h_m; q.mast_max_m = mast_max_m; q.radius_m = radius_m; q.R = c->radius;
    q.n_obs = n_obs; q.n_bis = n_bis;
    CHK(stage_start(c, &s.cold, stats));
    HIPCHK(c, mrtx_launch_sight(s.f, q, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kShadowRays : kNoRays);
}

int mrtx_sight_grid(mrtx_ctx* c, const MrtxSightGrid* g, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!g) return fail(c, MRTX_E_INVALID, "null grid");
    if (!sight_latlon_ok(g->obs_lat, g->obs_lon))
        return fail(c, MRTX_E_INVALID, "observer: latitude must lie in [-90, 90] and longitude be finite");
    if (!sight_height_ok(g->obs_h_m)) return fail(c, MRTX_E_INVALID, "observer height must lie in [0, 1e9] m");
    CHK(sight_check(c, g->target_h_m, g->mast_max_m, g->radius_m, g->n_bis, dev_out, host_out));
    std::vector<float> trt, tct, ort, oct;
    CHK(grid_tables(c, g, trt, tct));
    const double ll[2] = {g->obs_lat, g->obs_lon};
    CHK(point_tables(c, ll, 1, ort, oct));
    return sight_run(c, trt, tct, g->row_end - g->row_begin, g->w, false, ort, oct, std::vector<double>(1, g->obs_h_m),
                     g->target_h_m, g->mast_max_m, g->radius_m, g->n_bis, dev_out, host_out, out);
}

int mrtx_sight_points(mrtx_ctx* c, const double* target_latlon, int32_t n, const double* observer_llh, int32_t n_observers,
                      double target_h_m, double mast_max_m, double radius_m, int32_t n_bis, void* dev_out, float* host_out,
                      MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!target_latlon || !observer_llh) return fail(c, MRTX_E_INVALID, "null target or observer list");
    CHK(count_ok(c, n));
    if (n_observers != 1 && n_observers != n)
        return fail(c, MRTX_E_INVALID, "n_observers must be 1 or n (got %d for n = %d)", n_observers, n);
    CHK(sight_check(c, target_h_m, mast_max_m, radius_m, n_bis, dev_out, host_out));
    std::vector<float> trt, tct, ort, oct;
    CHK(point_tables(c, target_latlon, n, trt, tct));
    std::vector<double> oll((size_t)n_observers * 2), oh((size_t)n_observers);
    for (int32_t i = 0; i < n_observers; i++) {
        const double* o = observer_llh + 3 * (size_t)i;
        if (!sight_latlon_ok(o[0], o[1]))
            return fail(c, MRTX_E_INVALID, "observer %d: latitude must lie in [-90, 90] and longitude be finite", i);
        if (!sight_height_ok(o[2])) return fail(c, MRTX_E_INVALID, "observer %d: height must lie in [0, 1e9] m", i);
        oll[2 * (size_t)i] = o[0]; oll[2 * (size_t)i + 1] = o[1]; oh[(size_t)i] = o[2];
    }
    CHK(point_tables(c, oll.data(), n_observers, ort, oct));
    return sight_run(c, trt, tct, 1, n, true, ort, oct, oh, target_h_m, mast_max_m, radius_m, n_bis, dev_out, host_out, out);
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
    CHK(counts_ok(c, n, m));
    CHK(az_ok(c, n_az));
    if (entry == kThermal && (mode < 0 || mode > 2))
        return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL), 1 (SUMMARY) or 2 (FLUX) (got %d)", mode);
    if (entry == kThermalScatter && (mode < 0 || mode > 3))
        return fail(c, MRTX_E_INVALID, "mode must be 0 (FULL), 1 (SUMMARY), 2 (FLUX) or 3 (EXITANCE) (got %d)", mode);
    if (entry == kThermalColumn && (mode < 0 || mode > 5))
        return fail(c, MRTX_E_INVALID,
                    "mode must be 0 (FULL), 1 (SUMMARY), 2 (FLUX), 3 (EXITANCE), 4 (COLUMN) or 5 (VOLATILE) (got %d)", mode);
    if ((mode == 5) != (species != nullptr))
        return fail(c, MRTX_E_INVALID, "a species is required in mode 5 (VOLATILE) and must be null in every other mode");
    if (species) CHK(volatile_ok(c, *species));
    if (mode == 5 && ((uintptr_t)dev_out & 7))
        return fail(c, MRTX_E_INVALID, "VOLATILE writes float64 pairs: dev_out must be 8-byte aligned");
    CHK(at_most_one(c, dev_extra, host_extra, "extra"));
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
    CHK(horizon_args(c, dev_horizon, host_horizon, n, n_az, dev_out, host_out));
    const MrtxThermalModel& md = *model;
    double dmax = 0.0;
    CHK(thermal_model_ok(c, md, m, mode, &dmax));
    // outputs per point; VOLATILE's are float64
    const int64_t width = mode == 0 ? (int64_t)m - md.n_spin : mode == 2 ? (int64_t)m : mode == 3 ? 2 * ((int64_t)m - md.n_spin) :
                          mode == 4 ? ((int64_t)m - md.n_spin) * md.n_nodes : mode == 5 ? 2 * (int64_t)md.n_nodes : 4;
    CHK(outputs_fit(c, (int64_t)n * width));
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
    CHK(horizon_entries(c, host_horizon, n, n_az));
    std::vector<float> rtab, ctab, lights;
    CHK(point_tables(c, latlon, n, rtab, ctab));
    CHK(epoch_lights(c, epochs, m, lights));
    std::vector<float> occ_s, occ_b, occ_m;     // section 3.18: empty segments without the tables
    if (occ_source) CHK(occult_tables(c, occ_source, occ_body, m, occ_s, occ_b, occ_m));
    std::vector<float> fl((size_t)m);
    for (int32_t k = 0; k < m; k++) fl[k] = (float)flux[k];
    const size_t nx = host_extra ? (size_t)n * (size_t)m : 0;
    const size_t out_bytes = (size_t)n * (size_t)width * (mode == 5 ? sizeof(double) : sizeof(float));
    QueryStage s;
    ThermalC q;
    CHK(stage_query(c, s, false, n, n, true, dev_out, out_bytes,
                    {rtab, ctab, lights, fl, horizon_seg(host_horizon, n, n_az), {host_extra, nx}, occ_s, occ_b, occ_m}, q, q.g));
    float** const d = s.d;
    if (occ_source) { q.occ_src = d[6]; q.occ_body = d[7]; q.occ_mark = reinterpret_cast<const int32_t*>(d[8]); }
    q.horizon = horizon_at(host_horizon, d[4], dev_horizon);
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
    CHK(stage_start(c, &s.cold, true));      // the counters: q.caps
    HIPCHK(c, mrtx_launch_thermal(s.f, q, ext, c->stream));
    CHK(stage_finish(c, dev_out, static_cast<float*>(host_out), out_bytes, out, kNoRays));
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
static int view_ok(mrtx_ctx* c, int32_t k) {
    if (!view_k_ok(k)) return fail(c, MRTX_E_INVALID, "K must be 16, 32, ..., 1024 (got %d)", k);
    return MRTX_OK;
}

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
    CHK(count_ok(c, n));
    CHK(view_ok(c, k));
    CHK(outputs_fit(c, (int64_t)n * (2 * (int64_t)k + 1)));
    CHK(one_of(c, dev_out, host_out, "out"));
    std::vector<float> rtab, ctab, dirs((size_t)k * 2);
    CHK(point_tables(c, latlon, n, rtab, ctab));
    const bool stats = counting(c);
    mrtx_view_dir_samples(k, dirs.data());
    const size_t out_bytes = (size_t)n * (2 * (size_t)k + 1) * sizeof(float);
    QueryStage s;
    ViewC q;
    CHK(stage_query(c, s, true, n, n, true, dev_out, out_bytes, {rtab, ctab, dirs}, q, q.g));
    q.dirs = s.d[2];
    q.out = (float*)dev_out; q.K = k;
    CHK(stage_start(c, &s.cold, stats));
    HIPCHK(c, mrtx_launch_view_hits(s.f, q, stats, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, stats ? kBounceRays : kNoRays);
}

int mrtx_scatter_flux(mrtx_ctx* c, const int32_t* index, int32_t n, int32_t k, const void* dev_exitance,
                      const float* host_exitance, int64_t exitance_len, int32_t n_hits, int32_t m, double albedo_h,
                      double emissivity, void* dev_out, float* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!index) return fail(c, MRTX_E_INVALID, "null index table");
    if (n < 1 || m < 1 || n_hits < 0) return fail(c, MRTX_E_INVALID, "need n >= 1, m >= 1 and n_hits >= 0 (got %d, %d, %d)", n, m, n_hits);
    CHK(view_ok(c, k));
    if (!(std::isfinite(albedo_h) && albedo_h >= 0.0 && albedo_h < 1.0))
        return fail(c, MRTX_E_INVALID, "the hemispherical albedo must be finite and in [0, 1) (got %g)", albedo_h);
    if (!(std::isfinite(emissivity) && emissivity > 0.0 && emissivity <= 1.0))
        return fail(c, MRTX_E_INVALID, "the emissivity must be finite and in (0, 1] (got %g)", emissivity);
    CHK(one_of(c, dev_exitance, host_exitance, "exitance"));
    CHK(one_of(c, dev_out, host_out, "out"));
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
    CHK(stage_out(c, dev_out, out_bytes));      // no frame, no grid: the call reads no DEM
    CHK(stage_tables(c, {{index, ni}, {host_exitance, ne}}, d));
    ScatterC q;
    std::memset(&q, 0, sizeof q);
    q.idx = reinterpret_cast<const int32_t*>(d[0]);
    q.ex = host_exitance ? d[1] : (const float*)dev_exitance;   // (n_hits = 0: never read, but not null)
    q.out = (float*)dev_out;
    q.n = n; q.K = k; q.m = m; q.chunks = (m + 63) / 64;
    q.omah = (float)(1.0 - albedo_h); q.eps = (float)emissivity; q.inv_k = (float)(1.0 / k);
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_scatter_flux(q, c->stream));
    return stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays);
}

// ==== The calls on a window of the DEM's texel lattice: traverses and relief.  Moved here as they were; of the vocabulary above
// they use CHK alone (their texts are their own: "a window holds ...", "dev_out must be 4-byte aligned") ======================
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
        CHK(start_rule(k, s));
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
    CHK(traverse_sources(c, t, src_ij, src_start, n_src, start_rule, sn, sc));
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    std::vector<float> len((size_t)t->rows * 3);
    CHK(traverse_window(c, t, c->dem_h, c->dem_w, len.data()));
    const size_t N = (size_t)t->rows * (size_t)t->cols;
    CHK(traverse_host_penalty(c, host_penalty, N));
    int TS;
    CHK(traverse_tile_edge(c, TS));
    // ---- device work from here
    FrameC f;
    FrameCold cold;
    CHK(stage_frame(c, f, cold, false));
    const int tiles_x = (t->cols + TS - 1) / TS, tiles_y = (t->rows + TS - 1) / TS;
    const size_t tiles = (size_t)tiles_x * (size_t)tiles_y;
    const size_t val_b = host_val ? N * 8 : 0, pred_b = host_pred ? (N + 15) & ~(size_t)15 : 0;
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, val_b + pred_b + 2 * tiles * 4));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    void* d_val = host_val ? tb : dev_val;
    uint8_t* d_pred = host_pred ? reinterpret_cast<uint8_t*>(tb + val_b) : static_cast<uint8_t*>(dev_pred);
    uint32_t* flags = reinterpret_cast<uint32_t*>(tb + val_b + pred_b);
    const size_t np = host_penalty ? N : 0;
    float* d[5];
    CHK(stage_tables(c, {len, {sn.data(), 2 * sn.size()}, {sc.data(), 2 * sc.size()}, {host_penalty, np}, extra}, d));
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
    CHK(stage_start(c, nullptr, true));
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
    CHK(traverse_params(c, t));
    if (dev_penalty && host_penalty) return fail(c, MRTX_E_INVALID, "give at most one of dev_penalty and host_penalty");
    if ((dev_cost == nullptr) == (host_cost == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_cost and host_cost");
    if ((dev_pred == nullptr) == (host_pred == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_pred and host_pred");
    CHK(traverse_dev_buffers(c, t, dev_penalty, dev_cost, dev_pred));
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
    CHK(traverse_params(c, t));
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
    CHK(traverse_dev_buffers(c, t, dev_penalty, dev_arrival, dev_pred));
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
    CHK(traverse_params(c, t));
    if ((dev_out == nullptr) == (host_out == nullptr)) return fail(c, MRTX_E_INVALID, "give exactly one of dev_out and host_out");
    if (dev_out && (reinterpret_cast<uintptr_t>(dev_out) & 3)) return fail(c, MRTX_E_INVALID, "dev_out must be 4-byte aligned");
    if (!c->dem) return fail(c, MRTX_E_STATE, "no displacement map: call mrtx_upload_dem first");
    CHK(traverse_window(c, t, c->dem_h, c->dem_w, nullptr));
    FrameC f;
    FrameCold cold;
    CHK(stage_frame(c, f, cold, false));
    const size_t bytes = (size_t)t->rows * (size_t)t->cols * sizeof(float);
    CHK(stage_out(c, dev_out, bytes));
    TraverseC q;
    std::memset(&q, 0, sizeof q);
    traverse_fill_window(c, f, t, q);
    CHK(stage_start(c, nullptr, false));
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
    CHK(relief_params(c, r));
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
    CHK(relief_window(c, r, c->dem_h, c->dem_w, scale.data()));
    FrameC f;
    FrameCold cold;
    CHK(stage_frame(c, f, cold, false));
    const bool stats = (c->prm.flags & MRTX_F_COUNT_STATS) != 0;
    const size_t bytes = (size_t)r->rows * (size_t)r->cols * 16;
    float* d[1];
    CHK(stage_out(c, dev_out, bytes));
    CHK(stage_tables(c, {{scale.data(), 2 * scale.size()}}, d));
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
    CHK(stage_start(c, nullptr, stats));
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
    float* d[1] = {nullptr};
    CHK(stage_out(c, dev_out, 4 * N));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, 4 * N));
    CHK(stage_tables(c, {{host_relief, host_relief ? 4 * N : 0}}, d));
    ShareC q;
    std::memset(&q, 0, sizeof q);
    q.relief = host_relief ? reinterpret_cast<const float4*>(d[0]) : static_cast<const float4*>(dev_relief);
    q.sat = reinterpret_cast<uint32_t*>(c->trav_buf);
    q.out = static_cast<float*>(dev_out);
    q.rows = s->rows; q.cols = s->cols; q.Ri = s->Ri; q.Rj = s->Rj; q.wrap = s->wrap;
    q.gmax = (float)s->grade_max; q.smax = (float)s->rms_max;
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_relief_share(q, c->stream));
    CHK(stage_finish(c, dev_out, host_out, 4 * N, out, kNoRays));
    if (out) out->launches = 3;
    return MRTX_OK;
}

}  // extern "C"
