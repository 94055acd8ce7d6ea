// mrtx_lattice_api.hip -- host side of the lattice calls of libmoonrt.so: the entry points that work on a
// lattice of nodes and its tables, not on the DEM and its march.  mrtx_regions_label, mrtx_regions_stats, mrtx_regions_zonal,
// mrtx_regions_shape, mrtx_proximity, mrtx_regions_reach, mrtx_regions_outline, mrtx_contours, mrtx_fill, mrtx_fill_basins,
// mrtx_bowls and mrtx_rasterise.  Their kernels lie in a unit per stage (mrtx_regions.hip ... mrtx_raster.hip); the context and the staging, launch
// and read-back path are mrtx_api.hip's (mrtx_host.h).  No device code.
//
// Every entry point reads: parameters, checks, layout, launches, read-back.  The checks are calls of the small functions below,
// inline and in the order in which the call refuses: an argument set with two defects is refused for the first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "mrtx_host.h"
#include "mrtx_regions.h"
#include "mrtx_zonal.h"
#include "mrtx_proximity.h"
#include "mrtx_outline.h"
#include "mrtx_contour.h"
#include "mrtx_fill.h"
#include "mrtx_bowls.h"
#include "mrtx_raster.h"

using namespace mrtx_host;

namespace {

// ---- The vocabulary of the argument checks: each returns MRTX_OK or the code of fail() with its text.  CHK, one_of,
// at_most_one, aligned and variant are mrtx_host.h's: the terrain calls word them alike ---------------------------------------
int lattice_ok(mrtx_ctx* c, int32_t rows, int32_t cols, int32_t wrap) {
    if (rows < 1 || cols < 1) return fail(c, MRTX_E_INVALID, "empty lattice (%d x %d)", rows, cols);
    if ((int64_t)rows * (int64_t)cols > (int64_t)1 << 31)
        return fail(c, MRTX_E_INVALID, "a lattice holds at most 2^31 nodes (got %d x %d)", rows, cols);
    if (wrap != 0 && wrap != 1) return fail(c, MRTX_E_INVALID, "wrap must be 0 or 1 (got %d)", wrap);
    if (wrap && cols < 3) return fail(c, MRTX_E_INVALID, "a wrapped lattice needs cols >= 3 (got %d)", cols);
    return MRTX_OK;
}

int connectivity_ok(mrtx_ctx* c, int32_t connectivity) {
    if (connectivity != 4 && connectivity != 8) return fail(c, MRTX_E_INVALID, "connectivity must be 4 or 8 (got %d)", connectivity);
    return MRTX_OK;
}

int regions_fit(mrtx_ctx* c, uint32_t n_regions, size_t N) {
    if ((size_t)n_regions > N) return fail(c, MRTX_E_INVALID, "n_regions = %u exceeds the lattice's %zu nodes", n_regions, N);
    return MRTX_OK;
}

// Do no two of the device tables share a byte?  Every pair is tested but those among the first `may_alias` spans: the inputs
// of the calls that only read them.  Which calls those are is DESIGN.md section 4.34's to say; a null table overlaps nothing.
struct Span {
    const void* p;
    size_t bytes;
};
bool disjoint(std::initializer_list<Span> spans, size_t may_alias = 0) {
    const Span* s = spans.begin();
    for (size_t j = 1; j < spans.size(); j++)
        for (size_t i = 0; i < j; i++)
            if (j >= may_alias && spans_overlap(s[i].p, s[i].bytes, s[j].p, s[j].bytes)) return false;
    return true;
}

// the refusal of a label table after the launch that counted its bad entries
int label_refusal(mrtx_ctx* c, uint32_t bad, uint32_t n_regions) {
    return fail(c, MRTX_E_INVALID, "the label table holds %u entries outside -1 .. n_regions - 1 = %lld", bad, (long long)n_regions - 1);
}
int bad_labels(mrtx_ctx* c, const uint32_t* counter, uint32_t n_regions) {
    uint32_t bad = 0;
    HIPCHK(c, hipMemcpy(&bad, counter, sizeof bad, hipMemcpyDeviceToHost));
    return bad ? label_refusal(c, bad, n_regions) : MRTX_OK;
}

// where the kernels find a table: where the host's copy was staged, or else where the caller put it on the device
template <class T>
const T* in_table(const void* host, const void* staged, const void* dev) {
    return host ? static_cast<const T*>(staged) : static_cast<const T*>(dev);
}
template <class T>
T* out_table(const void* host, void* staged, void* dev) {
    return host ? static_cast<T*>(staged) : static_cast<T*>(dev);
}

// The result tables that mrtx_regions_outline and mrtx_contours share: records (rings, lines) and their vertices, each from the
// device, from the host or absent, with the caps the caller gives and the counts it gets.
struct TraceTables {
    const char *rec, *recs;                 // "ring" and "rings", "line" and "lines"
    const void *dev_recs, *host_recs;
    uint64_t rec_cap;
    const void *dev_vertices, *host_vertices;
    uint64_t vertex_cap;
    const uint64_t *n_recs, *n_vertices;
};

// both tables or neither (*has), no caps without tables, and somewhere to put the counts
int trace_tables(mrtx_ctx* c, const TraceTables& t, bool* has) {
    if (!t.n_recs || !t.n_vertices) return fail(c, MRTX_E_INVALID, "null n_%s or n_vertices", t.recs);
    CHK(at_most_one(c, t.dev_recs, t.host_recs, t.recs));
    CHK(at_most_one(c, t.dev_vertices, t.host_vertices, "vertices"));
    *has = t.dev_recs || t.host_recs;
    if (*has != (t.dev_vertices || t.host_vertices))
        return fail(c, MRTX_E_INVALID, "give a %s table and a vertex table, or neither to count", t.rec);
    if (!*has && (t.rec_cap || t.vertex_cap))
        return fail(c, MRTX_E_INVALID, "without tables %s_cap and vertex_cap must be 0 (got %llu, %llu)", t.rec,
                    (unsigned long long)t.rec_cap, (unsigned long long)t.vertex_cap);
    return MRTX_OK;
}

// the refusal of tables that the counts do not fit
int tables_too_small(mrtx_ctx* c, const TraceTables& t, uint64_t recs, uint64_t vertices) {
    return fail(c, MRTX_E_INVALID, "the tables are too small: %llu %s and %llu vertices are needed (%s_cap = %llu, vertex_cap = %llu)",
                (unsigned long long)recs, t.recs, (unsigned long long)vertices, t.rec, (unsigned long long)t.rec_cap,
                (unsigned long long)t.vertex_cap);
}

// the end of a stage of several launches: stage_finish, then the launches it made
int lattice_finish(mrtx_ctx* c, const void* dev_out, float* host_out, size_t out_bytes, MrtxStats* out, uint32_t launches) {
    CHK(stage_finish(c, dev_out, host_out, out_bytes, out, kNoRays));
    if (out) out->launches = launches;
    return MRTX_OK;
}

// The calls that wait between their launches (mrtx_fill, mrtx_bowls) keep their own time.  lap: the end of a device phase, its
// time added to *ms (the next phase starts with another record of ev0); report: what ran, into the caller's statistics.
int lap(mrtx_ctx* c, float* ms) {
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float t = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&t, c->ev0, c->ev1));
    *ms += t;
    return MRTX_OK;
}
void report(MrtxStats* out, float ms, uint32_t launches) {
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->kernel_ms = ms;
    out->launches = launches;
}

}  // namespace

extern "C" {

// ---- Connected regions of a per-node map ----------------------------------------------------------
static_assert(sizeof(MrtxRegion) == 56 && sizeof(RegionRec) == sizeof(MrtxRegion), "MrtxRegion is 56 bytes");

int mrtx_regions_label(mrtx_ctx* c, const MrtxRegions* r, const void* dev_field, const float* host_field, const void* dev_mask,
                       const uint8_t* host_mask, void* dev_labels, int32_t* host_labels, uint32_t* n_regions, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!r) return fail(c, MRTX_E_INVALID, "null regions block");
    if (r->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, r->rows, r->cols, r->wrap));
    CHK(connectivity_ok(c, r->connectivity));
    const bool has_field = dev_field || host_field, has_mask = dev_mask || host_mask;
    if (has_field == has_mask) return fail(c, MRTX_E_INVALID, "give exactly one of a field and a mask");
    if (dev_field && host_field) return fail(c, MRTX_E_INVALID, "give exactly one of dev_field and host_field");
    if (dev_mask && host_mask) return fail(c, MRTX_E_INVALID, "give exactly one of dev_mask and host_mask");
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    if (!n_regions) return fail(c, MRTX_E_INVALID, "null n_regions");
    if (has_field) {
        if (r->n_ch < 1 || r->n_ch > 16) return fail(c, MRTX_E_INVALID, "n_ch must lie in 1 .. 16 (got %d)", r->n_ch);
        if (r->ch < 0 || r->ch >= r->n_ch) return fail(c, MRTX_E_INVALID, "ch must lie in 0 .. n_ch - 1 (got %d of %d)", r->ch, r->n_ch);
        if (std::isnan(r->lo) || std::isnan(r->hi)) return fail(c, MRTX_E_INVALID, "lo and hi must not be NaN");
        if (r->lo > r->hi) return fail(c, MRTX_E_INVALID, "lo must be <= hi (got %g > %g)", r->lo, r->hi);
    }
    CHK(aligned(c, dev_field, 4, "dev_field", "float32"));
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    const size_t N = (size_t)r->rows * (size_t)r->cols;
    const size_t in_bytes = has_field ? 4 * N * (size_t)r->n_ch : N;
    if (!disjoint({{dev_field ? dev_field : dev_mask, in_bytes}, {dev_labels, 4 * N}}))
        return fail(c, MRTX_E_INVALID, "the device input and dev_labels must not overlap");
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    RegionsC q;
    std::memset(&q, 0, sizeof q);
    q.n_chunks = (uint32_t)((N + MRTX_RG_CHUNK - 1) / MRTX_RG_CHUNK);
    q.tiles_x = (r->cols + MRTX_RG_TW - 1) / MRTX_RG_TW;
    // scratch: the forest, the chunks' counts, K
    const size_t sums_at = 4 * N, total_at = sums_at + 4 * (size_t)q.n_chunks;
    CHK(stage_out(c, dev_labels, 4 * N));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, total_at + 16));
    if (host_field || host_mask) {      // the caller's memory stays put until stage_finish
        CHK(stage_buffer(c, c->illum_tab, c->illum_tab_bytes, std::max(in_bytes, (size_t)16)));
        HIPCHK(c, hipMemcpyAsync(c->illum_tab, host_field ? (const void*)host_field : (const void*)host_mask, in_bytes,
                                 hipMemcpyHostToDevice, c->stream));
    }
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    if (has_field) q.field = in_table<float>(host_field, c->illum_tab, dev_field);
    else q.mask = in_table<uint8_t>(host_mask, c->illum_tab, dev_mask);
    q.parent = reinterpret_cast<int32_t*>(tb);
    q.sums = reinterpret_cast<uint32_t*>(tb + sums_at);
    q.total = reinterpret_cast<uint32_t*>(tb + total_at);
    q.labels = static_cast<int32_t*>(dev_labels);
    q.rows = r->rows; q.cols = r->cols; q.wrap = r->wrap; q.conn8 = r->connectivity == 8; q.n_ch = r->n_ch; q.ch = r->ch;
    q.lo = (float)r->lo; q.hi = (float)r->hi;
    uint32_t launches = 0, K = 0;
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_regions_label(q, c->stream, &launches));
    CHK(stage_finish(c, dev_labels, reinterpret_cast<float*>(host_labels), 4 * N, out, kNoRays));
    HIPCHK(c, hipMemcpy(&K, q.total, sizeof K, hipMemcpyDeviceToHost));
    *n_regions = K;
    if (out) out->launches = launches;
    return MRTX_OK;
}

int mrtx_regions_stats(mrtx_ctx* c, int32_t rows, int32_t cols, int32_t wrap, const void* dev_labels, const int32_t* host_labels,
                       uint32_t n_regions, const uint32_t* row_weight, void* dev_out, MrtxRegion* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    CHK(lattice_ok(c, rows, cols, wrap));
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    CHK(one_of(c, dev_out, host_out, "out"));
    const size_t N = (size_t)rows * (size_t)cols;
    CHK(regions_fit(c, n_regions, N));
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_out, 8, "dev_out", "MrtxRegion"));
    const size_t out_bytes = sizeof(MrtxRegion) * (size_t)n_regions;
    if (!disjoint({{dev_labels, 4 * N}, {dev_out, out_bytes}})) return fail(c, MRTX_E_INVALID, "dev_labels and dev_out must not overlap");
    // MOONRT_REGIONS_CATALOGUE=plain: one set of atomics per node, the yardstick of the in-wave run reduction; the same records
    bool runs = true;
    CHK(variant(c, "MOONRT_REGIONS_CATALOGUE", "runs", "plain", &runs));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    float* d[2] = {nullptr, nullptr};
    CHK(stage_out(c, dev_out, std::max(out_bytes, sizeof(MrtxRegion))));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, 16));
    CHK(stage_tables(c, {{host_labels, host_labels ? N : 0}, {row_weight, row_weight ? (size_t)rows : 0}}, d));
    RegionStatsC q;
    std::memset(&q, 0, sizeof q);
    q.labels = in_table<int32_t>(host_labels, d[0], dev_labels);
    q.row_weight = in_table<uint32_t>(row_weight, d[1], nullptr);
    q.out = static_cast<RegionRec*>(dev_out);
    q.bad = reinterpret_cast<uint32_t*>(c->trav_buf);
    q.rows = rows; q.cols = cols; q.wrap = wrap; q.n_regions = n_regions;
    uint32_t launches = 0;
    HIPCHK(c, hipMemsetAsync(q.bad, 0, 16, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_regions_stats(q, runs, c->stream, &launches));
    CHK(lattice_finish(c, dev_out, reinterpret_cast<float*>(host_out), out_bytes, out, launches));
    return bad_labels(c, q.bad, n_regions);
}

// ---- Zonal statistics and outlines of labelled regions -------------------------------------------
static_assert(sizeof(MrtxZonal) == 56 && sizeof(ZonalRec) == sizeof(MrtxZonal), "MrtxZonal is 56 bytes");
static_assert(sizeof(MrtxRegionShape) == 32 && sizeof(ShapeRec) == sizeof(MrtxRegionShape), "MrtxRegionShape is 32 bytes");

int mrtx_regions_zonal(mrtx_ctx* c, const MrtxZonalSpec* z, const void* dev_labels, const int32_t* host_labels, uint32_t n_regions,
                       const void* dev_field, const float* host_field, const uint32_t* row_weight, void* dev_out,
                       MrtxZonal* host_out, void* dev_hist, uint64_t* host_hist, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!z) return fail(c, MRTX_E_INVALID, "null zonal block");
    if (z->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, z->rows, z->cols, z->wrap));
    if (z->n_ch < 1 || z->n_ch > 16) return fail(c, MRTX_E_INVALID, "n_ch must lie in 1 .. 16 (got %d)", z->n_ch);
    if (!std::isfinite(z->scale) || !(z->scale > 0.0)) return fail(c, MRTX_E_INVALID, "scale must be finite and > 0 (got %g)", z->scale);
    if (z->n_bins < 0 || z->n_bins > 4096) return fail(c, MRTX_E_INVALID, "n_bins must lie in 0 .. 4096 (got %d)", z->n_bins);
    if (z->n_bins) {
        if (z->hist_ch < 0 || z->hist_ch >= z->n_ch)
            return fail(c, MRTX_E_INVALID, "hist_ch must lie in 0 .. n_ch - 1 (got %d of %d)", z->hist_ch, z->n_ch);
        if (!std::isfinite(z->hist_lo) || !std::isfinite(z->hist_inv_w) || !(z->hist_inv_w > 0.0))
            return fail(c, MRTX_E_INVALID, "hist_lo must be finite and hist_inv_w finite and > 0 (got %g, %g)", z->hist_lo, z->hist_inv_w);
    }
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    CHK(one_of(c, dev_field, host_field, "field"));
    CHK(one_of(c, dev_out, host_out, "out"));
    if (z->n_bins == 0 && (dev_hist || host_hist)) return fail(c, MRTX_E_INVALID, "without bins dev_hist and host_hist must be NULL");
    if (z->n_bins && (dev_hist == nullptr) == (host_hist == nullptr))
        return fail(c, MRTX_E_INVALID, "give exactly one of dev_hist and host_hist");
    const size_t N = (size_t)z->rows * (size_t)z->cols;
    CHK(regions_fit(c, n_regions, N));
    const size_t H = z->n_bins ? (size_t)n_regions * (size_t)(z->n_bins + 2) : 0;
    if (H > ((size_t)1 << 28))
        return fail(c, MRTX_E_INVALID, "a histogram holds at most 2^28 columns (got %u x %d)", n_regions, z->n_bins + 2);
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_field, 4, "dev_field", "float32"));
    CHK(aligned(c, dev_out, 8, "dev_out", "MrtxZonal"));
    CHK(aligned(c, dev_hist, 8, "dev_hist", "uint64"));
    const size_t R = (size_t)n_regions * (size_t)z->n_ch;
    const size_t out_bytes = sizeof(MrtxZonal) * R, field_bytes = 4 * N * (size_t)z->n_ch, hist_bytes = 8 * H;
    if (!disjoint({{dev_labels, 4 * N}, {dev_field, field_bytes}, {dev_out, out_bytes}, {dev_hist, hist_bytes}}, 2))      // two inputs
        return fail(c, MRTX_E_INVALID, "the device inputs, dev_out and dev_hist must not overlap");
    // MOONRT_REGIONS_ZONAL=plain: one set of atomics per node, the yardstick of the in-wave run reduction; the same records
    bool runs = true;
    CHK(variant(c, "MOONRT_REGIONS_ZONAL", "runs", "plain", &runs));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // scratch: the count of bad entries, the packed extremes, and the histogram when it goes to the host
    const size_t keys_at = 16, hist_at = keys_at + 16 * R;
    float* d[3] = {nullptr, nullptr, nullptr};
    CHK(stage_out(c, dev_out, std::max(out_bytes, sizeof(MrtxZonal))));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, hist_at + (host_hist ? hist_bytes : 0) + 16));
    CHK(stage_tables(c, {{host_labels, host_labels ? N : 0}, {row_weight, row_weight ? (size_t)z->rows : 0}, {host_field, host_field ? N * (size_t)z->n_ch : 0}}, d));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    ZonalC q;
    std::memset(&q, 0, sizeof q);
    q.labels = in_table<int32_t>(host_labels, d[0], dev_labels);
    q.row_weight = in_table<uint32_t>(row_weight, d[1], nullptr);
    q.field = in_table<float>(host_field, d[2], dev_field);
    q.out = static_cast<ZonalRec*>(dev_out);
    q.bad = reinterpret_cast<uint32_t*>(tb);
    q.keys = reinterpret_cast<unsigned long long*>(tb + keys_at);
    q.hist = z->n_bins ? out_table<unsigned long long>(host_hist, tb + hist_at, dev_hist) : nullptr;
    q.scale = z->scale; q.hist_lo = z->hist_lo; q.hist_inv_w = z->hist_inv_w;
    q.rows = z->rows; q.cols = z->cols; q.n_ch = z->n_ch; q.hist_ch = z->hist_ch; q.n_bins = z->n_bins; q.n_regions = n_regions;
    uint32_t launches = 0;
    HIPCHK(c, hipMemsetAsync(q.bad, 0, 16, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_regions_zonal(q, runs, c->stream, &launches));
    CHK(lattice_finish(c, dev_out, reinterpret_cast<float*>(host_out), out_bytes, out, launches));
    if (host_hist && hist_bytes) HIPCHK(c, hipMemcpy(host_hist, q.hist, hist_bytes, hipMemcpyDeviceToHost));
    return bad_labels(c, q.bad, n_regions);
}

int mrtx_regions_shape(mrtx_ctx* c, int32_t rows, int32_t cols, int32_t wrap, int32_t connectivity, const void* dev_labels,
                       const int32_t* host_labels, uint32_t n_regions, const uint32_t* side_ew, const uint32_t* side_ns, void* dev_out,
                       MrtxRegionShape* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    CHK(lattice_ok(c, rows, cols, wrap));
    CHK(connectivity_ok(c, connectivity));
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    CHK(one_of(c, dev_out, host_out, "out"));
    if ((side_ew == nullptr) != (side_ns == nullptr)) return fail(c, MRTX_E_INVALID, "give both of side_ew and side_ns or neither");
    const size_t N = (size_t)rows * (size_t)cols;
    CHK(regions_fit(c, n_regions, N));
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_out, 8, "dev_out", "MrtxRegionShape"));
    const size_t out_bytes = sizeof(MrtxRegionShape) * (size_t)n_regions;
    if (!disjoint({{dev_labels, 4 * N}, {dev_out, out_bytes}})) return fail(c, MRTX_E_INVALID, "dev_labels and dev_out must not overlap");
    // MOONRT_REGIONS_ZONAL=plain: one set of atomics per node, the yardstick of the in-wave run reduction; the same records
    bool runs = true;
    CHK(variant(c, "MOONRT_REGIONS_ZONAL", "runs", "plain", &runs));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    float* d[3] = {nullptr, nullptr, nullptr};
    CHK(stage_out(c, dev_out, std::max(out_bytes, sizeof(MrtxRegionShape))));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, 16));
    CHK(stage_tables(c, {{host_labels, host_labels ? N : 0}, {side_ew, side_ew ? (size_t)rows : 0}, {side_ns, side_ns ? (size_t)rows + 1 : 0}}, d));
    ShapeC q;
    std::memset(&q, 0, sizeof q);
    q.labels = in_table<int32_t>(host_labels, d[0], dev_labels);
    q.side_ew = in_table<uint32_t>(side_ew, d[1], nullptr);
    q.side_ns = in_table<uint32_t>(side_ns, d[2], nullptr);
    q.out = static_cast<ShapeRec*>(dev_out);
    q.bad = reinterpret_cast<uint32_t*>(c->trav_buf);
    q.rows = rows; q.cols = cols; q.wrap = wrap; q.conn8 = connectivity == 8; q.n_regions = n_regions;
    uint32_t launches = 0;
    HIPCHK(c, hipMemsetAsync(q.bad, 0, 16, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_regions_shape(q, runs, c->stream, &launches));
    CHK(lattice_finish(c, dev_out, reinterpret_cast<float*>(host_out), out_bytes, out, launches));
    return bad_labels(c, q.bad, n_regions);
}

// ---- Proximity maps and the reach of labelled regions ---------------------------------------------
static_assert(sizeof(MrtxRegionReach) == 32 && sizeof(ReachRec) == sizeof(MrtxRegionReach), "MrtxRegionReach is 32 bytes");
static_assert(sizeof(MrtxProximity) == 16 && sizeof(ProxBox) == 32 && sizeof(ProxFeat) == 16, "the proximity blocks");

int mrtx_proximity(mrtx_ctx* c, const MrtxProximity* p, const void* dev_pos, const int32_t* host_pos, const void* dev_labels,
                   const int32_t* host_labels, void* dev_nearest, int32_t* host_nearest, void* dev_dist2, uint64_t* host_dist2,
                   uint64_t* pairs, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!p) return fail(c, MRTX_E_INVALID, "null proximity block");
    if (p->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, p->rows, p->cols, 0));
    if (p->mode != MRTX_PROX_TO_SET && p->mode != MRTX_PROX_TO_OUTSIDE)
        return fail(c, MRTX_E_INVALID, "mode must be MRTX_PROX_TO_SET or MRTX_PROX_TO_OUTSIDE (got %d)", p->mode);
    CHK(one_of(c, dev_pos, host_pos, "pos"));
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    CHK(one_of(c, dev_nearest, host_nearest, "nearest"));
    CHK(one_of(c, dev_dist2, host_dist2, "dist2"));
    CHK(aligned(c, dev_pos, 4, "dev_pos", "int32"));
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_nearest, 4, "dev_nearest", "int32"));
    CHK(aligned(c, dev_dist2, 8, "dev_dist2", "uint64"));
    const size_t N = (size_t)p->rows * (size_t)p->cols;
    if (!disjoint({{dev_pos, 12 * N}, {dev_labels, 4 * N}, {dev_nearest, 4 * N}, {dev_dist2, 8 * N}}))
        return fail(c, MRTX_E_INVALID, "dev_pos, dev_labels, dev_nearest and dev_dist2 must not overlap");
    // MOONRT_PROXIMITY=brute: every tile's features against every node, the yardstick of the pruned scan; the same bytes
    bool prune = true;
    CHK(variant(c, "MOONRT_PROXIMITY", "prune", "brute", &prune));
    // a host table is refused at its first bad coordinate (a device table's are counted by the tile kernel)
    if (host_pos)
        for (size_t n = 0; n < 3 * N; n++)
            if (host_pos[n] < -MRTX_PX_CMAX || host_pos[n] > MRTX_PX_CMAX)
                return fail(c, MRTX_E_INVALID, "coordinate %zu of node %zu must lie in -2^29 .. 2^29 (got %d)", n % 3, n / 3, host_pos[n]);
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // scratch: the counters, the tiles' boxes and feature lists, and the outputs the caller wants on the host
    const ProxLayout at = prox_layout(p->rows, p->cols, host_nearest != nullptr, host_dist2 != nullptr);
    float* d[2] = {nullptr, nullptr};
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, at.end));
    CHK(stage_tables(c, {{host_pos, host_pos ? 3 * N : 0}, {host_labels, host_labels ? N : 0}}, d));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    ProxC q;
    std::memset(&q, 0, sizeof q);
    q.pos = in_table<int32_t>(host_pos, d[0], dev_pos);
    q.labels = in_table<int32_t>(host_labels, d[1], dev_labels);
    q.nearest = out_table<int32_t>(host_nearest, tb + at.near_at, dev_nearest);
    q.dist2 = out_table<unsigned long long>(host_dist2, tb + at.d2_at, dev_dist2);
    q.pairs = reinterpret_cast<unsigned long long*>(tb);
    q.bad = reinterpret_cast<uint32_t*>(tb + 8);
    q.box = reinterpret_cast<ProxBox*>(tb + at.box_at);
    q.feat = reinterpret_cast<ProxFeat*>(tb + at.feat_at);
    q.rows = p->rows; q.cols = p->cols; q.outside = p->mode == MRTX_PROX_TO_OUTSIDE; q.tiles_x = at.tiles_x; q.tiles_y = at.tiles_y;
    uint32_t launches = 0;
    unsigned long long head[2] = {0, 0};                    // pairs, bad
    HIPCHK(c, hipMemsetAsync(tb, 0, 32, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_proximity(q, prune, c->stream, &launches));
    CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    if ((uint32_t)head[1])
        return fail(c, MRTX_E_INVALID, "%u coordinates of the device position table lie outside -2^29 .. 2^29", (uint32_t)head[1]);
    if (host_nearest) HIPCHK(c, hipMemcpy(host_nearest, q.nearest, 4 * N, hipMemcpyDeviceToHost));
    if (host_dist2) HIPCHK(c, hipMemcpy(host_dist2, q.dist2, 8 * N, hipMemcpyDeviceToHost));
    if (pairs) *pairs = head[0];
    return MRTX_OK;
}

int mrtx_regions_reach(mrtx_ctx* c, int32_t rows, int32_t cols, const void* dev_labels, const int32_t* host_labels, uint32_t n_regions,
                       const void* dev_dist2, const uint64_t* host_dist2, const void* dev_nearest, const int32_t* host_nearest,
                       void* dev_out, MrtxRegionReach* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    CHK(lattice_ok(c, rows, cols, 0));
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    CHK(one_of(c, dev_dist2, host_dist2, "dist2"));
    CHK(one_of(c, dev_nearest, host_nearest, "nearest"));
    CHK(one_of(c, dev_out, host_out, "out"));
    const size_t N = (size_t)rows * (size_t)cols;
    CHK(regions_fit(c, n_regions, N));
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_dist2, 8, "dev_dist2", "uint64"));
    CHK(aligned(c, dev_nearest, 4, "dev_nearest", "int32"));
    CHK(aligned(c, dev_out, 8, "dev_out", "MrtxRegionReach"));
    const size_t out_bytes = sizeof(MrtxRegionReach) * (size_t)n_regions;
    if (!disjoint({{dev_labels, 4 * N}, {dev_dist2, 8 * N}, {dev_nearest, 4 * N}, {dev_out, out_bytes}}, 3))      // three inputs
        return fail(c, MRTX_E_INVALID, "the device inputs and dev_out must not overlap");
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    float* d[3] = {nullptr, nullptr, nullptr};
    CHK(stage_out(c, dev_out, std::max(out_bytes, sizeof(MrtxRegionReach))));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, 16));
    CHK(stage_tables(c, {{host_labels, host_labels ? N : 0}, {host_dist2, host_dist2 ? 2 * N : 0}, {host_nearest, host_nearest ? N : 0}}, d));
    ReachC q;
    std::memset(&q, 0, sizeof q);
    q.labels = in_table<int32_t>(host_labels, d[0], dev_labels);
    q.dist2 = in_table<unsigned long long>(host_dist2, d[1], dev_dist2);
    q.nearest = in_table<int32_t>(host_nearest, d[2], dev_nearest);
    q.out = static_cast<ReachRec*>(dev_out);
    q.bad = reinterpret_cast<uint32_t*>(c->trav_buf);
    q.rows = rows; q.cols = cols; q.n_regions = n_regions;
    uint32_t launches = 0;
    HIPCHK(c, hipMemsetAsync(q.bad, 0, 16, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_regions_reach(q, c->stream, &launches));
    CHK(lattice_finish(c, dev_out, reinterpret_cast<float*>(host_out), out_bytes, out, launches));
    return bad_labels(c, q.bad, n_regions);
}

// ---- Region outlines: the ordered boundary rings of a label table --------------------------------
static_assert(sizeof(MrtxRing) == 48 && sizeof(RingRec) == sizeof(MrtxRing), "MrtxRing is 48 bytes");
static_assert(sizeof(OutlineJump) == 32, "two int4");

int mrtx_regions_outline(mrtx_ctx* c, const MrtxOutline* o, const void* dev_labels, const int32_t* host_labels, uint32_t n_regions,
                         const uint32_t* row_weight, void* dev_rings, MrtxRing* host_rings, uint64_t ring_cap, void* dev_vertices,
                         int32_t* host_vertices, uint64_t vertex_cap, uint64_t* n_rings, uint64_t* n_vertices, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!o) return fail(c, MRTX_E_INVALID, "null outline block");
    if (o->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, o->rows, o->cols, o->wrap));
    if ((int64_t)o->rows * (int64_t)o->cols > MRTX_OL_MAX_NODES)
        return fail(c, MRTX_E_INVALID, "an outlined lattice holds at most 2^28 nodes (got %d x %d)", o->rows, o->cols);
    CHK(connectivity_ok(c, o->connectivity));
    if (o->mode != MRTX_OUTLINE_ALL && o->mode != MRTX_OUTLINE_CORNERS)
        return fail(c, MRTX_E_INVALID, "mode must be MRTX_OUTLINE_ALL or MRTX_OUTLINE_CORNERS (got %d)", o->mode);
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    const TraceTables tabs = {"ring", "rings", dev_rings, host_rings, ring_cap, dev_vertices, host_vertices, vertex_cap, n_rings, n_vertices};
    bool has_rings;
    CHK(trace_tables(c, tabs, &has_rings));
    const size_t N = (size_t)o->rows * (size_t)o->cols;
    CHK(regions_fit(c, n_regions, N));
    // a table never needs more than one ring per three sides and one vertex per side
    const size_t ring_bytes = sizeof(MrtxRing) * (size_t)std::min<uint64_t>(ring_cap, 4 * N);
    const size_t vertex_bytes = 8 * (size_t)std::min<uint64_t>(vertex_cap, 4 * N);
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_rings, 8, "dev_rings", "MrtxRing"));
    CHK(aligned(c, dev_vertices, 4, "dev_vertices", "int32"));
    if (!disjoint({{dev_labels, 4 * N}, {dev_rings, ring_bytes}, {dev_vertices, vertex_bytes}}))
        return fail(c, MRTX_E_INVALID, "dev_labels, dev_rings and dev_vertices must not overlap");
    // MOONRT_REGIONS_OUTLINE=jump: pointer jumping over every boundary side, the yardstick of the contraction of the chains
    // inside a tile; the same bytes
    bool contract = MRTX_OL_DEFAULT_CONTRACT;
    CHK(variant(c, "MOONRT_REGIONS_OUTLINE", "contract", "jump", &contract));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::vector<uint64_t> cw;
    if (row_weight) {
        cw.assign((size_t)o->rows + 1, 0);
        for (int32_t i = 0; i < o->rows; i++) cw[(size_t)i + 1] = cw[i] + row_weight[i];
    }
    const OutlineNodeLayout nl = outline_node_layout(o->rows, o->cols);
    float* d[2] = {nullptr, nullptr};
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, nl.end));
    CHK(stage_tables(c, {{host_labels, host_labels ? N : 0}, {cw.data(), 2 * cw.size()}}, d));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    OutlineC q;
    std::memset(&q, 0, sizeof q);
    q.labels = in_table<int32_t>(host_labels, d[0], dev_labels);
    q.cw = in_table<unsigned long long>(row_weight, d[1], nullptr);
    q.bad = reinterpret_cast<uint32_t*>(tb);
    q.totals = reinterpret_cast<unsigned long long*>(tb + 16);
    q.bits = reinterpret_cast<uint8_t*>(tb + nl.bits_at);
    q.base = reinterpret_cast<uint32_t*>(tb + nl.base_at);
    q.node_sums = reinterpret_cast<uint2*>(tb + nl.sums_at);
    q.rows = o->rows; q.cols = o->cols; q.wrap = o->wrap; q.conn8 = o->connectivity == 8; q.all = o->mode == MRTX_OUTLINE_ALL;
    q.n_regions = n_regions; q.contract = contract;
    uint32_t launches = 0;
    unsigned long long head[6] = {0, 0, 0, 0, 0, 0};            // bad (and padding), then the four totals
    HIPCHK(c, hipMemsetAsync(tb, 0, 64, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_outline_mark(q, c->stream, &launches));
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // also: the pageable tables are no longer read
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    if ((uint32_t)head[0]) {                                    // as the sibling calls: the stage ends, out says what ran
        CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
        return label_refusal(c, (uint32_t)head[0], n_regions);
    }
    q.B = (uint32_t)head[2];
    q.rounds = outline_rounds(q.B);
    uint64_t rings = 0, vertices = 0;
    bool fits = true;
    if (q.B) {
        const OutlineSideLayout sl = outline_side_layout(q.B);
        CHK(stage_buffer(c, c->illum_out, c->illum_out_bytes, sl.end));
        char* sb = reinterpret_cast<char*>(c->illum_out);
        q.sid = reinterpret_cast<int32_t*>(sb + sl.sid_at);
        q.next = reinterpret_cast<int32_t*>(sb + sl.next_at);
        q.ringno = reinterpret_cast<uint32_t*>(sb + sl.ringno_at);
        q.flag = reinterpret_cast<uint8_t*>(sb + sl.flag_at);
        q.jflag = reinterpret_cast<uint8_t*>(sb + sl.jflag_at);
        q.jidx = reinterpret_cast<uint32_t*>(sb + sl.jidx_at);
        q.side_sums = reinterpret_cast<uint2*>(sb + sl.sums_at);
        q.jump[0] = reinterpret_cast<OutlineJump*>(sb + sl.jump_at[0]);
        q.jump[1] = reinterpret_cast<OutlineJump*>(sb + sl.jump_at[1]);
        // where the per-side result ends up, and the buffer that is dead by then (mrtx_outline.h)
        const int fin_at = (q.rounds & 1) ^ (contract ? 1 : 0);
        q.fin = q.jump[fin_at];
        HIPCHK(c, mrtx_launch_outline_trace(q, c->stream, &launches));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
        if (head[0] >> 32) {
            CHK(stage_finish(c, nullptr, nullptr, 0, out, kNoRays));
            return fail(c, MRTX_E_DEVICE, "the outline trace met %u broken successors or chains", (uint32_t)(head[0] >> 32));
        }
        rings = head[4]; vertices = head[5];
        fits = rings <= ring_cap && vertices <= vertex_cap;
        if (has_rings && fits) {
            // a table bound for the host lies in the jump buffer that the trace left dead
            char* dead = sb + sl.jump_at[fin_at ^ 1];
            q.rings = out_table<RingRec>(host_rings, dead, dev_rings);
            q.vertices = out_table<int32_t>(host_vertices, dead + outline_host_vertices_at(rings), dev_vertices);
            HIPCHK(c, mrtx_launch_outline_fill(q, rings, c->stream, &launches));
        }
    }
    CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
    if (has_rings && fits && q.B) {                             // the fill's own check of what the trace handed it
        HIPCHK(c, hipMemcpy(head, tb, 8, hipMemcpyDeviceToHost));
        if (head[0] >> 32) return fail(c, MRTX_E_DEVICE, "the outline fill met %u sides without a ring", (uint32_t)(head[0] >> 32));
    }
    *n_rings = rings;
    *n_vertices = vertices;
    if (has_rings && !fits) return tables_too_small(c, tabs, rings, vertices);
    if (host_rings && rings) HIPCHK(c, hipMemcpy(host_rings, q.rings, sizeof(MrtxRing) * (size_t)rings, hipMemcpyDeviceToHost));
    if (host_vertices && vertices) HIPCHK(c, hipMemcpy(host_vertices, q.vertices, 8 * (size_t)vertices, hipMemcpyDeviceToHost));
    return MRTX_OK;
}

// ---- Contour lines: the ordered isolines of a lattice at many levels ------------------------------
static_assert(sizeof(MrtxContours) == 20, "MrtxContours is 20 bytes");
static_assert(sizeof(MrtxContourLine) == 32 && alignof(MrtxContourLine) == 8 && sizeof(ContourLineRec) == sizeof(MrtxContourLine),
              "MrtxContourLine is 32 bytes");
static_assert(sizeof(ContourJump) == 16, "one int4");
static_assert(MRTX_CT_VOID == MRTX_FILL_NONE, "one mark for a node without a height");

int mrtx_contours(mrtx_ctx* c, const MrtxContours* k, const void* dev_z, const int32_t* host_z, const int32_t* host_levels,
                  void* dev_lines, MrtxContourLine* host_lines, uint64_t line_cap, void* dev_vertices, int32_t* host_vertices,
                  uint64_t vertex_cap, uint64_t* n_lines, uint64_t* n_vertices, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!k) return fail(c, MRTX_E_INVALID, "null contours block");
    if (k->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, k->rows, k->cols, k->wrap));
    if ((int64_t)k->rows * (int64_t)k->cols > MRTX_CT_MAX_NODES)
        return fail(c, MRTX_E_INVALID, "a contoured lattice holds at most 2^28 nodes (got %d x %d)", k->rows, k->cols);
    if (k->n_levels < 1 || k->n_levels > MRTX_CT_MAX_LEVELS) return fail(c, MRTX_E_INVALID, "n_levels must lie in 1 .. 65536 (got %d)", k->n_levels);
    if (!host_levels) return fail(c, MRTX_E_INVALID, "null host_levels");
    for (int32_t l = 0; l < k->n_levels; l++) {
        if (host_levels[l] < -MRTX_CT_ZMAX + 1 || host_levels[l] > MRTX_CT_ZMAX)
            return fail(c, MRTX_E_INVALID, "level %d must lie in -2^30 + 1 .. 2^30 (got %d)", l, host_levels[l]);
        if (l && host_levels[l] <= host_levels[l - 1])
            return fail(c, MRTX_E_INVALID, "the levels must ascend strictly (level %d = %d follows %d)", l, host_levels[l], host_levels[l - 1]);
    }
    CHK(one_of(c, dev_z, host_z, "z"));
    const TraceTables tabs = {"line", "lines", dev_lines, host_lines, line_cap, dev_vertices, host_vertices, vertex_cap, n_lines, n_vertices};
    bool has_lines;
    CHK(trace_tables(c, tabs, &has_lines));
    const size_t N = (size_t)k->rows * (size_t)k->cols;
    // a table never needs more than one line and one vertex per element, and there are fewer than 2^31 elements
    const size_t line_bytes = sizeof(MrtxContourLine) * (size_t)std::min<uint64_t>(line_cap, (uint64_t)1 << 31);
    const size_t vertex_bytes = 4 * (size_t)std::min<uint64_t>(vertex_cap, (uint64_t)1 << 31);
    CHK(aligned(c, dev_z, 4, "dev_z", "int32"));
    CHK(aligned(c, dev_lines, 8, "dev_lines", "MrtxContourLine"));
    CHK(aligned(c, dev_vertices, 4, "dev_vertices", "int32"));
    if (!disjoint({{dev_z, 4 * N}, {dev_lines, line_bytes}, {dev_vertices, vertex_bytes}}))
        return fail(c, MRTX_E_INVALID, "dev_z, dev_lines and dev_vertices must not overlap");
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const ContourNodeLayout nl = contour_node_layout(k->rows, k->cols, k->n_levels, host_z != nullptr);
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, nl.end));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    // the host tables (the caller's memory stays put until the end of the call)
    HIPCHK(c, hipMemcpyAsync(tb + nl.levels_at, host_levels, 4 * (size_t)k->n_levels, hipMemcpyHostToDevice, c->stream));
    if (host_z) HIPCHK(c, hipMemcpyAsync(tb + nl.z_at, host_z, 4 * N, hipMemcpyHostToDevice, c->stream));
    ContourC q;
    std::memset(&q, 0, sizeof q);
    q.z = in_table<int32_t>(host_z, tb + nl.z_at, dev_z);
    q.levels = reinterpret_cast<const int32_t*>(tb + nl.levels_at);
    q.bad = reinterpret_cast<uint32_t*>(tb);
    q.totals = reinterpret_cast<unsigned long long*>(tb + 16);
    q.rank = reinterpret_cast<uint32_t*>(tb + nl.rank_at);
    q.base = reinterpret_cast<uint32_t*>(tb + nl.base_at);
    q.node_sums = reinterpret_cast<unsigned long long*>(tb + nl.sums_at);
    q.rows = k->rows; q.cols = k->cols; q.wrap = k->wrap; q.n_levels = k->n_levels;
    uint32_t launches = 0;
    unsigned long long head[6] = {0, 0, 0, 0, 0, 0};            // bad (and padding), then the four totals
    HIPCHK(c, hipMemsetAsync(tb, 0, 64, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_contour_count(q, c->stream, &launches));
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // also: the pageable tables are no longer read
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    if ((uint32_t)head[0] || head[2] >= ((uint64_t)1 << 31)) {  // as the sibling calls: the stage ends, out says what ran
        CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
        if ((uint32_t)head[0])
            return fail(c, MRTX_E_INVALID, "%u heights lie outside -2^30 .. 2^30 and are not MRTX_FILL_NONE", (uint32_t)head[0]);
        return fail(c, MRTX_E_INVALID, "the levels cross the edges %llu times: a call holds fewer than 2^31 crossings", head[2]);
    }
    q.B = (uint32_t)head[2];
    q.rounds = contour_rounds(q.B);
    uint64_t lines = 0, vertices = 0;
    bool fits = true;
    if (q.B) {
        const ContourSideLayout sl = contour_side_layout(q.B);
        CHK(stage_buffer(c, c->illum_out, c->illum_out_bytes, sl.end));
        char* sb = reinterpret_cast<char*>(c->illum_out);
        q.eid = reinterpret_cast<int32_t*>(sb + sl.eid_at);
        q.succ = reinterpret_cast<int32_t*>(sb + sl.succ_at);
        q.len = reinterpret_cast<uint32_t*>(sb + sl.len_at);
        q.tailat = reinterpret_cast<int32_t*>(sb + sl.tailat_at);
        q.lineno = reinterpret_cast<uint32_t*>(sb + sl.lineno_at);
        q.side_sums = reinterpret_cast<uint2*>(sb + sl.sums_at);
        q.jump[0] = reinterpret_cast<ContourJump*>(sb + sl.jump_at[0]);
        q.jump[1] = reinterpret_cast<ContourJump*>(sb + sl.jump_at[1]);
        q.fin = q.jump[q.rounds & 1];
        HIPCHK(c, mrtx_launch_contour_trace(q, c->stream, &launches));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
        if ((head[0] >> 32) || head[5] != q.B) {                // the lines' lengths add up to the elements
            CHK(stage_finish(c, nullptr, nullptr, 0, out, kNoRays));
            return fail(c, MRTX_E_DEVICE, "the contour trace met %u broken successors and lines of %llu vertices for %u crossings",
                        (uint32_t)(head[0] >> 32), head[5], q.B);
        }
        lines = head[4]; vertices = head[5];
        fits = lines <= line_cap && vertices <= vertex_cap;
        if (has_lines && fits) {
            // the tables bound for the host lie in a block of their own, of exactly their size
            if (host_lines || host_vertices)
                CHK(stage_buffer(c, c->illum_tab, c->illum_tab_bytes, contour_host_vertices_at(lines) + 4 * (size_t)vertices));
            char* hb = reinterpret_cast<char*>(c->illum_tab);
            q.lines = out_table<ContourLineRec>(host_lines, hb, dev_lines);
            q.vertices = out_table<int32_t>(host_vertices, hb + contour_host_vertices_at(lines), dev_vertices);
            HIPCHK(c, mrtx_launch_contour_fill(q, lines, c->stream, &launches));
        }
    }
    CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
    if (has_lines && fits && q.B) {                             // the fill's own check of what the trace handed it
        HIPCHK(c, hipMemcpy(head, tb, 8, hipMemcpyDeviceToHost));
        if (head[0] >> 32) return fail(c, MRTX_E_DEVICE, "the contour fill met %u elements without a line", (uint32_t)(head[0] >> 32));
    }
    *n_lines = lines;
    *n_vertices = vertices;
    if (has_lines && !fits) return tables_too_small(c, tabs, lines, vertices);
    if (host_lines && lines) HIPCHK(c, hipMemcpy(host_lines, q.lines, sizeof(MrtxContourLine) * (size_t)lines, hipMemcpyDeviceToHost));
    if (host_vertices && vertices) HIPCHK(c, hipMemcpy(host_vertices, q.vertices, 4 * (size_t)vertices, hipMemcpyDeviceToHost));
    return MRTX_OK;
}

// ---- Terrain depressions: fill levels and the basin catalogue -------------------------------------
static_assert(sizeof(MrtxFill) == 24, "MrtxFill is 24 bytes");
static_assert(sizeof(MrtxBasin) == 48 && sizeof(BasinRec) == sizeof(MrtxBasin), "MrtxBasin is 48 bytes");
static_assert(MRTX_FILL_NONE == INT32_MAX, "the fill without an outlet");

// a host height table is refused at its first height beyond the bound (a device table's are counted by the kernels)
static int fill_host_heights(mrtx_ctx* c, const int32_t* host_z, size_t N) {
    if (host_z)
        for (size_t n = 0; n < N; n++)
            if (host_z[n] < -MRTX_FILL_ZMAX || host_z[n] > MRTX_FILL_ZMAX)
                return fail(c, MRTX_E_INVALID, "height %zu must lie in -2^30 .. 2^30 (got %d)", n, host_z[n]);
    return MRTX_OK;
}

int mrtx_fill(mrtx_ctx* c, const MrtxFill* f, const void* dev_z, const int32_t* host_z, const void* dev_outlet,
              const uint8_t* host_outlet, void* dev_fill, int32_t* host_fill, uint64_t* visits, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!f) return fail(c, MRTX_E_INVALID, "null fill block");
    if (f->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, f->rows, f->cols, f->wrap));
    CHK(connectivity_ok(c, f->connectivity));
    if (f->edge_outlets != 0 && f->edge_outlets != 1) return fail(c, MRTX_E_INVALID, "edge_outlets must be 0 or 1 (got %d)", f->edge_outlets);
    CHK(at_most_one(c, dev_outlet, host_outlet, "outlet"));
    if (!f->edge_outlets && !dev_outlet && !host_outlet)
        return fail(c, MRTX_E_INVALID, "no outlet source: edge_outlets = 0 needs an outlet table");
    CHK(one_of(c, dev_z, host_z, "z"));
    CHK(one_of(c, dev_fill, host_fill, "fill"));
    CHK(aligned(c, dev_z, 4, "dev_z", "int32"));
    CHK(aligned(c, dev_fill, 4, "dev_fill", "int32"));
    const size_t N = (size_t)f->rows * (size_t)f->cols;
    if (!disjoint({{dev_z, 4 * N}, {dev_outlet, N}, {dev_fill, 4 * N}}))
        return fail(c, MRTX_E_INVALID, "dev_z, dev_outlet and dev_fill must not overlap");
    // MOONRT_FILL=sweep: one Jacobi step over the whole lattice per launch, the yardstick of the tile scheme; the same bytes
    bool tiles = true;
    CHK(variant(c, "MOONRT_FILL", "tiles", "sweep", &tiles));
    CHK(fill_host_heights(c, host_z, N));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int tiles_x = (f->cols + MRTX_FILL_TS - 1) / MRTX_FILL_TS, tiles_y = (f->rows + MRTX_FILL_TS - 1) / MRTX_FILL_TS;
    const size_t n_tiles = (size_t)tiles_x * (size_t)tiles_y;
    // scratch: 64 bytes of counters (visits, bad, the change counters), the fill when it goes to the host, then the second
    // table of the sweep or the two flag arrays of the tiles
    const size_t tab_b = (4 * N + 15) & ~(size_t)15;
    const size_t fill_at = 64, work_at = fill_at + (host_fill ? tab_b : 0);
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, work_at + (tiles ? 8 * n_tiles : tab_b)));
    // the host tables: heights, then the outlet bytes (the caller's memory stays put until the end of the call)
    const size_t hz_b = host_z ? tab_b : 0;
    if (host_z || host_outlet) {
        CHK(stage_buffer(c, c->illum_tab, c->illum_tab_bytes, hz_b + (host_outlet ? N : 0) + 16));
        char* it = reinterpret_cast<char*>(c->illum_tab);
        if (host_z) HIPCHK(c, hipMemcpyAsync(it, host_z, 4 * N, hipMemcpyHostToDevice, c->stream));
        if (host_outlet) HIPCHK(c, hipMemcpyAsync(it + hz_b, host_outlet, N, hipMemcpyHostToDevice, c->stream));
    }
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    FillC q;
    std::memset(&q, 0, sizeof q);
    q.z = in_table<int32_t>(host_z, c->illum_tab, dev_z);
    q.outlet = in_table<uint8_t>(host_outlet, reinterpret_cast<const char*>(c->illum_tab) + hz_b, dev_outlet);
    int32_t* const d_fill = out_table<int32_t>(host_fill, tb + fill_at, dev_fill);
    int32_t* const d_other = reinterpret_cast<int32_t*>(tb + work_at);      // sweep only
    q.visits = reinterpret_cast<unsigned long long*>(tb);
    q.bad = reinterpret_cast<uint32_t*>(tb + 8);
    q.changed = reinterpret_cast<uint32_t*>(tb + 16);
    q.rows = f->rows; q.cols = f->cols; q.wrap = f->wrap; q.conn8 = f->connectivity == 8; q.edge_outlets = f->edge_outlets;
    q.tiles_x = tiles_x; q.tiles_y = tiles_y;
    uint32_t* fa = reinterpret_cast<uint32_t*>(tb + work_at);
    uint32_t* fb = fa + n_tiles;
    HIPCHK(c, hipMemsetAsync(tb, 0, 64, c->stream));
    if (tiles) HIPCHK(c, hipMemsetAsync(fa, 0, 8 * n_tiles, c->stream));
    CHK(stage_start(c, nullptr, false));
    q.w = d_fill;
    if (tiles) q.flag_in = fa;
    HIPCHK(c, mrtx_launch_fill_init(q, tiles, c->stream));
    // no launch cap: every store strictly lowers an int32, so the fixed point is reached after finitely many of them.  The
    // sweep reads one table and writes the other; a batch is an even number of launches, so it ends in the caller's table.
    static_assert(MRTX_FILL_BATCH % 2 == 0, "a batch of sweeps ends in the table it started from");
    uint32_t launches = 1;
    for (;;) {
        HIPCHK(c, hipMemsetAsync(q.changed, 0, MRTX_FILL_BATCH * sizeof(uint32_t), c->stream));
        for (int s = 0; s < MRTX_FILL_BATCH; s++) {
            q.slot = s;
            if (tiles) {
                q.flag_in = fa; q.flag_out = fb;
                HIPCHK(c, mrtx_launch_fill_relax(q, c->stream));
                std::swap(fa, fb);
            } else {
                q.w_in = (s & 1) ? d_other : d_fill;
                q.w = (s & 1) ? d_fill : d_other;
                HIPCHK(c, mrtx_launch_fill_sweep(q, c->stream));
            }
            launches++;
        }
        uint32_t last = 0;
        HIPCHK(c, hipMemcpyAsync(&last, q.changed + (MRTX_FILL_BATCH - 1), sizeof last, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (last == 0) break;       // a whole launch lowered nothing: every later one is empty too
    }
    float ms = 0.0f;
    CHK(lap(c, &ms));
    unsigned long long head[2] = {0, 0};                    // visits, bad
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    report(out, ms, launches);
    if (visits) *visits = head[0];
    if ((uint32_t)head[1])
        return fail(c, MRTX_E_INVALID, "%u heights of the device table lie outside -2^30 .. 2^30", (uint32_t)head[1]);
    if (host_fill) HIPCHK(c, hipMemcpy(host_fill, d_fill, 4 * N, hipMemcpyDeviceToHost));
    return MRTX_OK;
}

int mrtx_fill_basins(mrtx_ctx* c, int32_t rows, int32_t cols, int32_t wrap, int32_t connectivity, const void* dev_labels,
                     const int32_t* host_labels, uint32_t n_regions, const void* dev_z, const int32_t* host_z, const void* dev_fill,
                     const int32_t* host_fill, const uint32_t* row_weight, void* dev_out, MrtxBasin* host_out, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    CHK(lattice_ok(c, rows, cols, wrap));
    CHK(connectivity_ok(c, connectivity));
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    CHK(one_of(c, dev_z, host_z, "z"));
    CHK(one_of(c, dev_fill, host_fill, "fill"));
    CHK(one_of(c, dev_out, host_out, "out"));
    const size_t N = (size_t)rows * (size_t)cols;
    CHK(regions_fit(c, n_regions, N));
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_z, 4, "dev_z", "int32"));
    CHK(aligned(c, dev_fill, 4, "dev_fill", "int32"));
    CHK(aligned(c, dev_out, 8, "dev_out", "MrtxBasin"));
    const size_t out_bytes = sizeof(MrtxBasin) * (size_t)n_regions;
    if (!disjoint({{dev_labels, 4 * N}, {dev_z, 4 * N}, {dev_fill, 4 * N}, {dev_out, out_bytes}}, 3))      // three inputs
        return fail(c, MRTX_E_INVALID, "the device inputs and dev_out must not overlap");
    CHK(fill_host_heights(c, host_z, N));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // scratch: the counts of bad entries, then the packed pour and depth keys
    float* d[4] = {nullptr, nullptr, nullptr, nullptr};
    CHK(stage_out(c, dev_out, std::max(out_bytes, sizeof(MrtxBasin))));
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, 16 + 16 * (size_t)n_regions));
    CHK(stage_tables(c, {{host_labels, host_labels ? N : 0}, {host_z, host_z ? N : 0}, {host_fill, host_fill ? N : 0},
                         {row_weight, row_weight ? (size_t)rows : 0}}, d));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    BasinC q;
    std::memset(&q, 0, sizeof q);
    q.labels = in_table<int32_t>(host_labels, d[0], dev_labels);
    q.z = in_table<int32_t>(host_z, d[1], dev_z);
    q.fill = in_table<int32_t>(host_fill, d[2], dev_fill);
    q.row_weight = in_table<uint32_t>(row_weight, d[3], nullptr);
    q.out = static_cast<BasinRec*>(dev_out);
    q.bad = reinterpret_cast<uint32_t*>(tb);
    q.keys = reinterpret_cast<unsigned long long*>(tb + 16);
    q.rows = rows; q.cols = cols; q.wrap = wrap; q.conn8 = connectivity == 8; q.n_regions = n_regions;
    uint32_t launches = 0, bad[2] = {0, 0};
    HIPCHK(c, hipMemsetAsync(q.bad, 0, 16, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_fill_basins(q, c->stream, &launches));
    CHK(lattice_finish(c, dev_out, reinterpret_cast<float*>(host_out), out_bytes, out, launches));
    HIPCHK(c, hipMemcpy(bad, q.bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0]) return label_refusal(c, bad[0], n_regions);
    if (bad[1]) return fail(c, MRTX_E_INVALID, "%u heights of the device table lie outside -2^30 .. 2^30", bad[1]);
    return MRTX_OK;
}

// ---- The depression hierarchy: nested bowls, spill points, peak prominence ------------------------
static_assert(sizeof(MrtxBowls) == 32, "MrtxBowls is 32 bytes");
static_assert(sizeof(MrtxBowl) == 64 && alignof(MrtxBowl) == 8, "MrtxBowl is 64 bytes");
static_assert(sizeof(BowlEdge) == 16 && sizeof(BowlWalk) == 16, "the tables the host and the kernels share");
static_assert(MRTX_BOWLS_ZMAX == MRTX_FILL_ZMAX, "one bound on the heights");

static int32_t bowls_level(unsigned long long key) { return (int32_t)((uint32_t)(key >> 32) - 0x40000000u); }

// The sweep over the minima and the edges of the spanning forest, both in ascending key: the births, spills, parents and floors
// of section 3.25.  The edges of one pass node are one event.  Levels are still those the sweep saw (negated with invert), and
// count, weight, volume and n_leaves wait for the sums of the label pass (bowls_finish).  floor: the key of each bowl's floor.
static void bowls_tree(std::vector<unsigned long long>& minima, std::vector<BowlEdge>& edges, uint32_t outside,
                       std::vector<MrtxBowl>& rec, std::vector<BowlWalk>& walk) {
    const size_t M = minima.size();
    std::sort(minima.begin(), minima.end());
    std::sort(edges.begin(), edges.end(), [](const BowlEdge& x, const BowlEdge& y) { return x.pass < y.pass; });
    std::vector<uint32_t> ids(M);
    for (size_t k = 0; k < M; k++) ids[k] = (uint32_t)minima[k];
    std::sort(ids.begin(), ids.end());
    auto dense = [&](uint32_t node) -> uint32_t {
        return node == outside ? (uint32_t)M : (uint32_t)(std::lower_bound(ids.begin(), ids.end(), node) - ids.begin());
    };
    std::vector<uint32_t> up(M + 1);
    for (size_t k = 0; k <= M; k++) up[k] = (uint32_t)k;
    auto find = [&](uint32_t x) {
        while (up[x] != x) {
            up[x] = up[up[x]];
            x = up[x];
        }
        return x;
    };
    std::vector<int32_t> current(M + 1, -1);        // the current bowl of a component's representative; -1: open
    std::vector<unsigned long long> floor;
    auto born = [&](unsigned long long key, uint32_t children, unsigned long long floor_key, bool leaf) {
        MrtxBowl b;
        std::memset(&b, 0, sizeof b);
        b.born_at = (int32_t)(uint32_t)key; b.born_level = bowls_level(key);
        b.floor_at = (int32_t)(uint32_t)floor_key; b.floor_level = bowls_level(floor_key);
        b.spill_at = -1; b.spill_level = MRTX_FILL_NONE; b.parent = -1; b.n_children = children; b.n_leaves = leaf ? 1u : 0u;
        rec.push_back(b);
        floor.push_back(floor_key);
        BowlWalk w;
        w.spill = ~0ull; w.parent = -1; w.leaf_at = leaf ? b.born_at : -1;
        walk.push_back(w);
        return (int32_t)(rec.size() - 1);
    };
    auto spill = [&](int32_t b, unsigned long long key, int32_t parent) {
        rec[b].spill_at = (int32_t)(uint32_t)key; rec[b].spill_level = bowls_level(key); rec[b].parent = parent;
        walk[b].spill = key; walk[b].parent = parent;
    };
    size_t im = 0, ie = 0;
    std::vector<uint32_t> cs;
    while (im < M || ie < edges.size()) {
        if (im < M && (ie >= edges.size() || minima[im] < edges[ie].pass)) {
            current[dense((uint32_t)minima[im])] = born(minima[im], 0, minima[im], true);
            im++;
            continue;
        }
        const unsigned long long pass = edges[ie].pass;
        cs.clear();
        for (; ie < edges.size() && edges[ie].pass == pass; ie++)
            for (uint32_t end : {edges[ie].a, edges[ie].b}) {
                const uint32_t r = find(dense(end));
                if (std::find(cs.begin(), cs.end(), r) == cs.end()) cs.push_back(r);
            }
        bool open = false;
        uint32_t to = cs[0];
        for (uint32_t r : cs)
            if (current[r] < 0) { open = true; to = r; }
        int32_t now = -1;
        if (!open) {
            unsigned long long least = ~0ull;
            for (uint32_t r : cs) least = std::min(least, floor[current[r]]);
            now = born(pass, (uint32_t)cs.size(), least, false);
        }
        for (uint32_t r : cs) {
            if (current[r] >= 0) spill(current[r], pass, now);
            up[r] = to;
        }
        current[to] = now;
    }
}

// One pass up the records (parent > child): the sums of each bowl's own nodes become those of its region.  own: nodes, weight
// and the sum of w z' per bowl.  Then the levels go back into the caller's z.
static void bowls_finish(std::vector<MrtxBowl>& rec, std::vector<unsigned long long>& own, bool invert) {
    const size_t n = rec.size();
    for (size_t b = 0; b < n; b++) rec[b].own_count = (uint32_t)own[3 * b];
    for (size_t b = 0; b < n; b++) {
        MrtxBowl& r = rec[b];
        r.count = (uint32_t)own[3 * b];
        r.weight = own[3 * b + 1];
        r.volume = r.spill_at >= 0 ? (unsigned long long)(long long)r.spill_level * r.weight - own[3 * b + 2] : 0ull;
        if (r.parent >= 0) {
            const size_t p = (size_t)r.parent;
            for (int k = 0; k < 3; k++) own[3 * p + k] += own[3 * b + k];
            rec[p].n_leaves += r.n_leaves;
        }
        if (invert) { r.floor_level = -r.floor_level; r.born_level = -r.born_level; r.spill_level = -r.spill_level; }
    }
}

int mrtx_bowls(mrtx_ctx* c, const MrtxBowls* w, const void* dev_z, const int32_t* host_z, const void* dev_outlet,
               const uint8_t* host_outlet, const uint32_t* row_weight, void* dev_bowls, MrtxBowl* host_bowls, uint64_t bowl_cap,
               void* dev_label, int32_t* host_label, uint64_t* n_bowls, uint64_t* rounds, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!w) return fail(c, MRTX_E_INVALID, "null bowls block");
    if (w->reserved[0] != 0 || w->reserved[1] != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, w->rows, w->cols, w->wrap));
    CHK(connectivity_ok(c, w->connectivity));
    if (w->edge_outlets != 0 && w->edge_outlets != 1) return fail(c, MRTX_E_INVALID, "edge_outlets must be 0 or 1 (got %d)", w->edge_outlets);
    if (w->invert != 0 && w->invert != 1) return fail(c, MRTX_E_INVALID, "invert must be 0 or 1 (got %d)", w->invert);
    CHK(at_most_one(c, dev_outlet, host_outlet, "outlet"));
    if (!w->edge_outlets && !dev_outlet && !host_outlet)
        return fail(c, MRTX_E_INVALID, "no outlet source: edge_outlets = 0 needs an outlet table");
    CHK(one_of(c, dev_z, host_z, "z"));
    if (!n_bowls) return fail(c, MRTX_E_INVALID, "null n_bowls");
    CHK(at_most_one(c, dev_bowls, host_bowls, "bowls"));
    CHK(at_most_one(c, dev_label, host_label, "label"));
    const bool has_bowls = dev_bowls || host_bowls, has_label = dev_label || host_label;
    if (!has_bowls && bowl_cap) return fail(c, MRTX_E_INVALID, "without a bowl table bowl_cap must be 0 (got %llu)", (unsigned long long)bowl_cap);
    if (!has_bowls && has_label) return fail(c, MRTX_E_INVALID, "a label table needs a bowl table: a call without one only counts");
    const size_t N = (size_t)w->rows * (size_t)w->cols;
    CHK(aligned(c, dev_z, 4, "dev_z", "int32"));
    CHK(aligned(c, dev_bowls, 8, "dev_bowls", "MrtxBowl"));
    CHK(aligned(c, dev_label, 4, "dev_label", "int32"));
    // a lattice never holds more bowls than nodes
    const size_t bowl_bytes = sizeof(MrtxBowl) * (size_t)std::min<uint64_t>(bowl_cap, N);
    if (!disjoint({{dev_z, 4 * N}, {dev_outlet, N}, {dev_bowls, bowl_bytes}, {dev_label, 4 * N}}))
        return fail(c, MRTX_E_INVALID, "dev_z, dev_outlet, dev_bowls and dev_label must not overlap");
    CHK(fill_host_heights(c, host_z, N));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // scratch: 64 bytes of counters, then ptr, cpar and best2 (N + 1 words each), best (N + 1 double words), and the labels
    // when they go to the host
    const size_t words_b = (4 * (N + 1) + 15) & ~(size_t)15, keys_b = (8 * (N + 1) + 15) & ~(size_t)15;
    const size_t ptr_at = 64, cpar_at = ptr_at + words_b, best2_at = cpar_at + words_b, best_at = best2_at + words_b,
                 label_at = best_at + keys_b;
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, label_at + (host_label ? 4 * N : 0)));
    // the host tables: heights, the row weights, then the outlet bytes (the caller's memory stays put until the first wait)
    const size_t hz_b = host_z ? (4 * N + 15) & ~(size_t)15 : 0, rw_b = row_weight ? (4 * (size_t)w->rows + 15) & ~(size_t)15 : 0;
    CHK(stage_buffer(c, c->illum_tab, c->illum_tab_bytes, hz_b + rw_b + (host_outlet ? N : 0) + 16));
    char* it = reinterpret_cast<char*>(c->illum_tab);
    if (host_z) HIPCHK(c, hipMemcpyAsync(it, host_z, 4 * N, hipMemcpyHostToDevice, c->stream));
    if (row_weight) HIPCHK(c, hipMemcpyAsync(it + hz_b, row_weight, 4 * (size_t)w->rows, hipMemcpyHostToDevice, c->stream));
    if (host_outlet) HIPCHK(c, hipMemcpyAsync(it + hz_b + rw_b, host_outlet, N, hipMemcpyHostToDevice, c->stream));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    BowlC q;
    std::memset(&q, 0, sizeof q);
    q.z = in_table<int32_t>(host_z, it, dev_z);
    q.row_weight = in_table<uint32_t>(row_weight, it + hz_b, nullptr);
    q.outlet = in_table<uint8_t>(host_outlet, it + hz_b + rw_b, dev_outlet);
    q.counters = reinterpret_cast<uint32_t*>(tb);
    q.ptr = reinterpret_cast<uint32_t*>(tb + ptr_at);
    q.cpar = reinterpret_cast<uint32_t*>(tb + cpar_at);
    q.best2 = reinterpret_cast<uint32_t*>(tb + best2_at);
    q.best = reinterpret_cast<unsigned long long*>(tb + best_at);
    q.rows = w->rows; q.cols = w->cols; q.wrap = w->wrap; q.conn8 = w->connectivity == 8; q.edge_outlets = w->edge_outlets;
    q.invert = w->invert;
    static_assert(8 + MRTX_BOWLS_BATCH <= 16, "the counters fit their 64 bytes");
    HIPCHK(c, hipMemsetAsync(tb, 0, 64, c->stream));
    CHK(stage_start(c, nullptr, false));
    float ms = 0.0f;
    uint32_t launches = 1, head[16];
    HIPCHK(c, mrtx_launch_bowls_init(q, c->stream));
    // the jumps: a path of L nodes is short of its end after log2 L doublings, and a launch that moved nothing ends them
    for (;;) {
        HIPCHK(c, hipMemsetAsync(q.counters + 8, 0, MRTX_BOWLS_BATCH * sizeof(uint32_t), c->stream));
        for (int s = 0; s < MRTX_BOWLS_BATCH; s++) {
            q.slot = s;
            HIPCHK(c, mrtx_launch_bowls_jump(q, c->stream));
            launches++;
        }
        uint32_t last = 0;
        HIPCHK(c, hipMemcpyAsync(&last, q.counters + 8 + (MRTX_BOWLS_BATCH - 1), sizeof last, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (last == 0) break;
    }
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    if (head[0]) {
        CHK(lap(c, &ms));
        report(out, ms, launches);
        return fail(c, MRTX_E_INVALID, "%u heights of the device table lie outside -2^30 .. 2^30", head[0]);
    }
    // ---- the spanning forest over the catchments and the outside
    const uint32_t M = head[1];
    q.n_min = M;
    uint64_t n_rounds = 0;
    std::vector<unsigned long long> minima(M);
    std::vector<BowlEdge> edges;
    // the component tables: the minima's keys, the hooks and the edges; the walk table and the sums of the label pass take
    // their place later (at most 2 M bowls of 16 + 24 bytes)
    const size_t list_b = (8 * ((size_t)M + 1) + 15) & ~(size_t)15, hook_b = (4 * ((size_t)M + 1) + 15) & ~(size_t)15;
    if (M) {
        CHK(stage_buffer(c, c->illum_out, c->illum_out_bytes, std::max(list_b + hook_b + 16 * ((size_t)M + 1), 80 * (size_t)M + 64)));
        char* ob = reinterpret_cast<char*>(c->illum_out);
        q.list = reinterpret_cast<unsigned long long*>(ob);
        q.hook = reinterpret_cast<uint32_t*>(ob + list_b);
        q.edges = reinterpret_cast<BowlEdge*>(ob + list_b + hook_b);
        HIPCHK(c, mrtx_launch_bowls_list(q, c->stream));
        launches++;
        uint32_t n_edges = 0;
        for (;;) {                                              // a round halves the components that still have a cross edge
            HIPCHK(c, mrtx_launch_bowls_round(q, c->stream, &launches));
            HIPCHK(c, hipMemcpyAsync(head, tb, sizeof head, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (head[2] == n_edges) break;                      // nothing hooked: no component has a cross edge left
            n_edges = head[2];
            n_rounds++;
        }
        CHK(lap(c, &ms));
        if (head[3] != M || head[4] || n_edges > M) {
            report(out, ms, launches);
            return fail(c, MRTX_E_DEVICE, "the bowl stage listed %u of %u minima and chose %u edges", head[3], M, n_edges);
        }
        edges.resize(n_edges);
        HIPCHK(c, hipMemcpy(minima.data(), q.list, 8 * (size_t)M, hipMemcpyDeviceToHost));
        if (n_edges) HIPCHK(c, hipMemcpy(edges.data(), q.edges, sizeof(BowlEdge) * (size_t)n_edges, hipMemcpyDeviceToHost));
    } else {
        CHK(lap(c, &ms));
    }
    // ---- the host's share: proportional to the minima
    std::vector<MrtxBowl> rec;
    std::vector<BowlWalk> walk;
    bowls_tree(minima, edges, (uint32_t)N, rec, walk);
    const uint64_t total = rec.size();
    if (!has_bowls || total > bowl_cap) {
        report(out, ms, launches);
        *n_bowls = total;
        if (rounds) *rounds = n_rounds;
        if (has_bowls)
            return fail(c, MRTX_E_INVALID, "the bowl table is too small: %llu bowls are needed (bowl_cap = %llu)", (unsigned long long)total,
                        (unsigned long long)bowl_cap);
        return MRTX_OK;
    }
    // ---- the labels and the sums of each bowl's own nodes
    q.n_bowls = (uint32_t)total;
    q.label = out_table<int32_t>(host_label, tb + label_at, dev_label);
    std::vector<unsigned long long> own(3 * (size_t)total, 0ull);
    if (total || has_label) {
        if (total) {
            char* ob = reinterpret_cast<char*>(c->illum_out);
            q.walk = reinterpret_cast<const BowlWalk*>(ob);
            q.own = reinterpret_cast<unsigned long long*>(ob + sizeof(BowlWalk) * (size_t)total);
            HIPCHK(c, hipMemcpyAsync(ob, walk.data(), sizeof(BowlWalk) * (size_t)total, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(q.own, 0, 24 * (size_t)total, c->stream));
        }
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        HIPCHK(c, mrtx_launch_bowls_label(q, c->stream, &launches));
        CHK(lap(c, &ms));
        if (total) HIPCHK(c, hipMemcpy(own.data(), q.own, 24 * (size_t)total, hipMemcpyDeviceToHost));
    }
    bowls_finish(rec, own, w->invert != 0);
    report(out, ms, launches);
    *n_bowls = total;
    if (rounds) *rounds = n_rounds;
    if (total) {
        if (host_bowls) std::memcpy(host_bowls, rec.data(), sizeof(MrtxBowl) * (size_t)total);
        else HIPCHK(c, hipMemcpy(dev_bowls, rec.data(), sizeof(MrtxBowl) * (size_t)total, hipMemcpyHostToDevice));
    }
    if (host_label) HIPCHK(c, hipMemcpy(host_label, q.label, 4 * N, hipMemcpyDeviceToHost));
    return MRTX_OK;
}

// ---- Polygon rasterisation: rings and outlines burnt into a label table ---------------------------
static_assert(sizeof(MrtxRaster) == 28, "MrtxRaster is 28 bytes");
static_assert(sizeof(MrtxRasterRing) == 24 && sizeof(RasterRing) == sizeof(MrtxRasterRing), "MrtxRasterRing is 24 bytes");
static_assert(sizeof(MrtxPolygonCover) == 40 && sizeof(CoverRec) == sizeof(MrtxPolygonCover), "MrtxPolygonCover is 40 bytes");

int mrtx_rasterise(mrtx_ctx* c, const MrtxRaster* r, const void* dev_rings, const MrtxRasterRing* host_rings, uint64_t n_rings,
                   const void* dev_vertices, const int32_t* host_vertices, uint64_t n_vertices, uint32_t n_polygons,
                   const uint32_t* row_weight, void* dev_labels, int32_t* host_labels, void* dev_cover, MrtxPolygonCover* host_cover,
                   uint64_t* n_crossings, MrtxStats* out) {
    if (!c) return MRTX_E_INVALID;
    if (!r) return fail(c, MRTX_E_INVALID, "null raster block");
    if (r->reserved != 0) return fail(c, MRTX_E_INVALID, "reserved must be 0");
    CHK(lattice_ok(c, r->rows, r->cols, r->wrap));
    if ((int64_t)r->rows * (int64_t)r->cols > MRTX_RS_MAX_NODES)
        return fail(c, MRTX_E_INVALID, "a rasterised lattice holds at most 2^28 nodes (got %d x %d)", r->rows, r->cols);
    if (r->subcell_bits < 0 || r->subcell_bits > MRTX_RS_MAX_SUBCELL)
        return fail(c, MRTX_E_INVALID, "subcell_bits must lie in 0 .. 8 (got %d)", r->subcell_bits);
    if (r->rule != MRTX_RASTER_NONZERO && r->rule != MRTX_RASTER_EVENODD)
        return fail(c, MRTX_E_INVALID, "rule must be MRTX_RASTER_NONZERO or MRTX_RASTER_EVENODD (got %d)", r->rule);
    if (r->order != MRTX_RASTER_FIRST && r->order != MRTX_RASTER_LAST)
        return fail(c, MRTX_E_INVALID, "order must be MRTX_RASTER_FIRST or MRTX_RASTER_LAST (got %d)", r->order);
    // an empty table may come without a pointer
    if (n_rings) CHK(one_of(c, dev_rings, host_rings, "rings"));
    else CHK(at_most_one(c, dev_rings, host_rings, "rings"));
    if (n_vertices) CHK(one_of(c, dev_vertices, host_vertices, "vertices"));
    else CHK(at_most_one(c, dev_vertices, host_vertices, "vertices"));
    if (n_rings > MRTX_RS_MAX_COUNT || n_vertices > MRTX_RS_MAX_COUNT)
        return fail(c, MRTX_E_INVALID, "a call holds fewer than 2^31 rings and vertices (got %llu, %llu)", (unsigned long long)n_rings,
                    (unsigned long long)n_vertices);
    CHK(one_of(c, dev_labels, host_labels, "labels"));
    if (n_polygons) CHK(one_of(c, dev_cover, host_cover, "cover"));
    else CHK(at_most_one(c, dev_cover, host_cover, "cover"));
    const int32_t strips = raster_strips(r->cols);
    if ((uint64_t)n_polygons * (uint64_t)strips > MRTX_RS_MAX_BINS)
        return fail(c, MRTX_E_INVALID, "a call holds at most 2^28 bins (got %u polygons x %d strips of 64 columns)", n_polygons, strips);
    CHK(aligned(c, dev_rings, 8, "dev_rings", "MrtxRasterRing"));
    CHK(aligned(c, dev_vertices, 4, "dev_vertices", "int32"));
    CHK(aligned(c, dev_labels, 4, "dev_labels", "int32"));
    CHK(aligned(c, dev_cover, 8, "dev_cover", "MrtxPolygonCover"));
    const size_t N = (size_t)r->rows * (size_t)r->cols;
    const size_t ring_bytes = sizeof(MrtxRasterRing) * (size_t)n_rings, vertex_bytes = 8 * (size_t)n_vertices;
    const size_t cover_bytes = sizeof(MrtxPolygonCover) * (size_t)n_polygons;
    if (!disjoint({{dev_rings, ring_bytes}, {dev_vertices, vertex_bytes}, {dev_labels, 4 * N}, {dev_cover, cover_bytes}}, 2))      // two inputs
        return fail(c, MRTX_E_INVALID, "the device inputs, dev_labels and dev_cover must not overlap");
    // MOONRT_RASTER=brute: every node against every edge of every polygon, the yardstick of the binned crossings; the same bytes
    bool bins = true;
    CHK(variant(c, "MOONRT_RASTER", "bins", "brute", &bins));
    // ---- device work from here
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const RasterLayout at = raster_layout(r->rows, r->cols, n_rings, n_polygons, bins, host_labels != nullptr, host_cover != nullptr);
    float* d[3] = {nullptr, nullptr, nullptr};
    CHK(stage_buffer(c, c->trav_buf, c->trav_bytes, at.end));
    CHK(stage_tables(c, {{host_rings, host_rings ? 6 * (size_t)n_rings : 0}, {host_vertices, host_vertices ? 2 * (size_t)n_vertices : 0},
                         {row_weight, row_weight ? (size_t)r->rows : 0}}, d));
    char* tb = reinterpret_cast<char*>(c->trav_buf);
    RasterC q;
    std::memset(&q, 0, sizeof q);
    q.rings = in_table<RasterRing>(host_rings, d[0], dev_rings);
    q.vertices = in_table<int32_t>(host_vertices, d[1], dev_vertices);
    q.row_weight = in_table<uint32_t>(row_weight, d[2], nullptr);
    q.labels = out_table<int32_t>(host_labels, tb + at.labels_at, dev_labels);
    q.cover = out_table<CoverRec>(host_cover, tb + at.cover_at, dev_cover);
    q.head = reinterpret_cast<unsigned long long*>(tb);
    q.edge_off = reinterpret_cast<uint32_t*>(tb + at.edge_at);
    q.bin_off = reinterpret_cast<uint32_t*>(tb + at.bin_at);
    q.poly_off = reinterpret_cast<uint32_t*>(tb + at.poly_at);
    q.order = reinterpret_cast<uint32_t*>(tb + at.order_at);
    q.sums = reinterpret_cast<unsigned long long*>(tb + at.sums_at);
    q.n_rings = n_rings; q.n_vertices = n_vertices; q.n_polygons = n_polygons;
    q.n_bins = bins ? n_polygons * (uint32_t)strips : 0;
    q.rows = r->rows; q.cols = r->cols; q.wrap = r->wrap; q.s = r->subcell_bits; q.evenodd = r->rule == MRTX_RASTER_EVENODD;
    q.last = r->order == MRTX_RASTER_LAST; q.strips = strips; q.bins = bins;
    uint32_t launches = 0;
    unsigned long long head[RS_HEAD] = {0, 0, 0, 0, 0, 0, 0, 0};
    // the counters, the counts per bin or per polygon and the order of the rings start at zero
    HIPCHK(c, hipMemsetAsync(tb, 0, at.sums_at, c->stream));
    CHK(stage_start(c, nullptr, false));
    HIPCHK(c, mrtx_launch_raster_check(q, c->stream, &launches));
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // also: the pageable tables are no longer read
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    if (head[RS_BAD_RINGS] || head[RS_BAD_COORDS] || head[RS_EDGES] > MRTX_RS_MAX_COUNT) {      // the stage ends, out says what ran
        CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
        if (head[RS_BAD_RINGS] || head[RS_BAD_COORDS])
            return fail(c, MRTX_E_INVALID, "the ring table holds %llu bad records and the vertex table %llu coordinates outside -2^24 .. 2^24",
                        head[RS_BAD_RINGS], head[RS_BAD_COORDS]);
        return fail(c, MRTX_E_INVALID, "the rings hold %llu edges: a call holds fewer than 2^31", head[RS_EDGES]);
    }
    q.n_edges = (uint32_t)head[RS_EDGES];
    HIPCHK(c, mrtx_launch_raster_count(q, c->stream, &launches));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
    if (head[RS_CROSSINGS] > MRTX_RS_MAX_COUNT) {
        CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
        return fail(c, MRTX_E_INVALID, "the edges cross the columns %llu times: a call holds at most 2^31 - 1 crossings", head[RS_CROSSINGS]);
    }
    q.n_cross = (uint32_t)head[RS_CROSSINGS];
    if (bins) {
        CHK(stage_buffer(c, c->illum_out, c->illum_out_bytes, 8 * (size_t)q.n_cross + 16));
        q.cross = reinterpret_cast<uint2*>(c->illum_out);
    }
    HIPCHK(c, mrtx_launch_raster_cover(q, c->stream, &launches));
    CHK(lattice_finish(c, nullptr, nullptr, 0, out, launches));
    if (bins) {                                                 // the scan's own check of what the two passes over the edges found
        HIPCHK(c, hipMemcpy(head, tb, sizeof head, hipMemcpyDeviceToHost));
        if (head[RS_BINNED] != head[RS_CROSSINGS])
            return fail(c, MRTX_E_DEVICE, "the bins hold %llu crossings of %llu", head[RS_BINNED], head[RS_CROSSINGS]);
    }
    if (host_labels) HIPCHK(c, hipMemcpy(host_labels, q.labels, 4 * N, hipMemcpyDeviceToHost));
    if (host_cover && n_polygons) HIPCHK(c, hipMemcpy(host_cover, q.cover, cover_bytes, hipMemcpyDeviceToHost));
    if (n_crossings) *n_crossings = head[RS_CROSSINGS];
    return MRTX_OK;
}

}  // extern "C"
