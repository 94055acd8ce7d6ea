// mrtx_host.h -- what the three host units of libmoonrt.so share (mrtx_api.hip, mrtx_terrain_api.hip, mrtx_lattice_api.hip;
// DESIGN.md sections 4.34 and 4.35): the context, the refusal with its text and the checks every unit words alike, the scene's
// frame, and the staging, launch and read-back path of a stage (section 4.21).  Every function in namespace mrtx_host is
// defined once, in mrtx_api.hip.  Private: not installed, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/moonrt.h"
#include "mrtx_device.h"

struct mrtx_ctx {
    MrtxConfig cfg{};
    MrtxParams prm{};
    int tiles_x = 0, tiles_y = 0, n_tiles = 0, n_local = 0, slots = 0, tile_shift = 3;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> evs;         // stage boundaries of a deferred-path call (3 per block)
    // hand-over records of the deferred path stage (PathQ): 6 float arrays of 64 x chunks + one word per chunk
    float* path_rec = nullptr; uint32_t* path_meta = nullptr; uint8_t* path_npaths = nullptr; uint64_t path_cap = 0;
    uint32_t* path_ctr = nullptr;        // 8 x 16 work counters of path_kernel
    unsigned long long* wd_host = nullptr;   // pinned: path_kernel's watchdog word
    uint64_t path_budget_bytes = 64ull << 30;   // hand-over buffers: frames that need more are rendered in sub-parts (MOONRT_PATH_MAX_GB).  Sized for 288 GB of HBM:
                                                // a 4K frame with every pixel on the Moon (34 GB) stays ONE part -- 38.9 ms against 39.2 in two parts of 24 GB
    bool path_budget_env = false;               // the budget was given explicitly: take it as it is (else: at most half of the free memory)
    int path_nsub = 4, path_grp_log2 = 3;   // measured at cfg3: (0,1) 37 ms, (1,1) 20.5, (1,4) 16.1, (2,4) 16.3, (3,4) 16.6
    int path_waves[4] = {0, 0, 0, 0};    // persistent waves of path_kernel<stats, wide>, 0 = not asked yet
    // launches with fewer samples than this keep their paths inside the render wave (same result, bit for bit): the three
    // kernels + 5 120 persistent waves of the queue do not pay below ~8 M samples (4K: 1 spp 1.34 ms against 1.48, 2 spp 2.28 /
    // 2.41, 4 spp 3.42 / 3.16; cfg1 0.33 / 0.53; tools/spp_sweep.py).  MOONRT_PATH_QUEUE_MIN overrides (0 = always the queue).
    uint64_t path_queue_min = 8000000ull;
    bool path_fallback_said = false;     // the fall-back to in-wave paths (no memory for the records) was reported
    // overlapped path stage (MOONRT_PATH_OVERLAP = sub-parts, 0 = off): path_kernel + resolve of sub-part i run on stream2 beside
    // render_kernel of sub-part i+1 (two sets of hand-over buffers, ping-pong); MOONRT_PATH_OVERLAP_WAVES sizes the persistent
    // launch while it shares the chip (every path wave holds 96 VGPRs, a render wave 64)
    int path_overlap = 0, path_overlap_waves = 2048;
    int path_sets = 1;                   // buffer sets the allocations hold
    hipStream_t stream2 = nullptr;
    hipEvent_t ov_done[2] = {nullptr, nullptr}, ov_join = nullptr;
    uint64_t path_nomem_chunks = 0;      // a hand-over allocation of this many chunks failed: not retried until less is needed or mrtx_reset_accum
    bool gather_hits = true;             // mrtx_set_gather_hits: the hit buffer travels with the radiance
    bool path_alloc_fail_test = false;   // MOONRT_TEST_PATH_NOMEM=1: test hook, the hand-over allocation "fails"
    int path_refill = 32, path_segmin = 16, path_hitmin = 16, path_waves_env = 0;   // cfg3 sweep: (8,24,16) 16.2 ms, (24,24,16) 14.7, (32,16,16) 14.5, (48,24,16) 21.5
    float* accum = nullptr;
    float* hits = nullptr;
    void* scratch = nullptr;  // W*H*16 bytes, resolve target for read-back
    // "Gamma" post-process tables (tone_table): 256 / 65536 thresholds for the gamma they were built for (0 = not built)
    float* tone8_dev = nullptr; float tone8_gamma = 0.0f;
    float* tone16_dev = nullptr; float tone16_gamma = 0.0f;
    float* dem = nullptr; int dem_h = 0, dem_w = 0;   // padded (h+4) x (w+4) copy, always owned
    float* hmip = nullptr; int hm_h = 0, hm_w = 0, hm_shift = 0;       // horizon mip: cells of 8 max-mip cells, dilated by one cell (see horizon_kend)
    float* mip2 = nullptr; int m2_h = 0, m2_w = 0, m2_shift = 0;       // medium max-mip: cells a quarter of the max-mip's (path_kernel's step mask)
    float* mip = nullptr; int mip_h = 0, mip_w = 0, mip_shift = 0;   // max-mip of it, cell 2^mip_shift texels (+ one-cell border)
    uint8_t* color = nullptr; bool color_owned = false; int color_h = 0, color_w = 0;
    uint8_t* bg = nullptr; int bg_h = 0, bg_w = 0;
    uint32_t* overlay = nullptr;   // D12: frame-sized RGBA8 blended over the tone-mapped image, or null
    unsigned long long* stats_dev = nullptr;
    FrameCold* cold_dev = nullptr;
    FrameCold cold_uploaded;             // what cold_dev holds (valid once cold_valid): re-uploaded only when it changes
    bool cold_valid = false;
    // D11 overlay capsules: host copy in scene coordinates; device copies relative to the Moon centre + tile bins
    std::vector<float> caps_host;            // 12 floats per capsule
    float* caps_dev = nullptr; int32_t* caps_off_dev = nullptr; int32_t* caps_idx_dev = nullptr;
    size_t caps_dev_n = 0, caps_idx_cap = 0;
    std::vector<int32_t> caps_off_host;      // per local tile, valid for caps_version
    uint64_t caps_version = 0;               // scene_version the bins were built for
    int32_t* tile_list_dev = nullptr;   // n_local entries
    std::vector<int32_t> keep_uploaded;  // what tile_list_dev holds
    std::vector<int32_t> keep_cached;    // cull result for scene_version == cull_version
    uint64_t culled_px_cached = 0;
    int keep_front_cached = 0;           // leading entries of keep_cached that can see the Moon / Sun / an overlay (the rest is sky)
    uint64_t scene_version = 1, cull_version = 0;   // bumped by every setter that can change the cull
    std::vector<uint8_t> tile_dirty;     // local tiles written since the buffers were last zeroed
    // gather layout: with the sky cull in force only ACTIVE tiles travel (every rank derives every rank's list from the
    // scene, which is identical on all ranks by contract); act_slots = the longest list, shorter ones are padded with -1
    std::vector<std::vector<int32_t>> act_lists;
    uint64_t act_version = 0;
    bool act_on = false;
    int act_slots = 0;
    int32_t* act_dev = nullptr;          // world x act_slots, uploaded for act_uploaded_version
    size_t act_dev_cap = 0;
    uint64_t act_uploaded_version = 0;
    std::vector<uint8_t> peer_written;   // root: global tiles of other ranks that hold unpacked data
    int32_t* stale_dev = nullptr;
    size_t stale_cap = 0;
    uint32_t blocks_done = 0;
    double eye[3] = {0, -300, 0}, target[3] = {0, 0, 0}, up[3] = {0, 0, 1}, vfov = 4.2421875;
    double center[3] = {0, 0, 0}, radius = 10.0, u[3] = {0, 0, 1}, v[3] = {0, -1, 0};
    double light_pos[3] = {0, -21460, 0}, light_radius = 100.0, light_radiance = 0.0;
    double sun_pos[3] = {0, 3100, 0}, sun_radius = 0.0, sun_radiance = 2.0;
    bool moon_set = false, light_set = false;   // mrtx_set_moon_frame / mrtx_set_light were called (the illumination stage needs both)
    // Sun illumination stage (mrtx_illum_*): its OWN cold block, counters and buffers, so that it leaves the render state alone
    FrameCold* illum_cold = nullptr;
    unsigned long long* illum_stats = nullptr;   // ST_N counters
    float* illum_tab = nullptr; size_t illum_tab_bytes = 0;    // sample table + (sin, cos) tables
    float* illum_out = nullptr; size_t illum_out_bytes = 0;    // float4 per node when the caller gives no device buffer
    float* trav_buf = nullptr; size_t trav_bytes = 0;         // mrtx_traverse: tile flags, and the outputs the caller wants on the host
    std::string err;
};

namespace mrtx_host {

// the refusal: the text into the context (if there is one), the code back
int fail(mrtx_ctx* c, int code, const char* fmt, ...);

// a table comes from the device or from the host: "give exactly one of dev_<what> and host_<what>"
int one_of(mrtx_ctx* c, const void* dev, const void* host, const char* what);

// an optional table comes from one of them or from neither: "give at most one of dev_<what> and host_<what>"
int at_most_one(mrtx_ctx* c, const void* dev, const void* host, const char* what);

// a device table (or none) at a multiple of 4 or 8 bytes: "<name> must be <bytes>-byte aligned (<type>)"
int aligned(mrtx_ctx* c, const void* p, unsigned bytes, const char* name, const char* type);

// A two-valued variant switch of the environment: *is_first keeps the caller's default when the variable is not set.  One
// value is the stage's scheme, the other its yardstick: the same bytes by the plain scheme.
int variant(mrtx_ctx* c, const char* name, const char* first, const char* second, bool* is_first);

// The scene as the launches see it: the vector helpers, the Moon frame's rows and the light's constants that build_frame and
// the per-epoch tables both form, the per-launch constant blocks, and the march's mip levels (built when the step asks)
constexpr double kPiD = 3.14159265358979323846;
int check_vec(const double* p);     // three finite numbers
void cross(const double a[3], const double b[3], double o[3]);
void moon_rows(const double u[3], const double v[3], double M[3][3]);
void light_consts(const double M[3][3], const double center[3], const double pos[3], double radius, double radiance, float Lb[3],
                  float& rL2, float& rad2);
void build_frame(const mrtx_ctx* c, FrameC& f, FrameCold& k);
int ensure_mip(mrtx_ctx* c);

// do the two byte ranges share a byte?  A null pointer is no range.
bool spans_overlap(const void* a, size_t na, const void* b, size_t nb);

// grow one of the stage's device buffers to at least `bytes`
int stage_buffer(mrtx_ctx* c, float*& p, size_t& cap, size_t bytes);

// n 4-byte words (float or int32) of host memory for stage_tables
struct HostSeg {
    const void* p;
    size_t n;
    HostSeg(const void* p_, size_t n_) : p(p_), n(n_) {}
    HostSeg(const std::vector<float>& v) : p(v.data()), n(v.size()) {}
};

// The launch's tables in one device block, c->illum_tab: each segment at an offset rounded up to 16 bytes (the float4 loads
// of the epoch lights), copied straight from the caller's memory, which must stay put until stage_finish.  dev[i] = segment
// i's device address.  Called after stage_out, so that every buffer is grown before the first copy is queued.
int stage_tables(mrtx_ctx* c, std::initializer_list<HostSeg> segs, float** dev);

// where the launch writes: the caller's dev_out, or else c->illum_out grown to `bytes` (read back by stage_finish)
int stage_out(mrtx_ctx* c, void*& dev_out, size_t bytes);

// right before the launch: the cold block (if any) and zeroed counters (if asked) queued, then the start event
int stage_start(mrtx_ctx* c, const FrameCold* cold, bool zero);

// the counter slot of a launch's rays (mrtx_march.h's ST_SHADOW, ST_BOUNCE), or none when it did not count
enum StageRays { kNoRays = -1, kShadowRays = 2, kBounceRays = 8 };

// right after the launch: the end event, wait, time, read back, counters (rays: reported as shadow_rays or bounce_rays)
int stage_finish(mrtx_ctx* c, const void* dev_out, float* host_out, size_t out_bytes, MrtxStats* out, StageRays rays);

}  // namespace mrtx_host

#define HIPCHK(c, call)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return ::mrtx_host::fail((c), MRTX_E_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// a check or a step that did not pass ends the call with its code
#define CHK(call)                         \
    do {                                  \
        const int rc_ = (call);           \
        if (rc_ != MRTX_OK) return rc_;   \
    } while (0)
