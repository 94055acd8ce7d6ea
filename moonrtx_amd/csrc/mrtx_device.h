// mrtx_device.h -- data shared by the host side of libmoonrt.so and its gfx950 kernels.
//
// Per-launch constants, derived once on the host in float64 from the calls the reference makes on its renderer
// object (moon_renderer.py:570-650 for the static scene, :824-871 for the per-time-step update).
//   FrameC    -- what the march loops touch, passed to the kernel BY VALUE -> SGPRs (wave-uniform scalar
//                loads, no VGPR cost);
//   FrameCold -- what a sample touches once (camera / moon-frame matrices in float64, light, Sun disk, colour and
//                environment grids), kept in device memory behind FrameC::cold and read with scalar loads at the
//                point of use.  Keeping these out of the by-value block stops the compiler from holding ~150
//                SGPRs live from kernel entry (it spilled 81 of them into VGPR lanes and moved them back and forth
//                with v_readlane / v_writelane around every sample).
#pragma once
#include <stdint.h>

struct GridC {          // equirectangular grid: row 0 = +90 deg, column 0 = -180 deg
    int32_t h, w;       // (renderer_navigation.py:575-593)
    float row_scale, row_off, col_scale, col_off, wf;
};

// DEM layout in HBM (see dem_march() in mrtx_march.h): row pairs, element (r, c) = float2 (D[r][c], D[r+1][c]),
// so the 2x2 footprint of a bilinear evaluation is ONE 16-byte load (plain padded float32, two 8-byte loads: retired,
// DESIGN.md section 4.18).
#define MRTX_DEM_ELEM_BYTES 8

// Tile numbering.  Tile t belongs to rank t % world, and t counts the tiles in raster order with a cyclic shift of
// `shift` columns per tile row: t = ty * tiles_x + (tx + shift * ty) % tiles_x.  With plain raster numbering and
// tiles_x a multiple of world (120 columns at 3840 px, world 2/4/8) every rank would own whole tile COLUMNS, which line
// up with vertical features (the terminator at the default orientation): 12 % rank imbalance at world 8.  The shift
// -- the smallest odd number >= 3 coprime to world -- turns the ownership into a 2-D lattice.
static inline __host__ __device__ void mrtx_tile_xy(int t, int tiles_x, int shift, int& tx, int& ty) {
    ty = t / tiles_x;
    const int c = t % tiles_x - (int)(((long long)shift * ty) % tiles_x);
    tx = c < 0 ? c + tiles_x : c;
}
static inline __host__ __device__ int mrtx_tile_id(int tx, int ty, int tiles_x, int shift) {
    return ty * tiles_x + (int)((tx + (long long)shift * ty) % tiles_x);
}
static inline int mrtx_tile_shift(int world) {
    for (int s = 3;; s += 2) {
        int a = s, b = world;
        while (b) { const int r = a % b; a = b; b = r; }
        if (a == 1) return s;
    }
}

// path_kernel's medium-mip step mask (mrtx_kernels.hip: step_mask): 1 builds and uses it, 0 (default: it does not pay, see there) neither
#ifndef MRTX_PATH_MIP2
#define MRTX_PATH_MIP2 0
#endif
// The medium mip also cuts the skip interval of a segment from one end, with tests that stop at the first inconclusive step
// (first_kept_step / last_kept_step in mrtx_march.h; round 4): bit 2 (4) camera rays, from the front: render 15.4 -> 13.9 ms at cfg3;
// bit 1 (2) shadow rays in render_kernel, from the end: -> 13.8; bit 3 (8) path_kernel's marches, from the end: path stage 5.0 -> 4.65;
// bit 0 (1) the trial segment, from the end: +0.17 ms, off.  The host builds the medium mip when either switch is set.
#ifndef MRTX_M2_DELTA
#define MRTX_M2_DELTA 2      // medium-mip cell = max-mip cell >> MRTX_M2_DELTA (never below 4 texels)
#endif
#ifndef MRTX_SEG_MASK
#define MRTX_SEG_MASK 14
#endif

struct FrameCold {
    // D1 pinhole camera (moon_renderer.py:627-635)
    float Wd[3], Ux[3], Vy[3], two_over_w, two_over_h;
    double oc[3], cq;       // eye - centre, |oc|^2 - R^2
    double M[3][3];         // scene -> moon frame, rows = (east 90, lon 0, north)
    float Mf[3][3], centerf[3], eyef[3];
    // D5 light (moon_renderer.py:640-641, :859-860)
    float Lb[3], rL2, rad2;
    // D8 Sun disk (moon_renderer.py:647-650)
    int32_t sun_on;
    float sc[3], sun_cq, sun_rad;
    float Sb[3], sun_r2;    // disk centre in the moon frame (relative to the Moon centre), radius^2: continuation rays see it
    float eps, scene_eps;
    float dlat_scale, dlon_scale;
    GridC gc;
    int32_t bg_h, bg_w;
    float bg_row_scale, bg_row_off, bg_col_scale, bg_col_off;
    uint32_t key0;
    uint32_t path_seg_min, path_seg_max;   // D6: path length in segments (camera segment = 1); max 1 = direct only
    float const_albedo[3];
    const uint8_t* color;   // RGBA8 or null
    const uint8_t* bg;      // RGBA8 or null
    // D11 overlay tubes: 12 floats per capsule (a - centre, r, b - centre, 0, colour, 0) + per-local-tile CSR bins
    const float* caps;
    const int32_t* caps_off;   // n_local_tiles + 1
    const int32_t* caps_idx;
    int32_t n_caps;
    // output buffers: touched once per pixel, at the end of a wave's life -- kept out of the by-value block so that they do
    // not occupy SGPRs (and get spilled) across the march loops
    float* accum;           // W*H float4: running sums r,g,b,coverage
    float* hits;            // W*H float4: x,y,z,d of sample 0 of the last block
    unsigned long long* stats;  // 10 counters, see MrtxStats (render_kernel's; [15] = path_kernel's watchdog)
    unsigned long long* stats_paths;   // the same counters as path_kernel adds them (MrtxStats::camera_* = the render kernel's share)
    // horizon mip (horizon_kend in mrtx_march.h): hm_h x hm_w cells of 2^hm_shift texels, or null
    const float* hmip;
    int32_t hm_h, hm_w, hm_shift;
    float hm_cell;                  // cell size in texels
    float hm_krow, hm_kcol;         // angle -> texel rows (h / pi); angle -> texel columns (1.05 w / 2 pi)
    // medium max-mip (path_kernel's step mask, round 4): cells of 2^m2_shift texels (a quarter of the max-mip's), plain floats with a
    // one-cell border like the max-mip before pairing -- (m2_h + 2) x (m2_w + 2) -- or null
    const float* mip2;
    int32_t m2_pitch, m2_h, m2_w, m2_shift;
};

struct FrameC {
    int32_t W, H;
    float Rf, R2f;
    // D2 march (moon_renderer.py:586-588)
    float step, inv_step;
    float polar_rho2, row_hi, col_hi;   // segment fallback threshold (0.04 R^2); largest floats below h / w
    int32_t nbis, kmax;
    GridC gd;
    const float* dem;       // PADDED (h+4) x (w+4): element [0] is (row -2, col -2); see dem_march()
    int32_t dem_pitch, dem_wide;   // pitch = w+4 floats; wide = byte offsets need 64 bits (> 4 GiB)
    uint32_t dem_maxidx;           // (h+2)*pitch + (w+2): last padded index a 2x2 tap may start at
    const float* mip;       // max-mip, (mip_h+2) x (mip_w+2) incl. its border, or null (skipping disabled)
    int32_t mip_pitch, mip_h, mip_w, mip_shift;   // cell = 2^mip_shift texels
    const FrameCold* cold;  // device memory
    // image-tile sharding (new) + accumulation state
    int32_t tile_w, tile_h, tiles_x, tiles_y, rank, world, n_local_tiles;
    int32_t tile_shift;         // see mrtx_tile_xy()
    const int32_t* tile_list;   // local tile indices to render (sky tiles culled on the host), or null = all
    int32_t n_active;           // entries of tile_list (== n_local_tiles when null)

    int32_t xcd_share;      // 1: every tile is shared by the 8 XCDs (few tiles per launch), 0: whole tiles per XCD
    uint32_t first_block, n_blocks;
};

// Hand-over between render_kernel<MODE 2> (camera ray, first vertex, its direct light, the decision to go on) and
// path_kernel (everything after), one RECORD per lane of every wave-job ("chunk") of the render launch:
//   ray0/1/2  float4 each, only for the samples whose path goes on, compacted to the front of the chunk (npaths[chunk] of
//             them, lane_of[] says whose): continuation-ray origin (3), direction (3), path throughput (3), exact DEM texel
//             coordinates (2) of the point the march goes on from, RNG key of the sample (1)
//   lane_of   bits 0-5 the lane (sample) of the chunk the record belongs to, and what render_kernel's trial segment found
//             out about the ray: bit 6 = still marching after segment 1 (bits 8-31 = its horizon bound kend, the texel
//             coordinates are those of the END of segment 1), bit 7 = hit inside segment 1 (bits 8-31 = the step k that
//             landed at/below the surface, the coordinates are the origin's); neither = march from the origin
//   c4        the sample's radiance so far (direct term / Sun disk / environment / overlay colour); path_kernel writes
//             the final value back when the path adds light, resolve_paths_kernel sums the 64 lanes in the butterfly
//             order of the spec
//   meta      per chunk: bit 31 = the chunk was deferred, bits 0-14 / 15-29 = pixel (x0, y0) of the wave's pixel block
// A wave writes 1 KB (ray*) / 256 B (c*) contiguous per array.
struct PathQ {
    float4* ray0; float4* ray1; float4* ray2;
    float* c0; float* c1; float* c2;    // unused (null) since the three-array layout was retired; they stay because PathQ is a by-value kernel
                                        // argument and taking them out changes the generated code of both kernels
    float4* c4;                 // the running radiance, three floats PACKED: 12 bytes per sample (see c_load / c_store)
    uint32_t* lane_of;          // per ray record: lane + the state of its march after the trial segment (see above)
    uint8_t* npaths;            // per chunk: ray records it holds (0 for a chunk that was not deferred): zero before the launch
    uint32_t* meta;
    uint32_t n_chunks;          // wave-jobs of the render launch (grid x jobs per wave)
    uint32_t grid_a;            // blocks of the render launch; chunk = block * jobs + job
    int32_t njobs_log2;         // jobs (pixel blocks) per render wave: 1 or 2
    uint32_t* counters;         // path_kernel's work counters: 8 XCDs x n_sub, zero before the launch
    int32_t n_sub, grp_log2;    // counters per XCD; render blocks per group handed out = 1 << grp_log2
    uint32_t gs_base;           // global sample index of sample 0 of this block (first_block * S)
    int32_t s_log2, pw_log2;    // S = 1 << s_log2 samples per pixel in a wave, pixel block PW x PH, PW = 1 << pw_log2
    int32_t refill_min;         // path_kernel refills its idle lanes when at least this many are idle
    int32_t seg_min;            // ... sets up march segments when at least this many lanes need one
    int32_t rare_min;           // ... and runs the rare steps (a continuation ray hit terrain; a vertex got its direct
                                //     term) when at least this many lanes wait for them
};
// The running radiance of a sample, the earlier layouts (retired).  Round 3: ONE float4 per sample instead of
// three float arrays -- a path that adds light reads and writes one 64-byte sector instead of three: path stage 5.41 -> 5.19 ms at
// cfg3, render and resolve unchanged.  Round 4, as shipped: the three floats PACKED, 12 bytes per sample -- resolve_paths_kernel
// streams a quarter less, the render kernel writes a quarter less, a path's read-modify-write still touches one sector five times in
// eight: path stage 4.35 -> 4.28 ms, frame -0.12 ms.
#define MRTX_PATH_REC_BYTES 64  // per record: 3 x float4 + 3 x float + 1 word
#define MRTX_REC_RESUME 64u
#define MRTX_REC_HIT 128u

// Sun illumination stage (mrtx_illum_grid / mrtx_illum_points): by value -> SGPRs.  A node is (row, col) of
// a rows x cols block; its unit vector comes from the float32 (sin, cos) tables the host built in float64.
struct IllumC {
    const float* rtab;      // (sin lat, cos lat) per row of the band; a point list: per point
    const float* ctab;      // (sin lon, cos lon) per column; a point list: per point
    const float* sun;       // n_sun (u2, u3) pairs
    float* out;             // rows x cols float4 (lit, irr, mu, D)
    int32_t rows, cols;     // a point list is one row of n points
    int32_t points;         // 1: row table indexed by the column (the point) as well
    int32_t n_sun, n_log2;  // samples per node (power of two <= 64)
    int32_t pw_log2;        // a wave's node block is (1 << pw_log2) columns wide (set by the launcher)
    int32_t waves_x;        // node blocks per row of blocks (set by the launcher)
};

// Sun illumination over many dates (mrtx_illum_series): a point list (g.points = 1, g.rows = points,
// g.cols = the window's length) and a table of per-epoch light constants, two float4 per epoch: (Lb.xyz, rL2), (rad2, 0, 0, 0).
struct IllumSeriesC {
    IllumC g;
    const float* lights;    // 8 floats per epoch, 16-byte aligned
    const int32_t* first;   // per point: its window's first epoch; null: every window starts at epoch 0
};

// Terrain horizons (mrtx_horizon_points): a point list as the illumination stage holds it (g.points = 1,
// g.rows = points; only the row / column tables are read) and n_az = 1 << az_log2 azimuths per point, n_bis probes each.
struct HorizonC {
    IllumC g;
    float* out;             // n_points x n_az float32 elevations (degrees), point-major
    int32_t az_log2;        // log2(n_az), 2 .. 12
    int32_t n_bis;          // probes per (point, azimuth), 1 .. 24
};

// The Sun against a horizon (mrtx_horizon_sun): per (point, epoch) the visible fraction of the light's
// disc above the point's horizon.  One wave per point walks the epochs 64 at a time.
struct HorizonSunC {
    IllumC g;               // the point list (g.rows points), as in HorizonC
    const float* horizon;   // n_points x n_az float32 elevations (degrees)
    const float* lights;    // 8 floats per epoch, as IllumSeriesC's
    float* out;             // mode 0: n_points x m float32 fractions; mode 1: n_points float4 (mean, lit, full, longest dark run)
    int32_t az_log2;        // log2(n_az)
    int32_t m;              // epochs
    int32_t mode;           // 0 FULL, 1 SUMMARY
};

// Raised horizons (mrtx_horizon_raised): HorizonC and per point the raise of its march origin.  A
// struct of its own, so that horizon_kernel's arguments stay as they were.
struct HorizonRaisedC {
    HorizonC h;
    const float* hs;        // per point: (float)(height_m / radius_m * R), >= 0
};

// Joint windows of two bodies against one set of horizons (mrtx_horizon_windows): HorizonSunC's point
// list and horizons, two epoch-light tables of m epochs each and the two thresholds.  One wave per point.
struct HorizonWindowsC {
    IllumC g;               // the point list (g.rows points), as in HorizonC
    const float* horizon;   // n_points x n_az float32 elevations (degrees)
    const float* lights_a;  // 8 floats per epoch, as IllumSeriesC's
    const float* lights_b;
    float* out;             // n_points x 8 float32 (two float4 per point)
    float min_a, min_b;     // ok = f >= min
    int32_t az_log2;        // log2(n_az)
    int32_t m;              // epochs
};

// Site power budgets (mrtx_power_budget, DESIGN.md sections 3.17 and 4.19): HorizonSunC's point list, horizons and epoch lights,
// the generation table as float32 watts and the load table already quantised to int32 counts.  One wave per point.
struct PowerC {
    IllumC g;               // the point list (g.rows points), as in HorizonC
    const float* horizon;   // n_points x n_az float32 elevations (degrees)
    const float* lights;    // 8 floats per epoch, as IllumSeriesC's
    const float* gen;       // m float32: (float)gen_w[k]
    const int32_t* load;    // m int32: L_k = (int32)rintf((float)load_w[k] * scale), formed on the host
    void* out;              // mode 0: n_points x m int32 G_k; mode 1: n_points x 8 int64 (four 16-byte stores per point)
    long long capacity;     // counts, 0 .. 2^52
    long long initial;      // counts, 0 .. capacity
    float scale;            // 2^cpw_log2, exact
    float nE, nN, nU;       // FIXED: the panel's unit normal in the point's (east, north, up), float64 rounded once
    int32_t panel;          // 0 TRACK, 1 FIXED, 2 AZIMUTH
    int32_t az_log2;        // log2(n_az)
    int32_t m;              // epochs
    int32_t mode;           // 0 FULL, 1 SUMMARY
};

// Regolith surface temperatures (mrtx_thermal): per point the absorbed flux of every epoch from its
// vertex, its horizon row and the epoch's light constants, and a 1D heat-conduction column stepped through the epochs.  One
// lane per point; the column lives in registers, so the node count is capped at compile time.  The layer tables are shared by
// every point and travel in the kernel arguments (scalar loads).
#define MRTX_THERMAL_NODES 32
struct ThermalC {
    IllumC g;                   // the point list (g.rows points), as in HorizonC
    const float* horizon;       // n_points x n_az float32 elevations (degrees)
    const float* lights;        // 8 floats per epoch, as IllumSeriesC's
    const float* flux;          // per epoch the solar flux at the Moon, W m^-2
    float* out;                 // mode 0: n x (m - n_spin) float32 surface temperatures; 1: n float4; 2: n x m float32 fluxes;
                                // 4: n x (m - n_spin) x n_nodes float32; 5: n x n_nodes double2 (8-byte aligned)
    unsigned long long* caps;   // two counters, zeroed by the host: [0] surface solves that reached the Newton cap, [1] the
                                // (point, epoch)s after whose steps a node was non-finite or outside [20, 450] K
    int32_t az_log2;            // log2(n_az)
    int32_t m;                  // epochs, spin-up included
    int32_t mode;               // 0 FULL, 1 SUMMARY, 2 FLUX, 3 EXITANCE (EXT), 4 COLUMN, 5 VOLATILE (COL, section 3.16)
    int32_t n_nodes;            // 3 .. MRTX_THERMAL_NODES
    int32_t n_sub;              // explicit steps per epoch
    int32_t n_spin;             // spin-up epochs (stepped, not recorded), < m outside FLUX
    int32_t block;              // epochs per spin-up block
    int32_t n_reset;            // spin-up blocks after which the nodes below ref are reset
    int32_t ref;                // the reference node of the reset
    float es;                   // emissivity x Stefan-Boltzmann
    float q_geo;                // geothermal flux, W m^-2
    float chi3;                 // chi / 350^3: k(T) = kc (1 + chi3 T^3)
    float c[5];                 // heat capacity c0 + c1 T + ... + c4 T^4, J kg^-1 K^-1
    float alb[3];               // A0, a, b of A(theta) = A0 + a (theta / 45)^3 + b (theta / 90)^8, theta in degrees
    float inv_dz0;              // 1 / dz_0
    float kc[MRTX_THERMAL_NODES];   // contact conductivity per node
    float hdz[MRTX_THERMAL_NODES];  // 0.5 / dz_i: link i joins nodes i and i + 1 (its k is the mean of theirs)
    float a[MRTX_THERMAL_NODES];    // Delta x 2 / (rho_i (dz_{i-1} + dz_i)), interior nodes
    float qdz[MRTX_THERMAL_NODES];  // Q x dz_i: the steady step of link i (the bottom node's step: i = N - 2)
    // thermal_kernel<EXT = true> only (mrtx_thermal_scatter, section 3.11); mode 3 (EXITANCE) writes n x (m - n_spin) float2
    const float* xflux;             // null, or n x m float32 extra absorbed flux, point-major
    // thermal_kernel<WIDE, true, 2> only (mrtx_thermal_column's VOLATILE, section 3.16)
    double vb[4];                   // ln E(T) = vb[0] - vb[1] / T + vb[2] ln T + vb[3] T
    // thermal_kernel<.., OCC = true> only (mrtx_thermal_occulted, section 3.18); appended, so the members above keep their offsets
    const float* occ_src;           // m epochs of the far source, 8 floats each as `lights`
    const float* occ_body;          // m epochs of the occulting body
    const int32_t* occ_mark;        // per epoch: nonzero where some point of the bounding sphere may have g < 1
};

// The occultation of a source by a body (mrtx_occultation): per (point, epoch) the share g of the
// source's disc that the body's disc leaves uncovered, seen from the point's lifted vertex.  One wave per point walks the
// epochs 64 at a time; an epoch whose mark is 0 takes g = 1 without forming anything.
struct OccultC {
    IllumC g;               // the point list (g.rows points), as in HorizonC
    const float* src;       // 8 floats per epoch, as IllumSeriesC's lights: the source (the Sun at its true distance)
    const float* body;      // the same for the occulting body (the Earth)
    const int32_t* mark;    // m int32, the host's float64 prefilter: 0 = no point of the bounding sphere can have g < 1
    float* out;             // mode 0: n_points x m float32 g; mode 1: n_points x 8 float32 (two float4 per point)
    int32_t m;              // epochs
    int32_t mode;           // 0 FULL, 1 SUMMARY
};

// What terrain a point sees (mrtx_view_hits).
struct ViewC {
    IllumC g;                   // the point list (g.rows points), as in HorizonC
    const float* dirs;          // K (uh1, uh2) pairs
    float* out;                 // n x K float2 (lat, lon) of the hits, degrees (NaN: sky), then n float32 terrain shares
    int32_t K;                  // 16, 32, ..., 1024
};

// The gather of the scattered flux (mrtx_scatter_flux, section 3.11).
struct ScatterC {
    const int32_t* idx;         // n x K indices into the hit list, -1: sky
    const float* ex;            // n_hits x m float2 (M_vis, M_ir)
    float* out;                 // n x m float32 Q_sec, point-major
    int32_t n, K, m;
    int32_t chunks;             // (m + 63) / 64
    float omah, eps, inv_k;     // 1 - A_h, emissivity, 1 / K
};

// Terrain line of sight (mrtx_sight_grid / mrtx_sight_points): the targets are a band (g.rows x g.cols,
// row / column tables) or a point list (g.points = 1, g.rows = 1, g.cols = n); the observers a point list of n_obs entries
// (obs.points = 1; 1 or g.cols of them) with their raised heights in scene units.  One lane per target; a wave holds 64
// neighbouring targets of one row.
struct SightC {
    IllumC g;               // the targets (only the row / column tables and rows, cols, points are read)
    IllumC obs;             // the observers (tables only)
    const float* obs_hs;    // per observer: (float)(h / radius_m * R)
    float* out;             // rows x cols float32 extra mast heights (metres), +inf where even mast_max does not see
    double target_h_m, mast_max_m, radius_m, R;   // a target at parameter t is raised by target_h_m + t * mast_max_m metres
    int32_t n_obs;          // 1 or g.cols (a point list)
    int32_t n_bis;          // 0 .. 24
    int32_t waves_x;        // waves per row of targets (set by the launcher)
};

// Least-cost traverses (mrtx_traverse, DESIGN.md sections 3.13 and 4.14; kernels in mrtx_traverse.hip).  A window of the DEM's
// texel lattice, rows x cols nodes, node n = i * cols + j; the relaxation works on tiles of TS x TS nodes, one workgroup each.
struct TraverseC {
    const float* dem;           // the context's padded DEM (FrameC::dem's layout), always addressed with 64-bit offsets
    int64_t dem_pitch;          // w + 4 elements
    int32_t dem_w;              // W: columns wrap modulo W
    int32_t row0, col0, rows, cols, stride, wrap;
    const float* len;           // rows x 3 float32 (L_ew, L_ns, L_dg), mrtx_traverse_lengths
    const float* pen;           // rows x cols float32 penalties, or null (m = 1)
    double* d;                  // rows x cols float64 costs
    uint8_t* pred;              // rows x cols predecessor codes
    float rm, gmax, a_up, a_dn; // (float) of radius_m, max_grade, climb_cost, descent_cost
    int32_t tile, tiles_x, tiles_y;   // tile edge TS (8, 16 or 32) and the tile grid
    uint32_t* flag_in;          // per tile: relax it in this launch (cleared by the tile's workgroup)
    uint32_t* flag_out;         // per tile: relax it in the next launch
    uint32_t* changed;          // per launch slot of a batch: workgroups that lowered a cost
    int32_t slot;               // this launch's slot
    unsigned long long* visits; // [0] tile visits, [1] bad device penalty entries
    const int64_t* src_node;    // the sources, duplicates reduced on the host: node index and start cost
    const double* src_cost;
    int32_t n_src;
};

// Timed traverses (mrtx_traverse_timed, DESIGN.md sections 3.19 and 4.22; kernels in mrtx_traverse.hip): TraverseC's window,
// lattice, penalties, tiles, flags and counters (its d and src_cost are not used), with arrival ticks in place of costs and an
// optional availability table of w64 = (n_epochs + 63) / 64 words per node, bit e & 63 of word e >> 6 = epoch e.
struct TraverseTimedC {
    TraverseC t;
    unsigned long long* arr;            // rows x cols uint64 arrival ticks, UINT64_MAX = unreachable
    const unsigned long long* avail;    // rows x cols x w64 words, node-major, or null (always drivable, no end)
    const unsigned long long* src_tick; // the sources' start ticks (duplicates reduced on the host)
    double tpc;                         // ticks per unit of edge weight
    int32_t tpe;                        // ticks per epoch, >= 1
    int32_t n_epochs;                   // epochs in the table, 1 .. 2^24
    int32_t w64;                        // words per node
};

// The traverse stage's launchers (mrtx_traverse.hip), one per step and field: init + seed, one relaxation launch over every
// tile, pred + source_pred; hipErrorInvalidValue for a block the kernels must not be started with.
hipError_t mrtx_launch_traverse_init(const TraverseC& q, hipStream_t st);
hipError_t mrtx_launch_traverse_relax(const TraverseC& q, hipStream_t st);
hipError_t mrtx_launch_traverse_pred(const TraverseC& q, hipStream_t st);
hipError_t mrtx_launch_traverse_heights(const TraverseC& q, float* out, hipStream_t st);
hipError_t mrtx_launch_timed_init(const TraverseTimedC& q, hipStream_t st);
hipError_t mrtx_launch_timed_relax(const TraverseTimedC& q, hipStream_t st);
hipError_t mrtx_launch_timed_pred(const TraverseTimedC& q, hipStream_t st);

// Drive masks (mrtx_horizon_mask, DESIGN.md sections 3.19 and 4.22): HorizonWindowsC's inputs, the joint predicate kept as bits.
// A struct of its own, so that horizon_windows_kernel's arguments stay as they were.
struct HorizonMaskC {
    IllumC g;               // the point list (g.rows points), as in HorizonC
    const float* horizon;   // n_points x n_az float32 elevations (degrees)
    const float* lights_a;  // 8 floats per epoch, as IllumSeriesC's
    const float* lights_b;  // the same, or null: the bit is ok_a alone
    unsigned long long* out;    // n_points x (m + 63) / 64 words, point-major
    float min_a, min_b;     // ok = f >= min
    int32_t az_log2;        // log2(n_az)
    int32_t m;              // epochs
};

// Orbiter passes (mrtx_horizon_passes, DESIGN.md sections 3.27 and 4.33): HorizonSunC's point list and horizons, the points'
// raises and a table of satellite positions in the body axes, one float4 (x, y, z, 0) per (satellite, epoch) in scene units.
// FULL and SUMMARY: one wave per point; LIST: one wave per (point, satellite), first the counts, then the records.
struct PassRec {            // MrtxPass, field for field: 40 bytes
    int32_t point, sat, first, count, max_at;
    uint32_t flags;
    float rise_frac, set_frac, max_elev_deg, min_range_m;
};
struct PassesC {
    IllumC g;               // the point list (g.rows points), as in HorizonC
    const float* horizon;   // n_points x n_az float32 elevations (degrees)
    const float* hs;        // per point: (float)(height_m / radius_m * R), >= 0
    const float* sat;       // n_sat x m float4, satellite-major
    void* out;              // FULL: n x n_sat x m float4; SUMMARY: n x 8 float32; LIST: the PassRec table (fill)
    uint32_t* counts;       // LIST, count: n x n_sat passes per (point, satellite)
    const unsigned long long* base;   // LIST, fill: n x n_sat exclusive prefix sums of the counts
    float min_elev;         // (float)min_elev_deg
    float range_scale;      // (float)(radius_m / R): scene units -> metres
    int32_t az_log2;        // log2(n_az)
    int32_t m;              // epochs per satellite
    int32_t n_sat;
};

// Terrain relief (mrtx_relief, DESIGN.md sections 3.14 and 4.15; kernels in mrtx_relief.hip).  A window of the DEM's texel
// lattice as in TraverseC, never wrapped; the footprint of a node is the (2 ri + 1) x (2 rj + 1) lattice nodes around it, read
// straight from the DEM (rows outside [0, dem_h) make the node NaN, columns wrap modulo dem_w).
struct ReliefC {
    const float* dem;           // the context's padded DEM (FrameC::dem's layout), always addressed with 64-bit offsets
    int64_t dem_pitch;          // w + 4 elements
    int32_t dem_h, dem_w;
    int32_t row0, col0, rows, cols, stride, ri, rj;
    int32_t tiles_x;            // the tile grid's width (the tiled kernels)
    const double* scale;        // rows x 2 float64 (kx, ky), mrtx_relief_scales
    double inv_n, inv_xj, inv_xi;   // the plane fit's three reciprocals, formed on the host
    float rm;                   // (float)radius_m
    float4* out;                // rows x cols (grade, rms_m, ge, gn)
    unsigned long long* fetches;    // the counter of the texels the spec reads, or null
};

// The safe share of a landing ellipse (mrtx_relief_share): integer box sums of the predicate grade <= gmax && rms_m <= smax
// over a rows x cols relief map, through a summed-area table of uint32 counts.
struct ShareC {
    const float4* relief;       // rows x cols (grade, rms_m, ge, gn)
    uint32_t* sat;              // rows x cols: row prefix sums after share_rows_kernel, the table after share_cols_kernel
    float* out;                 // rows x cols float32 safe / total
    int32_t rows, cols, Ri, Rj, wrap;
    float gmax, smax;
};
