/*
 * moonrt.h -- C ABI of libmoonrt.so, the MI355X (gfx950) renderer that replaces the
 * PlotOptiX/OptiX backend behind MoonRTX's `self.rt` object.
 *
 * The reference has no C FFI: its renderer boundary is the Python object created at
 * moonrtx/moon_renderer.py:571-575 (`TkOptiX(width, height, on_launch_finished=...)`).
 * Every entry point below cites the reference call(s) on that object which it serves; the
 * Python facade `moonrtx_amd/tkoptix.py` maps those calls 1:1 onto this ABI through ctypes.
 *
 * Conventions
 *   - plain C types only; host pointers are borrowed for the duration of the call;
 *   - every function returns 0 on success or a negative MRTX_E_* code; the text of the last
 *     failure on a context is available from mrtx_last_error();
 *   - no C++ exception crosses the ABI and nothing aborts the process;
 *   - one context is driven by one thread at a time (the facade's render thread holds the
 *     `_padlock` while it calls in, moon_renderer.py:849-852).
 */
#ifndef MOONRT_H
#define MOONRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRTX_ABI_VERSION 7

enum {
    MRTX_OK = 0,
    MRTX_E_INVALID = -1,   /* bad argument                                   */
    MRTX_E_DEVICE = -2,    /* a HIP call failed (text in mrtx_last_error)    */
    MRTX_E_STATE = -3,     /* call made in the wrong state (e.g. no DEM yet) */
    MRTX_E_NOMEM = -4
};

typedef struct mrtx_ctx mrtx_ctx;

/* Frame + sharding description.  rank/world shard the image in tiles of tile_w x tile_h
 * pixels: tile t belongs to rank (t % world), where t numbers the tiles in raster order with a cyclic shift of s
 * columns per tile row -- t = ty * tiles_x + (tx + s * ty) % tiles_x, s = the smallest odd number >= 3 coprime to
 * world -- so that a rank's tiles form a 2-D lattice, not whole columns.  world == 1 renders everything. */
typedef struct MrtxConfig {
    int32_t device;          /* HIP device ordinal                                             */
    int32_t width, height;   /* TkOptiX(width=, height=)            moon_renderer.py:571-573   */
    int32_t rank, world;     /* image-tile sharding (new; the reference is single-GPU)        */
    int32_t tile_w, tile_h;  /* sharding / culling tile (multiples of 16), 0 = default: 16 x 16 for world <= 2, 32 x 32 else */
} MrtxConfig;

/* String-keyed knobs of the reference collapsed into one POD.
 *   set_float("scene_epsilon" | "marching_step" | "marching_step_eps")  moon_renderer.py:586-588
 *   set_float("tonemap_exposure" | "tonemap_gamma")                      moon_renderer.py:598-599, :367
 *   set_uint("path_seg_range", 2, 4)                                      moon_renderer.py:583
 *   set_param(min_accumulation_step=, max_accumulation_frames=)           moon_renderer.py:578, :475, :487 */
typedef struct MrtxParams {
    float scene_epsilon;
    float marching_step;
    float marching_step_eps;
    float tonemap_exposure;
    float tonemap_gamma;
    uint32_t path_seg_min, path_seg_max;   /* path length in ray segments, camera segment = 1; max <= 1 traces direct
                                              light only; beyond `min` the path survives Russian roulette            */
    uint32_t spp_per_launch;   /* samples per pixel per accumulation block: 1,2,4,...,64 */
    uint32_t max_spp;          /* max_accumulation_frames (informational for the ABI)   */
    uint32_t seed;
    float const_albedo[3];     /* reflectance used when no colour texture is bound       */
    uint32_t flags;            /* MRTX_F_*                                                */
} MrtxParams;

#define MRTX_F_COUNT_STATS 1u  /* maintain the deterministic sample counters of MrtxStats */
#define MRTX_F_NO_SKIP     4u  /* evaluate every march step (disable the result-preserving max-mip skip) */
#define MRTX_F_NO_CULL     8u  /* dispatch every tile (disable the host-side sky-tile cull) */
#define MRTX_F_NO_SORT     16u /* dispatch tiles in raster order (disable the limb-ring-first launch order) */
#define MRTX_F_FORCE_WIDE  2u  /* test hook: use the 64-bit DEM addressing path (normally only for DEMs > 4 GiB) */
#define MRTX_F_INWAVE_PATHS 32u /* path_seg_max > 1: keep the whole path inside the wave that traced the camera ray instead
                                   of continuing it behind a queue in path_kernel (same result bit for bit; A/B switch) */

typedef struct MrtxStats {
    uint64_t primary_rays;        /* camera samples (pixel x spp), the headline "ray"      */
    uint64_t primary_hits;        /* camera samples that hit the Moon                      */
    uint64_t shadow_rays;         /* light-sample rays marched                             */
    uint64_t height_samples;      /* DEM bilinear evaluations the march DEFINES (16 B each): every step of every
                                     segment until hit / exit, bisection, normal taps -- equals the oracle's count */
    uint64_t colour_fetches;      /* colour bilinear fetches (16 B each)                   */
    uint64_t background_fetches;  /* environment texel fetches (4 B each)                  */
    uint64_t dem_fetches;         /* DEM bilinear evaluations actually PERFORMED (steps the max-mip bound proves to
                                     be above the terrain are skipped; results are unchanged)                  */
    uint64_t mip_fetches;         /* max-mip texels read for those bounds (4 B each)                           */
    uint64_t bounce_rays;         /* D6 path-continuation rays marched (0 when path_seg_max <= 1)              */
    uint64_t bounce_sun_hits;     /* ... of which left the Moon and ended on the visible Sun disk              */
    double kernel_ms;             /* HIP-event time of the kernels of this call = primary_ms + paths_ms        */
    double primary_ms;            /* render_kernel: camera ray, first vertex, its direct light                 */
    double paths_ms;              /* path_kernel + resolve_paths_kernel: everything after the first vertex
                                     (0 unless path_seg_max > 1 and the queue-based path stage is in use)      */
    uint32_t launches;
    uint32_t reserved;
    /* ABI 7: the share of the counters above that render_kernel (the camera-ray stage: camera ray, first vertex, its shadow ray,
     * and with the path queue the FIRST segment of the continuation ray) performed itself; the rest was performed by path_kernel.
     * With the paths inside the render wave (or path_seg_max <= 1) these equal the totals.  bench.py prices each kernel's
     * algorithmic bytes with its own counts. */
    uint64_t camera_height_samples, camera_dem_fetches, camera_mip_fetches, camera_colour_fetches, camera_background_fetches;
} MrtxStats;

/* TkOptiX(width, height, ...) -- moon_renderer.py:571-575.  Allocates accumulation + hit buffers. */
int mrtx_create(const MrtxConfig* cfg, mrtx_ctx** out);
/* rt.close() -- moon_renderer.py:880-884 */
void mrtx_destroy(mrtx_ctx* ctx);
const char* mrtx_last_error(mrtx_ctx* ctx);
int mrtx_abi_version(void);
/* The configuration the context runs with: what mrtx_create was given, with the defaults filled in (tile_w / tile_h: 16 x 16
 * for world <= 2, 32 x 32 from four ranks up) -- so that a caller reports the tiling that was actually used. */
int mrtx_get_config(mrtx_ctx* ctx, MrtxConfig* out);

/* rt.set_displacement("moon", elevation, refresh=False) -- moon_renderer.py:624.
 * `host` is the float32 (h, w) array load_elevation_data returns (data_loader.py:166-247):
 * equirectangular, row 0 = +90 deg, column 0 = -180 deg, max exactly 1.0. */
int mrtx_upload_dem(mrtx_ctx* ctx, const float* host, int32_t h, int32_t w);
/* Same, from a device pointer (synthetic / device-built DEMs).  Either way the context keeps its OWN copy,
 * re-laid-out in row pairs -- element (r, c) = float2 (D[r][c], D[r+1][c]) -- with a two-texel border (wrap in longitude,
 * clamp in latitude), so a bilinear evaluation on the march path is ONE unconditional 16-byte load; 8 bytes per texel.
 * The caller may free its buffer when the call returns. */
int mrtx_bind_dem_device(mrtx_ctx* ctx, const void* dev_f32, int32_t h, int32_t w);

/* rt.set_texture_2d("moon_color", rgba_u8) + update_material("diffuse", {"ColorTextures": [...]})
 * -- moon_renderer.py:613-617.  NULL => const_albedo of MrtxParams. */
int mrtx_upload_color(mrtx_ctx* ctx, const uint8_t* rgba, int32_t h, int32_t w);
/* Same, from a device pointer; the context keeps its own row-pair copy (8 bytes per texel), the caller's array is read once. */
int mrtx_bind_color_device(mrtx_ctx* ctx, const void* dev_rgba8, int32_t h, int32_t w);

/* rt.set_background_mode("TextureEnvironment"); rt.set_background(star_map, gamma=, rt_format="UByte4")
 * -- moon_renderer.py:604-609.  NULL => black (`set_background(0)`). Texels are RGBA8, already in the
 * renderer's linear space (the facade applies the gamma of set_background on the host). */
int mrtx_upload_background(mrtx_ctx* ctx, const uint8_t* rgba, int32_t h, int32_t w);

/* add_postproc("Overlay") + set_texture_2d("frame_overlay", rgba, filter_mode="Nearest") -- renderer_video.py:137-144:
 * a frame-sized RGBA8 texture alpha-blended over the tone-mapped image in mrtx_read_rgba8 (exact: 50 % black over 46
 * reads 23, renderer_video.py:21-25).  NULL removes it. */
int mrtx_upload_overlay(mrtx_ctx* ctx, const uint8_t* rgba, int32_t h, int32_t w);

/* set_float / set_uint / set_param / set_ambient / add_postproc -- moon_renderer.py:578-600 */
int mrtx_set_params(mrtx_ctx* ctx, const MrtxParams* p);
void mrtx_default_params(MrtxParams* p);

/* setup_camera / update_camera / _optix.set_camera_fov -- moon_renderer.py:627-635,
 * renderer_navigation.py:73,150,224,521.  Pinhole; vfov is the vertical field of view, degrees. */
int mrtx_set_camera(mrtx_ctx* ctx, const double eye[3], const double target[3], const double up[3],
                    double vfov_deg);

/* set_data("moon", geom="ParticleSetTextured", geom_attr="DisplacedSurface", pos, u, v, r) and
 * update_data("moon", u=, v=) -- moon_renderer.py:620-621, :854.  u = north pole, v = direction of
 * longitude 0 (renderer_navigation.py:47-53, :486-490), both in scene coordinates. */
int mrtx_set_moon_frame(mrtx_ctx* ctx, const double center[3], double radius, const double u[3],
                        const double v[3]);

/* setup_light("sun", color=, radius=, in_geometry=False) / update_light(pos=, color=, radius=)
 * -- moon_renderer.py:640-641, :347, :859-860.  `radiance` is the light colour (scalar, white). */
int mrtx_set_light(mrtx_ctx* ctx, const double pos[3], double radius, double radiance);

/* set_data("sun_disk", geom="ParticleSet", mat="flat", pos, r, c=2.0) / update_data(...)
 * -- moon_renderer.py:647-650, :855.  radius <= 0 disables the disk. */
int mrtx_set_sun_disk(mrtx_ctx* ctx, const double pos[3], double radius, double radiance);

/* set_graph / update_graph / delete_geometry -- renderer_labels.py:295-300, :367-373, renderer_pins.py:54: ALL overlay
 * graphs flattened into capsules, 12 floats each (ax ay az r  bx by bz 0  cr cg cb 0), scene coordinates, flat colour;
 * they never shadow and are invisible to shadow / continuation rays (renderer_labels.py:132-139).  n = 0 removes them. */
int mrtx_set_capsules(mrtx_ctx* ctx, const float* caps12, int32_t n);

/* rt.refresh_scene() -- moon_renderer.py:488, :871: restart the accumulation cycle. */
int mrtx_reset_accum(mrtx_ctx* ctx);

/* One or more accumulation blocks (what the PlotOptiX render thread does between two
 * on_launch_finished callbacks, moon_renderer.py:574; renderer_status.py:239).  Each block adds
 * spp_per_launch samples to every pixel this rank owns.  Blocking.  `out` may be NULL. */
int mrtx_render(mrtx_ctx* ctx, int32_t n_blocks, MrtxStats* out);
/* The same block of samples, one part of the tile list at a time (parts 0 .. n_parts-1 in order; the sample counter
 * advances with the last one), so that the exchange can move part k while part k+1 renders: see mrtx_pack_part. */
int mrtx_render_part(mrtx_ctx* ctx, int32_t n_blocks, int32_t part, int32_t n_parts, MrtxStats* out);

/* Read-back.  All are full-frame W*H arrays, caller-allocated; on a sharded context pixels of
 * other ranks read as zero.
 *   linear : float32 RGBA, mean linear radiance, A = 1 where any sample hit geometry
 *   rgba8  : the "Gamma" post-process (exposure * L)^(1/gamma) -> 8 bit, moon_renderer.py:598-600
 *   hits   : float32 (x, y, z, d) in scene coordinates, d <= 0 == miss -- rt._get_hit_at(x, y),
 *            moon_renderer.py:1138, renderer_navigation.py:195-203 */
int mrtx_read_linear(mrtx_ctx* ctx, float* rgba_out);
int mrtx_read_rgba8(mrtx_ctx* ctx, uint8_t* out);
/* rt.save_image(path, bps="Bps16") -- renderer_dialogs.py:1222-1224 (".tiff" is saved with 16 bits per sample): the same
 * exposure + "Gamma" post-process at 16 bits, W*H*3 uint16 (RGB interleaved), caller-owned.  Both tone-mapped read-backs are
 * exact: level = round(N * (exposure * mean)^(1/gamma)) decided by comparing with N float32 thresholds
 * (float)pow((j - 0.5) / N, gamma) built on the host, so they equal the oracle's bytes. */
int mrtx_read_rgb16(mrtx_ctx* ctx, uint16_t* out);
int mrtx_read_hits(mrtx_ctx* ctx, float* xyzd_out);
/* One texel of the hit buffer (16 bytes over PCIe): what rt._get_hit_at(x, y) needs per mouse event
 * (moon_renderer.py:1137-1142) without pulling the 133 MB buffer of a 4K frame after every launch. */
int mrtx_read_hit(mrtx_ctx* ctx, int32_t x, int32_t y, float xyzd_out[4]);
int mrtx_samples_done(mrtx_ctx* ctx, uint32_t* out);

/* ---- multi-GPU exchange step (new: the reference is single-GPU) -------------------------------
 * A rank packs the tiles it owns (linear float4 radiance followed by float4 hits) into a compact
 * device buffer the caller provides (e.g. a torch tensor handed to an RCCL gather), and rank 0
 * scatters the gathered buffers back into frame order. */
/* Whether the hit buffer travels with the radiance (default 1: a packed slot is one tile of float4 sums followed by one tile of
 * float4 hits, 32 B per pixel).  0: sums only, 16 B per pixel -- the exchange moves the final linear framebuffer and nothing
 * else; the root's hit buffer then holds its own tiles only, and a pick (rt._get_hit_at(x, y), one texel per mouse event,
 * moon_renderer.py:1137-1142) is served by mrtx_read_hit on the rank that owns the pixel (moonrtx_amd/dist.py: FrameGather.hit_at).
 * Must be set alike on every rank; changes mrtx_shard_bytes* and the layout pack / unpack use. */
int mrtx_set_gather_hits(mrtx_ctx* ctx, int32_t on);
int mrtx_shard_bytes(mrtx_ctx* ctx, int32_t rank, uint64_t* out);   /* upper bound of a packed buffer (all tiles) */
/* Bytes the exchange moves per rank for the scene as it stands.  While the host-side sky cull is in force (no
 * environment map, no overlay geometry, MRTX_F_NO_CULL clear) only the tiles the cull keeps travel: every rank
 * derives every rank's tile list from its own copy of the scene -- identical on all ranks by contract -- so the
 * layout is never negotiated.  Equal on every rank (padded to the longest list), <= mrtx_shard_bytes().
 * pack/unpack below use this layout; a buffer of mrtx_shard_bytes() is always large enough. */
int mrtx_shard_bytes_active(mrtx_ctx* ctx, uint64_t* out);
int mrtx_pack_shard(mrtx_ctx* ctx, void* dev_dst, void* hip_stream);
/* The shard in parts.  A packed shard is [slot][sums tile, hits tile], so a range of slots is one contiguous piece;
 * part k of n_parts covers the same slot numbers on every rank (the tiles mrtx_render_part(.., k, n_parts) rendered),
 * is written at byte_off .. byte_off + byte_len of dev_dst, and can be handed to the collective while part k+1
 * still renders.  mrtx_shard_parts() says how many parts the scene allows (1 while the full layout is in force). */
int mrtx_shard_parts(mrtx_ctx* ctx, int32_t wanted, int32_t* out);
int mrtx_pack_part(mrtx_ctx* ctx, void* dev_dst, int32_t part, int32_t n_parts, uint64_t* byte_off, uint64_t* byte_len,
                   void* hip_stream);
int mrtx_unpack_shard(mrtx_ctx* ctx, int32_t src_rank, const void* dev_src, void* hip_stream);
/* Same for every peer at once: dev_srcs[r] is rank r's packed buffer (the own rank's entry is ignored); one
 * synchronisation.  Tiles of peers that held an earlier view's data and are sky in this one are zeroed. */
int mrtx_unpack_all(mrtx_ctx* ctx, const void* const* dev_srcs, int32_t n);

/* Raw device pointers of the context's buffers (for zero-copy wrapping by the host side). */
/* MRTX_BUF_DEM is the context's own copy of the displacement map in its march layout: (h+4) x (w+4) elements of
 * float2 (D[r][c], D[r+1][c]), two-texel border (rows clamp, columns wrap) -- not the array that was uploaded.
 * MRTX_BUF_COLOR likewise: (h+1) x (w+4) elements of two RGBA8 texels (T[r][c], T[r+1][c]).  mrtx_bind_dem_device and
 * mrtx_bind_color_device read the caller's device array once; the caller may free it afterwards. */
/* MRTX_BUF_MIP, MRTX_BUF_MIP2 and MRTX_BUF_HMIP are the structures the marches skip with, built from the DEM by the first
 * marching call for the march step in force (null and 0 bytes before that, and again after a new DEM): the max-mip in row
 * pairs, (mip_h+2) x (mip_w+2) elements of float2 (m[i][j], m[i+1][j]); the medium max-mip, (m2_h+2) x (m2_w+2) floats;
 * the horizon mip, hm_h x hm_w floats.  Read-only; the layouts are defined in DESIGN.md section 4.23. */
enum { MRTX_BUF_ACCUM = 0, MRTX_BUF_HITS = 1, MRTX_BUF_DEM = 2, MRTX_BUF_COLOR = 3, MRTX_BUF_MIP = 4, MRTX_BUF_MIP2 = 5,
       MRTX_BUF_HMIP = 6 };
int mrtx_device_ptr(mrtx_ctx* ctx, int32_t which, void** out, uint64_t* bytes);
/* out = { mip_shift, mip_h, mip_w, m2_shift, m2_h, m2_w, hm_shift, hm_h, hm_w }: cells of 2^shift texels, sizes without the
 * borders.  All zero while nothing is built. */
int mrtx_mip_info(mrtx_ctx* ctx, int32_t out[9]);

/* ---- ingest kernels (data_loader.py:166-247, the step before set_displacement) ----------------
 * Device-side restatement of load_elevation_data: int16 LDEM units -> block mean (two-stage f32,
 * axis 4 then axis 2) -> * 0.5/1737400 -> + 1 -> / max.  src_dev is (h*d, w*d) int16 on the device,
 * dst_dev is (h, w) float32 on the device.  radius_scale receives the pre-normalisation maximum. */
int mrtx_dem_from_ldem(int32_t device, const void* src_dev_i16, int32_t h, int32_t w, int32_t downscale,
                       void* dst_dev_f32, float* radius_scale, char* err, int32_t err_len);
/* Seeded synthetic LDEM-like int16 source written straight into device memory (bench input). */
int mrtx_synth_ldem(int32_t device, void* dst_dev_i16, int32_t h, int32_t w, uint32_t seed,
                    char* err, int32_t err_len);
/* Seeded synthetic RGBA8 albedo texture (already through the 0.2+0.75v LUT range), device memory. */
int mrtx_synth_color(int32_t device, void* dst_dev_rgba8, int32_t h, int32_t w, uint32_t seed,
                     char* err, int32_t err_len);
/* Plain device allocation helpers so the host side needs no other GPU runtime for inputs. */
int mrtx_dev_alloc(int32_t device, uint64_t bytes, void** out);
int mrtx_dev_free(int32_t device, void* p);
int mrtx_dev_download(int32_t device, void* host_dst, const void* dev_src, uint64_t bytes);
int mrtx_dev_upload(int32_t device, void* dev_dst, const void* host_src, uint64_t bytes);

/* Profiling aid: streams a `bytes`-sized buffer `repeats` times with 8-byte-per-lane loads (the render kernel's
 * access width) so rocprofv3's FETCH_SIZE can be calibrated against a known byte count. */
int mrtx_probe_stream(int32_t device, uint64_t bytes, int32_t repeats);

/* Math conformance probe: evaluates the renderer's own (lat, lon) primitive -- polynomial atan2 pair sharing
 * one reciprocal -- on the device for n moon-frame points (tests compare it with the oracle bit for bit). */
int mrtx_probe_latlon(int32_t device, const float* a, const float* b, const float* c, float* lat, float* lon,
                      int32_t n);

/* ---- Sun illumination of the terrain (additive to ABI 7) ----------------------------------
 * The question the status bar answers with astro.sun_altitude_at over the smooth sphere (renderer_status.py:121-157):
 * is this spot lit, and how much of the Sun does it see -- here on the real terrain, under the light and Moon frame
 * last given to mrtx_set_light / mrtx_set_moon_frame, with the march parameters of mrtx_set_params.  Per node, float4:
 *   lit  fraction of the n_sun Sun samples with cos > 0 whose shadow ray escapes (the visible fraction of the disk);
 *   irr  (1/n_sun) * sum of what those samples carry: the D5 direct term per unit albedo;
 *   mu   n . l toward the light centre (signed; the incidence);
 *   D    the displacement factor at the node (local radius / R).
 * The result depends on neither the camera, the seed, spp, path_seg_range nor the capsules; the render state
 * (accumulation, hit buffer, samples done) is left exactly as it was.  n_sun is 1, 2, 4, ..., 64. */
typedef struct MrtxIllumGrid {
    double lat_north, lat_south;   /* degrees, lat_north > lat_south, both in [-90, 90]                           */
    double lon_west, lon_east;     /* degrees, lon_west < lon_east (may run past +-180: the DEM wraps in longitude) */
    int32_t h, w;                  /* cells of the whole map; node (i, j) is the centre of cell (i, j), row 0 north */
    int32_t row_begin, row_end;    /* the band computed by this call: rows [row_begin, row_end) of the map         */
    int32_t n_sun;
    int32_t reserved;              /* 0 */
} MrtxIllumGrid;
/* A lat/lon map, one band of rows per call: (row_end - row_begin) x w float4, row-major, into dev_out (a device buffer of
 * the context's device) and / or host_out (at least one of them).  Bands are independent: a map is the concatenation of
 * its bands.  out may be NULL. */
int mrtx_illum_grid(mrtx_ctx* ctx, const MrtxIllumGrid* grid, void* dev_out, float* host_out, MrtxStats* out);
/* The same at n arbitrary points: latlon_deg = n (lat, lon) pairs in degrees, host_out4 = n float4.  A point placed on a
 * grid node gives that node's output bit for bit -- the status bar's cursor query (renderer_status.py:121-157). */
int mrtx_illum_points(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_sun, float* host_out4, MrtxStats* out);
/* The deterministic Sun-sample table the two calls above use: n (u2, u3) float pairs (n = 1: the Sun's centre (0, 0);
 * otherwise the Fibonacci set u2 = (i + 1/2) / n, u3 = frac(i * 0.6180339887498949), float64 rounded once).  No GPU. */
int mrtx_illum_sun_samples(int32_t n, float* out2);

/* ---- Sun illumination over many dates (additive to ABI 7) ---------------------------------------
 * An epoch is what mrtx_set_light + mrtx_set_moon_frame would set for one date; the Moon radius and the march parameters
 * are the context's.  112 bytes. */
typedef struct MrtxIllumEpoch {
    double light_pos[3], light_radius, light_radiance;   /* as mrtx_set_light */
    double center[3], u[3], v[3];                         /* as mrtx_set_moon_frame (without the radius) */
} MrtxIllumEpoch;
/* Point p reads the `count` consecutive epochs first[p], ..., first[p] + count - 1 of epochs[0 .. n_epochs) (first = NULL:
 * every point reads [0, count)); points may repeat.  Output: n_points x count float4 (lit, irr, mu, D), point-major, into
 * dev_out (a device buffer of the context's device) and / or host_out (at least one of them).  Entry (p, j) equals, bit for
 * bit, mrtx_illum_points at point p after mrtx_set_light / mrtx_set_moon_frame were given epoch first[p] + j, and the
 * counters equal the sum of those calls'.  Needs a DEM, but neither mrtx_set_light nor mrtx_set_moon_frame; leaves the
 * context's light, Moon frame and render state as they were.  At most 2^31 outputs per call.  out may be NULL. */
int mrtx_illum_series(mrtx_ctx* ctx, const double* latlon_deg, int32_t n_points, const MrtxIllumEpoch* epochs,
                      int32_t n_epochs, const int32_t* first, int32_t count, int32_t n_sun, void* dev_out, float* host_out,
                      MrtxStats* out);

/* ---- Terrain horizons (additive to ABI 7) --------------------------------------------------------
 * Per point and azimuth a = 0 .. n_az-1 (a / n_az of a turn from north through east) the elevation, degrees, found by n_bis
 * bisection probes over [-90, +90]; each probe is an illumination sample's visibility decision from the point's lifted origin
 * (the vertex of mrtx_illum_points).  n_az a power of two in [4, 4096], n_bis in [1, 24].  Output: n x n_az float32,
 * point-major, into exactly one of dev_out (a device buffer of the context's device) and host_out.  Needs a DEM, but neither
 * mrtx_set_light nor mrtx_set_moon_frame; leaves the light, Moon frame and render state as they were.  At most 2^31 outputs
 * per call.  out may be NULL. */
int mrtx_horizon_points(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, int32_t n_bis, void* dev_out,
                        float* host_out, MrtxStats* out);
/* The Sun against those horizons: per (point, epoch) the fraction f of the light's disc above the
 * horizon, interpolated at the light's azimuth.  The horizons (n x n_az float32, as mrtx_horizon_points writes them) come
 * from exactly one of dev_horizon and host_horizon; the epochs are mrtx_illum_series's.  mode 0 (FULL): n x m float32 f,
 * point-major; mode 1 (SUMMARY): n float4 (mean f, share of epochs with f > 0, share with f == 1, longest run of consecutive
 * epochs with f == 0, in epochs).  Output into exactly one of dev_out and host_out.  m <= 2^24 (the run is a float count,
 * exact to there); FULL: at most 2^31 outputs per call. */
int mrtx_horizon_sun(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                     const float* host_horizon, const MrtxIllumEpoch* epochs, int32_t m, int32_t mode, void* dev_out,
                     float* host_out, MrtxStats* out);

/* ---- Regolith surface temperatures (additive to ABI 7) ------------------------------------------
 * One heat-conduction column per point, driven by the Sun against the point's horizon.  The layer tables are built on the host
 * in float64 (MoonRT.thermal_grid); node i sits at depth z_i, dz[i] = z_{i+1} - z_i (i < n_nodes - 1). */
#define MRTX_THERMAL_MAX_NODES 32
typedef struct MrtxThermalModel {
    int32_t n_nodes;              /* 3 .. MRTX_THERMAL_MAX_NODES                                                          */
    int32_t n_sub;                /* explicit steps per epoch: Delta = spacing_s / n_sub                                  */
    int32_t n_spin;               /* leading spin-up epochs: stepped, not recorded (< m outside FLUX)                     */
    int32_t block;                /* epochs per spin-up block (one lunation), >= 1                                        */
    int32_t n_reset;              /* after each of the first n_reset spin-up blocks the nodes below ref_node are set to
                                     the block's mean of T[ref_node]; n_reset * block <= n_spin                           */
    int32_t ref_node;             /* 1 .. n_nodes - 2                                                                     */
    double spacing_s;             /* epoch spacing, seconds                                                               */
    double dz[MRTX_THERMAL_MAX_NODES];    /* node spacings, m                                                             */
    double rho[MRTX_THERMAL_MAX_NODES];   /* density per node, kg m^-3                                                    */
    double kc[MRTX_THERMAL_MAX_NODES];    /* contact conductivity per node, W m^-1 K^-1                                   */
    double chi;                   /* radiative conductivity: k(T) = kc (1 + chi (T / 350)^3)                              */
    double c[5];                  /* heat capacity c0 + c1 T + c2 T^2 + c3 T^3 + c4 T^4, J kg^-1 K^-1                     */
    double emissivity, sigma;     /* eps, Stefan-Boltzmann constant                                                       */
    double q_geo;                 /* geothermal flux, W m^-2                                                              */
    double albedo[3];             /* A0, a, b: A(theta) = A0 + a (theta / 45 deg)^3 + b (theta / 90 deg)^8                */
} MrtxThermalModel;
/* Per point the absorbed flux Q_abs = (1 - A(theta)) S_k f max(mu, 0) of every epoch (f: mrtx_horizon_sun's disc fraction,
 * mu = n . l as mrtx_illum_points forms it, theta = acos(mu), S_k = flux_Wm2[k]) and the column stepped through the epochs
 * (DESIGN.md section 3.10).  Horizons and epochs as for mrtx_horizon_sun (exactly one horizon source); the epochs are evenly
 * spaced by model->spacing_s.  mode 0 (FULL): n x (m - n_spin) float32 surface temperatures after each recorded epoch,
 * point-major; 1 (SUMMARY): n float4 (max, min, mean surface temperature, mean bottom-node temperature over the recorded
 * epochs); 2 (FLUX): n x m float32 Q_abs, no stepping.  Output into exactly one of dev_out and host_out; at most 2^31 outputs
 * per call, m <= 2^24.  Needs a DEM; leaves the light, Moon frame and render state as they were.  out->reserved receives the
 * number of surface solves that reached the Newton cap (saturating), kernel_ms and launches as usual.  Refused before the
 * launch: q_geo < emissivity sigma 20^4 (a geothermal floor below 20 K) and a radiative equilibrium under the largest
 * absorbed flux above 450 K.  After each epoch's steps the kernel checks every point's column: if any node was non-finite
 * or outside [20, 450] K, the call returns MRTX_E_INVALID with the number of such (point, epoch)s, and the output is not
 * valid. */
int mrtx_thermal(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                 const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux_Wm2, int32_t m,
                 const MrtxThermalModel* model, int32_t mode, void* dev_out, float* host_out, MrtxStats* out);

/* ---- Terrain-scattered sunlight and infrared (additive to ABI 7) -----------------------------------
 * One bounce: a point's hemisphere is sampled with K fixed cosine-weighted rays; each terrain hit becomes a point with its own
 * horizon and column, whose per-epoch exitance (reflected sunlight + thermal emission) drives the first point's column as an
 * extra absorbed flux: Q_sec = the mean over the K rays of (1 - A_h) M_vis + eps M_ir, sky rays adding 0. */
/* The K (uh1, uh2) pairs of the view directions: uh1 = (j + 1/2) / K, uh2 = frac(j * 0.6180339887498949), float64 rounded once
 * to float32; K in {16, 32, ..., 1024}.  out2: 2K floats. */
int mrtx_view_dir_samples(int32_t k, float* out2);
/* Per point (latlon_deg: n (lat, lon) pairs, degrees) the K view rays from the lifted vertex of mrtx_horizon_points, mapped
 * about the normal as a path's continuation ray is and marched and refined as it is.  Output (exactly one of dev_out and
 * host_out): n x K float2 (lat, lon) in degrees of each ray's first terrain hit, NaN for a ray that leaves the bounding sphere,
 * point-major; then n float32 terrain view factors (hits / K).  Needs a DEM; leaves the light, Moon frame and render state as
 * they were.  With MRTX_F_COUNT_STATS: bounce_rays (= n K), height_samples (5 per ray for its vertex + every march step + the
 * bisections of a hit), dem_fetches, mip_fetches. */
int mrtx_view_hits(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t k, void* dev_out, float* host_out,
                   MrtxStats* out);
/* The gather: Q_sec[p][e] = (1/K) sum over j = 0 .. K-1 with index[p][j] >= 0, in that order, of
 * (1 - albedo_h) M_vis + emissivity M_ir of hit index[p][j] at epoch e, float32 (section 3.11).  index: n x K int32 host table
 * into the hit list, -1 for sky; exitance (exactly one of dev_exitance and host_exitance, exitance_len floats available):
 * n_hits x m float2 (M_vis, M_ir), point-major, as mrtx_thermal_scatter's EXITANCE writes it.  Output: n x m float32,
 * point-major, into exactly one of dev_out and host_out. */
int mrtx_scatter_flux(mrtx_ctx* ctx, const int32_t* index, int32_t n, int32_t k, const void* dev_exitance,
                      const float* host_exitance, int64_t exitance_len, int32_t n_hits, int32_t m, double albedo_h,
                      double emissivity, void* dev_out, float* host_out, MrtxStats* out);
/* mrtx_thermal with two additions (MrtxThermalModel and mrtx_thermal are unchanged).  An optional extra absorbed flux, n x m
 * float32 point-major (exactly one of dev_extra and host_extra, at least extra_len >= n x m entries, or neither: then every
 * mode equals mrtx_thermal's bit for bit), is added to Q_abs in every epoch, spin-up and the start included; FLUX reports the
 * sum.  mode 3 (EXITANCE): n x (m - n_spin) float2 (M_vis, M_ir) per recorded epoch k: M_vis = A(theta) S_k f max(mu, 0) the
 * sunlight the facet reflects in epoch k, M_ir = eps sigma T0^4 with T0 the surface temperature after epoch k's steps.
 * mrtx_thermal's checks apply; a host table's largest entry joins the 450 K check, while a device table is not scanned on
 * the host (too costly), so only the range check after the launch guards it. */
int mrtx_thermal_scatter(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                         const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux_Wm2, int32_t m,
                         const MrtxThermalModel* model, int32_t mode, const void* dev_extra, const float* host_extra,
                         int64_t extra_len, void* dev_out, float* host_out, MrtxStats* out);

/* ---- Subsurface temperature columns and ice-stability depths (additive to ABI 7) -----------------
 * The free sublimation rate of a volatile, kg m^-2 s^-1: ln E(T) = b[0] - b[1] / T + b[2] ln T + b[3] T (the vapour-pressure
 * law with the Hertz-Knudsen factor sqrt(M / (2 pi R T)) folded in by the host: moonrtx_amd.volatiles.law). */
typedef struct MrtxVolatile { double b[4]; } MrtxVolatile;
/* mrtx_thermal_scatter with two more modes (modes 0-3, species NULL: its outputs, counters, refusals and range flag, bit for
 * bit).  mode 4 (COLUMN): n x (m - n_spin) x n_nodes float32, point-major, then epoch, then node: (float)T_i of every node
 * after each recorded epoch's steps, where FULL samples node 0; at most 2^31 outputs per call.  mode 5 (VOLATILE, species
 * required): n x n_nodes x 2 float64, 8-byte aligned, point-major: per node (E_mean_i, T_max_i).  After each recorded epoch's
 * steps, per node: tf = (float)T_i, Td = (double)tf, x = fma(b3, Td, fma(b2, log(Td), b0 - b1 / Td)), S_i = S_i + exp(x) (a
 * float64 left fold from 0 in epoch order), M_i = fmaxf(M_i, tf); the output is S_i / (double)(m - n_spin) and (double)M_i.  E
 * is taken at the float32-rounded temperature, which is exactly what COLUMN stores; spin-up epochs contribute nothing.  The
 * extra-flux table, the host checks, out->reserved and the [20, 450] K range flag are mrtx_thermal_scatter's.  Refused: a
 * species outside mode 5 or none in it; a non-finite coefficient; a law that does not strictly increase on [20, 450] K
 * (b1 / T^2 + b2 / T + b3 > 0 on the 1 K grid); x(450 K) > 700; an unaligned dev_out in mode 5.  mrtx_thermal and
 * mrtx_thermal_scatter refuse modes 4 and 5.  Needs a DEM; leaves the light, Moon frame and render state as they were. */
int mrtx_thermal_column(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                        const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux_Wm2, int32_t m,
                        const MrtxThermalModel* model, int32_t mode, const void* dev_extra, const float* host_extra,
                        int64_t extra_len, const MrtxVolatile* species, void* dev_out, void* host_out, MrtxStats* out);

/* ---- Terrain line of sight (additive to ABI 7) --------------------------------------------------
 * An end is a surface point (lat, lon, degrees) raised h >= 0 metres along its radial unit vector u, from the lifted vertex of
 * mrtx_horizon_points: P = fmaf(hs, u, o) with hs = (float)(h / radius_m * R), R the context's Moon radius and radius_m the
 * metric radius of D = 1 (1737400 * the DEM's radius_scale).  A probe marches the segment between the target and the
 * observer from its lower end as a shadow ray is marched, ending before the far end.  Per target the output is the extra mast
 * height m, metres (float32), at which it sees the observer: 0 if it does at target_h_m, otherwise n_bis - 1 bisection probes
 * over [0, mast_max_m] after one at mast_max_m; +inf if the last probe at mast_max_m (or, n_bis = 0, at 0) is blocked.  So
 * n_bis = 0 is a plain viewshed: m is 0 or +inf.  Needs a DEM, neither a light nor a Moon frame; leaves the light, Moon frame
 * and render state as they were.  Output into exactly one of dev_out and host_out.  At most 2^31 outputs per call.  With
 * MRTX_F_COUNT_STATS: shadow_rays (probes), height_samples (10 per target for the two vertices + every march step),
 * dem_fetches, mip_fetches. */
typedef struct MrtxSightGrid {
    double obs_lat, obs_lon, obs_h_m;          /* the observer end */
    double target_h_m, mast_max_m, radius_m;   /* every target's height, the bisection's mast range, metres per D = 1 */
    double lat_north, lat_south, lon_west, lon_east;   /* as MrtxIllumGrid */
    int32_t h, w, row_begin, row_end;          /* as MrtxIllumGrid: one band of rows per call */
    int32_t n_bis;                             /* 0 .. 24 */
    int32_t reserved;                          /* 0 */
} MrtxSightGrid;
/* The targets are the nodes of a band of a lat/lon map (mrtx_illum_grid's nodes): (row_end - row_begin) x w float32,
 * row-major. */
int mrtx_sight_grid(mrtx_ctx* ctx, const MrtxSightGrid* grid, void* dev_out, float* host_out, MrtxStats* out);
/* The targets are n (lat, lon) pairs; observer_llh holds n_observers (lat, lon, h_m) triples: 1 (shared) or n (one per
 * target).  Output: n float32. */
int mrtx_sight_points(mrtx_ctx* ctx, const double* target_latlon, int32_t n, const double* observer_llh, int32_t n_observers,
                      double target_h_m, double mast_max_m, double radius_m, int32_t n_bis, void* dev_out, float* host_out,
                      MrtxStats* out);

/* ---- Least-cost traverses (additive to ABI 7) ----------------------------------------------------
 * A window of the DEM's own texel lattice: node (i, j), 0 <= i < rows, 0 <= j < cols, is texel (row0 + i stride,
 * (col0 + j stride) mod W) of the (H, W) DEM, its height that texel's D.  stride >= 1; the last row lies inside the DEM; the
 * columns are distinct ((cols - 1) stride < W).  wrap = 1 (only with cols stride == W and cols >= 3) joins column cols - 1 to
 * column 0.  No edge crosses the pole.  At most 2^31 nodes.  Each node has 8 neighbours, directions 0..7 = N, NE, E, SE, S,
 * SW, W, NW as the step from a node v to its neighbour u.  The edge u -> v weighs, in float32 in this order (section 3.13):
 *   dh = (D_v - D_u) * Rm;  g = dh / L;  not driven if |g| > max_grade;
 *   c = (L + climb * max(dh, 0)) + descent * max(-dh, 0);  m = 0.5 (P_u + P_v) (1 without penalties);  w = c * m;
 *   not driven if w is infinite.
 * Rm = (float)radius_m, the metres of D = 1; L = the edge's length from mrtx_traverse_lengths.  The cost field is float64, the
 * least fixed point of d[v] = min(src[v], min over u of d[u] + (double)w(u -> v)) (+inf where unreachable). */
typedef struct MrtxTraverse {
    int32_t row0, col0, rows, cols, stride, wrap;
    double radius_m;        /* metres of D = 1 (> 0) */
    double max_grade;       /* rise over run (> 0; +inf: no slope limit) */
    double climb_cost;      /* metres of cost per metre climbed (>= 0, finite) */
    double descent_cost;    /* metres of cost per metre descended (>= 0, finite) */
    int32_t reserved;       /* 0 */
} MrtxTraverse;
/* Host only, no context: the window's per-row float32 edge lengths, metres, rows x 3 floats (L_ew, L_ns, L_dg): L_ew[i] along
 * row i, L_ns[i] from row i to row i + 1, L_dg[i] from row i to row i + 1 one column over (0 in the last row).  Each is the
 * float64 great-circle distance between the two texel centres on a sphere of radius_m, rounded once to float32.  An N-S or
 * diagonal edge uses the length of its upper (northern) row.  MRTX_E_INVALID for a bad window or a length that is not a
 * finite positive float32. */
int mrtx_traverse_lengths(const MrtxTraverse* t, int32_t dem_h, int32_t dem_w, float* out3);
/* The cost field and the predecessors of a window from n_src >= 1 sources: src_ij = n_src (i, j) nodes, src_cost = their start
 * costs (finite, >= 0; null: all 0; duplicates: the smallest wins).  Penalties: at most one of dev_penalty / host_penalty,
 * rows x cols float32, each finite in [1e-3, 1e6] or +inf (impassable); a host table is checked before any device call, a
 * device table in the kernel (a bad entry: MRTX_E_INVALID after the launch).  Output: exactly one of dev_cost / host_cost
 * (rows x cols float64, 8-byte aligned) and exactly one of dev_pred / host_pred (rows x cols uint8); the device tables
 * must not overlap.  pred: 8 = a source whose cost is its
 * start cost; else the first direction k whose neighbour u is in the window with d[u] < d[v], a driven edge u -> v and
 * d[u] + (double)w(u -> v) == d[v]; 255 = unreachable, 254 = none found.  Needs a DEM, neither a light nor a Moon frame; leaves
 * the light, Moon frame and render state as they were.  out: launches (tile relaxation launches) and kernel_ms;
 * tile_visits (optional): workgroups that relaxed a tile, which depends on scheduling. */
int mrtx_traverse(mrtx_ctx* ctx, const MrtxTraverse* t, const int32_t* src_ij, const double* src_cost, int32_t n_src,
                  const void* dev_penalty, const float* host_penalty, void* dev_cost, double* host_cost, void* dev_pred,
                  uint8_t* host_pred, uint64_t* tile_visits, MrtxStats* out);
/* The window's node heights: rows x cols float32 D (texel (row0 + i stride, (col0 + j stride) mod W), read directly) into
 * exactly one of dev_out / host_out, so that a route's heights need not reach into the context's DEM later.  The window is
 * checked as mrtx_traverse checks it; needs a DEM.  out: launches, kernel_ms. */
int mrtx_traverse_heights(mrtx_ctx* ctx, const MrtxTraverse* t, void* dev_out, float* host_out, MrtxStats* out);

/* ---- Timed traverses: drive masks and earliest arrival (additive to ABI 7) -----------------------
 * mrtx_horizon_windows' joint predicate kept as bits.  Per point W64 = (m + 63) / 64 uint64 words, point-major: bit k & 63 of
 * word k >> 6 is `both` at epoch k, ok_a = f_a >= (float)min_a and ok_b = f_b >= (float)min_b with f mrtx_horizon_sun FULL's
 * value bit for bit (equality counts as met); with epochs_b NULL the bit is ok_a alone and min_b is ignored.  The bits past
 * epoch m - 1 are 0.  Arguments, limits, state and counters are mrtx_horizon_windows': m <= 2^24, min in (0, 1], exactly one
 * of each pointer pair, dev_out 8-byte aligned; needs a DEM, neither a light nor a Moon frame; leaves the render state alone. */
int mrtx_horizon_mask(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                      const float* host_horizon, const MrtxIllumEpoch* epochs_a, const MrtxIllumEpoch* epochs_b, int32_t m,
                      double min_a, double min_b, void* dev_out, uint64_t* host_out, MrtxStats* out);
/* Time in integer ticks.  An edge u -> v of mrtx_traverse's float32 weight w lasts q ticks: x = (double)w * ticks_per_cost (one
 * float64 product), q = 1 if x <= 1, else ceil(x); it is not driven if w is infinite or x > 2^31.  Tick t lies in epoch
 * t / ticks_per_epoch; node v is available in epoch e iff bit e of its row of the availability table is set (the layout of
 * mrtx_horizon_mask) and e < n_epochs.  Without a table every epoch is available and there is no end.  A drive that starts at
 * tick t occupies ticks t .. t + q - 1 and arrives at t + q; it is allowed iff all of its epochs are available at both u and
 * v.  Waiting at a node is free.  g_uv(a) = (the least t >= a at which the drive is allowed) + q, and the arrival field is the
 * least fixed point of A[v] = min(src[v], min over u of g_uv(A[u])); UINT64_MAX where unreachable. */
typedef struct MrtxTraverseTimed {
    double  ticks_per_cost;   /* ticks per unit of edge weight w (finite, > 0): e.g. 1 s ticks at 0.2 m/s -> 5 */
    int32_t ticks_per_epoch;  /* >= 1 */
    int32_t n_epochs;         /* epochs in the availability table, 1 .. 2^24 (ignored without a table) */
    int32_t reserved;         /* 0 */
} MrtxTraverseTimed;
/* The arrival field and its predecessors.  Window, sources, penalties, outputs, refusals and their order as mrtx_traverse's;
 * src_tick = the sources' start ticks (null: all 0; duplicates: the smallest wins; a source need not be available at its
 * start tick), each below n_epochs * ticks_per_epoch with a table and below 2^62 without.  At most one of dev_avail /
 * host_avail (rows x cols x W64 uint64, node-major, W64 = (n_epochs + 63) / 64; both null: no table), exactly one of
 * dev_arrival / host_arrival (rows x cols uint64) and of dev_pred / host_pred.  dev_avail and dev_arrival are 8-byte aligned;
 * no two device tables overlap.  pred: 8 = a source whose arrival is its start tick; else the first direction k whose
 * neighbour u is in the window with A[u] < A[v], a driven edge and g_uv(A[u]) == A[v]; 255 = unreachable, 254 = none found.
 * Also refused: a null tt, reserved != 0, ticks_per_cost not finite and > 0, ticks_per_epoch < 1, n_epochs out of range while
 * a table is given.  out and tile_visits as mrtx_traverse's. */
int mrtx_traverse_timed(mrtx_ctx* ctx, const MrtxTraverse* t, const MrtxTraverseTimed* tt, const int32_t* src_ij,
                        const uint64_t* src_tick, int32_t n_src, const void* dev_penalty, const float* host_penalty,
                        const void* dev_avail, const uint64_t* host_avail, void* dev_arrival, uint64_t* host_arrival,
                        void* dev_pred, uint8_t* host_pred, uint64_t* tile_visits, MrtxStats* out);

/* ---- Terrain relief: slope, roughness and landing hazard (additive to ABI 7) -----------------------
 * A window of the DEM's texel lattice as MrtxTraverse's, never wrapped: node (i, j) is texel (row0 + i stride,
 * (col0 + j stride) mod W); the last row lies inside the DEM and the columns are distinct.  A node's footprint is the
 * (2 ri + 1) x (2 rj + 1) lattice nodes (i + di, j + dj), |di| <= ri, |dj| <= rj, 1 <= ri, rj <= 32, (2 rj + 1) stride <= W,
 * read straight from the DEM: it may reach outside the window, its columns wrap modulo W, and a node whose footprint would
 * leave the DEM's rows [0, H) gets four NaNs -- so a node's bits do not depend on the window it is computed in.  Per node the
 * least-squares plane c + aj dj + ai di through z = (double)D - 1 over the footprint and the residual about it, all sums
 * float64 left folds in the order of section 3.14; output float4 (grade, rms_m, ge, gn): ge = aj kx[i] the gradient to the east
 * and gn = -(ai ky[i]) to the north (rise over run), grade = sqrtf((float)(ge ge + gn gn)), rms_m = the root mean square
 * residual in metres.  At most 2^31 nodes. */
typedef struct MrtxRelief {
    int32_t row0, col0, rows, cols, stride;
    int32_t ri, rj;         /* the footprint's half-heights in lattice nodes, 1 .. 32 */
    int32_t reserved;       /* 0 */
    double radius_m;        /* metres of D = 1 (> 0) */
} MrtxRelief;
/* Host only, no context: the window's per-row metric scales, rows x 2 float64 (kx, ky): kx[i] = radius_m over the distance
 * along row i between neighbouring lattice nodes, radius_m cos(lat_i) stride 2 pi / W, and ky[i] = radius_m over the N-S
 * distance between neighbouring lattice rows, radius_m stride pi / H; lat_i the latitude of row i's texel centres.  The window
 * and the footprint are checked against the (dem_h, dem_w) DEM as mrtx_relief checks them; MRTX_E_INVALID if they are bad or a
 * scale is not finite and positive. */
int mrtx_relief_scales(const MrtxRelief* r, int32_t dem_h, int32_t dem_w, double* out2);
/* The relief map of a window: rows x cols float4 into exactly one of dev_out (16-byte aligned) and host_out.  Needs a DEM,
 * neither a light nor a Moon frame; leaves the light, Moon frame and render state as they were.  out: launches, kernel_ms;
 * with MRTX_F_COUNT_STATS dem_fetches = the texels the definition reads, (2 ri + 1)(2 rj + 1) per node that is not NaN. */
int mrtx_relief(mrtx_ctx* ctx, const MrtxRelief* r, void* dev_out, float* host_out, MrtxStats* out);
/* The safe share of a landing ellipse over a relief map of rows x cols float4 (exactly one of dev_relief, 16-byte aligned, and
 * host_relief): per node (float)safe / (float)total, float32, where total counts the nodes of the (2 Ri + 1) x (2 Rj + 1) box
 * around it that lie inside the map (wrap = 1: column cols - 1 joins column 0, needs cols >= 3; a box wider than the circle
 * holds every column once) and safe those with grade <= grade_max and rms_m <= rms_max (a NaN node is unsafe).
 * 0 <= Ri, Rj <= 1024; the thresholds are >= 0 (+inf: no limit).  Output: rows x cols float32 into exactly one of dev_out and
 * host_out; device tables must not overlap.  Needs no DEM.  out: launches, kernel_ms. */
typedef struct MrtxReliefShare {
    int32_t rows, cols;
    int32_t Ri, Rj;         /* the box's half-heights in map nodes, 0 .. 1024 */
    int32_t wrap;           /* 1: the map closes the circle of longitude */
    int32_t reserved;       /* 0 */
    double grade_max;       /* rise over run */
    double rms_max;         /* metres */
} MrtxReliefShare;
int mrtx_relief_share(mrtx_ctx* ctx, const MrtxReliefShare* s, const void* dev_relief, const float* host_relief, void* dev_out,
                      float* host_out, MrtxStats* out);

/* ---- Connected regions of a per-node map (additive to ABI 7) ---------------------------------------
 * A lattice of rows x cols nodes, node (i, j) at index i cols + j, at most 2^31 nodes; wrap = 1 (needs cols >= 3) joins column
 * cols - 1 to column 0, as in MrtxTraverse and MrtxReliefShare.  The set is given by exactly one of a field, rows x cols x n_ch
 * float32 (1 <= n_ch <= 16): node in the set iff x >= (float)lo && x <= (float)hi for x = its channel ch (a NaN is out; lo =
 * -inf and hi = +inf are allowed; lo <= hi, neither NaN), and a mask, rows x cols uint8: nonzero is in (n_ch, ch, lo, hi are
 * not read then).  connectivity: 4 (N, E, S, W) or 8; no edge crosses the first or the last row.  A region is a connected
 * component of the set, its root its least node index; regions are numbered 0 .. K - 1 in ascending order of their roots. */
typedef struct MrtxRegions {
    int32_t rows, cols;
    int32_t wrap;           /* 1: column cols - 1 joins column 0 */
    int32_t connectivity;   /* 4 or 8 */
    int32_t n_ch, ch;       /* the field's channels and the one compared */
    double lo, hi;          /* the closed interval of the set, compared as float32 */
    int32_t reserved;       /* 0 */
} MrtxRegions;
/* One region of the catalogue, 56 bytes, all integers, so that it does not depend on the order of summation.  dj is a node's
 * column relative to its region's root: j - root_j, and with wrap ((j - root_j + cols / 2) mod cols) - cols / 2 (integer
 * division, non-negative mod). */
typedef struct MrtxRegion {
    uint64_t weight;        /* the sum of row_weight[i] over the region's nodes (= count without weights) */
    int64_t sum_i;          /* the sum of i */
    int64_t sum_dj;         /* the sum of dj */
    uint32_t count;         /* nodes */
    int32_t root_i, root_j; /* the root: the least node index */
    int32_t i_min, i_max;   /* row extent */
    int32_t dj_min, dj_max; /* column extent relative to the root's column */
    uint32_t reserved;      /* 0 */
} MrtxRegion;
/* The labels of the set's regions: rows x cols int32, the region's number or -1 outside the set, into exactly one of
 * dev_labels (4-byte aligned) and host_labels; *n_regions = K.  The input is exactly one of dev_field (4-byte aligned),
 * host_field, dev_mask and host_mask; a device input must not overlap dev_labels.  Needs no DEM, no light and no Moon frame,
 * and leaves the render state alone.  The number of launches depends on (rows, cols, wrap, connectivity) alone.  A refused
 * call leaves *n_regions as it was.  out: launches, kernel_ms. */
int mrtx_regions_label(mrtx_ctx* ctx, const MrtxRegions* r, const void* dev_field, const float* host_field, const void* dev_mask,
                       const uint8_t* host_mask, void* dev_labels, int32_t* host_labels, uint32_t* n_regions, MrtxStats* out);
/* The catalogue of a label table (exactly one of dev_labels, 4-byte aligned, and host_labels; it may be the caller's own):
 * n_regions records into exactly one of dev_out (8-byte aligned, not overlapping dev_labels) and host_out.  row_weight: rows
 * uint32 in host memory, the area of one node of row i in a unit of the caller's, or NULL: every node weighs 1.  Every entry
 * of the table is checked in the kernels: one >= n_regions or < -1 is never used as an index, and the call returns
 * MRTX_E_INVALID after the launch (the records are then not valid).  n_regions = 0 is valid: the table is checked and nothing
 * is written.  A number no node carries gives count = 0, root (-1, -1) and extents 0.  out: launches, kernel_ms. */
int mrtx_regions_stats(mrtx_ctx* ctx, int32_t rows, int32_t cols, int32_t wrap, const void* dev_labels, const int32_t* host_labels,
                       uint32_t n_regions, const uint32_t* row_weight, void* dev_out, MrtxRegion* host_out, MrtxStats* out);

/* ---- Zonal statistics and outlines of labelled regions (additive to ABI 7) -------------------------
 * What is inside each region of a label table and what shape it has.  Lattice, wrap, label tables and their bound checks are
 * mrtx_regions_stats': every entry is checked in the kernels, one >= n_regions or < -1 is never used as an index and gives
 * MRTX_E_INVALID after the launch; n_regions = 0 checks the table and writes nothing; a number no node carries gets an empty
 * record.  Both calls need no DEM, no light and no Moon frame and leave the render state alone; the number of launches depends
 * on the lattice, n_regions and the options alone.  Every result is exact: integer sums modulo 2^64 (counts modulo 2^32) and
 * float comparisons, nothing depends on the order of a reduction. */
typedef struct MrtxZonalSpec {
    int32_t rows, cols;
    int32_t wrap;           /* 0 or 1, checked as in mrtx_regions_stats (the statistics themselves do not depend on it) */
    int32_t n_ch;           /* the field's channels, 1 .. 16: every one gets a record per region */
    double scale;           /* the fixed point: q = llrint((double)x * scale), finite and > 0 */
    int32_t hist_ch;        /* the channel of the histogram, 0 .. n_ch - 1 (not read when n_bins = 0) */
    int32_t n_bins;         /* 0: no histogram; else 1 .. 4096 */
    double hist_lo;         /* the lower edge of bin 0, finite */
    double hist_inv_w;      /* bins per unit of the field, n_bins / (hi - lo): finite and > 0 */
    int32_t reserved;       /* 0 */
} MrtxZonalSpec;
/* One channel of one region, 56 bytes.  A NaN adds to n_nan only; every other value (the infinities too) is counted.  Its
 * fixed-point value is q = llrint((double)x * scale), one float64 product rounded half to even; when |(double)x * scale| >=
 * 2^31 the value adds to n_clipped and q is +-2^31 with the product's sign.  min, max and their places are taken in the total
 * order of the float32 bit patterns (-0.0 precedes +0.0), the least node index among equals. */
typedef struct MrtxZonal {
    uint64_t wcount;        /* the sum of row_weight[i] over the counted nodes (= count without weights) */
    int64_t wsum;           /* the sum of row_weight[i] * q, modulo 2^64 */
    int64_t sum;            /* the sum of q */
    uint32_t count;         /* counted nodes: the value is not NaN */
    uint32_t n_nan;
    uint32_t n_clipped;
    float min, max;         /* +inf and -inf when count == 0 */
    int32_t min_at, max_at; /* node index i cols + j of the extreme; -1 when count == 0 */
    uint32_t reserved;      /* 0 */
} MrtxZonal;
/* n_regions x n_ch records, region-major, into exactly one of dev_out (8-byte aligned) and host_out, of the field rows x cols
 * x n_ch float32 in exactly one of dev_field (4-byte aligned) and host_field, over the label table in exactly one of
 * dev_labels and host_labels.  row_weight: rows uint32 in host memory or NULL (every node weighs 1).  With n_bins > 0 also
 * n_regions x (n_bins + 2) uint64, at most 2^28 in all, into exactly one of dev_hist (8-byte aligned) and host_hist (both
 * NULL when n_bins = 0): a counted value of channel hist_ch adds its node's weight to column 0 when t = ((double)x - hist_lo)
 * * hist_inv_w < 0, to column n_bins + 1 when t >= n_bins, else to column 1 + floor(t) (one float64 subtraction, one float64
 * product).  No two device tables may overlap.  MOONRT_REGIONS_ZONAL = runs (default) | plain chooses between the in-wave
 * reduction of runs of one label and one set of atomics per node; both give the same bytes.  out: launches, kernel_ms. */
int mrtx_regions_zonal(mrtx_ctx* ctx, const MrtxZonalSpec* z, const void* dev_labels, const int32_t* host_labels,
                       uint32_t n_regions, const void* dev_field, const float* host_field, const uint32_t* row_weight,
                       void* dev_out, MrtxZonal* host_out, void* dev_hist, uint64_t* host_hist, MrtxStats* out);
/* One region's outline, 32 bytes.  A side of a node's cell is on the boundary when the node across it lies outside the lattice
 * or carries another label (-1 included); with wrap the node east of the last column is column 0; a north or south side is
 * never wrapped.  q1, q3, qd: the 2 x 2 windows of nodes (i - 1 .. i, j - 1 .. j), i = 0 .. rows, j = 0 .. cols (with wrap j =
 * 0 .. cols - 1, column j - 1 taken mod cols; nodes outside the lattice belong to no region), in which exactly one, exactly
 * three, and exactly the two nodes of one diagonal carry the region's label.  euler = (q1 - q3 + 2 qd) / 4 for connectivity 4
 * and (q1 - q3 - 2 qd) / 4 for 8 (Gray 1971): components minus holes. */
typedef struct MrtxRegionShape {
    uint64_t perimeter;     /* the sum of the lengths of the boundary sides */
    uint32_t sides_ns;      /* boundary sides that face north or south */
    uint32_t sides_ew;      /* boundary sides that face east or west */
    uint32_t q1, q3, qd;
    int32_t euler;
} MrtxRegionShape;
/* n_regions records into exactly one of dev_out (8-byte aligned, not overlapping dev_labels) and host_out.  side_ew: rows
 * uint32 in host memory, the length of the east and of the west side of a cell of row i; side_ns: rows + 1 uint32, entry i the
 * length of the side between rows i - 1 and i (entry 0 the north side of row 0, entry rows the south side of the last row);
 * both or neither, with neither every side counts 1.  connectivity: 4 or 8, the sense in which euler counts.  out: launches,
 * kernel_ms. */
int mrtx_regions_shape(mrtx_ctx* ctx, int32_t rows, int32_t cols, int32_t wrap, int32_t connectivity, const void* dev_labels,
                       const int32_t* host_labels, uint32_t n_regions, const uint32_t* side_ew, const uint32_t* side_ns,
                       void* dev_out, MrtxRegionShape* host_out, MrtxStats* out);

/* ---- Proximity maps and the reach of labelled regions (additive to ABI 7) --------------------------
 * Every node's nearest feature node and the exact squared distance to it, between node positions in three dimensions.  The
 * lattice is that of mrtx_regions_stats (at most 2^31 nodes, node (i, j) at index v = i cols + j) but has no wrap flag and no
 * metric of its own: the positions carry the geometry, so seam and pole need no special case.  Positions: three int32 (x, y, z)
 * per node in a unit of the caller's, every coordinate in -2^29 .. 2^29.  d2(u, v) = (xu - xv)^2 + (yu - yv)^2 + (zu - zv)^2 in
 * uint64, at most 3 x 2^60.  The features are the nodes with label >= 0 (MRTX_PROX_TO_SET) or with label < 0
 * (MRTX_PROX_TO_OUTSIDE).  For every node v, nearest[v] is the feature u that minimises (d2(u, v), u) lexicographically (ties
 * go to the least node index) and dist2[v] that d2; a feature node is treated like any other.  Without features nearest = -1
 * and dist2 = UINT64_MAX everywhere.  Nothing depends on the order of evaluation.  Both calls need no DEM, no light and no Moon
 * frame and leave the render state alone; the number of launches depends on the lattice and the variant alone. */
#define MRTX_PROX_TO_SET 0
#define MRTX_PROX_TO_OUTSIDE 1
typedef struct MrtxProximity {
    int32_t rows, cols;
    int32_t mode;           /* MRTX_PROX_TO_SET or MRTX_PROX_TO_OUTSIDE */
    int32_t reserved;       /* 0 */
} MrtxProximity;
/* Positions rows x cols x 3 int32 in exactly one of dev_pos and host_pos, labels rows x cols int32 in exactly one of dev_labels
 * and host_labels; nearest rows x cols int32 into exactly one of dev_nearest and host_nearest, dist2 rows x cols uint64 into
 * exactly one of dev_dist2 (8-byte aligned) and host_dist2; the other device tables are 4-byte aligned and no two device
 * tables may overlap.  A coordinate outside -2^29 .. 2^29 gives MRTX_E_INVALID: in a host table before any device call, in a
 * device table after the launch (the kernels clamp it, so nothing else goes wrong), as mrtx_traverse treats its penalties.
 * pairs (or NULL): the number of (node, feature) distance evaluations, the same from run to run.  MOONRT_PROXIMITY = prune
 * (default) | brute chooses between the scan that skips the feature tiles an integer bound proves too far and the scan of
 * every feature; both give the same bytes.  out: launches, kernel_ms. */
int mrtx_proximity(mrtx_ctx* ctx, const MrtxProximity* p, const void* dev_pos, const int32_t* host_pos, const void* dev_labels,
                   const int32_t* host_labels, void* dev_nearest, int32_t* host_nearest, void* dev_dist2, uint64_t* host_dist2,
                   uint64_t* pairs, MrtxStats* out);
/* The reach of one region, 32 bytes: the extremes of a dist2 table over the region's nodes, the least node index among equals. */
typedef struct MrtxRegionReach {
    uint64_t d2_max, d2_min;    /* over the region's nodes; 0 and UINT64_MAX when count == 0 */
    int32_t max_at, min_at;     /* least node index attaining each; -1 when count == 0 */
    int32_t min_nearest;        /* nearest[min_at]; -1 when count == 0 */
    uint32_t count;
} MrtxRegionReach;
/* n_regions records into exactly one of dev_out (8-byte aligned, overlapping no device input) and host_out, of any dist2 /
 * nearest pair (each in exactly one of its device and host pointer; dev_dist2 8-byte aligned) over any label table, checked as
 * in mrtx_regions_stats: an entry >= n_regions or < -1 is never used as an index and gives MRTX_E_INVALID after the launch;
 * n_regions = 0 checks the table and writes nothing.  On MRTX_PROX_TO_OUTSIDE distances of the regions' own labels d2_max and
 * max_at are the radius and the centre of the largest circle that fits in each region; on MRTX_PROX_TO_SET distances to another
 * set d2_min, min_at and min_nearest say how close each region comes to it, where, and to which of its nodes.  out: launches,
 * kernel_ms. */
int mrtx_regions_reach(mrtx_ctx* ctx, int32_t rows, int32_t cols, const void* dev_labels, const int32_t* host_labels,
                       uint32_t n_regions, const void* dev_dist2, const uint64_t* host_dist2, const void* dev_nearest,
                       const int32_t* host_nearest, void* dev_out, MrtxRegionReach* host_out, MrtxStats* out);

/* ---- Region outlines: the ordered boundary rings of a label table (additive to ABI 7) --------------
 * Lattice and labels are mrtx_regions_stats', with at most 2^28 nodes, so that every side id fits an int32.  The cell of node
 * (i, j) has the corners NW (y, x) = (i, j), NE (i, j + 1), SE (i + 1, j + 1), SW (i + 1, j).  Side k of node v has the id
 * 4 v + k and runs with the region on its right: 0 north NW -> NE, 1 east NE -> SE, 2 south SE -> SW, 3 west SW -> NW.  It is a
 * boundary side by mrtx_regions_shape's rule.  Successor of boundary side k of node (i, j) with label l: with the travel
 * direction T[k] = (0,1), (1,0), (0,-1), (-1,0), the outward direction D[k] = (-1,0), (0,1), (1,0), (0,-1), a = (i, j) + T[k]
 * and b = a + D[k] (columns mod cols under wrap; a node outside the lattice carries no label): side k - 1 of b when a and b
 * carry l (a left turn); side k of a when only a does (straight on); side k - 1 of b when only b does and connectivity is 8
 * (through the saddle); else side k + 1 of the same node (a right turn).  The successor map is a permutation of the boundary
 * sides and its cycles are the rings.  A ring's head is its least side id; rings are numbered by ascending head; a side's
 * position is its distance from the head along the successor map.  MRTX_OUTLINE_ALL: every side contributes its start corner.
 * MRTX_OUTLINE_CORNERS: only a side whose k differs from its predecessor's; a ring without a turn (a straight line all round a
 * wrapped window) contributes its head's start corner alone.  The vertex table holds (y, x) int32 pairs, ring after ring, each
 * ring from its head on.  x is unwrapped along the ring: the head's start corner has its natural column, every later vertex
 * the previous one plus the signed column steps of the sides between, so a ring across the seam is continuous and x may leave
 * 0 .. cols.
 * Exact for any label table, connected or not: (1) the areas of a label's rings add up to its MrtxRegion.count, (2) their
 * wareas to its MrtxRegion.weight, (3) their n_sides to sides_ns + sides_ew of its MrtxRegionShape, (4) its outer rings (wind
 * == 0, area > 0) minus its holes (wind == 0, area < 0) are MrtxRegionShape.euler at the same connectivity; winding rings
 * (wind != 0) count on neither side, so the number of hole rings is also right for a region that winds round the seam. */
#define MRTX_OUTLINE_ALL 0
#define MRTX_OUTLINE_CORNERS 1
typedef struct MrtxOutline {
    int32_t rows, cols, wrap;
    int32_t connectivity;   /* 4 or 8 */
    int32_t mode;           /* MRTX_OUTLINE_ALL or MRTX_OUTLINE_CORNERS */
    int32_t reserved;       /* 0 */
} MrtxOutline;
typedef struct MrtxRing {
    int64_t area;           /* the sum of i + 1 over the ring's south sides minus the sum of i over its north sides */
    int64_t warea;          /* the same with cw[i + 1] and cw[i], cw the exclusive prefix sum of row_weight */
    uint64_t first;         /* index of the ring's first vertex in the vertex table */
    uint32_t n_sides;
    uint32_t n_vertices;    /* in the chosen mode */
    int32_t label;
    int32_t head;           /* the least side id */
    int32_t wind;           /* (north sides - south sides) / cols: 0 without wrap, else -1, 0 or +1 */
    uint32_t reserved;      /* 0 */
} MrtxRing;
/* Labels in exactly one of dev_labels (4-byte aligned) and host_labels; row_weight: rows uint32 in host memory or NULL (every
 * row weighs 1 and warea == area).  *n_rings and *n_vertices receive the true totals whenever the label table passes its
 * checks.  With all four table pointers NULL and both caps 0 the call only counts.  Otherwise exactly one of dev_rings (8-byte
 * aligned) and host_rings and exactly one of dev_vertices (4-byte aligned) and host_vertices is given, with room for ring_cap
 * records and vertex_cap (y, x) pairs; no two device tables may overlap.  When both totals fit, the tables are written; when
 * either does not, nothing is written to either, the call returns MRTX_E_INVALID naming both needed sizes, and the counts are
 * still set.  A refused call leaves the two counts as they were.  The call needs no DEM, light or Moon frame and leaves the
 * render state alone.  MOONRT_REGIONS_OUTLINE = contract (default) | jump chooses between pointer jumping over the chains of
 * boundary sides inside tiles of 16 x 64 nodes and over every boundary side; both give the same bytes.  The number of launches
 * depends on the lattice, the options, the variant and the number of boundary sides alone.  out: launches, kernel_ms (from the
 * first launch to the last, the host's reads of the counts between them included); written also when the call fails for a
 * bad label, not when it is refused. */
int mrtx_regions_outline(mrtx_ctx* ctx, const MrtxOutline* o, const void* dev_labels, const int32_t* host_labels,
                         uint32_t n_regions, const uint32_t* row_weight, void* dev_rings, MrtxRing* host_rings, uint64_t ring_cap,
                         void* dev_vertices, int32_t* host_vertices, uint64_t vertex_cap, uint64_t* n_rings, uint64_t* n_vertices,
                         MrtxStats* out);

/* ---- Terrain depressions: fill levels and the basin catalogue (additive to ABI 7) -----------------
 * Lattice, wrap and connectivity are mrtx_regions_label's (at most 2^31 nodes, node (i, j) at index v = i cols + j, wrap joins
 * column cols - 1 to column 0 and needs cols >= 3, no edge crosses the first or the last row).  Heights z[v]: int32 in a unit of
 * the caller's, |z| <= 2^30.  Outlets: with edge_outlets = 1 every node of the first and of the last row and, without wrap, of
 * the first and of the last column; and every node whose byte in the optional uint8 outlet table is nonzero.  fill[v] is the
 * minimum, over all lattice paths from v to any outlet, of the maximum z on the path, both ends included; for an outlet fill =
 * z; without any outlet (an all-zero table with edge_outlets = 0) fill = MRTX_FILL_NONE everywhere.  depth = fill - z >= 0, and a
 * node is in a depression iff depth > 0.  Nothing depends on the order of evaluation.  Both calls need no DEM, no light and no
 * Moon frame and leave the render state alone. */
#define MRTX_FILL_NONE 2147483647
typedef struct MrtxFill {
    int32_t rows, cols, wrap;
    int32_t connectivity;   /* 4 or 8 */
    int32_t edge_outlets;   /* 0 or 1; 0 needs an outlet table */
    int32_t reserved;       /* 0 */
} MrtxFill;
/* Heights rows x cols int32 in exactly one of dev_z and host_z; the outlet table rows x cols uint8 in at most one of
 * dev_outlet and host_outlet (both NULL: none); the fill rows x cols int32 into exactly one of dev_fill and host_fill.  Device
 * int32 tables are 4-byte aligned and no two device tables may overlap.  A height beyond +-2^30 gives MRTX_E_INVALID: in a host
 * table at its first occurrence before any device call, in a device table after the launches (the kernels clamp it, so nothing
 * else goes wrong), as mrtx_proximity treats its coordinates.  MOONRT_FILL = tiles (default) | sweep chooses between the
 * relaxation in LDS tiles of 32 x 32 nodes, launched over the tiles whose surroundings changed, and one Jacobi step over the
 * whole lattice per launch; both give the same bytes.  visits (or NULL): the tile visits, or the node updates of the sweep;
 * with tiles it and the number of launches may differ from run to run.  There is no launch cap: every store lowers an int32.
 * out: launches, kernel_ms (from the first launch to the last, the host's reads of the change counter included). */
int mrtx_fill(mrtx_ctx* ctx, const MrtxFill* f, const void* dev_z, const int32_t* host_z, const void* dev_outlet,
              const uint8_t* host_outlet, void* dev_fill, int32_t* host_fill, uint64_t* visits, MrtxStats* out);
/* One region of a label table over a fill, 48 bytes.  The depth of a node is (int64)fill - z held in 0 .. INT32_MAX, so any fill
 * table is accepted.  pour_at is chosen among the nodes u that carry another label (-1 included) and are adjacent, in the given
 * connectivity and wrap, to a node of the region: the u that minimises (fill[u], u) lexicographically.  For a connected component
 * of {depth > 0} at the fill's connectivity, level_min == level_max == pour_level. */
typedef struct MrtxBasin {
    uint64_t weight;        /* the sum of row_weight[i] over the region's nodes */
    uint64_t volume;        /* the sum of row_weight[i] * depth, modulo 2^64 */
    uint32_t count;         /* nodes */
    int32_t level_min, level_max;   /* the extremes of fill over the region; INT32_MAX and INT32_MIN when count == 0 */
    int32_t depth_max;      /* the largest depth; 0 when count == 0 */
    int32_t deepest_at;     /* the least node index with the largest depth; -1 when count == 0 */
    int32_t pour_at;        /* -1 when no node qualifies: count == 0, or the region covers the whole lattice */
    int32_t pour_level;     /* fill[pour_at]; INT32_MAX when pour_at == -1 */
    uint32_t reserved;      /* 0 */
} MrtxBasin;
/* n_regions records into exactly one of dev_out (8-byte aligned, overlapping no device input) and host_out, of the heights and
 * the fill (each in exactly one of its device, 4-byte aligned, and host pointer) over any label table, checked as in
 * mrtx_regions_stats: an entry >= n_regions or < -1 is never used as an index and gives MRTX_E_INVALID after the launch;
 * n_regions = 0 checks the table and writes nothing.  Heights beyond +-2^30 are treated as in mrtx_fill.  row_weight: rows uint32
 * in host memory or NULL (every node weighs 1).  out: launches, kernel_ms. */
int mrtx_fill_basins(mrtx_ctx* ctx, int32_t rows, int32_t cols, int32_t wrap, int32_t connectivity, const void* dev_labels,
                     const int32_t* host_labels, uint32_t n_regions, const void* dev_z, const int32_t* host_z,
                     const void* dev_fill, const int32_t* host_fill, const uint32_t* row_weight, void* dev_out,
                     MrtxBasin* host_out, MrtxStats* out);

/* ---- The depression hierarchy: nested bowls, spill points, peak prominence (additive to ABI 7) ----
 * Lattice, wrap, connectivity, heights and outlets are mrtx_fill's.  key(v) = (z[v], v), compared lexicographically; the outside
 * is one virtual node below every key, adjacent to every outlet.  The nodes are taken in ascending key.  A node without a taken
 * neighbour that is no outlet gives birth to a leaf bowl.  A node that joins two or more closed components (components of taken
 * nodes that do not hold the outside) makes the current bowl of each spill there and gives birth to a meta bowl, their parent.
 * A node that is an outlet or touches an open component makes the current bowl of every closed component it touches spill with
 * parent = -1.  The region of a bowl is every node of its component taken strictly before its spill node, nested bowls
 * included.  label[v] is the innermost bowl that holds v: the current bowl of v's component just after v was taken, or -1.
 * Bowls are numbered by ascending key of born_at, so parent > child.  fill[v] == max(z[v], spill_level of the root bowl above
 * label[v]), and == z[v] where label[v] == -1.  invert = 1: all of the above for -z, the three levels reported negated back, so
 * that floor_level is a summit's height, spill_level its key col and floor_level - spill_level its prominence; volume is the
 * sum of row_weight (z - spill_level).  The call needs no DEM, no light and no Moon frame and leaves the render state alone. */
typedef struct MrtxBowls {
    int32_t rows, cols, wrap;
    int32_t connectivity;   /* 4 or 8 */
    int32_t edge_outlets;   /* 0 or 1 */
    int32_t invert;         /* 0: depressions; 1: peaks */
    int32_t reserved[2];    /* 0 */
} MrtxBowls;
typedef struct MrtxBowl {
    uint64_t weight;        /* the sum of row_weight[i] over the region */
    uint64_t volume;        /* the sum of row_weight[i] * (spill_level - z) over the region, modulo 2^64; 0 if it never spills */
    uint32_t count;         /* nodes of the region */
    uint32_t own_count;     /* nodes whose label is this bowl */
    int32_t floor_at, floor_level;  /* the least-key node of the region and its height */
    int32_t born_at, born_level;    /* the birth node and its height */
    int32_t spill_at, spill_level;  /* the spill node and its height; -1 and MRTX_FILL_NONE (-MRTX_FILL_NONE with invert) for a
                                     * bowl that never spills: only without any outlet */
    int32_t parent;         /* the parent bowl, or -1 */
    uint32_t n_children;    /* direct children; 0 for a leaf */
    uint32_t n_leaves;      /* leaf bowls in the region; 1 for a leaf */
    uint32_t reserved;      /* 0 */
} MrtxBowl;
/* Pointer pairs, alignment, overlap and heights beyond +-2^30 as in mrtx_fill (dev_bowls 8-byte aligned, dev_label 4-byte); edge_outlets = 0
 * needs an outlet table, and with an all-zero one no bowl ever spills.  row_weight: rows uint32 in host memory or NULL (every
 * node weighs 1).  The records go
 * into at most one of dev_bowls and host_bowls, which holds bowl_cap records.  With neither, bowl_cap must be 0 and so must both
 * label pointers: the call only counts.  When the records do not fit, nothing is written and the call returns MRTX_E_INVALID
 * naming the needed size; *n_bowls is set all the same.  The labels rows x cols int32 go into at most one of dev_label and
 * host_label (both NULL: no label table).  rounds (or NULL): the merge rounds of the device stage.  out: launches, kernel_ms (the
 * device phases; the host's sort and union-find over the minima between them is not counted).  A refused call leaves n_bowls,
 * rounds and out as they were. */
int mrtx_bowls(mrtx_ctx* ctx, const MrtxBowls* b, const void* dev_z, const int32_t* host_z, const void* dev_outlet,
               const uint8_t* host_outlet, const uint32_t* row_weight, void* dev_bowls, MrtxBowl* host_bowls, uint64_t bowl_cap,
               void* dev_label, int32_t* host_label, uint64_t* n_bowls, uint64_t* rounds, MrtxStats* out);

/* ---- Contour lines: the ordered isolines of a lattice at many levels (additive to ABI 7) ----------
 * Lattice and wrap are mrtx_regions_outline's (at most 2^28 nodes, node (i, j) at v = i cols + j).  Heights z[v]: int32 in
 * -2^30 .. 2^30, or MRTX_FILL_NONE for a void node.  Levels c[0] < c[1] < ...: n_levels int32 in host memory, each in -2^30 + 1 ..
 * 2^30.  At level c a node is above when z >= c and below when z < c, so the line is the isoline of c - 1/2 and no node lies
 * on a line.  Edge 2 v + 0 joins v to its east neighbour (column 0 after column cols - 1 under wrap, else absent there), edge
 * 2 v + 1 to its south neighbour (absent in the last row).  An edge is crossed at c when both its nodes are valid and exactly one
 * is above; the crossing lies at t = (2 c - 1 - 2 z_own) / (2 (z_other - z_own)) from the edge's own node v, strictly inside
 * (0, 1).  A vertex is its edge id.  Cell (i, j) has the corners NW (i, j), NE (i, j + 1), SE (i + 1, j + 1), SW (i + 1, j); it
 * exists for i < rows - 1 and j < cols - 1 (j < cols under wrap) and carries no segment when a corner is void.  Its sides run
 * clockwise, N NW -> NE, E NE -> SE, S SE -> SW, W SW -> NW; a crossed side a -> b is an entry when a is above and an exit when b
 * is.  A segment runs from an entry to an exit, the above side on its right (rows run down, columns right).  With two entries
 * the centre decides: z_NW + z_NE + z_SE + z_SW >= 4 c - 2 (centre above) pairs each entry with the next side clockwise, else with
 * the previous one.  An element is a pair (edge, level index); its successor is the exit paired with it in the cell it enters,
 * if that cell exists and has no void corner.  The components of this partial injection are the lines: cycles (closed) and
 * paths (open; a crossed edge between two cells that carry no segment is an open line of one vertex).  A line's head is its
 * start when it is open and its least (edge, level index) when it is closed; lines are numbered by ascending head; the vertex
 * table holds int32 edge ids, line after line, each line from its head along the successors, a closed line's head not
 * repeated.  The vertices of level index l are exactly the edges crossed at c[l], each once. */
typedef struct MrtxContours {
    int32_t rows, cols, wrap;
    int32_t n_levels;       /* 1 .. 65536 */
    int32_t reserved;       /* 0 */
} MrtxContours;
typedef struct MrtxContourLine {
    uint64_t first;         /* index of the line's first vertex in the vertex table */
    uint32_t n_vertices;
    int32_t level_index;    /* index into the level table */
    int32_t level;          /* the level c */
    int32_t head;           /* edge id of the first vertex */
    int32_t tail;           /* edge id of the last vertex */
    uint32_t closed;        /* 0 or 1 */
} MrtxContourLine;
/* Heights in exactly one of dev_z (4-byte aligned) and host_z.  *n_lines and *n_vertices receive the true totals whenever the
 * heights pass their check.  With all four table pointers NULL and both caps 0 the call only counts.  Otherwise exactly one of
 * dev_lines (8-byte aligned) and host_lines and exactly one of dev_vertices (4-byte aligned) and host_vertices is given, with room
 * for line_cap records and vertex_cap edge ids; no two device tables may overlap.  When both totals fit, the tables are written;
 * when either does not, nothing is written to either, the call returns MRTX_E_INVALID naming both needed sizes, and the counts
 * are still set.  A height outside the range gives MRTX_E_INVALID after the first launches (it is treated as void, so nothing
 * else goes wrong); 2^31 or more elements give MRTX_E_INVALID after the count.  A refused call leaves the two counts as they
 * were.  The call needs no DEM, light or Moon frame and leaves the render state alone.  The number of launches depends on the
 * lattice, n_levels and the number of elements alone.  out: launches, kernel_ms (from the first launch to the last, the host's
 * reads of the counts between them included); written also when the call fails for a bad height, not when it is refused. */
int mrtx_contours(mrtx_ctx* ctx, const MrtxContours* k, const void* dev_z, const int32_t* host_z, const int32_t* host_levels,
                  void* dev_lines, MrtxContourLine* host_lines, uint64_t line_cap, void* dev_vertices, int32_t* host_vertices,
                  uint64_t vertex_cap, uint64_t* n_lines, uint64_t* n_vertices, MrtxStats* out);

/* ---- Polygon rasterisation: rings and outlines burnt into a label table (additive to ABI 7) ---------
 * The inverse of mrtx_regions_outline.  Lattice, wrap and corner coordinates are that call's (at most 2^28 nodes): the cell of
 * node (i, j) has its NW corner at (y, x) = (i, j) and its centre at (i + 1/2, j + 1/2).  Vertices are (y, x) int32 pairs in
 * units of 2^-s of a cell, s = subcell_bits in 0 .. 8 (s = 0: exactly the outlines' coordinates), every coordinate within
 * +-2^24 units.  A ring's edges join consecutive vertices; the closing edge goes from the last vertex to (y_first, x_first +
 * wind cols 2^s), which must lie within +-2^25 units: the way MrtxRing.wind and the unwrapped x of the outline vertices read, so
 * a ring all the way round a wrapped window closes on the cylinder, and an MRTX_OUTLINE_CORNERS ring without a turn (one
 * vertex, wind = +-1) is one horizontal edge cols long.  polygon lies in 0 .. n_polygons - 1; a polygon's rings may come in any
 * order, and a polygon may have none.
 * The winding number of a node, with a ray from its centre straight towards row -infinity, in doubled units Y = 2 y, X = 2 x,
 * S = 2^s (unwrapped column ju has its centre at xc = (2 ju + 1) S, row i at yc = (2 i + 1) S): an edge (Y0, X0) -> (Y1, X1)
 * with X0 != X1 spans every ju with min(X0, X1) <= xc < max(X0, X1), where it sits at y* = Y0 + (xc - X0)(Y1 - Y0) / (X1 - X0);
 * the crossing counts for every row with yc >= y*, so from i0 = ceil((y* - S) / 2 S) on, in exact integers, with the sign +1
 * when X1 > X0 and -1 when X1 < X0.  The column is ju mod cols under wrap (an edge longer than cols hits a column more than
 * once, and each hit counts); without wrap a ju outside 0 .. cols - 1 is dropped.  i0 is clipped up to 0, a crossing with i0 >=
 * rows has no effect.  w_p(i, j) is the sum of the signs of polygon p's crossings of column j with i0 <= i.  Polygon p covers the
 * node when w_p != 0 (MRTX_RASTER_NONZERO) or when w_p is odd (MRTX_RASTER_EVENODD); a node centre on an edge shared by two
 * polygons belongs to exactly one of them.  labels[v]: the least (MRTX_RASTER_FIRST) or the greatest (MRTX_RASTER_LAST, the
 * painter's order) index among the polygons that cover v, or -1.  Rasterising the rings of mrtx_regions_outline, label as
 * polygon, gives back the label table they came from, at either connectivity, in either mode and under either rule. */
#define MRTX_RASTER_NONZERO 0
#define MRTX_RASTER_EVENODD 1
#define MRTX_RASTER_FIRST 0
#define MRTX_RASTER_LAST 1
typedef struct MrtxRaster {
    int32_t rows, cols, wrap;
    int32_t subcell_bits;   /* 0 .. 8 */
    int32_t rule;           /* MRTX_RASTER_NONZERO or MRTX_RASTER_EVENODD */
    int32_t order;          /* MRTX_RASTER_FIRST or MRTX_RASTER_LAST */
    int32_t reserved;       /* 0 */
} MrtxRaster;
typedef struct MrtxRasterRing {
    uint64_t first;         /* index of the ring's first vertex in the vertex table */
    uint32_t n_vertices;    /* >= 1 */
    int32_t polygon;
    int32_t wind;           /* 0 without wrap, else -1, 0 or +1 */
    uint32_t reserved;      /* 0 */
} MrtxRasterRing;
typedef struct MrtxPolygonCover {
    uint64_t weight;        /* the row_weight sum of the nodes the polygon covers */
    uint64_t owned_weight;  /* ... of the nodes whose label it is */
    uint32_t count;         /* the nodes the polygon covers */
    uint32_t owned;         /* the nodes whose label it is */
    int32_t i_min, i_max;   /* the row extent of the covered nodes, -1 when there are none */
    int32_t first_at;       /* the least covered node index, -1 when there is none */
    uint32_t reserved;      /* 0 */
} MrtxPolygonCover;
/* Every table in exactly one of its device pointer (rings and cover 8-byte, vertices and labels 4-byte aligned) and its host
 * pointer; a table without entries (n_rings, n_vertices or n_polygons == 0) may come without either.  The two inputs may share
 * memory; no other two device tables may overlap.  row_weight: rows uint32 in host memory or NULL (every row weighs 1).
 * labels: rows x cols int32; cover: n_polygons records.  n_polygons == 0 or n_rings == 0 is legal and gives an all -1 table.
 * n_rings and n_vertices stay below 2^31, and n_polygons x ceil(cols / 64) at or below 2^28.  The two input tables are checked
 * on the device: a record with polygon out of range, first + n_vertices beyond the table, n_vertices == 0, a wind that is not
 * allowed (or whose closing point leaves +-2^25), reserved != 0, or a coordinate beyond +-2^24 gives MRTX_E_INVALID after the
 * first launches, with the count of each in the message, and nothing is written; so do 2^31 or more edges or crossings, after
 * their count.  *n_crossings (may be NULL) receives the number of (edge, column) hits inside the lattice.  A refused call
 * leaves outputs, the count and the statistics as they were.  The call needs no DEM, light or Moon frame and leaves the render
 * state alone.  MOONRT_RASTER = bins (default) | brute chooses between crossings gathered per polygon and strip of 64 columns and
 * every node against every edge; both give the same bytes, the same on every run.  The number of launches depends on the variant
 * alone.  out: launches, kernel_ms (from the first launch to the last, the host's reads of the counts between them included);
 * written also when the call fails for a bad table, not when it is refused. */
int mrtx_rasterise(mrtx_ctx* ctx, const MrtxRaster* r, const void* dev_rings, const MrtxRasterRing* host_rings, uint64_t n_rings,
                   const void* dev_vertices, const int32_t* host_vertices, uint64_t n_vertices, uint32_t n_polygons,
                   const uint32_t* row_weight, void* dev_labels, int32_t* host_labels, void* dev_cover,
                   MrtxPolygonCover* host_cover, uint64_t* n_crossings, MrtxStats* out);

/* ---- Mast-height horizons and joint windows (additive to ABI 7) ----------------------------------
 * mrtx_horizon_points from a raised origin: point p marches from P = fmaf(hs, u, o), hs = (float)(height_m[p] / radius_m * R),
 * the raised end of mrtx_sight_points (so a mast top is one point for the horizon and for the line of sight).  height_m: n
 * doubles, each finite in [0, 1e4] metres; radius_m > 0 the metres of D = 1.  Azimuths, bisection and probe directions are
 * mrtx_horizon_points'; a point with hs == 0 is that call's bit for bit (output and counters), a point with hs > 0 marches
 * every probe (no n . d > 0 test: a mast top sees below its facet's plane, and the horizon's dip is negative), from where the
 * probe enters the bounding sphere when P lies outside it (clear when it misses the sphere).  Output, limits and state as
 * mrtx_horizon_points: n x n_az float32 into exactly one of dev_out and host_out.  out may be NULL. */
int mrtx_horizon_raised(mrtx_ctx* ctx, const double* latlon_deg, const double* height_m, double radius_m, int32_t n,
                        int32_t n_az, int32_t n_bis, void* dev_out, float* host_out, MrtxStats* out);
/* Two bodies against one set of horizons, reduced per point: f_a and f_b are, bit for bit,
 * mrtx_horizon_sun FULL's fractions for the epoch tables epochs_a and epochs_b (m epochs each, the same dates); per epoch
 * ok_a = f_a >= (float)min_a, ok_b = f_b >= (float)min_b, both = ok_a && ok_b.  min_a, min_b in (0, 1]; m <= 2^24;
 * horizons from exactly one of dev_horizon and host_horizon.  Output: n x 8 float32, point-major, into exactly one of dev_out
 * (16-byte aligned) and host_out:
 *   [0] share of epochs with ok_a        [1] longest run of consecutive epochs with !ok_a
 *   [2] share with ok_b                  [3] longest run with !ok_b
 *   [4] share with both                  [5] longest run with both
 *   [6] index of the first epoch of that run (the earliest such run; -1 if [5] is 0)
 *   [7] longest run with !both
 * Shares are (float)(count / (double)m); runs and the index are exact float counts.  No n x m buffer is allocated.  Needs a
 * DEM, but neither a light nor a Moon frame; leaves the light, Moon frame and render state as they were.  out: launches,
 * kernel_ms. */
int mrtx_horizon_windows(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                         const float* host_horizon, const MrtxIllumEpoch* epochs_a, const MrtxIllumEpoch* epochs_b, int32_t m,
                         double min_a, double min_b, void* dev_out, float* host_out, MrtxStats* out);

/* ---- Site power budgets (additive to ABI 7) --------------------------------------------------------
 * Does an asset survive at a site, and on how much battery?  Energy is counted in integers: one count is 2^-cpw_log2 W times
 * the epoch spacing. */
#define MRTX_PANEL_TRACK   0   /* two-axis tracking: c = 1                                                              */
#define MRTX_PANEL_FIXED   1   /* a fixed panel with unit normal normal_enu: c = max(0, n . l)                          */
#define MRTX_PANEL_AZIMUTH 2   /* a vertical panel turned toward the Sun's azimuth: c = min(1, cos of the Sun's elevation) */
typedef struct MrtxPowerModel {
    int32_t panel;          /* MRTX_PANEL_*                                                                              */
    double normal_enu[3];   /* FIXED: the panel's normal in local (east, north, up) of each point, any length > 0        */
    int32_t cpw_log2;       /* counts per watt = 2^cpw_log2, in [-20, 20]                                                */
    int64_t capacity;       /* the battery, counts: 0 <= initial <= capacity <= 2^52                                     */
    int64_t initial;        /* its charge before epoch 0, counts                                                         */
} MrtxPowerModel;
/* Horizons, epochs and points as for mrtx_horizon_sun (exactly one of dev_horizon and host_horizon; m <= 2^24).  gen_w[k] is
 * the power in watts the array delivers facing the whole unobstructed Sun at epoch k, load_w[k] the power drawn during it: m
 * doubles each, finite, >= 0 and at most 2^28 counts after scaling.  Per (point, epoch), in float32: f = mrtx_horizon_sun
 * FULL's fraction bit for bit, c the panel's factor from the Sun's direction in the point's frame,
 *   G_k = (int32)rintf((((float)gen_w[k] * f) * c) * 2^cpw_log2),  L_k = (int32)rintf((float)load_w[k] * 2^cpw_log2),
 * e_k = G_k - L_k; from there on int64.  mode 0 (FULL): n x m int32 G_k, point-major, at most 2^31 outputs per call.  mode 1
 * (SUMMARY): n x 8 int64, point-major (dev_out 16-byte aligned); with S_j = e_0 + ... + e_j (S_-1 = 0), s_-1 = initial,
 * t_k = s_{k-1} + e_k and s_k = min(capacity, max(0, t_k)):
 *   [0] sum of G_k                          [1] S_{m-1}
 *   [2] D = max(0, max_j (max_{-1 <= i < j} S_i - S_j)): the least capacity which, starting full, never empties
 *   [3] first and [4] last epoch of that drawdown ([4] the smallest j that attains D, [3] = i + 1 for the latest i < j with
 *       S_i maximal; both -1 if D == 0)
 *   [5] min_k s_k     [6] epochs with t_k < 0 (load not met)     [7] sum of max(0, -t_k) (energy not delivered)
 * Output into exactly one of dev_out and host_out; no n x m buffer is allocated in SUMMARY.  Needs a DEM, but neither a light
 * nor a Moon frame; leaves the light, Moon frame and render state as they were.  out: launches, kernel_ms. */
int mrtx_power_budget(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                      const float* host_horizon, const MrtxIllumEpoch* epochs, const double* gen_w, const double* load_w,
                      int32_t m, const MrtxPowerModel* model, int32_t mode, void* dev_out, void* host_out, MrtxStats* out);

/* ---- The Earth's occultation of the Sun (additive to ABI 7) ----------------------------------------
 * Per (point, epoch) the share g in [0, 1] of the source's disc that the body's disc leaves uncovered, seen from the lifted
 * vertex of mrtx_horizon_points: the geometric discs of epochs_source (the Sun moved out to its true distance:
 * moonrtx_amd.ephemeris.far_sun_epochs) and epochs_body (the Earth: earth_epochs), m rows each for the same dates, by the
 * planar two-disc rule of section 3.18 in float32.  No atmosphere.  The host marks in float64 the epochs in which no point of
 * the Moon's bounding sphere can see the discs overlap; those take g = 1, the value the rule would give, without being formed.
 * m <= 2^24.  mode 0 (FULL): n x m float32, point-major, at most 2^31 outputs per call.  mode 1 (SUMMARY): n x 8 float32,
 * point-major (dev_out 16-byte aligned), no n x m buffer:
 *   [0] mean g                                   [1] min g
 *   [2] share of epochs with g < 1               [3] share with g == 0          (both (float)(count / (double)m))
 *   [4] longest run of consecutive epochs with g < 1
 *   [5] index of the first epoch of that run (the earliest such run; -1 if [4] is 0)
 *   [6] longest run with g == 0                  [7] number of maximal runs of g < 1: the eclipses the point saw
 * Output into exactly one of dev_out and host_out.  Refused with MRTX_E_INVALID before any launch: a null table, m < 1, a
 * non-finite entry, a negative source radius, a body radius <= 0, a body whose centre is nearer to the Moon's centre than the
 * bounding sphere plus its own radius, a body that is not nearer than the source from every point of the bounding sphere, a
 * bad mode, both or neither output, a misaligned dev_out in SUMMARY.  Needs a DEM, but neither a light nor a Moon frame;
 * leaves the light, Moon frame and render state as they were.  out: launches, kernel_ms. */
int mrtx_occultation(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, const MrtxIllumEpoch* epochs_source,
                     const MrtxIllumEpoch* epochs_body, int32_t m, int32_t mode, void* dev_out, float* host_out, MrtxStats* out);
/* mrtx_thermal_column under that occultation.  occ_source and occ_body: both NULL (then mrtx_thermal_column bit for bit in
 * every mode: outputs, counters, refusals, range flag) or both given, m rows each, checked as mrtx_occultation checks them.
 * With the tables the disc fraction f of every epoch k, spin-up included, becomes f * g_k with g_k mrtx_occultation's value at
 * the point for epoch k: in Q_abs, in FLUX and in EXITANCE's M_vis.  The product is exact where the terrain hides nothing of
 * the disc and an approximation elsewhere (section 3.18). */
int mrtx_thermal_occulted(mrtx_ctx* ctx, const double* latlon_deg, int32_t n, int32_t n_az, const void* dev_horizon,
                          const float* host_horizon, const MrtxIllumEpoch* epochs, const double* flux_Wm2, int32_t m,
                          const MrtxThermalModel* model, int32_t mode, const void* dev_extra, const float* host_extra,
                          int64_t extra_len, const MrtxVolatile* species, const MrtxIllumEpoch* occ_source,
                          const MrtxIllumEpoch* occ_body, void* dev_out, void* host_out, MrtxStats* out);

/* ---- Orbiter passes: relay contact windows against terrain horizons (additive to ABI 7) ------------
 * When can a point talk to a relay orbiter?  S satellites, each a table of m positions in the Moon-fixed frame (the library's
 * body axes: x = r cos(lat) sin(lon), y = r cos(lat) cos(lon), z = r sin(lat); metres), against the horizons of
 * mrtx_horizon_points / mrtx_horizon_raised.  A satellite is a point source: in view iff its margin g > 0. */
#define MRTX_PASSES_FULL    0
#define MRTX_PASSES_SUMMARY 1
#define MRTX_PASSES_LIST    2
typedef struct MrtxPasses {
    int32_t n_sat;          /* S in [1, 256]                                                                             */
    int32_t m;              /* epochs per satellite, 1 .. 2^24; S * m <= 2^24                                            */
    int32_t mode;           /* MRTX_PASSES_*                                                                             */
    int32_t reserved;       /* 0                                                                                         */
    double  radius_m;       /* metres of D = 1 (> 0), as mrtx_horizon_raised                                             */
    double  min_elev_deg;   /* elevation mask above the local horizontal, in [-90, 90)                                   */
} MrtxPasses;
typedef struct MrtxPass {   /* 40 bytes */
    int32_t point, sat, first, count;   /* epochs first .. first + count - 1 have g > 0                                  */
    int32_t max_at;                     /* earliest epoch of the pass's greatest elevation                               */
    uint32_t flags;                     /* bit 0: begins at epoch 0, bit 1: ends at epoch m - 1 (open ends)              */
    float rise_frac, set_frac;          /* AOS = first - rise_frac, LOS = first + count - 1 + set_frac, in epochs        */
    float max_elev_deg, min_range_m;
} MrtxPass;
/* Points, horizons, n_az and "exactly one of dev_horizon and host_horizon" as mrtx_horizon_windows; height_m (NULL: the ground)
 * as mrtx_horizon_raised: per point in [0, 1e4] metres, the direction to a satellite is taken from P = fmaf(hs, u, o), and NULL
 * and all-zero heights give the same bits.  sat_pos_m: S x m x 3 doubles; each component becomes (float)(x / radius_m * R).
 * Per (point, satellite, epoch) in float32: t = X - P, range = |t|, the unit direction, its elevation es and azimuth and the
 * interpolated horizon hh exactly as mrtx_horizon_sun forms them for a light's centre; g = es - fmaxf(hh, (float)min_elev_deg).
 *   FULL     n x S x m float4 (es deg, azimuth deg in [0, 360), range in metres = range * (float)(radius_m / R), g), point-major
 *            then satellite; at most 2^27 outputs per call; into exactly one of dev_out (16-byte aligned) and host_out.
 *   SUMMARY  n x 8 float32 (dev_out 16-byte aligned), no n x S x m table; with c_k the number of satellites in view at epoch k:
 *            [0] share of epochs with c_k >= 1             [1] longest run with c_k == 0 (the longest outage)
 *            [2] longest run with c_k >= 1                 [3] first epoch of that run (the earliest such run; -1 if none)
 *            [4] number of maximal runs of c_k >= 1        [5] greatest es over all in-view (s, k); -90 if none
 *            [6] (float)(sum of c_k / (double)m)           [7] share of epochs with c_k >= 2
 *            Shares are (float)(count / (double)m); runs and indices are exact float counts.
 *   LIST     MrtxPass records, one per maximal run of g > 0 of one (point, satellite), in ascending (point, sat, first).  With
 *            g_a = g[first - 1] <= 0 < g_b = g[first]: rise_frac = g_b / (g_b - g_a) (0 with flag bit 0 when first == 0);
 *            set_frac = g_l / (g_l - g_n) from the last epoch's margin and the next one's (0 with flag bit 1 at m - 1);
 *            max_elev_deg, max_at and min_range_m over the pass's own epochs.  *n_passes always receives the true total; with
 *            dev_out == host_out == NULL and pass_cap == 0 the call only counts; when the total exceeds pass_cap nothing is
 *            written and the call returns MRTX_E_INVALID naming the needed size.  dev_out 8-byte aligned.
 * pass_cap and n_passes are read in LIST only (n_passes may be NULL otherwise).  Refused with MRTX_E_INVALID before any launch:
 * a non-finite position, a position within the Moon's bounding sphere (mrtx_occultation's) plus the largest raise, S * m > 2^24,
 * a bad mode, both outputs or (outside a LIST count) neither, a misaligned dev_out.  Needs a DEM, but neither a light nor a Moon
 * frame; leaves the light, Moon frame and render state as they were.  out: launches, kernel_ms. */
int mrtx_horizon_passes(mrtx_ctx* ctx, const MrtxPasses* k, const double* latlon_deg, const double* height_m, int32_t n,
                        int32_t n_az, const void* dev_horizon, const float* host_horizon, const double* sat_pos_m, void* dev_out,
                        void* host_out, uint64_t pass_cap, uint64_t* n_passes, MrtxStats* out);

/* ---- Joint availability of mask rows: site pairs and the step of greedy site sets (additive to ABI 7)
 * Rows of W64 = (m + 63) / 64 uint64 words in mrtx_horizon_mask's layout, 1 <= m <= 2^24: table A of n_a rows, table B of n_b
 * rows; with n_b == 0 and both B pointers null B is A itself.  1 <= n_a, n_b <= 2^24 and n W64 < 2^31 per table.  The bits past
 * epoch m - 1 of any input row are ignored and may hold garbage, as mrtx_traverse_timed allows.  Joint word w of pair (a, b):
 * J = ((A[a][w] OP B[b][w]) | base[w]) & V_w with OP = OR (MRTX_PAIRS_ANY: either site available) or AND (MRTX_PAIRS_BOTH: both at
 * once), base an optional single row (the union of the sites already chosen; null: 0) and V_w all ones but in the last word,
 * where it keeps bits 0 .. m - 1 - 64 (W64 - 1).  Per pair: count = the set bits of J (uint32); gap = the length of the longest
 * run of consecutive epochs in [0, m) whose bit is clear (uint32); gap_first = the first epoch of the earliest such run (int32);
 * with every epoch set gap = 0 and gap_first = -1.
 * Eligibility: without positions every pair, but a == b when B is A.  Positions are three int32 per row as mrtx_proximity's, each
 * coordinate in -2^29 .. 2^29, d2 in uint64; with them a pair is eligible iff additionally d2_min <= d2(a, b) <= d2_max, both
 * ends inclusive (d2_min and d2_max are ignored without positions).
 *   MRTX_PAIRS_ROWS   B and positions must be null.  n_a records of 16 bytes {int32 partner = -1; uint32 count; uint32 gap;
 *                     int32 gap_first} of (A[a] | base) & V; op and rank are ignored.  The statistics of any mask row, and the
 *                     step of a greedy extension: every candidate against the union so far.
 *   MRTX_PAIRS_BEST   n_a records of the same 16 bytes: partner = the eligible b that is first under the rank, the other fields
 *                     that pair's.  MRTX_PAIRS_BY_COUNT: largest count, then smallest gap, then least b; MRTX_PAIRS_BY_GAP:
 *                     smallest gap, then largest count, then least b.  Without an eligible partner {-1, 0, 0, -1}.
 *   MRTX_PAIRS_TABLE  n_a x n_b records of 8 bytes {uint32 count; uint32 gap}, row-major (n_a x n_a when B is A); an ineligible
 *                     pair gets {0xFFFFFFFF, 0xFFFFFFFF}; n_a n_b <= 2^28.  rank is ignored.
 * Nothing depends on the order of evaluation: two runs give the same bytes. */
#define MRTX_PAIRS_ANY  0
#define MRTX_PAIRS_BOTH 1
#define MRTX_PAIRS_ROWS  0
#define MRTX_PAIRS_BEST  1
#define MRTX_PAIRS_TABLE 2
#define MRTX_PAIRS_BY_COUNT 0
#define MRTX_PAIRS_BY_GAP   1
typedef struct MrtxMaskPairs {
    int32_t n_a, n_b, m;
    int32_t op, mode, rank;     /* MRTX_PAIRS_ANY / BOTH, MRTX_PAIRS_ROWS / BEST / TABLE, MRTX_PAIRS_BY_COUNT / BY_GAP */
    int32_t reserved[2];        /* 0 */
    uint64_t d2_min, d2_max;
} MrtxMaskPairs;                /* 48 bytes */
/* Exactly one pointer of each required pair (a, out), at most one of each optional pair (b, base, pos_a, pos_b); a B table iff
 * n_b > 0; pos_b is given iff pos_a is given and B is not A.  Device tables of words and dev_out are 8-byte aligned, positions
 * 4-byte aligned; no device output overlaps a device input.  A coordinate outside -2^29 .. 2^29 gives MRTX_E_INVALID: in a host
 * table before any device call, in a device table after the launch (the kernels clamp it, so nothing else goes wrong), as
 * mrtx_proximity does.  pairs (or NULL): the number of eligible pairs evaluated -- ordered pairs when B is A, n_a in ROWS -- the
 * same from run to run and in both variants.  MOONRT_PAIRS = prune (default) | brute chooses between skipping the pairs of row
 * tiles that an exact integer box-to-box bound proves ineligible and looking at every tile pair; both give the same bytes and
 * the same pairs.  Needs no DEM, no light and no Moon frame and leaves the render state alone; the number of launches depends
 * on the arguments alone.  out: launches, kernel_ms. */
int mrtx_mask_pairs(mrtx_ctx* ctx, const MrtxMaskPairs* p, const void* dev_a, const uint64_t* host_a, const void* dev_b,
                    const uint64_t* host_b, const void* dev_base, const uint64_t* host_base, const void* dev_pos_a,
                    const int32_t* host_pos_a, const void* dev_pos_b, const int32_t* host_pos_b, void* dev_out, void* host_out,
                    uint64_t* pairs, MrtxStats* out);

/* Math conformance probe (ABI 7): the kernels' domain-restricted reciprocal (v_rcp_f32 + Newton steps) and square root (v_sqrt_f32 + a
 * +-1 ulp residual fix) against the compiler's IEEE expansions of 1.0f / x and sqrtf(x), ON THE DEVICE, for the n float bit patterns
 * from lo_bits on: which = 0 one Newton step, 1 two steps (what the kernels use), 2 the square root.  mismatches = how many differ;
 * first_bad_bits = the smallest bit pattern that does (0 if none).  The whole domain is 2^32 patterns: seconds. */
int mrtx_probe_cr(int32_t device, int32_t which, uint32_t lo_bits, uint64_t n, uint64_t* mismatches, uint32_t* first_bad_bits);

#ifdef __cplusplus
}
#endif
#endif /* MOONRT_H */
