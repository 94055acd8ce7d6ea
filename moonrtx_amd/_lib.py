"""ctypes loader for libmoonrt.so (the C ABI of include/moonrt.h).

The library is built in-tree by `moonrtx_amd.build.build_native()` / `make -C moonrtx_amd/csrc`.
There is NO CPU fallback: if the shared object is missing or a symbol is absent this module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOONRT_LIB") or os.path.join(_HERE, "libmoonrt.so")   # MOONRT_LIB: A/B builds only

ABI_VERSION = 7


class MrtxConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("rank", C.c_int32), ("world", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32)]


class MrtxParams(C.Structure):
    _fields_ = [("scene_epsilon", C.c_float), ("marching_step", C.c_float), ("marching_step_eps", C.c_float),
                ("tonemap_exposure", C.c_float), ("tonemap_gamma", C.c_float),
                ("path_seg_min", C.c_uint32), ("path_seg_max", C.c_uint32),
                ("spp_per_launch", C.c_uint32), ("max_spp", C.c_uint32), ("seed", C.c_uint32),
                ("const_albedo", C.c_float * 3), ("flags", C.c_uint32)]


class MrtxStats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("primary_hits", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("height_samples", C.c_uint64), ("colour_fetches", C.c_uint64),
                ("background_fetches", C.c_uint64), ("dem_fetches", C.c_uint64), ("mip_fetches", C.c_uint64), ("bounce_rays", C.c_uint64),
                ("bounce_sun_hits", C.c_uint64),
                ("kernel_ms", C.c_double), ("primary_ms", C.c_double), ("paths_ms", C.c_double),
                ("launches", C.c_uint32), ("reserved", C.c_uint32),
                # ABI 7: render_kernel's own share of the counters (the rest is path_kernel's)
                ("camera_height_samples", C.c_uint64), ("camera_dem_fetches", C.c_uint64), ("camera_mip_fetches", C.c_uint64),
                ("camera_colour_fetches", C.c_uint64), ("camera_background_fetches", C.c_uint64)]


class MrtxIllumGrid(C.Structure):
    """One band of a lat/lon Sun-illumination map (mrtx_illum_grid)."""
    _fields_ = [("lat_north", C.c_double), ("lat_south", C.c_double), ("lon_west", C.c_double), ("lon_east", C.c_double),
                ("h", C.c_int32), ("w", C.c_int32), ("row_begin", C.c_int32), ("row_end", C.c_int32),
                ("n_sun", C.c_int32), ("reserved", C.c_int32)]


class MrtxSightGrid(C.Structure):
    """One band of a viewshed map (mrtx_sight_grid)."""
    _fields_ = [("obs_lat", C.c_double), ("obs_lon", C.c_double), ("obs_h_m", C.c_double), ("target_h_m", C.c_double),
                ("mast_max_m", C.c_double), ("radius_m", C.c_double), ("lat_north", C.c_double), ("lat_south", C.c_double),
                ("lon_west", C.c_double), ("lon_east", C.c_double), ("h", C.c_int32), ("w", C.c_int32),
                ("row_begin", C.c_int32), ("row_end", C.c_int32), ("n_bis", C.c_int32), ("reserved", C.c_int32)]


class MrtxTraverse(C.Structure):
    """A window of the DEM's texel lattice and the effort model of a least-cost traverse (mrtx_traverse, DESIGN.md section
    3.13)."""
    _fields_ = [("row0", C.c_int32), ("col0", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32),
                ("wrap", C.c_int32), ("radius_m", C.c_double), ("max_grade", C.c_double), ("climb_cost", C.c_double),
                ("descent_cost", C.c_double), ("reserved", C.c_int32)]


class MrtxTraverseTimed(C.Structure):
    """The tick scales of a timed traverse (mrtx_traverse_timed)."""
    _fields_ = [("ticks_per_cost", C.c_double), ("ticks_per_epoch", C.c_int32), ("n_epochs", C.c_int32), ("reserved", C.c_int32)]


class MrtxRelief(C.Structure):
    """A window of the DEM's texel lattice and the footprint of a relief map (mrtx_relief)."""
    _fields_ = [("row0", C.c_int32), ("col0", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32),
                ("ri", C.c_int32), ("rj", C.c_int32), ("reserved", C.c_int32), ("radius_m", C.c_double)]


class MrtxReliefShare(C.Structure):
    """The box and the thresholds of a landing ellipse's safe share (mrtx_relief_share)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("Ri", C.c_int32), ("Rj", C.c_int32), ("wrap", C.c_int32),
                ("reserved", C.c_int32), ("grade_max", C.c_double), ("rms_max", C.c_double)]


class MrtxRegions(C.Structure):
    """The lattice, the connectivity and the interval of a region labelling (mrtx_regions_label)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wrap", C.c_int32), ("connectivity", C.c_int32),
                ("n_ch", C.c_int32), ("ch", C.c_int32), ("lo", C.c_double), ("hi", C.c_double), ("reserved", C.c_int32)]


class MrtxRegion(C.Structure):
    """One record of a region catalogue (mrtx_regions_stats): 56 bytes, all integers."""
    _fields_ = [("weight", C.c_uint64), ("sum_i", C.c_int64), ("sum_dj", C.c_int64), ("count", C.c_uint32),
                ("root_i", C.c_int32), ("root_j", C.c_int32), ("i_min", C.c_int32), ("i_max", C.c_int32),
                ("dj_min", C.c_int32), ("dj_max", C.c_int32), ("reserved", C.c_uint32)]


class MrtxZonalSpec(C.Structure):
    """The lattice, the fixed point and the histogram of zonal statistics (mrtx_regions_zonal)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wrap", C.c_int32), ("n_ch", C.c_int32), ("scale", C.c_double),
                ("hist_ch", C.c_int32), ("n_bins", C.c_int32), ("hist_lo", C.c_double), ("hist_inv_w", C.c_double),
                ("reserved", C.c_int32)]


class MrtxZonal(C.Structure):
    """One channel of one region (mrtx_regions_zonal): 56 bytes, all exact."""
    _fields_ = [("wcount", C.c_uint64), ("wsum", C.c_int64), ("sum", C.c_int64), ("count", C.c_uint32), ("n_nan", C.c_uint32),
                ("n_clipped", C.c_uint32), ("min", C.c_float), ("max", C.c_float), ("min_at", C.c_int32), ("max_at", C.c_int32),
                ("reserved", C.c_uint32)]


class MrtxRegionShape(C.Structure):
    """One region's outline (mrtx_regions_shape): 32 bytes, all integers."""
    _fields_ = [("perimeter", C.c_uint64), ("sides_ns", C.c_uint32), ("sides_ew", C.c_uint32), ("q1", C.c_uint32),
                ("q3", C.c_uint32), ("qd", C.c_uint32), ("euler", C.c_int32)]


PROX_TO_SET = 0
PROX_TO_OUTSIDE = 1


class MrtxProximity(C.Structure):
    """The lattice and the feature set of a proximity map (mrtx_proximity)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32)]


class MrtxRegionReach(C.Structure):
    """The extremes of a dist2 table over one region (mrtx_regions_reach): 32 bytes."""
    _fields_ = [("d2_max", C.c_uint64), ("d2_min", C.c_uint64), ("max_at", C.c_int32), ("min_at", C.c_int32),
                ("min_nearest", C.c_int32), ("count", C.c_uint32)]


OUTLINE_ALL = 0
OUTLINE_CORNERS = 1


class MrtxOutline(C.Structure):
    """The lattice and the options of a region outline (mrtx_regions_outline)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wrap", C.c_int32), ("connectivity", C.c_int32), ("mode", C.c_int32),
                ("reserved", C.c_int32)]


class MrtxRing(C.Structure):
    """One boundary ring of a label table (mrtx_regions_outline): 48 bytes, all integers."""
    _fields_ = [("area", C.c_int64), ("warea", C.c_int64), ("first", C.c_uint64), ("n_sides", C.c_uint32),
                ("n_vertices", C.c_uint32), ("label", C.c_int32), ("head", C.c_int32), ("wind", C.c_int32),
                ("reserved", C.c_uint32)]


class MrtxContours(C.Structure):
    """The lattice and the number of levels of a contour call (mrtx_contours)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wrap", C.c_int32), ("n_levels", C.c_int32), ("reserved", C.c_int32)]


class MrtxContourLine(C.Structure):
    """One contour line (mrtx_contours): 32 bytes, all integers."""
    _fields_ = [("first", C.c_uint64), ("n_vertices", C.c_uint32), ("level_index", C.c_int32), ("level", C.c_int32),
                ("head", C.c_int32), ("tail", C.c_int32), ("closed", C.c_uint32)]


# MrtxContourLine, field for field (32 bytes)
CONTOUR_LINE_DTYPE = np.dtype([("first", "<u8"), ("n_vertices", "<u4"), ("level_index", "<i4"), ("level", "<i4"), ("head", "<i4"),
                               ("tail", "<i4"), ("closed", "<u4")])
assert CONTOUR_LINE_DTYPE.itemsize == 32 == C.sizeof(MrtxContourLine)
CONTOUR_MAX_LEVELS = 65536


RASTER_NONZERO, RASTER_EVENODD = 0, 1
RASTER_FIRST, RASTER_LAST = 0, 1


class MrtxRaster(C.Structure):
    """The lattice and the options of a polygon rasterisation (mrtx_rasterise)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wrap", C.c_int32), ("subcell_bits", C.c_int32), ("rule", C.c_int32),
                ("order", C.c_int32), ("reserved", C.c_int32)]


class MrtxRasterRing(C.Structure):
    """One ring of a polygon (mrtx_rasterise): 24 bytes."""
    _fields_ = [("first", C.c_uint64), ("n_vertices", C.c_uint32), ("polygon", C.c_int32), ("wind", C.c_int32),
                ("reserved", C.c_uint32)]


class MrtxPolygonCover(C.Structure):
    """What one polygon covers and owns (mrtx_rasterise): 40 bytes, all integers."""
    _fields_ = [("weight", C.c_uint64), ("owned_weight", C.c_uint64), ("count", C.c_uint32), ("owned", C.c_uint32),
                ("i_min", C.c_int32), ("i_max", C.c_int32), ("first_at", C.c_int32), ("reserved", C.c_uint32)]


FILL_NONE = 2 ** 31 - 1         # MRTX_FILL_NONE: the fill of a lattice without any outlet
FILL_ZMAX = 2 ** 30             # |z| <= 2^30


class MrtxFill(C.Structure):
    """The lattice and the outlets of a depression fill (mrtx_fill)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wrap", C.c_int32), ("connectivity", C.c_int32),
                ("edge_outlets", C.c_int32), ("reserved", C.c_int32)]


class MrtxBasin(C.Structure):
    """One region of a label table over a fill (mrtx_fill_basins): 48 bytes, all integers."""
    _fields_ = [("weight", C.c_uint64), ("volume", C.c_uint64), ("count", C.c_uint32), ("level_min", C.c_int32),
                ("level_max", C.c_int32), ("depth_max", C.c_int32), ("deepest_at", C.c_int32), ("pour_at", C.c_int32),
                ("pour_level", C.c_int32), ("reserved", C.c_uint32)]


class MrtxBowls(C.Structure):
    """The lattice, the outlets and the direction of a depression hierarchy (mrtx_bowls)."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wrap", C.c_int32), ("connectivity", C.c_int32),
                ("edge_outlets", C.c_int32), ("invert", C.c_int32), ("reserved", C.c_int32 * 2)]


class MrtxBowl(C.Structure):
    """One bowl of the hierarchy (mrtx_bowls): 64 bytes, all integers."""
    _fields_ = [("weight", C.c_uint64), ("volume", C.c_uint64), ("count", C.c_uint32), ("own_count", C.c_uint32),
                ("floor_at", C.c_int32), ("floor_level", C.c_int32), ("born_at", C.c_int32), ("born_level", C.c_int32),
                ("spill_at", C.c_int32), ("spill_level", C.c_int32), ("parent", C.c_int32), ("n_children", C.c_uint32),
                ("n_leaves", C.c_uint32), ("reserved", C.c_uint32)]


PASSES_FULL, PASSES_SUMMARY, PASSES_LIST = 0, 1, 2         # MRTX_PASSES_*: MoonRT.PASS_MODES names them


class MrtxPasses(C.Structure):
    """The satellites, the mode and the elevation mask of an orbiter-pass call (mrtx_horizon_passes)."""
    _fields_ = [("n_sat", C.c_int32), ("m", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32), ("radius_m", C.c_double),
                ("min_elev_deg", C.c_double)]


class MrtxPass(C.Structure):
    """One pass of one satellite over one point (mrtx_horizon_passes): 40 bytes."""
    _fields_ = [("point", C.c_int32), ("sat", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("max_at", C.c_int32),
                ("flags", C.c_uint32), ("rise_frac", C.c_float), ("set_frac", C.c_float), ("max_elev_deg", C.c_float),
                ("min_range_m", C.c_float)]


# MrtxPass, field for field (40 bytes)
PASS_DTYPE = np.dtype([("point", "<i4"), ("sat", "<i4"), ("first", "<i4"), ("count", "<i4"), ("max_at", "<i4"), ("flags", "<u4"),
                       ("rise_frac", "<f4"), ("set_frac", "<f4"), ("max_elev_deg", "<f4"), ("min_range_m", "<f4")])
assert PASS_DTYPE.itemsize == 40 == C.sizeof(MrtxPass)
PASS_COLUMNS = ("share_any", "longest_outage", "longest_contact", "first_contact", "contacts", "max_elev_deg", "mean_in_view",
                "share_two")
PASS_OPEN_START, PASS_OPEN_END = 1, 2                       # MrtxPass.flags


PAIRS_ANY, PAIRS_BOTH = 0, 1                                # MRTX_PAIRS_*: the op
PAIRS_ROWS, PAIRS_BEST, PAIRS_TABLE = 0, 1, 2               # the mode
PAIRS_BY_COUNT, PAIRS_BY_GAP = 0, 1                         # the rank
PAIRS_CHUNK_WORDS = 32                                      # csrc/mrtx_pairs.h's MRTX_PAIRS_CHUNK: the words staged in LDS at a time


class MrtxMaskPairs(C.Structure):
    """The tables, the operation, the mode and the distance bounds of a joint-availability call (mrtx_mask_pairs, DESIGN.md
    section 3.28): 48 bytes."""
    _fields_ = [("n_a", C.c_int32), ("n_b", C.c_int32), ("m", C.c_int32), ("op", C.c_int32), ("mode", C.c_int32),
                ("rank", C.c_int32), ("reserved", C.c_int32 * 2), ("d2_min", C.c_uint64), ("d2_max", C.c_uint64)]


# the BEST and ROWS record (16 bytes) and the TABLE record (8 bytes) of mrtx_mask_pairs
PAIR_DTYPE = np.dtype([("partner", "<i4"), ("count", "<u4"), ("gap", "<u4"), ("gap_first", "<i4")])
PAIR_TABLE_DTYPE = np.dtype([("count", "<u4"), ("gap", "<u4")])
assert PAIR_DTYPE.itemsize == 16 and PAIR_TABLE_DTYPE.itemsize == 8 and C.sizeof(MrtxMaskPairs) == 48


class MrtxIllumEpoch(C.Structure):
    """One date of a Sun-illumination series (mrtx_illum_series): what mrtx_set_light and
    mrtx_set_moon_frame would set for it."""
    _fields_ = [("light_pos", C.c_double * 3), ("light_radius", C.c_double), ("light_radiance", C.c_double),
                ("center", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3)]


THERMAL_MAX_NODES = 32


class MrtxThermalModel(C.Structure):
    """The layer tables and constants of the regolith column (mrtx_thermal)."""
    _fields_ = [("n_nodes", C.c_int32), ("n_sub", C.c_int32), ("n_spin", C.c_int32), ("block", C.c_int32),
                ("n_reset", C.c_int32), ("ref_node", C.c_int32), ("spacing_s", C.c_double),
                ("dz", C.c_double * THERMAL_MAX_NODES), ("rho", C.c_double * THERMAL_MAX_NODES),
                ("kc", C.c_double * THERMAL_MAX_NODES), ("chi", C.c_double), ("c", C.c_double * 5),
                ("emissivity", C.c_double), ("sigma", C.c_double), ("q_geo", C.c_double), ("albedo", C.c_double * 3)]


class MrtxVolatile(C.Structure):
    """The free sublimation rate of a volatile, ln E(T) = b0 - b1 / T + b2 ln T + b3 T in kg m^-2 s^-1 (mrtx_thermal_column's
    VOLATILE; volatiles.law builds it)."""
    _fields_ = [("b", C.c_double * 4)]


class MrtxPowerModel(C.Structure):
    """The panel and the battery of a site power budget (mrtx_power_budget)."""
    _fields_ = [("panel", C.c_int32), ("normal_enu", C.c_double * 3), ("cpw_log2", C.c_int32), ("capacity", C.c_int64),
                ("initial", C.c_int64)]


PANEL_TRACK, PANEL_FIXED, PANEL_AZIMUTH = 0, 1, 2           # MRTX_PANEL_*: MoonRT.PANELS names them
F_COUNT_STATS = 1
F_FORCE_WIDE = 2
F_NO_SKIP = 4
F_NO_CULL = 8
F_NO_SORT = 16
F_INWAVE_PATHS = 32
BUF_ACCUM, BUF_HITS, BUF_DEM, BUF_COLOR = 0, 1, 2, 3
BUF_MIP, BUF_MIP2, BUF_HMIP = 4, 5, 6           # the march's skip structures

_D3 = C.POINTER(C.c_double)
_VP = C.c_void_p

# name -> (restype, argtypes): every symbol include/moonrt.h declares
SIGNATURES = {
    "mrtx_abi_version": (C.c_int, []),
    "mrtx_get_config": (C.c_int, [_VP, C.POINTER(MrtxConfig)]),
    "mrtx_set_gather_hits": (C.c_int, [_VP, C.c_int32]),
    "mrtx_create": (C.c_int, [C.POINTER(MrtxConfig), C.POINTER(_VP)]),
    "mrtx_destroy": (None, [_VP]),
    "mrtx_last_error": (C.c_char_p, [_VP]),
    "mrtx_upload_dem": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32]),
    "mrtx_bind_dem_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32]),
    "mrtx_upload_color": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32]),
    "mrtx_bind_color_device": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32]),
    "mrtx_upload_background": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32]),
    "mrtx_upload_overlay": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32]),
    "mrtx_set_params": (C.c_int, [_VP, C.POINTER(MrtxParams)]),
    "mrtx_default_params": (None, [C.POINTER(MrtxParams)]),
    "mrtx_set_camera": (C.c_int, [_VP, _D3, _D3, _D3, C.c_double]),
    "mrtx_set_moon_frame": (C.c_int, [_VP, _D3, C.c_double, _D3, _D3]),
    "mrtx_set_light": (C.c_int, [_VP, _D3, C.c_double, C.c_double]),
    "mrtx_set_sun_disk": (C.c_int, [_VP, _D3, C.c_double, C.c_double]),
    "mrtx_set_capsules": (C.c_int, [_VP, _VP, C.c_int32]),
    "mrtx_reset_accum": (C.c_int, [_VP]),
    "mrtx_render": (C.c_int, [_VP, C.c_int32, C.POINTER(MrtxStats)]),
    "mrtx_render_part": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(MrtxStats)]),
    "mrtx_read_linear": (C.c_int, [_VP, _VP]),
    "mrtx_read_rgba8": (C.c_int, [_VP, _VP]),
    "mrtx_read_rgb16": (C.c_int, [_VP, _VP]),
    "mrtx_read_hits": (C.c_int, [_VP, _VP]),
    "mrtx_read_hit": (C.c_int, [_VP, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    "mrtx_samples_done": (C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    "mrtx_shard_bytes": (C.c_int, [_VP, C.c_int32, C.POINTER(C.c_uint64)]),
    "mrtx_shard_bytes_active": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "mrtx_shard_parts": (C.c_int, [_VP, C.c_int32, C.POINTER(C.c_int32)]),
    "mrtx_pack_part": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _VP]),
    "mrtx_pack_shard": (C.c_int, [_VP, _VP, _VP]),
    "mrtx_unpack_shard": (C.c_int, [_VP, C.c_int32, _VP, _VP]),
    "mrtx_unpack_all": (C.c_int, [_VP, C.POINTER(_VP), C.c_int32]),
    "mrtx_device_ptr": (C.c_int, [_VP, C.c_int32, C.POINTER(_VP), C.POINTER(C.c_uint64)]),
    "mrtx_mip_info": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "mrtx_dem_from_ldem": (C.c_int, [C.c_int32, _VP, C.c_int32, C.c_int32, C.c_int32, _VP,
                                     C.POINTER(C.c_float), C.c_char_p, C.c_int32]),
    "mrtx_synth_ldem": (C.c_int, [C.c_int32, _VP, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p, C.c_int32]),
    "mrtx_synth_color": (C.c_int, [C.c_int32, _VP, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p, C.c_int32]),
    "mrtx_dev_alloc": (C.c_int, [C.c_int32, C.c_uint64, C.POINTER(_VP)]),
    "mrtx_dev_free": (C.c_int, [C.c_int32, _VP]),
    "mrtx_dev_download": (C.c_int, [C.c_int32, _VP, _VP, C.c_uint64]),
    "mrtx_dev_upload": (C.c_int, [C.c_int32, _VP, _VP, C.c_uint64]),
    "mrtx_probe_stream": (C.c_int, [C.c_int32, C.c_uint64, C.c_int32]),
    "mrtx_probe_cr": (C.c_int, [C.c_int32, C.c_int32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "mrtx_probe_latlon": (C.c_int, [C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_int32]),
    "mrtx_illum_grid": (C.c_int, [_VP, C.POINTER(MrtxIllumGrid), _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_illum_points": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.POINTER(MrtxStats)]),
    "mrtx_illum_sun_samples": (C.c_int, [C.c_int32, _VP]),
    "mrtx_illum_series": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, C.c_int32, _VP, _VP,
                                    C.POINTER(MrtxStats)]),
    "mrtx_horizon_points": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_horizon_sun": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP,
                                   C.POINTER(MrtxStats)]),
    "mrtx_horizon_raised": (C.c_int, [_VP, _VP, _VP, C.c_double, C.c_int32, C.c_int32, C.c_int32, _VP, _VP,
                                      C.POINTER(MrtxStats)]),
    "mrtx_horizon_windows": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, C.c_double, C.c_double,
                                       _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_power_budget": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_int32, C.POINTER(MrtxPowerModel),
                                    C.c_int32, _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_sight_grid": (C.c_int, [_VP, C.POINTER(MrtxSightGrid), _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_sight_points": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, _VP,
                                    _VP, C.POINTER(MrtxStats)]),
    "mrtx_traverse_lengths": (C.c_int, [C.POINTER(MrtxTraverse), C.c_int32, C.c_int32, _VP]),
    "mrtx_traverse": (C.c_int, [_VP, C.POINTER(MrtxTraverse), _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_traverse_heights": (C.c_int, [_VP, C.POINTER(MrtxTraverse), _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_horizon_mask": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, C.c_double, C.c_double,
                                    _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_traverse_timed": (C.c_int, [_VP, C.POINTER(MrtxTraverse), C.POINTER(MrtxTraverseTimed), _VP, _VP, C.c_int32, _VP, _VP,
                                      _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_relief_scales": (C.c_int, [C.POINTER(MrtxRelief), C.c_int32, C.c_int32, _VP]),
    "mrtx_relief": (C.c_int, [_VP, C.POINTER(MrtxRelief), _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_relief_share": (C.c_int, [_VP, C.POINTER(MrtxReliefShare), _VP, _VP, _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_regions_label": (C.c_int, [_VP, C.POINTER(MrtxRegions), _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_uint32),
                                     C.POINTER(MrtxStats)]),
    "mrtx_regions_stats": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_uint32, _VP, _VP, _VP,
                                     C.POINTER(MrtxStats)]),
    "mrtx_regions_zonal": (C.c_int, [_VP, C.POINTER(MrtxZonalSpec), _VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                     C.POINTER(MrtxStats)]),
    "mrtx_regions_shape": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP,
                                     C.POINTER(MrtxStats)]),
    "mrtx_proximity": (C.c_int, [_VP, C.POINTER(MrtxProximity), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_uint64),
                                 C.POINTER(MrtxStats)]),
    "mrtx_regions_reach": (C.c_int, [_VP, C.c_int32, C.c_int32, _VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP,
                                     C.POINTER(MrtxStats)]),
    "mrtx_regions_outline": (C.c_int, [_VP, C.POINTER(MrtxOutline), _VP, _VP, C.c_uint32, _VP, _VP, _VP, C.c_uint64, _VP, _VP,
                                       C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_rasterise": (C.c_int, [_VP, C.POINTER(MrtxRaster), _VP, _VP, C.c_uint64, _VP, _VP, C.c_uint64, C.c_uint32, _VP, _VP, _VP, _VP,
                                 _VP, C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_contours": (C.c_int, [_VP, C.POINTER(MrtxContours), _VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, C.c_uint64,
                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_fill": (C.c_int, [_VP, C.POINTER(MrtxFill), _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_fill_basins": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, _VP,
                                   _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_bowls": (C.c_int, [_VP, C.POINTER(MrtxBowls), _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP,
                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_thermal": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP,
                               C.POINTER(MrtxStats)]),
    "mrtx_view_dir_samples": (C.c_int, [C.c_int32, _VP]),
    "mrtx_view_hits": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_scatter_flux": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                    C.c_double, _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_thermal_scatter": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP,
                                       C.c_int64, _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_thermal_column": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP,
                                      C.c_int64, C.POINTER(MrtxVolatile), _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_occultation": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP, C.POINTER(MrtxStats)]),
    "mrtx_horizon_passes": (C.c_int, [_VP, C.POINTER(MrtxPasses), _VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP,
                                      C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_mask_pairs": (C.c_int, [_VP, C.POINTER(MrtxMaskPairs), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                  C.POINTER(C.c_uint64), C.POINTER(MrtxStats)]),
    "mrtx_thermal_occulted": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP,
                                        C.c_int64, C.POINTER(MrtxVolatile), _VP, _VP, _VP, _VP, C.POINTER(MrtxStats)]),
}

_lib = None
_preloaded_runtime = None


class NativeLibraryError(RuntimeError):
    pass


def hip_runtimes_loaded():
    """Paths of every libamdhip64 copy mapped into this process (more than one means two HIP/HSA runtimes are alive:
    the second one to initialise finds no GPUs)."""
    seen = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(" ", 1)[-1].strip()
                if "libamdhip64" in os.path.basename(path):
                    real = os.path.realpath(path)
                    if real not in seen:
                        seen.append(real)
    except OSError:
        pass
    return seen


def _elf_dynamic_strings(path):
    """(DT_SONAME or None, [DT_NEEDED ...]) of a little-endian ELF64 shared object, read from the file (no loader involved)."""
    import struct
    with open(path, "rb") as f:
        data = f.read()
    if data[:6] != b"\x7fELF\x02\x01":
        raise ValueError(f"{path}: not a little-endian ELF64 file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    soname, needed = None, []
    for sec in secs:
        if sec[1] != 6:                       # SHT_DYNAMIC
            continue
        stroff = secs[sec[6]][4]              # sh_link -> the string table's file offset
        for i in range(sec[5] // 16):
            tag, val = struct.unpack_from("<qQ", data, sec[4] + 16 * i)
            if tag == 0:
                break
            if tag in (1, 14):                # DT_NEEDED, DT_SONAME
                end = data.index(b"\0", stroff + val)
                name = data[stroff + val:end].decode()
                if tag == 14:
                    soname = name
                else:
                    needed.append(name)
    return soname, needed


def _preload_torch_hip_runtime():
    """ONE HIP runtime per process, whatever the import order.

    libmoonrt.so needs `libamdhip64.so.7` (a SONAME); the torch wheel bundles its own copy of the runtime and asks for it by
    FILE name (`libamdhip64.so`, RPATH $ORIGIN).  The dynamic loader reuses an already-loaded library when the requested name
    equals its SONAME or its file -- so "torch first" gives one runtime (torch's copy satisfies libmoonrt's SONAME request),
    but "libmoonrt first" used to give two (/opt/rocm's for libmoonrt, then torch's for torch), and torch / RCCL then
    reported "no GPUs found".  When a torch installation is present its copy is therefore loaded here, BEFORE
    libmoonrt.so and without importing torch: either order now ends on that single copy.  Without torch the system
    runtime is used.  MOONRT_HIP_RUNTIME=system skips this (then import torch before this package)."""
    global _preloaded_runtime
    if os.environ.get("MOONRT_HIP_RUNTIME") == "system" or hip_runtimes_loaded():
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.isfile(path):
        # Only a copy that IS what libmoonrt asks for may stand in for it: the wheel's SONAME must be one of libmoonrt's
        # DT_NEEDED names.  Otherwise the loader would pull the system runtime in beside it (two runtimes), or libmoonrt would
        # silently run on a runtime of another major version: leave the system runtime alone then (round-2 advisor finding).
        try:
            soname, _ = _elf_dynamic_strings(path)
            _, needed = _elf_dynamic_strings(LIB_PATH)
        except (OSError, ValueError, IndexError, __import__("struct").error):
            return
        if soname is None or soname not in needed:
            return
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
            _preloaded_runtime = path
        except OSError:
            pass            # fall back to the system runtime; load() checks for duplicates below


def load():
    """Return the loaded library; raise NativeLibraryError if it is missing or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C moonrtx_amd/csrc` (needs hipcc). There is no CPU fallback.")
    _preload_torch_hip_runtime()
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.mrtx_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"ABI version mismatch: library {lib.mrtx_abi_version()}, host {ABI_VERSION}")
    rts = hip_runtimes_loaded()
    if len(rts) > 1:
        raise NativeLibraryError("two HIP runtimes are loaded in this process (" + ", ".join(rts) + "): the second one to "
                                 "initialise will see no GPUs. Import moonrtx_amd (or torch) before anything else loads "
                                 "another libamdhip64, or set LD_LIBRARY_PATH so that both resolve to one copy.")
    _lib = lib
    return lib


def assert_single_hip_runtime():
    """Called before a torch.distributed / RCCL group is created: fail loudly instead of 'no GPUs found'."""
    rts = hip_runtimes_loaded()
    if len(rts) > 1:
        raise NativeLibraryError("two HIP runtimes are loaded in this process: " + ", ".join(rts))
    return rts


def vec3(v):
    a = (C.c_double * 3)(float(v[0]), float(v[1]), float(v[2]))
    return a
