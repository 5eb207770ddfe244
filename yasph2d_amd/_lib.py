"""ctypes binding of libsphx.so (include/sphx.h).  Fails loudly if the library is missing: there is no fallback."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPHX_LIB: load another build of the same library (kernel A/B experiments, tools/ab_build.sh)
LIB_PATH = os.environ.get("SPHX_LIB") or os.path.join(_HERE, "libsphx.so")
CSRC = os.path.join(_HERE, "csrc")

# status codes (sphx.h)
OK, ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_READY, ERR_NONFINITE, ERR_NEIGHBOR_PANIC, ERR_CAPACITY, ERR_OUT_OF_DOMAIN = range(9)
FLAG_NEIGHBOR_CAP, FLAG_DENSITY_ITER_CAP, FLAG_DIVERGENCE_ITER_CAP, FLAG_WARMUP, FLAG_STRAY_PARTICLES, FLAG_DENSE_CELL = 1, 2, 4, 8, 16, 32
KERNEL_WENDLAND_C2, KERNEL_POLY6, KERNEL_SPIKY = 0, 1, 2
VISCOSITY_XSPH, VISCOSITY_PHYSICAL = 0, 1  # sphx_params.viscosity_model


class SphxParams(C.Structure):
    _fields_ = [
        ("smoothing_length", C.c_float),
        ("particle_mass", C.c_float),
        ("fluid_density", C.c_float),
        ("particle_radius", C.c_float),
        ("gravity", C.c_float * 2),
        ("grid_min", C.c_float * 2),
        ("xsph_epsilon", C.c_float),
        ("max_avg_density_error", C.c_float),
        ("max_density_iterations", C.c_uint32),
        ("max_divergence_error", C.c_float),
        ("max_divergence_iterations", C.c_uint32),
        ("fixed_density_iterations", C.c_uint32),
        ("fixed_divergence_iterations", C.c_uint32),
        ("device", C.c_int32),
        ("list_span_limit", C.c_uint32),
        ("viscosity_model", C.c_uint32),
        ("fluid_viscosity", C.c_float),
        ("reserved", C.c_uint32 * 1),
    ]


class SphxTimerLaw(C.Structure):
    _fields_ = [
        ("adaptive", C.c_uint32),
        ("cfl_factor", C.c_float),
        ("particle_diameter", C.c_float),
        ("reserved", C.c_uint32),
        ("timestep_min_ns", C.c_uint64),
        ("timestep_max_ns", C.c_uint64),
        ("simulation_step_ns", C.c_uint64),
    ]


class SphxStepStats(C.Structure):
    _fields_ = [
        ("density_iterations", C.c_uint32),
        ("divergence_iterations", C.c_uint32),
        ("warmstart_density", C.c_uint32),
        ("warmstart_divergence", C.c_uint32),
        ("avg_density_error", C.c_float),
        ("avg_divergence", C.c_float),
        ("dt_prev", C.c_float),
        ("dt", C.c_float),
        ("vmax", C.c_float),
        ("flags", C.c_uint32),
        ("remote_entries", C.c_uint32),
        ("neighbor_entries", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class SphxKernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double), ("algorithmic_bytes", C.c_double)]


def build(force=False):
    """hipcc --offload-arch=gfx950 build of libsphx.so via csrc/Makefile (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)


SAMPLE_DEVICE_POINTERS = 1  # sphx_sample_points / sphx_sample_grid flags


class SphxSampleOut(C.Structure):
    _fields_ = [("density", C.c_void_p), ("fraction", C.c_void_p), ("velocity", C.c_void_p), ("count", C.c_void_p)]


CONTOUR_DEVICE_POINTERS = 1  # sphx_surface_contour flags
CONTOUR_FIELDS = dict(fraction=0, density=1)  # SPHX_CONTOUR_FIELD_*


class SphxContourOut(C.Structure):
    _fields_ = [("segments", C.c_void_p), ("cell", C.c_void_p), ("values", C.c_void_p), ("count", C.c_void_p)]


SAMPLE_FIELD_BITS = dict(density=1, fraction=2, velocity=4, count=8)  # SPHX_SAMPLE_FIELD_* (sphx_tile_sample_*)


class SphxMultiSampleOut(C.Structure):  # sphx_multi_sample_out: host pointers
    _fields_ = [("density", C.c_void_p), ("fraction", C.c_void_p), ("velocity", C.c_void_p), ("count", C.c_void_p), ("tile", C.c_void_p)]


class SphxMultiContourOut(C.Structure):  # sphx_multi_contour_out: host pointers
    _fields_ = [("segments", C.c_void_p), ("cell", C.c_void_p), ("tile", C.c_void_p), ("count", C.c_void_p)]


class SphxTileRect(C.Structure):  # sphx_tile_rect: cells, half-open
    _fields_ = [("x0", C.c_uint32), ("x1", C.c_uint32), ("y0", C.c_uint32), ("y1", C.c_uint32)]


RENDER_DEVICE_POINTERS = 1  # sphx_render flags
RENDER_NONE, RENDER_BOUNDARY = 0xFFFFFFFF, 0xFFFFFFFE  # owner codes


class SphxRenderView(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("center", C.c_float * 2), ("pixel_per_world_unit", C.c_float),
                ("radius", C.c_float), ("min_pixel_radius", C.c_float), ("speed_scale", C.c_float), ("background", C.c_uint8 * 4),
                ("boundary", C.c_uint8 * 4), ("reserved", C.c_uint32 * 2)]


class SphxRenderOut(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("owner", C.c_void_p)]


class SphxRenderLayer(C.Structure):  # sphx_render_layer: one tile's (or rank's) picture at the full size of the view
    _fields_ = [("key", C.c_void_p), ("owner", C.c_void_p), ("rgba", C.c_void_p)]


REMOVE_OUTSIDE = 1  # sphx_remove flags
REMOVE_MAX_RECTS = 8


class SphxRect(C.Structure):
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float)]


QUERY_DEVICE_POINTERS, QUERY_BOUNDARY = 1, 2  # sphx_query_radius flags
QUERY_NONE = 0xFFFFFFFF       # nearest of a point that accepts nothing
QUERY_NONE_WORD = 0x7F800000  # ... and its nearest_dist_sq (+inf)
SELECT_OUTSIDE, SELECT_DEVICE_POINTERS = 1, 2  # sphx_select flags


class SphxQueryOut(C.Structure):  # 56 bytes
    _fields_ = [("offsets", C.c_void_p), ("index", C.c_void_p), ("id", C.c_void_p), ("dist_sq", C.c_void_p), ("nearest", C.c_void_p),
                ("nearest_dist_sq", C.c_void_p), ("count", C.c_void_p)]


class SphxSelectOut(C.Structure):  # 24 bytes
    _fields_ = [("index", C.c_void_p), ("id", C.c_void_p), ("count", C.c_void_p)]


class SphxMultiQueryOut(C.Structure):  # sphx_multi_query_out: host pointers, 72 bytes
    _fields_ = [("offsets", C.c_void_p), ("id", C.c_void_p), ("dist_sq", C.c_void_p), ("slot", C.c_void_p), ("nearest_id", C.c_void_p),
                ("nearest_slot", C.c_void_p), ("nearest_dist_sq", C.c_void_p), ("tile", C.c_void_p), ("count", C.c_void_p)]


class SphxMultiSelectOut(C.Structure):  # sphx_multi_select_out: host pointers, 32 bytes
    _fields_ = [("id", C.c_void_p), ("tile", C.c_void_p), ("slot", C.c_void_p), ("count", C.c_void_p)]


class SphxTileQueryPart(C.Structure):  # sphx_tile_query_part: host pointers, 88 bytes
    _fields_ = [("n_points", C.c_uint32), ("reserved", C.c_uint32), ("total", C.c_uint64), ("kept", C.c_uint64), ("point", C.c_void_p),
                ("offset", C.c_void_p), ("nearest_slot", C.c_void_p), ("nearest_id", C.c_void_p), ("nearest_dist_sq", C.c_void_p),
                ("slot", C.c_void_p), ("id", C.c_void_p), ("dist_sq", C.c_void_p)]


STATE_DEVICE_BUFFER = 1  # sphx_state_save / sphx_state_load flags
STATE_SECTIONS = ("positions", "velocities", "particle_id", "density", "alpha", "kappa", "stiffness", "accel", "boundary")  # SPHX_STATE_SEC_*
MULTI_STATE_SECTIONS = ("positions", "velocities", "particle_id", "density", "alpha", "kappa", "stiffness", "boundary")  # SPHX_MULTI_STATE_SEC_*
TILE_STATE_ZERO_KAPPA, TILE_STATE_ZERO_STIFFNESS = 1, 2  # sphx_tile_state_pack flags


TRACK_DEVICE_POINTERS = 1  # sphx_track_fetch / sphx_track_read / sphx_download_by_id flags
TRACK_MAX_IDS = 16384
TRACK_ABSENT = 0xFFFFFFFF      # slot of an id no particle carries
TRACK_ABSENT_WORD = 0x7FC00000  # ... and every float of its record


class SphxTrackOut(C.Structure):
    _fields_ = [("slot", C.c_void_p), ("pos", C.c_void_p), ("vel", C.c_void_p), ("density", C.c_void_p)]


class SphxMultiTrackOut(C.Structure):  # sphx_multi_track_out: host pointers
    _fields_ = [("tile", C.c_void_p), ("slot", C.c_void_p), ("pos", C.c_void_p), ("vel", C.c_void_p), ("density", C.c_void_p)]


class SphxTrackStatus(C.Structure):
    _fields_ = [("m", C.c_uint32), ("recording", C.c_uint32), ("max_frames", C.c_uint32), ("every", C.c_uint32), ("frames", C.c_uint32),
                ("dropped", C.c_uint32), ("reserved", C.c_uint32 * 2)]


FIELDS_DEVICE_POINTERS = 1  # sphx_particle_fields flags


class SphxFieldsOut(C.Structure):
    _fields_ = [("vel_grad", C.c_void_p), ("divergence", C.c_void_p), ("vorticity", C.c_void_p), ("color_grad", C.c_void_p)]


FIELD_BITS = dict(vel_grad=1, divergence=2, vorticity=4, color_grad=8)  # SPHX_FIELD_* (sphx_tile_particle_fields_*)


class SphxMultiFieldsOut(C.Structure):  # sphx_multi_fields_out: host pointers
    _fields_ = [("vel_grad", C.c_void_p), ("divergence", C.c_void_p), ("vorticity", C.c_void_p), ("color_grad", C.c_void_p),
                ("ids", C.c_void_p), ("tile", C.c_void_p)]


STATS_DEVICE_POINTERS = 1  # sphx_fluid_stats flags
STATS_MAX_RECTS = 8


class SphxStatsRec(C.Structure):  # 128 bytes
    _fields_ = [("count", C.c_uint64), ("nonfinite", C.c_uint64), ("density_count", C.c_uint64), ("density_valid", C.c_uint32),
                ("reserved", C.c_uint32), ("sum_pos", C.c_double * 2), ("sum_vel", C.c_double * 2), ("sum_speed_sq", C.c_double),
                ("sum_angular", C.c_double), ("sum_density", C.c_double), ("sum_density_sq", C.c_double), ("max_speed_sq", C.c_double),
                ("min_pos", C.c_float * 2), ("max_pos", C.c_float * 2), ("min_density", C.c_float), ("max_density", C.c_float)]


class SphxStatsFrame(C.Structure):  # 16 bytes
    _fields_ = [("step", C.c_uint64), ("dt", C.c_float), ("n", C.c_uint32)]


class SphxStatsStatus(C.Structure):
    _fields_ = [("n_rects", C.c_uint32), ("recording", C.c_uint32), ("max_frames", C.c_uint32), ("every", C.c_uint32), ("frames", C.c_uint32),
                ("dropped", C.c_uint32), ("reserved", C.c_uint32 * 2)]


GAUGE_DEVICE_POINTERS = 1  # sphx_gauge_levels flags
GAUGE_FIELDS = dict(fraction=0, density=1)  # SPHX_GAUGE_FIELD_*
GAUGE_NONE = 0xFFFFFFFF
GAUGE_MAX = 1024


class SphxGauge(C.Structure):  # 32 bytes: a ray of n samples
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("dx", C.c_float), ("dy", C.c_float), ("n", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class SphxGaugeRec(C.Structure):  # 32 bytes
    _fields_ = [("first", C.c_uint32), ("last", C.c_uint32), ("inside", C.c_uint32), ("t", C.c_float), ("x", C.c_float), ("y", C.c_float),
                ("f_last", C.c_float), ("f_next", C.c_float)]


class SphxProbeRec(C.Structure):  # 32 bytes
    _fields_ = [("density", C.c_float), ("fraction", C.c_float), ("velocity", C.c_float * 2), ("count", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class SphxProbeStatus(C.Structure):  # 32 bytes
    _fields_ = [("m_points", C.c_uint32), ("n_gauges", C.c_uint32), ("recording", C.c_uint32), ("max_frames", C.c_uint32), ("every", C.c_uint32),
                ("frames", C.c_uint32), ("dropped", C.c_uint32), ("reserved", C.c_uint32)]


class SphxTimerState(C.Structure):
    _fields_ = [("fixed", C.c_uint32), ("cfl_factor", C.c_float), ("timestep_max_ns", C.c_uint64), ("timestep_min_ns", C.c_uint64),
                ("simulation_step_ns", C.c_uint64), ("timestep_target_frame_ns", C.c_uint64), ("total_simulated_ns", C.c_uint64),
                ("num_simulation_steps", C.c_uint32), ("reserved", C.c_uint32)]


class SphxMultiOptions(C.Structure):
    _fields_ = [("halo_cells", C.c_uint32), ("fixed_halo", C.c_uint32), ("rebalance_every", C.c_uint32), ("layout", C.c_uint32),
                ("cap_records", C.c_uint32), ("overlap_exchange", C.c_uint32), ("reserved", C.c_uint32 * 2)]


COMM_EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p)
COMM_ALLREDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double))
COMM_ABORT = C.CFUNCTYPE(None, C.c_void_p)


class SphxCommOps(C.Structure):
    _fields_ = [("user", C.c_void_p), ("rank", C.c_int), ("world", C.c_int), ("exchange", COMM_EXCHANGE), ("allreduce", COMM_ALLREDUCE),
                ("abort", COMM_ABORT)]


class SphxMultiInfo(C.Structure):
    _fields_ = [("world", C.c_uint32), ("local_tiles", C.c_uint32), ("halo_now", C.c_uint32), ("halo_max", C.c_uint32), ("peers", C.c_uint32),
                ("n_local", C.c_uint32), ("cap_records", C.c_uint32), ("grid_layout", C.c_uint32), ("axis", C.c_int32), ("band_packs", C.c_uint32),
                ("exchanges", C.c_uint64), ("rebalances", C.c_uint64), ("build_particles", C.c_uint64), ("neighbor_entries", C.c_uint64),
                ("remote_entries", C.c_uint64), ("owned_local", C.c_uint64), ("transport", C.c_char * 96),
                ("halo_bytes_packed", C.c_uint64), ("halo_bytes_sent", C.c_uint64), ("ownership_seconds", C.c_double)]


LAYOUT_AUTO, LAYOUT_STRIPS, LAYOUT_GRID = 0, 1, 2

# every symbol include/sphx.h declares: (restype, argtypes)
_vp, _u16p = C.c_void_p, C.c_void_p
_f, _u32, _u64, _i = C.c_float, C.c_uint32, C.c_uint64, C.c_int
class SphxTileStateOut(C.Structure):  # sphx_tile_state_out: seven device pointers
    _fields_ = [(k, C.c_void_p) for k in ("pos", "vel", "id", "density", "alpha", "kappa", "stiffness")]


SIGNATURES = {
    "sphx_abi_version": (_u32, []),
    "sphx_default_params": (_i, [_f, _f, _f, C.POINTER(SphxParams)]),
    "sphx_create": (_i, [C.POINTER(SphxParams), C.POINTER(_vp)]),
    "sphx_destroy": (None, [_vp]),
    "sphx_last_error": (C.c_char_p, [_vp]),
    "sphx_set_boundary": (_i, [_vp, _vp, _u32]),
    "sphx_upload": (_i, [_vp, _vp, _vp, _u32]),
    "sphx_append": (_i, [_vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "sphx_remove": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, C.POINTER(_u32)]),
    "sphx_query_radius": (_i, [_vp, _vp, _u32, _f, _u64, _u32, C.POINTER(SphxQueryOut)]),
    "sphx_select": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _u32, C.POINTER(SphxSelectOut)]),
    "sphx_state_size": (_i, [_vp, C.POINTER(_u64)]),
    "sphx_state_save": (_i, [_vp, _vp, _u64, _u32, C.POINTER(_u64)]),
    "sphx_state_load": (_i, [_vp, _vp, _u64, _u32]),
    "sphx_state_digest": (_i, [_vp, C.POINTER(_u64)]),
    "sphx_state_save_file": (_i, [_vp, C.c_char_p]),
    "sphx_state_load_file": (_i, [_vp, C.c_char_p]),
    "sphx_track_set": (_i, [_vp, _vp, _u32]),
    "sphx_track_fetch": (_i, [_vp, _u32, C.POINTER(SphxTrackOut)]),
    "sphx_track_record": (_i, [_vp, _u32, _u32]),
    "sphx_track_get_status": (_i, [_vp, C.POINTER(SphxTrackStatus)]),
    "sphx_track_read": (_i, [_vp, _u32, _u32, _u32, _vp]),
    "sphx_particle_fields": (_i, [_vp, _u32, C.POINTER(SphxFieldsOut)]),
    "sphx_multi_track_set": (_i, [_vp, _vp, _u32]),
    "sphx_multi_track_fetch": (_i, [_vp, _u32, C.POINTER(SphxMultiTrackOut)]),
    "sphx_multi_track_record": (_i, [_vp, _u32, _u32]),
    "sphx_multi_track_get_status": (_i, [_vp, C.POINTER(SphxTrackStatus)]),
    "sphx_multi_track_read": (_i, [_vp, _u32, _u32, _u32, _vp, _vp]),
    "sphx_multi_download_by_id": (_i, [_vp, _u32, _u32, _u32, C.POINTER(SphxMultiTrackOut), C.POINTER(_u32)]),
    "sphx_track_merge": (_i, [_u32, C.POINTER(SphxMultiTrackOut), _u32, C.POINTER(SphxMultiTrackOut), C.POINTER(_u32)]),
    "sphx_track_merge_frames": (_i, [_u64, C.POINTER(_vp), C.POINTER(_vp), _u32, _vp, _vp]),
    "sphx_tile_track_install": (_i, [_vp, _vp, _vp, _u32, _u32]),
    "sphx_tile_track_fetch_enqueue": (_i, [_vp]),
    "sphx_tile_track_fetch": (_i, [_vp, _vp, _vp, _vp]),
    "sphx_tile_track_window_enqueue": (_i, [_vp, _u32, _u32, _u32]),
    "sphx_tile_track_window_fetch": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "sphx_tile_track_record": (_i, [_vp, _u32, _u32]),
    "sphx_tile_track_frame": (_i, [_vp]),
    "sphx_tile_track_read": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "sphx_fluid_stats": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _vp]),
    "sphx_stats_record": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _u32]),
    "sphx_stats_get_status": (_i, [_vp, C.POINTER(SphxStatsStatus)]),
    "sphx_stats_read": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "sphx_gauge_levels": (_i, [_vp, _vp, _u32, _i, _i, _f, _u32, _vp, _vp]),
    "sphx_gauge_reduce": (_i, [_vp, _vp, _u32, _f, _vp]),
    "sphx_probe_record": (_i, [_vp, _vp, _u32, _vp, _u32, _i, _i, _f, _u32, _u32]),
    "sphx_probe_get_status": (_i, [_vp, C.POINTER(SphxProbeStatus)]),
    "sphx_probe_read": (_i, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "sphx_multi_gauge_levels": (_i, [_vp, _vp, _u32, _i, _i, _f, _u32, _vp, _vp, _vp]),
    "sphx_gauge_merge": (_i, [_vp, _u32, _f, _vp, _u32, _vp]),
    "sphx_multi_probe_record": (_i, [_vp, _vp, _u32, _vp, _u32, _i, _i, _f, _u32, _u32]),
    "sphx_multi_probe_get_status": (_i, [_vp, C.POINTER(SphxProbeStatus)]),
    "sphx_multi_probe_read": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "sphx_tile_gauge_levels": (_i, [_vp, _vp, _u32, _i, _i, _f]),
    "sphx_tile_gauge_fetch": (_i, [_vp, _vp, _vp, _vp]),
    "sphx_tile_probe_record": (_i, [_vp, _vp, _u32, _vp, _u32, _i, _i, _f, _u32, _u32]),
    "sphx_tile_probe_due": (_i, [_vp]),
    "sphx_tile_probe_frame": (_i, [_vp, _f, _u32]),
    "sphx_tile_probe_read": (_i, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "sphx_tile_fluid_stats": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _vp]),
    "sphx_tile_stats_record": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _u32]),
    "sphx_tile_stats_frame": (_i, [_vp, _f, _u32]),
    "sphx_tile_stats_read": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "sphx_multi_fluid_stats": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _vp, _vp]),
    "sphx_multi_stats_record": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _u32]),
    "sphx_multi_stats_get_status": (_i, [_vp, C.POINTER(SphxStatsStatus)]),
    "sphx_multi_stats_read": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "sphx_tile_state_pack": (_i, [_vp, _u32, C.POINTER(SphxTileStateOut), C.POINTER(_u64), C.POINTER(_u32)]),
    "sphx_tile_state_fetch": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u32)]),
    "sphx_tile_upload_state": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u32]),
    "sphx_get_tiling_invariant": (_i, [_vp]),
    "sphx_multi_state_size": (_i, [_vp, C.POINTER(_u64)]),
    "sphx_multi_state_save": (_i, [_vp, _vp, _u64, _u32, C.POINTER(_u64)]),
    "sphx_multi_state_load": (_i, [_vp, C.POINTER(_vp), C.POINTER(_u64), _u32, _u32]),
    "sphx_multi_state_digest": (_i, [_vp, C.POINTER(_u64)]),
    "sphx_multi_state_save_file": (_i, [_vp, C.c_char_p]),
    "sphx_multi_state_load_file": (_i, [_vp, C.c_char_p]),
    "sphx_multi_append": (_i, [_vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "sphx_multi_remove": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, C.POINTER(_u64)]),
    "sphx_tile_remove_mark": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32]),
    "sphx_tile_remove_fetch": (_i, [_vp, C.POINTER(_u32)]),
    "sphx_tile_append": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "sphx_tile_grow": (_i, [_vp, _u32]),
    "sphx_debug_correction_counts": (_i, [_vp, _vp]),
    "sphx_debug_quiet_counts": (_i, [_vp, _vp]),
    "sphx_debug_takeover_counts": (_i, [_vp, _vp]),
    "sphx_debug_rigid_counts": (_i, [_vp, _vp]),
    "sphx_debug_rigid_predict_counts": (_i, [_vp, _vp]),
    "sphx_debug_download_accel": (_i, [_vp, _vp]),
    "sphx_debug_download_wcsph_half_step": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "sphx_download_by_id": (_i, [_vp, _u32, _u32, _u32, C.POINTER(SphxTrackOut), C.POINTER(_u32)]),
    "sphx_download": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "sphx_download_boundary": (_i, [_vp, _vp, _vp]),
    "sphx_num_particles": (_u32, [_vp]),
    "sphx_num_boundary": (_u32, [_vp]),
    "sphx_sample_points": (_i, [_vp, _vp, _u32, _i, _u32, C.POINTER(SphxSampleOut)]),
    "sphx_sample_grid": (_i, [_vp, _f, _f, _f, _f, _u32, _u32, _i, _u32, C.POINTER(SphxSampleOut)]),
    "sphx_surface_contour": (_i, [_vp, _f, _f, _f, _f, _u32, _u32, _i, _i, _f, _u32, _u32, C.POINTER(SphxContourOut)]),
    "sphx_contour_chain": (_i, [_vp, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "sphx_multi_sample_points": (_i, [_vp, _vp, _u32, _i, _u32, C.POINTER(SphxMultiSampleOut)]),
    "sphx_multi_sample_grid": (_i, [_vp, _f, _f, _f, _f, _u32, _u32, _i, _u32, C.POINTER(SphxMultiSampleOut)]),
    "sphx_sample_merge": (_i, [_u32, C.POINTER(SphxMultiSampleOut), _u32, C.POINTER(SphxMultiSampleOut)]),
    "sphx_multi_query_radius": (_i, [_vp, _vp, _u32, _f, _u64, _u32, C.POINTER(SphxMultiQueryOut)]),
    "sphx_query_merge": (_i, [_u32, C.POINTER(SphxMultiQueryOut), C.POINTER(_u64), _u32, _u64, C.POINTER(SphxMultiQueryOut)]),
    "sphx_multi_select": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32, _u64, C.POINTER(SphxMultiSelectOut)]),
    "sphx_tile_query_radius": (_i, [_vp, _vp, _u32, _f, _u32, _u32]),
    "sphx_tile_query_fetch": (_i, [_vp, _u64, C.POINTER(SphxTileQueryPart)]),
    "sphx_tile_select": (_i, [_vp, C.POINTER(SphxRect), _u32, _u32]),
    "sphx_tile_select_fetch": (_i, [_vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "sphx_multi_tile_rects": (_i, [_vp, C.POINTER(SphxTileRect), C.POINTER(_u32)]),
    "sphx_multi_ghost_rings": (_i, [_vp, C.POINTER(C.c_double)]),
    "sphx_tile_sample_points": (_i, [_vp, _vp, _u32, _i, _u32]),
    "sphx_tile_sample_points_fetch": (_i, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "sphx_tile_sample_window": (_i, [_vp, _f, _f, _f, _f, _u32, _u32, _i, _u32, C.POINTER(_u32)]),
    "sphx_tile_sample_window_fetch": (_i, [_vp, C.POINTER(SphxSampleOut)]),
    "sphx_multi_surface_contour": (_i, [_vp, _f, _f, _f, _f, _u32, _u32, _i, _i, _f, _u32, _u32, C.POINTER(SphxMultiContourOut)]),
    "sphx_contour_merge": (_i, [C.POINTER(SphxMultiContourOut), C.POINTER(_u32), _u32, _u32, C.POINTER(SphxMultiContourOut)]),
    "sphx_tile_contour_sample": (_i, [_vp, _f, _f, _f, _f, _u32, _u32, _i, _i, C.POINTER(_u32)]),
    "sphx_tile_contour_border_fetch": (_i, [_vp, _vp, _u32]),
    "sphx_tile_contour_cut": (_i, [_vp, _f, _u32, _vp, _u32]),
    "sphx_tile_contour_fetch": (_i, [_vp, _vp, _vp, C.POINTER(_u32)]),
    "sphx_multi_particle_fields": (_i, [_vp, _u32, C.POINTER(SphxMultiFieldsOut), C.POINTER(C.c_uint64)]),
    "sphx_tile_owned_count": (_i, [_vp, C.POINTER(_u32)]),
    "sphx_tile_particle_fields_enqueue": (_i, [_vp, _u32, _u32]),
    "sphx_tile_particle_fields_fetch": (_i, [_vp, C.POINTER(SphxFieldsOut), _vp, _u32, C.POINTER(_u32)]),
    "sphx_render_fit": (_i, [_u32, _u32, _f, _f, _f, _f, C.POINTER(SphxRenderView)]),
    "sphx_render": (_i, [_vp, C.POINTER(SphxRenderView), _u32, C.POINTER(SphxRenderOut)]),
    "sphx_multi_render": (_i, [_vp, C.POINTER(SphxRenderView), _u32, C.POINTER(SphxRenderOut)]),
    "sphx_multi_render_layer": (_i, [_vp, C.POINTER(SphxRenderView), _u32, C.POINTER(SphxRenderLayer)]),
    "sphx_render_merge": (_i, [_u32, _u32, C.POINTER(SphxRenderLayer), _u32, C.POINTER(SphxRenderLayer)]),
    "sphx_tile_render_layer": (_i, [_vp, C.POINTER(SphxRenderView), _u32, C.POINTER(SphxRenderLayer)]),
    "sphx_tile_render_window": (_i, [_vp, C.POINTER(SphxRenderView), _u32, C.POINTER(_u32), C.POINTER(SphxRenderLayer)]),
    "sphx_clear_cached": (_i, [_vp]),
    "sphx_step_begin": (_i, [_vp, _f, C.POINTER(_f)]),
    "sphx_step_begin_law": (_i, [_vp, _f, _vp, _vp]),
    "sphx_timer_law_of": (_i, [_vp, _f, _vp]),
    "sphx_timer_set_target_frame": (None, [_vp, _u64]),
    "sphx_timer_on_step_started": (None, [_vp]),
    "sphx_step_finish": (_i, [_vp, _f, C.POINTER(SphxStepStats)]),
    "sphx_update_neighborhood": (_i, [_vp]),
    "sphx_update_densities": (_i, [_vp, _i]),
    "sphx_compute_alpha": (_i, [_vp]),
    "sphx_download_solver_state": (_i, [_vp, _vp, _vp, _vp]),
    "sphx_download_neighbors": (_i, [_vp, _vp, _vp, C.POINTER(_u64)]),
    "sphx_download_cells": (_i, [_vp, _i, _vp, _vp, C.POINTER(_u32)]),
    "sphx_grid_info": (_i, [_vp, _i, C.POINTER(_u32)]),
    "sphx_last_flags": (_u32, [_vp]),
    "sphx_get_constants": (_i, [_vp, _vp]),
    "sphx_get_viscosity": (_i, [_vp, C.POINTER(_u32), C.POINTER(_f), C.POINTER(_f)]),
    "sphx_reserve": (_i, [_vp, _u32]),
    "sphx_tile_configure": (_i, [_vp, _i, _u32, _u32, _u32, _i, _i]),
    "sphx_tile_upload": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "sphx_tile_pack": (_i, [_vp, _vp, _vp, _u32]),
    "sphx_tile_apply": (_i, [_vp, _vp, _vp, _u32]),
    "sphx_tile_count_kept": (_i, [_vp]),
    "sphx_sub_regrid": (_i, [_vp, C.POINTER(_u32)]),
    "sphx_sub_regrid_div": (_i, [_vp, C.POINTER(_u32)]),
    "sphx_sub_regrid_warm": (_i, [_vp, C.POINTER(_u32)]),
    "sphx_sub_nonpressure": (_i, [_vp, _f, C.POINTER(_f)]),
    "sphx_sub_predict": (_i, [_vp, _f]),
    "sphx_sub_warmstart": (_i, [_vp, _i, _f]),
    "sphx_sub_iteration": (_i, [_vp, _i, _f, _i, C.POINTER(C.c_double), C.POINTER(_u64)]),
    "sphx_sub_predict_iteration": (_i, [_vp, _f, C.POINTER(C.c_double), C.POINTER(_u64)]),
    "sphx_tile_band_packs": (_i, [_vp, C.POINTER(_u32)]),
    "sphx_tile_send_counts": (_i, [_vp, _vp, _u32, _u32, C.POINTER(_u32)]),
    "sphx_sub_advect": (_i, [_vp, _f]),
    "sphx_shm_open": (_vp, [C.c_char_p, _i, _i]),
    "sphx_shm_allreduce": (_i, [_vp, _vp, _i, _i, _vp]),
    "sphx_shm_allgather": (_i, [_vp, _vp, _i, _vp]),
    "sphx_shm_abort": (None, [_vp]),
    "sphx_sub_run_ahead": (_i, [_vp, C.c_float]),
    "sphx_tile_carry_warmstart": (_i, [_vp, _i, _i]),
    "sphx_set_tiling_invariant": (_i, [_vp, _i]),
    "sphx_tile_defer_advect": (_i, [_vp, _i]),
    "sphx_build_stats": (_i, [_vp, _vp, _vp, _vp]),
    "sphx_shm_close": (None, [_vp]),
    "sphx_tile_configure_rect": (_i, [_vp, _vp, _u32, _vp, _u32]),
    "sphx_tile_pack_n": (_i, [_vp, _vp, _u32, _u32]),
    "sphx_tile_apply_n": (_i, [_vp, _vp, _u32, _u32]),
    "sphx_tile_advect_pack_n": (_i, [_vp, _f, _vp, _u32, _u32]),
    "sphx_view_request": (_i, [_vp, _u32, C.POINTER(_u32)]),
    "sphx_view_fetch": (_i, [_vp, _i, C.POINTER(C.POINTER(_f)), C.POINTER(_u32)]),
    "sphx_synchronize": (_i, [_vp]),
    "sphx_set_stream": (_i, [_vp, _vp]),
    "sphx_profile_enable": (_i, [_vp, _i]),
    "sphx_profile_reset": (_i, [_vp]),
    "sphx_profile_filter": (_i, [_vp, C.c_char_p, _u32]),
    "sphx_profile_get": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "sphx_profile_event_overhead": (_i, [_vp, C.POINTER(C.c_double)]),
    "sphx_multi_default_options": (_i, [C.POINTER(SphxMultiOptions)]),
    "sphx_multi_create": (_i, [C.POINTER(SphxParams), C.POINTER(C.c_int), _i, C.POINTER(SphxMultiOptions), C.POINTER(_vp)]),
    "sphx_multi_create_rank": (_i, [C.POINTER(SphxParams), _i, C.POINTER(SphxCommOps), C.c_char_p, _i, _i, C.POINTER(SphxMultiOptions), C.POINTER(_vp)]),
    "sphx_multi_destroy": (None, [_vp]),
    "sphx_multi_last_error": (C.c_char_p, [_vp]),
    "sphx_multi_set_layout": (_i, [_vp, _i, _vp, _u32]),
    "sphx_multi_set_grid_layout": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "sphx_multi_set_boundary": (_i, [_vp, _vp, _u32]),
    "sphx_multi_upload": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "sphx_multi_clear_cached": (_i, [_vp]),
    "sphx_multi_step_begin": (_i, [_vp, _f, C.POINTER(_f)]),
    "sphx_multi_step_finish": (_i, [_vp, _f, C.POINTER(SphxStepStats)]),
    "sphx_multi_synchronize": (_i, [_vp]),
    "sphx_multi_num_owned": (_u64, [_vp]),
    "sphx_multi_download": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "sphx_multi_info": (_i, [_vp, C.POINTER(SphxMultiInfo)]),
    "sphx_multi_tile_ctx": (_vp, [_vp, _u32]),
    "sphx_multi_simulation_step": (_i, [_vp, _vp, _f, C.POINTER(SphxStepStats)]),
    "sphx_multi_simulation_steps": (_i, [_vp, _vp, _f, _u32, C.POINTER(SphxStepStats), C.POINTER(_u32)]),
    # host mirror
    "sphx_world_create": (_vp, [_f, _f, _f]),
    "sphx_world_destroy": (None, [_vp]),
    "sphx_world_properties": (None, [_vp, _vp]),
    "sphx_world_remove_all_fluid_particles": (None, [_vp]),
    "sphx_world_remove_all_boundary_particles": (None, [_vp]),
    "sphx_world_add_fluid_rect": (None, [_vp, _f, _f, _f, _f, _f]),
    "sphx_world_add_boundary_thick_line": (None, [_vp, _f, _f, _f, _f, _u32]),
    "sphx_world_add_boundary_line": (None, [_vp, _f, _f, _f, _f]),
    "sphx_world_reset_fluid": (None, [_vp, _f]),
    "sphx_world_num_dynamic_particles": (_u32, [_vp]),
    "sphx_world_num_boundary_particles": (_u32, [_vp]),
    "sphx_world_positions": (_vp, [_vp]),
    "sphx_world_velocities": (_vp, [_vp]),
    "sphx_world_densities": (_vp, [_vp]),
    "sphx_world_boundary": (_vp, [_vp]),
    "sphx_world_particle_ids": (_vp, [_vp]),
    "sphx_world_set_particles": (None, [_vp, _vp, _vp, _u32]),
    "sphx_world_set_boundary": (None, [_vp, _vp, _u32]),
    "sphx_world_set_gravity": (None, [_vp, _f, _f]),
    "sphx_duration_from_secs_f32": (_u64, [_f]),
    "sphx_duration_as_secs_f32": (_f, [_u64]),
    "sphx_timer_create_adaptive": (_vp, [_u64, _u64, _f]),
    "sphx_timer_create_fixed": (_vp, [_u64]),
    "sphx_timer_destroy": (None, [_vp]),
    "sphx_timer_restart": (None, [_vp]),
    "sphx_timer_simulation_step_ns": (_u64, [_vp]),
    "sphx_timer_update_simulation_step": (_u64, [_vp, _f, _f]),
    "sphx_timer_total_simulated_ns": (_u64, [_vp]),
    "sphx_timer_num_steps": (_u32, [_vp]),
    "sphx_timer_get_state": (_i, [_vp, C.POINTER(SphxTimerState)]),
    "sphx_timer_set_state": (_i, [_vp, C.POINTER(SphxTimerState)]),
    "sphx_solver_save": (_i, [_vp, _vp, _vp, C.c_char_p]),
    "sphx_solver_load": (_i, [_vp, _vp, _vp, C.c_char_p]),
    "sphx_solver_multi_checkpoint": (_i, [_vp, _vp, _vp, C.c_char_p]),
    "sphx_solver_multi_restore": (_i, [_vp, _vp, _vp, C.c_char_p]),
    "sphx_solver_create_dfsph": (_i, [_vp, C.POINTER(SphxParams), C.POINTER(_vp)]),
    "sphx_solver_create_wcsph": (_i, [_vp, C.POINTER(SphxParams), C.POINTER(_vp)]),
    "sphx_solver_create_dfsph_multi": (_i, [_vp, C.POINTER(SphxParams), C.POINTER(C.c_int), _i, C.POINTER(SphxMultiOptions), C.POINTER(_vp)]),
    "sphx_wcsph_step_begin": (_i, [_vp, _f, C.POINTER(_f)]),
    "sphx_wcsph_step_finish": (_i, [_vp, _f, C.POINTER(SphxStepStats)]),
    "sphx_solver_destroy": (None, [_vp]),
    "sphx_solver_clear_cached_data": (None, [_vp]),
    "sphx_solver_simulation_step": (_i, [_vp, _vp, _vp, _i, C.POINTER(SphxStepStats)]),
    "sphx_solver_simulation_steps": (_i, [_vp, _vp, _vp, _i, _u32, C.POINTER(SphxStepStats), C.POINTER(_u32)]),
    "sphx_solver_sync_world": (_i, [_vp, _vp]),
    "sphx_solver_append": (_i, [_vp, _vp, _vp, _vp, _u32, _i, C.POINTER(_u32)]),
    "sphx_solver_remove": (_i, [_vp, _vp, C.POINTER(SphxRect), _u32, _u32, _i, C.POINTER(_u32)]),
    "sphx_solver_ctx": (_vp, [_vp]),
    "sphx_solver_multi": (_vp, [_vp]),
    "sphx_solver_last_error": (C.c_char_p, [_vp]),
}

_lib = None


def lib():
    """Load libsphx.so.  Raises if it has not been built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (hipcc, gfx950).  yasph2d_amd has no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own HIP runtime.  If libsphx pulled in /opt/rocm's copy first, torch.cuda would later
    # find "No HIP GPUs" in the same process (two runtimes fighting over the device).  Loading torch first makes both share one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


class SphxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sphx error {code}: {msg}")
        self.code = code
