"""Host-side mirror of the reference interface over the C ABI of libefusion_hip.so (include/ef_hip.h).

``ElasticFusion`` keeps the reference's public names (Core/ElasticFusion.h:40-255): processFrame, predict,
get_T_wc, getTick/setTick, getTimeDelta, getConfidenceThreshold, setRgbOnly/..., savePly; the ctor takes the
reference's argument names plus the Resolution / Intrinsics singletons as plain arguments.
``ops`` exposes the operator tier (the cudafuncs.cuh free functions and the GLSL passes) on numpy arrays:
each call uploads, runs the HIP kernel(s) through the C ABI and downloads — it is what the parity tests use.

There is NO fallback: if the shared library is missing or no GPU is present, everything here raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# EF_HIP_LIB: developer override (A/B of two builds on one GPU box, tools/ab_bench.py); never a CPU fallback
LIB_PATH = os.environ.get("EF_HIP_LIB") or os.path.join(_HERE, "libefusion_hip.so")
_lib = None

c_f, c_i, c_u32, P = C.c_float, C.c_int, C.c_uint32, C.c_void_p


class EFError(RuntimeError):
    pass


class ef_config(C.Structure):
    _fields_ = [("width", c_i), ("height", c_i), ("fx", c_f), ("fy", c_f), ("cx", c_f), ("cy", c_f),
                ("time_delta", c_i), ("confidence", c_f), ("depth_cut", c_f), ("icp_weight", c_f),
                ("fast_odom", c_i), ("so3", c_i), ("frame_to_frame_rgb", c_i), ("pyramid", c_i), ("rgb_only", c_i),
                ("close_loops", c_i), ("max_surfels", c_u32), ("device", c_i), ("stream", P)]


class ef_intr(C.Structure):
    _fields_ = [("fx", c_f), ("fy", c_f), ("cx", c_f), ("cy", c_f)]


class ef_cam(C.Structure):
    _fields_ = [("cols", c_i), ("rows", c_i), ("fx", c_f), ("fy", c_f), ("cx", c_f), ("cy", c_f)]


class ef_gn_state(C.Structure):   # what one Gauss-Newton update hands to the next (ef_op_gn_update)
    _fields_ = [("Rcurr", c_f * 9), ("tcurr", c_f * 3), ("resultRt", C.c_double * 16), ("krkinv", c_f * 9), ("kt", c_f * 3),
                ("lastRGBErrorLevel", c_f), ("rgb_broken", c_i)]


class ef_gn_update_args(C.Structure):
    _fields_ = [("sums", c_f * 58), ("prev", ef_gn_state), ("Rprev", c_f * 9), ("tprev", c_f * 3), ("count", c_i), ("sigma", c_i),
                ("icp", c_i), ("rgb", c_i), ("rgb_only", c_i), ("icp_weight", c_f), ("knext", ef_intr), ("level_changes", c_i),
                ("split_tail", c_i)]


class ef_model_maps_op(C.Structure):   # ef_op_model_maps
    _fields_ = [("cols", c_i), ("rows", c_i), ("pred_vertex", P), ("pred_normal", P), ("fill_vertex", P), ("fill_normal", P), ("pred_image", P),
                ("fill_image", P), ("R", c_f * 9), ("t", c_f * 3), ("max_depth_rgb", c_f), ("camera_frame", c_i), ("force_fill_image", c_i),
                ("tally", c_i), ("dense_count", C.c_uint), ("dense_samples", c_i), ("vmap", P * 3), ("nmap", P * 3), ("depth0", P), ("last0", P),
                ("joint", c_i), ("raw", P), ("rgb3", P), ("depth_cut", c_f), ("filtered", P), ("metric", P), ("metric_filtered", P), ("next0", P)]


class ef_track_end_out(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("logged", C.c_double * 16), ("T_cw", c_f * 16), ("pose_f", c_f * 16),
                ("R_wc_f", c_f * 9), ("t_wc_f", c_f * 3), ("weighting", c_f)]


class ef_timing(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", c_f)]


class ef_kernel_time(C.Structure):   # ef_get_kernel_timing / ef_get_splat_timing / ef_get_tracker_timing
    _fields_ = [("name", C.c_char_p), ("avg_us", c_f), ("launches", c_i), ("bytes_per_launch", C.c_double), ("bytes_per_launch_survey", C.c_double)]


class ef_tracker_plan(C.Structure):
    _fields_ = [("script", c_i), ("n_small", c_i), ("n_iter", c_i), ("levels", C.c_ulonglong), ("res_bytes", C.c_uint), ("res_budget", C.c_uint)]


class ef_render_params(C.Structure):
    _fields_ = [("width", c_i), ("height", c_i), ("fx", c_f), ("fy", c_f), ("cx", c_f), ("cy", c_f), ("T_wc", C.c_double * 16),
                ("max_depth", c_f), ("threshold", c_f), ("draw_unstable", c_i), ("color_type", c_i), ("draw_window", c_i),
                ("time", c_i), ("time_delta", c_i)]


class ef_register_params(C.Structure):
    _fields_ = [("max_dist", c_f), ("min_conf", c_f), ("min_normal_cos", c_f), ("max_iterations", c_i), ("min_pairs", c_i),
                ("stop_translation", C.c_double), ("stop_rotation", C.c_double)]


class ef_register_sums(C.Structure):
    _fields_ = [("A", C.c_double * 36), ("b", C.c_double * 6), ("e", C.c_double), ("pairs", c_u32), ("points", c_u32)]


class ef_register_result(C.Structure):
    _fields_ = [("status", c_i), ("iterations", c_i), ("pairs", c_u32), ("rms_first", C.c_double), ("rms_last", C.c_double),
                ("A", C.c_double * 36)]


class ef_map_selection(C.Structure):
    _fields_ = [("tests", c_u32), ("T_bw", C.c_double * 16), ("box_min", c_f * 3), ("box_max", c_f * 3), ("conf_min", c_f), ("conf_max", c_f),
                ("init_time_min", c_i), ("init_time_max", c_i), ("last_time_min", c_i), ("last_time_max", c_i), ("radius_min", c_f),
                ("radius_max", c_f), ("id_min", c_u32), ("id_max", c_u32), ("label_class", c_i), ("label_min_prob", c_f)]


class ef_insert_params(C.Structure):
    _fields_ = [("gate", c_i), ("min_separation", c_f), ("min_conf", c_f), ("min_normal_cos", c_f), ("init_time", c_i), ("last_time", c_i)]


class ef_insert_result(C.Structure):
    _fields_ = [("inserted", c_u32), ("duplicates", c_u32), ("skipped", c_u32), ("count_after", c_u32)]


class ef_fuse_params(C.Structure):
    _fields_ = [("min_separation", c_f), ("min_conf", c_f), ("min_normal_cos", c_f), ("append", c_i), ("init_time", c_i), ("last_time", c_i)]


class ef_fuse_result(C.Structure):
    _fields_ = [("fused", c_u32), ("absorbed", c_u32), ("weightless", c_u32), ("novel", c_u32), ("skipped", c_u32), ("inserted", c_u32),
                ("count_after", c_u32)]


class ef_thin_params(C.Structure):
    _fields_ = [("cell", c_f), ("keep", c_i)]


class ef_thin_result(C.Structure):
    _fields_ = [("participants", c_u32), ("cells", c_u32), ("removed", c_u32), ("count_after", c_u32)]


class ef_carve_params(C.Structure):
    _fields_ = [("width", c_i), ("height", c_i), ("fx", c_f), ("fy", c_f), ("cx", c_f), ("cy", c_f), ("min_depth", c_f), ("max_depth", c_f),
                ("margin", c_f), ("margin_quad", c_f), ("window", c_i), ("min_views", c_i), ("protect", c_i)]


class ef_carve_views(C.Structure):
    _fields_ = [("n", c_i), ("T_wc16", C.c_void_p), ("depth", C.c_void_p)]


class ef_carve_result(C.Structure):
    _fields_ = [("participants", c_u32), ("observed", c_u32), ("free_space", c_u32), ("protected_", c_u32), ("removed", c_u32),
                ("count_after", c_u32)]


class ef_outlier_params(C.Structure):
    _fields_ = [("mode", c_i), ("radius", c_f), ("cell", c_f), ("min_conf", c_f), ("min_neighbors", c_i), ("k", c_i), ("std_ratio", c_f),
                ("max_mean_dist", c_f), ("flag_sparse", c_i)]


class ef_outlier_result(C.Structure):
    _fields_ = [("sum", C.c_double), ("sum_sq", C.c_double), ("participants", c_u32), ("measured", c_u32), ("sparse", c_u32),
                ("outliers", c_u32), ("count_after", c_u32), ("threshold", c_f)]


class ef_component_params(C.Structure):
    _fields_ = [("radius", c_f), ("cell", c_f), ("min_conf", c_f), ("min_size", c_u32), ("max_size", c_u32)]


class ef_component_result(C.Structure):
    _fields_ = [("nodes", c_u32), ("components", c_u32), ("largest", c_u32), ("rejected_rows", c_u32), ("rejected_components", c_u32),
                ("count_after", c_u32), ("status", c_u32)]


class ef_plane_params(C.Structure):
    _fields_ = [("distance", c_f), ("normal_cos", c_f), ("min_conf", c_f), ("hypotheses", c_u32), ("seed", c_u32), ("max_planes", c_u32),
                ("min_inliers", c_u32), ("refine", c_u32), ("axis_mode", c_u32), ("axis", c_f * 3), ("axis_bound", c_f)]


class ef_plane_model(C.Structure):
    _fields_ = [("normal", c_f * 3), ("d", c_f), ("inliers", c_u32), ("sampled_inliers", c_u32), ("hypothesis", c_u32),
                ("valid_hypotheses", c_u32), ("participants", c_u32), ("thickness", c_f)]


class ef_plane_result(C.Structure):
    _fields_ = [("nodes", c_u32), ("planes", c_u32), ("on_rows", c_u32), ("off_rows", c_u32), ("count_after", c_u32)]


class ef_normal_params(C.Structure):
    _fields_ = [("radius", c_f), ("cell", c_f), ("min_conf", c_f), ("k", c_i), ("min_neighbors", c_i), ("orientation", c_i), ("side", c_i),
                ("viewpoint", c_f * 3), ("line_ratio", c_f), ("max_curvature", c_f), ("set_radius", c_i), ("radius_scale", c_f)]


class ef_normal_result(C.Structure):
    _fields_ = [("participants", c_u32), ("estimated", c_u32), ("sparse", c_u32), ("degenerate", c_u32), ("flipped", c_u32), ("listed", c_u32)]


class ef_region_params(C.Structure):
    _fields_ = [("radius", c_f), ("cell", c_f), ("min_conf", c_f), ("k", c_i), ("min_neighbors", c_i), ("line_ratio", c_f),
                ("normal_source", c_i), ("two_sided", c_i), ("min_normal_cos", c_f), ("max_curvature", c_f), ("attach_borders", c_i),
                ("min_size", c_u32), ("max_size", c_u32)]


class ef_region_result(C.Structure):
    _fields_ = [("nodes", c_u32), ("cores", c_u32), ("borders", c_u32), ("attached", c_u32), ("unassigned", c_u32), ("regions", c_u32),
                ("largest", c_u32), ("rejected_rows", c_u32), ("rejected_regions", c_u32), ("listed", c_u32), ("count_after", c_u32),
                ("status", c_u32)]


class ef_smooth_params(C.Structure):
    _fields_ = [("radius", c_f), ("cell", c_f), ("min_conf", c_f), ("k", c_i), ("min_neighbors", c_i), ("iterations", c_i), ("weighting", c_i),
                ("normal_gate", c_i), ("min_normal_cos", c_f), ("strength", c_f), ("max_shift", c_f), ("line_ratio", c_f), ("set_normal", c_i),
                ("shift_threshold", c_f)]


class ef_smooth_result(C.Structure):
    _fields_ = [("participants", c_u32), ("smoothed", c_u32), ("sparse", c_u32), ("degenerate", c_u32), ("clamped", c_u32), ("moved", c_u32),
                ("listed", c_u32), ("largest_shift", c_f)]


class ef_boundary_params(C.Structure):
    _fields_ = [("radius", c_f), ("cell", c_f), ("min_conf", c_f), ("k", c_i), ("min_neighbors", c_i), ("normal_source", c_i), ("line_ratio", c_f),
                ("max_gap", c_f), ("min_size", c_u32), ("max_size", c_u32)]


class ef_boundary_result(C.Structure):
    _fields_ = [("participants", c_u32), ("interior", c_u32), ("boundary", c_u32), ("sparse", c_u32), ("degenerate", c_u32), ("loops", c_u32),
                ("accepted", c_u32), ("largest", c_u32), ("listed", c_u32), ("status", c_u32)]


CARVE_MAX_VIEWS = 32   # EF_CARVE_MAX_VIEWS of include/ef_hip.h
BOUNDARY_STORED, BOUNDARY_ESTIMATED = 0, 1          # EF_BOUNDARY_STORED / _ESTIMATED of include/ef_hip.h: normal_source of ef_boundary_params
BOUNDARY_NONE, BOUNDARY_INTERIOR, BOUNDARY_BOUNDARY, BOUNDARY_SPARSE, BOUNDARY_DEGENERATE = 0, 1, 2, 3, 4   # EF_BOUNDARY_*: a row's status byte (the last four also `what`)
BOUNDARY_LOOPS_ACCEPTED, BOUNDARY_LOOPS_REJECTED = 5, 6   # EF_BOUNDARY_LOOPS_*: `what` of ef_map_boundaries_select beside the four verdicts
SMOOTH_UNIFORM, SMOOTH_COMPACT = 0, 1               # EF_SMOOTH_UNIFORM / _COMPACT of include/ef_hip.h: weighting of ef_smooth_params
SMOOTH_NONE, SMOOTH_SMOOTHED, SMOOTH_SPARSE, SMOOTH_DEGENERATE = 0, 1, 2, 3   # EF_SMOOTH_*: a row's status byte (the last three also `what`)
SMOOTH_CLAMPED, SMOOTH_SHIFTED = 4, 5               # EF_SMOOTH_CLAMPED / _SHIFTED: `what` of ef_map_smooth_select beside the three statuses
REGION_NONE = 0xFFFFFFFF                             # EF_REGION_NONE of include/ef_hip.h: the label of a row without a region
REGION_KIND_NONE, REGION_KIND_CORE, REGION_KIND_BORDER = 0, 1, 2   # EF_REGION_KIND_*: a row's kind byte
REGIONS_ESTIMATED, REGIONS_STORED = 0, 1            # EF_REGIONS_ESTIMATED / _STORED: normal_source of ef_region_params
REGIONS_REJECTED, REGIONS_ACCEPTED, REGIONS_UNASSIGNED, REGIONS_BORDERS = 0, 1, 2, 3   # EF_REGIONS_*: which rows ef_map_regions_select lists
NORMALS_KEEP_SIDE, NORMALS_VIEWPOINT = 0, 1         # EF_NORMALS_KEEP_SIDE / _VIEWPOINT of include/ef_hip.h: how an estimate is oriented
NORMAL_NONE, NORMAL_ESTIMATED, NORMAL_SPARSE, NORMAL_DEGENERATE = 0, 1, 2, 3   # EF_NORMAL_*: a row's status byte (the last three also `what`)
NORMALS_CURVED, NORMALS_FLAT = 4, 5                 # EF_NORMALS_CURVED / _FLAT: `what` of ef_map_normals_select beside the three statuses
PLANE_NONE = 0xFFFFFFFF                              # EF_PLANE_NONE of include/ef_hip.h: plane[] of a row on no found plane
PLANE_MAX_PLANES, PLANE_MAX_HYPOTHESES = 16, 4096   # EF_PLANE_MAX_*
PLANE_AXIS_OFF, PLANE_AXIS_NORMAL, PLANE_AXIS_INPLANE = 0, 1, 2   # EF_PLANE_AXIS_*: the constraint on a plane's normal
PLANES_ON, PLANES_OFF = 0, 1                        # EF_PLANES_*: which nodes ef_map_planes_select lists
COMPONENT_NONE = 0xFFFFFFFF                          # EF_COMPONENT_NONE of include/ef_hip.h: the label of a row that is no node
COMPONENTS_REJECTED, COMPONENTS_ACCEPTED = 0, 1     # EF_COMPONENTS_*: which nodes ef_map_components_select lists
OUTLIER_RADIUS, OUTLIER_STATISTICAL = 0, 1   # EF_OUTLIER_* of include/ef_hip.h: the two filters
OUTLIER_SUM_LANES = 4096                     # EF_OUTLIER_SUM_LANES: P of the summation order
THIN_KEEP_MAX_CONF, THIN_KEEP_NEWEST, THIN_KEEP_FIRST = 0, 1, 2   # EF_THIN_KEEP_* of include/ef_hip.h
THIN_ROWS_REMOVED, THIN_ROWS_REPRESENTATIVES = 0, 1               # EF_THIN_ROWS_*
INSERT_KEEP = -1   # EF_INSERT_KEEP of include/ef_hip.h
FUSE_SKIPPED, FUSE_NOVEL, FUSE_WEIGHTLESS, FUSE_ABSORBED, FUSE_FUSED, FUSE_INSERTED = 0, 1, 2, 3, 4, 5   # EF_FUSE_*: a record's outcome byte
ROW_NONE = 0xFFFFFFFF

# EF_SEL_* of include/ef_hip.h
SEL_BOX, SEL_CONF, SEL_INIT_TIME, SEL_LAST_TIME, SEL_RADIUS, SEL_ID, SEL_LABEL, SEL_INVERT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x100

REG_CONVERGED, REG_MAX_ITERATIONS, REG_TOO_FEW_PAIRS, REG_DEGENERATE = 0, 1, 2, 3   # EF_REG_* of include/ef_hip.h
REG_STATUS = {REG_CONVERGED: "CONVERGED", REG_MAX_ITERATIONS: "MAX_ITERATIONS", REG_TOO_FEW_PAIRS: "TOO_FEW_PAIRS", REG_DEGENERATE: "DEGENERATE"}


def _sums_dict(s: ef_register_sums) -> dict:
    return {"A": np.array(s.A, np.float64).reshape(6, 6), "b": np.array(s.b, np.float64), "e": float(s.e), "pairs": int(s.pairs),
            "points": int(s.points)}


def _sums_struct(sums) -> ef_register_sums:
    if isinstance(sums, ef_register_sums):
        return sums
    s = ef_register_sums()
    s.A[:] = np.ascontiguousarray(sums["A"], np.float64).reshape(36).tolist()
    s.b[:] = np.ascontiguousarray(sums["b"], np.float64).reshape(6).tolist()
    s.e = float(sums.get("e", 0.0))
    s.pairs = int(sums.get("pairs", 0))
    s.points = int(sums.get("points", 0))
    return s


def _pose16(T):
    if T is None:
        return None, None
    a = np.ascontiguousarray(T, np.float64).reshape(16)
    return a, _ptr(a)


def register_update(sums, T=None):
    """ef_register_update (plain double on the host: needs neither a context nor a GPU): solves A xi = b and returns
    (exp(xi) T as 4 x 4 float64, xi, degenerate); sums is what registerStep returns (or any dict with "A" 6 x 6 and "b" 6)."""
    s = _sums_struct(sums)
    keep, pT = _pose16(T)
    out = np.zeros(16, np.float64)
    xi = np.zeros(6, np.float64)
    rc = lib().ef_register_update(C.byref(s), pT, _ptr(out), _ptr(xi))
    if rc not in (0, REG_DEGENERATE):
        _chk(rc)
    return out.reshape(4, 4), xi, rc == REG_DEGENERATE


def boundary_gap(radians: float) -> float:
    """ef_boundary_gap_from_angle (plain double on the host: needs neither a context nor a GPU): the max_gap of ef_boundary_params, in TURN
    units, for an angle inside (0, 2 pi); exact at the quarter turns (pi / 2 -> 1, pi -> 2)"""
    g = C.c_double(0.0)
    _chk(lib().ef_boundary_gap_from_angle(float(radians), C.byref(g)))
    return g.value


def boundary_angle(gap: float) -> float:
    """the inverse of boundary_gap: the angle in radians of a gap in TURN units inside (0, 4).  gap = n + sin b / (sin b + cos b) with n whole
    quarter turns and b in [0, pi / 2), so tan b = f / (1 - f) for the fraction f"""
    gap = float(gap)
    if not 0.0 < gap < 4.0:
        raise ValueError("a gap lies inside (0, 4)")
    n = math.floor(gap)
    f = gap - n
    return n * (math.pi / 2) + math.atan2(f, 1.0 - f)


DATATERM = np.dtype([("zero", np.int16, 2), ("one", np.int16, 2), ("diff", np.float32), ("valid", np.uint8),
                     ("pad", np.uint8, 3)])


def lib():
    """Loads libefusion_hip.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EFError(f"{LIB_PATH} not built: run `python -m elasticfusion_amd.build` (hipcc, gfx950). "
                          "There is no CPU fallback for this engine.")
        _lib = _bind(C.CDLL(LIB_PATH))
    return _lib


def use_library(path: str | None = None):
    """Rebinds this module to another build of the same C ABI (build.FAST_LIB, the opt-in fast-order build; an A/B build given by path).
    None = back to the product library.  The next lib() loads it and declares its signatures anew."""
    global _lib, LIB_PATH
    _lib = None
    LIB_PATH = path or os.path.join(_HERE, "libefusion_hip.so")


HEADER = os.path.join(os.path.dirname(_HERE), "include", "ef_hip.h")
_PROTOTYPE = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w+[\s*]+)(ef_\w+)\s*\(([^()]*)\)\s*;", re.M)
_SCALARS = {"int": c_i, "unsigned": c_u32, "uint32_t": c_u32, "float": c_f, "double": C.c_double, "size_t": C.c_size_t, "int64_t": C.c_int64}
_RETURNS = {"int": c_i, "void": None, "float": c_f}
_signatures = None


def _kind(decl, table, max_words, prototype):
    """the ctypes type of a return type (max_words 1) or of one parameter with or without its name (max_words 2)"""
    words = re.sub(r"\*|\bconst\b", " ", decl).split()
    if "*" in decl:
        return C.c_char_p if table is _RETURNS and words == ["char"] else P
    if not 1 <= len(words) <= max_words or words[0] not in table:
        raise EFError(f"{HEADER}: no ctypes kind for '{decl.strip()}' of {prototype}")
    return table[words[0]]


def signatures() -> dict:
    """name -> (restype, argtypes) of every ef_* function include/ef_hip.h declares.  The kinds form a closed set: any pointer is a
    c_void_p (byref, arrays, None, a CFUNCTYPE object, an int at full width), scalars and callback typedefs go by the tables, a
    const char* is returned as bytes; a prototype with anything else raises."""
    global _signatures
    if _signatures is None:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)
        text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
        params = dict(_SCALARS, ef_fern_tracker=FERN_TRACKER, ef_loop_solver=LOOP_SOLVER, ef_view_fetch=P)
        found = {}
        for ret, name, args in _PROTOTYPE.findall(text):
            prototype = " ".join(f"{ret}{name}({args})".split())
            args = [] if args.strip() in ("", "void") else args.split(",")
            found[name] = (_kind(ret, _RETURNS, 1, prototype), [_kind(a, params, 2, prototype) for a in args])
        _signatures = found
    return _signatures


def _bind(library, prefix="ef_", exported_as=None):
    """the one place signatures are declared: restype and argtypes of every header prototype `prefix`* the library exports (a variant
    build may lack a symbol; exported_as: the prefix another implementation of the same C interface exports them under)"""
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(library, (exported_as or prefix) + name[len(prefix):], None) if name.startswith(prefix) else None
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return library


def _chk(rc: int, ctx=None):
    if rc != 0:
        msg = lib().ef_last_error(ctx)
        raise EFError(f"libefusion_hip error {rc}: {msg.decode() if msg else ''}")


def device_count() -> int:
    n = c_i(0)
    rc = lib().ef_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _ptr(a: np.ndarray):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(P)


def _dev(v):
    """a device pointer given as int, c_void_p or None, as a pointer parameter takes it (at full width)"""
    return v if v is None or isinstance(v, P) else int(v)


class DevBuf:
    """A raw HIP allocation owned through the C ABI (ef_dev_alloc / ef_dev_free)."""

    def __init__(self, nbytes: int, fill: int | None = 0):
        self.p = P()
        self.nbytes = int(nbytes)
        _chk(lib().ef_dev_alloc(C.byref(self.p), self.nbytes))
        if fill is not None:
            _chk(lib().ef_dev_memset(self.p, fill, self.nbytes))

    @classmethod
    def from_array(cls, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes, fill=None)
        if a.nbytes:
            _chk(lib().ef_dev_upload(b.p, _ptr(a), a.nbytes))
        return b

    def to_array(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes, (out.nbytes, self.nbytes)
        if out.nbytes:
            _chk(lib().ef_dev_download(_ptr(out), self.p, out.nbytes))
        return out

    def __del__(self):
        if getattr(self, "p", None):
            try:
                lib().ef_dev_free(self.p)
            except Exception:
                pass
            self.p = None


def default_config(**kw) -> ef_config:
    cfg = ef_config()
    lib().ef_default_config(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config field {k}")
        setattr(cfg, k, v)
    return cfg


def write_freiburg(path: str, T_wc, timestamps):
    """ef_write_freiburg on host arrays (no GPU): the reference's trajectory dump (ElasticFusion.cpp:112-139)"""
    T = np.ascontiguousarray(T_wc, np.float64).reshape(-1, 16)
    ts = np.ascontiguousarray(timestamps, np.int64)
    assert len(T) == len(ts)
    _chk(lib().ef_write_freiburg(path.encode(), _ptr(T), _ptr(ts), len(T)))


class GlobalLoop(C.Structure):   # ef_global_loop
    _fields_ = [("attempted", c_i), ("closest", c_i), ("n_constraints", c_i), ("accepted", c_i), ("graph_nodes", c_i), ("icp_error", c_f),
                ("icp_count", c_f), ("T_wc_recovery", C.c_double * 16)]


class RelocState(C.Structure):   # ef_reloc_state
    _fields_ = [("lost", c_i), ("tracking_ok", c_i), ("tracking_count", c_i), ("last_frame_recovery", c_i)]


class LocalLoop(C.Structure):   # ef_local_loop
    _fields_ = [("attempted", c_i), ("cov_ok", c_i), ("gates_ok", c_i), ("n_constraints", c_i), ("applied", c_i),
                ("graph_nodes", c_i), ("graph_capacity", c_i), ("reserved_", c_i), ("stats", c_f * 6), ("cov_diag", C.c_double * 6),
                ("T_wc_curr", C.c_double * 16), ("T_wc_est", C.c_double * 16)]


LOOP_SOLVER = C.CFUNCTYPE(c_i, C.c_void_p, C.POINTER(LocalLoop), C.POINTER(C.c_double), c_i, C.POINTER(c_f), C.POINTER(c_i))


def solve_local_deformation(nodes4, constraints, src_time, last_deform_time=0):
    """ef_solve_local_deformation on host arrays (no GPU): -> (graph [n, 16] float32, error, mean constraint error) or None"""
    nodes4 = np.ascontiguousarray(nodes4, np.float32).reshape(-1, 4)
    cons = np.ascontiguousarray(constraints, np.float64).reshape(-1, 8)
    g = np.zeros((max(len(nodes4), 1), 16), np.float32)
    e, m = c_f(0), c_f(0)
    rc = lib().ef_solve_local_deformation(_ptr(nodes4), len(nodes4), _ptr(cons), len(cons), int(src_time),
                                          int(last_deform_time), _ptr(g), C.byref(e), C.byref(m))
    return (g[:len(nodes4)], e.value, m.value) if rc == 0 else None


class GraphConstraint(C.Structure):   # ef_graph_constraint
    _fields_ = [("src", C.c_double * 3), ("target", C.c_double * 3), ("src_time", C.c_int64), ("target_time", C.c_int64), ("relative", c_i), ("pin", c_i)]


def graph_constraints(rows):
    """rows of (src xyz, target xyz, src_time, target_time, relative, pin) -> ef_graph_constraint array"""
    arr = (GraphConstraint * max(len(rows), 1))()
    for a, (src, target, st, tt, rel, pin) in zip(arr, rows):
        a.src[:] = [float(x) for x in src]
        a.target[:] = [float(x) for x in target]
        a.src_time, a.target_time, a.relative, a.pin = int(st), int(tt), int(bool(rel)), int(bool(pin))
    return arr


def solve_deformation(nodes4, rows, fernMatch=False, last_deform_time=0, poses=None, pose_times=None, gates=None):
    """ef_solve_deformation (Deformation::constrain in general form, host only).  rows as graph_constraints takes them.
    -> dict(accepted, graph [n, 16], error, meanConsErr, poses [k, 4, 4] deformed along, new_relative rows)"""
    nodes4 = np.ascontiguousarray(nodes4, np.float32).reshape(-1, 4)
    cons = graph_constraints(rows)
    g = np.zeros((max(len(nodes4), 1), 16), np.float32)
    P16 = np.ascontiguousarray(np.zeros((0, 4, 4)) if poses is None else poses, np.float64).reshape(-1, 4, 4).copy()
    times = np.ascontiguousarray([] if pose_times is None else pose_times, np.int64)
    assert len(times) == len(P16)
    rel = (GraphConstraint * max(len(rows), 1))()
    n_rel, e, m = c_i(0), c_f(0), c_f(0)
    gz = None if gates is None else (c_f * 3)(*[float(x) for x in gates])
    rc = lib().ef_solve_deformation_gated(_ptr(nodes4), len(nodes4), cons, len(rows), int(bool(fernMatch)), int(last_deform_time),
                                          _ptr(P16) if len(P16) else None, _ptr(times) if len(P16) else None, len(P16), _ptr(g), C.byref(e),
                                          C.byref(m), rel, C.byref(n_rel), gz)
    if rc not in (0, -4):
        _chk(rc)
    new_rel = [(list(r.src), list(r.target), r.src_time, r.target_time, True, False) for r in rel[:n_rel.value]]
    return dict(accepted=rc == 0, graph=g[:len(nodes4)], error=e.value, meanConsErr=m.value, poses=P16, new_relative=new_rel)


FERN_TRACKER = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(c_f), C.POINTER(c_f), C.POINTER(C.c_double), C.POINTER(c_f), C.POINTER(c_f),
                           C.POINTER(C.c_double), C.POINTER(c_f), C.POINTER(c_f))


def _fern_tracker(tracker, w, h):
    """tracker(fern_verts, fern_norms, T_wc_fern, verts, norms, T_wc) -> (T_wc_est, icp_error, icp_count) on w x h views as an ef_fern_tracker"""
    px = w * h * 4

    def tramp(_user, fv, fn, Tf, cv, cn, Tio, err, cnt):
        A = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt).copy()
        Te, e, k = tracker(A(fv, px, np.float32).reshape(h, w, 4), A(fn, px, np.float32).reshape(h, w, 4), A(Tf, 16, np.float64).reshape(4, 4),
                           A(cv, px, np.float32).reshape(h, w, 4), A(cn, px, np.float32).reshape(h, w, 4), A(Tio, 16, np.float64).reshape(4, 4))
        Te = np.ascontiguousarray(Te, np.float64).reshape(16)
        for i in range(16):
            Tio[i] = Te[i]
        err[0], cnt[0] = float(e), float(k)

    return FERN_TRACKER(tramp)


class Ferns:
    """The reference's fern database (Core/Ferns.h:35-184) over ef_ferns_* — host-side, no GPU.  Same members where they make
    sense on arrays: addFrame, findFrame (-> T_wc_est, constraints [n, 6]), lastClosest, frames (count), conservatory (table).
    Views are the 1/8-resolution images ``ElasticFusion.imageResized(..., 8)`` returns: rgb [h, w, 3|4] uint8, verts / norms
    [h, w, 4] float32.  ``tracker(fern_verts, fern_norms, T_wc_fern, verts, norms, T_wc) -> (T_wc_est, icp_error, icp_count)``
    stands where the reference runs its 80x60 RGBDOdometry (Ferns.cpp:243-258)."""

    _prefix = "ef_ferns_"      # symbol prefix and library are overridable: a subclass can bind another implementation of the same C interface

    def _library(self):
        return lib()

    def _f(self, name):
        return getattr(self._L, self._prefix + name)

    def __init__(self, n=500, maxDepth=3000, photoThresh=115.0, width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, seed=0):
        self._h = None
        self._L = self._library()
        if self._L is not _lib:     # another implementation: the header's ef_ferns_* signatures, under its prefix
            _bind(self._L, Ferns._prefix, self._prefix)
        self.num, self.w, self.h = int(n), width // 8, height // 8
        self._h = self._f("create")(int(n), int(maxDepth), photoThresh, int(width), int(height), fx, fy, cx, cy, int(seed))
        if not self._h:
            raise EFError("ef_ferns_create: bad arguments")

    _owned = True

    def close(self):
        if self._h and self._owned:
            self._f("destroy")(self._h)
        self._h = None

    __del__ = close

    def _view(self, rgb, verts, norms):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.shape[:2] == (self.h, self.w) and rgb.shape[2] in (3, 4), rgb.shape
        verts = np.ascontiguousarray(verts, np.float32).reshape(self.h, self.w, 4)
        norms = np.ascontiguousarray(norms, np.float32).reshape(self.h, self.w, 4)
        return rgb, verts, norms

    @property
    def conservatory(self):
        t = np.zeros((self.num, 6), np.int32)
        _chk(self._f("get_table")(self._h, _ptr(t)))
        return t

    @conservatory.setter
    def conservatory(self, table):
        t = np.ascontiguousarray(table, np.int32).reshape(self.num, 6)
        _chk(self._f("set_table")(self._h, _ptr(t)))

    def addFrame(self, rgb, verts, norms, T_wc, srcTime, threshold) -> bool:
        rgb, verts, norms = self._view(rgb, verts, norms)
        T = np.ascontiguousarray(T_wc, np.float64).reshape(4, 4)
        rc = self._f("add_frame")(self._h, _ptr(rgb), rgb.shape[2], _ptr(verts), _ptr(norms), _ptr(T), int(srcTime), float(threshold))
        if rc < 0:
            _chk(rc)
        return rc == 1

    def findFrame(self, rgb, verts, norms, T_wc, time, lost, tracker):
        rgb, verts, norms = self._view(rgb, verts, norms)
        T = np.ascontiguousarray(T_wc, np.float64).reshape(4, 4)
        cb = _fern_tracker(tracker, self.w, self.h)
        T_est = np.zeros((4, 4), np.float64)
        cons = np.zeros((self.num, 6), np.float64)
        n = c_i(0)
        rc = self._f("find_frame")(self._h, _ptr(rgb), rgb.shape[2], _ptr(verts), _ptr(norms), _ptr(T), int(time), int(bool(lost)), cb, None,
                                       _ptr(T_est), _ptr(cons), self.num, C.byref(n))
        if rc < -1:
            _chk(rc)
        return T_est, cons[:n.value].copy()

    @property
    def lastClosest(self) -> int:
        return self._f("last_closest")(self._h)

    def __len__(self):
        return self._f("count")(self._h)

    def frame(self, i):
        """-> dict(codes, goodCodes, srcTime, T_wc, rgb, verts, norms) of stored frame i"""
        codes = np.zeros(self.num, np.uint8)
        good, src = c_i(0), c_i(0)
        T = np.zeros((4, 4), np.float64)
        rgb = np.zeros((self.h, self.w, 3), np.uint8)
        verts = np.zeros((self.h, self.w, 4), np.float32)
        norms = np.zeros((self.h, self.w, 4), np.float32)
        _chk(self._f("get_frame")(self._h, int(i), _ptr(codes), C.byref(good), C.byref(src), _ptr(T), _ptr(rgb), _ptr(verts), _ptr(norms)))
        return dict(codes=codes, goodCodes=good.value, srcTime=src.value, T_wc=T, rgb=rgb, verts=verts, norms=norms)

    def setFramePose(self, i, T_wc):
        T = np.ascontiguousarray(T_wc, np.float64).reshape(4, 4)
        _chk(self._f("set_frame_pose")(self._h, int(i), _ptr(T)))

    def blockHDAware(self, a, b) -> float:
        return self._f("block_hd_aware")(self._h, int(a), int(b))

    def photometricCheck(self, rgb, verts, T_wc_est, i) -> float:
        rgb, verts, _ = self._view(rgb, verts, verts)
        T = np.ascontiguousarray(T_wc_est, np.float64).reshape(4, 4)
        return self._f("photometric_check")(self._h, _ptr(rgb), rgb.shape[2], _ptr(verts), _ptr(T), int(i))


class Closure:
    """ef_closure_*: the host side of the loop closures around the fern database (ElasticFusion.cpp:392-445, 511-526, 588-589, 609-618)."""

    def __init__(self, n=500, depthCut=3.0, photoThresh=115.0, fernThresh=0.3095, width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, seed=0,
                 _borrowed=None):
        L = lib()
        self._owned = _borrowed is None
        self.w, self.h = width // 8, height // 8
        self._h = _borrowed if _borrowed is not None else L.ef_closure_create(int(n), depthCut, photoThresh, fernThresh, int(width), int(height), fx, fy,
                                                                              cx, cy, int(seed))
        if not self._h:
            raise EFError("ef_closure_create: bad arguments")
        self.ferns = Ferns.__new__(Ferns)        # a view of the database the closure object owns
        self.ferns._L, self.ferns._h, self.ferns._owned = L, L.ef_closure_ferns(self._h), False
        self.ferns.num, self.ferns.w, self.ferns.h = int(n), self.w, self.h

    def close(self):
        if self._h and self._owned:
            lib().ef_closure_destroy(self._h)
        self._h = None

    __del__ = close

    def _view(self, rgb, verts, norms):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        return rgb, np.ascontiguousarray(verts, np.float32).reshape(self.h, self.w, 4), np.ascontiguousarray(norms, np.float32).reshape(self.h, self.w, 4)

    def globalClosure(self, rgb, verts, norms, T_wc, tick, tracker, nodes4):
        """-> (accepted, T_recovery [4, 4], graph [nodes, 16]); tracker as in Ferns.findFrame"""
        rgb, verts, norms = self._view(rgb, verts, norms)
        T = np.ascontiguousarray(T_wc, np.float64).reshape(4, 4)
        nodes4 = np.ascontiguousarray(nodes4, np.float32).reshape(-1, 4)
        cb = _fern_tracker(tracker, self.w, self.h)
        Tr = np.zeros((4, 4), np.float64)
        g = np.zeros((1024, 16), np.float32)
        n = c_i(0)
        rc = lib().ef_closure_global(self._h, _ptr(rgb), rgb.shape[2], _ptr(verts), _ptr(norms), _ptr(T), int(tick), cb, None, _ptr(nodes4), len(nodes4),
                                     _ptr(Tr), _ptr(g), C.byref(n))
        if rc < 0:
            _chk(rc)
        return rc == 1, Tr, g[:n.value].copy()

    def relocalise(self, rgb, verts, norms, T_wc, tick, tracker):
        """a LOST camera's mid-frame step (ef_closure_relocalise: Ferns::findFrame with lost = true) -> (found, T_recovery [4, 4])"""
        rgb, verts, norms = self._view(rgb, verts, norms)
        T = np.ascontiguousarray(T_wc, np.float64).reshape(4, 4)
        cb = _fern_tracker(tracker, self.w, self.h)
        Tr = np.zeros((4, 4), np.float64)
        rc = lib().ef_closure_relocalise(self._h, _ptr(rgb), rgb.shape[2], _ptr(verts), _ptr(norms), _ptr(T), int(tick), cb, None, _ptr(Tr))
        if rc < 0:
            _chk(rc)
        return rc == 1, Tr

    def logPose(self, T_wc, tick):
        """the end of a lost camera's frame (ef_closure_log_pose): the pose joins the trajectory, no keyframe is stored"""
        T = np.ascontiguousarray(T_wc, np.float64).reshape(4, 4)
        _chk(lib().ef_closure_log_pose(self._h, _ptr(T), int(tick)))

    def localClosure(self, constraints8, tick, nodes4):
        cons = np.ascontiguousarray(constraints8, np.float64).reshape(-1, 8)
        nodes4 = np.ascontiguousarray(nodes4, np.float32).reshape(-1, 4)
        g = np.zeros((1024, 16), np.float32)
        n = c_i(0)
        rc = lib().ef_closure_local(self._h, _ptr(cons), len(cons), int(tick), _ptr(nodes4), len(nodes4), _ptr(g), C.byref(n))
        if rc < 0:
            _chk(rc)
        return rc == 1, g[:n.value].copy()

    def endFrame(self, rgb, verts, norms, T_wc, tick) -> bool:
        rgb, verts, norms = self._view(rgb, verts, norms)
        T = np.ascontiguousarray(T_wc, np.float64).reshape(4, 4)
        rc = lib().ef_closure_end_frame(self._h, _ptr(rgb), rgb.shape[2], _ptr(verts), _ptr(norms), _ptr(T), int(tick))
        if rc < 0:
            _chk(rc)
        return rc == 1

    def setGates(self, entry=0.06, meanConsErr=3e-4, energy=0.12):
        """the three gates of the global deformation (ef_closure_set_gates); defaults = the reference's constants"""
        _chk(lib().ef_closure_set_gates(self._h, entry, meanConsErr, energy))

    def counts(self):
        v = [c_i(0) for _ in range(4)]
        _chk(lib().ef_closure_counts(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("deforms", "fernDeforms", "relative", "trajectory"), (x.value for x in v)))

    @staticmethod
    def _rows(arr, n):
        return np.array([list(r.src) + list(r.target) + [r.src_time, r.target_time, r.relative, r.pin] for r in arr[:n]], np.float64).reshape(-1, 10)

    def lastRows(self):
        """-> (rows [n, 10] handed to the optimiser by the last closure, its energy, its mean constraint error)"""
        n = lib().ef_closure_last_rows(self._h, None, 0, None, None)
        arr = (GraphConstraint * max(n, 1))()
        e, m = c_f(0), c_f(0)
        lib().ef_closure_last_rows(self._h, arr, n, C.byref(e), C.byref(m))
        return self._rows(arr, n), e.value, m.value

    def relativeConstraints(self):
        n = lib().ef_closure_relative(self._h, None, 0)
        arr = (GraphConstraint * max(n, 1))()
        lib().ef_closure_relative(self._h, arr, n)
        return self._rows(arr, n)

    def trajectory(self):
        n = lib().ef_closure_trajectory(self._h, None, 0)
        T = np.zeros((max(n, 1), 4, 4), np.float64)
        lib().ef_closure_trajectory(self._h, _ptr(T), n)
        return T[:n]


class ElasticFusion:
    """Mirror of ``class ElasticFusion`` (Core/ElasticFusion.h) over the C ABI."""

    IMAGES = dict(depth_filtered=(0, np.uint16, 1), depth_metric=(1, np.float32, 1), depth_metric_filtered=(2, np.float32, 1),
                  image=(3, np.uint8, 4), vertex=(4, np.float32, 4), normal=(5, np.float32, 4), time=(6, np.uint16, 1),
                  fill_image=(7, np.uint8, 4), fill_vertex=(8, np.float32, 4), fill_normal=(9, np.float32, 4),
                  index=(10, np.uint32, 1), vertConf=(11, np.float32, 4), colorTime=(12, np.float32, 4), normRad=(13, np.float32, 4),
                  old_image=(14, np.uint8, 4), old_vertex=(15, np.float32, 4), old_normal=(16, np.float32, 4), old_time=(17, np.uint16, 1))
    TRACKER = dict(vmap_curr=(0, np.float32, 3), nmap_curr=(1, np.float32, 3), vmap_g_prev=(2, np.float32, 3),
                   nmap_g_prev=(3, np.float32, 3), lastDepth=(4, np.float32, 1), nextDepth=(5, np.float32, 1),
                   lastImage=(6, np.uint8, 1), nextImage=(7, np.uint8, 1), lastNextImage=(8, np.uint8, 1),
                   dIdx=(9, np.int16, 1), dIdy=(10, np.int16, 1), depth_tmp=(11, np.uint16, 1), rgbMask=(12, np.uint8, 1),
                   corres=(13, np.uint32, 1))

    def __init__(self, width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, timeDelta=2147483647 // 2,
                 confidence=10.0, depthCut=3.0, icpThresh=10.0, fastOdom=False, so3=True, frameToFrameRGB=False,
                 closeLoops=False, maxSurfels=4 * 1024 * 1024, device=0, stream=None, countThresh=35000, errThresh=5e-05,
                 covThresh=1e-05, reloc=False):
        cfg = default_config(width=width, height=height, fx=fx, fy=fy, cx=cx, cy=cy, time_delta=timeDelta,
                             confidence=confidence, depth_cut=depthCut, icp_weight=icpThresh, fast_odom=int(fastOdom),
                             so3=int(so3), frame_to_frame_rgb=int(frameToFrameRGB), close_loops=int(closeLoops),
                             max_surfels=maxSurfels, device=device, stream=stream)
        self.cfg = cfg
        self.h = P()
        _chk(lib().ef_create(C.byref(cfg), C.byref(self.h)))
        self._solver = None
        if closeLoops:
            _chk(lib().ef_set_loop_thresholds(self.h, countThresh, errThresh, covThresh), self.h)
        if reloc:
            self.setRelocalisation(True)

    def close(self):
        if getattr(self, "h", None):
            lib().ef_destroy(self.h)
            self.h = None

    __del__ = close

    # --- frame tier ---
    def processFrame(self, rgb: np.ndarray, depth: np.ndarray, timestamp: int = 0, weightMultiplier: float = 1.0, in_T_wc=None):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        assert rgb.size == self.cfg.width * self.cfg.height * 3 and depth.size == self.cfg.width * self.cfg.height
        T = None if in_T_wc is None else np.ascontiguousarray(in_T_wc, np.float64).reshape(16)
        _chk(lib().ef_process_frame(self.h, _ptr(rgb), _ptr(depth), timestamp, weightMultiplier,
                                    _ptr(T) if T is not None else None), self.h)

    def processFrameDevice(self, rgb_dev, depth_dev, timestamp: int = 0, weightMultiplier: float = 1.0, in_T_wc=None):
        """rgb_dev / depth_dev: raw device pointers (int or c_void_p) of frames already resident in HBM."""
        T = None if in_T_wc is None else np.ascontiguousarray(in_T_wc, np.float64).reshape(16)
        _chk(lib().ef_process_frame_dev(self.h, _dev(rgb_dev), _dev(depth_dev), timestamp, weightMultiplier,
                                        _ptr(T) if T is not None else None), self.h)

    # --- local loop closure, front half (ElasticFusion.cpp:447-527; closeLoops=True contexts) ---
    def setLoopSolver(self, fn):
        """fn(info: LocalLoop, constraints [n, 8] float64) -> None (reject) | graph [nodes, 16] float32 (accept).
        Stands where Deformation::constrain stands in the reference; called inside processFrame."""
        if fn is None:
            self._solver = None
            _chk(lib().ef_set_loop_solver(self.h, LOOP_SOLVER(), None), self.h)   # (a NULL callback: a CFUNCTYPE parameter takes no None)
            return

        def tramp(user, info, cons, n, graph_out, nodes_out):
            c = np.ctypeslib.as_array(cons, shape=(n, 8)).copy() if n > 0 else np.zeros((0, 8))
            g = fn(info.contents, c)
            if g is None:
                return 0
            g = np.ascontiguousarray(g, np.float32).reshape(-1, 16)
            nodes_out[0] = len(g)
            if len(g) > info.contents.graph_capacity:   # graph_out only has room for graph_capacity nodes: let the engine reject the count
                return 1
            C.memmove(graph_out, g.ctypes.data, g.nbytes)
            return 1
        self._solver = LOOP_SOLVER(tramp)
        _chk(lib().ef_set_loop_solver(self.h, self._solver, None), self.h)

    # --- relocalisation (the reference constructor's `reloc`; ElasticFusion.cpp:326-366, 411-413, 536, 601-604) ---
    def setRelocalisation(self, on=True):
        _chk(lib().ef_set_relocalisation(self.h, int(on)), self.h)

    def relocState(self) -> RelocState:
        s = RelocState()
        _chk(lib().ef_get_relocalisation(self.h, C.byref(s)), self.h)
        return s

    def getLost(self) -> bool:
        return bool(self.relocState().lost)

    # --- global loop closure (ElasticFusion.cpp:392-445, 609-618; closeLoops=True contexts) ---
    def enableGlobalClosure(self, n=500, photoThresh=115.0, fernThresh=0.3095, seed=0):
        """ef_enable_global_closure: the fern database, its 1/8-resolution tracker and the closure bookkeeping inside processFrame"""
        _chk(lib().ef_enable_global_closure(self.h, int(n), photoThresh, fernThresh, int(seed)), self.h)
        self._closure = Closure(n=n, width=self.cfg.width, height=self.cfg.height, _borrowed=lib().ef_get_closure(self.h))
        return self._closure

    def getFerns(self):
        """the fern database of the context (Ferns view: len() = frames.size(), lastClosest(), frame(i))"""
        return self.closure().ferns

    def closure(self):
        # every look at the closure object goes through ef_get_closure: the engine defers the end-of-frame bookkeeping (keyframe decision,
        # trajectory entry) to its next synchronisation point, and ef_get_closure is one
        lib().ef_get_closure(self.h)
        return self._closure

    def globalLoop(self) -> GlobalLoop:
        g = GlobalLoop()
        _chk(lib().ef_get_global_loop(self.h, C.byref(g)), self.h)
        return g

    def useBuiltinLoopSolver(self, on=True):
        """the built-in deformation-graph optimiser where Deformation::constrain stands (ef_use_builtin_loop_solver)"""
        _chk(lib().ef_use_builtin_loop_solver(self.h, int(on)), self.h)

    def localLoop(self):
        """(info, constraints [n, 8]) of the last processFrame."""
        info = LocalLoop()
        cons = np.zeros((4096, 8), np.float64)
        n = c_i(0)
        _chk(lib().ef_get_local_loop(self.h, C.byref(info), _ptr(cons), len(cons), C.byref(n)), self.h)
        return info, cons[:n.value].copy()

    def imageResized(self, name: str, factor: int) -> np.ndarray:
        """Resize::{image,vertex,time}: the named predicted / fill-in / inactive image, NEAREST-downsampled on the device."""
        which, dt, ch = self.IMAGES[name]
        h, w = self.cfg.height // factor, self.cfg.width // factor
        out = np.zeros((h, w, ch) if ch > 1 else (h, w), dt)
        _chk(lib().ef_get_image_resized(self.h, which, factor, _ptr(out), out.nbytes), self.h)
        return out

    def sampleGraph(self, max_nodes=1024):
        """Deformation::sampleGraphModel: [n, 4] float32 {x, y, z, initTime} of every 5000th surfel."""
        out = np.zeros((max_nodes, 4), np.float32)
        n = c_i(0)
        _chk(lib().ef_sample_graph(self.h, _ptr(out), max_nodes, C.byref(n)), self.h)
        return out[:n.value].copy()

    def predict(self):
        _chk(lib().ef_predict(self.h), self.h)

    def setResidentLevels(self, on=True):
        """level-resident pixel data in the persistent tracker launch (ef_set_resident_levels; default on)"""
        _chk(lib().ef_set_resident_levels(self.h, int(on)), self.h)

    def setFusedStep(self, on=True):
        """level-0 update step inside the correspondence-search launch (ef_set_fused_step)"""
        _chk(lib().ef_set_fused_step(self.h, int(on)), self.h)

    def setTrackOnly(self, on=True):
        """odometry on a frozen map: track + predict, no fusion (ef_set_track_only; BASELINE.json configs[4])"""
        _chk(lib().ef_set_track_only(self.h, int(on)), self.h)

    def setPersistentTracker(self, on=True):
        """small pyramid levels + SO(3) in one persistent launch (default) or one launch per step (ef_set_persistent_tracker)"""
        _chk(lib().ef_set_persistent_tracker(self.h, int(on)), self.h)

    def debugInjectTrackerAbort(self):
        """test hook (ef_debug_inject_tracker_abort): what a persistent tracker launch leaves when a wait timed out after admission"""
        _chk(lib().ef_debug_inject_tracker_abort(self.h), self.h)

    def synchronize(self):
        _chk(lib().ef_synchronize(self.h), self.h)

    def trackerFallbacks(self) -> int:
        """persistent tracker launches that ran on one workgroup because other work held part of the chip (ef_get_tracker_fallbacks)"""
        n = c_i(0)
        _chk(lib().ef_get_tracker_fallbacks(self.h, C.byref(n)), self.h)
        return n.value

    def trackerPlan(self) -> dict:
        """which launches the last tracked frame ran (ef_get_tracker_plan): script 0 / 1 / 2, n_small, n_iter, levels (one per iteration inside the
        one launch), res_bytes, res_budget; host state only, synchronises nothing"""
        p = ef_tracker_plan()
        _chk(lib().ef_get_tracker_plan(self.h, C.byref(p)), self.h)
        n = p.n_iter if p.script == 1 else p.n_small
        return dict(script=p.script, n_small=p.n_small, n_iter=p.n_iter, levels=[(p.levels >> (2 * i)) & 3 for i in range(n)],
                    res_bytes=p.res_bytes, res_budget=p.res_budget)

    def debugOccupy(self, workgroups: int, microseconds: int):
        """test hook: CU-filling workgroups spinning on a stream of their own (ef_debug_occupy)"""
        _chk(lib().ef_debug_occupy(self.h, int(workgroups), int(microseconds)), self.h)

    def stream(self) -> int:
        return int(lib().ef_stream(self.h) or 0)

    def get_T_wc(self) -> np.ndarray:
        T = np.zeros(16, np.float64)
        _chk(lib().ef_get_pose(self.h, _ptr(T)), self.h)
        return T.reshape(4, 4)

    def getTick(self) -> int:
        t = c_i(0)
        _chk(lib().ef_get_tick(self.h, C.byref(t)), self.h)
        return t.value

    def setTick(self, v: int):
        _chk(lib().ef_set_tick(self.h, v), self.h)

    def getTimeDelta(self) -> int:
        return self.cfg.time_delta

    def getConfidenceThreshold(self) -> float:
        return self.cfg.confidence

    def getMaxDepthProcessed(self) -> float:
        return 20.0

    def trackingStats(self):
        out = np.zeros(6, np.float32)
        A = np.zeros((6, 6), np.float64)
        b = np.zeros(6, np.float64)
        _chk(lib().ef_get_tracking_stats(self.h, _ptr(out), _ptr(A), _ptr(b)), self.h)
        return out, A, b

    def getCovariance(self) -> np.ndarray:
        c = np.zeros(36, np.float64)
        _chk(lib().ef_get_covariance(self.h, _ptr(c)), self.h)
        return c.reshape(6, 6)

    def trajectory(self):
        n = c_i(0)
        _chk(lib().ef_get_trajectory(self.h, None, None, 2**31 - 1, C.byref(n)), self.h)   # how many poses are logged (one per processed frame)
        cap = max(int(n.value), 1)
        T = np.zeros((cap, 16), np.float64)
        ts = np.zeros(cap, np.int64)
        _chk(lib().ef_get_trajectory(self.h, _ptr(T), _ptr(ts), cap, C.byref(n)), self.h)
        return T[:n.value].reshape(-1, 4, 4).copy(), ts[:n.value].copy()

    def lastCount(self) -> int:
        n = c_u32(0)
        _chk(lib().ef_map_count(self.h, C.byref(n)), self.h)
        return n.value

    def downloadMap(self) -> np.ndarray:
        n = self.lastCount()
        out = np.zeros((max(n, 1), 12), np.float32)
        got = c_u32(0)
        _chk(lib().ef_map_download(self.h, _ptr(out), n, C.byref(got)), self.h)
        return out[:got.value].copy()

    # --- GlobalModel::renderPointCloud without OpenGL (ef_render_model) ---
    RENDER_OUTPUTS = dict(rgba=(np.uint8, 4), depth=(np.float32, 1), vertex=(np.float32, 4), normal=(np.float32, 4), index=(np.uint32, 1))

    def renderParams(self, T_wc=None, width=None, height=None, fx=None, fy=None, cx=None, cy=None, threshold=None, drawUnstable=False,
                     drawNormals=False, drawColors=False, drawWindow=False, drawTimes=False, time=None, timeDelta=None,
                     maxDepth=1000.0) -> ef_render_params:
        """ef_render_params: None = the context's default (ef_default_render_params: frame camera, current pose, getConfidenceThreshold(),
        getTick(), getTimeDelta()); the colour type is the reference's drawNormals ? 1 : drawColors ? 2 : drawTimes ? 3 : 0"""
        p = ef_render_params()
        _chk(lib().ef_default_render_params(self.h, C.byref(p)), self.h)
        if T_wc is not None:
            p.T_wc[:] = [float(v) for v in np.asarray(T_wc, np.float64).reshape(16)]
        for name, v in (("width", width), ("height", height)):
            if v is not None:
                setattr(p, name, int(v))
        for name, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy), ("threshold", threshold)):
            if v is not None:
                setattr(p, name, float(v))
        if time is not None:
            p.time = int(time)
        if timeDelta is not None:
            p.time_delta = int(timeDelta)
        p.max_depth = float(maxDepth)
        p.draw_unstable = int(bool(drawUnstable))
        p.color_type = 1 if drawNormals else 2 if drawColors else 3 if drawTimes else 0
        p.draw_window = int(bool(drawWindow))
        return p

    def renderPointCloud(self, T_wc=None, width=None, height=None, fx=None, fy=None, cx=None, cy=None, threshold=None,
                         drawUnstable=False, drawNormals=False, drawColors=False, drawWindow=False, drawTimes=False, time=None,
                         timeDelta=None, maxDepth=1000.0, outputs=("rgba",)) -> dict:
        """GlobalModel::renderPointCloud (GlobalModel.cpp:286-350) into host images: the current map seen from the pinhole camera
        {width, height, fx, fy, cx, cy} at T_wc (world <- camera).  outputs: any of rgba (H x W x 4 u8), depth (H x W f32), vertex /
        normal (H x W x 4 f32, camera frame, w = confidence / radius), index (H x W u32, row of downloadMap(); 0xFFFFFFFF = nothing)."""
        p = self.renderParams(T_wc, width, height, fx, fy, cx, cy, threshold, drawUnstable, drawNormals, drawColors, drawWindow, drawTimes,
                              time, timeDelta, maxDepth)
        unknown = [o for o in outputs if o not in self.RENDER_OUTPUTS]
        if unknown:
            raise ValueError(f"unknown render outputs {unknown}")
        res = {}
        for o in outputs:
            dt, ch = self.RENDER_OUTPUTS[o]
            res[o] = np.zeros((max(p.height, 0), max(p.width, 0)) + ((ch,) if ch > 1 else ()), dt)
        args = [_ptr(res[o]) if o in res else None for o in ("rgba", "depth", "vertex", "normal", "index")]
        _chk(lib().ef_render_model(self.h, C.byref(p), *args), self.h)
        return res

    def renderPointCloudDevice(self, params: ef_render_params, rgba=None, depth=None, vertex=None, normal=None, index=None):
        """ef_render_model_dev: raw device pointers (int, c_void_p or None), enqueued on the context's stream without synchronising"""
        args = [_dev(v) for v in (rgba, depth, vertex, normal, index)]
        _chk(lib().ef_render_model_dev(self.h, C.byref(params), *args), self.h)

    # --- stable surfel IDs and per-surfel labels (ef_set_surfel_ids / ef_enable_labels / ef_fuse_labels) ---
    def _labelView(self, view):
        """renderParams keywords -> ef_render_params (None for no keywords: the C default view)"""
        if not view:
            return None
        return self.renderParams(**view)

    def setSurfelIds(self, on=True):
        """every surfel carries a uint32 ID >= 1 (downloadMap()[:, 5] viewed as uint32), unique for the context's lifetime"""
        _chk(lib().ef_set_surfel_ids(self.h, int(bool(on))), self.h)

    def surfelIds(self) -> np.ndarray:
        n = self.lastCount()
        out = np.zeros(max(n, 1), np.uint32)
        got = c_u32(0)
        _chk(lib().ef_get_surfel_ids(self.h, _ptr(out), n, C.byref(got)), self.h)
        return out[:got.value].copy()

    def enableLabels(self, numClasses: int):
        """a float32 [rows][numClasses] table that follows the map by ID (0: off)"""
        self.numClasses = int(numClasses)
        _chk(lib().ef_enable_labels(self.h, int(numClasses)), self.h)

    def fuseLabels(self, probs: np.ndarray, **view):
        """one observation: probs C x H x W float32 for the view given by renderParams keywords (none: the frame camera, drawUnstable)"""
        p = self._labelView(view)
        probs = np.ascontiguousarray(probs, np.float32)
        _chk(lib().ef_fuse_labels(self.h, None if p is None else C.byref(p), _ptr(probs)), self.h)

    def fuseLabelsDevice(self, probs_dev, params: ef_render_params | None = None):
        """ef_fuse_labels_dev: a raw device pointer to C x H x W float32, enqueued on the context's stream"""
        _chk(lib().ef_fuse_labels_dev(self.h, None if params is None else C.byref(params), _dev(probs_dev)), self.h)

    def labels(self):
        """(ids, probs): the current rows' IDs and their C floats each, in map row order"""
        n = self.lastCount()
        ids = np.zeros(max(n, 1), np.uint32)
        probs = np.zeros((max(n, 1), max(getattr(self, "numClasses", 1), 1)), np.float32)
        got = c_u32(0)
        _chk(lib().ef_get_labels(self.h, _ptr(ids), _ptr(probs), n, C.byref(got)), self.h)
        return ids[:got.value].copy(), probs[:got.value].copy()

    def setLabels(self, probs: np.ndarray):
        """the whole table: one row of C floats per surfel, in surfelIds() order"""
        probs = np.ascontiguousarray(probs, np.float32).reshape(-1, getattr(self, "numClasses", 1))
        _chk(lib().ef_set_labels(self.h, _ptr(probs), len(probs)), self.h)

    def renderLabels(self, **view):
        """(label H x W int32, prob H x W float32) of the view given by renderParams keywords; -1 / 0 where nothing is drawn"""
        p = self.renderParams(**view)
        label = np.zeros((p.height, p.width), np.int32)
        prob = np.zeros((p.height, p.width), np.float32)
        _chk(lib().ef_render_labels(self.h, C.byref(p), _ptr(label), _ptr(prob)), self.h)
        return label, prob

    def renderLabelsDevice(self, params: ef_render_params, label=None, prob=None):
        """ef_render_labels_dev: raw device pointers (int, c_void_p or None), enqueued on the context's stream"""
        args = [_dev(v) for v in (label, prob)]
        _chk(lib().ef_render_labels_dev(self.h, C.byref(params), *args), self.h)

    # --- spatial index and nearest-surfel / kNN queries (ef_query_nearest / ef_query_knn) ---
    QUERY_DEFAULT_CELL = 0.02   # EF_QUERY_DEFAULT_CELL of include/ef_hip.h

    def setQueryCell(self, cell_m: float):
        """the index grid's cell edge in metres; results never depend on it"""
        _chk(lib().ef_set_query_cell(self.h, cell_m), self.h)

    def debugQueryLanes(self, lanes: int):
        _chk(lib().ef_debug_query_lanes(self.h, lanes), self.h)

    def queryNearest(self, points, max_dist: float, min_conf: float = -1.0, ids: bool = False):
        """per point (n x 3) the nearest surfel with confidence > min_conf within max_dist, ties to the lower row: (rows uint32, dist = sqrt(d2),
        plane distance along the surfel's normal[, ids]); a miss is row 0xFFFFFFFF, dist inf, plane 0, id 0.  min_conf < 0: every surfel."""
        row, d2, *rest = self.queryNearestRaw(points, max_dist, min_conf, ids)
        return (row, np.sqrt(d2), *rest)

    def queryNearestRaw(self, points, max_dist: float, min_conf: float = -1.0, ids: bool = False):
        """(rows, dist2, plane[, ids]) exactly as ef_query_nearest writes them (dist2 not rooted)"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(pts)
        row = np.zeros(max(n, 1), np.uint32)
        d2 = np.zeros(max(n, 1), np.float32)
        plane = np.zeros(max(n, 1), np.float32)
        sid = np.zeros(max(n, 1), np.uint32) if ids else None
        _chk(lib().ef_query_nearest(self.h, _ptr(pts), n, max_dist, min_conf, _ptr(row), _ptr(sid) if ids else None, _ptr(d2), _ptr(plane)), self.h)
        return (row[:n], d2[:n], plane[:n], sid[:n]) if ids else (row[:n], d2[:n], plane[:n])

    def queryKnn(self, points, k: int, max_dist: float, min_conf: float = -1.0):
        """per point the first min(k, eligible) surfels in (d2, row) order: (rows n x k uint32, dist2 n x k float32, count n uint32); unused slots
        are misses (0xFFFFFFFF, inf); count is the number of ALL surfels within max_dist and may exceed k"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n, k = len(pts), int(k)
        kk = min(max(k, 1), 16)
        rows = np.zeros((max(n, 1), kk), np.uint32)
        d2 = np.zeros((max(n, 1), kk), np.float32)
        cnt = np.zeros(max(n, 1), np.uint32)
        _chk(lib().ef_query_knn(self.h, _ptr(pts), n, k, max_dist, min_conf, _ptr(rows), _ptr(d2), _ptr(cnt)), self.h)
        return rows[:n], d2[:n], cnt[:n]

    def queryNearestDevice(self, points_dev, n: int, max_dist: float, min_conf: float = -1.0, row=None, ids=None, dist2=None, plane=None):
        """ef_query_nearest_dev: raw device pointers (int, c_void_p or None), enqueued on the context's stream"""
        args = [_dev(v) for v in (points_dev, row, ids, dist2, plane)]
        _chk(lib().ef_query_nearest_dev(self.h, args[0], n, max_dist, min_conf, *args[1:]), self.h)

    def queryKnnDevice(self, points_dev, n: int, k: int, max_dist: float, min_conf: float = -1.0, rows=None, dist2=None, count=None):
        """ef_query_knn_dev: raw device pointers (int, c_void_p or None), enqueued on the context's stream"""
        args = [_dev(v) for v in (points_dev, rows, dist2, count)]
        _chk(lib().ef_query_knn_dev(self.h, args[0], n, int(k), max_dist, min_conf, *args[1:]), self.h)

    # --- rigid registration of a point set against the map (ef_register_step / ef_register_cloud) ---
    def registerParams(self, **kw) -> ef_register_params:
        """ef_default_register_params with fields replaced by keyword"""
        return self._params(ef_register_params, lib().ef_default_register_params, kw, "registration")

    def _params(self, struct_type, default_fn, kw, what):
        """the library's defaults (default_fn fills a struct_type) with fields replaced by keyword"""
        p = struct_type()
        _chk(default_fn(self.h, C.byref(p)), self.h)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown {what} parameter {k}")
            setattr(p, k, v)
        return p

    def _registerArgs(self, points, normals, params, kw):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert nrm is None or len(nrm) == len(pts), (len(pts), len(nrm))
        if params is None:
            params = self.registerParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        return pts, nrm, params

    def registerStep(self, points, normals=None, T=None, params: ef_register_params | None = None, pairs: bool = False, **kw):
        """one point-to-plane step of the cloud (n x 3, optional normals n x 3) at pose T (4 x 4, cloud -> world; None = identity):
        {"A" 6 x 6, "b", "e", "pairs", "points"[, "row" uint32 n, "plane" float32 n with pairs=True]}, all float64 sums of the device"""
        pts, nrm, params = self._registerArgs(points, normals, params, kw)
        n = len(pts)
        keep, pT = _pose16(T)
        s = ef_register_sums()
        row = np.zeros(max(n, 1), np.uint32) if pairs else None
        plane = np.zeros(max(n, 1), np.float32) if pairs else None
        _chk(lib().ef_register_step(self.h, _ptr(pts), None if nrm is None else _ptr(nrm), n, C.byref(params), pT, C.byref(s),
                                    None if row is None else _ptr(row), None if plane is None else _ptr(plane)), self.h)
        out = _sums_dict(s)
        if pairs:
            out["row"], out["plane"] = row[:n], plane[:n]
        return out

    @staticmethod
    def _registerResult(r: ef_register_result) -> dict:
        return {"status": int(r.status), "status_name": REG_STATUS.get(int(r.status), "?"), "iterations": int(r.iterations),
                "pairs": int(r.pairs), "rms_first": float(r.rms_first), "rms_last": float(r.rms_last),
                "A": np.array(r.A, np.float64).reshape(6, 6)}

    def registerCloud(self, points, normals=None, T_init=None, params: ef_register_params | None = None, pairs: bool = False, **kw):
        """point-to-plane ICP of the cloud against the map from T_init (None = identity): (T 4 x 4 float64, result dict with "status",
        "iterations", "pairs", "rms_first", "rms_last", "A"[, "row", "plane" at the returned pose with pairs=True])"""
        pts, nrm, params = self._registerArgs(points, normals, params, kw)
        n = len(pts)
        keep, pT = _pose16(T_init)
        T = np.zeros(16, np.float64)
        res = ef_register_result()
        row = np.zeros(max(n, 1), np.uint32) if pairs else None
        plane = np.zeros(max(n, 1), np.float32) if pairs else None
        _chk(lib().ef_register_cloud(self.h, _ptr(pts), None if nrm is None else _ptr(nrm), n, C.byref(params), pT, _ptr(T),
                                     C.byref(res), None if row is None else _ptr(row), None if plane is None else _ptr(plane)), self.h)
        out = self._registerResult(res)
        if pairs:
            out["row"], out["plane"] = row[:n], plane[:n]
        return T.reshape(4, 4), out

    def registerStepDevice(self, points_dev, n: int, normals_dev=None, T=None, params: ef_register_params | None = None, row=None, plane=None,
                           **kw):
        """ef_register_step_dev: raw device pointers (int, c_void_p or None) for points / normals / row / plane; waits for the sums"""
        params = params if params is not None else self.registerParams(**kw)
        args = [_dev(v) for v in (points_dev, normals_dev, row, plane)]
        keep, pT = _pose16(T)
        s = ef_register_sums()
        _chk(lib().ef_register_step_dev(self.h, args[0], args[1], n, C.byref(params), pT, C.byref(s), args[2], args[3]), self.h)
        return _sums_dict(s)

    def registerCloudDevice(self, points_dev, n: int, normals_dev=None, T_init=None, params: ef_register_params | None = None, row=None,
                            plane=None, **kw):
        """ef_register_cloud_dev: raw device pointers (int, c_void_p or None) for points / normals / row / plane"""
        params = params if params is not None else self.registerParams(**kw)
        args = [_dev(v) for v in (points_dev, normals_dev, row, plane)]
        keep, pT = _pose16(T_init)
        T = np.zeros(16, np.float64)
        res = ef_register_result()
        _chk(lib().ef_register_cloud_dev(self.h, args[0], args[1], n, C.byref(params), pT, _ptr(T), C.byref(res), args[2], args[3]),
             self.h)
        return T.reshape(4, 4), self._registerResult(res)

    # --- select, extract and erase surfels (ef_map_select / ef_map_gather / ef_map_erase) ---
    @staticmethod
    def mapSelection(**kw) -> ef_map_selection:
        """ef_default_map_selection (tests 0 = every row) with fields replaced by keyword: tests (OR of api.SEL_*), T_bw (4 x 4, box <- world),
        box_min / box_max (3 each), conf_min / conf_max, init_time_min / _max, last_time_min / _max, radius_min / _max, id_min / id_max,
        label_class, label_min_prob"""
        s = ef_map_selection()
        lib().ef_default_map_selection(C.byref(s))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise TypeError(f"unknown selection field {k}")
            if k == "T_bw":
                s.T_bw[:] = [float(x) for x in np.asarray(v, np.float64).reshape(16)]
            elif k in ("box_min", "box_max"):
                getattr(s, k)[:] = [float(x) for x in np.asarray(v, np.float32).reshape(3)]
            else:
                setattr(s, k, v)
        return s

    def _selection(self, sel, kw) -> ef_map_selection:
        if sel is None:
            return self.mapSelection(**kw)
        assert not kw, "give a selection or keywords, not both"
        return sel

    def selectSurfels(self, sel: ef_map_selection | None = None, max_rows: int | None = None, count: bool = False, **kw):
        """the selected rows of downloadMap() in ascending order (uint32), at most max_rows of them (None: all); count=True: (rows, total)"""
        sel = self._selection(sel, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        _chk(lib().ef_map_select(self.h, C.byref(sel), _ptr(rows) if cap else None, cap, C.byref(total)), self.h)
        out = rows[:min(cap, total.value)].copy()
        return (out, total.value) if count else out

    def countSurfels(self, sel: ef_map_selection | None = None, **kw) -> int:
        """the number of selected rows (ef_map_select without a list)"""
        sel = self._selection(sel, kw)
        total = c_u32(0)
        _chk(lib().ef_map_select(self.h, C.byref(sel), None, 0, C.byref(total)), self.h)
        return total.value

    def selectSurfelsDevice(self, sel: ef_map_selection, rows_dev, max_rows: int, count_dev):
        """ef_map_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0), enqueued on the context's stream"""
        args = [_dev(v) for v in (rows_dev, count_dev)]
        _chk(lib().ef_map_select_dev(self.h, C.byref(sel), args[0], int(max_rows), args[1]), self.h)

    def gatherSurfels(self, rows) -> np.ndarray:
        """downloadMap()[rows] without the download: n x 12 float32 in the order of rows (duplicates allowed; a row past the map gives zeros)"""
        rows = np.ascontiguousarray(rows, np.uint32).reshape(-1)
        n = len(rows)
        out = np.zeros((max(n, 1), 12), np.float32)
        _chk(lib().ef_map_gather(self.h, _ptr(rows) if n else None, n, _ptr(out)), self.h)
        return out[:n].copy()

    def gatherSurfelsDevice(self, rows_dev, n: int, surfels_dev):
        """ef_map_gather_dev: raw device pointers (int or c_void_p), enqueued on the context's stream"""
        args = [_dev(v) for v in (rows_dev, surfels_dev)]
        _chk(lib().ef_map_gather_dev(self.h, args[0], int(n), args[1]), self.h)

    def eraseSurfels(self, sel: ef_map_selection | None = None, **kw) -> int:
        """removes the selected surfels from the map (stable; the prediction is renewed once frames have run); returns how many went"""
        sel = self._selection(sel, kw)
        removed = c_u32(0)
        _chk(lib().ef_map_erase(self.h, C.byref(sel), C.byref(removed)), self.h)
        return removed.value

    def eraseRows(self, rows) -> int:
        """removes the named rows of downloadMap() (any order; duplicates and rows past the map are ignored); returns how many went"""
        rows = np.ascontiguousarray(rows, np.uint32).reshape(-1)
        removed = c_u32(0)
        _chk(lib().ef_map_erase_rows(self.h, _ptr(rows) if len(rows) else None, len(rows), C.byref(removed)), self.h)
        return removed.value

    def eraseRowsDevice(self, rows_dev, n: int) -> int:
        """ef_map_erase_rows_dev: a raw device pointer (int or c_void_p) to n uint32 rows; synchronises like every erase"""
        removed = c_u32(0)
        _chk(lib().ef_map_erase_rows_dev(self.h, _dev(rows_dev), int(n), C.byref(removed)), self.h)
        return removed.value

    # --- insert surfels (ef_map_insert) ---
    def insertParams(self, **kw) -> ef_insert_params:
        """ef_default_insert_params (gate 1, min_separation 0.01, min_conf -1, min_normal_cos 0.5, both times the tick) with fields replaced
        by keyword"""
        return self._params(ef_insert_params, lib().ef_default_insert_params, kw, "insert")

    def insertSurfels(self, surfels, T=None, params: ef_insert_params | None = None, rows: bool = False, n: int | None = None, **kw):
        """appends the records (n x 12 float32 in downloadMap()'s layout, or a DevBuf holding n of them: ef_map_insert_dev) moved by T (4 x 4,
        records -> world; None: copied) that pass the gate: {"inserted", "duplicates", "skipped", "count_after"}; rows=True: (result, new_row,
        match_row), uint32 per record with api.ROW_NONE where there is none.  A refused insert (EF_ECAPACITY: nothing changed) raises EFError
        with the counts in its .result"""
        if params is None:
            params = self.insertParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        return self._appendSurfels(lib().ef_map_insert, lib().ef_map_insert_dev, params, ef_insert_result, False, surfels, T, rows, n)

    def _appendSurfels(self, fn_host, fn_dev, params, result_type, with_outcome, surfels, T, rows, n):
        """insertSurfels / fuseSurfels behind their parameters: the host or the DevBuf tier by the type of surfels, one uint32 array per record
        for new_row and match_row and (with_outcome) one byte for the outcome when rows is set, the result struct as a dict"""
        keep, pT = _pose16(T)
        res = result_type()
        kinds = [(np.uint32, ROW_NONE), (np.uint32, ROW_NONE)] + ([(np.uint8, 0)] if with_outcome else [])
        if isinstance(surfels, DevBuf):
            n = surfels.nbytes // 48 if n is None else int(n)
            assert n * 48 <= surfels.nbytes, (n, surfels.nbytes)
            devs = [DevBuf(max(n, 1) * np.dtype(t).itemsize) for t, _ in kinds] if rows else [None] * len(kinds)
            rc = fn_dev(self.h, surfels.p if n else None, n, pT, C.byref(params), C.byref(res), *[d.p if rows else None for d in devs])
            arrays = [d.to_array(t, (n,)) if rows and rc == 0 else None for d, (t, _) in zip(devs, kinds)]
        else:
            rec = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
            n = len(rec)
            arrays = [np.full(max(n, 1), fill, t) if rows else None for t, fill in kinds]
            rc = fn_host(self.h, _ptr(rec) if n else None, n, pT, C.byref(params), C.byref(res), *[_ptr(a) if rows else None for a in arrays])
            if rows:
                arrays = [a[:n] for a in arrays]
        out = {k: int(getattr(res, k)) for k, _ in result_type._fields_}
        if rc != 0:
            try:
                _chk(rc, self.h)
            except EFError as e:
                e.result = out
                e.rc = rc
                raise
        return (out, *arrays) if rows else out

    # --- fuse surfels into the map (ef_map_fuse) ---
    def fuseParams(self, **kw) -> ef_fuse_params:
        """ef_default_fuse_params (the insert's defaults: min_separation 0.01, min_conf -1, min_normal_cos 0.5, both times the tick; append 1)
        with fields replaced by keyword"""
        return self._params(ef_fuse_params, lib().ef_default_fuse_params, kw, "fuse")

    def fuseSurfels(self, surfels, T=None, params: ef_fuse_params | None = None, rows: bool = False, n: int | None = None, **kw):
        """merges the records (n x 12 float32 in downloadMap()'s layout, or a DevBuf holding n of them: ef_map_fuse_dev) moved by T (4 x 4,
        records -> world; None: copied) into the map surfels they match, at most one record per surfel, and with append=1 appends those that
        match nothing as insertSurfels would: {"fused", "absorbed", "weightless", "novel", "skipped", "inserted", "count_after"}; rows=True:
        (result, new_row, match_row, outcome), uint32 per record with api.ROW_NONE where there is none and one api.FUSE_* byte per record.
        A refused fuse (EF_ECAPACITY: nothing changed) raises EFError with the counts in its .result"""
        if params is None:
            params = self.fuseParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        return self._appendSurfels(lib().ef_map_fuse, lib().ef_map_fuse_dev, params, ef_fuse_result, True, surfels, T, rows, n)

    # --- thin the map to one surfel per voxel (ef_map_thin / ef_map_thin_select) ---
    def thinParams(self, **kw) -> ef_thin_params:
        """ef_default_thin_params (cell = the default query cell, keep = THIN_KEEP_MAX_CONF) with fields replaced by keyword"""
        return self._params(ef_thin_params, lib().ef_default_thin_params, kw, "thin")

    def _thinArgs(self, params, among, kw):
        if params is None:
            params = self.thinParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    def thinSelect(self, params: ef_thin_params | None = None, among=None, representatives: bool = False, max_rows: int | None = None,
                   count: bool = False, **kw):
        """the rows a thin with these parameters would remove (or, representatives=True, keep as the one surfel of their cell) in ascending
        order (uint32), at most max_rows of them (None: all); the map does not change.  among: an ef_map_selection, a dict of mapSelection
        keywords or None (every surfel participates); other keywords are ef_thin_params fields.  count=True: (rows, total)"""
        params, among, pa = self._thinArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        what = THIN_ROWS_REPRESENTATIVES if representatives else THIN_ROWS_REMOVED
        _chk(lib().ef_map_thin_select(self.h, C.byref(params), pa, what, _ptr(rows) if cap else None, cap, C.byref(total)), self.h)
        out = rows[:min(cap, total.value)].copy()
        return (out, total.value) if count else out

    def thinSelectDevice(self, params: ef_thin_params, among, representatives: bool, rows_dev, max_rows: int, count_dev):
        """ef_map_thin_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0), enqueued on the context's stream"""
        params, among, pa = self._thinArgs(params, among, {})
        args = [_dev(v) for v in (rows_dev, count_dev)]
        what = THIN_ROWS_REPRESENTATIVES if representatives else THIN_ROWS_REMOVED
        _chk(lib().ef_map_thin_select_dev(self.h, C.byref(params), pa, what, args[0], int(max_rows), args[1]), self.h)

    def thinSurfels(self, params: ef_thin_params | None = None, among=None, **kw) -> dict:
        """removes every participant that is not the representative of its cell (ef_map_thin: what eraseRows(thinSelect(...)) leaves):
        {"participants", "cells", "removed", "count_after"}"""
        params, among, pa = self._thinArgs(params, among, kw)
        res = ef_thin_result()
        _chk(lib().ef_map_thin(self.h, C.byref(params), pa, C.byref(res)), self.h)
        return {"participants": int(res.participants), "cells": int(res.cells), "removed": int(res.removed), "count_after": int(res.count_after)}

    # --- carve free space: remove the surfels that depth views see through (ef_map_carve / ef_map_carve_select) ---
    def carveParams(self, **kw) -> ef_carve_params:
        """ef_default_carve_params (the frame camera, min_depth 0.3, max_depth = the depth cut-off, margin 0.02, margin_quad 0.0025, window 1,
        min_views 1, protect 1) with fields replaced by keyword"""
        return self._params(ef_carve_params, lib().ef_default_carve_params, kw, "carve")

    def _carveArgs(self, depths, poses, params, among, kw):
        """(params, views, among's pointer, what must stay alive).  depths: [K, H, W] or [H, W] uint16 millimetres, or a DevBuf holding K
        images of the parameters' size; poses: [K, 4, 4] T_wc, or None for the current pose with K = 1"""
        T = self.get_T_wc().reshape(1, 16) if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        if params is None:
            if not isinstance(depths, DevBuf) and "width" not in kw and "height" not in kw:
                kw = dict(kw, width=int(np.shape(depths)[-1]), height=int(np.shape(depths)[-2]))
            params = self.carveParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(depths, DevBuf):
            assert len(T) * params.width * params.height * 2 <= depths.nbytes, (len(T), depths.nbytes)
            keep, dp = depths, depths.p
        else:
            keep = np.ascontiguousarray(depths, np.uint16).reshape(-1, params.height, params.width)
            assert len(keep) == len(T), (keep.shape, T.shape)
            dp = _ptr(keep)
        views = ef_carve_views(len(T), _ptr(T), dp)
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, views, (C.byref(among) if among is not None else None), (T, keep, among)

    def carveSelect(self, depths, poses=None, params: ef_carve_params | None = None, among=None, max_rows: int | None = None,
                    count: bool = False, votes: bool = False, **kw):
        """the rows a carve with these views would remove, in ascending order (uint32), at most max_rows of them (None: all); the map does
        not change.  depths: [K, H, W] or [H, W] uint16 millimetres; poses: [K, 4, 4] T_wc or None (the current pose, K = 1); among: an
        ef_map_selection, a dict of mapSelection keywords or None (every surfel participates); other keywords are ef_carve_params fields
        (width and height default to the images').  count=True adds the total, votes=True the [rows of the map, 2] uint8 {free, support}:
        rows[, total][, votes]"""
        params, views, pa, keep = self._carveArgs(depths, poses, params, among, kw)
        n = self.lastCount() if max_rows is None or votes else 0      # (asked only where it sizes an array)
        cap = n if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        v2 = np.zeros((max(n, 1), 2), np.uint8) if votes else None
        total = c_u32(0)
        _chk(lib().ef_map_carve_select(self.h, C.byref(params), C.byref(views), pa, _ptr(rows) if cap else None, cap, C.byref(total),
                                       _ptr(v2) if votes else None), self.h)
        out = (rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((v2[:n],) if votes else ())
        return out if len(out) > 1 else out[0]

    def carveSelectDevice(self, depths_dev, poses, params: ef_carve_params, among, rows_dev, max_rows: int, count_dev, votes_dev=None):
        """ef_map_carve_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0 and for votes) for the K images, rows,
        count and votes; poses [K, 4, 4] on the host; enqueued on the context's stream"""
        T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        views = ef_carve_views(len(T), _ptr(T), _dev(depths_dev))
        _chk(lib().ef_map_carve_select_dev(self.h, C.byref(params), C.byref(views), C.byref(among) if among is not None else None,
                                           _dev(rows_dev), int(max_rows), _dev(count_dev), _dev(votes_dev)), self.h)

    def carveSurfels(self, depths, poses=None, params: ef_carve_params | None = None, among=None, **kw) -> dict:
        """removes the surfels the views see through (ef_map_carve; depths a DevBuf: ef_map_carve_dev): what eraseRows(carveSelect(...))
        leaves.  {"participants", "observed", "free_space", "protected_", "removed", "count_after"}"""
        params, views, pa, keep = self._carveArgs(depths, poses, params, among, kw)
        res = ef_carve_result()
        fn = lib().ef_map_carve_dev if isinstance(depths, DevBuf) else lib().ef_map_carve
        _chk(fn(self.h, C.byref(params), C.byref(views), pa, C.byref(res)), self.h)
        return {k: int(getattr(res, k)) for k, _ in ef_carve_result._fields_}

    # --- remove outlier surfels: neighbourhood statistics of the map (ef_map_neighbor_stats / ef_map_outliers_select / ef_map_remove_outliers) ---
    def outlierParams(self, **kw) -> ef_outlier_params:
        """ef_default_outlier_params (OUTLIER_STATISTICAL, k 8, std_ratio 2, max_mean_dist 0, flag_sparse 1, radius 0.03, min_neighbors 4,
        min_conf -1, cell 0.03) with fields replaced by keyword"""
        return self._params(ef_outlier_params, lib().ef_default_outlier_params, kw, "outlier")

    def _outlierArgs(self, params, among, kw):
        if params is None:
            params = self.outlierParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    @staticmethod
    def _outlierResult(res: ef_outlier_result) -> dict:
        return {k: (float if k in ("sum", "sum_sq") else np.float32 if k == "threshold" else int)(getattr(res, k)) for k, _ in ef_outlier_result._fields_}

    def neighborStats(self, params: ef_outlier_params | None = None, among=None, **kw):
        """(mean_dist float32, count uint32) per row of downloadMap(): the mean distance to the k nearest other surfels within radius (+inf
        with fewer than k of them, and for a row that takes no part) and the number of ALL of them; the map does not change.  among: an
        ef_map_selection, a dict of mapSelection keywords or None (every surfel participates); other keywords are ef_outlier_params fields"""
        params, among, pa = self._outlierArgs(params, among, kw)
        n = self.lastCount()
        mean = np.zeros(max(n, 1), np.float32)
        count = np.zeros(max(n, 1), np.uint32)
        _chk(lib().ef_map_neighbor_stats(self.h, C.byref(params), pa, _ptr(mean), _ptr(count), n), self.h)
        return mean[:n], count[:n]

    def outlierSelect(self, params: ef_outlier_params | None = None, among=None, max_rows: int | None = None, count: bool = False,
                      result: bool = False, **kw):
        """the rows removeOutliers with these parameters would remove, in ascending order (uint32), at most max_rows of them (None: all); the
        map does not change.  among and the keywords as neighborStats takes them.  count=True adds the total, result=True the dict of
        ef_outlier_result: rows[, total][, result]"""
        params, among, pa = self._outlierArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        res = ef_outlier_result()
        _chk(lib().ef_map_outliers_select(self.h, C.byref(params), pa, _ptr(rows) if cap else None, cap, C.byref(total),
                                          C.byref(res) if result else None), self.h)
        out = (rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((self._outlierResult(res),) if result else ())
        return out if len(out) > 1 else out[0]

    def outlierSelectDevice(self, params: ef_outlier_params, among, rows_dev, max_rows: int, count_dev, result_dev=None):
        """ef_map_outliers_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0 and for the result), enqueued on
        the context's stream"""
        params, among, pa = self._outlierArgs(params, among, {})
        _chk(lib().ef_map_outliers_select_dev(self.h, C.byref(params), pa, _dev(rows_dev), int(max_rows), _dev(count_dev), _dev(result_dev)), self.h)

    def neighborStatsDevice(self, params: ef_outlier_params, among, mean_dev, count_dev, max_rows: int):
        """ef_map_neighbor_stats_dev: raw device pointers (int, c_void_p or None) for max_rows floats and max_rows uint32"""
        params, among, pa = self._outlierArgs(params, among, {})
        _chk(lib().ef_map_neighbor_stats_dev(self.h, C.byref(params), pa, _dev(mean_dev), _dev(count_dev), int(max_rows)), self.h)

    def removeOutliers(self, params: ef_outlier_params | None = None, among=None, **kw) -> dict:
        """removes the outlier surfels (ef_map_remove_outliers: what eraseRows(outlierSelect(...)) leaves); not idempotent: what is left has
        another mean and deviation.  The dict of ef_outlier_result: {"sum", "sum_sq", "participants", "measured", "sparse", "outliers",
        "count_after", "threshold"}"""
        params, among, pa = self._outlierArgs(params, among, kw)
        res = ef_outlier_result()
        _chk(lib().ef_map_remove_outliers(self.h, C.byref(params), pa, C.byref(res)), self.h)
        return self._outlierResult(res)

    # --- connected components of the map under "closer than r" (ef_map_components / ef_map_components_select / ef_map_remove_components) ---
    def componentParams(self, **kw) -> ef_component_params:
        """ef_default_component_params (radius 0.03, cell 0.03, min_conf -1, min_size 50, max_size 0) with fields replaced by keyword"""
        return self._params(ef_component_params, lib().ef_default_component_params, kw, "component")

    def _componentArgs(self, params, among, kw):
        if params is None:
            params = self.componentParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    @staticmethod
    def _componentResult(res: ef_component_result) -> dict:
        return {k: int(getattr(res, k)) for k, _ in ef_component_result._fields_}

    def components(self, params: ef_component_params | None = None, among=None, result: bool = False, **kw):
        """(label uint32, size uint32) per row of downloadMap(): the smallest row of the surfel's connected component under "closer than
        radius" and the component's number of nodes; COMPONENT_NONE and 0 for a row that is no node; the map does not change.  among: an
        ef_map_selection, a dict of mapSelection keywords or None (every surfel participates); other keywords are ef_component_params
        fields.  result=True adds the dict of ef_component_result"""
        params, among, pa = self._componentArgs(params, among, kw)
        n = self.lastCount()
        label = np.zeros(max(n, 1), np.uint32)
        size = np.zeros(max(n, 1), np.uint32)
        res = ef_component_result()
        _chk(lib().ef_map_components(self.h, C.byref(params), pa, _ptr(label), _ptr(size), n, C.byref(res)), self.h)
        return (label[:n], size[:n]) + ((self._componentResult(res),) if result else ())

    def componentSelect(self, params: ef_component_params | None = None, among=None, what: int = COMPONENTS_REJECTED, max_rows: int | None = None,
                        count: bool = False, result: bool = False, **kw):
        """the nodes of the rejected components (what = COMPONENTS_REJECTED: fewer than min_size or, with max_size != 0, more than max_size
        nodes; the rows removeComponents with these parameters would remove) or of the accepted ones (COMPONENTS_ACCEPTED), in ascending order
        (uint32), at most max_rows of them (None: all); the map does not change.  among and the keywords as components takes them.
        count=True adds the total, result=True the dict of ef_component_result: rows[, total][, result]"""
        params, among, pa = self._componentArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        res = ef_component_result()
        _chk(lib().ef_map_components_select(self.h, C.byref(params), pa, int(what), _ptr(rows) if cap else None, cap, C.byref(total),
                                            C.byref(res) if result else None), self.h)
        out = (rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((self._componentResult(res),) if result else ())
        return out if len(out) > 1 else out[0]

    def componentSelectDevice(self, params: ef_component_params, among, what: int, rows_dev, max_rows: int, count_dev, result_dev=None):
        """ef_map_components_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0 and for the result), enqueued on
        the context's stream"""
        params, among, pa = self._componentArgs(params, among, {})
        _chk(lib().ef_map_components_select_dev(self.h, C.byref(params), pa, int(what), _dev(rows_dev), int(max_rows), _dev(count_dev),
                                                _dev(result_dev)), self.h)

    def componentsDevice(self, params: ef_component_params, among, label_dev, size_dev, max_rows: int, result_dev=None):
        """ef_map_components_dev: raw device pointers (int, c_void_p or None) for max_rows uint32 each and for the result"""
        params, among, pa = self._componentArgs(params, among, {})
        _chk(lib().ef_map_components_dev(self.h, C.byref(params), pa, _dev(label_dev), _dev(size_dev), int(max_rows), _dev(result_dev)), self.h)

    def removeComponents(self, params: ef_component_params | None = None, among=None, **kw) -> dict:
        """removes the nodes of the rejected components (ef_map_remove_components: what eraseRows(componentSelect(...)) leaves); idempotent: a
        second call with the same arguments removes nothing.  The dict of ef_component_result: {"nodes", "components", "largest",
        "rejected_rows", "rejected_components", "count_after", "status"}"""
        params, among, pa = self._componentArgs(params, among, kw)
        res = ef_component_result()
        _chk(lib().ef_map_remove_components(self.h, C.byref(params), pa, C.byref(res)), self.h)
        return self._componentResult(res)

    # --- planes of the map by sequential RANSAC (ef_map_planes / ef_map_planes_select / ef_map_remove_planes) ---
    def planeParams(self, **kw) -> ef_plane_params:
        """ef_default_plane_params (distance 0.01, normal_cos 0, min_conf -1, hypotheses 1024, seed 0, max_planes 4, min_inliers 500, refine 1,
        axis_mode PLANE_AXIS_OFF, axis (0, 0, 1), axis_bound 0.95) with fields replaced by keyword; axis: three floats"""
        if "axis" in kw:
            kw = dict(kw, axis=(c_f * 3)(*[float(v) for v in kw["axis"]]))
        return self._params(ef_plane_params, lib().ef_default_plane_params, kw, "plane")

    def _planeArgs(self, params, among, kw):
        if params is None:
            params = self.planeParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    @staticmethod
    def _planeResult(res: ef_plane_result) -> dict:
        return {k: int(getattr(res, k)) for k, _ in ef_plane_result._fields_}

    @staticmethod
    def _planeModels(models, planes: int) -> list:
        """the first `planes` entries of an ef_plane_model array as dicts: normal (float32 [3]), d and thickness (numpy float32), the integers"""
        out = []
        for m in models[:planes]:
            d = {k: int(getattr(m, k)) for k in ("inliers", "sampled_inliers", "hypothesis", "valid_hypotheses", "participants")}
            d.update(normal=np.array(list(m.normal), np.float32), d=np.float32(m.d), thickness=np.float32(m.thickness))
            out.append(d)
        return out

    def planes(self, params: ef_plane_params | None = None, among=None, result: bool = False, **kw):
        """(plane uint32 per row of downloadMap(), list of model dicts[, result]): the index of the plane the surfel lies on, PLANE_NONE for
        a surfel on none, and per found plane {"normal", "d", "inliers", "sampled_inliers", "hypothesis", "valid_hypotheses", "participants",
        "thickness"}; the map does not change.  among: an ef_map_selection, a dict of mapSelection keywords or None (every surfel
        participates); other keywords are ef_plane_params fields.  result=True adds the dict of ef_plane_result"""
        params, among, pa = self._planeArgs(params, among, kw)
        n = self.lastCount()
        plane = np.zeros(max(n, 1), np.uint32)
        models = (ef_plane_model * PLANE_MAX_PLANES)()
        res = ef_plane_result()
        _chk(lib().ef_map_planes(self.h, C.byref(params), pa, _ptr(plane), n, models, C.byref(res)), self.h)
        return (plane[:n], self._planeModels(models, res.planes)) + ((self._planeResult(res),) if result else ())

    def planeSelect(self, params: ef_plane_params | None = None, among=None, what: int = PLANES_ON, which: int = -1, max_rows: int | None = None,
                    count: bool = False, models: bool = False, result: bool = False, **kw):
        """the rows on plane `which` (what = PLANES_ON; which = -1: on any found plane; the rows removePlanes with these arguments would
        remove) or every other participant (PLANES_OFF), in ascending order (uint32), at most max_rows of them (None: all); the map does not
        change.  among and the keywords as planes takes them.  count=True adds the total, models=True the list of model dicts, result=True
        the dict of ef_plane_result: rows[, total][, models][, result]"""
        params, among, pa = self._planeArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        mods = (ef_plane_model * PLANE_MAX_PLANES)()
        res = ef_plane_result()
        _chk(lib().ef_map_planes_select(self.h, C.byref(params), pa, int(what), int(which), _ptr(rows) if cap else None, cap, C.byref(total), mods,
                                        C.byref(res)), self.h)
        out = ((rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((self._planeModels(mods, res.planes),) if models else ())
               + ((self._planeResult(res),) if result else ()))
        return out if len(out) > 1 else out[0]

    def planeSelectDevice(self, params: ef_plane_params, among, what: int, which: int, rows_dev, max_rows: int, count_dev, models_dev=None,
                          result_dev=None):
        """ef_map_planes_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0, for the models and for the result),
        enqueued on the context's stream"""
        params, among, pa = self._planeArgs(params, among, {})
        _chk(lib().ef_map_planes_select_dev(self.h, C.byref(params), pa, int(what), int(which), _dev(rows_dev), int(max_rows), _dev(count_dev),
                                            _dev(models_dev), _dev(result_dev)), self.h)

    def planesDevice(self, params: ef_plane_params, among, plane_dev, max_rows: int, models_dev=None, result_dev=None):
        """ef_map_planes_dev: raw device pointers (int, c_void_p or None) for max_rows uint32, params.max_planes models and the result"""
        params, among, pa = self._planeArgs(params, among, {})
        _chk(lib().ef_map_planes_dev(self.h, C.byref(params), pa, _dev(plane_dev), int(max_rows), _dev(models_dev), _dev(result_dev)), self.h)

    def removePlanes(self, params: ef_plane_params | None = None, among=None, which: int = -1, models: bool = False, **kw):
        """removes the rows on plane `which` (-1: on any found plane) (ef_map_remove_planes: what eraseRows(planeSelect(...)) leaves).  The
        dict of ef_plane_result: {"nodes", "planes", "on_rows", "off_rows", "count_after"}; models=True: (result, list of model dicts)"""
        params, among, pa = self._planeArgs(params, among, kw)
        mods = (ef_plane_model * PLANE_MAX_PLANES)()
        res = ef_plane_result()
        _chk(lib().ef_map_remove_planes(self.h, C.byref(params), pa, int(which), mods, C.byref(res)), self.h)
        return (self._planeResult(res), self._planeModels(mods, res.planes)) if models else self._planeResult(res)

    # --- estimate normals, curvature and spacing from the map's neighbourhoods (ef_map_normals / ef_map_normals_select / ef_map_reestimate_normals) ---
    def normalParams(self, **kw) -> ef_normal_params:
        """ef_default_normal_params (radius 0.03, cell 0.03, min_conf -1, k 12, min_neighbors 5, NORMALS_KEEP_SIDE, side -1, viewpoint (0, 0, 0),
        line_ratio 1e-4, max_curvature 0.05, set_radius 0, radius_scale 1) with fields replaced by keyword; viewpoint: three floats"""
        if "viewpoint" in kw:
            kw = dict(kw, viewpoint=(c_f * 3)(*[float(v) for v in kw["viewpoint"]]))
        return self._params(ef_normal_params, lib().ef_default_normal_params, kw, "normal")

    def _normalArgs(self, params, among, kw):
        if params is None:
            params = self.normalParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    @staticmethod
    def _normalResult(res: ef_normal_result) -> dict:
        return {k: int(getattr(res, k)) for k, _ in ef_normal_result._fields_}

    def estimateNormals(self, params: ef_normal_params | None = None, among=None, **kw) -> dict:
        """per row of downloadMap(): {"normals" float32 [n, 3], "curvature" float32, "spacing" float32, "count" uint32, "status" uint8
        (api.NORMAL_*)}: the PCA normal of the k nearest other surfels within radius, oriented by params.orientation, the surface variation,
        the mean distance to the used neighbours and the number of ALL neighbours; the map does not change.  among: an ef_map_selection, a dict
        of mapSelection keywords or None (every surfel participates); other keywords are ef_normal_params fields"""
        params, among, pa = self._normalArgs(params, among, kw)
        n = self.lastCount()
        m = max(n, 1)
        out = dict(normals=np.zeros((m, 3), np.float32), curvature=np.zeros(m, np.float32), spacing=np.zeros(m, np.float32),
                   count=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
        _chk(lib().ef_map_normals(self.h, C.byref(params), pa, _ptr(out["normals"]), _ptr(out["curvature"]), _ptr(out["spacing"]),
                                  _ptr(out["count"]), _ptr(out["status"]), n), self.h)
        return {k: v[:n] for k, v in out.items()}

    def estimateNormalsDevice(self, params: ef_normal_params, among, normals_dev, curvature_dev, spacing_dev, count_dev, status_dev, max_rows: int):
        """ef_map_normals_dev: raw device pointers (int, c_void_p or None) for max_rows x 3 floats, max_rows floats twice, max_rows uint32 and
        max_rows bytes, enqueued on the context's stream"""
        params, among, pa = self._normalArgs(params, among, {})
        _chk(lib().ef_map_normals_dev(self.h, C.byref(params), pa, _dev(normals_dev), _dev(curvature_dev), _dev(spacing_dev), _dev(count_dev),
                                      _dev(status_dev), int(max_rows)), self.h)

    def normalSelect(self, params: ef_normal_params | None = None, among=None, what: int = NORMAL_ESTIMATED, max_rows: int | None = None,
                     count: bool = False, result: bool = False, **kw):
        """the rows `what` names (NORMAL_ESTIMATED / _SPARSE / _DEGENERATE, NORMALS_CURVED: estimated and curvature > max_curvature,
        NORMALS_FLAT: estimated and not curved) in ascending order (uint32), at most max_rows of them (None: all); the map does not change.
        among and the keywords as estimateNormals takes them.  count=True adds the total, result=True the dict of ef_normal_result:
        rows[, total][, result]"""
        params, among, pa = self._normalArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        res = ef_normal_result()
        _chk(lib().ef_map_normals_select(self.h, C.byref(params), pa, int(what), _ptr(rows) if cap else None, cap, C.byref(total),
                                         C.byref(res) if result else None), self.h)
        out = (rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((self._normalResult(res),) if result else ())
        return out if len(out) > 1 else out[0]

    def normalSelectDevice(self, params: ef_normal_params, among, what: int, rows_dev, max_rows: int, count_dev, result_dev=None):
        """ef_map_normals_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0 and for the result), enqueued on the
        context's stream"""
        params, among, pa = self._normalArgs(params, among, {})
        _chk(lib().ef_map_normals_select_dev(self.h, C.byref(params), pa, int(what), _dev(rows_dev), int(max_rows), _dev(count_dev),
                                             _dev(result_dev)), self.h)

    def reestimateNormals(self, params: ef_normal_params | None = None, among=None, **kw) -> dict:
        """writes the estimate into the normal of every ESTIMATED row and, with set_radius, radius_scale * spacing into its radius
        (ef_map_reestimate_normals); every other word of the map keeps its bits.  The dict of ef_normal_result: {"participants", "estimated",
        "sparse", "degenerate", "flipped", "listed"}"""
        params, among, pa = self._normalArgs(params, among, kw)
        res = ef_normal_result()
        _chk(lib().ef_map_reestimate_normals(self.h, C.byref(params), pa, C.byref(res)), self.h)
        return self._normalResult(res)

    # --- smooth regions of the map (ef_map_regions / ef_map_regions_select / ef_map_remove_regions) ---
    def regionParams(self, **kw) -> ef_region_params:
        """ef_default_region_params (radius 0.03, cell 0.03, min_conf -1, k 12, min_neighbors 5, line_ratio 1e-4, REGIONS_ESTIMATED, two_sided 0,
        min_normal_cos cos 15 deg, max_curvature 0.05, attach_borders 1, min_size 50, max_size 0) with fields replaced by keyword"""
        return self._params(ef_region_params, lib().ef_default_region_params, kw, "region")

    def _regionArgs(self, params, among, kw):
        if params is None:
            params = self.regionParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    @staticmethod
    def _regionResult(res: ef_region_result) -> dict:
        return {k: int(getattr(res, k)) for k, _ in ef_region_result._fields_}

    def regions(self, params: ef_region_params | None = None, among=None, result: bool = False, **kw):
        """(label uint32, size uint32, kind uint8) per row of downloadMap(): the smallest core row of the surfel's smooth region (the connected
        components of the low-curvature surfels under "within radius and normals within min_normal_cos", crease surfels attached to the region
        of their nearest smooth core), the region's number of rows, and REGION_KIND_*; REGION_NONE and 0 for a row without a region; the map
        does not change.  among: an ef_map_selection, a dict of mapSelection keywords or None (every surfel participates); other keywords are
        ef_region_params fields.  result=True adds the dict of ef_region_result"""
        params, among, pa = self._regionArgs(params, among, kw)
        n = self.lastCount()
        label = np.zeros(max(n, 1), np.uint32)
        size = np.zeros(max(n, 1), np.uint32)
        kind = np.zeros(max(n, 1), np.uint8)
        res = ef_region_result()
        _chk(lib().ef_map_regions(self.h, C.byref(params), pa, _ptr(label), _ptr(size), _ptr(kind), n, C.byref(res)), self.h)
        return (label[:n], size[:n], kind[:n]) + ((self._regionResult(res),) if result else ())

    def regionSelect(self, params: ef_region_params | None = None, among=None, what: int = REGIONS_REJECTED, max_rows: int | None = None,
                     count: bool = False, result: bool = False, **kw):
        """the rows of one list in ascending order (uint32), at most max_rows of them (None: all): the nodes of the rejected regions (what =
        REGIONS_REJECTED: fewer than min_size or, with max_size != 0, more than max_size rows) or of the accepted ones (REGIONS_ACCEPTED), the
        borders without a region (REGIONS_UNASSIGNED) or every border, the crease lines (REGIONS_BORDERS); the map does not change.  among
        and the keywords as regions takes them.  count=True adds the total, result=True the dict of ef_region_result: rows[, total][, result]"""
        params, among, pa = self._regionArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        res = ef_region_result()
        _chk(lib().ef_map_regions_select(self.h, C.byref(params), pa, int(what), _ptr(rows) if cap else None, cap, C.byref(total),
                                         C.byref(res) if result else None), self.h)
        out = (rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((self._regionResult(res),) if result else ())
        return out if len(out) > 1 else out[0]

    def regionSelectDevice(self, params: ef_region_params, among, what: int, rows_dev, max_rows: int, count_dev, result_dev=None):
        """ef_map_regions_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0 and for the result), enqueued on the
        context's stream"""
        params, among, pa = self._regionArgs(params, among, {})
        _chk(lib().ef_map_regions_select_dev(self.h, C.byref(params), pa, int(what), _dev(rows_dev), int(max_rows), _dev(count_dev),
                                             _dev(result_dev)), self.h)

    def regionsDevice(self, params: ef_region_params, among, label_dev, size_dev, kind_dev, max_rows: int, result_dev=None):
        """ef_map_regions_dev: raw device pointers (int, c_void_p or None) for max_rows uint32 twice, max_rows bytes and the result"""
        params, among, pa = self._regionArgs(params, among, {})
        _chk(lib().ef_map_regions_dev(self.h, C.byref(params), pa, _dev(label_dev), _dev(size_dev), _dev(kind_dev), int(max_rows),
                                      _dev(result_dev)), self.h)

    def removeRegions(self, params: ef_region_params | None = None, among=None, what: int = REGIONS_REJECTED, **kw) -> dict:
        """removes the rows of the list `what` (ef_map_remove_regions: what eraseRows(regionSelect(..., what=what)) leaves); not idempotent:
        the rows that stay have other neighbours, and with them other normals and curvatures.  The dict of ef_region_result for the map as it
        was, with listed = the rows removed and count_after = the count left"""
        params, among, pa = self._regionArgs(params, among, kw)
        res = ef_region_result()
        _chk(lib().ef_map_remove_regions(self.h, C.byref(params), pa, int(what), C.byref(res)), self.h)
        return self._regionResult(res)

    # --- smooth the map's positions by moving least squares (ef_map_smooth / ef_map_smooth_select / ef_map_smooth_apply) ---
    def smoothParams(self, **kw) -> ef_smooth_params:
        """ef_default_smooth_params (radius 0.03, cell 0.03, min_conf -1, k 12, min_neighbors 5, iterations 1, SMOOTH_COMPACT, normal_gate 0,
        min_normal_cos 0.9, strength 1, max_shift = radius, line_ratio 1e-4, set_normal 0, shift_threshold 0) with fields replaced by keyword;
        max_shift follows a radius given by keyword unless it is given too"""
        if "radius" in kw and "max_shift" not in kw:
            kw = dict(kw, max_shift=kw["radius"])
        return self._params(ef_smooth_params, lib().ef_default_smooth_params, kw, "smooth")

    def _smoothArgs(self, params, among, kw):
        if params is None:
            params = self.smoothParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    @staticmethod
    def _smoothResult(res: ef_smooth_result) -> dict:
        return {k: (float(getattr(res, k)) if k == "largest_shift" else int(getattr(res, k))) for k, _ in ef_smooth_result._fields_}

    def smoothMap(self, params: ef_smooth_params | None = None, among=None, result: bool = False, **kw):
        """per row of downloadMap(): {"position" float32 [n, 3], "normal" float32 [n, 3], "curvature" float32, "shift" float32, "count" uint32,
        "status" uint8 (api.SMOOTH_*)}: the position after `iterations` projections onto the weighted least-squares plane of the k nearest
        other surfels within radius (the neighbourhoods are those of the map as it stands), the last fit's normal and surface variation, the
        distance moved and the number of ALL neighbours; the map does not change.  among: an ef_map_selection, a dict of mapSelection keywords
        or None (every surfel participates); other keywords are ef_smooth_params fields.  result=True adds the dict of ef_smooth_result"""
        params, among, pa = self._smoothArgs(params, among, kw)
        n = self.lastCount()
        m = max(n, 1)
        out = dict(position=np.zeros((m, 3), np.float32), normal=np.zeros((m, 3), np.float32), curvature=np.zeros(m, np.float32),
                   shift=np.zeros(m, np.float32), count=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
        res = ef_smooth_result()
        _chk(lib().ef_map_smooth(self.h, C.byref(params), pa, _ptr(out["position"]), _ptr(out["normal"]), _ptr(out["curvature"]),
                                 _ptr(out["shift"]), _ptr(out["count"]), _ptr(out["status"]), n, C.byref(res)), self.h)
        out = {k: v[:n] for k, v in out.items()}
        return (out, self._smoothResult(res)) if result else out

    def smoothMapDevice(self, params: ef_smooth_params, among, position_dev, normal_dev, curvature_dev, shift_dev, count_dev, status_dev,
                        max_rows: int, result_dev=None):
        """ef_map_smooth_dev: raw device pointers (int, c_void_p or None) for max_rows x 3 floats twice, max_rows floats twice, max_rows uint32,
        max_rows bytes and the result, enqueued on the context's stream"""
        params, among, pa = self._smoothArgs(params, among, {})
        _chk(lib().ef_map_smooth_dev(self.h, C.byref(params), pa, _dev(position_dev), _dev(normal_dev), _dev(curvature_dev), _dev(shift_dev),
                                     _dev(count_dev), _dev(status_dev), int(max_rows), _dev(result_dev)), self.h)

    def smoothSelect(self, params: ef_smooth_params | None = None, among=None, what: int = SMOOTH_SHIFTED, max_rows: int | None = None,
                     count: bool = False, result: bool = False, **kw):
        """the rows `what` names (SMOOTH_SMOOTHED / _SPARSE / _DEGENERATE, SMOOTH_CLAMPED: a step was cut at max_shift, SMOOTH_SHIFTED: moved
        further than shift_threshold) in ascending order (uint32), at most max_rows of them (None: all); the map does not change.  among and
        the keywords as smoothMap takes them.  count=True adds the total, result=True the dict of ef_smooth_result: rows[, total][, result]"""
        params, among, pa = self._smoothArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        res = ef_smooth_result()
        _chk(lib().ef_map_smooth_select(self.h, C.byref(params), pa, int(what), _ptr(rows) if cap else None, cap, C.byref(total),
                                        C.byref(res) if result else None), self.h)
        out = (rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((self._smoothResult(res),) if result else ())
        return out if len(out) > 1 else out[0]

    def smoothSelectDevice(self, params: ef_smooth_params, among, what: int, rows_dev, max_rows: int, count_dev, result_dev=None):
        """ef_map_smooth_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0 and for the result), enqueued on the
        context's stream"""
        params, among, pa = self._smoothArgs(params, among, {})
        _chk(lib().ef_map_smooth_select_dev(self.h, C.byref(params), pa, int(what), _dev(rows_dev), int(max_rows), _dev(count_dev),
                                            _dev(result_dev)), self.h)

    def applySmooth(self, params: ef_smooth_params | None = None, among=None, **kw) -> dict:
        """writes the smoothed position of every participant into the map and, with set_normal, the last fit's normal into the SMOOTHED rows
        (ef_map_smooth_apply); every other word of the map keeps its bits.  Not idempotent.  The dict of ef_smooth_result: {"participants",
        "smoothed", "sparse", "degenerate", "clamped", "moved", "listed", "largest_shift"}"""
        params, among, pa = self._smoothArgs(params, among, kw)
        res = ef_smooth_result()
        _chk(lib().ef_map_smooth_apply(self.h, C.byref(params), pa, C.byref(res)), self.h)
        return self._smoothResult(res)

    # --- the map's open boundaries and holes (ef_map_boundaries / ef_map_boundaries_select) ---
    def boundaryParams(self, **kw) -> ef_boundary_params:
        """ef_default_boundary_params (radius 0.03, cell 0.03, min_conf -1, k 12, min_neighbors 5, BOUNDARY_STORED, line_ratio 1e-4, max_gap 1 = a
        right angle in TURN units (boundary_gap / boundary_angle convert), min_size 1, max_size 0) with fields replaced by keyword"""
        return self._params(ef_boundary_params, lib().ef_default_boundary_params, kw, "boundary")

    def _boundaryArgs(self, params, among, kw):
        if params is None:
            params = self.boundaryParams(**kw)
        else:
            assert not kw, "give params or keywords, not both"
        if isinstance(among, dict):
            among = self.mapSelection(**among)
        return params, among, (C.byref(among) if among is not None else None)

    @staticmethod
    def _boundaryResult(res: ef_boundary_result) -> dict:
        return {k: int(getattr(res, k)) for k, _ in ef_boundary_result._fields_}

    def boundaries(self, params: ef_boundary_params | None = None, among=None, result: bool = False, **kw):
        """per row of downloadMap(): {"gap" float32 (the widest angular gap the neighbours leave seen along the normal, in TURN units: 1 = a right
        angle), "count" uint32, "status" uint8 (api.BOUNDARY_*), "label" uint32, "size" uint32 (the boundary loop of a BOUNDARY row: its smallest
        row and its number of rows; COMPONENT_NONE and 0 for every other row)}; the map does not change.  among: an ef_map_selection, a dict of
        mapSelection keywords or None (every surfel participates); other keywords are ef_boundary_params fields.  result=True adds the dict of
        ef_boundary_result"""
        params, among, pa = self._boundaryArgs(params, among, kw)
        n = self.lastCount()
        m = max(n, 1)
        out = dict(gap=np.zeros(m, np.float32), count=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8), label=np.zeros(m, np.uint32),
                   size=np.zeros(m, np.uint32))
        res = ef_boundary_result()
        _chk(lib().ef_map_boundaries(self.h, C.byref(params), pa, _ptr(out["gap"]), _ptr(out["count"]), _ptr(out["status"]), _ptr(out["label"]),
                                     _ptr(out["size"]), n, C.byref(res)), self.h)
        out = {k: v[:n] for k, v in out.items()}
        return (out, self._boundaryResult(res)) if result else out

    def boundariesDevice(self, params: ef_boundary_params, among, gap_dev, count_dev, status_dev, label_dev, size_dev, max_rows: int,
                         result_dev=None):
        """ef_map_boundaries_dev: raw device pointers (int, c_void_p or None) for max_rows floats, max_rows uint32, max_rows bytes, max_rows
        uint32 twice and the result, enqueued on the context's stream"""
        params, among, pa = self._boundaryArgs(params, among, {})
        _chk(lib().ef_map_boundaries_dev(self.h, C.byref(params), pa, _dev(gap_dev), _dev(count_dev), _dev(status_dev), _dev(label_dev),
                                         _dev(size_dev), int(max_rows), _dev(result_dev)), self.h)

    def boundarySelect(self, params: ef_boundary_params | None = None, among=None, what: int = BOUNDARY_BOUNDARY, max_rows: int | None = None,
                       count: bool = False, result: bool = False, **kw):
        """the rows `what` names (BOUNDARY_INTERIOR / _BOUNDARY / _SPARSE / _DEGENERATE: the rows of that status; BOUNDARY_LOOPS_ACCEPTED /
        _REJECTED: the rows of the boundary loops within / outside min_size .. max_size) in ascending order (uint32), at most max_rows of them
        (None: all); the map does not change.  among and the keywords as boundaries takes them.  count=True adds the total, result=True the
        dict of ef_boundary_result: rows[, total][, result]"""
        params, among, pa = self._boundaryArgs(params, among, kw)
        cap = self.lastCount() if max_rows is None else int(max_rows)
        rows = np.zeros(max(cap, 1), np.uint32)
        total = c_u32(0)
        res = ef_boundary_result()
        _chk(lib().ef_map_boundaries_select(self.h, C.byref(params), pa, int(what), _ptr(rows) if cap else None, cap, C.byref(total),
                                            C.byref(res) if result else None), self.h)
        out = (rows[:min(cap, total.value)].copy(),) + ((total.value,) if count else ()) + ((self._boundaryResult(res),) if result else ())
        return out if len(out) > 1 else out[0]

    def boundarySelectDevice(self, params: ef_boundary_params, among, what: int, rows_dev, max_rows: int, count_dev, result_dev=None):
        """ef_map_boundaries_select_dev: raw device pointers (int, c_void_p or None for rows with max_rows 0 and for the result), enqueued on
        the context's stream"""
        params, among, pa = self._boundaryArgs(params, among, {})
        _chk(lib().ef_map_boundaries_select_dev(self.h, C.byref(params), pa, int(what), _dev(rows_dev), int(max_rows), _dev(count_dev),
                                                _dev(result_dev)), self.h)

    def setReferenceDownload(self, on=True):
        """downloadMap / savePly read what GlobalModel::downloadMap reads (the pre-clean buffer, quirk Q14) instead of model()"""
        _chk(lib().ef_set_reference_download(self.h, int(on)), self.h)

    def uploadMap(self, surfels: np.ndarray):
        s = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
        _chk(lib().ef_map_upload(self.h, _ptr(s), len(s)), self.h)

    def getPoseQT(self) -> np.ndarray:
        """T_wc as the engine holds it: unit quaternion x y z w + translation (7 doubles), no matrix round trip (ef_get_pose_qt)"""
        qt = np.zeros(7, np.float64)
        _chk(lib().ef_get_pose_qt(self.h, _ptr(qt)), self.h)
        return qt

    def checkpoint(self, last_rgb, last_depth) -> dict:
        """what a replay carries from one processFrame to the next: map, tick, pose and the frame processed last"""
        return dict(map=self.downloadMap(), tick=self.getTick(), qt=self.getPoseQT(), rgb=np.ascontiguousarray(last_rgb, np.uint8).copy(),
                    depth=np.ascontiguousarray(last_depth, np.uint16).copy())

    def restore(self, ck: dict):
        """resume from ``checkpoint()`` in a fresh context (ef_map_upload + ef_restore_state): the next processFrame continues the replay"""
        self.uploadMap(ck["map"])
        qt = np.ascontiguousarray(ck["qt"], np.float64).reshape(7)
        _chk(lib().ef_restore_state(self.h, int(ck["tick"]), _ptr(qt), _ptr(ck["rgb"]), _ptr(ck["depth"])), self.h)

    def savePly(self, path: str):
        _chk(lib().ef_save_ply(self.h, path.encode()), self.h)

    def saveFreiburg(self, path: str):
        _chk(lib().ef_save_freiburg(self.h, path.encode()), self.h)

    def setRgbOnly(self, v): _chk(lib().ef_set_rgb_only(self.h, int(v)), self.h)
    def setIcpWeight(self, v): _chk(lib().ef_set_icp_weight(self.h, v), self.h)
    def setPyramid(self, v): _chk(lib().ef_set_pyramid(self.h, int(v)), self.h)
    def setFastOdom(self, v): _chk(lib().ef_set_fast_odom(self.h, int(v)), self.h)
    def setSo3(self, v): _chk(lib().ef_set_so3(self.h, int(v)), self.h)
    def setFrameToFrameRGB(self, v): _chk(lib().ef_set_frame_to_frame_rgb(self.h, int(v)), self.h)
    def setConfidenceThreshold(self, v): _chk(lib().ef_set_confidence_threshold(self.h, v), self.h)
    def setDepthCutoff(self, v): _chk(lib().ef_set_depth_cutoff(self.h, v), self.h)
    def setInputOverlap(self, on): _chk(lib().ef_set_input_overlap(self.h, int(on)), self.h)
    def setInputCuMask(self, one_in_n): _chk(lib().ef_set_input_cu_mask(self.h, int(one_in_n)), self.h)
    def setDeformation(self, graph, isFern=False):
        g = np.ascontiguousarray(graph, np.float32).reshape(-1, 16)
        _chk(lib().ef_set_deformation(self.h, _ptr(g), len(g), int(isFern)), self.h)

    def setGraphReplay(self, on): _chk(lib().ef_set_graph_replay(self.h, int(on)), self.h)

    def image(self, name: str) -> np.ndarray:
        which, dt, ch = self.IMAGES[name]
        W, H = self.cfg.width, self.cfg.height
        out = np.zeros((H, W, ch) if ch > 1 else (H, W), dt)
        _chk(lib().ef_get_image(self.h, which, _ptr(out), out.nbytes), self.h)
        return out

    def trackerBuffer(self, name: str, level: int = 0, tracker: int = 0) -> np.ndarray:
        """tracker: 0 = frameToModel, 1 = modelToModel (closeLoops contexts only)"""
        which, dt, planes = self.TRACKER[name]
        w, h = self.cfg.width >> level, self.cfg.height >> level
        out = np.zeros((h * planes, w), dt)
        _chk(lib().ef_get_tracker_buffer_of(self.h, tracker, which, level, _ptr(out), out.nbytes), self.h)
        return out

    def enableTiming(self, on=True):
        _chk(lib().ef_enable_timing(self.h, int(on)), self.h)

    def timings(self) -> dict:
        arr = (ef_timing * 32)()
        n = c_i(0)
        _chk(lib().ef_get_timings(self.h, arr, 32, C.byref(n)), self.h)
        return {arr[i].name.decode(): arr[i].ms for i in range(n.value)}


# ------------------------------------------------------------------------------------------------
# operator tier on numpy arrays (upload -> HIP kernel via the C ABI -> download)
# ------------------------------------------------------------------------------------------------
class ops:
    @staticmethod
    def _f32(a):
        return np.ascontiguousarray(a, np.float32)

    @staticmethod
    def _image_op(name, src, dtype, scale, *scalars):
        """the single-image operators: src (H x W [x C]) uploaded, ef_op_<name>(src, W, H, *scalars, dst, stream 0) run, dst (H / scale x
        W / scale of dtype) downloaded"""
        h, w = src.shape[:2]
        shape = (h // scale, w // scale)
        s, d = DevBuf.from_array(src), DevBuf(shape[0] * shape[1] * np.dtype(dtype).itemsize)
        _chk(getattr(lib(), "ef_op_" + name)(s.p, w, h, *scalars, d.p, None))
        return d.to_array(dtype, shape)

    @staticmethod
    def pyr_down(src):
        return ops._image_op("pyr_down", src, np.uint16, 2)

    @staticmethod
    def create_vmap(depth, fx, fy, cx, cy, cutoff, init=None):
        h, w = depth.shape
        d = DevBuf.from_array(depth)
        v = DevBuf.from_array(np.zeros((3 * h, w), np.float32) if init is None else init)
        k = ef_intr(fx, fy, cx, cy)
        _chk(lib().ef_op_create_vmap(C.byref(k), d.p, w, h, cutoff, v.p, None))
        return v.to_array(np.float32, (3 * h, w))

    @staticmethod
    def create_nmap(vmap, init=None):
        h3, w = vmap.shape
        v = DevBuf.from_array(vmap)
        n = DevBuf.from_array(np.zeros((h3, w), np.float32) if init is None else init)
        _chk(lib().ef_op_create_nmap(v.p, w, h3 // 3, n.p, None))
        return n.to_array(np.float32, (h3, w))

    @staticmethod
    def transform_maps(vmap, nmap, R, t):
        h3, w = vmap.shape
        v, n = DevBuf.from_array(vmap), DevBuf.from_array(nmap)
        R9, t3 = ops._f32(R).reshape(9), ops._f32(t).reshape(3)
        _chk(lib().ef_op_transform_maps(v.p, n.p, w, h3 // 3, _ptr(R9), _ptr(t3), v.p, n.p, None))
        return v.to_array(np.float32, (h3, w)), n.to_array(np.float32, (h3, w))

    @staticmethod
    def copy_maps(vtex, ntex):
        h, w, _ = vtex.shape
        v4, n4 = DevBuf.from_array(ops._f32(vtex)), DevBuf.from_array(ops._f32(ntex))
        tmp, vm, nm = DevBuf(h * w * 16), DevBuf(h * w * 12), DevBuf(h * w * 12)
        _chk(lib().ef_op_copy_maps(v4.p, n4.p, w, h, tmp.p, vm.p, nm.p, None))
        return tmp.to_array(np.float32, (h, w, 4)), vm.to_array(np.float32, (3 * h, w)), nm.to_array(np.float32, (3 * h, w))

    @staticmethod
    def resize_map(src, normalize, init=None):
        h3, w = src.shape
        s = DevBuf.from_array(src)
        o = DevBuf.from_array(np.zeros((h3 // 2, w // 2), np.float32) if init is None else init)
        fn = lib().ef_op_resize_nmap if normalize else lib().ef_op_resize_vmap
        _chk(fn(s.p, w, h3 // 3, o.p, None))
        return o.to_array(np.float32, (h3 // 2, w // 2))

    @staticmethod
    def pyr_down_gauss_f(src):
        return ops._image_op("pyr_down_gauss_f", src, np.float32, 2)

    @staticmethod
    def pyr_down_uchar_gauss(src):
        return ops._image_op("pyr_down_uchar_gauss", src, np.uint8, 2)

    @staticmethod
    def vertices_to_depth(vmaps_tmp, cutoff):
        return ops._image_op("vertices_to_depth", ops._f32(vmaps_tmp), np.float32, 1, cutoff)

    @staticmethod
    def bgr_to_intensity(rgba):
        return ops._image_op("image_bgr_to_intensity", rgba, np.uint8, 1)

    @staticmethod
    def derivative_images(img):
        h, w = img.shape
        s, dx, dy = DevBuf.from_array(img), DevBuf(h * w * 2), DevBuf(h * w * 2)
        _chk(lib().ef_op_compute_derivative_images(s.p, w, h, dx.p, dy.p, None))
        return dx.to_array(np.int16, (h, w)), dy.to_array(np.int16, (h, w))

    @staticmethod
    def project_to_point_cloud(depth, fx, fy, cx, cy, level=0):
        h, w = depth.shape
        s, d = DevBuf.from_array(depth), DevBuf(h * w * 12)
        k = ef_intr(fx, fy, cx, cy)
        _chk(lib().ef_op_project_to_point_cloud(s.p, w, h, C.byref(k), level, d.p, None))
        return d.to_array(np.float32, (h, w, 3))

    @staticmethod
    def icp_step(Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, distThres, angleThres):
        h3, w = vmap_curr.shape
        bufs = [DevBuf.from_array(a) for a in (vmap_curr, nmap_curr, vmap_g_prev, nmap_g_prev)]
        A, b, res = np.zeros((6, 6), np.float32), np.zeros(6, np.float32), np.zeros(2, np.float32)
        k = ef_intr(*intr)
        _chk(lib().ef_op_icp_step(_ptr(ops._f32(Rcurr).reshape(9)), _ptr(ops._f32(tcurr)), bufs[0].p, bufs[1].p,
                                  _ptr(ops._f32(Rprev_inv).reshape(9)), _ptr(ops._f32(tprev)), C.byref(k), bufs[2].p, bufs[3].p,
                                  distThres, angleThres, w, h3 // 3, _ptr(A), _ptr(b), _ptr(res), None))
        return A, b, res

    @staticmethod
    def rgb_residual(minScale, dIdx, dIdy, lastDepth, nextDepth, lastImage, nextImage, maxDepthDelta, kt, krkinv):
        h, w = nextImage.shape
        bufs = [DevBuf.from_array(a) for a in (dIdx, dIdy, lastDepth, nextDepth, lastImage, nextImage)]
        corres = DevBuf(h * w * 16)
        sigma, count = c_i(0), c_i(0)
        _chk(lib().ef_op_compute_rgb_residual(minScale, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, bufs[4].p, bufs[5].p, corres.p,
                                              maxDepthDelta, _ptr(ops._f32(kt)), _ptr(ops._f32(krkinv).reshape(9)), w, h,
                                              C.byref(sigma), C.byref(count), None))
        return corres.to_array(DATATERM, (h, w)), sigma.value, count.value

    @staticmethod
    def rgb_step(corres, sigma, cloud, fx, fy, dIdx, dIdy, sobelScale):
        h, w = corres.shape
        bufs = [DevBuf.from_array(a) for a in (corres, ops._f32(cloud), dIdx, dIdy)]
        A, b = np.zeros((6, 6), np.float32), np.zeros(6, np.float32)
        _chk(lib().ef_op_rgb_step(bufs[0].p, sigma, bufs[1].p, fx, fy, bufs[2].p, bufs[3].p, sobelScale, w, h,
                                  _ptr(A), _ptr(b), None))
        return A, b

    @staticmethod
    def so3_step(lastImage, nextImage, imageBasis, kinv, krlr):
        h, w = nextImage.shape
        li, ni = DevBuf.from_array(lastImage), DevBuf.from_array(nextImage)
        A, b, res = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32)
        _chk(lib().ef_op_so3_step(li.p, ni.p, _ptr(ops._f32(imageBasis).reshape(9)), _ptr(ops._f32(kinv).reshape(9)),
                                  _ptr(ops._f32(krlr).reshape(9)), w, h, _ptr(A), _ptr(b), _ptr(res), None))
        return A, b, res

    @staticmethod
    def model_maps(pred_vertex, pred_normal, fill_vertex, fill_normal, R, t, maxDepthRGB=6.0, pred_image=None, fill_image=None, camera_frame=False,
                   force_fill_image=False, tally=False, dense_count=0, dense_samples=1, joint=False, raw=None, rgb=None, depth_cut=3.0, init=None):
        """The tracker's model-side input launch on caller-supplied maps (ef_op_model_maps): k_model_maps, or -- joint -- k_frame_inputs with the
        pre-processing of (raw, rgb) in the same grid.  init: dict name -> contents an output starts from (vmap0..2, nmap0..2, depth0, last0,
        and the joint outputs; zeros otherwise).  Returns a dict of arrays with those names plus dense_count."""
        h, w, _ = pred_vertex.shape
        init = init or {}
        keep = [DevBuf.from_array(ops._f32(a)) for a in (pred_vertex, pred_normal, fill_vertex, fill_normal)]
        a = ef_model_maps_op()
        a.cols, a.rows = w, h
        a.pred_vertex, a.pred_normal, a.fill_vertex, a.fill_normal = (b.p for b in keep)
        if pred_image is not None:
            imgs = [DevBuf.from_array(np.ascontiguousarray(i, np.uint8)) for i in (pred_image, fill_image)]
            keep += imgs
            a.pred_image, a.fill_image = imgs[0].p, imgs[1].p
        a.R[:] = [float(v) for v in ops._f32(R).reshape(9)]
        a.t[:] = [float(v) for v in ops._f32(t).reshape(3)]
        a.max_depth_rgb = float(maxDepthRGB)
        a.camera_frame, a.force_fill_image, a.tally = int(camera_frame), int(force_fill_image), int(tally)
        a.dense_count, a.dense_samples = int(dense_count), int(dense_samples)
        spec = {}
        for l in range(3):
            spec[f"vmap{l}"] = spec[f"nmap{l}"] = (np.float32, (3 * (h >> l), w >> l))
        spec["depth0"], spec["last0"] = (np.float32, (h, w)), (np.uint8, (h, w))
        if joint:
            spec.update(filtered=(np.uint16, (h, w)), metric=(np.float32, (h, w)), metric_filtered=(np.float32, (h, w)), next0=(np.uint8, (h, w)))
        out = {}
        for name, (dt, shp) in spec.items():
            start = np.zeros(shp, dt) if name not in init else np.ascontiguousarray(init[name], dt)
            assert start.shape == shp, (name, start.shape, shp)
            out[name] = DevBuf.from_array(start)
        for l in range(3):
            a.vmap[l], a.nmap[l] = out[f"vmap{l}"].p, out[f"nmap{l}"].p
        a.depth0, a.last0 = out["depth0"].p, out["last0"].p
        if joint:
            fr = [DevBuf.from_array(np.ascontiguousarray(raw, np.uint16)), DevBuf.from_array(np.ascontiguousarray(rgb, np.uint8))]
            assert raw.shape == (h, w) and rgb.shape == (h, w, 3)
            keep += fr
            a.joint, a.raw, a.rgb3, a.depth_cut = 1, fr[0].p, fr[1].p, float(depth_cut)
            a.filtered, a.metric, a.metric_filtered, a.next0 = (out[n].p for n in ("filtered", "metric", "metric_filtered", "next0"))
        left = C.c_uint(0)
        _chk(lib().ef_op_model_maps(C.byref(a), C.byref(left), None))
        res = {name: out[name].to_array(*spec[name]) for name in spec}
        res["dense_count"] = int(left.value)
        return res

    @staticmethod
    def sobel_mask(nextImage, nextDepth):
        """k_sobel_levels on a caller's pyramids (ef_op_sobel_mask): nextImage / nextDepth are lists of three levels; returns four lists
        (dIdx, dIdy, mask, corres) of three arrays each."""
        h, w = nextImage[0].shape
        img = [DevBuf.from_array(np.ascontiguousarray(a, np.uint8)) for a in nextImage]
        dep = [DevBuf.from_array(ops._f32(a)) for a in nextDepth]
        for l in range(3):
            assert nextImage[l].shape == nextDepth[l].shape == (h >> l, w >> l), (l, nextImage[l].shape, nextDepth[l].shape)
        # (outputs start from a pattern no result can be mistaken for: 0xA5 bytes)
        outs = [[DevBuf((h >> l) * (w >> l) * sz, fill=0xA5) for l in range(3)] for sz in (2, 2, 1, 4)]
        arr = lambda bufs: (P * 3)(*[b.p for b in bufs])
        _chk(lib().ef_op_sobel_mask(arr(img), arr(dep), w, h, arr(outs[0]), arr(outs[1]), arr(outs[2]), arr(outs[3]), None))
        return tuple([b.to_array(dt, (h >> l, w >> l)) for l, b in enumerate(bufs)] for bufs, dt in zip(outs, (np.int16, np.int16, np.uint8, np.uint32)))

    @staticmethod
    def clean_deform(cam, T_wc, time, idx, vc, ct, nr, confThreshold, timeDelta, maxDepth, surfels, newUnstable, graph, depth, isFern=0):
        s = ops._f32(surfels).reshape(-1, 12)
        nu = ops._f32(newUnstable).reshape(-1, 12)
        g = ops._f32(graph).reshape(-1, 16)
        bufs = [DevBuf.from_array(a) for a in (idx, ops._f32(vc), ops._f32(ct), ops._f32(nr), g, ops._f32(depth))]
        sb, nb = DevBuf.from_array(s), DevBuf.from_array(nu if len(nu) else np.zeros((1, 12), np.float32))
        out = DevBuf((len(s) + len(nu) + 1) * 48)
        n = c_u32(0)
        _chk(lib().ef_op_clean_deform(C.byref(cam), _ptr(ops._T(T_wc)), time, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p,
                                      confThreshold, timeDelta, maxDepth, sb.p, len(s), nb.p, len(nu),
                                      bufs[4].p, len(g), bufs[5].p, int(isFern), out.p, C.byref(n), None))
        return out.to_array(np.float32, (n.value, 12))

    LINALG = dict(ldlt6=0, ldlt3f=1, polar3=2, rodrigues=3, se3_inverse=4, se3_log_norm=5, scalar=6, ldlt6_wave=7, ldlt6_every_lane=8,
                  mat_to_quat=9, se3_mul=10, se3_castf=11, se3_inverse_f=12, m4_affine_inverse=13, ldlt_pivots=14, lu_inverse6=15)

    @staticmethod
    def linalg(which, vec, n_out):
        """The driver's Eigen/Sophus arithmetic as the device evaluates it (ef_op_linalg)."""
        v = np.ascontiguousarray(np.asarray(vec, np.float64).reshape(-1))
        out = np.zeros(n_out, np.float64)
        _chk(lib().ef_op_linalg(ops.LINALG[which], _ptr(v), v.size, _ptr(out), n_out))
        return out

    GN_STATE = ("Rcurr", "tcurr", "resultRt", "krkinv", "kt", "lastRGBErrorLevel", "rgb_broken")

    @staticmethod
    def gn_update(sums, prev, Rprev, tprev, count, sigma, icp, rgb, rgbOnly, icpWeight, knext, level_changes, split_tail, lastA, lastb, stats):
        """One Gauss-Newton update step as the tracker's kernels run it, on caller-supplied state (ef_op_gn_update).  prev: dict with the
        members of GN_STATE; knext: (fx, fy, cx, cy); lastA [36], lastb [6], stats [4] = lastICPError, lastICPCount, lastRGBError,
        lastRGBCount before the step.  Returns (next: dict, lastA, lastb, stats) after it."""
        a = ef_gn_update_args()
        a.sums[:] = [float(v) for v in ops._f32(sums).reshape(58)]
        for name in ("Rcurr", "tcurr", "krkinv", "kt"):
            getattr(a.prev, name)[:] = [float(v) for v in ops._f32(prev[name]).reshape(-1)]
        a.prev.resultRt[:] = [float(v) for v in np.asarray(prev["resultRt"], np.float64).reshape(16)]
        a.prev.lastRGBErrorLevel, a.prev.rgb_broken = float(np.float32(prev["lastRGBErrorLevel"])), int(prev["rgb_broken"])
        a.Rprev[:] = [float(v) for v in ops._f32(Rprev).reshape(9)]
        a.tprev[:] = [float(v) for v in ops._f32(tprev).reshape(3)]
        a.count, a.sigma, a.icp, a.rgb, a.rgb_only = int(count), int(sigma), int(icp), int(rgb), int(rgbOnly)
        a.icp_weight, a.knext, a.level_changes, a.split_tail = float(icpWeight), ef_intr(*[float(v) for v in knext]), int(level_changes), int(split_tail)
        nxt = ef_gn_state()
        A = np.ascontiguousarray(np.asarray(lastA, np.float64).reshape(36)).copy()
        b = np.ascontiguousarray(np.asarray(lastb, np.float64).reshape(6)).copy()
        st = ops._f32(stats).reshape(4).copy()
        _chk(lib().ef_op_gn_update(C.byref(a), C.byref(nxt), _ptr(A), _ptr(b), _ptr(st)))
        out = {n: np.array(getattr(nxt, n)) for n in ("Rcurr", "tcurr", "resultRt", "krkinv", "kt")}
        out["lastRGBErrorLevel"], out["rgb_broken"] = np.float32(nxt.lastRGBErrorLevel), int(nxt.rgb_broken)
        return out, A, b, st

    @staticmethod
    def track_end_tail(Rcurr, tcurr, Rprev, tprev, q_prev, t_prev, rgb, weightMultiplier):
        """The end of tracking on one lane (0.3 m guard, re-orthonormalisation, the float pose matrices, the velocity weighting, the logged
        pose) on caller-supplied state (ef_op_track_end_tail); returns a dict of arrays."""
        o = ef_track_end_out()
        qp = np.ascontiguousarray(np.asarray(q_prev, np.float64).reshape(4))
        tp = np.ascontiguousarray(np.asarray(t_prev, np.float64).reshape(3))
        _chk(lib().ef_op_track_end_tail(_ptr(ops._f32(Rcurr).reshape(9)), _ptr(ops._f32(tcurr).reshape(3)), _ptr(ops._f32(Rprev).reshape(9)),
                                        _ptr(ops._f32(tprev).reshape(3)), _ptr(qp), _ptr(tp), int(rgb), weightMultiplier, C.byref(o)))
        out = {n: np.array(getattr(o, n)) for n in ("q", "t", "logged", "T_cw", "pose_f", "R_wc_f", "t_wc_f")}
        out["weighting"] = np.float32(o.weighting)
        return out

    @staticmethod
    def filter_depth(raw, maxD):
        return ops._image_op("filter_depth", raw, np.uint16, 1, maxD)

    @staticmethod
    def metricise_depth(d_in, maxD):
        return ops._image_op("metricise_depth", d_in, np.float32, 1, maxD)

    @staticmethod
    def seed_map(cam, rgb, dm, dmf, time, maxDepth):
        Pn = cam.cols * cam.rows
        bufs = [DevBuf.from_array(a) for a in (rgb, dm, dmf)]
        out = DevBuf(Pn * 48)
        n = c_u32(0)
        _chk(lib().ef_op_seed_map(C.byref(cam), bufs[0].p, bufs[1].p, bufs[2].p, time, maxDepth, out.p, C.byref(n), None))
        return out.to_array(np.float32, (n.value, 12))

    @staticmethod
    def _T(T):
        return np.ascontiguousarray(T, np.float64).reshape(16)

    @staticmethod
    def predict_indices(cam, T_wc, time, surfels, maxDepth, timeDelta):
        s = ops._f32(surfels).reshape(-1, 12)
        Pn = cam.cols * cam.rows
        sb = DevBuf.from_array(s)
        idx, vc, ct, nr = DevBuf(Pn * 4), DevBuf(Pn * 16), DevBuf(Pn * 16), DevBuf(Pn * 16)
        _chk(lib().ef_op_predict_indices(C.byref(cam), _ptr(ops._T(T_wc)), time, sb.p, len(s), maxDepth, timeDelta,
                                         idx.p, vc.p, ct.p, nr.p, None))
        shp = (cam.rows, cam.cols)
        return (idx.to_array(np.uint32, shp), vc.to_array(np.float32, shp + (4,)), ct.to_array(np.float32, shp + (4,)),
                nr.to_array(np.float32, shp + (4,)))

    @staticmethod
    def combined_predict(cam, T_wc, surfels, maxDepth, confThreshold, time, maxTime, timeDelta):
        s = ops._f32(surfels).reshape(-1, 12)
        Pn = cam.cols * cam.rows
        sb = DevBuf.from_array(s)
        img, vt, nm, tm = DevBuf(Pn * 4), DevBuf(Pn * 16), DevBuf(Pn * 16), DevBuf(Pn * 2)
        _chk(lib().ef_op_combined_predict(C.byref(cam), _ptr(ops._T(T_wc)), sb.p, len(s), maxDepth, confThreshold,
                                          time, maxTime, timeDelta, img.p, vt.p, nm.p, tm.p, None))
        shp = (cam.rows, cam.cols)
        return (img.to_array(np.uint8, shp + (4,)), vt.to_array(np.float32, shp + (4,)), nm.to_array(np.float32, shp + (4,)),
                tm.to_array(np.uint16, shp))

    @staticmethod
    def synthesize_depth(cam, T_wc, surfels, maxDepth, confThreshold, time, maxTime, timeDelta):
        s = ops._f32(surfels).reshape(-1, 12)
        Pn = cam.cols * cam.rows
        sb, d = DevBuf.from_array(s), DevBuf(Pn * 4)
        _chk(lib().ef_op_synthesize_depth(C.byref(cam), _ptr(ops._T(T_wc)), sb.p, len(s), maxDepth, confThreshold,
                                          time, maxTime, timeDelta, d.p, None))
        return d.to_array(np.float32, (cam.rows, cam.cols))

    @staticmethod
    def fill_in(cam, image, vertex, normal, depthFiltered, rgb, passthrough=0, passthroughImage=0):
        bufs = [DevBuf.from_array(a) for a in (image, ops._f32(vertex), ops._f32(normal), depthFiltered, rgb)]
        Pn = cam.cols * cam.rows
        fi, fv, fn = DevBuf(Pn * 4), DevBuf(Pn * 16), DevBuf(Pn * 16)
        _chk(lib().ef_op_fill_in(C.byref(cam), bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, bufs[4].p, passthrough, passthroughImage,
                                 fi.p, fv.p, fn.p, None))
        shp = (cam.rows, cam.cols)
        return fi.to_array(np.uint8, shp + (4,)), fv.to_array(np.float32, shp + (4,)), fn.to_array(np.float32, shp + (4,))

    @staticmethod
    def dense_enough(cam, image):
        b = DevBuf.from_array(image)
        d = c_i(0)
        _chk(lib().ef_op_dense_enough(C.byref(cam), b.p, C.byref(d), None))
        return bool(d.value)

    @staticmethod
    def fuse(cam, T_wc, time, rgb, dm, dmf, idx, vc, ct, nr, maxDepth, weighting, surfels):
        s = ops._f32(surfels).reshape(-1, 12)
        bufs = [DevBuf.from_array(a) for a in (rgb, dm, dmf, idx, ops._f32(vc), ops._f32(ct), ops._f32(nr))]
        sb = DevBuf.from_array(s)
        nu = DevBuf((cam.cols // 2) * (cam.rows // 2) * 48)
        n = c_u32(0)
        _chk(lib().ef_op_fuse(C.byref(cam), _ptr(ops._T(T_wc)), time, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, bufs[4].p, bufs[5].p,
                              bufs[6].p, maxDepth, weighting, sb.p, len(s), nu.p, C.byref(n), None))
        return sb.to_array(np.float32, (len(s), 12)), nu.to_array(np.float32, (n.value, 12))

    @staticmethod
    def clean(cam, T_wc, time, idx, vc, ct, nr, confThreshold, timeDelta, maxDepth, surfels, newUnstable):
        s = ops._f32(surfels).reshape(-1, 12)
        nu = ops._f32(newUnstable).reshape(-1, 12)
        bufs = [DevBuf.from_array(a) for a in (idx, ops._f32(vc), ops._f32(ct), ops._f32(nr))]
        sb, nb = DevBuf.from_array(s), DevBuf.from_array(nu if len(nu) else np.zeros((1, 12), np.float32))
        out = DevBuf((len(s) + len(nu) + 1) * 48)
        n = c_u32(0)
        _chk(lib().ef_op_clean(C.byref(cam), _ptr(ops._T(T_wc)), time, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, confThreshold,
                               timeDelta, maxDepth, sb.p, len(s), nb.p, len(nu), out.p, C.byref(n), None))
        return out.to_array(np.float32, (n.value, 12))
