"""ctypes binding of include/gsplat/gs_abi.h (libgsplat_hip.so).

There is no CPU fallback: if the HIP library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $GSPLAT_LIB: another build of the same library (A/B measurements of compiler flags); never a different implementation
LIB_PATH = os.environ.get("GSPLAT_LIB") or os.path.abspath(os.path.join(_HERE, "..", "lib", "libgsplat_hip.so"))

GS_FLAG_EXACT_BLEND = 0x1
GS_FLAG_F32_TAP = 0x2
GS_FLAG_TIMING = 0x4
GS_FLAG_AUX_OUTPUTS = 0x8
GS_FLAG_SPLAT_STATE = 0x10

GS_STAGE_NAMES = ("preprocess", "scan", "emit", "sort", "ranges", "blend")

(GS_BUF_TILE_COUNTS, GS_BUF_TILE_OFFSETS, GS_BUF_GAUSSIAN_DATA, GS_BUF_KEYS_UNSORTED, GS_BUF_VALUES_UNSORTED, GS_BUF_KEYS,
 GS_BUF_VALUES, GS_BUF_RANGES, GS_BUF_RGBA8, GS_BUF_RGB_F32, GS_BUF_BLOCK_MASKS) = range(11)
GS_BUF_ALPHA_F32 = 13  # GS_FLAG_AUX_OUTPUTS (11 and 12 are the library's profiling and test taps)
GS_BUF_DEPTH_F32 = 14
GS_BUF_SPLAT_STATE = 15  # GS_FLAG_SPLAT_STATE

GS_OPT_BLEND_ABLATION = 1
GS_OPT_PERSISTENT_GRID = 2
GS_OPT_RESET_TIMING = 3
GS_OPT_EMIT_ORDER = 4
GS_OPT_UNFUSED = 5
GS_OPT_DEBUG_VIEW = 6
GS_OPT_TILE_CULL = 7
GS_OPT_FRAMES_IN_FLIGHT = 8
GS_OPT_FRAME_GRAPH = 9
GS_OPT_PROJ_CHUNKS = 10
GS_OPT_SELECT_TINT = 11

GS_ERR_INVALID_ARGUMENT = -1
GS_ERR_NO_SCENE = -5
GS_ERR_NO_FRAME = -6

# gs_pick
GS_PICK_OK = 0
GS_PICK_OUTSIDE_SLAB = 1
GS_PICK_NONE = 0xFFFFFFFF
GS_PICK_MAX_QUERIES = 65536
GS_PICK_MAX_CONTRIB = 256

# splat state (GS_FLAG_SPLAT_STATE)
GS_SPLAT_HIDDEN = 0x1
GS_SPLAT_SELECTED = 0x2
GS_STATE_SET, GS_STATE_CLEAR, GS_STATE_TOGGLE, GS_STATE_ASSIGN = 1, 2, 3, 4
GS_REGION_ALL, GS_REGION_SPHERE, GS_REGION_BOX, GS_REGION_SCREEN_RECT, GS_REGION_SCREEN_MASK = range(5)
GS_SELECT_TINT_DEFAULT = 0x80FFFF00

# splat transforms
GS_XFORM_POSITION, GS_XFORM_ORIENT, GS_XFORM_SIZE = 0x1, 0x2, 0x4

# colour grades
GS_GRADE_MATRIX, GS_GRADE_OFFSET, GS_GRADE_OPACITY = 0x1, 0x2, 0x4

# snapshots and write-back
GS_PART_POSITION, GS_PART_GEOMETRY, GS_PART_SH, GS_PART_STATE = 0x1, 0x2, 0x4, 0x8
GS_PART_RECORD = 0x7

# splat attributes (gs_attr.kind)
(GS_ATTR_POS_X, GS_ATTR_POS_Y, GS_ATTR_POS_Z, GS_ATTR_OPACITY_LOGIT, GS_ATTR_LOG_SCALE_MIN, GS_ATTR_LOG_SCALE_MAX, GS_ATTR_LOG_SCALE_SUM,
 GS_ATTR_ANISOTROPY, GS_ATTR_DC_R, GS_ATTR_DC_G, GS_ATTR_DC_B, GS_ATTR_DIST2, GS_ATTR_PLANE, GS_ATTR_COVER_HITS, GS_ATTR_COVER_MAX_WEIGHT,
 GS_ATTR_COVER_SUM, GS_ATTR_COUNT) = range(17)
GS_ATTR_NAMES = ("POS_X", "POS_Y", "POS_Z", "OPACITY_LOGIT", "LOG_SCALE_MIN", "LOG_SCALE_MAX", "LOG_SCALE_SUM", "ANISOTROPY", "DC_R", "DC_G",
                 "DC_B", "DIST2", "PLANE", "COVER_HITS", "COVER_MAX_WEIGHT", "COVER_SUM")
GS_ATTR_MAX_BINS = 1024
GS_CONSENSUS_MAX = 4096

# cell merge
GS_MERGE_SUM_DOUBLES = 64
GS_MERGE_NONE = 0xFFFFFFFF  # group_of of a splat that is in no merged group
GS_MERGE_DEFAULT_MAX_MEMBERS = 65536

# neighbourhoods
GS_ERR_CAPACITY = -8
GS_NEIGH_LIMIT_NONE = 0xFFFFFFFF  # gs_neigh.limit: count every neighbour

# clusters
GS_CLUSTER_NONE = 0xFFFFFFFF  # the label of a splat that is no member
GS_CLUSTER_MAX_ROUNDS = 64

# thinning
GS_THIN_NONE = 0xFFFFFFFF         # the keeper of a splat that is no member
GS_THIN_NO_PRIORITY = 0xFFFFFFFF  # gs_thin.priority.kind: no priority attribute
GS_THIN_ORDER_INDEX, GS_THIN_ASCENDING = 0x1, 0x2  # gs_thin.flags
GS_THIN_DEFAULT_ROUNDS = 64

# nearest neighbours
GS_KNN_MAX_K = 32
GS_KNN_NONE = 0xFFFFFFFF  # nearest of a splat without an accepted source (and of a splat that was no query)
GS_KNN_REFINE = 0x1       # gs_knn.flags: only the splats whose dist2 reads +inf now are queried and written

# surface
GS_SURFACE_ORIENT, GS_SURFACE_KEEP_SUMS = 0x1, 0x2  # gs_surface.flags
GS_SURFACE_SUM_WORDS = 10  # count, S x y z, M xx xy xz yy yz zz
(GS_SURFACE_VARIATION, GS_SURFACE_PLANARITY, GS_SURFACE_LINEARITY, GS_SURFACE_SPHERICITY, GS_SURFACE_FACING, GS_SURFACE_FACING_SIGNED,
 GS_SURFACE_COUNT) = range(7)  # gs_surface_range.kind

# packed scenes (gs_export_packed's order)
GS_PACK_ORDER_INDEX, GS_PACK_ORDER_MORTON = 0, 1

# every symbol include/gsplat/gs_abi.h declares
ABI_SYMBOLS = ("gs_last_error", "gs_abi_version", "gs_create", "gs_destroy", "gs_upload_splats", "gs_upload_splats_device",
               "gs_share_splats",
               "gs_ply_load", "gs_ply_free", "gs_upload_ply",
               "gs_render", "gs_render_debug", "gs_render_to", "gs_wait", "gs_render_host", "gs_wait_ticket", "gs_host_alloc", "gs_host_free", "gs_read_rgba8", "gs_read_buffer", "gs_device_ptr",
               "gs_get_stats", "gs_pick", "gs_state_region", "gs_state_ids", "gs_state_count", "gs_state_write",
               "gs_state_list", "gs_export_splats", "gs_export_splats_device", "gs_compact", "gs_ply_save", "gs_export_ply",
               "gs_append_splats", "gs_append_splats_device", "gs_append_ply", "gs_duplicate_splats",
               "gs_xform_compose", "gs_transform_splats", "gs_grade_compose", "gs_grade_splats",
               "gs_write_splats", "gs_write_splats_device", "gs_snapshot_take", "gs_snapshot_restore", "gs_snapshot_swap",
               "gs_snapshot_get_info", "gs_snapshot_free",
               "gs_coverage_accumulate", "gs_coverage_reset", "gs_coverage_read", "gs_state_coverage",
               "gs_attr_summary", "gs_attr_histogram", "gs_attr_read", "gs_state_attr", "gs_attr_moments", "gs_moments_host",
               "gs_neigh_count", "gs_neigh_read", "gs_state_neigh",
               "gs_cluster_label", "gs_cluster_read", "gs_state_cluster", "gs_state_cluster_linked",
               "gs_knn_search", "gs_knn_read", "gs_state_knn",
               "gs_thin_sample", "gs_thin_read", "gs_state_thin", "gs_thin_host",
               "gs_pair_moments", "gs_pair_moments_host", "gs_pair_plane_moments", "gs_pair_plane_moments_host",
               "gs_attr_consensus", "gs_consensus_host", "gs_attr_gather", "gs_planes_through",
               "gs_cell_merge", "gs_cell_merge_device", "gs_cell_merge_host",
               "gs_surface_estimate", "gs_surface_read", "gs_surface_read_sums", "gs_state_surface", "gs_surface_host",
               "gs_pack_encode", "gs_pack_decode", "gs_pack_save", "gs_pack_load", "gs_pack_logit_table", "gs_export_packed", "gs_upload_packed",
               "gs_append_packed", "gs_set_option", "gs_slab_width", "gs_assemble_slabs", "gs_sort_pairs_u32",
               "gs_exclusive_scan_u32")


class GsConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("tile_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("col_begin", ctypes.c_uint32),
                ("col_end", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("max_intersections", ctypes.c_uint64),
                ("stream", ctypes.c_void_p)]


class GsStats(ctypes.Structure):
    _fields_ = [("num_gaussians", ctypes.c_uint64), ("num_visible", ctypes.c_uint64), ("num_intersections", ctypes.c_uint64),
                ("num_processed", ctypes.c_uint64), ("num_tiles", ctypes.c_uint32), ("sort_passes", ctypes.c_uint32),
                ("frames", ctypes.c_uint64), ("stage_us", ctypes.c_float * 6), ("frame_us", ctypes.c_float),
                ("stage_us_mean", ctypes.c_float * 6), ("frame_us_mean", ctypes.c_float), ("frames_timed", ctypes.c_uint32), ("depth_ordered", ctypes.c_uint32), ("num_evaluated", ctypes.c_uint64),
                ("capacity", ctypes.c_uint64), ("max_intersections_seen", ctypes.c_uint64), ("truncated_frames", ctypes.c_uint64),
                ("tight_binning", ctypes.c_uint32), ("frames_in_flight", ctypes.c_uint32), ("graph_frames", ctypes.c_uint64),
                ("num_row_items", ctypes.c_uint64), ("num_row_slots", ctypes.c_uint64), ("row_capacity", ctypes.c_uint64)]


class GsPickQuery(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32)]


class GsPickResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_uint32), ("list_length", ctypes.c_uint32), ("hit_count", ctypes.c_uint32),
                ("first_id", ctypes.c_uint32), ("first_depth", ctypes.c_float), ("max_id", ctypes.c_uint32),
                ("max_weight", ctypes.c_float), ("median_id", ctypes.c_uint32), ("median_depth", ctypes.c_float),
                ("alpha", ctypes.c_float), ("depth_acc", ctypes.c_float), ("reserved", ctypes.c_uint32)]


class GsPickContrib(ctypes.Structure):
    _fields_ = [("id", ctypes.c_uint32), ("weight", ctypes.c_float)]


class GsRegion(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("a", ctypes.c_float * 3), ("b", ctypes.c_float * 3),
                ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("x1", ctypes.c_uint32), ("y1", ctypes.c_uint32),
                ("uniforms160", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("where_mask", ctypes.c_uint32),
                ("where_value", ctypes.c_uint32)]


class GsXform(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("m", ctypes.c_float * 12), ("q", ctypes.c_float * 4),
                ("log_scale", ctypes.c_float), ("sh1", ctypes.c_float * 9), ("sh2", ctypes.c_float * 25), ("sh3", ctypes.c_float * 49)]


class GsGrade(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("a", ctypes.c_float * 9), ("dc", ctypes.c_float * 3),
                ("opacity_logit", ctypes.c_float), ("reserved", ctypes.c_float)]


class GsSnapshotInfo(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("n_at_take", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("parts", ctypes.c_uint32),
                ("dense", ctypes.c_uint32)]


class GsCoverageRec(ctypes.Structure):
    _fields_ = [("sum_q", ctypes.c_uint64), ("hits", ctypes.c_uint32), ("max_weight", ctypes.c_float)]


class GsCoverRegion(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("x1", ctypes.c_uint32),
                ("y1", ctypes.c_uint32), ("mask", ctypes.c_void_p)]


class GsAttr(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("p", ctypes.c_float * 4)]


class GsAttrSummary(ctypes.Structure):
    _fields_ = [("matched", ctypes.c_uint64), ("nan", ctypes.c_uint64), ("min", ctypes.c_float), ("max", ctypes.c_float)]


GS_MOMENTS_MAX_ATTRS = 3


class GsExact(ctypes.Structure):  # hi = RN(sum), lo = RN(sum - hi)
    _fields_ = [("hi", ctypes.c_double), ("lo", ctypes.c_double)]


class GsAttrMoments(ctypes.Structure):  # prod: 00, 01, 02, 11, 12, 22
    _fields_ = [("matched", ctypes.c_uint64), ("counted", ctypes.c_uint64), ("sum", GsExact * 3), ("prod", GsExact * 6)]


class GsNeigh(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("radius", ctypes.c_float), ("limit", ctypes.c_uint32), ("src_mask", ctypes.c_uint32),
                ("src_value", ctypes.c_uint32), ("qry_mask", ctypes.c_uint32), ("qry_value", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("max_candidates", ctypes.c_uint64)]


class GsNeighInfo(ctypes.Structure):
    _fields_ = [("queried", ctypes.c_uint64), ("sources", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("cells", ctypes.c_uint32 * 3),
                ("cell_edge", ctypes.c_float)]


class GsCluster(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("radius", ctypes.c_float), ("mask", ctypes.c_uint32), ("value", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2), ("max_candidates", ctypes.c_uint64)]


class GsClusterInfo(ctypes.Structure):
    _fields_ = [("members", ctypes.c_uint64), ("clusters", ctypes.c_uint64), ("largest", ctypes.c_uint64), ("candidates", ctypes.c_uint64),
                ("rounds", ctypes.c_uint32), ("cells", ctypes.c_uint32 * 3), ("cell_edge", ctypes.c_float), ("reserved", ctypes.c_uint32)]


class GsThin(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("radius", ctypes.c_float), ("mask", ctypes.c_uint32), ("value", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("max_rounds", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
                ("max_candidates", ctypes.c_uint64), ("priority", GsAttr), ("reserved", ctypes.c_uint32 * 2)]


class GsThinInfo(ctypes.Structure):
    _fields_ = [("members", ctypes.c_uint64), ("kept", ctypes.c_uint64), ("dropped", ctypes.c_uint64), ("largest", ctypes.c_uint64),
                ("candidates", ctypes.c_uint64), ("rounds", ctypes.c_uint32), ("cells", ctypes.c_uint32 * 3), ("cell_edge", ctypes.c_float),
                ("reserved", ctypes.c_uint32)]


class GsKnn(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("radius", ctypes.c_float), ("k", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("src_mask", ctypes.c_uint32), ("src_value", ctypes.c_uint32), ("qry_mask", ctypes.c_uint32), ("qry_value", ctypes.c_uint32),
                ("max_candidates", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class GsKnnInfo(ctypes.Structure):
    _fields_ = [("queried", ctypes.c_uint64), ("sources", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("unresolved", ctypes.c_uint64),
                ("cells", ctypes.c_uint32 * 3), ("cell_edge", ctypes.c_float)]


class GsPairMoments(ctypes.Structure):  # pq: row-major (a, b)
    _fields_ = [("matched", ctypes.c_uint64), ("paired", ctypes.c_uint64), ("sum_p", GsExact * 3), ("sum_q", GsExact * 3), ("pq", GsExact * 9),
                ("pp", GsExact * 3), ("qq", GsExact * 3)]


class GsPairPlaneMoments(ctypes.Structure):  # G: the upper triangle of sum g g^T, row-major; h: sum g_k r
    _fields_ = [("matched", ctypes.c_uint64), ("paired", ctypes.c_uint64), ("G", GsExact * 21), ("h", GsExact * 6), ("rr", GsExact), ("d2", GsExact)]


class GsMerge(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("mask", ctypes.c_uint32), ("value", ctypes.c_uint32), ("cell", ctypes.c_float),
                ("min_members", ctypes.c_uint32), ("max_members", ctypes.c_uint32), ("op", ctypes.c_uint32), ("bits", ctypes.c_uint32)]


class GsMergeInfo(ctypes.Structure):
    _fields_ = [("eligible", ctypes.c_uint64), ("groups", ctypes.c_uint64), ("members", ctypes.c_uint64), ("largest", ctypes.c_uint64),
                ("cells", ctypes.c_uint32 * 3), ("cell_edge", ctypes.c_float)]


class GsSurface(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("radius", ctypes.c_float), ("flags", ctypes.c_uint32), ("src_mask", ctypes.c_uint32),
                ("src_value", ctypes.c_uint32), ("qry_mask", ctypes.c_uint32), ("qry_value", ctypes.c_uint32), ("toward", ctypes.c_float * 3),
                ("max_candidates", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class GsSurfaceInfo(ctypes.Structure):
    _fields_ = [("queried", ctypes.c_uint64), ("sources", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("unresolved", ctypes.c_uint64),
                ("cells", ctypes.c_uint32 * 3), ("cell_edge", ctypes.c_float)]


class GsSurfaceRange(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("lo", ctypes.c_float), ("hi", ctypes.c_float),
                ("inside", ctypes.c_uint32), ("axis", ctypes.c_float * 3)]


class GsPackInfo(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("file_bytes", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64)]


# numpy views of the same records (what Renderer.pick returns)
PICK_RESULT_DTYPE = np.dtype([(n, np.float32 if t is ctypes.c_float else np.uint32) for n, t in GsPickResult._fields_])
PICK_CONTRIB_DTYPE = np.dtype([("id", np.uint32), ("weight", np.float32)])
# gs_coverage_rec (what Renderer.read_coverage returns): sum_q / 2^32 is the sum of the weights alpha T, floor'ed per accepted pair
COVERAGE_DTYPE = np.dtype([("sum_q", np.uint64), ("hits", np.uint32), ("max_weight", np.float32)])


class GsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gsplat error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Loads libgsplat_hip.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libgsplat_hip.so not built: run `python gaussian-splatting-wgpu_amd/csrc/build.py` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, i32, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32
    L.gs_last_error.restype = ctypes.c_char_p
    L.gs_abi_version.restype = i32
    L.gs_create.argtypes = [ctypes.POINTER(GsConfig), ctypes.POINTER(vp)]
    L.gs_destroy.argtypes = [vp]
    L.gs_upload_splats.argtypes = [vp, vp, u64]
    L.gs_upload_splats_device.argtypes = [vp, vp, u64]
    L.gs_share_splats.argtypes = [vp, vp]
    L.gs_ply_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(i32)]
    L.gs_ply_free.argtypes = [vp]
    L.gs_upload_ply.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(u64)]
    L.gs_render.argtypes = [vp, vp]
    L.gs_render_debug.argtypes = [vp, vp]
    L.gs_render_to.argtypes = [vp, vp, vp]
    L.gs_wait.argtypes = [vp]
    L.gs_render_host.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_wait_ticket.argtypes = [vp, u64]
    L.gs_host_alloc.argtypes = [u64, ctypes.POINTER(vp)]
    L.gs_host_free.argtypes = [vp]
    L.gs_read_rgba8.argtypes = [vp, vp, u64]
    L.gs_read_buffer.argtypes = [vp, i32, vp, u64, ctypes.POINTER(u64)]
    L.gs_device_ptr.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.gs_get_stats.argtypes = [vp, ctypes.POINTER(GsStats)]
    L.gs_pick.argtypes = [vp, vp, u32, vp, u32, vp]
    L.gs_state_region.argtypes = [vp, ctypes.POINTER(GsRegion), u32, u32, ctypes.POINTER(u64)]
    L.gs_state_ids.argtypes = [vp, vp, u64, u32, u32]
    L.gs_state_count.argtypes = [vp, u32, u32, ctypes.POINTER(u64)]
    L.gs_state_write.argtypes = [vp, vp, u64]
    L.gs_state_list.argtypes = [vp, u32, u32, vp, u64, ctypes.POINTER(u64)]
    L.gs_export_splats.argtypes = [vp, u32, u32, vp, u64, ctypes.POINTER(u64), vp]
    L.gs_export_splats_device.argtypes = [vp, u32, u32, vp, u64, ctypes.POINTER(u64), vp]
    L.gs_compact.argtypes = [vp, u32, u32, ctypes.POINTER(u64), vp]
    L.gs_ply_save.argtypes = [ctypes.c_char_p, vp, u64, i32]
    L.gs_export_ply.argtypes = [vp, ctypes.c_char_p, u32, u32, i32, ctypes.POINTER(u64)]
    L.gs_append_splats.argtypes = [vp, vp, u64, u32, ctypes.POINTER(u64)]
    L.gs_append_splats_device.argtypes = [vp, vp, u64, u32, ctypes.POINTER(u64)]
    L.gs_append_ply.argtypes = [vp, ctypes.c_char_p, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.gs_duplicate_splats.argtypes = [vp, u32, u32, u32, ctypes.POINTER(u64), ctypes.POINTER(u64), vp]
    L.gs_xform_compose.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_float,
                                   ctypes.POINTER(ctypes.c_float), ctypes.POINTER(GsXform)]
    L.gs_transform_splats.argtypes = [vp, u32, u32, ctypes.POINTER(GsXform), ctypes.POINTER(u64)]
    L.gs_grade_compose.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_float, ctypes.c_float,
                                   ctypes.c_float, ctypes.c_float, ctypes.POINTER(GsGrade)]
    L.gs_grade_splats.argtypes = [vp, u32, u32, ctypes.POINTER(GsGrade), ctypes.POINTER(u64)]
    L.gs_write_splats.argtypes = [vp, vp, u64, vp, vp, u32, ctypes.POINTER(u64)]
    L.gs_write_splats_device.argtypes = [vp, vp, u64, vp, vp, u32, ctypes.POINTER(u64)]
    L.gs_snapshot_take.argtypes = [vp, u32, u32, u32, ctypes.POINTER(vp)]
    L.gs_snapshot_restore.argtypes = [vp, vp, u32, ctypes.POINTER(u64)]
    L.gs_snapshot_swap.argtypes = [vp, vp, u32, ctypes.POINTER(u64)]
    L.gs_snapshot_get_info.argtypes = [vp, ctypes.POINTER(GsSnapshotInfo)]
    L.gs_snapshot_free.argtypes = [vp]
    L.gs_coverage_accumulate.argtypes = [vp, ctypes.POINTER(GsCoverRegion), ctypes.POINTER(u64)]
    L.gs_coverage_reset.argtypes = [vp]
    L.gs_coverage_read.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_state_coverage.argtypes = [vp, u32, ctypes.c_float, u32, u32, u32, u32, u32, ctypes.POINTER(u64)]
    f32 = ctypes.c_float
    L.gs_attr_summary.argtypes = [vp, ctypes.POINTER(GsAttr), u32, u32, ctypes.POINTER(GsAttrSummary)]
    L.gs_attr_moments.argtypes = [vp, ctypes.POINTER(GsAttr), u32, u32, u32, ctypes.POINTER(GsAttrMoments)]
    L.gs_moments_host.argtypes = [ctypes.POINTER(vp), u32, u64, vp, u32, u32, ctypes.POINTER(GsAttrMoments)]
    L.gs_attr_histogram.argtypes = [vp, ctypes.POINTER(GsAttr), u32, u32, f32, f32, u32, vp]
    L.gs_attr_read.argtypes = [vp, ctypes.POINTER(GsAttr), u32, u32, vp, u64, ctypes.POINTER(u64), vp]
    L.gs_state_attr.argtypes = [vp, ctypes.POINTER(GsAttr), f32, f32, u32, u32, u32, u32, u32, ctypes.POINTER(u64)]
    L.gs_neigh_count.argtypes = [vp, ctypes.POINTER(GsNeigh), ctypes.POINTER(GsNeighInfo)]
    L.gs_neigh_read.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_state_neigh.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, ctypes.POINTER(u64)]
    L.gs_cluster_label.argtypes = [vp, ctypes.POINTER(GsCluster), ctypes.POINTER(GsClusterInfo)]
    L.gs_cluster_read.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_state_cluster.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, ctypes.POINTER(u64)]
    L.gs_state_cluster_linked.argtypes = [vp, u32, u32, u32, u32, u32, u32, ctypes.POINTER(u64)]
    L.gs_thin_sample.argtypes = [vp, ctypes.POINTER(GsThin), ctypes.POINTER(GsThinInfo)]
    L.gs_thin_read.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_state_thin.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, ctypes.POINTER(u64)]
    L.gs_thin_host.argtypes = [vp, vp, vp, u64, vp, vp, ctypes.POINTER(GsThin), vp, vp, ctypes.POINTER(GsThinInfo)]
    L.gs_knn_search.argtypes = [vp, ctypes.POINTER(GsKnn), ctypes.POINTER(GsKnnInfo)]
    L.gs_knn_read.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_state_knn.argtypes = [vp, f32, f32, u32, u32, u32, u32, u32, ctypes.POINTER(u64)]
    L.gs_pair_moments.argtypes = [vp, u32, u32, vp, f32, ctypes.POINTER(GsPairMoments)]
    L.gs_pair_moments_host.argtypes = [vp, vp, vp, u64, vp, vp, u32, u32, f32, ctypes.POINTER(GsPairMoments)]
    L.gs_pair_plane_moments.argtypes = [vp, u32, u32, vp, vp, vp, f32, ctypes.POINTER(GsPairPlaneMoments)]
    L.gs_pair_plane_moments_host.argtypes = [vp, vp, vp, u64, vp, vp, vp, u32, u32, vp, f32, ctypes.POINTER(GsPairPlaneMoments)]
    L.gs_attr_consensus.argtypes = [vp, u32, vp, u32, f32, f32, u32, u32, vp, ctypes.POINTER(u64)]
    L.gs_consensus_host.argtypes = [vp, vp, vp, u64, vp, u32, u32, u32, vp, u32, f32, f32, vp, ctypes.POINTER(u64)]
    L.gs_attr_gather.argtypes = [vp, ctypes.POINTER(GsAttr), vp, u64, vp]
    L.gs_planes_through.argtypes = [vp, u32, vp]
    L.gs_cell_merge.argtypes = [vp, ctypes.POINTER(GsMerge), vp, u64, vp, vp, ctypes.POINTER(GsMergeInfo)]
    L.gs_cell_merge_device.argtypes = [vp, ctypes.POINTER(GsMerge), vp, u64, vp, vp, ctypes.POINTER(GsMergeInfo)]
    L.gs_cell_merge_host.argtypes = [vp, vp, u64, ctypes.POINTER(GsMerge), vp, u64, vp, vp, ctypes.POINTER(GsMergeInfo)]
    L.gs_surface_estimate.argtypes = [vp, ctypes.POINTER(GsSurface), ctypes.POINTER(GsSurfaceInfo)]
    L.gs_surface_read.argtypes = [vp, vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_surface_read_sums.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.gs_state_surface.argtypes = [vp, ctypes.POINTER(GsSurfaceRange), u32, u32, u32, u32, ctypes.POINTER(u64)]
    L.gs_surface_host.argtypes = [vp, vp, u64, ctypes.POINTER(GsSurface), vp, vp, vp, vp, ctypes.POINTER(GsSurfaceInfo)]
    L.gs_pack_encode.argtypes = [vp, u64, i32, vp, vp, vp, ctypes.POINTER(u64)]
    L.gs_pack_decode.argtypes = [vp, vp, vp, u64, i32, vp]
    L.gs_pack_save.argtypes = [ctypes.c_char_p, vp, u64, i32]
    L.gs_pack_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(i32)]
    L.gs_pack_logit_table.argtypes = [vp]
    L.gs_export_packed.argtypes = [vp, ctypes.c_char_p, u32, u32, i32, i32, ctypes.POINTER(GsPackInfo), vp]
    L.gs_upload_packed.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(u64)]
    L.gs_append_packed.argtypes = [vp, ctypes.c_char_p, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.gs_set_option.argtypes = [vp, i32, ctypes.c_int64]
    L.gs_slab_width.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.gs_assemble_slabs.argtypes = [vp, vp, ctypes.POINTER(u32), u32, u64, vp]
    L.gs_sort_pairs_u32.argtypes = [i32, vp, vp, u64, u32]
    L.gs_exclusive_scan_u32.argtypes = [i32, vp, u64, ctypes.POINTER(u64)]
    for name in ABI_SYMBOLS:
        if name not in ("gs_last_error", "gs_ply_free", "gs_host_free"):
            getattr(L, name).restype = i32
    L.gs_ply_free.restype = None
    L.gs_host_free.restype = None
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise GsError(rc, load().gs_last_error().decode("utf-8", "replace"))


def sort_pairs(keys, values=None, key_bits=32, device=0):
    """GPUSorter.sort (radix_sort/sort.ts:341-350) on host arrays; returns sorted copies."""
    k = np.array(keys, dtype=np.uint32, copy=True)
    v = None if values is None else np.array(values, dtype=np.uint32, copy=True)
    check(load().gs_sort_pairs_u32(device, k.ctypes.data, None if v is None else v.ctypes.data, k.size, key_bits))
    return k, v


def exclusive_scan(data, device=0):
    """ExclusiveScanner.scan (exclusive_scan.ts:208-325): returns (offsets, total)."""
    d = np.array(data, dtype=np.uint32, copy=True)
    total = ctypes.c_uint64(0)
    check(load().gs_exclusive_scan_u32(device, d.ctypes.data, d.size, ctypes.byref(total)))
    return d, int(total.value)


def load_ply(path):
    """Native PackedGaussians (ply.ts:162-228): returns (records float32 [n,80], sh_degree)."""
    L = load()
    rec, n, deg = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int32()
    check(L.gs_ply_load(str(path).encode(), ctypes.byref(rec), ctypes.byref(n), ctypes.byref(deg)))
    try:
        arr = np.ctypeslib.as_array(ctypes.cast(rec, ctypes.POINTER(ctypes.c_float)), shape=(max(n.value, 1) * 80,))[: n.value * 80]
        return arr.reshape(n.value, 80).copy(), deg.value
    finally:
        L.gs_ply_free(rec)


def save_ply(path, records, sh_degree=3):
    """gs_ply_save, the inverse of load_ply: float32 [n,80] records -> a binary little-endian 3DGS .ply (coefficients above
    sh_degree are not written)."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 80)
    check(load().gs_ply_save(str(path).encode(), rec.ctypes.data if rec.shape[0] else None, rec.shape[0], int(sh_degree)))


def compose_xform(rot=(1, 0, 0, 0), translate=(0, 0, 0), scale=1.0, pivot=None):
    """gs_xform_compose: the GsXform of p' = scale R (p - pivot) + pivot + translate, R the rotation of the quaternion `rot`
    (r, x, y, z; any non-zero length).  Host mathematics in double, no GPU: the 3x4 matrix, the normalised quaternion, log(scale)
    and the SH band matrices of R."""
    f3, f4 = ctypes.c_float * 3, ctypes.c_float * 4
    x = GsXform()
    check(load().gs_xform_compose(f4(*[float(v) for v in rot]), f3(*[float(v) for v in translate]), float(scale),
                                  None if pivot is None else f3(*[float(v) for v in pivot]), ctypes.byref(x)))
    return x


def compose_grade(gain=None, offset=None, saturation=1.0, black=0.0, white=1.0, opacity_gain=1.0):
    """gs_grade_compose: the GsGrade of C' = diag(gain) Sat(saturation) ((C - black) / (white - black)) + offset on the displayed
    colour, and of the opacity's odds multiplied by opacity_gain.  Host mathematics in double, no GPU: the 3x3 matrix over the SH
    coefficients, the band-0 offset and log(opacity_gain).  gain, offset: three numbers or None ((1, 1, 1) / (0, 0, 0))."""
    f3 = ctypes.c_float * 3
    g = GsGrade()
    check(load().gs_grade_compose(None if gain is None else f3(*[float(v) for v in gain]),
                                  None if offset is None else f3(*[float(v) for v in offset]), float(saturation), float(black),
                                  float(white), float(opacity_gain), ctypes.byref(g)))
    return g
