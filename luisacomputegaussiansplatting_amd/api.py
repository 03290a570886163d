"""ctypes binding of liblcgs_hip.so + the Python mirror of the reference's operator classes.

Reference interfaces mirrored here (paths relative to the reference repository):
  * ``Camera`` / ``get_lookat_cam`` ...............  lcgs/include/lcgs/util/camera.h:15-82
  * ``SHProcessor.process`` .......................  lcgs/include/lcgs/sh_preprocessor.h:30-37
  * ``GSProjector.forward`` + its two proxies .....  lcgs/include/lcgs/gs_projector.h:16-43
  * ``GSTileSplatter.forward`` + its three proxies   lcgs/include/lcgs/gs_tile_splatter.h:28-35, proxy.h:43-71
  * ``read_gs_ply`` ...............................  app/gaussians.cpp:75-171
  * ``Renderer`` (the per-frame loop body) ........  app/main.cpp:266-308

Device buffers are torch CUDA(=HIP) tensors; only their ``data_ptr()`` crosses the C ABI.

The C ABI is declared ONCE here: ``STRUCTS`` (the ctypes mirror of every struct of include/lcgs_hip.h) and ``SIGNATURES``
(restype and argtypes of every function), both held to the header by tests/test_abi.py.  Call sites pass plain Python values.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "liblcgs_hip.so"
_lib = None


class LcgsError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"lcgs status {status}: {message}")
        self.status = status


def library_path() -> str:
    return os.path.join(_PKG_DIR, _LIB_NAME)


def build_library(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into liblcgs_hip.so (in-tree).  Works without a GPU."""
    args = ["make", "-C", os.path.join(_PKG_DIR, "csrc"), "-j8"]
    if force:
        subprocess.check_call(args + ["clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return library_path()


# ---------------------------------------------------------------------------------------------- struct mirrors
# constants of include/lcgs_hip.h the mirrors and the wrappers need
LCGS_MAX_STAGES, LCGS_MAX_RANKS = 16, 64
LCGS_ERR_STATE = 8
DEPTH_Z, DEPTH_INV_Z = 0, 1  # LCGS_DEPTH_Z, LCGS_DEPTH_INV_Z
_DEPTH_MODES = {"z": DEPTH_Z, "inv_z": DEPTH_INV_Z}
LCGS_KNN_CHUNK = 256  # sorted points per query workgroup of the nearest-neighbour search (sizes around its multiples are edge cases)
LCGS_TSDF_VIEW_CHUNK = 42  # kTsdfViewChunk: views per launch of tsdf_integrate (view counts around its multiples are edge cases)
LCGS_ERR_CAPACITY = 5
LCGS_FEATURES_MAX = 256  # the most channels lcgs_render_features / lcgs_render_backward_features take
LCGS_FILTER3D_VIEW_CHUNK = 64  # kFilter3dViewChunk: views per launch of filter3d_accumulate (view counts around its multiples are edge cases)
# lcgs_set_fit_loss kinds (LCGS_LOSS_* in include/lcgs_hip.h)
LOSS_L2, LOSS_PHOTOMETRIC = 0, 1
# lcgs_set_raster_mode modes (LCGS_RASTER_* in include/lcgs_hip.h)
RASTER_CLASSIC, RASTER_ANTIALIASED = 0, 1
_RASTER_MODES = {"classic": RASTER_CLASSIC, "antialiased": RASTER_ANTIALIASED}

_KEYS = ("pos", "scale", "rotq", "sh", "opacity")


class Camera(C.Structure):
    """struct Camera, lcgs/include/lcgs/util/camera.h:15-25"""

    _fields_ = [
        ("position", C.c_float * 3),
        ("front", C.c_float * 3),
        ("up", C.c_float * 3),
        ("right", C.c_float * 3),
        ("fov", C.c_float),
        ("aspect_ratio", C.c_float),
        ("width", C.c_int),
        ("height", C.c_int),
    ]

    def to_dict(self):
        return {
            "position": list(self.position), "front": list(self.front), "up": list(self.up),
            "right": list(self.right), "fov": float(self.fov), "aspect_ratio": float(self.aspect_ratio),
            "width": int(self.width), "height": int(self.height),
        }

    @staticmethod
    def from_dict(d) -> "Camera":
        cam = Camera()
        for k in ("position", "front", "up", "right"):
            for i in range(3):
                getattr(cam, k)[i] = float(d[k][i])
        cam.fov = float(d["fov"])
        cam.aspect_ratio = float(d["aspect_ratio"])
        cam.width = int(d["width"])
        cam.height = int(d["height"])
        return cam


class _TileAccel(C.Structure):
    _fields_ = [
        ("tiles_touched", C.c_void_p), ("point_offsets", C.c_void_p), ("point_list_keys_unsorted", C.c_void_p),
        ("point_list_unsorted", C.c_void_p), ("point_list_keys", C.c_void_p), ("point_list", C.c_void_p),
        ("ranges", C.c_void_p), ("capacity", C.c_int64),
    ]


class _TileInput(C.Structure):
    _fields_ = [
        ("num_gaussians", C.c_int), ("bg_color", C.c_float * 3), ("means_2d", C.c_void_p),
        ("depth_features", C.c_void_p), ("conic", C.c_void_p), ("color_features", C.c_void_p),
        ("opacity_features", C.c_void_p),
    ]


class _TileOutput(C.Structure):
    _fields_ = [
        ("height", C.c_int), ("width", C.c_int), ("target_img", C.c_void_p), ("radii", C.c_void_p),
        ("final_T", C.c_void_p), ("n_contrib", C.c_void_p),
    ]


class _StageTimes(C.Structure):
    _fields_ = [("count", C.c_int), ("name", C.c_char_p * LCGS_MAX_STAGES), ("ms", C.c_float * LCGS_MAX_STAGES)]


class _FrameStats(C.Structure):
    _fields_ = [("num_gaussians", C.c_int64), ("num_visible", C.c_int64), ("num_rendered", C.c_int64),
                ("num_pairs", C.c_int64), ("num_tiles", C.c_int64), ("equal_depth_unresolved", C.c_int64),
                ("list_shift", C.c_int64)]


class _Grads(C.Structure):
    _fields_ = [("d_dL_dpos", C.c_void_p), ("d_dL_dscale", C.c_void_p), ("d_dL_drotq", C.c_void_p),
                ("d_dL_dsh", C.c_void_p), ("d_dL_dopacity", C.c_void_p)]


class _Params(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("scale", C.c_void_p), ("rotq", C.c_void_p), ("sh", C.c_void_p),
                ("opacity", C.c_void_p)]


class _AdamConfig(C.Structure):
    _fields_ = [("lr_pos", C.c_float), ("lr_sh_dc", C.c_float), ("lr_sh_rest", C.c_float), ("lr_opacity", C.c_float),
                ("lr_scale", C.c_float), ("lr_rot", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("step", C.c_int), ("visible_only", C.c_int)]


class _DensifyStats(C.Structure):
    _fields_ = [("grad_accum", C.c_void_p), ("denom", C.c_void_p), ("max_radii", C.c_void_p)]


class _DensifyConfig(C.Structure):
    _fields_ = [("grad_threshold", C.c_float), ("percent_dense", C.c_float), ("scene_extent", C.c_float),
                ("min_opacity", C.c_float), ("max_screen_size", C.c_int), ("seed", C.c_uint64)]


class _McmcConfig(C.Structure):
    _fields_ = [("min_opacity", C.c_float), ("n_max", C.c_int), ("seed", C.c_uint64)]


class _McmcNoiseConfig(C.Structure):
    _fields_ = [("noise_lr", C.c_float), ("lr_pos", C.c_float), ("k", C.c_float), ("x0", C.c_float), ("seed", C.c_uint64),
                ("step", C.c_int)]


class _ContribStats(C.Structure):
    _fields_ = [("weight_sum", C.c_void_p), ("weight_max", C.c_void_p), ("pixels", C.c_void_p), ("views", C.c_void_p)]


class _FeatureChannel(C.Structure):
    _fields_ = [("channels", C.c_int), ("d_features", C.c_void_p), ("d_dL_dfeature_map", C.c_void_p),
                ("d_dL_dfeatures", C.c_void_p)]


class _PruneConfig(C.Structure):
    _fields_ = [("min_weight_max", C.c_float), ("min_weight_sum", C.c_float), ("min_pixels", C.c_uint64),
                ("min_views", C.c_uint64)]


class _InitConfig(C.Structure):
    _fields_ = [("initial_opacity", C.c_float), ("min_dist2", C.c_float)]


class _TsdfVolume(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel_size", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("d_tsdf", C.c_void_p), ("d_weight", C.c_void_p), ("d_rgb", C.c_void_p)]


class _TsdfConfig(C.Structure):
    _fields_ = [("trunc", C.c_float), ("depth_max", C.c_float), ("alpha_min", C.c_float)]


class _DepthPriorConfig(C.Structure):
    _fields_ = [("kind", C.c_int), ("align", C.c_int), ("scale", C.c_float), ("shift", C.c_float), ("weight", C.c_float),
                ("alpha_min", C.c_float), ("patch", C.c_int), ("patch_x", C.c_int), ("patch_y", C.c_int)]


class Similarity(C.Structure):
    """lcgs_similarity: new = scale * rot * old + trans (rot row-major)"""

    _fields_ = [("rot", C.c_float * 9), ("scale", C.c_float), ("trans", C.c_float * 3)]


class SimilarityPlan(C.Structure):
    """lcgs_similarity_plan: what the transform kernels read (q stored (w, x, y, z); D_l row-major)"""

    _fields_ = [("M", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float), ("q", C.c_float * 4), ("D1", C.c_float * 9),
                ("D2", C.c_float * 25), ("D3", C.c_float * 49)]


class _SparseRows(C.Structure):
    _fields_ = [("d_rows", C.c_void_p), ("num_rows", C.c_int64), ("owner_first", C.c_int64 * (LCGS_MAX_RANKS + 2))]


class _CommStats(C.Structure):
    _fields_ = [("bytes_sent", C.c_int64), ("bytes_received", C.c_int64), ("touched_rows", C.c_int64),
                ("collective_groups", C.c_int)]


class _SelftestReport(C.Structure):
    _fields_ = [("world_size", C.c_int), ("rank", C.c_int), ("allreduce_ok", C.c_int), ("allreduce_ms", C.c_double),
                ("p2p_ok", C.c_int), ("p2p_ms", C.c_double), ("owner_step_ok", C.c_int), ("owner_step_ms", C.c_double),
                ("owner_max_grad_err", C.c_double), ("timed_out", C.c_int), ("message", C.c_char * 256)]


class _SceneHost(C.Structure):
    _fields_ = [("num_gaussians", C.c_int), ("sh_degree", C.c_int), ("pos", C.POINTER(C.c_float)),
                ("feature", C.POINTER(C.c_float)), ("opacity", C.POINTER(C.c_float)),
                ("scale", C.POINTER(C.c_float)), ("rotq", C.POINTER(C.c_float))]


# the header's struct name -> its mirror: every struct include/lcgs_hip.h defines with a body, except lcgs_comm_id (128
# opaque bytes the host carries between ranks: any 128-byte buffer, passed as a plain address)
STRUCTS = {
    "lcgs_camera": Camera, "lcgs_tile_accel": _TileAccel, "lcgs_tile_input": _TileInput, "lcgs_tile_output": _TileOutput,
    "lcgs_stage_times": _StageTimes, "lcgs_frame_stats": _FrameStats, "lcgs_grads": _Grads, "lcgs_params": _Params,
    "lcgs_adam_config": _AdamConfig, "lcgs_densify_stats": _DensifyStats, "lcgs_densify_config": _DensifyConfig,
    "lcgs_mcmc_config": _McmcConfig, "lcgs_mcmc_noise_config": _McmcNoiseConfig,
    "lcgs_init_config": _InitConfig, "lcgs_tsdf_volume": _TsdfVolume, "lcgs_tsdf_config": _TsdfConfig, "lcgs_depth_prior_config": _DepthPriorConfig, "lcgs_contrib_stats": _ContribStats, "lcgs_prune_config": _PruneConfig,
    "lcgs_feature_channel": _FeatureChannel, "lcgs_similarity": Similarity, "lcgs_similarity_plan": SimilarityPlan,
    "lcgs_sparse_rows": _SparseRows, "lcgs_comm_stats": _CommStats, "lcgs_comm_selftest_report": _SelftestReport,
    "lcgs_scene_host": _SceneHost,
}


# ---------------------------------------------------------------------------------------------- signatures
def _signatures() -> dict:
    """name -> (restype, argtypes) of every function include/lcgs_hip.h declares, in the header's order.

    lcgs_status -> c_int, void -> None; scalars are the exact ctypes scalar; const char* -> c_char_p; int* / int64_t*
    out-parameters -> POINTER of the scalar; a pointer to a struct of STRUCTS -> POINTER(mirror); handle out-parameters and
    arrays of pointers -> POINTER(c_void_p); everything else that is an address (opaque handles, device and host data,
    `float x[3]` parameters, lcgs_comm_id*) -> c_void_p."""
    st, i, i64, u64, f, d, s, p = C.c_int, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_char_p, C.c_void_p
    pi, pi64, pp = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_void_p)
    ptr = {name[len("lcgs_"):]: C.POINTER(mirror) for name, mirror in STRUCTS.items()}
    cam, grads, params, adam = ptr["camera"], ptr["grads"], ptr["params"], ptr["adam_config"]
    dstats, packs = ptr["densify_stats"], [ptr["params"]] * 4
    cstats, prune = ptr["contrib_stats"], ptr["prune_config"]
    return {
        # library / context
        "lcgs_version": (s, []),
        "lcgs_last_error": (s, []),
        "lcgs_create": (st, [i, p, pp]),
        "lcgs_destroy": (st, [p]),
        "lcgs_set_stream": (st, [p, p]),
        "lcgs_synchronize": (st, [p]),
        # host camera helpers
        "lcgs_get_lookat_cam": (None, [p, p, p, cam]),
        "lcgs_local_to_world_matrix": (None, [cam, p]),
        "lcgs_world_to_local_matrix": (None, [cam, p]),
        "lcgs_projection_matrix": (None, [f, f, f, f, p]),
        # stage-level operators
        "lcgs_sh_process": (st, [p, i, p, cam, p, p, i, i]),
        "lcgs_project_forward": (st, [p, i, p, p, p, f, p, p, p, cam, i]),
        "lcgs_tile_splat_forward": (st, [p, ptr["tile_accel"], ptr["tile_input"], ptr["tile_output"], i, pi]),
        "lcgs_set_stage_mode": (st, [p, i]),
        "lcgs_stage_flush": (st, [p]),
        "lcgs_inclusive_sum_u32": (st, [p, p, p, i64]),
        "lcgs_sort_pairs_u64_u32": (st, [p, p, p, p, p, i64, i, i]),
        # the scene a context renders
        "lcgs_scene_bind": (st, [p, i, i, p, p, p, p, p]),
        "lcgs_scene_upload": (st, [p, i, i, p, p, p, p, p]),
        "lcgs_scene_load_ply": (st, [p, s, pi]),
        "lcgs_set_ingest_order": (st, [p, i]),
        "lcgs_scene_reorder_spatial": (st, [p, p]),
        "lcgs_scene_permutation": (st, [p, pp]),
        "lcgs_scene_pointers": (st, [p, pi, pi, pp, pp, pp, pp, pp]),
        "lcgs_scene_modified": (st, [p]),
        "lcgs_debug_verify_derived": (st, [p, pi64]),
        "lcgs_scene_declare_static": (st, [p, i, p, p, p]),
        "lcgs_scene_use_half_sh": (st, [p, i]),
        "lcgs_set_lod": (st, [p, i]),
        "lcgs_set_raster_mode": (st, [p, i]),
        "lcgs_scene_download": (st, [p, p, p, p, p, p]),
        # the fused frame
        "lcgs_render_forward": (st, [p, cam, p, f, p, p, i, pi]),
        "lcgs_render_forward_batch": (st, [p, i, cam, p, f, pp]),
        "lcgs_set_profiling": (st, [p, i]),
        "lcgs_get_stage_times": (st, [p, ptr["stage_times"]]),
        "lcgs_get_frame_stats": (st, [p, ptr["frame_stats"]]),
        "lcgs_set_list_policy": (st, [p, i]),
        "lcgs_debug_last_lists": (st, [p, p, p]),
        "lcgs_debug_last_state": (st, [p, p, p]),
        "lcgs_debug_blend_exp": (st, [p, p, p, i64]),
        "lcgs_debug_pipeline_counts": (st, [p, p, p, p]),
        "lcgs_debug_early_cull_count": (st, [p, p]),
        # backward
        "lcgs_render_backward": (st, [p, p, grads]),
        "lcgs_render_backward_accumulate": (st, [p, p, grads]),
        "lcgs_render_backward_compact": (st, [p, p, grads]),
        "lcgs_visible_rows": (st, [p, pp, pp]),
        # depth and alpha maps
        "lcgs_render_maps": (st, [p, i, p, p]),
        "lcgs_render_backward_maps": (st, [p, p, i, p, p, i, grads]),
        # depth-distortion map
        "lcgs_render_distortion": (st, [p, i, f, p]),
        "lcgs_render_backward_distortion": (st, [p, p, i, f, p, p, p, i, grads]),
        # normal map
        "lcgs_render_normals": (st, [p, p]),
        "lcgs_render_backward_normals": (st, [p, p, i, f, p, p, p, p, i, grads]),
        # caller-supplied feature channels
        "lcgs_render_features": (st, [p, i, i, p, p]),
        "lcgs_render_backward_features": (st, [p, p, i, f, p, p, p, p, ptr["feature_channel"], i, grads]),
        # per-splat blend-weight statistics
        "lcgs_contrib_accumulate": (st, [p, i, cstats]),
        # camera gradient
        "lcgs_camera_backward": (st, [p, p]),
        "lcgs_render_backward_camera": (st, [p, p, i, p, p, p]),
        "lcgs_camera_grad_to_twist": (st, [cam, p, p]),
        # optimiser step, losses
        "lcgs_adam_step": (st, [p, i, i, adam, grads, *packs]),
        "lcgs_render_backward_adam": (st, [p, p, i, i, adam, *packs]),
        "lcgs_l2_loss_backward": (st, [p, i, i, p, p, p, p]),
        "lcgs_photometric_loss_backward": (st, [p, i, i, p, p, f, p, p, p]),
        "lcgs_normal_consistency_loss_backward": (st, [p, cam, p, p, p, f, f, p, p, p, p]),
        "lcgs_depth_prior_loss_backward": (st, [p, i, i, p, p, p, p, ptr["depth_prior_config"], p, p, p, p]),
        # per-view bilateral-grid colour correction
        "lcgs_bilagrid_slice": (st, [p, i, i, p, i, i, i, p, p]),
        "lcgs_bilagrid_backward": (st, [p, i, i, p, i, i, i, p, p, p, p]),
        "lcgs_bilagrid_tv_loss_backward": (st, [p, p, i, i, i, i, f, p, p]),
        "lcgs_set_fit_loss": (st, [p, i, f]),
        "lcgs_fit_views": (st, [p, i, cam, p, f, pp, grads, p]),
        # adaptive density control
        "lcgs_densify_accumulate": (st, [p, i, dstats]),
        "lcgs_absgrad_accumulate": (st, [p, i, p, i, p, p, dstats, p]),
        "lcgs_densify": (st, [p, i, i, ptr["densify_config"], dstats, *packs, *packs[:3], dstats, i64, p, p, pi64]),
        "lcgs_contrib_keep_mask": (st, [p, i, prune, cstats, p]),
        "lcgs_prune": (st, [p, i, i, prune, cstats, *packs, *packs[:3], i64, p, pi64]),
        "lcgs_opacity_reset": (st, [p, i, f, *packs]),
        # 3DGS-MCMC density control
        "lcgs_mcmc_relocate": (st, [p, i, i, ptr["mcmc_config"], *packs, p, p, pi64]),
        "lcgs_mcmc_add": (st, [p, i, i, ptr["mcmc_config"], *packs, i64, i64, p, p]),
        "lcgs_mcmc_noise": (st, [p, i, ptr["mcmc_noise_config"], *packs[:2], p]),
        "lcgs_mcmc_regularize": (st, [p, i, f, f, grads]),
        # Mip-Splatting's 3-D smoothing filter
        "lcgs_filter3d_accumulate": (st, [p, i, p, i, cam, p, p]),
        "lcgs_filter3d_finalize": (st, [p, i, p, f, p]),
        "lcgs_filter3d_apply": (st, [p, i, p, p, p, p, p]),
        "lcgs_filter3d_backward": (st, [p, i, p, p, p, p, p, p, p]),
        # scene similarity transforms
        "lcgs_similarity_plan_make": (st, [ptr["similarity"], ptr["similarity_plan"], p]),
        "lcgs_camera_transform": (st, [cam, ptr["similarity"], cam]),
        "lcgs_scene_transform": (st, [p, i, i, ptr["similarity"], *packs[:2]]),
        "lcgs_scene_box_keep_mask": (st, [p, i, p, ptr["similarity"], p, p]),
        # a scene from a point cloud
        "lcgs_knn_mean_dist2": (st, [p, i64, p, p]),
        "lcgs_scene_init_from_points": (st, [p, i, i, p, p, ptr["init_config"], *packs[:2]]),
        "lcgs_scene_extent": (st, [i, cam, p, p]),
        "lcgs_points_read_ply": (st, [s, pi64, pp, pp]),
        "lcgs_points_free": (None, [p, p]),
        # TSDF fusion, marching tetrahedra
        "lcgs_tsdf_integrate": (st, [p, ptr["tsdf_volume"], ptr["tsdf_config"], i, cam, pp, pp, pp]),
        "lcgs_tsdf_mesh_count": (st, [p, ptr["tsdf_volume"], f, p, p]),
        "lcgs_tsdf_mesh_extract": (st, [p, ptr["tsdf_volume"], f, u64, u64, p, p, p, p, p]),
        "lcgs_mesh_write_ply": (st, [s, u64, p, p, u64, p]),
        # multi-GPU
        "lcgs_comm_unique_id": (st, [p]),
        "lcgs_comm_create": (st, [p, p, i, i, pp]),
        "lcgs_comm_destroy": (st, [p]),
        "lcgs_comm_info": (st, [p, pi, pi]),
        "lcgs_comm_set_transport": (st, [p, i]),
        "lcgs_comm_shard_rows": (None, [i64, i, i, pi64, pi64]),
        "lcgs_grads_allreduce": (st, [p, p, i, i, grads]),
        "lcgs_adam_step_sharded": (st, [p, p, i, i, adam, grads, *packs]),
        "lcgs_comm_track_touched_rows": (st, [p, i]),
        "lcgs_comm_get_stats": (st, [p, ptr["comm_stats"]]),
        "lcgs_adam_step_sparse": (st, [p, p, i, i, adam, grads, *packs]),
        "lcgs_sparse_touched_rows": (st, [p, p, i, i, ptr["sparse_rows"]]),
        "lcgs_sparse_message_words": (i64, [i64, i]),
        "lcgs_sparse_pack": (st, [p, i, grads, p, i64, p]),
        "lcgs_sparse_accumulate": (st, [p, i, grads, p, i64, i64, i64]),
        # splat ownership
        "lcgs_owner_project": (st, [p, i, cam, f, i, i, i, p, p, pi]),
        "lcgs_owner_project_views": (st, [p, i, i, cam, f, i, i, i, pp, pp]),
        "lcgs_owner_counts": (st, [p, i, i, pi]),
        "lcgs_owner_render": (st, [p, cam, p, i, p, p, p, i]),
        "lcgs_owner_render_backward": (st, [p, p, p]),
        "lcgs_owner_backward": (st, [p, i, p, grads, i]),
        "lcgs_comm_owner_rows": (None, [i64, i, i, pi64, pi64]),
        "lcgs_owner_step_forward": (st, [p, p, cam, p, f, p]),
        "lcgs_owner_step_backward": (st, [p, p, p, grads]),
        "lcgs_owner_step_set_async": (st, [p, i]),
        "lcgs_owner_step_finish": (st, [p, p, pi]),
        "lcgs_comm_selftest": (st, [p, p, d, ptr["comm_selftest_report"]]),
        "lcgs_loopback_group_create": (st, [i, pp]),
        "lcgs_loopback_group_destroy": (st, [p]),
        "lcgs_comm_create_loopback": (st, [p, p, i, pp]),
        # scene ingest / image egress
        "lcgs_ply_read": (st, [s, ptr["scene_host"]]),
        "lcgs_ply_write_raw": (st, [s, i, p, p, p, p, p, p]),
        "lcgs_ply_filter_rows": (st, [s, s, i64, p]),
        "lcgs_scene_host_free": (None, [ptr["scene_host"]]),
        "lcgs_synth_scene": (st, [i, u64, i64, i64, p, p, p, p, p]),
        "lcgs_image_to_rgb8": (None, [i, i, p, p]),
        "lcgs_image_to_rgb8_device": (st, [p, i, i, p, p]),
        "lcgs_write_png": (st, [s, i, i, p]),
    }


SIGNATURES = _signatures()
# every symbol include/lcgs_hip.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = list(SIGNATURES)


def load_library():
    """dlopen liblcgs_hip.so.  Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch ships its own libamdhip64, and a process that initialises two copies loses
    # the device in the second.  When torch is installed it is imported first, so that liblcgs_hip.so (linked against
    # the same soname) binds to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise LcgsError(-1, f"{path} is missing: run luisacomputegaussiansplatting_amd.build_library() "
                            f"(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _check(status: int):
    if status != 0:
        raise LcgsError(status, load_library().lcgs_last_error().decode(errors="replace"))


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _ptr(t) -> C.c_void_p:
    """device (or host) pointer of a torch tensor / numpy array / int / None"""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, int):
        return C.c_void_p(t)
    if hasattr(t, "data_ptr"):
        assert t.is_contiguous(), "buffers crossing the C ABI must be contiguous"
        return C.c_void_p(t.data_ptr())
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return C.c_void_p(t.ctypes.data)
    raise TypeError(type(t))


def _grads(g) -> _Grads:
    """lcgs_grads of a dict with the keys pos / scale / rotq / sh / opacity, or of the five buffers in that order"""
    return _Grads(*[_ptr(t) for t in ([g[k] for k in _KEYS] if isinstance(g, dict) else g)])


def _params(*dicts, partial: bool = False) -> list:
    """one lcgs_params per dict (keys as above; partial: a missing key is a NULL member)"""
    return [_Params(*[_ptr(d.get(k) if partial else d[k]) for k in _KEYS]) for d in dicts]


def _densify_stats(d: dict) -> _DensifyStats:
    return _DensifyStats(_ptr(d["grad_accum"]), _ptr(d["denom"]), _ptr(d["max_radii"]))


_CONTRIB_KEYS = ("weight_sum", "weight_max", "pixels", "views")


def _contrib_stats(d: dict) -> _ContribStats:
    """lcgs_contrib_stats of a dict; a missing key (or None) is a NULL member"""
    return _ContribStats(*[_ptr(d.get(k)) for k in _CONTRIB_KEYS])


def _contrib_rows(d: dict) -> int:
    return next((int(d[k].shape[0]) for k in _CONTRIB_KEYS if d.get(k) is not None), 0)  # (all NULL: the library refuses)


def _prune_config(min_weight_max: float = 0.0, min_weight_sum: float = 0.0, min_pixels: int = 0, min_views: int = 0) -> _PruneConfig:
    return _PruneConfig(min_weight_max, min_weight_sum, int(min_pixels), int(min_views))


def _adam_config(lr: dict, betas, eps: float, step: int, visible_only: int) -> _AdamConfig:
    return _AdamConfig(lr["pos"], lr["sh_dc"], lr["sh_rest"], lr["opacity"], lr["scale"], lr["rot"], betas[0], betas[1], eps,
                       int(step), int(visible_only))


# ---------------------------------------------------------------------------------------------- camera
def get_lookat_cam(pos, target, world_up, width: Optional[int] = None, height: Optional[int] = None,
                   fov: Optional[float] = None) -> Camera:
    """get_lookat_cam (camera.h:74-82); width/height additionally apply app/main.cpp:204-207."""
    cam = Camera()
    load_library().lcgs_get_lookat_cam(_f3(pos), _f3(target), _f3(world_up), C.byref(cam))
    if width is not None:
        cam.width, cam.height = int(width), int(height)
        cam.aspect_ratio = float(np.float32(width) / np.float32(height))
    if fov is not None:
        cam.fov = float(fov)
    return cam


def similarity(rot=None, scale: float = 1.0, trans=(0.0, 0.0, 0.0)) -> Similarity:
    """lcgs_similarity of a 3 x 3 rotation (None: the identity), a uniform scale and a translation: new = scale rot old + trans"""
    r = np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3)
    return Similarity((C.c_float * 9)(*[float(x) for x in r.reshape(9)]), float(scale), _f3(trans))


def similarity_plan(xf: Similarity):
    """lcgs_similarity_plan_make: (SimilarityPlan, D64) -- the binary32 plan the kernels read and the unrounded band matrices as
    three binary64 arrays D_1 [3, 3], D_2 [5, 5], D_3 [7, 7] (B_l(R d) = D_l B_l(d) in the basis of the library's SH terms)."""
    plan, d64 = SimilarityPlan(), np.zeros(83, np.float64)
    _check(load_library().lcgs_similarity_plan_make(C.byref(xf), C.byref(plan), _ptr(d64)))
    return plan, (d64[:9].reshape(3, 3).copy(), d64[9:34].reshape(5, 5).copy(), d64[34:].reshape(7, 7).copy())


def camera_transform(cam: Camera, xf: Similarity) -> Camera:
    """lcgs_camera_transform: the camera that sees the scene transformed by xf as `cam` saw the original"""
    out = Camera()
    _check(load_library().lcgs_camera_transform(C.byref(cam), C.byref(xf), C.byref(out)))
    return out


def _mat(fn, *args) -> np.ndarray:
    m = (C.c_float * 16)()
    fn(*args, m)
    return np.array(m, dtype=np.float32).reshape(4, 4).T.copy()  # (row, col) indexing


def local_to_world_matrix(cam: Camera) -> np.ndarray:
    return _mat(load_library().lcgs_local_to_world_matrix, C.byref(cam))


def world_to_local_matrix(cam: Camera) -> np.ndarray:
    return _mat(load_library().lcgs_world_to_local_matrix, C.byref(cam))


def projection_matrix(tanfovx: float, tanfovy: float, znear: float = 0.1, zfar: float = 100.0) -> np.ndarray:
    return _mat(load_library().lcgs_projection_matrix, tanfovx, tanfovy, znear, zfar)


# ---------------------------------------------------------------------------------------------- context
class Context:
    """One (GPU, stream) pair: Context::create_device + create_stream of app/main.cpp:162-163."""

    def __init__(self, device_id: int = 0, stream: Optional[int] = None):
        lib = load_library()
        if stream is None:
            try:
                import torch

                if torch.cuda.is_available():
                    stream = torch.cuda.current_stream(device_id).cuda_stream
            except ImportError:
                stream = 0
        self._h = C.c_void_p(0)
        _check(lib.lcgs_create(device_id, stream, C.byref(self._h)))
        self.device_id = device_id

    def close(self):
        if self._h:
            load_library().lcgs_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(load_library().lcgs_synchronize(self._h))

    def set_stream(self, stream: int):
        _check(load_library().lcgs_set_stream(self._h, stream))

    def set_stage_mode(self, mode: str):
        """lcgs_set_stage_mode: "exact" (default: every operator runs at once and leaves the reference's buffers behind) or
        "deferred" (process / forward are recorded, a matching splatter call renders the fused frame instead)"""
        _check(load_library().lcgs_set_stage_mode(self._h, {"exact": 0, "deferred": 1}[mode]))

    def stage_flush(self):
        _check(load_library().lcgs_stage_flush(self._h))

    def blend_exp(self, d_x, d_out, n: int):
        """diagnostics: the compositing loop's exp (gs_math.hpp::blend_exp) over n device values"""
        _check(load_library().lcgs_debug_blend_exp(self._h, _ptr(d_x), _ptr(d_out), n))

    # lcpp primitives
    def inclusive_sum(self, d_in, d_out, n: int):
        _check(load_library().lcgs_inclusive_sum_u32(self._h, _ptr(d_in), _ptr(d_out), n))

    def sort_pairs(self, keys_in, keys_out, vals_in, vals_out, n: int, begin_bit: int = 0, end_bit: int = 64):
        _check(load_library().lcgs_sort_pairs_u64_u32(self._h, _ptr(keys_in), _ptr(keys_out), _ptr(vals_in),
                                                      _ptr(vals_out), n, begin_bit, end_bit))


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---------------------------------------------------------------------------------------------- proxies
@dataclass
class GPUPointsProxy:  # sh_preprocessor.h:16-20
    N: int = 0
    stride: int = 3
    pos: object = None


@dataclass
class GSProjectorInputProxy:  # gs_projector.h:16-22
    num_gaussians: int
    pos: object
    scale: object
    rotq: object
    scale_modifier: float = 1.0


@dataclass
class GSProjectorOutputProxy:  # gs_projector.h:24-28
    means_2d: object
    covs_2d: object
    depth: object


@dataclass
class GSTileSplatterInputProxy:  # proxy.h:43-54
    num_gaussians: int
    bg_color: tuple
    means_2d: object
    depth_features: object
    conic: object
    color_features: object
    opacity_features: object


@dataclass
class GSTileSplatterAccelProxy:  # proxy.h:56-64
    tiles_touched: object
    point_offsets: object
    point_list_keys_unsorted: object
    point_list_unsorted: object
    point_list_keys: object
    point_list: object
    ranges: object


@dataclass
class GSSplatForwardOutputProxy:  # proxy.h:66-71
    height: int
    width: int
    target_img: object
    radii: object
    final_T: object = None
    n_contrib: object = None


# ---------------------------------------------------------------------------------------------- operators
class SHProcessor:
    """lcgs::SHProcessor (sh_preprocessor.h:22-57)."""

    def __init__(self):
        self.ctx: Optional[Context] = None

    def create(self, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()

    def process(self, proxy: GPUPointsProxy, camera: Camera, sh, color, channel: int = 3, level: int = 3):
        if self.ctx is None:
            raise LcgsError(-1, "SHProcessor.create() was not called")
        _check(load_library().lcgs_sh_process(self.ctx._h, proxy.N, _ptr(proxy.pos), C.byref(camera), _ptr(sh), _ptr(color),
                                              level, channel))


class GSProjector:
    """lcgs::GSProjector (gs_projector.h:30-87)."""

    def __init__(self):
        self.ctx: Optional[Context] = None

    def create(self, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()

    def forward(self, input: GSProjectorInputProxy, output: GSProjectorOutputProxy, cam: Camera,
                use_focal: bool = True):
        if self.ctx is None:
            raise LcgsError(-1, "GSProjector.create() was not called")
        _check(load_library().lcgs_project_forward(
            self.ctx._h, input.num_gaussians, _ptr(input.pos), _ptr(input.scale), _ptr(input.rotq), input.scale_modifier,
            _ptr(output.means_2d), _ptr(output.covs_2d), _ptr(output.depth), C.byref(cam), bool(use_focal)))


class GSTileSplatter:
    """lcgs::GSTileSplatter (gs_tile_splatter.h:19-106)."""

    m_blocks = (16, 16)  # module.h:17

    def __init__(self):
        self.ctx: Optional[Context] = None
        self.num_rendered = 0  # gs_tile_splatter.h:23

    def create(self, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()

    def forward(self, accel: GSTileSplatterAccelProxy, input: GSTileSplatterInputProxy,
                output: GSSplatForwardOutputProxy, use_focal: bool = True) -> int:
        if self.ctx is None:
            raise LcgsError(-1, "GSTileSplatter.create() was not called")
        cap = int(accel.point_list.numel()) if hasattr(accel.point_list, "numel") else int(accel.point_list.size)
        a = _TileAccel(_ptr(accel.tiles_touched), _ptr(accel.point_offsets), _ptr(accel.point_list_keys_unsorted),
                       _ptr(accel.point_list_unsorted), _ptr(accel.point_list_keys), _ptr(accel.point_list),
                       _ptr(accel.ranges), cap)
        i = _TileInput(int(input.num_gaussians), _f3(input.bg_color), _ptr(input.means_2d),
                       _ptr(input.depth_features), _ptr(input.conic), _ptr(input.color_features),
                       _ptr(input.opacity_features))
        o = _TileOutput(int(output.height), int(output.width), _ptr(output.target_img), _ptr(output.radii),
                        _ptr(output.final_T), _ptr(output.n_contrib))
        n = C.c_int(0)
        _check(load_library().lcgs_tile_splat_forward(self.ctx._h, C.byref(a), C.byref(i), C.byref(o), bool(use_focal),
                                                      C.byref(n)))
        self.num_rendered = n.value
        return n.value


class Renderer:
    """The fused per-frame path: what app/main.cpp:266-308 does (SHProcessor.process + GSProjector.forward +
    GSTileSplatter.forward) as one stream submission."""

    def __init__(self, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self._keep = []  # keeps bound tensors alive
        self.P = 0
        self.sh_degree = 3
        # bumped by everything that replaces the state lcgs_render_backward works from (scene binding, a new frame):
        # render_autograd's backward compares it with the value its own forward left behind
        self._generation = 0

    def bind_scene(self, pos, scale, rotq, sh, opacity, sh_degree: int = 3):
        P = int(pos.shape[0])
        self._keep = [pos, scale, rotq, sh, opacity]
        self.P, self.sh_degree = P, sh_degree
        self._generation += 1
        _check(load_library().lcgs_scene_bind(self.ctx._h, P, sh_degree, _ptr(pos), _ptr(scale), _ptr(rotq), _ptr(sh),
                                              _ptr(opacity)))

    def declare_static(self, pos=None, scale=None, rotq=None):
        """lcgs_scene_declare_static: caller-owned arrays that do not change between frames get the cull pass's 16-byte
        {position, extent bound} rows (what a context-owned scene has by itself).  No arguments: withdraw."""
        if pos is None:
            _check(load_library().lcgs_scene_declare_static(self.ctx._h, 0, None, None, None))
            return
        self._static = [pos, scale, rotq]
        _check(load_library().lcgs_scene_declare_static(self.ctx._h, int(pos.shape[0]), _ptr(pos), _ptr(scale), _ptr(rotq)))

    def reorder_scene_spatial(self):
        """lcgs_scene_reorder_spatial: the context re-orders its scene along a Morton curve and renders from its own
        copy from now on.  Returns the permutation (device int32 tensor): new splat r = old splat perm[r]."""
        import torch

        perm = torch.empty(self.P, dtype=torch.int32, device=f"cuda:{self.ctx.device_id}")
        _check(load_library().lcgs_scene_reorder_spatial(self.ctx._h, _ptr(perm)))
        self._generation += 1
        self._keep = None  # the caller's arrays are no longer read
        return perm

    def _set_ingest_order(self, order: Optional[str]):
        if order is not None:
            _check(load_library().lcgs_set_ingest_order(self.ctx._h, {"file": 0, "spatial": 1}[order]))

    def upload_scene(self, scene: dict, sh_degree: int = 3, order: Optional[str] = None):
        """lcgs_scene_upload: host arrays -> device copies owned by the context, kept in spatial order by default
        (order="file" keeps the given order); see permutation() / scene_tensors()."""
        self._set_ingest_order(order)
        arrs = [np.ascontiguousarray(scene[k], dtype=np.float32) for k in _KEYS]
        P = int(arrs[0].reshape(-1, 3).shape[0])
        self.P, self.sh_degree = P, sh_degree
        self._generation += 1
        _check(load_library().lcgs_scene_upload(self.ctx._h, P, sh_degree, *[_ptr(a) for a in arrs]))

    def load_ply(self, path: str, order: Optional[str] = None) -> int:
        """read_gs_ply + upload with the de-interleave / activations on the device (lcgs_scene_load_ply).  order:
        "spatial" (the library's default: the context keeps its scene along a Morton curve) or "file"."""
        self._set_ingest_order(order)
        n = C.c_int(0)
        _check(load_library().lcgs_scene_load_ply(self.ctx._h, path.encode(), C.byref(n)))
        self.P, self.sh_degree, self._keep = n.value, 3, []
        self._generation += 1
        return n.value

    def _device_view(self, ptr: int, shape, typestr: str):
        """a torch tensor ALIASING context-owned device memory (no copy; valid while the context keeps that array)"""
        import torch

        class _View:
            __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}

        return torch.as_tensor(_View(), device=f"cuda:{self.ctx.device_id}")

    def scene_tensors(self) -> dict:
        """lcgs_scene_pointers as torch tensors aliasing the bound arrays (the context's own after load_ply / a re-order).
        The C ABI hands these out as const: the context keeps data derived from them (include/lcgs_hip.h).  torch has no
        read-only tensors, so the views are writable -- after writing them in place by anything but the library's own
        optimiser steps, call scene_modified(), or frames cull from stale rows (verify_derived() is the test-mode guard)."""
        ptrs = [C.c_void_p() for _ in _KEYS]
        n, deg = C.c_int(0), C.c_int(0)
        _check(load_library().lcgs_scene_pointers(self.ctx._h, C.byref(n), C.byref(deg), *[C.byref(p) for p in ptrs]))
        P, feat = n.value, (deg.value + 1) ** 2 * 3
        shapes = {"pos": (P, 3), "scale": (P, 3), "rotq": (P, 4), "sh": (P, feat), "opacity": (P,)}
        return {k: self._device_view(p.value, shapes[k], "<f4") for k, p in zip(_KEYS, ptrs)}

    def scene_modified(self):
        """lcgs_scene_modified: the bound arrays were written behind the library's back; derived data is dropped / rebuilt."""
        _check(load_library().lcgs_scene_modified(self.ctx._h))

    def verify_derived(self) -> int:
        """lcgs_debug_verify_derived: derived rows in use that no longer match the bound arrays (0 = consistent)."""
        n = C.c_int64(0)
        _check(load_library().lcgs_debug_verify_derived(self.ctx._h, C.byref(n)))
        return int(n.value)

    def permutation(self):
        """lcgs_scene_permutation: int32 device tensor, [r] = file index of splat r; None while in file / caller order."""
        p = C.c_void_p()
        _check(load_library().lcgs_scene_permutation(self.ctx._h, C.byref(p)))
        return self._device_view(p.value, (self.P,), "<i4") if p.value else None

    def use_half_sh(self, enable: bool = True):
        """lcgs_scene_use_half_sh: opt-in f16 copy of the SH coefficients for the fused forward (outside the 1e-4 bar)."""
        _check(load_library().lcgs_scene_use_half_sh(self.ctx._h, bool(enable)))

    def set_lod(self, min_radius_px: int):
        """lcgs_set_lod: opt-in footprint cull (0 = off): splats whose reference radius is below min_radius_px pixels are
        dropped from the fused frame.  Changes the image; never the default."""
        _check(load_library().lcgs_set_lod(self.ctx._h, int(min_radius_px)))

    def set_raster_mode(self, mode: str):
        """lcgs_set_raster_mode: "classic" (default: the reference's frame) or "antialiased" (every splat's opacity times
        rho = sqrt(det cov2d / det(cov2d + 0.3 I)), the 2-D filter of Mip-Splatting; same radii and num_rendered).  A kept
        frame remembers its mode: backward, maps, contrib and the camera gradient follow the frame, not the context.  The
        stage-level operators and the ownership step ignore it."""
        if mode not in _RASTER_MODES:
            raise ValueError(f"raster mode must be one of {sorted(_RASTER_MODES)}, not {mode!r}")
        _check(load_library().lcgs_set_raster_mode(self.ctx._h, _RASTER_MODES[mode]))

    def download_scene(self) -> dict:
        """Host copies of the bound scene (same keys and shapes as read_gs_ply)."""
        P, feat = self.P, (self.sh_degree + 1) ** 2 * 3
        out = {"pos": np.zeros((P, 3), np.float32), "scale": np.zeros((P, 3), np.float32),
               "rotq": np.zeros((P, 4), np.float32), "sh": np.zeros((P, feat), np.float32),
               "opacity": np.zeros((P,), np.float32)}
        _check(load_library().lcgs_scene_download(self.ctx._h, *[_ptr(out[k]) for k in _KEYS]))
        return out

    def forward(self, cam: Camera, img, bg=(0.0, 0.0, 0.0), scale_modifier: float = 1.0, radii=None,
                keep_state: bool = False, sync: bool = True) -> Optional[int]:
        n = C.c_int(0)
        self._generation += 1
        _check(load_library().lcgs_render_forward(self.ctx._h, C.byref(cam), _f3(bg), scale_modifier, _ptr(img), _ptr(radii),
                                                  bool(keep_state), C.byref(n) if sync else None))
        return n.value if sync else None

    def forward_batch(self, cams, imgs, bg=(0.0, 0.0, 0.0), scale_modifier: float = 1.0):
        """lcgs_render_forward_batch: one image per camera, two frames in flight; enqueues only."""
        n = len(cams)
        assert n == len(imgs)
        cam_arr = (Camera * n)(*cams)
        ptrs = (C.c_void_p * n)(*[_ptr(t).value for t in imgs])
        self._generation += 1
        _check(load_library().lcgs_render_forward_batch(self.ctx._h, n, cam_arr, _f3(bg), scale_modifier, ptrs))

    def backward(self, dL_dimg, dpos, dscale, drotq, dsh, dopacity, compact: bool = False, accumulate: bool = False):
        """lcgs_render_backward; compact=True: lcgs_render_backward_compact (row r = the frame's r-th on-screen
        splat, see visible_rows; only those rows are written); accumulate=True: lcgs_render_backward_accumulate (dense
        rows added to what the arrays hold: a further view of a multi-view batch)."""
        if compact and accumulate:
            raise ValueError("compact rows belong to one frame: they cannot be accumulated over views")
        g = _grads((dpos, dscale, drotq, dsh, dopacity))
        lib = load_library()
        fn = lib.lcgs_render_backward_compact if compact else (lib.lcgs_render_backward_accumulate if accumulate
                                                               else lib.lcgs_render_backward)
        _check(fn(self.ctx._h, _ptr(dL_dimg), C.byref(g)))

    def render_maps(self, depth, alpha, mode: str = "z"):
        """lcgs_render_maps: the accumulated depth (mode "z": view-space z, "inv_z": 1 / z) and the accumulated opacity of the
        last keep_state frame, H x W floats each; either may be None.  Enqueues only."""
        _check(load_library().lcgs_render_maps(self.ctx._h, _DEPTH_MODES[mode], _ptr(depth), _ptr(alpha)))

    def backward_maps(self, dL_dimg, dL_ddepth, dL_dalpha, dpos, dscale, drotq, dsh, dopacity, mode: str = "z",
                      accumulate: bool = False):
        """lcgs_render_backward_maps: dense rows of the gradient of <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha>
        for the last keep_state frame; any of the three incoming gradients may be None (not all)."""
        g = _grads((dpos, dscale, drotq, dsh, dopacity))
        _check(load_library().lcgs_render_backward_maps(self.ctx._h, _ptr(dL_dimg), _DEPTH_MODES[mode], _ptr(dL_ddepth),
                                                        _ptr(dL_dalpha), bool(accumulate), C.byref(g)))

    def render_distortion(self, dist, mode: str = "z", center: float = 0.0):
        """lcgs_render_distortion: the depth-distortion map of the last keep_state frame, H x W floats --
        sum_{i<j} w_i w_j (v_i - v_j)^2 per pixel in the closed form A M2 - M1^2 about `center` (any finite float; a typical
        depth of the scene cuts the cancellation).  Not normalised, not clamped, no background.  Enqueues only."""
        _check(load_library().lcgs_render_distortion(self.ctx._h, _DEPTH_MODES[mode], float(center), _ptr(dist)))

    def backward_distortion(self, dL_dimg, dL_ddepth, dL_dalpha, dL_ddist, dpos, dscale, drotq, dsh, dopacity, mode: str = "z",
                            center: float = 0.0, accumulate: bool = False):
        """lcgs_render_backward_distortion: backward_maps with the distortion map's incoming gradient as a fourth channel; any
        of the four may be None (not all).  With dL_ddist None it is backward_maps."""
        g = _grads((dpos, dscale, drotq, dsh, dopacity))
        _check(load_library().lcgs_render_backward_distortion(self.ctx._h, _ptr(dL_dimg), _DEPTH_MODES[mode], float(center),
                                                              _ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(dL_ddist),
                                                              bool(accumulate), C.byref(g)))

    def render_normals(self, normal):
        """lcgs_render_normals: the view-space normal map of the last keep_state frame, 3 x H x W floats (CHW) -- per pixel the
        sum of w_i n_i over the blended entries, n_i the splat's shortest axis turned to face the camera (include/lcgs_hip.h has
        the definition).  Not normalised, not clamped, no background.  Enqueues only."""
        _check(load_library().lcgs_render_normals(self.ctx._h, _ptr(normal)))

    def backward_normals(self, dL_dimg, dL_ddepth, dL_dalpha, dL_ddist, dL_dnormal, dpos, dscale, drotq, dsh, dopacity,
                         mode: str = "z", center: float = 0.0, accumulate: bool = False):
        """lcgs_render_backward_normals: backward_distortion with the normal map's incoming gradient (3 x H x W) as a fifth
        channel; any of the five may be None (not all).  With dL_dnormal None it is backward_distortion.  camera_backward is
        refused behind a call that passed dL_dnormal."""
        g = _grads((dpos, dscale, drotq, dsh, dopacity))
        _check(load_library().lcgs_render_backward_normals(self.ctx._h, _ptr(dL_dimg), _DEPTH_MODES[mode], float(center),
                                                           _ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(dL_ddist), _ptr(dL_dnormal),
                                                           bool(accumulate), C.byref(g)))

    def render_features(self, features, out):
        """lcgs_render_features: the caller's per-splat vectors blended like colour over the last keep_state frame.  features:
        [P, K] float32 rows in the context's row order (after upload_scene: features[permutation()]); out: K x H x W floats
        (CHW), per pixel the sum of w_i f_i over the blended entries.  Not normalised, not clamped, no background.  Enqueues only."""
        P, K = int(features.shape[0]), int(features.shape[1])
        _check(load_library().lcgs_render_features(self.ctx._h, P, K, _ptr(features), _ptr(out)))

    def backward_features(self, dL_dimg, dL_ddepth, dL_dalpha, dL_ddist, dL_dnormal, features, dL_dfeature_map, dL_dfeatures,
                          dpos=None, dscale=None, drotq=None, dsh=None, dopacity=None, mode: str = "z", center: float = 0.0,
                          accumulate: bool = False):
        """lcgs_render_backward_features: backward_normals with the feature map's incoming gradient (K x H x W) as one more
        channel group; dL_dfeatures ([P, K], overwritten or, accumulate, added to) may be None (the features are frozen).  With
        features None it is backward_normals.  All five gradient arrays None: the frozen-geometry mode -- dL_dfeatures alone,
        every other incoming gradient must then be None, and the frame's 2-D gradient rows are left as they were."""
        rows = (dpos, dscale, drotq, dsh, dopacity)
        g = None if all(t is None for t in rows) else _grads(rows)
        feat = None
        if features is not None:
            feat = _FeatureChannel(int(features.shape[1]), _ptr(features), _ptr(dL_dfeature_map), _ptr(dL_dfeatures))
        _check(load_library().lcgs_render_backward_features(
            self.ctx._h, _ptr(dL_dimg), _DEPTH_MODES[mode], float(center), _ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(dL_ddist),
            _ptr(dL_dnormal), None if feat is None else C.byref(feat), bool(accumulate), None if g is None else C.byref(g)))

    def camera_backward(self, out12):
        """lcgs_camera_backward: the camera gradient of the last backward of the kept frame -- 12 floats on the device in the
        order of Camera's members (position, front, up, right), overwritten.  Enqueues only."""
        _check(load_library().lcgs_camera_backward(self.ctx._h, _ptr(out12)))

    def backward_camera(self, dL_dimg, dL_ddepth, dL_dalpha, out12, mode: str = "z"):
        """lcgs_render_backward_camera: the walks and the camera pass, no parameter gradients; any of the three incoming
        gradients may be None (not all)."""
        _check(load_library().lcgs_render_backward_camera(self.ctx._h, _ptr(dL_dimg), _DEPTH_MODES[mode], _ptr(dL_ddepth),
                                                          _ptr(dL_dalpha), _ptr(out12)))

    def fit_views(self, cams, targets, dpos, dscale, drotq, dsh, dopacity, losses, bg=(0.0, 0.0, 0.0),
                  scale_modifier: float = 1.0):
        """lcgs_fit_views: the views of one optimiser step -- forward, the loss selected by set_fit_loss (L2 unless told
        otherwise) against targets[j], backward -- with the dense gradients summed into the five arrays and losses[j] (device
        tensor of len(cams) floats) = view j's loss; consecutive views overlap (forward beside the previous backward)."""
        n = len(cams)
        if len(targets) != n:
            raise ValueError("one target image per camera")
        cam_arr = (Camera * n)(*cams)
        ptrs = (C.c_void_p * n)(*[_ptr(t).value for t in targets])
        g = _grads((dpos, dscale, drotq, dsh, dopacity))
        _check(load_library().lcgs_fit_views(self.ctx._h, n, cam_arr, _f3(bg), scale_modifier, ptrs, C.byref(g),
                                             _ptr(losses)))
        self._generation += 1

    # ---- splat ownership: the frame in two halves
    OWNER_RECORD_FLOATS, OWNER_GRAD_FLOATS = 12, 12

    def owner_project(self, slot: int, cam: "Camera", row_first: int, row_count: int, keep_state: bool = True,
                      scale_modifier: float = 1.0):
        """lcgs_owner_project: the per-splat half of `cam`'s frame on the rows [row_first, row_first + row_count) of the bound
        scene -> (global row indices int32 [n], packed records float32 [n, 12]) of the rows that reach the screen."""
        import torch

        dev = torch.device("cuda", self.ctx.device_id)
        out_rows = torch.empty(max(row_count, 1), dtype=torch.int32, device=dev)
        out_recs = torch.empty(max(row_count, 1), self.OWNER_RECORD_FLOATS, dtype=torch.float32, device=dev)
        n = C.c_int(0)
        _check(load_library().lcgs_owner_project(self.ctx._h, slot, C.byref(cam), scale_modifier, row_first, row_count,
                                                 bool(keep_state), _ptr(out_rows), _ptr(out_recs), C.byref(n)))
        out_rows, out_recs = out_rows[:n.value], out_recs[:n.value]
        self._generation += 1
        return out_rows, out_recs

    def owner_project_all(self, cams, row_first: int, row_count: int, keep_state: bool = True, scale_modifier: float = 1.0):
        """The same for every view of a step -- view v into slot v -- with ONE synchronisation: lcgs_owner_project_views (N
        pipelines side by side), then lcgs_owner_counts.  -> [(rows, records)] per view."""
        import torch

        dev = torch.device("cuda", self.ctx.device_id)
        lib, N = load_library(), len(cams)
        outs = [(torch.empty(max(row_count, 1), dtype=torch.int32, device=dev),
                 torch.empty(max(row_count, 1), self.OWNER_RECORD_FLOATS, dtype=torch.float32, device=dev)) for _ in range(N)]
        # lcgs_owner_project_views: the N pipelines side by side on the context's lanes, joined on its stream
        rows_p = (C.c_void_p * N)(*[o[0].data_ptr() for o in outs])
        recs_p = (C.c_void_p * N)(*[o[1].data_ptr() for o in outs])
        _check(lib.lcgs_owner_project_views(self.ctx._h, 0, N, (Camera * N)(*cams), scale_modifier, row_first, row_count,
                                            bool(keep_state), rows_p, recs_p))
        counts = (C.c_int * N)()
        _check(lib.lcgs_owner_counts(self.ctx._h, 0, N, counts))
        self._generation += 1
        return [(r[:counts[v]], q[:counts[v]]) for v, (r, q) in enumerate(outs)]

    def owner_render(self, cam: "Camera", rows, recs, img, bg=(0.0, 0.0, 0.0), keep_state: bool = True):
        """lcgs_owner_render: the rest of the frame from received records (ascending global rows)"""
        _check(load_library().lcgs_owner_render(self.ctx._h, C.byref(cam), _f3(bg), int(rows.shape[0]), _ptr(rows), _ptr(recs),
                                                _ptr(img), bool(keep_state)))
        self._generation += 1

    def owner_render_backward(self, dL_dimg, grads2d):
        """lcgs_owner_render_backward: 2-D gradients (float32 [n, 12]) of the rows the last owner_render drew"""
        _check(load_library().lcgs_owner_render_backward(self.ctx._h, _ptr(dL_dimg), _ptr(grads2d)))

    def owner_backward(self, slot: int, grads2d, dpos, dscale, drotq, dsh, dopacity, accumulate: bool):
        """lcgs_owner_backward: the slot's rows' 2-D gradients -> parameter gradients at their rows of the full-size arrays"""
        g = _grads((dpos, dscale, drotq, dsh, dopacity))
        _check(load_library().lcgs_owner_backward(self.ctx._h, slot, _ptr(grads2d), C.byref(g), bool(accumulate)))

    def l2_loss_backward(self, img, target, dL_dimg, loss):
        """lcgs_l2_loss_backward: loss[0] = mean((img - target)^2), dL_dimg = 2 (img - target) / numel (device tensors)"""
        _, H, W = img.shape
        _check(load_library().lcgs_l2_loss_backward(self.ctx._h, W, H, _ptr(img), _ptr(target), _ptr(dL_dimg), _ptr(loss)))

    def photometric_loss_backward(self, img, target, dL_dimg, loss, lambda_dssim: float = 0.2, terms=None):
        """lcgs_photometric_loss_backward: loss[0] = (1 - lambda) mean|img - target| + lambda (1 - SSIM(img, target)), the 3DGS
        training loss (11 x 11 Gaussian window, sigma 1.5, zero padding); dL_dimg (None: evaluation only) = its gradient
        w.r.t. img; terms (optional, 2 floats) = (L1, SSIM).  Device tensors, img / target CHW float32; the same inputs give
        the same bits."""
        _, H, W = img.shape
        _check(load_library().lcgs_photometric_loss_backward(self.ctx._h, W, H, _ptr(img), _ptr(target), lambda_dssim,
                                                             _ptr(dL_dimg), _ptr(loss), _ptr(terms)))

    def normal_consistency_loss_backward(self, cam: Camera, depth, alpha, normal, dL_ddepth, dL_dalpha, dL_dnormal, loss,
                                         weight: float = 0.05, alpha_min: float = 1e-3):
        """lcgs_normal_consistency_loss_backward: loss[0] = weight x the mean over the interior pixels of alpha - normal . nt,
        nt the unit normal of the rendered depth surface z = depth / max(alpha, alpha_min) (central differences of the
        back-projected points, facing the camera), from a frame's depth [H, W] (mode "z"), alpha [H, W] and normal [3, H, W] maps;
        cam supplies width, height, fov and aspect ratio only.  dL_ddepth, dL_dalpha, dL_dnormal (all three, or all None:
        evaluation only) = its gradients, what backward_normals takes, written whole.  Device tensors, float32; binary64
        inside; the same inputs give the same bits."""
        _check(load_library().lcgs_normal_consistency_loss_backward(self.ctx._h, C.byref(cam), _ptr(depth), _ptr(alpha), _ptr(normal),
                                                                    weight, alpha_min, _ptr(dL_ddepth), _ptr(dL_dalpha),
                                                                    _ptr(dL_dnormal), _ptr(loss)))

    def depth_prior_loss_backward(self, depth, alpha, prior, dL_ddepth, dL_dalpha, loss, mask=None, kind: str = "pearson",
                                  align: str = "fit", scale: float = 1.0, shift: float = 0.0, weight: float = 1.0,
                                  alpha_min: float = 1e-3, patch: int = 0, patch_offset=(0, 0), stats=None):
        """lcgs_depth_prior_loss_backward: the rendered depth v = depth / max(alpha, alpha_min) of a frame's maps [H, W] against
        a depth the caller brings, prior [H, W], over the pixels where mask (optional, uint8 / bool [H, W]) is set and the prior
        is finite.  kind "pearson": loss[0] = weight x the mean over the groups of 1 - corr(v, prior); kind "l1": weight x the
        mean of |v - (s prior + t)|, (s, t) the group's least-squares fit (align "fit", detached) or (scale, shift) (align
        "given").  A group is the image (patch 0) or a patch x patch block (32, 64, 128) of the grid anchored at
        -patch_offset.  dL_ddepth, dL_dalpha (both, or both None: evaluation only) = its gradients, what backward_maps takes,
        written whole; stats (optional, 4 floats) = (N_c, G, s, t).  Device tensors, float32; binary64 inside; the same
        inputs give the same bits."""
        import torch

        H, W = depth.shape
        for name, t, dtypes in (("depth", depth, (torch.float32,)), ("alpha", alpha, (torch.float32,)),
                                ("prior", prior, (torch.float32,)), ("mask", mask, (torch.uint8, torch.bool)),
                                ("dL_ddepth", dL_ddepth, (torch.float32,)), ("dL_dalpha", dL_dalpha, (torch.float32,))):
            # (a mismatched buffer would be an out-of-bounds device access behind the C ABI, which sees pointers only)
            if t is not None and (t.dtype not in dtypes or tuple(t.shape) != (H, W) or t.device != depth.device or not t.is_contiguous()):
                raise ValueError(f"{name}: expected a contiguous {dtypes[0]} ({H}, {W}) tensor on {depth.device}, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
        for name, t, numel in (("loss", loss, 1), ("stats", stats, 4)):  # ... and so would a short or misplaced output
            if t is None and name == "loss":
                raise ValueError("loss: expected a float32 tensor of 1 element, got None")
            if t is not None and (t.dtype != torch.float32 or t.numel() != numel or t.device != depth.device or not t.is_contiguous()):
                raise ValueError(f"{name}: expected a contiguous float32 tensor of {numel} element(s) on {depth.device}, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
        kinds, aligns = {"pearson": 0, "l1": 1}, {"fit": 0, "given": 1}
        if kind not in kinds or align not in aligns:
            raise ValueError(f"kind must be one of {sorted(kinds)} and align one of {sorted(aligns)}, got {kind!r}, {align!r}")
        cfg = _DepthPriorConfig(kinds[kind], aligns[align], scale, shift, weight, alpha_min, int(patch), int(patch_offset[0]),
                                int(patch_offset[1]))
        _check(load_library().lcgs_depth_prior_loss_backward(self.ctx._h, W, H, _ptr(depth), _ptr(alpha), _ptr(prior), _ptr(mask),
                                                             C.byref(cfg), _ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(loss), _ptr(stats)))

    @staticmethod
    def _bilagrid_buffers(first, **named):
        """every named tensor (name -> (tensor or None, shape)) is float32, on `first`'s device and of its shape: a mismatched
        buffer would be an out-of-bounds device access behind the C ABI, which sees pointers only"""
        import torch

        for name, (t, shape) in named.items():
            if t is None:
                continue
            if t.dtype != torch.float32 or t.device != first.device or tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name}: expected float32 {tuple(shape)} on {first.device}, got {t.dtype} {tuple(t.shape)} "
                                 f"on {t.device}")

    def bilagrid_slice(self, grid, img, out):
        """lcgs_bilagrid_slice: out [3, H, W] = one view's bilateral grid [12, L, GH, GW] (3 x 4 affine colour transforms; channel
        4 r + k = row r, column k, column 3 the offset) sliced at (pixel x, pixel y, luminance of img's pixel) and applied to img
        [3, H, W].  Device tensors, float32 (shapes, dtype and device are checked: ValueError); out must not overlap img or grid.  An identity
        grid returns img bit for bit."""
        _, L, GH, GW = grid.shape
        _, H, W = img.shape
        self._bilagrid_buffers(img, grid=(grid, (12, L, GH, GW)), img=(img, (3, H, W)), out=(out, (3, H, W)))
        _check(load_library().lcgs_bilagrid_slice(self.ctx._h, W, H, _ptr(grid), GW, GH, L, _ptr(img), _ptr(out)))

    def bilagrid_backward(self, grid, img, dL_dout, dL_dimg=None, dL_dgrid=None):
        """lcgs_bilagrid_backward: from dL_dout [3, H, W], dL_dimg [3, H, W] and / or dL_dgrid [12, L, GH, GW] (None: not wanted;
        not both) of bilagrid_slice(grid, img).  Both are written whole, never accumulated: vertices no pixel reaches get exact
        zeros.  dL/dgrid is a fixed-order gather (no atomics): the same inputs give the same bits."""
        _, L, GH, GW = grid.shape
        _, H, W = img.shape
        self._bilagrid_buffers(img, grid=(grid, (12, L, GH, GW)), img=(img, (3, H, W)), dL_dout=(dL_dout, (3, H, W)),
                               dL_dimg=(dL_dimg, (3, H, W)), dL_dgrid=(dL_dgrid, (12, L, GH, GW)))
        _check(load_library().lcgs_bilagrid_backward(self.ctx._h, W, H, _ptr(grid), GW, GH, L, _ptr(img), _ptr(dL_dout),
                                                     _ptr(dL_dimg), _ptr(dL_dgrid)))

    def bilagrid_tv_loss_backward(self, grids, dL_dgrids, loss, weight: float = 10.0):
        """lcgs_bilagrid_tv_loss_backward: loss[0] = weight / N x the total variation of grids [N, 12, L, GH, GW] (the mean squared
        forward difference along x, y and z, summed over the three axes); dL_dgrids (None: evaluation only, the same loss bits)
        = its gradient, written whole.  Device tensors, float32; binary64 inside."""
        N, _, L, GH, GW = grids.shape
        self._bilagrid_buffers(grids, grids=(grids, (N, 12, L, GH, GW)), dL_dgrids=(dL_dgrids, (N, 12, L, GH, GW)),
                               loss=(loss, (1,)))
        _check(load_library().lcgs_bilagrid_tv_loss_backward(self.ctx._h, _ptr(grids), N, GW, GH, L, weight, _ptr(dL_dgrids),
                                                             _ptr(loss)))

    def set_fit_loss(self, kind: int, lambda_dssim: float = 0.2):
        """lcgs_set_fit_loss: the loss fit_views applies from now on -- LOSS_L2 (default) or LOSS_PHOTOMETRIC"""
        _check(load_library().lcgs_set_fit_loss(self.ctx._h, kind, lambda_dssim))

    def visible_rows(self):
        """lcgs_visible_rows of the last forward frame: (splat index of every compact row, row count) as a device
        int32 tensor copy (synchronises the context)."""
        import torch

        rows, count = C.c_void_p(), C.c_void_p()
        _check(load_library().lcgs_visible_rows(self.ctx._h, C.byref(rows), C.byref(count)))
        self.ctx.synchronize()
        n = self.frame_stats()["num_visible"]
        if n == 0:
            return torch.empty(0, dtype=torch.int32, device=f"cuda:{self.ctx.device_id}")
        return self._device_view(rows.value, (n,), "<i4").clone()  # the array is the context's: cloned before returning

    def set_profiling(self, enabled: bool):
        _check(load_library().lcgs_set_profiling(self.ctx._h, bool(enabled)))

    def stage_times(self) -> dict:
        t = _StageTimes()
        _check(load_library().lcgs_get_stage_times(self.ctx._h, C.byref(t)))
        return {t.name[i].decode(): float(t.ms[i]) for i in range(t.count)}

    def frame_stats(self) -> dict:
        s = _FrameStats()
        _check(load_library().lcgs_get_frame_stats(self.ctx._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in _FrameStats._fields_}

    def last_lists(self, d_list, d_ranges):
        """lcgs_debug_last_lists: the last fused frame's sorted lists (original splat indices) and ranges.  Per TILE after a frame
        with keep_state=True; a frame without it lists its pairs per block of 2 x 2 tiles (the first ceil(gx / 2) * ceil(gy / 2)
        ranges, row-major; the rest zero).  Either argument may be None."""
        _check(load_library().lcgs_debug_last_lists(self.ctx._h, _ptr(d_list), _ptr(d_ranges)))

    def pipeline_counts(self) -> dict:
        """lcgs_debug_pipeline_counts: forward frames that ran their head on the head stream, that chained, that used the
        bounded renderer grid"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(load_library().lcgs_debug_pipeline_counts(self.ctx._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"piped": a.value, "chained": b.value, "bounded": c.value}

    def early_cull_count(self) -> int:
        """lcgs_debug_early_cull_count: frames whose cull pass ran one slot ahead on the cull stream (those that chained while
        the GPU was behind the host)"""
        a = C.c_uint64(0)
        _check(load_library().lcgs_debug_early_cull_count(self.ctx._h, C.byref(a)))
        return a.value

    def set_list_policy(self, policy: str):
        """lcgs_set_list_policy: "tile" (the reference's per-tile lists), "block" (per 2 x 2 tiles), "auto" (default)"""
        _check(load_library().lcgs_set_list_policy(self.ctx._h, {"tile": 0, "block": 1, "auto": 2}[policy]))

    def last_state(self, d_final_T, d_n_contrib):
        """lcgs_debug_last_state: per pixel, what the last keep_state frame kept for its backward (final transmittance; 1-based
        list position of the last contributor).  Either argument may be None."""
        _check(load_library().lcgs_debug_last_state(self.ctx._h, _ptr(d_final_T), _ptr(d_n_contrib)))

    def adam_step(self, grads: dict, raw: dict, m: dict, v: dict, activated: dict, step: int, lr: dict,
                  betas=(0.9, 0.999), eps: float = 1e-15, visible_only: bool = False, sh_degree: int = 3,
                  compact_grads: bool = False):
        """lcgs_adam_step: gradients w.r.t. the activated values -> Adam on the raw parameters -> refreshed activated
        arrays.  Every dict has the keys pos / scale / rotq / sh / opacity (device tensors); lr has pos, sh_dc,
        sh_rest, opacity, scale, rot.  compact_grads (with visible_only): `grads` hold backward(compact=True) rows."""
        if compact_grads and not visible_only:
            raise ValueError("compact gradient rows only exist for the on-screen splats: visible_only must be set")
        P = int(raw["pos"].shape[0])
        cfg = _adam_config(lr, betas, eps, step, (2 if compact_grads else 1) if visible_only else 0)
        g, packs = _grads(grads), _params(raw, m, v, activated)
        _check(load_library().lcgs_adam_step(self.ctx._h, P, sh_degree, C.byref(cfg), C.byref(g), *map(C.byref, packs)))

    def backward_adam(self, dL_dimg, raw: dict, m: dict, v: dict, activated: dict, step: int, lr: dict,
                      betas=(0.9, 0.999), eps: float = 1e-15, sh_degree: int = 3):
        """lcgs_render_backward_adam: the backward of the last keep_state frame with the on-screen-only Adam update applied
        where the per-splat gradients are formed -- no gradient arrays (= backward(compact=True) + adam_step(visible_only,
        compact_grads), bit for bit)."""
        P = int(raw["pos"].shape[0])
        cfg, packs = _adam_config(lr, betas, eps, step, 2), _params(raw, m, v, activated)
        _check(load_library().lcgs_render_backward_adam(self.ctx._h, _ptr(dL_dimg), P, sh_degree, C.byref(cfg),
                                                        *map(C.byref, packs)))

    # ---- adaptive density control
    def densify_accumulate(self, stats: dict):
        """lcgs_densify_accumulate: the last keep_state frame and its backward -> stats["grad_accum"] (float32), ["denom"]
        (int32 bits of a uint32 count), ["max_radii"] (int32), device tensors of P entries, on-screen rows only."""
        st = _densify_stats(stats)
        _check(load_library().lcgs_densify_accumulate(self.ctx._h, int(stats["denom"].shape[0]), C.byref(st)))

    def absgrad_accumulate(self, dL_dimg=None, dL_ddepth=None, dL_dalpha=None, mode: str = "z", stats: Optional[dict] = None,
                           absgrad=None):
        """lcgs_absgrad_accumulate: the AbsGS statistic of the last keep_state frame -- per on-screen row the sum over pixels of
        the absolute per-pixel gradient of the pixel-space mean of <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha> (any
        gradient may be None, not all; mode as in render_maps).  stats: densify_accumulate's dict, grad_accum += the norm of the
        sums in NDC units, denom and max_radii as densify_accumulate; absgrad: float32 [P, 2], the sums ADDED in pixel units
        (gsplat's means2d.absgrad).  Either output may be None, not both.  Needs no backward and disturbs none; only enqueues."""
        st = None if stats is None else _densify_stats(stats)
        rows = int(stats["denom"].shape[0]) if stats is not None else (int(absgrad.numel()) // 2 if absgrad is not None else 0)
        _check(load_library().lcgs_absgrad_accumulate(self.ctx._h, rows, _ptr(dL_dimg), _DEPTH_MODES[mode], _ptr(dL_ddepth),
                                                      _ptr(dL_dalpha), None if st is None else C.byref(st), _ptr(absgrad)))

    def densify(self, stats: dict, raw: dict, m: dict, v: dict, out_raw: dict, out_m: dict, out_v: dict, out_activated: dict,
                out_stats: dict, grad_threshold: float = 2e-4, percent_dense: float = 0.01, scene_extent: float = 1.0,
                min_opacity: float = 0.005, max_screen_size: int = 0, seed: int = 0, noise=None, src_row=None,
                sh_degree: int = 3, capacity: Optional[int] = None) -> int:
        """lcgs_densify: clone / split / prune `raw` with its Adam moments into the out_* arrays (out of place, source order kept,
        new rows beside their parents) -> the new row count.  Dicts as in adam_step; the out_* tensors hold `capacity` rows
        (default: out_raw["opacity"]'s length).  noise: [P, 2, 3] normals for the split children, None: the built-in sampler
        keyed by seed.  src_row: optional int32 [capacity], output row -> source row.  Raises LcgsError (status 5, .needed = rows)
        when the rewrite does not fit; nothing is written then.  Rebind out_activated and render a synchronising frame next."""
        P = int(raw["opacity"].shape[0])
        cap = int(out_raw["opacity"].shape[0]) if capacity is None else int(capacity)
        cfg = _DensifyConfig(grad_threshold, percent_dense, scene_extent, min_opacity, int(max_screen_size), int(seed))
        packs = _params(raw, m, v, out_raw, out_m, out_v, out_activated)
        st, out_st = _densify_stats(stats), _densify_stats(out_stats)
        n = C.c_int64(0)
        try:
            _check(load_library().lcgs_densify(self.ctx._h, P, sh_degree, C.byref(cfg), C.byref(st), *map(C.byref, packs),
                                               C.byref(out_st), cap, _ptr(noise), _ptr(src_row), C.byref(n)))
        except LcgsError as err:
            err.needed = int(n.value)
            raise
        return int(n.value)

    # ---- contribution-based pruning
    def contrib_accumulate(self, stats: dict):
        """lcgs_contrib_accumulate: the last keep_state frame -> stats["weight_sum"], ["weight_max"] (float32), ["pixels"],
        ["views"] (int32 bits of uint32 counts), device tensors of P entries zeroed by the caller; any key may be missing, not
        all.  Only rows some pixel blended are touched.  Needs no backward; only enqueues."""
        st = _contrib_stats(stats)
        _check(load_library().lcgs_contrib_accumulate(self.ctx._h, _contrib_rows(stats), C.byref(st)))

    def contrib_keep_mask(self, stats: dict, keep, **minimums):
        """lcgs_contrib_keep_mask: keep[i] (uint8 device tensor of P entries) = 1 iff row i meets every given minimum
        (min_weight_max, min_weight_sum, min_pixels, min_views; 0 or absent: not tested)."""
        cfg, st = _prune_config(**minimums), _contrib_stats(stats)
        _check(load_library().lcgs_contrib_keep_mask(self.ctx._h, int(keep.shape[0]), C.byref(cfg), C.byref(st), _ptr(keep)))

    def prune(self, stats: dict, raw: dict, m: dict, v: dict, out_raw: dict, out_m: dict, out_v: dict, out_activated: dict,
              src_row=None, sh_degree: int = 3, capacity: Optional[int] = None, **minimums) -> int:
        """lcgs_prune: the rows of `raw` (with their Adam moments) that meet every given minimum (as in contrib_keep_mask), into
        the out_* arrays -- out of place, source order kept, bit for bit -> the new row count.  Dicts as in densify; src_row:
        optional int32 [capacity], output row -> source row.  Raises LcgsError (status 5, .needed = rows) when the kept rows do
        not fit; nothing is written then.  Rebind out_activated and render a synchronising frame next."""
        P = int(raw["opacity"].shape[0])
        cap = int(out_raw["opacity"].shape[0]) if capacity is None else int(capacity)
        cfg, st = _prune_config(**minimums), _contrib_stats(stats)
        packs = _params(raw, m, v, out_raw, out_m, out_v, out_activated)
        n = C.c_int64(0)
        try:
            _check(load_library().lcgs_prune(self.ctx._h, P, sh_degree, C.byref(cfg), C.byref(st), *map(C.byref, packs), cap,
                                             _ptr(src_row), C.byref(n)))
        except LcgsError as err:
            err.needed = int(n.value)
            raise
        return int(n.value)

    def opacity_reset(self, raw: dict, m: dict, v: dict, activated: dict, max_opacity: float = 0.01):
        """lcgs_opacity_reset: raw opacity = min(raw opacity, logit(max_opacity)), its moments zeroed, activated opacity
        rewritten.  Only the "opacity" entries of the dicts are needed."""
        P = int(raw["opacity"].shape[0])
        packs = _params(raw, m, v, activated, partial=True)
        _check(load_library().lcgs_opacity_reset(self.ctx._h, P, max_opacity, *map(C.byref, packs)))

    # ---- 3DGS-MCMC density control
    def mcmc_relocate(self, raw: dict, m: dict, v: dict, activated: dict, min_opacity: float = 0.005, n_max: int = 51,
                      seed: int = 0, src_in=None, src_row=None, sh_degree: int = 3) -> int:
        """lcgs_mcmc_relocate: every dead row (opacity <= min_opacity) becomes a copy of a live row drawn with probability
        proportional to opacity; source and copies get the corrected opacity and scale, zero Adam moments -> rows relocated.  In
        place; dicts as in adam_step.  src_in: optional int32 [#dead] sources instead of the built-in sampler keyed by seed.
        src_row: optional int32 [P], the source of a relocated row, its own index otherwise.  Synchronises once.  Rebind (or
        scene_modified) before the next frame."""
        P = int(raw["opacity"].shape[0])
        cfg, packs, n = _McmcConfig(min_opacity, int(n_max), int(seed)), _params(raw, m, v, activated), C.c_int64(0)
        _check(load_library().lcgs_mcmc_relocate(self.ctx._h, P, sh_degree, C.byref(cfg), *map(C.byref, packs), _ptr(src_in),
                                                 _ptr(src_row), C.byref(n)))
        return int(n.value)

    def mcmc_add(self, num_gaussians: int, num_new: int, raw: dict, m: dict, v: dict, activated: dict, min_opacity: float = 0.005,
                 n_max: int = 51, seed: int = 0, src_in=None, src_row=None, sh_degree: int = 3, capacity: Optional[int] = None):
        """lcgs_mcmc_add: rows [num_gaussians, num_gaussians + num_new) of the tensors (which hold `capacity` rows, default
        raw["opacity"]'s length) become copies of live rows among the first num_gaussians, drawn and corrected as in
        mcmc_relocate.  src_in / src_row: optional int32 [num_new].  Raises LcgsError: status 5 when the rows do not fit (nothing
        is touched), 8 when no row is live, 1 for a bad entry of src_in."""
        cap = int(raw["opacity"].shape[0]) if capacity is None else int(capacity)
        cfg, packs = _McmcConfig(min_opacity, int(n_max), int(seed)), _params(raw, m, v, activated)
        _check(load_library().lcgs_mcmc_add(self.ctx._h, int(num_gaussians), sh_degree, C.byref(cfg), *map(C.byref, packs),
                                            int(num_new), cap, _ptr(src_in), _ptr(src_row)))

    def mcmc_noise(self, raw: dict, activated: dict, lr_pos: float, step: int, noise_lr: float = 5e5, k: float = 100.0,
                   x0: float = 0.995, seed: int = 0, noise=None):
        """lcgs_mcmc_noise: pos += (noise_lr lr_pos g(opacity)) Sigma eps in place on raw["pos"] (and activated["pos"] when it is
        another tensor); g is ~0 for opaque splats.  noise: optional [P, 3] normals, None: the built-in sampler keyed by
        (seed, row, step).  Needs raw pos / scale / rotq / opacity and activated pos.  Only enqueues."""
        P = int(raw["opacity"].shape[0])
        cfg = _McmcNoiseConfig(noise_lr, lr_pos, k, x0, int(seed), int(step))
        packs = _params(raw, activated, partial=True)
        _check(load_library().lcgs_mcmc_noise(self.ctx._h, P, C.byref(cfg), *map(C.byref, packs), _ptr(noise)))

    def mcmc_regularize(self, grads: dict, lambda_opacity: float = 0.01, lambda_scale: float = 0.01):
        """lcgs_mcmc_regularize: grads["opacity"] += lambda_opacity / P, grads["scale"] += lambda_scale / (3 P) -- the gradients of
        lambda_opacity mean(opacity) + lambda_scale mean(scale) w.r.t. the activated values; call it before adam_step (whose
        on-screen-only mode then applies it to on-screen rows only).  Only enqueues."""
        P = int(grads["opacity"].shape[0])
        g = _Grads(None, _ptr(grads["scale"]), None, None, _ptr(grads["opacity"]))
        _check(load_library().lcgs_mcmc_regularize(self.ctx._h, P, lambda_opacity, lambda_scale, C.byref(g)))

    # ---- Mip-Splatting's 3-D smoothing filter
    def filter3d_accumulate(self, pos, cams, min_z, max_focal: float = 0.0) -> float:
        """lcgs_filter3d_accumulate: min_z[i] = min(min_z[i], view depth of row i) over the views of `cams` (a sequence of Camera)
        that see the row -- depth > 0.2 and inside 1.3 x the view's frustum, Mip-Splatting's rule.  pos [P, 3] and min_z [P]
        (start it at +inf) are device tensors; returns max(max_focal, the views' focal lengths in pixels) for the next call /
        filter3d_finalize.  Only enqueues."""
        cams = list(cams)
        arr = (Camera * len(cams))(*cams) if cams else None
        focal = C.c_float(max_focal)
        _check(load_library().lcgs_filter3d_accumulate(self.ctx._h, int(min_z.shape[0]), _ptr(pos), len(cams), arr, _ptr(min_z),
                                                       C.byref(focal)))
        return float(focal.value)

    def filter3d_finalize(self, min_z, max_focal: float, filt):
        """lcgs_filter3d_finalize: filt[i] = (min_z[i] / max_focal) * sqrt(0.2), a row no view saw taking the largest finite
        min_z; all zeros (the identity filter) when no row was seen.  Only enqueues, no read-back."""
        _check(load_library().lcgs_filter3d_finalize(self.ctx._h, int(min_z.shape[0]), _ptr(min_z), max_focal, _ptr(filt)))

    def filter3d_apply(self, scale, opacity, filt, scale_out, opacity_out):
        """lcgs_filter3d_apply: scale_out = sqrt(scale^2 + filt^2), opacity_out = opacity * sqrt(prod_k scale_k^2 / (scale_k^2 +
        filt^2)) from ACTIVATED scale [P, 3] / opacity [P]; rows with filt == 0 are copied.  Out of place (aliased outputs are
        refused); a context bound to scale_out rebuilds its derived rows.  Only enqueues."""
        _check(load_library().lcgs_filter3d_apply(self.ctx._h, int(opacity.shape[0]), _ptr(scale), _ptr(opacity), _ptr(filt),
                                                  _ptr(scale_out), _ptr(opacity_out)))

    def filter3d_backward(self, scale, opacity, filt, dscale, dopacity, rows=None, count=None):
        """lcgs_filter3d_backward: dscale / dopacity, gradients w.r.t. the FILTERED scale and opacity, become gradients w.r.t. the
        unfiltered activated values (what adam_step takes), in place.  rows / count (device int32 tensors or addresses, as
        lcgs_visible_rows gives them): gradient row r < count[0] belongs to row rows[r] -- the compact rows of
        backward(compact=True); None: dense rows.  Only enqueues."""
        _check(load_library().lcgs_filter3d_backward(self.ctx._h, int(opacity.shape[0]), _ptr(scale), _ptr(opacity), _ptr(filt),
                                                     _ptr(rows), _ptr(count), _ptr(dscale), _ptr(dopacity)))

    # ---- scene similarity transforms
    def scene_transform(self, xf: Similarity, src: dict, dst: Optional[dict] = None, sh_degree: Optional[int] = None):
        """lcgs_scene_transform: the ACTIVATED arrays of `src` (device tensors under pos / scale / rotq / sh / opacity) moved by
        new = scale rot old + trans into `dst` -- positions, scales, orientations, and the SH bands rotated with the scene.  dst
        None: in place on every array src holds; otherwise every array dst holds is written (the same tensor as in src, or a
        disjoint one) and the others are skipped -- {"sh": t} rotates the colours only.  One defined bit pattern per output.  A
        context whose bound scene is written drops its derived rows, its f16 coefficients and its kept frame.  Only enqueues."""
        dst = src if dst is None else dst
        ref = src.get("opacity", src.get("pos", src.get("rotq")))
        P = int(ref.shape[0]) if ref is not None else int(next(iter(src.values())).shape[0])
        if sh_degree is None:
            sh_degree = {3: 0, 12: 1, 27: 2, 48: 3}[int(src["sh"].numel()) // max(P, 1)] if "sh" in src and P else 3
        i, o = _params(src, dst, partial=True)
        _check(load_library().lcgs_scene_transform(self.ctx._h, P, sh_degree, C.byref(xf), C.byref(i), C.byref(o)))

    def scene_box_keep_mask(self, pos, world_to_box: Similarity, half_extent, keep):
        """lcgs_scene_box_keep_mask: keep[i] (uint8 device tensor [P]) = 1 iff row i of pos [P, 3], taken into the box's frame by
        world_to_box, lies within half_extent on all three axes (faces included; +inf: unbounded; NaN positions dropped) -- the
        bytes ply_filter_rows takes after a copy to the host.  Only enqueues."""
        _check(load_library().lcgs_scene_box_keep_mask(self.ctx._h, int(pos.shape[0]), _ptr(pos), C.byref(world_to_box),
                                                       _f3(half_extent), _ptr(keep)))

    # ---- a surface out of the scene: TSDF fusion of depth maps, marching tetrahedra
    def tsdf_integrate(self, volume: "TsdfVolume", cams, depths, alphas=None, images=None, trunc: Optional[float] = None,
                       depth_max: float = 1e4, alpha_min: float = 0.5):
        """lcgs_tsdf_integrate: fuses the views `cams` (a sequence of Camera) into `volume`, in order -- depths[v] [H, W] the
        accumulated view z of render_maps (divided by alphas[v] where given; pixels with alpha < alpha_min are skipped), images[v]
        [3, H, W] the colours of a volume with rgb.  alphas / images: None, or sequences that may hold None.  trunc: the truncation
        distance (default: 4 voxels).  Curless & Levoy's running mean, nearest-pixel lookup; a batch leaves the bits of the same
        views passed one call at a time.  Only enqueues."""
        cams, n = list(cams), len(cams)
        assert len(depths) == n and (alphas is None or len(alphas) == n) and (images is None or len(images) == n)
        for k, c in enumerate(cams):
            assert int(depths[k].numel()) == c.width * c.height, f"depth map {k} is not {c.height} x {c.width}"

        def table(maps):
            return None if maps is None else (C.c_void_p * max(n, 1))(*[_ptr(m) for m in maps])

        cfg = _TsdfConfig(4.0 * volume.voxel_size if trunc is None else trunc, depth_max, alpha_min)
        vol = volume._struct()
        _check(load_library().lcgs_tsdf_integrate(self.ctx._h, C.byref(vol), C.byref(cfg), n, (Camera * max(n, 1))(*cams), table(depths),
                                                  table(alphas), table(images)))

    def tsdf_mesh_count(self, volume: "TsdfVolume", weight_min: float = 1.0):
        """lcgs_tsdf_mesh_count: (vertices, triangles) of the mesh tsdf_mesh would return.  Synchronises once."""
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        vol = volume._struct()
        _check(load_library().lcgs_tsdf_mesh_count(self.ctx._h, C.byref(vol), weight_min, C.addressof(nv), C.addressof(nt)))
        return int(nv.value), int(nt.value)

    def tsdf_mesh(self, volume: "TsdfVolume", weight_min: float = 1.0):
        """lcgs_tsdf_mesh_count + lcgs_tsdf_mesh_extract: the zero level set of `volume` over the cells whose 8 samples all have
        weight >= weight_min, by marching tetrahedra -- (vertices [V, 3] float32, rgb [V, 3] float32 or None, triangles [T, 3]
        int64 holding the 32-bit indices), device tensors; welded, consistently oriented (normals point from inside to outside),
        deterministic."""
        import torch

        nv, nt = self.tsdf_mesh_count(volume, weight_min)
        dev = volume.tsdf.device
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((nv, 3), dtype=torch.float32, device=dev) if volume.rgb is not None else None
        tri = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        got_v, got_t = C.c_uint64(0), C.c_uint64(0)
        vol = volume._struct()
        _check(load_library().lcgs_tsdf_mesh_extract(self.ctx._h, C.byref(vol), weight_min, nv, nt, _ptr(vertices), _ptr(rgb), _ptr(tri),
                                                     C.addressof(got_v), C.addressof(got_t)))
        assert (got_v.value, got_t.value) == (nv, nt)
        return vertices, rgb, tri.to(torch.int64) & 0xFFFFFFFF

    # ---- a scene from a point cloud
    def init_from_points(self, pos, rgb, sh_degree: int = 3, initial_opacity: float = 0.1, min_dist2: float = 1e-7):
        """lcgs_scene_init_from_points, 3DGS's create_from_pcd: device tensors pos [n, 3] and rgb [n, 3] in [0, 1] -> (raw,
        activated), dicts of fresh device tensors keyed pos / scale / rotq / sh / opacity.  Scales come from the exact mean squared
        distance to the three nearest neighbours; activated pos / sh ARE raw's.  Nothing is bound; moments are the caller's."""
        import torch

        n, feat = int(pos.shape[0]), (sh_degree + 1) ** 2 * 3
        shapes = {"pos": (n, 3), "scale": (n, 3), "rotq": (n, 4), "sh": (n, feat), "opacity": (n,)}
        raw = {k: torch.empty(shp, dtype=torch.float32, device=pos.device) for k, shp in shapes.items()}
        act = {k: raw[k] if k in ("pos", "sh") else torch.empty_like(raw[k]) for k in _KEYS}
        self.init_from_points_into(pos, rgb, raw, act, sh_degree, initial_opacity, min_dist2)
        return raw, act

    def init_from_points_into(self, pos, rgb, raw: dict, activated: dict, sh_degree: int = 3, initial_opacity: float = 0.1,
                              min_dist2: float = 1e-7):
        """the same into the caller's arrays (dicts as in adam_step; activated pos / sh may be raw's or separate buffers)"""
        cfg = _InitConfig(initial_opacity, min_dist2)
        packs = _params(raw, activated)
        _check(load_library().lcgs_scene_init_from_points(self.ctx._h, int(pos.shape[0]), sh_degree, _ptr(pos), _ptr(rgb),
                                                          C.byref(cfg), *map(C.byref, packs)))


class TsdfVolume:
    """lcgs_tsdf_volume: a dense TSDF lattice of dims = (nx, ny, nz) samples, sample (i, j, k) at origin + voxel_size * (i, j, k);
    device tensors tsdf / weight [nz, ny, nx] and rgb [nz, ny, nx, 3] (or None), zeroed."""

    def __init__(self, origin, voxel_size: float, dims, rgb: bool = False, device="cuda:0"):
        import torch

        self.origin = tuple(float(x) for x in origin)
        self.voxel_size = float(voxel_size)
        self.dims = tuple(int(x) for x in dims)
        nx, ny, nz = self.dims
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.rgb = torch.zeros((nz, ny, nx, 3), dtype=torch.float32, device=device) if rgb else None

    @classmethod
    def from_tensors(cls, origin, voxel_size: float, dims, tsdf, weight, rgb=None) -> "TsdfVolume":
        """a volume over the caller's contiguous device tensors (nx ny nz floats each, rgb three per sample), left as they are"""
        self = cls.__new__(cls)
        self.origin, self.voxel_size, self.dims = tuple(float(x) for x in origin), float(voxel_size), tuple(int(x) for x in dims)
        n = self.dims[0] * self.dims[1] * self.dims[2]
        assert tsdf.numel() == n and weight.numel() == n and (rgb is None or rgb.numel() == 3 * n)
        self.tsdf, self.weight, self.rgb = tsdf, weight, rgb
        return self

    def zero_(self):
        for t in (self.tsdf, self.weight, self.rgb):
            if t is not None:
                t.zero_()
        return self

    def _struct(self) -> _TsdfVolume:
        return _TsdfVolume(_f3(self.origin), self.voxel_size, *self.dims, _ptr(self.tsdf).value, _ptr(self.weight).value,
                           _ptr(self.rgb).value)


def write_mesh_ply(path: str, vertices, triangles, rgb=None):
    """lcgs_mesh_write_ply: a binary PLY of vertices [V, 3], optional rgb [V, 3] in [0, 1] (written as uchar) and triangles
    [T, 3]; tensors (copied to the host) or arrays"""
    host = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=dt)
    v, t = host(vertices, np.float32).reshape(-1, 3), host(triangles, np.uint32).reshape(-1, 3)
    c = None if rgb is None else host(rgb, np.float32).reshape(-1, 3)
    assert c is None or c.shape == v.shape
    _check(load_library().lcgs_mesh_write_ply(os.fsencode(path), v.shape[0], _ptr(v), _ptr(c), t.shape[0], _ptr(t)))


def knn_mean_dist2(ctx: Context, pos):
    """lcgs_knn_mean_dist2: device tensor pos [n, 3] float32 -> device tensor [n], the mean squared distance of every point to
    its three nearest neighbours (exact in binary32, independent of the order of the points; include/lcgs_hip.h has the definition)"""
    import torch

    out = torch.empty(int(pos.shape[0]), dtype=torch.float32, device=pos.device)
    _check(load_library().lcgs_knn_mean_dist2(ctx._h, int(pos.shape[0]), _ptr(pos), _ptr(out)))
    return out


def scene_extent(cameras):
    """lcgs_scene_extent, 3DGS's getNerfppNorm: (center float32 [3], radius) of a list of Camera -- radius is what
    Renderer.densify takes as scene_extent"""
    n = len(cameras)
    center, radius = np.zeros(3, np.float32), np.zeros(1, np.float32)
    _check(load_library().lcgs_scene_extent(n, (Camera * max(n, 1))(*cameras), _ptr(center), _ptr(radius)))
    return center, float(radius[0])


def mcmc_num_new(P: int, cap_max: int, growth: float = 1.05) -> int:
    """3DGS-MCMC's growth step: the rows Renderer.mcmc_add appends to a scene of P rows -- 5 % at a time up to cap_max"""
    return max(0, min(int(cap_max), int(growth * P)) - int(P))


def read_points_ply(path: str) -> dict:
    """lcgs_points_read_ply: a point-cloud PLY (x y z, red green blue) -> {"pos": float32 [n, 3], "rgb": float32 [n, 3] in [0, 1]}"""
    lib = load_library()
    n, pos, rgb = C.c_int64(0), C.c_void_p(), C.c_void_p()
    _check(lib.lcgs_points_read_ply(path.encode(), C.byref(n), C.byref(pos), C.byref(rgb)))
    try:
        def grab(p):
            if n.value == 0:
                return np.zeros((0, 3), np.float32)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value * 3,)).reshape(n.value, 3).copy()

        return {"pos": grab(pos), "rgb": grab(rgb)}
    finally:
        lib.lcgs_points_free(pos, rgb)


def _rows(fn, num_gaussians: int, world_size: int, rank: int):
    first, count = C.c_int64(0), C.c_int64(0)
    fn(num_gaussians, world_size, rank, C.byref(first), C.byref(count))
    return first.value, count.value


def shard_rows(num_gaussians: int, world_size: int, rank: int):
    """lcgs_comm_shard_rows: (first, count) of the rows rank `rank` owns in the sharded optimiser step; the last
    num_gaussians mod world_size rows (the tail) are kept by every rank.  Pure host arithmetic (no GPU needed)."""
    return _rows(load_library().lcgs_comm_shard_rows, num_gaussians, world_size, rank)


def owner_rows(num_gaussians: int, world_size: int, rank: int):
    """lcgs_comm_owner_rows: (first, count) of the rows a rank OWNS in the ownership step (the tail with the last rank)"""
    return _rows(load_library().lcgs_comm_owner_rows, num_gaussians, world_size, rank)


class LoopbackGroup:
    """lcgs_loopback_group: the rendezvous of N in-process communicators (N contexts on ONE device, one host thread each) --
    the ownership step's C code path with N > 1 participants on a single GPU.  Tests and rehearsals only."""

    def __init__(self, world_size: int):
        self.world_size = world_size
        self._h = C.c_void_p(0)
        _check(load_library().lcgs_loopback_group_create(world_size, C.byref(self._h)))

    def close(self):
        if self._h:
            _check(load_library().lcgs_loopback_group_destroy(self._h))
            self._h = C.c_void_p(0)


class Comm:
    """lcgs_comm: the RCCL communicator of a view-parallel job, attached to one context.

    `exchange(payload: bytes | None) -> bytes` carries the 128-byte rendezvous token from rank 0 (which passes it in)
    to every other rank (which pass None): any broadcast the host has (torch.distributed, a pipe, a file)."""

    def __init__(self, ctx: Context, rank: int, world_size: int, exchange=None, loopback: "LoopbackGroup" = None):
        lib = load_library()
        if loopback is not None:  # an in-process communicator: N contexts on one device, one host thread each
            self.ctx, self.rank, self.world_size = ctx, rank, loopback.world_size
            self._h = C.c_void_p(0)
            _check(lib.lcgs_comm_create_loopback(ctx._h, loopback._h, rank, C.byref(self._h)))
            return
        token = (C.c_char * 128)()
        if rank == 0:
            _check(lib.lcgs_comm_unique_id(token))
        if world_size > 1 or exchange is not None:
            if exchange is None:
                raise ValueError("world_size > 1 needs an exchange function for the rendezvous token")
            got = exchange(bytes(token.raw) if rank == 0 else None)
            assert len(got) == 128
            C.memmove(token, got, 128)
        self.ctx, self.rank, self.world_size = ctx, rank, world_size
        self._h = C.c_void_p(0)
        _check(lib.lcgs_comm_create(ctx._h, token, rank, world_size, C.byref(self._h)))

    def close(self):
        if self._h:
            load_library().lcgs_comm_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def abandon(self):
        """forget the handle WITHOUT destroying the communicator: for one whose self-test left a phase stuck inside RCCL
        (lcgs_comm_destroy would wait for its stream, i.e. for ever) -- the process is expected to report and exit"""
        self._h = C.c_void_p(0)

    def info(self):
        """lcgs_comm_info: (rank, world_size) as the communicator itself -- i.e. RCCL -- sees them"""
        rk, ws = C.c_int(-1), C.c_int(-1)
        _check(load_library().lcgs_comm_info(self._h, C.byref(rk), C.byref(ws)))
        return int(rk.value), int(ws.value)

    def owner_step_forward(self, cams, img, bg=(0.0, 0.0, 0.0), scale_modifier: float = 1.0):
        """lcgs_owner_step_forward: the ownership step's first half with its transport -- this rank's rows projected for every
        view, records exchanged (RCCL send / recv, or the loopback), this rank's view rendered into img"""
        arr = (Camera * len(cams))(*cams)
        _check(load_library().lcgs_owner_step_forward(self.ctx._h, self._h, arr, _f3(bg), scale_modifier, _ptr(img)))

    def owner_step_backward(self, dL_dimg, grads: dict):
        """lcgs_owner_step_backward: the view's 2-D gradients back to the owners, parameter gradients at this rank's own rows"""
        g = _grads(grads)
        _check(load_library().lcgs_owner_step_backward(self.ctx._h, self._h, _ptr(dL_dimg), C.byref(g)))

    def selftest(self, timeout_s: float = 30.0, check: bool = True) -> dict:
        """lcgs_comm_selftest (a collective: every rank calls it): a 1 KB all-reduce, zero- and one-byte messages to every peer
        in one group, an ownership step on a 10 000-splat scene with and without read-back -- each phase against timeout_s.
        Returns the report as a dict (`ok`, per-phase `*_ok` / `*_ms`, `timed_out`, `message`); check=True raises on failure."""
        rep = _SelftestReport()
        status = load_library().lcgs_comm_selftest(self.ctx._h, self._h, timeout_s, C.byref(rep))
        out = {"ok": status == 0, "world_size": int(rep.world_size), "rank": int(rep.rank),
               "allreduce_ok": int(rep.allreduce_ok), "allreduce_ms": round(float(rep.allreduce_ms), 3),
               "p2p_ok": int(rep.p2p_ok), "p2p_ms": round(float(rep.p2p_ms), 3),
               "owner_step_ok": int(rep.owner_step_ok), "owner_step_ms": round(float(rep.owner_step_ms), 3),
               "owner_max_grad_err": float(rep.owner_max_grad_err), "timed_out": int(rep.timed_out),
               "message": rep.message.decode(errors="replace")}
        if check:
            _check(status)
        return out

    def owner_step_set_async(self, enable: bool = True):
        """lcgs_owner_step_set_async: steps size their messages from the previous step's counts and read nothing back; every
        such step must be closed with owner_step_finish()"""
        _check(load_library().lcgs_owner_step_set_async(self._h, bool(enable)))

    def owner_step_finish(self) -> bool:
        """lcgs_owner_step_finish: True = some rank's step was short (a clipped message, truncated pairs): EVERY rank calls
        forward + backward again"""
        redo = C.c_int(0)
        _check(load_library().lcgs_owner_step_finish(self.ctx._h, self._h, C.byref(redo)))
        return bool(redo.value)

    def owner_step(self, cams, img, dL_dimg, grads: dict, bg=(0.0, 0.0, 0.0), scale_modifier: float = 1.0) -> int:
        """forward + backward + finish, repeated while the step was short; returns the number of repetitions (0 normally)"""
        for attempt in range(3):
            self.owner_step_forward(cams, img, bg, scale_modifier)
            self.owner_step_backward(dL_dimg, grads)
            if not self.owner_step_finish():
                return attempt
        raise LcgsError(LCGS_ERR_STATE, "the ownership step did not settle after two repetitions")

    def set_transport(self, transport: str):
        """lcgs_comm_set_transport: "f32" (default, exact) or "f16" (opt-in: half the bytes, ~sqrt(N) x 5e-4 relative)"""
        _check(load_library().lcgs_comm_set_transport(self._h, {"f32": 0, "f16": 1}[transport]))

    def allreduce_grads(self, grads: dict, sh_degree: int = 3):
        """lcgs_grads_allreduce: in-place sum over the ranks of the five dense gradient arrays (chunked, overlapping the
        backward's tail); the context's stream waits for the result."""
        P = int(grads["pos"].shape[0])
        g = _grads(grads)
        _check(load_library().lcgs_grads_allreduce(self.ctx._h, self._h, P, sh_degree, C.byref(g)))

    def _adam_step(self, fn, grads, raw, m, v, activated, step, lr, betas, eps, sh_degree):
        P = int(raw["pos"].shape[0])
        cfg, g, packs = _adam_config(lr, betas, eps, step, 0), _grads(grads), _params(raw, m, v, activated)
        _check(fn(self.ctx._h, self._h, P, sh_degree, C.byref(cfg), C.byref(g), *map(C.byref, packs)))

    def adam_step_sharded(self, grads: dict, raw: dict, m: dict, v: dict, activated: dict, step: int, lr: dict,
                          betas=(0.9, 0.999), eps: float = 1e-15, sh_degree: int = 3):
        """lcgs_adam_step_sharded: reduce-scatter -> Adam on the own rows (+ tail) -> all-gather of the activated arrays."""
        self._adam_step(load_library().lcgs_adam_step_sharded, grads, raw, m, v, activated, step, lr, betas, eps, sh_degree)

    # ---- sparse gradient exchange (lcgs_hip.h "Sparse gradient exchange")
    def track_touched_rows(self, enable: bool = True):
        """lcgs_comm_track_touched_rows: dense backward passes on this context flag the rows their frame touched"""
        _check(load_library().lcgs_comm_track_touched_rows(self._h, bool(enable)))

    def stats(self) -> dict:
        """lcgs_comm_get_stats: what the last collective call of this communicator moved (per GPU, from actual counts)"""
        st = _CommStats()
        _check(load_library().lcgs_comm_get_stats(self._h, C.byref(st)))
        return {"bytes_sent": int(st.bytes_sent), "bytes_received": int(st.bytes_received),
                "touched_rows": int(st.touched_rows), "collective_groups": int(st.collective_groups)}

    def adam_step_sparse(self, grads: dict, raw: dict, m: dict, v: dict, activated: dict, step: int, lr: dict,
                         betas=(0.9, 0.999), eps: float = 1e-15, sh_degree: int = 3):
        """lcgs_adam_step_sparse: touched rows -> their owners (send / recv) -> Adam on the own rows -> all-gather"""
        self._adam_step(load_library().lcgs_adam_step_sparse, grads, raw, m, v, activated, step, lr, betas, eps, sh_degree)

    def sparse_touched_rows(self, num_gaussians: int, world_size: Optional[int] = None):
        """lcgs_sparse_touched_rows -> (device address of the ascending row list, owner_first[0 .. N + 1]) for an exchange
        over `world_size` ranks (default: the communicator's own); consumes the step's touched set and synchronises"""
        n = self.world_size if world_size is None else world_size
        out = _SparseRows()
        _check(load_library().lcgs_sparse_touched_rows(self.ctx._h, self._h, num_gaussians, n, C.byref(out)))
        return int(out.d_rows or 0), [int(out.owner_first[i]) for i in range(n + 2)]

    def sparse_pack(self, grads: dict, rows_addr: int, first: int, count: int, msg, sh_degree: int = 3):
        """lcgs_sparse_pack: rows [first, first + count) of the touched list -> one message (a float32 tensor of
        sparse_message_words(count) elements)"""
        g = _grads(grads)
        _check(load_library().lcgs_sparse_pack(self.ctx._h, sh_degree, C.byref(g), rows_addr + 4 * first, count, _ptr(msg)))

    def sparse_accumulate(self, grads: dict, msg, count: int, sh_degree: int = 3, row_first: int = 0, row_count: int = -1):
        """lcgs_sparse_accumulate: add a received message's rows to the dense gradient rows; only rows in
        [row_first, row_first + row_count) are accepted (default: every row of the arrays)"""
        g = _grads(grads)
        if row_count < 0:
            row_first, row_count = 0, int(grads["pos"].shape[0])
        _check(load_library().lcgs_sparse_accumulate(self.ctx._h, sh_degree, C.byref(g), _ptr(msg), count, row_first,
                                                     row_count))


def sparse_message_words(count: int, sh_degree: int = 3) -> int:
    """4-byte words of a sparse-exchange message of `count` rows: indices + the five attribute blocks"""
    return count * (1 + 3 + 3 + 4 + (sh_degree + 1) ** 2 * 3 + 1)


def _autograd_frame(renderer: "Renderer", view: Camera, scene, bg, scale_modifier: float, outputs: str = "image",
                    depth_mode: str = "z", center: float = 0.0, cam12=None, features=None):
    """The one differentiable frame behind render_autograd and its variants: binds the scene, renders `view` with keep_state,
    renders the maps `outputs` asks for ("image": the image alone; "maps": plus depth and alpha; "distortion": plus the
    distortion map about `center`; "normals": plus the normal map; "features": the image, alpha and the blended map of the
    caller's `features` rows, a sixth differentiable input behind the five scene tensors) and, on backward, differentiates that frame -- after binding its saved scene and rendering
    its view again when the renderer's generation has moved -- through the one Renderer backward that fits.  cam12 (a tensor
    or None): the pose is an input too, in front of the five scene tensors, and gets the camera gradient."""
    import torch

    feats = outputs == "features"
    maps, dist, nrm, pose = outputs not in ("image", "features"), outputs in ("distortion", "normals"), outputs == "normals", cam12 is not None

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *inputs):
            params = inputs[1:] if pose else inputs
            args = [t.detach().contiguous() for t in params]
            renderer.bind_scene(*args[:5])
            dev = args[0].device
            img = torch.empty(3, view.height, view.width, device=dev, dtype=torch.float32)
            extra = [torch.empty(view.height, view.width, device=dev, dtype=torch.float32) for _ in range(3 if dist else 2 if maps else 0)]
            n = renderer.forward(view, img, bg=bg, scale_modifier=scale_modifier, keep_state=True, sync=True)
            if n == 0:
                img[:] = torch.tensor(bg, device=dev).view(3, 1, 1)  # nothing drawn: the image is the background
            if maps:
                renderer.render_maps(extra[0], extra[1], mode=depth_mode)
            if dist:
                renderer.render_distortion(extra[2], mode=depth_mode, center=center)
            if nrm:
                extra.append(torch.empty(3, view.height, view.width, device=dev, dtype=torch.float32))
                renderer.render_normals(extra[3])
            if feats:
                extra = [torch.empty(view.height, view.width, device=dev, dtype=torch.float32),
                         torch.empty(args[5].shape[1], view.height, view.width, device=dev, dtype=torch.float32)]
                renderer.render_maps(None, extra[0])
                renderer.render_features(args[5], extra[1])
            ctx.shapes = [t.shape for t in params]
            if pose:
                ctx.cam_like = (inputs[0].shape, inputs[0].device)
            ctx.empty = n == 0
            ctx.generation = renderer._generation
            ctx.save_for_backward(*args)
            if not maps and not feats:
                return img  # (its single gradient arrives materialised)
            ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None and is passed as NULL
            return (img, *extra)

        @staticmethod
        def backward(ctx, *incoming):
            args = ctx.saved_tensors
            want_cam = pose and ctx.needs_input_grad[0]
            want_scene = not pose or any(ctx.needs_input_grad[1:])
            g12 = torch.zeros(12, device=args[0].device, dtype=torch.float32) if pose else None
            grads = [torch.zeros_like(t) for t in args] if want_scene else None  # (the pose alone: no parameter rows)
            incoming = [None if g is None or g.numel() == 0 else g.contiguous() for g in incoming]
            if not ctx.empty and any(g is not None for g in incoming):
                if renderer._generation != ctx.generation:  # the renderer's frame state is no longer this frame's
                    renderer.bind_scene(*args[:5])
                    scratch = torch.empty(3, view.height, view.width, device=args[0].device, dtype=torch.float32)
                    renderer.forward(view, scratch, bg=bg, scale_modifier=scale_modifier, keep_state=True, sync=True)
                    ctx.generation = renderer._generation
                if feats:
                    gi, ga, gf = incoming
                    if gf is None:  # the feature map is not in the loss: no feature channel, dL/dfeatures stays zero
                        renderer.backward_maps(gi, None, ga, *grads[:5])
                    else:
                        renderer.backward_features(gi, None, ga, None, None, args[5], gf, grads[5], *grads[:5])
                elif not want_scene:
                    renderer.backward_camera(*incoming, g12, mode=depth_mode)
                elif nrm:
                    renderer.backward_normals(*incoming, *grads, mode=depth_mode, center=center)
                elif dist:
                    renderer.backward_distortion(*incoming, *grads, mode=depth_mode, center=center)
                elif maps:
                    renderer.backward_maps(*incoming, *grads, mode=depth_mode)
                else:
                    renderer.backward(*incoming, *grads)
                if want_scene and want_cam:
                    renderer.camera_backward(g12)
            out = tuple(g.view(s) for g, s in zip(grads, ctx.shapes)) if want_scene else (None,) * 5
            if pose:
                shape, dev = ctx.cam_like
                out = (g12.to(dev).view(shape) if want_cam else None,) + out
            return out

    return _Fn.apply(*((cam12,) if pose else ()), *scene, *((features,) if feats else ()))


def render_autograd(renderer: "Renderer", cam: Camera, pos, scale, rotq, sh, opacity, bg=(0.0, 0.0, 0.0),
                    scale_modifier: float = 1.0):
    """Differentiable frame for torch: `img = render_autograd(r, cam, pos, scale, rotq, sh, opacity)` (activated
    parameters, CHW float image); `img.backward(...)` / `torch.autograd.grad` run lcgs_render_backward.  torch is the
    owner of the tensors and of the autograd graph only; both directions are the HIP kernels.

    lcgs_render_backward differentiates the LAST keep_state frame of the context.  Several render_autograd frames of one
    renderer may be alive at once (a multi-view loss), or the renderer may have been used for something else between a
    frame's forward and its backward: the backward notices (the renderer's generation counter has moved), binds its own
    saved scene again and re-renders its own view with keep_state before differentiating -- the cost of one extra
    forward instead of gradients silently computed from another view's lists."""
    return _autograd_frame(renderer, cam, (pos, scale, rotq, sh, opacity), bg, scale_modifier)


def render_autograd_maps(renderer: "Renderer", cam: Camera, pos, scale, rotq, sh, opacity, bg=(0.0, 0.0, 0.0),
                         scale_modifier: float = 1.0, depth_mode: str = "z"):
    """render_autograd with the frame's depth and alpha maps: returns (img [3, H, W], depth [H, W], alpha [H, W]) as
    include/lcgs_hip.h defines them (accumulated depth of view z or, depth_mode="inv_z", of 1 / z; nothing normalised, no
    background in the maps).  The backward runs lcgs_render_backward_maps with the three incoming gradients; an output the loss
    does not use arrives as None (or zero-shaped) and is passed as NULL.  Like render_autograd it re-renders its own view
    when the renderer's generation has moved."""
    return _autograd_frame(renderer, cam, (pos, scale, rotq, sh, opacity), bg, scale_modifier, "maps", depth_mode)


def render_autograd_distortion(renderer: "Renderer", cam: Camera, pos, scale, rotq, sh, opacity, bg=(0.0, 0.0, 0.0),
                               depth_mode: str = "z", center: float = 0.0, scale_modifier: float = 1.0):
    """render_autograd_maps with the frame's depth-distortion map: returns (img [3, H, W], depth [H, W], alpha [H, W],
    dist [H, W]) as include/lcgs_hip.h defines them (dist = sum_{i<j} w_i w_j (v_i - v_j)^2, evaluated about `center`; not
    normalised, not clamped).  The backward runs lcgs_render_backward_distortion with the four incoming gradients; an output
    the loss does not use arrives as None (or zero-shaped) and is passed as NULL.  Like render_autograd it re-renders its own
    view when the renderer's generation has moved."""
    return _autograd_frame(renderer, cam, (pos, scale, rotq, sh, opacity), bg, scale_modifier, "distortion", depth_mode, center)


def render_autograd_normals(renderer: "Renderer", cam: Camera, pos, scale, rotq, sh, opacity, bg=(0.0, 0.0, 0.0),
                            depth_mode: str = "z", center: float = 0.0, scale_modifier: float = 1.0):
    """render_autograd_distortion with the frame's view-space normal map: returns (img [3, H, W], depth [H, W], alpha [H, W],
    dist [H, W], normal [3, H, W]) as include/lcgs_hip.h defines them (normal = sum_i w_i n_i, n_i the splat's shortest axis
    facing the camera; not normalised, not clamped).  The backward runs lcgs_render_backward_normals with the five incoming
    gradients; an output the loss does not use arrives as None (or zero-shaped) and is passed as NULL.  Like render_autograd it
    re-renders its own view when the renderer's generation has moved.  The pose is not an input: the camera gradient of the
    normal channel is not offered."""
    return _autograd_frame(renderer, cam, (pos, scale, rotq, sh, opacity), bg, scale_modifier, "normals", depth_mode, center)


def render_autograd_features(renderer: "Renderer", cam: Camera, pos, scale, rotq, sh, opacity, features, bg=(0.0, 0.0, 0.0),
                             scale_modifier: float = 1.0):
    """render_autograd with the caller's per-splat feature rows blended like colour: returns (img [3, H, W], alpha [H, W],
    feature_map [K, H, W]) as include/lcgs_hip.h defines them (feature_map = sum_i w_i f_i; not normalised, not clamped, no
    background).  features: [P, K] float32 in the order of the five scene tensors (a bound scene keeps the caller's order).  The
    backward runs lcgs_render_backward_features and the gradient goes to all six inputs; an output the loss does not use
    arrives as None (or zero-shaped) and is passed as NULL.  Like render_autograd it re-renders its own view when the
    renderer's generation has moved."""
    return _autograd_frame(renderer, cam, (pos, scale, rotq, sh, opacity), bg, scale_modifier, "features", features=features)


def normal_consistency_autograd(renderer: "Renderer", cam: Camera, depth, alpha, normal, weight: float = 0.05,
                                alpha_min: float = 1e-3):
    """Differentiable normal-consistency loss for torch: `loss = normal_consistency_autograd(r, cam, depth, alpha, normal)`, a
    scalar tensor, from a frame's depth (mode "z"), alpha and normal maps.  The forward is ONE
    lcgs_normal_consistency_loss_backward call that also stores the three gradients; the backward hands them out scaled by
    the incoming scalar.  Composes with the frame: `_, depth, alpha, _, normal = render_autograd_normals(r, cam, ...)`."""
    import torch

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, depth, alpha, normal):
            args = [t.detach().contiguous() for t in (depth, alpha, normal)]
            grads = [torch.empty_like(t) for t in args]
            loss = torch.empty(1, device=args[0].device, dtype=torch.float32)
            renderer.normal_consistency_loss_backward(cam, *args, *grads, loss, weight, alpha_min)
            ctx.save_for_backward(*grads)
            ctx.shapes = (depth.shape, alpha.shape, normal.shape)
            return loss[0]

        @staticmethod
        def backward(ctx, g_loss):
            return tuple((g * g_loss).view(s) if need else None
                         for g, s, need in zip(ctx.saved_tensors, ctx.shapes, ctx.needs_input_grad))

    return _Fn.apply(depth, alpha, normal)


def depth_prior_autograd(renderer: "Renderer", depth, alpha, prior, mask=None, kind: str = "pearson", align: str = "fit",
                         scale: float = 1.0, shift: float = 0.0, weight: float = 1.0, alpha_min: float = 1e-3, patch: int = 0,
                         patch_offset=(0, 0), stats=None):
    """Differentiable depth-prior loss for torch: `loss = depth_prior_autograd(r, depth, alpha, prior)`, a scalar tensor
    differentiable in depth and alpha (the prior and the mask are data).  The forward is ONE lcgs_depth_prior_loss_backward call
    that also stores the two gradients; the backward hands them out scaled by the incoming scalar.  Composes with the frame:
    `_, depth, alpha = render_autograd_maps(r, cam, ..., depth_mode="inv_z")`.  The other arguments are
    Renderer.depth_prior_loss_backward's."""
    import torch

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, depth, alpha):
            args = [t.detach().contiguous() for t in (depth, alpha)]
            grads = [torch.empty_like(t) for t in args]
            loss = torch.empty(1, device=args[0].device, dtype=torch.float32)
            renderer.depth_prior_loss_backward(*args, prior.detach().contiguous(), *grads, loss,
                                               None if mask is None else mask.detach().contiguous(), kind, align, scale, shift,
                                               weight, alpha_min, patch, patch_offset, stats)
            ctx.save_for_backward(*grads)
            ctx.shapes = (depth.shape, alpha.shape)
            return loss[0]

        @staticmethod
        def backward(ctx, g_loss):
            return tuple((g * g_loss).view(s) if need else None
                         for g, s, need in zip(ctx.saved_tensors, ctx.shapes, ctx.needs_input_grad))

    return _Fn.apply(depth, alpha)


def bilagrid_identity(num: int, dims=(16, 16, 8), device="cuda:0"):
    """`num` bilateral grids [num, 12, L, GH, GW], dims = (GW, GH, L), every cell the identity transform: channels 0, 5 and 10
    (the diagonal of the 3 x 4 matrix) are 1, the rest 0.  An ordinary float32 tensor: make it a parameter and step it with
    torch's optimiser."""
    import torch

    GW, GH, L = dims
    grids = torch.zeros(num, 12, L, GH, GW, dtype=torch.float32, device=device)
    grids[:, (0, 5, 10)] = 1.0
    return grids


def bilagrid_autograd(renderer: "Renderer", grid, img):
    """Differentiable bilateral-grid slice for torch: `out = bilagrid_autograd(r, grid, img)`, grid [12, L, GH, GW] one view's
    slab (e.g. `grids[v]`), img [3, H, W] the rendered frame (render_autograd's output).  The backward is ONE
    lcgs_bilagrid_backward call that computes only the gradients autograd asks for."""
    import torch

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, grid, img):
            grid, img = grid.detach().contiguous(), img.detach().contiguous()
            out = torch.empty_like(img)
            renderer.bilagrid_slice(grid, img, out)
            ctx.save_for_backward(grid, img)
            return out

        @staticmethod
        def backward(ctx, g_out):
            grid, img = ctx.saved_tensors
            g_grid = torch.empty_like(grid) if ctx.needs_input_grad[0] else None
            g_img = torch.empty_like(img) if ctx.needs_input_grad[1] else None
            if g_grid is not None or g_img is not None:
                renderer.bilagrid_backward(grid, img, g_out.contiguous(), g_img, g_grid)
            return g_grid, g_img

    return _Fn.apply(grid, img)


def bilagrid_tv_autograd(renderer: "Renderer", grids, weight: float = 10.0):
    """Differentiable total-variation term of bilateral grids for torch: `loss = bilagrid_tv_autograd(r, grids)`, a scalar
    tensor, grids [N, 12, L, GH, GW] (or one grid [12, L, GH, GW]).  The forward is ONE lcgs_bilagrid_tv_loss_backward call that
    also stores the gradient; the backward hands it out scaled by the incoming scalar."""
    import torch

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, grids):
            g = grids.detach().contiguous()
            g = g[None] if g.dim() == 4 else g
            grad = torch.empty_like(g)
            loss = torch.empty(1, device=g.device, dtype=torch.float32)
            renderer.bilagrid_tv_loss_backward(g, grad, loss, weight)
            ctx.save_for_backward(grad)
            ctx.shape = grids.shape
            return loss[0]

        @staticmethod
        def backward(ctx, g_loss):
            return (ctx.saved_tensors[0] * g_loss).view(ctx.shape)

    return _Fn.apply(grids)


def filter3d_autograd(renderer: "Renderer", scale, opacity, filt):
    """Differentiable 3-D smoothing filter for torch: `scale_f, opacity_f = filter3d_autograd(r, scale, opacity, filt)` from
    ACTIVATED scale [P, 3] and opacity [P] and the per-splat filter of Renderer.filter3d_finalize (a constant: no gradient).
    Forward is lcgs_filter3d_apply into fresh tensors, backward lcgs_filter3d_backward on dense rows.  Composes with the
    frames: `render_autograd(r, cam, pos, scale_f, rotq, sh, opacity_f)`."""
    import torch

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, scale, opacity, filt):
            args = [t.detach().contiguous() for t in (scale, opacity, filt)]
            scale_f, opacity_f = torch.empty_like(args[0]), torch.empty_like(args[1])
            renderer.filter3d_apply(*args, scale_f, opacity_f)
            ctx.save_for_backward(*args)
            ctx.shapes = (scale.shape, opacity.shape)
            return scale_f, opacity_f

        @staticmethod
        def backward(ctx, g_scale, g_opacity):
            args = ctx.saved_tensors
            # (the call works in place: on copies, the incoming gradients are autograd's)
            g_scale = torch.zeros_like(args[0]) if g_scale is None else g_scale.contiguous().clone()
            g_opacity = torch.zeros_like(args[1]) if g_opacity is None else g_opacity.contiguous().clone()
            renderer.filter3d_backward(*args, g_scale, g_opacity)
            return g_scale.view(ctx.shapes[0]), g_opacity.view(ctx.shapes[1]), None

    return _Fn.apply(scale, opacity, filt)


CAM12_FIELDS = ("position", "front", "up", "right")  # the camera gradient's order: Camera's first four members


def camera_grad_to_twist(cam: Camera, g12) -> np.ndarray:
    """lcgs_camera_grad_to_twist (host only): the 12 numbers of a camera gradient -> the gradient w.r.t. a twist
    (omega[3], tau[3]) applied in the camera's own frame, at zero."""
    g = np.ascontiguousarray(np.asarray(g12, dtype=np.float32).reshape(12))
    out = np.zeros(6, dtype=np.float32)
    _check(load_library().lcgs_camera_grad_to_twist(C.byref(cam), g.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def camera_with_vectors(cam: Camera, v12) -> Camera:
    """a copy of `cam` whose position / front / up / right are the twelve numbers of v12 (struct order)"""
    v = np.asarray(v12, dtype=np.float32).reshape(4, 3)
    out = Camera.from_dict(cam.to_dict())
    for k, name in enumerate(CAM12_FIELDS):
        for c in range(3):
            getattr(out, name)[c] = float(v[k, c])
    return out


def render_autograd_camera(renderer: "Renderer", cam: Camera, cam12, pos, scale, rotq, sh, opacity, bg=(0.0, 0.0, 0.0),
                           scale_modifier: float = 1.0, mode: str = "z"):
    """render_autograd_maps with a differentiable pose: returns (img, depth, alpha); `cam12` is a float32 tensor of twelve in
    the order of Camera's members (position, front, up, right) that REPLACES those four vectors of `cam` (fov, aspect ratio
    and size are cam's).  The backward returns the camera gradient for cam12 (the twelve numbers as independent variables:
    chain a pose parameterisation onto them, e.g. camera_grad_to_twist) plus the scene gradients.  When no scene tensor
    requires grad it runs lcgs_render_backward_camera and allocates no parameter rows."""
    view = camera_with_vectors(cam, cam12.detach().cpu().numpy())
    return _autograd_frame(renderer, view, (pos, scale, rotq, sh, opacity), bg, scale_modifier, "maps", mode, cam12=cam12)


# ---------------------------------------------------------------------------------------------- host io
def read_gs_ply(path: str) -> dict:
    """read_gs_ply (app/gaussians.cpp:75-171): activated, repacked host arrays."""
    lib = load_library()
    s = _SceneHost()
    _check(lib.lcgs_ply_read(path.encode(), C.byref(s)))
    try:
        P = s.num_gaussians

        def grab(p, n, shape):
            if P == 0:
                return np.zeros(shape, dtype=np.float32)
            return np.ctypeslib.as_array(p, shape=(n,)).reshape(shape).copy()

        return {
            "pos": grab(s.pos, P * 3, (P, 3)), "sh": grab(s.feature, P * 48, (P, 48)),
            "opacity": grab(s.opacity, P, (P,)), "scale": grab(s.scale, P * 3, (P, 3)),
            "rotq": grab(s.rotq, P * 4, (P, 4)), "sh_degree": int(s.sh_degree),
        }
    finally:
        lib.lcgs_scene_host_free(C.byref(s))


def write_ply_raw(path: str, pos, f_dc, f_rest, opacity_logit, log_scale, rot):
    a = [np.ascontiguousarray(x, dtype=np.float32) for x in (pos, f_dc, f_rest, opacity_logit, log_scale, rot)]
    P = int(a[0].reshape(-1, 3).shape[0])
    _check(load_library().lcgs_ply_write_raw(path.encode(), P, *[_ptr(x) for x in a]))


def ply_filter_rows(in_path: str, out_path: str, keep):
    """lcgs_ply_filter_rows: the vertex records of a binary PLY whose keep entry is non-zero, bit for bit and in order, behind
    the same header with the new count.  keep: one entry per vertex of the file (any array; compared with 0)."""
    k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
    _check(load_library().lcgs_ply_filter_rows(in_path.encode(), out_path.encode(), int(k.size), _ptr(k)))


def synth_scene(kind: int, seed: int, count: int, first: int = 0) -> dict:
    """Deterministic synthetic stand-in scene: kind 0 object-like, 1 unbounded-like."""
    out = {
        "pos": np.empty((count, 3), np.float32), "sh": np.empty((count, 48), np.float32),
        "opacity": np.empty((count,), np.float32), "scale": np.empty((count, 3), np.float32),
        "rotq": np.empty((count, 4), np.float32),
    }
    _check(load_library().lcgs_synth_scene(kind, seed, first, count, _ptr(out["pos"]), _ptr(out["sh"]), _ptr(out["opacity"]),
                                           _ptr(out["scale"]), _ptr(out["rotq"])))
    return out


def image_to_rgb8(img_chw: np.ndarray) -> np.ndarray:
    """app/main.cpp:323-335"""
    img = np.ascontiguousarray(img_chw, dtype=np.float32)
    _, H, W = img.shape
    out = np.empty((H, W, 3), np.uint8)
    load_library().lcgs_image_to_rgb8(W, H, _ptr(img), _ptr(out))
    return out


def write_png(path: str, rgb: np.ndarray):
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    H, W, _ = rgb.shape
    _check(load_library().lcgs_write_png(path.encode(), W, H, _ptr(rgb)))
