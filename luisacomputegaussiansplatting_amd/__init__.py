"""luisacomputegaussiansplatting_amd -- MI355X-native (gfx950) 3D Gaussian Splatting hot path.

The product is ``liblcgs_hip.so`` (C ABI in ``include/lcgs_hip.h``, hand-written HIP kernels in
``csrc/kernels``).  This package is the thin Python mirror of the reference's operator API
(``SHProcessor`` / ``GSProjector`` / ``GSTileSplatter`` + proxy structs, lcgs/include/lcgs/*.h) on top of
that C ABI.  torch is used only as the owner of device memory and streams.

There is no CPU fallback: every operator raises ``LcgsError`` if the HIP library is missing or no
gfx950 device is present.
"""
from . import api  # noqa: F401
from .api import (  # noqa: F401
    Camera,
    Comm,
    Context,
    DEPTH_INV_Z,
    DEPTH_Z,
    GSProjector,
    GSProjectorInputProxy,
    GSProjectorOutputProxy,
    GSSplatForwardOutputProxy,
    GSTileSplatter,
    GSTileSplatterAccelProxy,
    GSTileSplatterInputProxy,
    GPUPointsProxy,
    LOSS_L2,
    LOSS_PHOTOMETRIC,
    LcgsError,
    RASTER_ANTIALIASED,
    RASTER_CLASSIC,
    Renderer,
    SHProcessor,
    Similarity,
    SimilarityPlan,
    TsdfVolume,
    bilagrid_autograd,
    bilagrid_identity,
    bilagrid_tv_autograd,
    build_library,
    camera_grad_to_twist,
    camera_transform,
    camera_with_vectors,
    depth_prior_autograd,
    filter3d_autograd,
    get_lookat_cam,
    image_to_rgb8,
    knn_mean_dist2,
    library_path,
    load_library,
    local_to_world_matrix,
    mcmc_num_new,
    normal_consistency_autograd,
    ply_filter_rows,
    projection_matrix,
    read_gs_ply,
    read_points_ply,
    render_autograd,
    render_autograd_camera,
    render_autograd_distortion,
    render_autograd_features,
    render_autograd_normals,
    render_autograd_maps,
    scene_extent,
    shard_rows,
    similarity,
    similarity_plan,
    synth_scene,
    world_to_local_matrix,
    write_mesh_ply,
    write_png,
    write_ply_raw,
)

__version__ = "0.1"
