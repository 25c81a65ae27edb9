"""ctypes binding of libsgam_hip.so (include/sgam_hip.h).  There is NO fallback: if the library is
missing or a call fails, the product path raises — results never come from a CPU/torch substitute."""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# SGAM_HIP_LIB: an alternative build of the same library (kernel A/B experiments, scripts/tsdf_variants.sh); default = the in-tree build
LIB_PATH = os.environ.get("SGAM_HIP_LIB") or os.path.join(_PKG, "lib", "libsgam_hip.so")

c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class ConvDesc(ctypes.Structure):
    """mirror of struct sgam_conv_desc"""
    _fields_ = [(n, c_i32) for n in (
        "B", "Hi", "Wi", "Cin", "Ho", "Wo", "N", "KH", "KW", "stride", "pad_t", "pad_l", "upsample2x",
        "lda", "ldb", "ldc", "ldr", "n_valid", "bias_per_row", "plan_bm", "plan_bn", "plan_ksplit")]


class TsdfGrid(ctypes.Structure):
    """mirror of struct sgam_tsdf_grid"""
    _fields_ = [("voxel_length", c_f32), ("sdf_trunc", c_f32), ("unit_base", c_i32 * 3), ("unit_dims", c_i32 * 3)]


class TsdfSrc(ctypes.Structure):
    """mirror of struct sgam_tsdf_src"""
    _fields_ = [("depth", c_vp), ("rgb_u8", c_vp), ("cam2world", c_f32 * 16), ("world2cam", c_f32 * 16)]


class TsdfScene(ctypes.Structure):
    """mirror of struct sgam_tsdf_scene (one entry of the scene-batched kernels' DEVICE table)"""
    _fields_ = [("unit_table", c_vp), ("unit_stamp", c_vp), ("counters", c_vp), ("brick_list", c_vp), ("brick_tsdf", c_vp),
                ("brick_weight", c_vp), ("brick_color", c_vp), ("max_bricks", c_i32), ("max_list", c_i32)]


# name -> (restype, argtypes); must list every symbol include/sgam_hip.h declares
ABI_VERSION = 10     # include/sgam_hip.h: sgam_abi_version() of the library these prototypes were written against

PROTOTYPES = {
    "sgam_abi_version": (c_i32, []),
    "sgam_build_info": (ctypes.c_char_p, []),
    "sgam_build_commit": (ctypes.c_char_p, []),
    "sgam_build_digest": (ctypes.c_char_p, []),
    "sgam_prof_enable": (c_i32, [c_i32]),
    "sgam_prof_mark_empty": (c_i32, [c_vp]),
    "sgam_prof_count": (c_i32, []),
    "sgam_prof_get": (c_i32, [c_i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                              ctypes.POINTER(c_f32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "sgam_prof_get_shape": (c_i32, [c_i32, ctypes.POINTER(c_i32)]),
    "sgam_conv2d_workspace_bytes": (c_i64, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_plan": (c_i32, [ctypes.POINTER(ConvDesc), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                 ctypes.POINTER(c_i32)]),
    "sgam_conv2d_nhwc_f32": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "sgam_conv2d_gn_nhwc_f32": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64,
                                        c_vp]),
    "sgam_pack_conv_weight": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_f32x_set_range_flag": (c_i32, [c_vp]),
    "sgam_conv2d_f32x_workspace_bytes": (c_i64, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_f32x_plan": (c_i32, [ctypes.POINTER(ConvDesc), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                      ctypes.POINTER(c_i32)]),
    "sgam_conv2d_nhwc_f32x": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_f32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_i64,
                                      c_vp]),
    "sgam_conv2d_f32x_stats_chunks": (c_i32, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_f32x_stats_mode": (c_i32, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_stats_nhwc_f32x": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_f32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_i64, c_vp]),
    "sgam_groupnorm_from_partials_f32": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32,
                                                 c_i32, c_vp, c_i64, c_vp]),
    "sgam_conv2d_f32x_gn_fusable": (c_i32, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_f32x_uses_halo": (c_i32, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_gn_nhwc_f32x": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_f32, c_vp, c_vp,
                                         c_vp, c_vp, c_vp, c_i64, c_vp]),
    "sgam_conv2d_f32x_gn_foldable": (c_i32, [ctypes.POINTER(ConvDesc), c_i32]),
    "sgam_conv2d_gnp_nhwc_f32x": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_vp, c_i32, c_f32, c_vp, c_vp, c_i32, c_vp, c_f32, c_vp,
                                          c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "sgam_groupnorm_stats_from_partials_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_groupnorm_meanrstd_nhwc_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i64, c_vp]),
    "sgam_tsdf_integrate_srcs_f32": (c_i32, [ctypes.POINTER(TsdfGrid), ctypes.POINTER(TsdfSrc), c_i32, c_i32, c_i32, c_f32, c_f32, c_f32,
                                             c_f32, c_f32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_tsdf_integrate_scenes_f32": (c_i32, [ctypes.POINTER(TsdfGrid), c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32,
                                               c_f32, c_i32, c_i32, c_vp, c_vp]),
    "sgam_tsdf_raycast_scenes_f32": (c_i32, [ctypes.POINTER(TsdfGrid), c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_f32,
                                             c_f32, c_vp, c_vp, c_vp]),
    "sgam_tsdf_ray_mult_f32": (c_i32, [c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp]),
    "sgam_tsdf_raycast_depth_f32": (c_i32, [ctypes.POINTER(TsdfGrid), c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_vp, c_f32,
                                            c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_tsdf_extract_points_f32": (c_i32, [ctypes.POINTER(TsdfGrid), c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_tsdf_mesh_workspace_bytes": (c_i64, [ctypes.POINTER(TsdfGrid), c_i32]),
    "sgam_tsdf_extract_mesh_f32": (c_i32, [ctypes.POINTER(TsdfGrid), c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_f32, c_f32, c_f32,
                                           c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "sgam_mesh_render_depth_f32": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_vp, c_f32, c_f32,
                                           c_vp, c_vp]),
    "sgam_mesh_render_rgbd_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_mesh_render_rgbd_f32": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_vp, c_f32,
                                          c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "sgam_points_render_rgbd_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    "sgam_points_render_rgbd_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32,
                                            c_f32, c_f32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "sgam_points_unproject_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_f32, c_f32, c_vp, c_vp, c_vp]),
    "sgam_points_nn_brute_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp]),
    "sgam_points_grid_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    "sgam_points_grid_build": (c_i32, [c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "sgam_points_nn_grid_f32": (c_i32, [c_vp, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_f32, c_vp, c_vp,
                                        c_vp]),
    "sgam_points_nn_reduce_partials": (c_i64, [c_i64]),
    "sgam_points_nn_reduce": (c_i32, [c_vp, c_i64, c_f32, c_vp, c_vp]),
    "sgam_points_knn_brute_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp, c_vp, c_vp]),
    "sgam_points_knn_grid_f32": (c_i32, [c_vp, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_i32, c_f32,
                                         c_i32, c_vp, c_vp, c_vp]),
    "sgam_points_voxel_workspace_bytes": (c_i64, [c_i32]),
    "sgam_points_voxel_sample_f32": (c_i32, [c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "sgam_points_knn_mean_distance": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "sgam_points_md_reduce_partials": (c_i64, [c_i64]),
    "sgam_points_md_reduce": (c_i32, [c_vp, c_i64, ctypes.c_double, c_i32, c_vp, c_vp]),
    "sgam_points_normals_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_points_transform_f32": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_points_icp_partials": (c_i64, [c_i64]),
    "sgam_points_icp_accumulate": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "sgam_points_icp_update": (c_i32, [c_vp, c_i64, c_i32, ctypes.c_double, ctypes.c_double, c_vp, c_vp, c_vp]),
    "sgam_points_color_gradient_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "sgam_points_icp_accumulate_colored": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, ctypes.c_double, c_vp, c_vp]),
    "sgam_mesh_components_workspace_bytes": (c_i64, [c_i32]),
    "sgam_mesh_components_i32": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_mark_vertices_i32": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_remap_triangles_i32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_mesh_incidence_count_i32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "sgam_mesh_incidence_fill_i32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_vertex_normals_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "sgam_mesh_smooth_step_f32": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_i64, ctypes.c_double, c_vp]),
    "sgam_points_voxel_assign_f32": (c_i32, [c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_dedup_workspace_bytes": (c_i64, [c_i32]),
    "sgam_mesh_cluster_triangles_i32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_quadric_init_f64": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i64, ctypes.c_double, c_vp, c_vp, c_vp]),
    "sgam_mesh_collapse_evaluate_f64": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i32, c_vp, c_vp,
                                                c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_collapse_workspace_bytes": (c_i64, [c_i32]),
    "sgam_mesh_collapse_select_i32": (c_i32, [c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_f32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "sgam_mesh_collapse_apply_f64": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp,
                                             c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_distance_brute_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_grid_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32, c_i32]),
    "sgam_mesh_grid_count": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "sgam_mesh_grid_build": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "sgam_mesh_distance_grid_f32": (c_i32, [c_vp, c_i32, c_i64, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_f32, c_vp, c_vp,
                                            c_vp, c_vp]),
    "sgam_mesh_triangle_area2_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_mesh_raycast_brute_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_vp]),
    "sgam_mesh_raycast_grid_f32": (c_i32, [c_vp, c_i32, c_i64, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_i32, c_f32, c_f32,
                                           c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_visibility_grid_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32,
                                              c_i64, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "sgam_mesh_visibility_brute_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32,
                                               c_f32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp]),
    "sgam_rays_pinhole_f32": (c_i32, [c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_vp, c_vp]),
    "sgam_mesh_bvh_workspace_bytes": (c_i64, [c_i64]),
    "sgam_mesh_bvh_keys": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_bvh_build": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "sgam_mesh_distance_bvh_f32": (c_i32, [c_vp, c_i32, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_i64, c_f32, c_vp, c_vp, c_vp,
                                           c_vp, c_vp]),
    "sgam_mesh_raycast_bvh_f32": (c_i32, [c_vp, c_i32, c_i64, c_vp, c_i64, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_mesh_visibility_bvh_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32,
                                             c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "sgam_mesh_sample_f32": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, ctypes.c_uint64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_gemm_gn_f32x_fits": (c_i32, [c_i32, c_i32, c_i32, c_i32]),
    "sgam_gemm_panel_f32x": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32,
                                     c_i32, c_vp]),
    "sgam_gemm_gn_f32x": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_im2col_t_f32": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_vp, c_i32, c_i64, c_vp]),
    "sgam_col2im_gather_f32": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_vp, c_i32, c_vp]),
    "sgam_unpack_conv_weight_grad_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_colsum_workspace_bytes": (c_i64, [c_i32, c_i32]),
    "sgam_colsum_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "sgam_groupnorm_bwd_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_groupnorm_bwd_nhwc_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                            c_vp, c_i64, c_vp]),
    "sgam_softmax_bwd_rows_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_l1_loss_grad_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_vq_bwd_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_vp]),
    "sgam_vq_codebook_grad_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_axpby_f32": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_vp]),
    "sgam_adam_step_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_f32, c_i32, c_vp]),
    "sgam_adam_multi_step_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_vp]),
    "sgam_batchnorm_workspace_bytes": (c_i64, [c_i32, c_i32]),
    "sgam_batchnorm_stats_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_f32, c_f32, c_vp, c_i64, c_vp]),
    "sgam_bn_lrelu_fwd_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_f32, c_vp]),
    "sgam_bn_lrelu_bwd_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_f32, c_vp, c_i64,
                                      c_vp]),
    "sgam_hinge_terms_f32": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_f32, c_vp]),
    "sgam_sumsq_partial_f32": (c_i32, [c_vp, c_vp, c_i64, c_vp]),
    "sgam_maxpool2x2_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_maxpool2x2_bwd_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_channel_affine_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "sgam_lpips_level_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp]),
    "sgam_recon_stats_partials": (c_i64, [c_i32, c_i32]),
    "sgam_recon_stats_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_ssim_partials": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    "sgam_ssim_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_index_histogram_i32": (c_i32, [c_vp, c_i64, c_vp, c_i32, c_vp]),
    "sgam_kmeans_chunk_points": (c_i32, [c_i32, c_i32, c_i32]),
    "sgam_kmeans_assign_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    "sgam_kmeans_assign_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "sgam_kmeans_update_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_kmeans_update_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "sgam_kmeans_init_points_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, ctypes.c_uint64, ctypes.c_uint64, c_vp]),
    "sgam_codebook_countdown_i32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "sgam_codebook_scatter_rows_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp]),
    "sgam_pack_conv_weight_f32x": (c_i32, [c_vp, c_vp, c_f32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_split_rows_f32x": (c_i32, [c_vp, c_vp, c_f32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_conv2d_h16_workspace_bytes": (c_i64, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_h16_plan": (c_i32, [ctypes.POINTER(ConvDesc), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                     ctypes.POINTER(c_i32)]),
    "sgam_conv2d_nhwc_h16": (c_i32, [ctypes.POINTER(ConvDesc), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i64,
                                     c_vp]),
    "sgam_conv2d_h16_generic_stats_chunks": (c_i32, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_stats_nhwc_h16": (c_i32, [ctypes.POINTER(ConvDesc), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i64,
                                           c_vp]),
    "sgam_conv2d_h16_uses_halo": (c_i32, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_h16_stats_chunks": (c_i32, [ctypes.POINTER(ConvDesc)]),
    "sgam_pack_conv_weight_h16_frag": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_conv2d_halo_h16_workspace_bytes": (c_i64, [ctypes.POINTER(ConvDesc)]),
    "sgam_conv2d_halo_nhwc_h16": (c_i32, [ctypes.POINTER(ConvDesc), c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp,
                                          c_i32, c_vp, c_vp, c_i64, c_vp]),
    "sgam_conv2d_h16_gn_foldable": (c_i32, [ctypes.POINTER(ConvDesc), c_i32]),
    "sgam_conv2d_halo_gnp_nhwc_h16": (c_i32, [ctypes.POINTER(ConvDesc), c_i32, c_vp, c_vp, c_i32, c_f32, c_vp, c_vp, c_i32, c_vp, c_vp,
                                              c_vp, c_vp, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "sgam_groupnorm_from_partials_h16": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32,
                                                 c_i32, c_vp, c_i64, c_vp]),
    "sgam_groupnorm_meanrstd_nhwc_h16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i64, c_vp]),
    "sgam_pack_conv_weight_h16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_cast_f32_h16": (c_i32, [c_vp, c_vp, c_i32, c_i64, c_vp]),
    "sgam_cast_h16_f32": (c_i32, [c_vp, c_vp, c_i32, c_i64, c_vp]),
    "sgam_groupnorm_h16_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_groupnorm_nhwc_h16": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp,
                                        c_i64, c_vp]),
    "sgam_softmax_rows_h16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_softmax_rows_blockdiag_h16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp]),
    "sgam_encode_head_h16": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_transpose_h16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_groupnorm_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_groupnorm_nhwc_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp,
                                        c_i64, c_vp]),
    "sgam_groupnorm_stats_nhwc_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i64,
                                              c_vp]),
    "sgam_softmax_rows_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_softmax_rows_blockdiag_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp]),
    "sgam_attention_f32x_workspace_bytes": (c_i64, [c_i32, c_i32]),
    "sgam_attention_f32x": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp, c_i32, c_vp, c_i64, c_vp]),
    "sgam_attention_h16_workspace_bytes": (c_i64, [c_i32, c_i32]),
    "sgam_attention_h16": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i32, c_vp, c_i64, c_vp]),
    "sgam_attention_f32x_batched_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_attention_f32x_batched": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i32, c_vp, c_i64, c_vp]),
    "sgam_attention_proj_f32x_batched": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_f32, c_vp, c_vp, c_i32, c_vp,
                                                 c_i32, c_vp, c_vp, c_i64, c_vp]),
    "sgam_attention_h16_batched_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_attention_h16_batched": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i32, c_vp, c_i64, c_vp]),
    "sgam_attn_block_f32x_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_attn_block_f32x": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_f32, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp, c_f32, c_vp, c_vp, c_i32,
                                     c_vp, c_vp, c_i64, c_vp]),
    "sgam_attention_small_f32x_fits": (c_i32, [c_i32, c_i32, c_i32]),
    "sgam_attention_small_f32x": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i32, c_vp]),
    "sgam_attention_small_h16": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i32, c_vp]),
    "sgam_groupnorm_table_from_partials": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_pack_qkv_weight_h16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp]),
    "sgam_pack_weight_tp_h16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "sgam_attn_block_proj_h16": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp,
                                         c_vp, c_vp, c_i32, c_vp, c_i64, c_vp]),
    "sgam_attn_block_h16_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_attn_block_h16": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_i32,
                                    c_vp, c_i64, c_vp]),
    "sgam_row_sumsq_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp]),
    "sgam_vq_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_vq_nearest_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp,
                                    c_i64, c_vp]),
    "sgam_vq_commit_loss_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_vq_gather_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "sgam_vq_topk_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "sgam_vq_sample_topk_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint64, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                        c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "sgam_nchw_to_nhwc_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_nhwc_to_nchw_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "sgam_encode_head_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "sgam_forward_splat_f32": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                       ctypes.POINTER(c_f32), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, c_vp, c_vp]),
    "sgam_forward_splat_srcs_f32": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                            ctypes.POINTER(c_f32), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_vp, c_vp, c_vp]),
    "sgam_forward_splat_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    "sgam_forward_splat_workspace_zero_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    "sgam_forward_splat_tiled_f32": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                             ctypes.POINTER(c_f32), c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_forward_splat_tiled_srcs_f32": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                                  ctypes.POINTER(c_f32), c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                  c_vp]),
    "sgam_depth_normalise_f32": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i64, c_vp]),
    "sgam_inverse_warp_f32": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp,
                                      c_vp]),
    "sgam_inverse_warp_srcs_f32": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                           c_vp, c_vp, c_vp]),
    "sgam_rgb_u8_to_f32": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_vp]),
    "sgam_frame_feedback_f32": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "sgam_resize_lanczos_u8": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32,
                                       c_vp, c_vp, c_vp, c_vp]),
    "sgam_resize_nearest_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_f32, c_f32, c_vp, c_vp]),
    "sgam_resize_bicubic_u8": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32,
                                       c_vp, c_vp, c_i32, c_vp]),
    "sgam_frame_depth_codec_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(ctypes.c_double), c_vp, c_i32,
                                           c_i32, c_vp]),
    # FID evaluation (csrc/inception.hip; the ReLU entry point of csrc/conv_gemm.hip)
    "sgam_conv2d_relu_nhwc_f32": (c_i32, [ctypes.POINTER(ConvDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "sgam_inception_preprocess_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "sgam_pool3x3_out_size": (c_i32, [c_i32, c_i32, c_i32, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    "sgam_pool3x3_nhwc_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_i32, c_vp]),
    "sgam_global_avgpool_nhwc_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "sgam_activation_stats_state_doubles": (c_i64, [c_i32]),
    "sgam_activation_stats_update_f64": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp]),
    "sgam_activation_stats_finalize_f64": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    # KID and precision / recall / density / coverage on a device fp64 Gram (csrc/feature_metrics.hip)
    "sgam_feature_gram_f64": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "sgam_kid_subsets_u32": (c_i32, [c_i32, c_i32, c_i32, c_i32, ctypes.c_uint64, c_vp, c_i64, c_vp, c_vp]),
    "sgam_kid_mmd_f64": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, ctypes.c_double, ctypes.c_double, c_vp, c_i64, c_vp, c_vp]),
    "sgam_feature_prdc_f64": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    # global registration: FPFH, nearest feature, RANSAC (csrc/point_global.hip)
    "sgam_points_fpfh_counts": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "sgam_points_fpfh_combine_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "sgam_features_match_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "sgam_points_ransac_hypotheses": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_uint64, c_vp, c_vp, c_vp, c_vp]),
    "sgam_points_ransac_score_workspace_bytes": (c_i64, [c_i32]),
    "sgam_points_ransac_score": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i32, c_f32, c_i32, c_vp, c_i64, c_vp, c_vp,
                                         c_vp]),
    "sgam_points_ransac_inliers": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    # multiway registration: the pose graph, its optimiser and the dense fp64 SPD solve (csrc/pose_graph.hip)
    "sgam_pose_graph_check": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32]),
    "sgam_pose_graph_linearize": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_vp]),
    "sgam_pose_graph_assemble": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_pose_graph_fold": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "sgam_pose_graph_gate": (c_i32, [c_vp, c_i32, c_i32, ctypes.c_double, c_vp, c_vp, c_vp]),
    "sgam_pose_graph_trial": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_pose_graph_decide": (c_i32, [c_i32, c_i32, c_vp, c_i32, c_i32, ctypes.c_double, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "sgam_spd_solve_workspace_doubles": (c_i64, [c_i32]),
    "sgam_spd_solve_f64": (c_i32, [c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    # reprojection view consistency between stored frames (csrc/view_consistency.hip)
    "sgam_view_consistency_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_view_consistency_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp,
                                          c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    # direct RGB-D odometry of frame pairs in lock step (csrc/rgbd_odometry.hip)
    "sgam_rgbd_pyramid_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "sgam_rgbd_odometry_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "sgam_rgbd_odometry_accumulate_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32,
                                                  ctypes.c_double, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "sgam_rgbd_odometry_update": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.c_double, ctypes.c_double, c_vp, c_vp,
                                          c_vp, c_vp]),
    "sgam_points_radius_count_brute_f32": (c_i32, [c_vp, c_i32, c_f32, c_vp, c_vp]),
    "sgam_points_radius_count_grid_f32": (c_i32, [c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_f32, c_vp,
                                                  c_vp]),
    "sgam_points_dbscan_workspace_bytes": (c_i64, [c_i32]),
    "sgam_points_dbscan_brute_f32": (c_i32, [c_vp, c_i32, c_f32, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_points_dbscan_grid_f32": (c_i32, [c_vp, c_i32, c_f32, c_f32, c_f32, c_f32, c_i32, c_i32, c_i32, c_vp, c_i64, c_f32, c_i32, c_vp,
                                            c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "sgam_points_planes_workspace_bytes": (c_i64, [c_i32, c_i32]),
    "sgam_points_segment_planes_f32": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f32, c_i32, ctypes.c_uint64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp,
                                               c_vp]),
    "sgam_points_plane_score_f32": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_f32, c_i32, c_vp, c_vp]),
    "sgam_points_cluster_boxes_f32": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
}

_ERRORS = {-1: "SGAM_EINVAL (bad shape / unsupported size)", -2: "SGAM_EALIGN (pointer/stride alignment)",
           -3: "SGAM_EWORKSPACE (workspace missing or too small)"}


class SgamHipError(RuntimeError):
    pass


_lib = None


def load():
    """Load libsgam_hip.so; raise loudly if it has not been built (python -m sgam_neurips22_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).  It must be in the
    # process BEFORE this library so that our DT_NEEDED libamdhip64.so.7 binds to that same runtime instance;
    # loading /opt/rocm's copy first gives two runtimes in one process (hipErrorNoDevice on the second).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise SgamHipError(
            f"{LIB_PATH} is missing: the HIP backend has not been built. Run "
            "`python -m sgam_neurips22_amd.build` (needs hipcc). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.sgam_abi_version() != ABI_VERSION:
        raise SgamHipError(f"{LIB_PATH} speaks ABI v{lib.sgam_abi_version()}, these bindings v{ABI_VERSION}: rebuild "
                           "(`python -m sgam_neurips22_amd.build`)")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = _ERRORS.get(rc, f"hipError_t {rc}" if rc > 0 else f"error {rc}")
        raise SgamHipError(f"{what} failed: {msg}")
