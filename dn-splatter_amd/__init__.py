"""dn-splatter_amd — MI355X-native (gfx950) renderer that drops in behind
``DNSplatterModel.get_outputs`` of maturk/dn-splatter.

Public surface = the four gsplat symbols dn-splatter imports (dn_splatter/dn_model.py:29-35) plus
the fused one-pass renderer and the get_outputs mirror:

    from dn_splatter_amd import rasterization, rasterize_gaussians, quat_to_rotmat, num_sh_bases
    from dn_splatter_amd import render_dn, DNSplatterRenderer

All rendering arithmetic runs in hand-written HIP kernels (``csrc/*.hip`` -> ``libdnsplat.so``,
C ABI in ``include/dnsplat.h``).  There is no CPU fallback: without a GPU, or without the built
library, the ops raise.
"""
from ._lib import DnsplatError, build as build_library, lib as load_library  # noqa: F401
from .legacy import num_sh_bases, quat_to_rotmat, rasterize_gaussians  # noqa: F401
from .rendering import rasterization  # noqa: F401
from .fused import render_dn  # noqa: F401
from .model import Camera, DNSplatterRenderer, RendererConfig, get_viewmat  # noqa: F401
from ._ops import set_bin_policy, set_deterministic, set_grad_arena, set_sh_exchange  # noqa: F401
from . import dp  # noqa: F401
from .densify import DensifyStats  # noqa: F401
from .install import install, install_losses, install_metrics, install_ssim, uninstall  # noqa: F401
from .fused_loss import LocalPearsonDepthLoss, PearsonDepthLoss, local_pearson_depth, pearson_depth  # noqa: F401
from .fused_loss import ags_mesh_loss_fused, ags_normal_loss  # noqa: F401
from . import fused_metrics, torch_metrics  # noqa: F401
from .fused_metrics import image_metrics, image_metrics_dict  # noqa: F401
from . import export  # noqa: F401
from .export import OrientedPointCloud, export_oriented_points  # noqa: F401
from . import density, torch_density  # noqa: F401
from .density import GaussianDensityField, build_index, density_volume, install_density, knn  # noqa: F401
from . import levelset, torch_levelset  # noqa: F401
from .levelset import LevelSetCloud, export_level_set_points, install_level_sets, level_surface_points  # noqa: F401
from . import marching, torch_marching  # noqa: F401
from .marching import marching_cubes, marching_cubes_mesh, mcubes_marching_cubes  # noqa: F401
from . import geometry, torch_geometry  # noqa: F401
from .geometry import (PDMetrics, calculate_accuracy, calculate_completeness, cloud_distances, cloud_metrics, install_pd_metrics,  # noqa: F401
                       mesh_metrics, sample_mesh_surface)
from . import mesh_cull, torch_mesh_cull  # noqa: F401
from .mesh_cull import cull_mesh, culled_mesh_metrics, cut_mesh, render_mesh_depth, vertex_visibility  # noqa: F401
from . import tsdf, torch_tsdf  # noqa: F401
from .tsdf import TSDFVolume, fuse_tsdf_mesh  # noqa: F401
from . import mesh_clusters, torch_mesh_clusters  # noqa: F401
from .mesh_clusters import cluster_connected_triangles, filter_small_clusters  # noqa: F401
from . import cloud_filter, torch_cloud_filter  # noqa: F401
from .cloud_filter import remove_statistical_outlier, voxel_down_sample  # noqa: F401
from . import icp, torch_icp  # noqa: F401
from .icp import ICPResult, get_align_transformation, registration_icp, transform_mesh, transform_points  # noqa: F401
from . import subdivide, torch_subdivide  # noqa: F401
from .subdivide import subdivide_mesh, subdivide_to_size  # noqa: F401
from . import normals, torch_normals  # noqa: F401
from .normals import depth_normals, estimate_normals, normal_consistency_mask, points3D_normals  # noqa: F401

__all__ = [
    "rasterization", "rasterize_gaussians", "quat_to_rotmat", "num_sh_bases", "render_dn",
    "DNSplatterRenderer", "RendererConfig", "Camera", "get_viewmat", "set_bin_policy", "set_deterministic", "set_grad_arena", "set_sh_exchange", "dp", "DensifyStats",
    "install", "install_losses", "install_metrics", "install_ssim", "uninstall", "image_metrics", "image_metrics_dict",
    "fused_metrics", "torch_metrics", "PearsonDepthLoss", "LocalPearsonDepthLoss", "pearson_depth",
    "local_pearson_depth", "ags_normal_loss", "ags_mesh_loss_fused", "export", "OrientedPointCloud",
    "export_oriented_points", "density", "torch_density", "GaussianDensityField", "build_index", "density_volume", "install_density", "knn",
    "levelset", "torch_levelset", "LevelSetCloud", "export_level_set_points", "install_level_sets", "level_surface_points",
    "marching", "torch_marching", "marching_cubes", "marching_cubes_mesh", "mcubes_marching_cubes",
    "geometry", "torch_geometry", "PDMetrics", "calculate_accuracy", "calculate_completeness", "cloud_distances", "cloud_metrics",
    "install_pd_metrics", "mesh_metrics", "sample_mesh_surface",
    "mesh_cull", "torch_mesh_cull", "cull_mesh", "culled_mesh_metrics", "cut_mesh", "render_mesh_depth", "vertex_visibility",
    "tsdf", "torch_tsdf", "TSDFVolume", "fuse_tsdf_mesh",
    "mesh_clusters", "torch_mesh_clusters", "cluster_connected_triangles", "filter_small_clusters",
    "cloud_filter", "torch_cloud_filter", "remove_statistical_outlier", "voxel_down_sample",
    "icp", "torch_icp", "ICPResult", "registration_icp", "get_align_transformation", "transform_points", "transform_mesh",
    "subdivide", "torch_subdivide", "subdivide_to_size", "subdivide_mesh",
    "normals", "torch_normals", "estimate_normals", "points3D_normals", "depth_normals", "normal_consistency_mask",
    "build_library", "load_library", "DnsplatError",
]
