"""sfm_amd: MI355X-native matching + bundle-adjustment hot path."""

from .twoview import FundamentalMixin, estimate_fundamental_batched, find_fundamental  # noqa: F401
from .essential import EssentialMixin, estimate_essential_batched, find_essential  # noqa: F401
from .homography import HomographyMixin, estimate_homography_batched, find_homography  # noqa: F401
from .pose import InitialPairMixin, recover_pose, recover_pose_batched  # noqa: F401
from .tracks import Tracks, build_tracks, tracks_from_pair_files  # noqa: F401
from .triangulate import Triangulation, triangulate_tracks, triangulate_tracks_raw  # noqa: F401
from .incremental import Reconstruction, classify_tracks, evaluate_tracks, reconstruct_tracks, resection_lists  # noqa: F401
from .features import Features, PyramidFeatures, detect_and_describe_batched, detect_features, pyramid_levels  # noqa: F401
from .interchange import read_pnm, save_obj_mesh, save_ply_mesh, save_ply_points, write_png, write_pnm  # noqa: F401
from .guided import guided_match_pairs  # noqa: F401
from .depth import (DepthMaps, FusedCloud, dense_from_reconstruction, depth_maps, depth_maps_from_arrays, depth_ranges, plane_depths, select_sources,  # noqa: F401
                    view_backprojection, view_warps)
from .mesh import (Mesh, MeshRender, MeshTexture, RenderScore, TsdfVolume, check_score_arguments, mesh_texture, mesh_vertex_colors, render_mesh,  # noqa: F401
                   score_render, tsdf_volume_from_arrays)
from .mesh_clean import MeshComponents, check_clean_arguments, clean_mesh, mesh_components  # noqa: F401
from .mesh_fill import MeshEdges, check_fill_arguments, fill_mesh_holes, mesh_edges  # noqa: F401
from .mesh_decimate import check_decimate_arguments, decimate_mesh  # noqa: F401
from .mesh_smooth import MeshAdjacency, check_smooth_arguments, mesh_adjacency, mesh_vertex_normals, smooth_mesh  # noqa: F401
from .exposure import ExposureGains, apply_gains, check_exposure_arguments, mesh_exposure_tables, solve_gains  # noqa: F401
