"""emap_amd - MI355X-native render hot path of EMAP (cvg/EMAP) behind the reference's class API.

Public names mirror reference ``src/models``: UDFNetwork, SingleVarianceNetwork, BetaNetwork,
RenderingNetwork, UDFRendererBlending, sample_pdf, get_embedder, EdgeLoss.
"""
from .embedder import get_embedder, Embedder  # noqa: F401
from .loss import EdgeLoss  # noqa: F401
from .udf_model import UDFNetwork, SingleVarianceNetwork, BetaNetwork, RenderingNetwork  # noqa: F401
from .udf_renderer_blending import UDFRendererBlending, sample_pdf  # noqa: F401
from .ray_sampler import DeviceRaySampler  # noqa: F401
from .schedule import TrainSchedule  # noqa: F401
from .monitor import TrainMonitor  # noqa: F401
from . import edge_metrics  # noqa: F401
from .edge_metrics import (nearest_neighbors, chamfer_distance, compute_chamfer_distance, compute_precision_recall_IOU,  # noqa: F401
                           downsample_point_cloud_average, sample_segments, evaluate_edges, metrics_from_stats, f_score)
from . import parametric_edges  # noqa: F401
from .parametric_edges import (sample_edges, bezier_curve_length, get_pred_points_and_directions, process_geometry_data,  # noqa: F401
                               compute_visibility, finish_parametric_edges, evaluate_parametric_edges)
from . import dtu_eval  # noqa: F401
from .dtu_eval import point_visibility_counts, compute_point_visibility, gt_edge_points, evaluate_dtu, DTU_SCANS  # noqa: F401
from . import edge_fitting as fitting  # noqa: F401  (emap_amd.edge_fitting is the reference's FUNCTION, imported below; the module is emap_amd.fitting)
from .edge_fitting import connect_points, edge_fitting, edge_fit, merge, get_parametric_edge  # noqa: F401
from . import edge_raster  # noqa: F401
from .edge_raster import rasterize_edges, rasterize_parametric_edges, to_dataset_edges, make_parametric_scene  # noqa: F401
from . import edge_score  # noqa: F401
from .edge_score import (distance_maps, score_edge_maps, score_parametric_edges, score_rendered_views,  # noqa: F401
                         filter_edges_by_support)
from . import edge_field  # noqa: F401
from .edge_field import (edge_segments, polyline_segments, point_edge_distances, edge_udf, evaluate_udf,  # noqa: F401
                         evaluate_points_on_edges)

__all__ = ["UDFNetwork", "SingleVarianceNetwork", "BetaNetwork", "RenderingNetwork", "UDFRendererBlending",
           "sample_pdf", "get_embedder", "Embedder", "EdgeLoss", "DeviceRaySampler", "TrainSchedule", "TrainMonitor",
           "edge_metrics", "nearest_neighbors", "chamfer_distance", "compute_chamfer_distance", "compute_precision_recall_IOU",
           "downsample_point_cloud_average", "sample_segments", "evaluate_edges", "metrics_from_stats", "f_score",
           "parametric_edges", "sample_edges", "bezier_curve_length", "get_pred_points_and_directions", "process_geometry_data",
           "compute_visibility", "finish_parametric_edges", "evaluate_parametric_edges",
           "dtu_eval", "point_visibility_counts", "compute_point_visibility", "gt_edge_points", "evaluate_dtu", "DTU_SCANS",
           "connect_points", "edge_fitting", "edge_fit", "merge", "get_parametric_edge",
           "edge_raster", "rasterize_edges", "rasterize_parametric_edges", "to_dataset_edges", "make_parametric_scene",
           "edge_score", "distance_maps", "score_edge_maps", "score_parametric_edges", "score_rendered_views", "filter_edges_by_support",
           "edge_field", "edge_segments", "polyline_segments", "point_edge_distances", "edge_udf", "evaluate_udf", "evaluate_points_on_edges"]
