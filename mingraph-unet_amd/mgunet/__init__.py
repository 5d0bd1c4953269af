"""mgunet: MI355X-native MinGraph-UNet segmentation hot path (host-side mirror of the reference's
model/ API over libmgunet.so).  Importing works without a GPU; running anything needs one."""
from .config import build_from_config, get_config_recursively, load_config  # noqa: F401
from .detection import DetectionHead  # noqa: F401
from .engine import CosineAnnealingLR, E2ETrainer, FlatAdam, MinGraphUNet, MinGraphUNetE2E, ReduceLROnPlateau, StepLR, Trainer, scheduler_from_config, trainer_from_config, adam_state_dict, allreduce_mean_, argmax_classes, gat_forward_csr, segment_batch, shard_batch  # noqa: F401
from .gat import GATNetwork, GraphAttentionLayer, MultiHeadGATLayer, seed_dropout  # noqa: F401
from .losses import (EllipticalShapeLoss, FeatureConsistencyLoss, TVLoss, class_weights, dice_loss, lovasz_softmax,  # noqa: F401
                     pixel_cross_entropy)
from .preprocess import CLAHE, EdgeDetector, GaussianSmoother, HistogramEqualizer, ImagePreprocessor, RandomAffineColor, RandomElasticAffineColor, RandomFlipRotate, affine_fixed, bspline_weights_q14, color_matrix_q12, elastic_control, elastic_field, draw_flip_rotate, gaussian_kernel_q8, luma_sums, patch_clahe_features_u8, patch_features_u8, patch_smooth_features_u8, pil_rotation_fixed, postprocess_segmentation  # noqa: F401
from .metrics import SegmentationEvaluator, allreduce_eval_state, evaluate_segmentation, metrics_from_confusion, segmentation_metrics  # noqa: F401
from .objects import (ObjectShapes, ObjectTable, YieldEvaluator, clean_masks, connected_components, distance_transform,  # noqa: F401
                      evaluate_yield, object_shapes, split_objects, yield_estimation_metrics)
from .border import border_distances, border_weights  # noqa: F401
from .tta import object_scores, predict_tta  # noqa: F401
from .instances import (InstanceEvaluator, OverlapTable, evaluate_instances, instance_metrics, match_masks, object_detection_mAP,  # noqa: F401
                        object_overlaps, panoptic_totals)
from .maskio import (OutlineTable, RunTable, encode_masks, labels_from_runs, object_outlines, objects_from_annotations,  # noqa: F401
                     rasterize_polygons, rle_from_string, rle_to_string, runs_from_coco)
from .boundary import BoundaryEvaluator, BoundaryTables, boundary_metrics, boundary_tables, evaluate_boundaries  # noqa: F401
from .video import VideoCounter, count_video, frame_shifts, link_objects, track_ids  # noqa: F401
from .tiled import predict_tiled, tile_grid, tile_weights  # noqa: F401
from .refine import EdgeRefiner, bilateral_tables, refine_probs  # noqa: F401
from .superpixels import SuperpixelGraph, connect_regions, lab_tables, region_adjacency, region_features, region_pool, slic_labels, superpixel_graph  # noqa: F401
from .graphcut import GraphCut, MultiCut, cut_capacities, cut_energy, cut_energy_multi, graph_cut, graph_cut_multi, label_costs  # noqa: F401
from .mincut import MinCutRefinement, PatchSegmentPredictor  # noqa: F401
from .patch_graph import PatchGraphConstructor  # noqa: F401
from .patch_inputs import patch_labels, patch_node_features  # noqa: F401
from .region import FeatureFusion, region_edge_index, region_fuse, region_mean_pool, region_stage  # noqa: F401
from .unet import ConvBlock, DecoderBlock, UNet, UNetDecoder, UNetEncoder  # noqa: F401
from ._lib import build, lib  # noqa: F401

__all__ = ["SuperpixelGraph", "connect_regions", "lab_tables", "region_adjacency", "region_features", "region_pool", "slic_labels", "superpixel_graph", "TVLoss", "dice_loss", "lovasz_softmax", "pixel_cross_entropy", "class_weights", "FeatureConsistencyLoss", "EllipticalShapeLoss", "ImagePreprocessor", "RandomFlipRotate", "RandomAffineColor", "RandomElasticAffineColor", "bspline_weights_q14", "elastic_control", "elastic_field", "affine_fixed", "color_matrix_q12", "luma_sums", "draw_flip_rotate", "pil_rotation_fixed", "EdgeDetector", "HistogramEqualizer", "GaussianSmoother", "gaussian_kernel_q8", "patch_smooth_features_u8", "CLAHE", "patch_clahe_features_u8",
           "patch_features_u8", "patch_node_features", "patch_labels", "postprocess_segmentation", "DetectionHead", "FeatureFusion", "region_stage", "region_mean_pool", "region_fuse", "region_edge_index", "MinCutRefinement", "PatchSegmentPredictor", "graph_cut", "cut_capacities", "cut_energy", "GraphCut", "graph_cut_multi", "label_costs", "cut_energy_multi", "MultiCut", "UNet", "UNetEncoder", "UNetDecoder", "ConvBlock", "DecoderBlock", "GATNetwork", "MultiHeadGATLayer",
           "GraphAttentionLayer", "PatchGraphConstructor", "MinGraphUNet", "MinGraphUNetE2E", "segment_batch", "argmax_classes",
           "gat_forward_csr", "shard_batch", "segmentation_metrics", "metrics_from_confusion", "SegmentationEvaluator", "evaluate_segmentation",
           "allreduce_eval_state", "clean_masks", "connected_components", "border_distances", "border_weights", "ObjectTable", "yield_estimation_metrics", "YieldEvaluator", "evaluate_yield", "object_shapes", "ObjectShapes", "object_overlaps", "OverlapTable", "match_masks", "panoptic_totals", "instance_metrics", "object_detection_mAP", "InstanceEvaluator", "evaluate_instances", "encode_masks", "runs_from_coco", "labels_from_runs", "rle_to_string", "rle_from_string", "RunTable", "object_outlines", "OutlineTable", "rasterize_polygons", "objects_from_annotations", "boundary_tables", "BoundaryTables", "boundary_metrics", "BoundaryEvaluator", "evaluate_boundaries", "frame_shifts", "link_objects", "track_ids", "VideoCounter", "count_video", "predict_tta", "object_scores", "predict_tiled", "tile_grid", "tile_weights", "refine_probs", "bilateral_tables", "EdgeRefiner", "Trainer", "E2ETrainer", "FlatAdam", "StepLR", "CosineAnnealingLR", "ReduceLROnPlateau", "trainer_from_config", "scheduler_from_config", "adam_state_dict", "allreduce_mean_", "load_config", "get_config_recursively", "build_from_config", "build", "lib"]
