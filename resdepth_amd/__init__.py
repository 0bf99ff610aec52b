"""resdepth_amd -- MI355X-native (gfx950) implementation of the ResDepth U-Net training hot path.

Python host surface mirroring the reference (UNet / Trainer / batch dict), hand-written HIP kernels
underneath (libresdepth_hip.so, C ABI in include/resdepth_hip.h).  No CPU fallback.
"""
from .unet import UNet, SkipConnection  # noqa: F401
from .loss import MaskedL1Loss, MaskedLoss, masked_l1_loss, masked_loss  # noqa: F401
from .optim import FusedAdam, FusedSGD, get_optimizer  # noqa: F401
from .trainer import Trainer, AverageMeter, DevicePrefetcher  # noqa: F401
from .graph import GraphedTrainStep  # noqa: F401
from .plan import PlannedTrainStep  # noqa: F401
from .data import SyntheticDsmOrthoDataset, synthetic_batch  # noqa: F401
from .inference import predict_linear_blend, SyntheticRasterTiles  # noqa: F401
from .ensemble import PairSweep, predict_pairs_linear_blend  # noqa: F401
from .sampler import GpuGridTiles, GpuPatchSampler, GpuTrainSet, GpuValSet, SamplerLoader  # noqa: F401
from . import normalization  # noqa: F401
from .evaluation import (dilate_mask, dsm_slope, error_map, evaluate_binned, evaluate_pairs_performance,  # noqa: F401
                         evaluate_pairs_statistics, evaluate_performance, evaluate_statistics, get_statistics_masked,
                         print_binned, print_statistics)
from .coregistration import coregister, estimate_shift, translate  # noqa: F401
from .morphology import buffer_mask, distance_transform, edge_distance, fill_voids  # noqa: F401
from .ortho import RPC, orthorectify, project_grid  # noqa: F401
from .factories import (get_loss, get_model, get_scheduler, get_trainer, valid_tile_size,  # noqa: F401
                        validate_tile_size)

__all__ = ["UNet", "SkipConnection", "MaskedL1Loss", "masked_l1_loss", "MaskedLoss", "masked_loss", "FusedAdam", "FusedSGD", "get_optimizer", "Trainer", "AverageMeter", "DevicePrefetcher", "GraphedTrainStep", "PlannedTrainStep",
           "SyntheticDsmOrthoDataset", "synthetic_batch", "predict_linear_blend", "SyntheticRasterTiles", "predict_pairs_linear_blend", "PairSweep",
           "GpuPatchSampler", "SamplerLoader", "GpuGridTiles", "GpuTrainSet", "GpuValSet", "normalization", "get_loss", "get_model", "get_scheduler", "get_trainer", "valid_tile_size", "validate_tile_size",
           "dilate_mask", "evaluate_statistics", "evaluate_performance", "print_statistics", "get_statistics_masked",
           "evaluate_pairs_statistics", "evaluate_pairs_performance", "dsm_slope", "error_map", "evaluate_binned", "print_binned",
           "estimate_shift", "coregister", "translate", "distance_transform", "edge_distance", "buffer_mask", "fill_voids",
           "RPC", "orthorectify", "project_grid"]
