"""factorizer_amd — MI355X-native drop-in for the hot path of pashtari/factorizer.

``import factorizer_amd as ft`` exposes the reference's flat names for that path
(factorizer/__init__.py:1-6): ft.NMF, ft.SWMatricize, ft.FactorizerBlock, ft.Factorizer, ...
Device tensors run hand-written gfx950 kernels through libfactorizer_hip.so
(include/factorizer_hip.h); there is no silent fallback when the library is missing.
"""
from .utils import as_tuple, has_args, is_partializable, partialize
from .matricize import Matricize, Reshape, SWMatricize
from .nmf import (NMF, SVD, BCDSolver, Compose, CoordinateDescent, FastMultiplicativeUpdate, Initializer,
                  LeastSquares, MatrixFactorization, MultiplicativeUpdate, NNDSVDInit, ProjectedGradient,
                  RandomInit, SemiMultiplicativeUpdate, SVDInit, WeightedMultiplicativeUpdate, relative_error)
from .layers import MLP, LayerNorm, Linear, PosEmbed, PositionalEmbedding
from .convs import Conv2d, Conv3d, ConvTranspose2d, ConvTranspose3d
from .instance_norm import InstanceNorm1d, InstanceNorm2d, InstanceNorm3d, convert_instance_norm, instance_norm
from .group_norm import GroupNorm, convert_group_norm, group_norm
from .cnn import BasicBlock, DoubleConv, PreActivationBlock, SepConv
from .blocks import FactMixer, FactorizerBlock, FactorizerStage
from .losses import (DeepSupervisionLoss, DiceCELoss, deep_supervision_loss, dice_bce_loss, dice_ce_loss,
                     dice_ce_softmax_loss, dice_ce_softmax_loss_composed)
from .metrics import (DiceMetric, HausdorffDistanceMetric, dice_metric, discretize, hausdorff_distance, mask_edges,
                      multiclass_counts, one_hot_mask, segmentation_counts)
from .augment import (AugmentParams, BatchAugment, RandCropAugment, affine_resample, augment_batch, crop_augment_batch,
                      draw_augment_params, draw_crop_origins, gaussian_noise_field, gaussian_smooth)
from .volume import (BRATS_CLASSES, BRATS_LABEL_VALUES, PreparedVolume, foreground_bbox, normalize_intensity, prepare_volume,
                     restore_prediction)
from .respace import (ResampleGeometry, SpacedVolume, orientation_of, prepare_spaced_volume, resample_volume,
                      restore_spaced_prediction, spacing_geometry)
from .training import FlatAdamW, WarmupCosineSchedule, load_checkpoint, load_checkpoints
from .parallel import FlatGradSync
from .inference import SlidingWindowInferer, SlidingWindowInfererAdapt, sliding_window_inference
from .ushape import (Factorizer, Same, UNet, UNetDecoder, UNetDecoderBlock, UNetEncoder,
                   UNetEncoderBlock, UNetStage)
from .deconver import Deconv, DeconvInitializer, DeconvMixer, Deconver, DeconverBlock, DeconverStage, Stem

__version__ = "0.1.0"
