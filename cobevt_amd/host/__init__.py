"""Host-side mirror of the reference's nn.Module interface for the FAX hot path."""
from .runtime import compute_dtype, get_compute_dtype, get_compute_mode, get_matrix_path, set_compute_dtype  # noqa: F401
from .fax_modules import (Attention as FaxAttention, BEVEmbedding, Bottleneck, CrossViewSwapAttention,  # noqa: F401
                          CrossWinAttention, FAXModule, generate_grid, get_view_matrix)
from .swap_fusion_modules import (Attention as SwapAttention, SwapFusionBlock, SwapFusionBlockMask,  # noqa: F401
                                  SwapFusionEncoder)
from .base_transformer import (BaseEncoder, BaseTransformer, CavAttention, CavPositionalEncoding, FeedForward, HGTCavAttention, PreNorm,  # noqa: F401
                               PreNormResidual, RelTemporalEncoding, RTE)  # noqa: F401
from .resnet_ms import ResnetEncoder  # noqa: F401
from .naive_decoder import NaiveDecoder  # noqa: F401
from .naive_compress import NaiveCompressor  # noqa: F401
from .bev_seg_head import BevSegHead  # noqa: F401
from .fuse_utils import regroup  # noqa: F401
from .corpbevt import STTF, CorpBEVT  # noqa: F401
from .fax_fused_transformer import FaxFusedTransformer  # noqa: F401
from .cvt_modules import CrossAttention, CrossViewAttention, CrossViewModule  # noqa: F401
from .cross_view_transformer import CrossViewTransformer  # noqa: F401
from .cross_view_transformer_swap_fuse import CrossViewTransformerSwapFuse  # noqa: F401
from .cross_view_transformer_fcooper import CrossViewTransformerFcooper  # noqa: F401
from .cross_view_transformer_att_fuse import CrossViewTransformerAttFuse  # noqa: F401
from .v2v_fuse import ConvGRU, DiscoNetFusion, PixelWeightedFusionSoftmax, V2VNetFusion  # noqa: F401
from .cross_view_transformer_v2vnet import CrossViewTransformerV2VNet  # noqa: F401
from .cross_view_transformer_disconet import CrossViewTransformerDiscoNet  # noqa: F401
from .pillar_vfe import PFNLayer, PillarVFE  # noqa: F401
from .point_pillar_scatter import PointPillarScatter  # noqa: F401
from .sp_voxel_preprocessor import SpVoxelPreprocessor  # noqa: F401
from .sp_voxel_preprocessor_3d import SpVoxelPreprocessor3D  # noqa: F401
from .base_bev_backbone import BaseBEVBackbone  # noqa: F401
from .point_pillar_fusebevt import PointPillarFuseBEVT  # noqa: F401
from .self_attn import AttFusion  # noqa: F401
from .auto_encoder import AutoEncoder  # noqa: F401
from .att_bev_backbone import AttBEVBackbone  # noqa: F401
from .point_pillar_intermediate import PointPillarIntermediate  # noqa: F401
from .mean_vfe import MeanVFE  # noqa: F401
from .sparse_backbone_3d import SparseConv3d, SubMConv3d, VoxelBackBone8x  # noqa: F401
from .height_compression import HeightCompression  # noqa: F401
from .pipeline import CapturedCall, CapturedCorpBEVT, HostFrameFeeder, PipelinedCorpBEVT  # noqa: F401
# the data formats either side of the path
from .camera_bev_postprocessor import CameraBevPostprocessor  # noqa: F401
from .voxel_postprocessor import VoxelPostprocessor  # noqa: F401
from .bev_preprocessor import BevPreprocessor  # noqa: F401
from .lidar_bev_postprocessor import LidarBevPostprocessor  # noqa: F401
from .data_augmentor import DataAugmentor  # noqa: F401
from .pcd_utils import shuffle_order  # noqa: F401
from . import eval_utils  # noqa: F401
from .eval_utils import calculate_ap, caluclate_tp_fp, eval_final_results, voc_ap  # noqa: F401
from .rgb_preprocessor import RgbPreProcessor  # noqa: F401
from .intermediate_fusion_dataset import collate_batch  # noqa: F401
from .train_utils import load_saved_model, setup_lr_schedular, setup_optimizer, to_device  # noqa: F401
from .optim import FusedAdam, FusedAdamW  # noqa: F401
from .lr_scheduler import CosineLRScheduler  # noqa: F401
from .seg_utils import cal_iou_training, mean_IU, mean_precision  # noqa: F401
from .vanilla_seg_loss import VanillaSegLoss  # noqa: F401
from .point_pillar_loss import PointPillarLoss  # noqa: F401
from .train_graph import CapturedTrainStep  # noqa: F401
# the train()-mode forwards (host.training.pillar_vfe / point_pillar_scatter / point_pillar_fusebevt, and mean_vfe / voxel_backbone8x /
# height_compression of the SECOND-style encoder) are functions of host.training
from . import training  # noqa: F401,E402
