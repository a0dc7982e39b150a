"""nuScenes models — mirror of nuscenes/cross_view_transformer/model/{encoder_pyramid_axial.py, encoder.py, cvt.py, decoder.py}
(hydra `_target_` classes of config/model/cvt_pyramid_axial.yaml, SinBEVT on the FAX hot path, and config/model/cvt.yaml, the original
Cross-View Transformer on the CVT operators)."""
from .encoder_pyramid_axial import Normalize, PyramidAxialEncoder  # noqa: F401
from .encoder import BEVEmbedding, CrossAttention, CrossViewAttention, Encoder  # noqa: F401
from .decoder import Decoder, DecoderBlock  # noqa: F401
from .cvt import CrossViewTransformer  # noqa: F401
from .efficientnet import EfficientNetExtractor  # noqa: F401
from .metrics import BaseIoUMetric, IoUMetric  # noqa: F401
from .transforms import LoadDataTransform, Sample  # noqa: F401
from .losses import BinarySegmentationLoss, CenterLoss, MultipleLoss, SigmoidFocalLoss  # noqa: F401
