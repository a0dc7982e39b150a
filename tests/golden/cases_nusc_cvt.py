"""The nuScenes CVT case (config/model/cvt.yaml: Encoder + Decoder + CrossViewTransformer) shared by make_golden_nusc_cvt.py
(gv20_nuscenes_cvt.npz) and the tests: constructor arguments, procedural inputs and the test-side oracle composition.

cvt.yaml's encoder is the OPV2V CVT encoder on an EfficientNet-B4 backbone with the extrinsics inverted in the model, so the
composition is oracle.cvt's cross_view_attention / bev_grid, oracle.resnet's bottleneck and oracle.nuscenes' decoder - oracle/
itself has no function for this model."""
import copy

import torch.nn.functional as F

from cobevt_amd import synth
import oracle.cvt as o_cvt
import oracle.nuscenes as o_nu
from oracle.resnet import bn_eval, bottleneck_forward

SEED = 0
IMAGE = (224, 480)
LAYER_NAMES = ["reduction_2", "reduction_4"]
FEATURE_SHAPES = [(32, 56, 120), (112, 14, 30)]          # EfficientNet-B4 reduction_2 / reduction_4 at 224 x 480
NUSC_CVT = dict(
    encoder=dict(
        dim=128, scale=1.0, middle=[2, 2],
        cross_view=dict(heads=4, dim_head=32, qkv_bias=True, skip=True, no_image_features=False,
                        image_height=IMAGE[0], image_width=IMAGE[1]),
        bev_embedding=dict(sigma=1.0, bev_height=200, bev_width=200, h_meters=100.0, w_meters=100.0, offset=0.0,
                           decoder_blocks=[128, 128, 64])),
    decoder=dict(dim=128, blocks=[128, 128, 64], residual=True, factor=2),
    dim_last=64, outputs={"bev": [0, 1], "center": [1, 2]})


def config():
    return copy.deepcopy(NUSC_CVT)


def inputs():
    """(backbone feature maps [(6, 32, 56, 120), (6, 112, 14, 30)], image (1, 6, 3, 224, 480), intrinsics, extrinsics (ego -> camera))"""
    feats, image, intr, ext = synth.nuscenes_inputs("gv20", SEED)
    return [feats[0], feats[2]], image, intr, ext


def build(modules, backbone, cfg=None):
    """modules: the reference's cross_view_transformer.model namespace or cobevt_amd.host.nuscenes (same class names / arguments);
    -> CrossViewTransformer(Encoder(backbone, ...), Decoder(...)) in eval mode"""
    c = config() if cfg is None else cfg
    enc = modules.Encoder(backbone, **c["encoder"])
    return modules.CrossViewTransformer(enc, modules.Decoder(**c["decoder"]), c["dim_last"], c["outputs"]).eval()


def oracle_encoder(sd, pfx, cfg, features, intrinsics, extrinsics):
    """Encoder.forward (encoder.py:319-337) after the backbone: features list of (b*n, C, h, w) -> (b, d, H, W)"""
    b, n = intrinsics.shape[:2]
    I_inv, E_inv = intrinsics.inverse(), extrinsics.inverse()            # both inverted in the model (:323-324)
    grid = o_cvt.bev_grid(**cfg["bev_embedding"])
    x = sd[pfx + "bev_embedding.learned_features"]
    x = x[None].expand(b, *x.shape)
    for i, feature in enumerate(features):
        feature = feature.reshape(b, n, *feature.shape[1:])
        x = o_cvt.cross_view_attention(sd, pfx + "cross_views.%d." % i, cfg["cross_view"], x, grid, feature, I_inv, E_inv)
        for j in range(cfg["middle"][i]):
            x = bottleneck_forward(sd, pfx + "layers.%d.%d." % (i, j), x)
    return x


def oracle_model(sd, cfg, features, intrinsics, extrinsics):
    """CrossViewTransformer.forward (cvt.py:35-40) on this encoder -> ({name: logits}, encoder output)"""
    x = oracle_encoder(sd, "encoder.", cfg["encoder"], features, intrinsics, extrinsics)
    y = o_nu.decoder(sd, "decoder.", len(cfg["decoder"]["blocks"]), x)
    z = F.relu(bn_eval(F.conv2d(y, sd["to_logits.0.weight"], padding=1), sd, "to_logits.1"))
    z = F.conv2d(z, sd["to_logits.3.weight"], sd["to_logits.3.bias"])
    return {k: z[:, a:b] for k, (a, b) in cfg["outputs"].items()}, x


def oracle_from_images(sd, cfg, image, intrinsics, extrinsics):
    """the same with the backbone: oracle.efficientnet on the normalised images"""
    import oracle.efficientnet as o_eff
    feats = o_eff.efficientnet_extractor(sd, "encoder.backbone.", LAYER_NAMES, o_nu.normalize(image.flatten(0, 1)))
    return oracle_model(sd, cfg, feats, intrinsics, extrinsics)
