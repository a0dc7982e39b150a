"""Thin tensor-level wrappers over the C ABI (include/cobevt_hip.h) + host-side weight preparation.

torch is used for device memory, streams and one-time weight folding only; every arithmetic op of the
forward path is a HIP kernel launched through ctypes.  All functions require CUDA (ROCm) tensors and raise
otherwise — there is no CPU path here (the CPU restatement lives in oracle/ and is test infrastructure).
"""
import ctypes
import os
import math
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import lib as _L
from .lib import CobevtHipError

BF16, FP32 = 0, 1
USE_CONV3X3 = True   # route eligible 3x3 convs to the LDS-patch kernel (tests flip this to cover both paths)
USE_CONV3_S2 = True      # 3x3 / stride-2 convs through the strip kernel instead of the generic implicit GEMM
USE_CONV3_SMALL_TILES = True   # grids below the CU count: 32-cout tiles in four-wave workgroups of one / two strips (conv3_tiling)
USE_CONV3_DS = True      # layer3.0 / layer4.0: the projection shortcut inside conv2's launch (cobevt_conv3x3_ds_wfrag_nhwc)
USE_CONV3_WFRAG = True   # ... and, where the fragment-ordered weight table exists, to the barrier-free-per-tap variant
CONV3_VARIANT = 0    # 0 = automatic tile choice of cobevt_conv3x3_wfrag_nhwc; >0 pins one (tools/conv_probe.py)
USE_GEMM_ROWS = True  # route 1x1 stride-1 convs / linears to the dense-row GEMM with fused LayerNorm
USE_GEMM_ROWS2 = False  # dense-row GEMMs through the persistent fragment-ordered kernel (cobevt_linear_rows_wfrag):
USE_GEMM_ROWS3 = True     # K <= 128 bf16 dense rows on the row-chain-style kernel (gemm_rows3.hip)
GEMM_ROWS3_MIN_M = 0
GEMM_ROWS3_MAX_K = 512     # 128: only single-tile rows take the 32-row kernel
GEMM_ROWS3_STRIDED = 1     # stride-2 1x1 convs (ResNet down-sampling) too
GEMM_ROWS3_ROWS64_MIN_M = 0   # > 0: launches with at least this many rows use 64-row workgroups
# measured 3-20 % SLOWER than two independent workgroups per CU (196 VGPRs -> one workgroup per CU, only one 32-KB tile
# of loads in flight per CU: latency-bound on HBM); kept for the parity tests and as the base for a deeper prefetch
USE_STEM_POOL = True  # stem conv + max pool in one launch (the stem map never reaches HBM)
USE_STEM = True       # 7x7/s2 image stem through the space-to-depth kernel instead of the generic small-Cin igemm
ROW_CHAIN_ROWS = 0     # rows per workgroup of the fused row chain: 0 = default (32), 64
USE_ROW_CHAIN = True  # fuse out-proj + skip + pre-norm MLP (+ post-norm) after attention into one launch (bf16)
USE_BOTTLENECK_F32 = True  # the FAX Bottleneck(128, 32) as one launch in fp32 storage (csrc/bottleneck_f32.hip; round 6)
USE_GEMM_ROWS3_F32 = True  # dense-row GEMMs of the fp32 modes on 32-row workgroups with fragment-ordered weights (csrc/gemm_rows3_f32.hip; round 6)
USE_ROW_CHAIN_F32 = True  # ... and its fp32-storage form for C = 128 / hidden 256 (csrc/row_chain_f32.hip; round 6)
BASICBLOCK_TILE_ROWS = 0   # 0 = kernel default; 8 | 16 pins the output tile height (tools/bb_probe.py)
USE_BASICBLOCK = True  # stride-1 BasicBlocks on 64 / 128 channels as one launch (intermediate map stays in LDS)
BASICBLOCK_MAX_C = 128   # widest stride-1 BasicBlock run as one launch (A/B: 64 = the 128-channel blocks of layer 2 as two strip launches)
USE_DSBLOCK = True  # layer2's stride-2 BasicBlock with its projection shortcut as one launch (bf16)
USE_EMBED_GEMM = False  # compute the BEV query embedding inside the to_q GEMM instead of materialising the query:
USE_EMBED_GEMM3 = True    # the BEV query produced inside the launch that projects it.  128 -> 128 with LayerNorm (every OPV2V level): the
                          # wave-level kernel of bev_query.hip (rows in registers, weights in LDS); other widths keep the embedding
                          # kernel + GEMM - inside the 32-row GEMM of gemm_rows3.hip the staging threads become VALU-bound (3 % slower)
# measured SLOWER on MI355X (119 vs 92 us on the level-0 shape, 361 vs 364 frames/s): the producer's 64 LDS
# coefficient reads + ~400 VALU per thread cost more than the 170 MB of HBM traffic they save; kept for parity tests
USE_CHAIN_NEXT = True  # ... and let the row-local GEMM that consumes its output next ride in the same launch
USE_HEAD_CONV = True    # 3x3 convs with <= 4 output channels to NCHW fp32 logits (BevSegHead) on the direct kernel
USE_PROJ_CHAIN = True   # FAX key / value side at 128 feature channels: BN -> ReLU -> 1x1 conv (+ ray embedding) -> LayerNorm -> to_k | to_v
                        # of both attentions in ONE launch per operand, the key / value map itself never reaches HBM (row_chain.hip)
USE_PROJ_CHAIN_KV = True     # FAX key AND value side of a level with 256 / 384 / 512 feature channels in ONE launch (proj_chain_k.hip) instead of four
USE_PROJ_CHAIN_WAVE = True   # ... on maps of >= 32768 rows as independent waves with the rows in registers and the weights in LDS (proj_chain128.hip)
USE_SWAP_STAGE = True   # a SwapFusionBlock half (attention + row chain + next to_qkv) as one launch (swap_stage.hip)
USE_BOTTLENECK = True   # FAX ResNetBottleNeck (128 -> 32 -> 32 -> 128) as one launch (bottleneck.hip) instead of three
ATTN_VARIANT = 0    # 0 = automatic (K/V-resident attention kernel where it applies), 1 = always the streaming kernel, 2 = ... with 64-key tiles (A/B runs)
USE_ATTN_BIG_RESIDENT = False  # True only SUPPRESSES the key split for plain bf16 windows of 513 .. 1024 keys, nothing more.  Which kernel such a window
                               # takes is decided in C (csrc/attn_select.hpp), whose gate COBEVT_ATTN_BIG is ON by default: unsplit, it runs on the
                               # K/V-resident kernel in one launch with or without this flag.  Split vs. unsplit measured neutral (659.0 / 659.7 /
                               # 668.2 vs 659.2 / 660.3 / 660.5 frames/s, one frame 1.900 vs 1.904 ms, profiles/r06_attn_big_resident_ab.txt):
                               # the key split stays the default
ATTN_KSPLIT = 2     # streaming attention on a small grid with >= 1024 keys (FAX level 2 / global attention): share the keys of a window out
                    # over this many workgroups per query tile + a merge pass (0 / 1 = off).  Round 3 measured it neutral (0 / 2 / 4 =
                    # 582 / 578 / 569 frames/s, profiles/r03_ab_key_split.txt) and left it off; with the round-5 pipeline 2 is a small
                    # consistent gain: 0 / 2 / 4 = 590.9 / 598.3 / 593.0 and 591.4 / 595.2 / 593.4 frames/s, one frame 2.037 / 2.033 /
                    # 2.037 ms (profiles/r05_ab_same_job.txt); parity-tested (tests/test_kernels_gpu.py::test_attention_key_split_matches_single_pass)
ATTN_QSPLIT = 0     # 0 = automatic query split of the resident attention kernel; > 0 pins it (tools/attn_probe.py)

# the integer knobs above (everything else COBEVT_FLAGS accepts is a USE_* boolean)
INT_KNOBS = ("CONV3_VARIANT", "BASICBLOCK_TILE_ROWS", "ROW_CHAIN_ROWS", "GEMM_ROWS3_MIN_M", "GEMM_ROWS3_MAX_K", "GEMM_ROWS3_STRIDED",
             "GEMM_ROWS3_ROWS64_MIN_M", "BASICBLOCK_MAX_C", "ATTN_VARIANT", "ATTN_QSPLIT", "ATTN_KSPLIT")


def dcode(dtype):
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.float32:
        return FP32
    raise CobevtHipError("compute dtype must be torch.bfloat16 or torch.float32, got %s" % dtype)


def _apply_env_flags():
    """COBEVT_FLAGS="USE_EMBED_GEMM=0,CONV3_VARIANT=150": A/B switches for bench runs (every flag names a HIP path)."""
    for item in os.environ.get("COBEVT_FLAGS", "").split(","):
        if "=" in item:
            k, v = item.split("=", 1)
            k = k.strip()
            if k not in globals() or not (k.startswith("USE_") or k in INT_KNOBS):
                raise CobevtHipError("COBEVT_FLAGS: unknown switch %r" % k)
            globals()[k] = int(v) if not k.startswith("USE_") else bool(int(v))


_apply_env_flags()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise CobevtHipError("cobevt_amd kernels need tensors on a ROCm device (got a CPU tensor); "
                                 "there is no CPU fallback")


def _ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


# ----------------------------------------------------------------------------------------------
# optional per-launch timing (bench.py roofline leg): HIP events on the launch stream around each C-ABI call
# ----------------------------------------------------------------------------------------------
_PROFILE = None


class LaunchProfile(object):
    """with LaunchProfile() as prof: model(batch) -> prof.summary(): {family: {calls, ms, flops, bytes}}"""

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _PROFILE
        _PROFILE = self
        return self

    def __exit__(self, *exc):
        global _PROFILE
        _PROFILE = None

    def summary(self, by_shape=False):
        torch.cuda.synchronize()
        out = {}
        for fam, flops, nbytes, e0, e1 in self.records:
            if not by_shape:
                fam = fam.split("|")[0]
            d = out.setdefault(fam, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["calls"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


class _Timed(object):
    __slots__ = ("fam", "flops", "nbytes", "e0")

    def __init__(self, fam, flops, nbytes):
        self.fam, self.flops, self.nbytes = fam, flops, nbytes

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e0.record()

    def __exit__(self, *exc):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        _PROFILE.records.append((self.fam, self.flops, self.nbytes, self.e0, e1))


class _NoTime(object):
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


_NOTIME = _NoTime()


def _timed(fam, flops_fn):
    """flops_fn() -> (algorithmic flops, algorithmic bytes); only evaluated while profiling."""
    if _PROFILE is None:
        return _NOTIME
    f, b = flops_fn()
    return _Timed(fam, f, b)


# ----------------------------------------------------------------------------------------------
# weight preparation (host, once per module/dtype)
# ----------------------------------------------------------------------------------------------
def bn_affine(bn):
    """Eval-mode BatchNorm as per-channel (scale, shift) in float64."""
    g = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(bn.running_var).double()
    b = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(bn.running_var).double()
    s = g / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s, b - bn.running_mean.detach().double() * s


class ConvPlan(object):
    """A conv / linear layer lowered to the implicit-GEMM kernel: folded, re-laid-out weights + static params."""

    def __init__(self, weight, bias=None, bn=None, pre_bn=None, pre_relu=False, stride=1, pad=0, act=0,
                 upsample=False, store_mode=0, dtype=torch.bfloat16, device="cuda", smallc=False, ln=None,
                 ln_folded_eps=None, pad_br=None):
        """ln = nn.LayerNorm-like (weight, bias, eps) applied to the input rows of a Linear / 1x1 layer: its affine
        is folded here (W' = W diag(gamma), b' = b + W beta) so the kernels only have to normalise."""
        w = weight.detach().double().cpu()
        if w.dim() == 2:
            w = w[:, :, None, None]
        cout, cin, kh, kw = w.shape
        # pad = zero rows / columns before the first input pixel (top, left); pad_br = after the last one (bottom, right) when
        # it differs - TensorFlow-"same" padding of the EfficientNet stem.  Only the generic implicit GEMM takes the
        # asymmetric form (its gather bounds-checks every tap).
        asym = pad_br is not None and int(pad_br) != int(pad)
        self.pad_br = int(pad if pad_br is None else pad_br)
        b = bias.detach().double().cpu() if bias is not None else torch.zeros(cout, dtype=torch.float64)
        has_bias = bias is not None or bn is not None
        self.has_ln, self.ln_eps = False, 0.0
        if ln_folded_eps is not None:        # the caller already folded a LayerNorm affine into weight / bias: normalise only
            if ln is not None or kh != 1 or kw != 1 or bn is not None or pre_bn is not None:
                raise CobevtHipError("ln_folded_eps applies to plain Linear / 1x1 layers without another ln")
            self.has_ln, self.ln_eps = True, float(ln_folded_eps)
        if ln is not None:
            if kh != 1 or kw != 1 or bn is not None or pre_bn is not None:
                raise CobevtHipError("LayerNorm folding applies to plain Linear / 1x1 layers")
            g, be = ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu()
            b = b + (w[:, :, 0, 0] @ be)
            w = w * g[None, :, None, None]
            has_bias = True
            self.has_ln, self.ln_eps = True, float(ln.eps)
        if bn is not None:
            s, sh = bn_affine(bn)
            s, sh = s.cpu(), sh.cpu()
            w = w * s[:, None, None, None]
            b = b * s + sh
        self.dtype = dtype
        self.code = dcode(dtype)
        bke = 32 if self.code == BF16 else 16
        ch = 8 if self.code == BF16 else 4
        K = kh * kw * cin
        kpad = (K + bke - 1) // bke * bke
        wk = torch.zeros(cout, kpad, dtype=torch.float64)
        wk[:, :K] = w.permute(0, 2, 3, 1).reshape(cout, K)
        self.wgt = wk.to(torch.float32).to(dtype).to(device).contiguous()
        self.bias = b.to(torch.float32).to(device).contiguous() if has_bias else None
        self.pre_scale = self.pre_shift = None
        if pre_bn is not None:
            s, sh = bn_affine(pre_bn)
            self.pre_scale = s.to(torch.float32).to(device).contiguous()
            self.pre_shift = sh.to(torch.float32).to(device).contiguous()
        self.pre_relu = int(bool(pre_relu))
        self.klut = None
        self.smallc = int(bool(smallc))
        if not smallc and cin % ch != 0:
            raise CobevtHipError("Cin=%d must be a multiple of %d for the %s kernel (use smallc=True for image "
                                 "inputs)" % (cin, ch, dtype))
        if smallc:
            k = torch.arange(kpad)
            tap, c = k // cin, k % cin
            code = ((tap // kw) << 20) | ((tap % kw) << 10) | c
            code[k >= K] = -1
            self.klut = code.to(torch.int32).to(device).contiguous()
        # 3x3 / stride 1 / pad 1 fast path (conv3x3.hip): weights [Cout][Cin/cc][9][cc]
        self.wgt3, self.cc3 = None, 0
        if kh == 3 and kw == 3 and int(stride) in (1, 2) and int(pad) == 1 and not asym and int(act) <= 2 and not smallc and pre_bn is None \
                and int(store_mode) in (0, 1) and not (int(stride) == 2 and (upsample or int(store_mode) != 0)):
            cands = (64, 32) if self.code == BF16 else (32, 16)
            for cc in cands:
                if cin % cc == 0:
                    w3 = w.permute(0, 2, 3, 1).reshape(cout, 9, cin // cc, cc).permute(0, 2, 1, 3)
                    if int(stride) == 1:          # the LDS-staged kernel is stride 1 only
                        self.wgt3 = w3.to(torch.float32).to(dtype).to(device).contiguous()
                    self.cc3 = cc
                    break
        # the same weights in MFMA B-fragment order for cobevt_conv3x3_wfrag_nhwc (128-byte chunks only):
        # [Cout_p/32][Cin/cc][9][KG][lane = 32*half + cout%32][16 bytes], Cout zero-padded to a multiple of 128
        self.wfrag, self.coutp3 = None, 0
        if self.cc3 and self.cc3 == (64 if self.code == BF16 else 32):
            cc, coutp = self.cc3, (cout + 127) // 128 * 128
            wp = torch.zeros(coutp, cin // cc, 9, cc, dtype=torch.float64)
            wp[:cout] = w.permute(0, 2, 3, 1).reshape(cout, 9, cin // cc, cc).permute(0, 2, 1, 3)
            wf = wp.reshape(coutp // 32, 32, cin // cc, 9, 4, 2, ch).permute(0, 2, 3, 4, 5, 1, 6)
            self.wfrag = wf.to(torch.float32).to(dtype).to(device).contiguous()
            self.coutp3 = coutp
        # ResNet stem fast path (stem7x7.hip): 7x7 / stride 2 / pad 3 on 3 channels as a 4x4 conv on the 2x2
        # space-to-depth image; W'[n][a][b][dy][dx][c] = w[n][c][2a+dy-1][2b+dx-1]
        self.wgt_stem = None
        if smallc and kh == 7 and kw == 7 and int(stride) == 2 and int(pad) == 3 and not asym and int(act) <= 2 and cin == 3 and pre_bn is None \
                and int(store_mode) == 0 and not upsample and cout % (8 if self.code == BF16 else 4) == 0:
            ws = torch.zeros(cout, 4, 4, 16, dtype=torch.float64)
            for a in range(4):
                for bb in range(4):
                    for dy in range(2):
                        for dx in range(2):
                            ih, iw = 2 * a + dy - 1, 2 * bb + dx - 1
                            if 0 <= ih < 7 and 0 <= iw < 7:
                                ws[:, a, bb, dy * 6 + dx * 3:dy * 6 + dx * 3 + 3] = w[:, :, ih, iw]
            self.wgt_stem = ws.reshape(cout, 256).to(torch.float32).to(dtype).to(device).contiguous()
        # dense-row GEMM fast path (gemm_rows.hip) for 1x1 / stride 1: weights [Cout][K rounded to a 256-byte tile]
        self.wgt_rows, self.kp_rows, self.wfrag_rows = None, 0, None
        if kh == 1 and kw == 1 and int(stride) in (1, 2) and int(pad) == 0 and not asym and not smallc and int(store_mode) == 0 \
                and not upsample:
            tk = 128 if self.code == BF16 else 64
            kp = (K + tk - 1) // tk * tk
            wr = torch.zeros(cout, kp, dtype=torch.float64)
            wr[:, :K] = w.reshape(cout, K)
            self.wgt_rows = wr.to(torch.float32).to(dtype).to(device).contiguous()
            self.kp_rows = kp
            # the same matrix in MFMA fragment order for the fused row chain (row_chain.hip):
            # [N_p/32 tiles][kp/16 k-groups][lane = 32*half + n%32][8 bf16], N zero-padded to a multiple of 128
            eg = 8 if self.code == BF16 else 4          # elements per 16 bytes
            npad = (cout + 127) // 128 * 128
            wp_ = torch.zeros(npad, kp, dtype=torch.float64)
            wp_[:cout] = wr
            wf = wp_.reshape(npad // 32, 32, kp // (2 * eg), 2, eg).permute(0, 2, 3, 1, 4)
            self.wfrag_rows = wf.to(torch.float32).to(dtype).to(device).contiguous()
        # BevSegHead-style 3x3 convs with 1..4 output channels to fp32 NCHW logits: a direct kernel (postprocess.hip)
        self.wgt_head = None
        if kh == 3 and kw == 3 and int(stride) == 1 and int(pad) == 1 and not asym and not smallc and int(store_mode) == 2 and int(act) == 0 \
                and not upsample and pre_bn is None and cout <= 4 and cin * (2 if self.code == BF16 else 4) <= 256 and cin % ch == 0:
            self.wgt_head = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).to(torch.float32).to(device).contiguous()
        self.cin, self.cout, self.kh, self.kw = cin, cout, kh, kw
        self.K, self.kpad = K, kpad
        self.stride, self.pad, self.act = int(stride), int(pad), int(act)
        self.upsample = int(bool(upsample))
        self.store_mode = int(store_mode)

    def out_hw(self, h, w):
        hv, wv = (2 * h, 2 * w) if self.upsample else (h, w)
        return ((hv + self.pad + self.pad_br - self.kh) // self.stride + 1,
                (wv + self.pad + self.pad_br - self.kw) // self.stride + 1)


def ln_fusable(plan):
    """The row normalisation can run inside the dense-row GEMM when the row fits one 256-byte K-tile."""
    return USE_GEMM_ROWS and plan.wgt_rows is not None and plan.K <= (128 if plan.code == BF16 else 64)


def conv3_tiling(n, ho, wo, cin, cout, cc, cus=256, stride=1, bf16=True, packed=0):
    """Pick the 3x3 kernel / tile shape for one launch: 0 = the LDS-staged kernel (cobevt_conv3x3_nhwc), else the
    `variant` of cobevt_conv3x3_wfrag_nhwc (100 + 10*MT + bn64: MT strips of 2x16 pixels x 128|64 couts per workgroup).
    The LDS-staged kernel runs two workgroups per CU and wins once its grid is >= 2 per CU; below that the kernel time
    is whole workgroup lifetimes, so the strip count MT is chosen to make the grid a whole number of waves of `cus`
    workgroups (cycle model: 12k fixed + 40 cycles per MFMA-tile-step, both from the s_memtime traces)."""
    if stride == 1:
        if cout <= 32 and bf16 and cc == 64:
            # 32-cout tiles in four-wave workgroups, two per CU (a 64-cout tile would waste half its MFMAs): one round of
            # 2 * cus workgroups if the strips allow it, else the fewest strips per workgroup (tools/conv_graph_probe.py)
            nstrips = n * (-(-ho // 2)) * (-(-wo // 16))
            best = None
            for mt in ((1, 2, 3, 4, 5) if USE_CONV3_SMALL_TILES else (3, 4, 5)):
                blocks = -(-nstrips // mt) * -(-cout // 32)
                cost = -(-blocks // (2 * cus)) * (6000 + 9 * (cin // cc) * mt * 80)
                if best is None or cost < best[0]:
                    best = (cost, 100 + 10 * mt + 3)
            return best[1]
        if cout < 64:
            return 0
        th, bn = (16, 64) if cout <= 64 else (8, 128)
        blocks_old = n * (-(-ho // th)) * (-(-wo // 16)) * (-(-cout // bn))
        if blocks_old >= 2 * cus and not (packed and cout >= 128):      # (the LDS-staged kernel has no packed form)
            return 0
    nstrips = n * (-(-ho // 2)) * (-(-wo // 16))
    nsteps = 9 * (cin // cc)
    best = None
    for bn64 in ((1,) if cout <= 64 else (0, 1)):
        tile_n = 64 if bn64 else 128
        for mt in (3, 4, 5, 6):
            blocks = -(-nstrips // mt) * -(-cout // tile_n)
            # packed (third library, fp32 storage): the 128-cout tiles' waves own two k-groups per tap and issue ONE MFMA for both
            # (csrc/common.hpp kXPack); the 64-cout tiles' waves own one and cannot
            # (second library: three MFMAs per k-group pair instead of four on those tiles, kXPack3 - packed = 0.75)
            per_step = int(40 * (float(packed) if packed else 1.0)) if (packed and not bn64) else 40
            cost = -(-blocks // cus) * (12000 + nsteps * mt * (tile_n // 32) * per_step
                                       + (1500 * mt * (cin // cc) if stride == 2 else 0))   # exposed patch refills
            if best is None or cost < best[0]:
                best = (cost, 100 + 10 * mt + bn64, blocks)
    if USE_CONV3_SMALL_TILES and stride == 1 and bf16 and cc == 64 and not packed and best[2] < cus:
        # a grid that does not reach the CU count (one image: the decoder maps, the small FAX maps): the launch lasts one workgroup
        # lifetime, so the shortest workgroup wins - 32-cout tiles in four-wave workgroups with one or two strips each (round 6)
        for mt in (1, 2, 3, 4, 5):
            blocks = -(-nstrips // mt) * -(-cout // 32)
            cost = -(-blocks // (2 * cus)) * (6000 + nsteps * mt * 80)
            if cost < best[0]:
                best = (cost, 100 + 10 * mt + 3, blocks)
    return best[1]


def conv3_packed(code, lib_variant):
    """conv3_tiling's `packed`: the cost of an MFMA step of a 128-cout strip tile in an fp32-storage library (0: the native one)"""
    return {"f32h": 0.5, "f32s": 0.75}.get(lib_variant, 0) if code == FP32 else 0


def conv3_variant(n, ho, wo, cin, cout, cc, stride, bf16=True, packed=0):
    """The 3x3 kernel of one launch: CONV3_VARIANT when pinned, else conv3_tiling's choice (0, the LDS-staged kernel, is stride 1 only)"""
    variant = CONV3_VARIANT or conv3_tiling(n, ho, wo, cin, cout, cc, stride=stride, bf16=bf16, packed=packed)
    return (151 if cout <= 64 else 150) if (variant == 0 and stride == 2) else variant


ConvRoute = namedtuple("ConvRoute", "kernel ln_fused variant rows", defaults=(0, 0))
CONV_SYMBOLS = {"head": "cobevt_conv3x3_head_nchw", "stem": "cobevt_stem_conv7x7s2", "rows_small_k": "cobevt_linear_rows_small_k",
                "rows_wfrag": "cobevt_linear_rows_wfrag", "rows": "cobevt_linear_rows", "strips": "cobevt_conv3x3_wfrag_nhwc",
                "conv3": "cobevt_conv3x3_nhwc", "igemm": "cobevt_conv2d_nhwc"}


def conv_route(plan, n, h, w, out_hw=None, has_residual=False, lib_variant=""):
    """The kernel (a key of CONV_SYMBOLS) conv2d launches for `plan` on an (n, h, w) input, from the plan, the switches above and the
    arguments alone (out_hw: a preallocated result's size).  ln_fused: the LayerNorm runs inside the GEMM, not as a launch before it."""
    p, (ho, wo) = plan, plan.out_hw(h, w)
    ln, bf16, m, exact = bool(p.has_ln and ln_fusable(p)), p.code == BF16, n * ho * wo, out_hw is None or tuple(out_hw) == (ho, wo)
    if p.wgt_head is not None and USE_HEAD_CONV and exact and not has_residual:
        return ConvRoute("head", ln)
    if p.wgt_stem is not None and USE_STEM and h % 2 == 0 and w % 2 == 0 and exact and not has_residual:
        return ConvRoute("stem", ln)
    if p.wgt_rows is not None and USE_GEMM_ROWS and (exact or not has_residual):
        ch, use3, max_k = (8, USE_GEMM_ROWS3, GEMM_ROWS3_MAX_K) if bf16 else (4, USE_GEMM_ROWS3_F32, 512)
        ln_ok = not ln or (p.kp_rows <= 128 if bf16 else (p.K == 128 and p.pre_scale is None))
        s2_ok = p.stride == 1 or (not has_residual and bool(GEMM_ROWS3_STRIDED or not bf16))
        if (use3 and p.wfrag_rows is not None and exact and p.kp_rows <= max_k and p.K % ch == 0 and p.cout % ch == 0 and p.cout <= 4096
                and p.store_mode == 0 and ln_ok and s2_ok and m >= GEMM_ROWS3_MIN_M):
            return ConvRoute("rows_small_k", ln, 0, 64 if (GEMM_ROWS3_ROWS64_MIN_M and m >= GEMM_ROWS3_ROWS64_MIN_M) else 32)
        return ConvRoute("rows_wfrag" if (USE_GEMM_ROWS2 and p.wfrag_rows is not None and p.cout % ch == 0) else "rows", ln)
    # (the stride-2 strip variants sit at the 256-VGPR limit in fp32: with the operand split of the f32s library they spill
    # hundreds of registers, so that library's three stride-2 3x3 convs of a ResNet take the generic implicit GEMM)
    if p.wfrag is not None and exact and USE_CONV3X3 and USE_CONV3_WFRAG \
            and (p.stride == 1 or (USE_CONV3_S2 and not (p.code == FP32 and lib_variant == "f32s"))):
        variant = conv3_variant(n, ho, wo, p.cin, p.cout, p.cc3, p.stride, bf16, conv3_packed(p.code, lib_variant))
        if variant > 0:
            return ConvRoute("strips", ln, variant)
    return ConvRoute("conv3" if (p.wgt3 is not None and exact and USE_CONV3X3) else "igemm", ln)


def _launch_conv2d_nhwc(x, wgt, bias, residual, pre_scale, pre_shift, klut, out, ho, wo, kh, kw, stride=1, pad=0, upsample=0, pre_relu=0,
                        act=0, store_mode=0, out_hw=None, variant=None):
    (n, h, w, cin), (cout, kpad), (out_h, out_w) = x.shape, wgt.shape, out_hw or (ho, wo)
    dims = _ints([dcode(wgt.dtype), n, h, w, cin, ho, wo, cout, kh, kw, stride, pad, kh * kw * cin, kpad, upsample, pre_relu, act,
                  store_mode, out_h, out_w, klut is not None])
    _L.call("cobevt_conv2d_nhwc", _p(x), _p(wgt), _p(bias), _p(residual), _p(pre_scale), _p(pre_shift), _p(klut), _p(out), dims, _stream(),
            variant=variant)


def _launch_conv3x3(x, wgt, bias, residual, out, cout=None, tile=0, stride=1, upsample=0, act=0, store_mode=0, variant=None):
    """tile 0: cobevt_conv3x3_nhwc on plan.wgt3, else cobevt_conv3x3_wfrag_nhwc on plan.wfrag (cc, padded Cout: the table's sizes)"""
    dims = [dcode(x.dtype), *x.shape, cout if tile else wgt.shape[0], upsample, act, store_mode]
    dims += [x.shape[3] // wgt.shape[1], wgt.shape[0] * 32, tile, stride] if tile else [wgt.shape[3]]
    _L.call("cobevt_conv3x3_wfrag_nhwc" if tile else "cobevt_conv3x3_nhwc", _p(x), _p(wgt), _p(bias), _p(residual), _p(out), _ints(dims),
            _stream(), variant=variant)


def _launch_rows(x, wgt, bias, residual, pre_scale, pre_shift, out, kp=0, rows=0, wfrag=False, pre_relu=0, act=0, ln=0, ln_eps=0.0,
                 stride=1, variant=None):
    """rows > 0: cobevt_linear_rows_small_k (plan.wfrag_rows), else cobevt_linear_rows_wfrag (wfrag) or cobevt_linear_rows (plan.wgt_rows)"""
    (n, h, w, K), (out_h, out_w, cout), code = x.shape, out.shape[1:], dcode(x.dtype)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if rows:
        dims = (ctypes.c_long * 14)(code, n * ho * wo, cout, K, K, pre_relu, act, int(ln), stride, ho, wo, h, w, rows)
    else:
        dims = (ctypes.c_long * 16)(code, n * ho * wo, cout, K, kp, K, pre_relu, act, ho, wo, out_h, out_w, int(ln), stride, h, w)
    symbol = "cobevt_linear_rows_small_k" if rows else "cobevt_linear_rows_wfrag" if wfrag else "cobevt_linear_rows"
    _L.call(symbol, _p(x), _p(wgt), _p(bias), _p(residual), *(() if rows or wfrag else (None, None)), _p(pre_scale), _p(pre_shift), _p(out),
            dims, ctypes.c_float(ln_eps), _stream(), variant=variant)


def conv2d(x, plan, residual=None, out=None):
    """x: (N,H,W,Cin) channels-last contiguous in plan.dtype (fp32 image for smallc plans).  Returns the output
    in the layout selected by plan.store_mode.  `out` may be a pre-zeroed, spatially larger (N,Hp,Wp,Cout) map.
    Plans built with ln=... normalise the rows of x first (LayerNorm affine already folded into the weights)."""
    _need_cuda(x, residual, out)
    n, h, w, cin = x.shape
    if cin != plan.cin or not x.is_contiguous():
        raise CobevtHipError("conv2d: bad input %s (contiguous=%s) for Cin=%d" % (tuple(x.shape), x.is_contiguous(), plan.cin))
    if x.dtype != (torch.float32 if plan.smallc else plan.dtype):
        raise CobevtHipError("conv2d: input dtype %s does not match plan (%s, smallc=%d)" % (x.dtype, plan.dtype, plan.smallc))
    p, sm, (ho, wo), out_hw = plan, plan.store_mode, plan.out_hw(h, w), None
    if out is None:
        shape = (n, ho // 2, wo // 2, p.cout * 4) if sm == 1 else (n, p.cout, ho, wo) if sm == 2 else (n, ho, wo, p.cout)
        out = torch.empty(shape, device=x.device, dtype=p.dtype if sm in (0, 1) else torch.float32)
    else:
        if sm not in (0, 3) or out.dim() != 4 or out.shape[0] != n or out.shape[3] != p.cout or not out.is_contiguous():
            raise CobevtHipError("conv2d: incompatible `out`")
        out_hw = (out.shape[1], out.shape[2])
        if out_hw[0] < ho or out_hw[1] < wo:
            raise CobevtHipError("conv2d: `out` smaller than the convolution result")
    if residual is not None and (tuple(residual.shape) != (n, ho, wo, p.cout) or residual.dtype != p.dtype
                                 or not residual.is_contiguous()):
        raise CobevtHipError("conv2d: residual must be (N,Ho,Wo,Cout) contiguous in the compute dtype")
    def cost():
        esz = 2 if p.code == BF16 else 4
        nbytes = x.numel() * x.element_size() + p.cout * p.K * esz + out.numel() * out.element_size()
        return 2.0 * m * p.cout * p.K, float(nbytes + (0 if residual is None else residual.numel() * esz))

    r = conv_route(p, n, h, w, out_hw, residual is not None, _L.get_variant())
    k, ln, m = r.kernel, r.ln_fused, n * ho * wo
    if p.has_ln and not ln:
        x = layernorm(x, None, None, p.ln_eps)
    if k == "head":
        with _timed("head3x3|%d->%d %dx%dx%d" % (cin, p.cout, n, ho, wo), cost):
            _L.call("cobevt_conv3x3_head_nchw", _p(x), _p(p.wgt_head), _p(p.bias), _p(out), p.code, n, h, w, cin, p.cout, _stream())
    elif k == "stem":
        sdims = _ints([p.code, n, h, w, p.cout, p.act])
        with _timed("stem7x7|%dx%dx%d" % (n, h, w), cost):
            _L.call("cobevt_stem_conv7x7s2", _p(x), _p(p.wgt_stem), _p(p.bias), _p(out), sdims, _stream())
    elif k in ("strips", "conv3"):
        with _timed("conv3x3|%d->%d %dx%dx%d" % (cin, p.cout, n, ho, wo), cost):
            _launch_conv3x3(x, p.wfrag if r.variant else p.wgt3, p.bias, residual, out, cout=p.cout, tile=r.variant, stride=p.stride,
                            upsample=p.upsample, act=p.act, store_mode=sm)
    elif k == "igemm":
        with _timed("igemm|k%ds%d %d->%d M=%d%s" % (p.kh, p.stride, cin, p.cout, m, " stem" if p.smallc else ""), cost):
            _launch_conv2d_nhwc(x, p.wgt, p.bias, residual, p.pre_scale, p.pre_shift, p.klut, out, ho, wo, p.kh, p.kw, stride=p.stride,
                                pad=p.pad, upsample=p.upsample, pre_relu=p.pre_relu, act=p.act, store_mode=sm, out_hw=out_hw)
    else:
        fam = "gemm_rows|%d->%d M=%d%s%s" % (cin, p.cout, m, " ln" if ln else "", " s%d" % p.stride if p.stride > 1 else "")
        with _timed(fam + " r32" if r.rows else fam, cost):
            _launch_rows(x, p.wgt_rows if k == "rows" else p.wfrag_rows, p.bias, residual, p.pre_scale, p.pre_shift, out, kp=p.kp_rows,
                         rows=r.rows, wfrag=k == "rows_wfrag", pre_relu=p.pre_relu, act=p.act, ln=ln, ln_eps=p.ln_eps, stride=p.stride)
    return out


DECONV_MAX_STRIDE = 8


class DeconvPlan(object):
    """nn.ConvTranspose2d(Cin, Cout, s, stride=s, bias=False) (+ the eval BatchNorm that follows it) lowered to cobevt_deconv_nhwc:
    `wgt` [s*s*Cout][Kpad] with row (dy*s + dx)*Cout + co = weight[:, co, dy, dx] * bn_scale[co] (folded in float64, then rounded to the
    compute dtype; columns >= Cin zero) and `shift` fp32[Cout].  weight: (Cin, Cout, s, s), the ConvTranspose2d layout.  device="cpu"
    builds the same tensors without a GPU (the layout tests)."""

    def __init__(self, weight, bn=None, stride=1, dtype=torch.bfloat16, device="cuda", act=1):
        if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
            raise CobevtHipError("DeconvPlan: weight must be (Cin, Cout, s, s), got %s" % (tuple(weight.shape),))
        cin, cout, s, _ = (int(d) for d in weight.shape)
        if int(stride) != stride or int(stride) != s:
            raise CobevtHipError("DeconvPlan: only kernel = stride (no overlapping taps) is supported: a %d x %d kernel with stride %r" % (s, s, stride))
        if not 1 <= s <= DECONV_MAX_STRIDE:
            raise CobevtHipError("DeconvPlan: stride %d is outside 1 .. %d" % (s, DECONV_MAX_STRIDE))
        self.dtype, self.code = dtype, dcode(dtype)
        bke, ch = (32, 8) if self.code == BF16 else (16, 4)
        if cin % ch != 0:
            raise CobevtHipError("DeconvPlan: Cin=%d must be a multiple of %d for the %s kernel" % (cin, ch, dtype))
        if cout % 32 != 0:
            raise CobevtHipError("DeconvPlan: Cout=%d must be a multiple of 32 (one MFMA tile = 32 channels of one tap)" % cout)
        w = weight.detach().double().cpu()
        shift = torch.zeros(cout, dtype=torch.float64)
        if bn is not None:
            sc, shift = (t.cpu() for t in bn_affine(bn))
            w = w * sc[None, :, None, None]
        kpad = (cin + bke - 1) // bke * bke
        wk = torch.zeros(s * s * cout, kpad, dtype=torch.float64)
        wk[:, :cin] = w.permute(2, 3, 1, 0).reshape(s * s * cout, cin)
        self.wgt = wk.to(torch.float32).to(dtype).to(device).contiguous()
        self.shift = shift.to(torch.float32).to(device).contiguous()
        self.cin, self.cout, self.stride, self.kpad, self.act = cin, cout, s, kpad, int(act)


def deconv_into(x, plan, out, c_off=0):
    """x (N,H,W,Cin) contiguous in plan.dtype -> out[:, :, :, c_off : c_off + Cout] of the contiguous (N, s*H, s*W, ldc) map `out` (same
    dtype), pixel-shuffled, with the plan's shift and activation: one cobevt_deconv_nhwc launch that writes exactly that slice.
    Returns `out`."""
    p, s = plan, plan.stride
    if x.dim() != 4 or x.shape[3] != p.cin or not x.is_contiguous():
        raise CobevtHipError("deconv_into: bad input %s (contiguous=%s) for Cin=%d" % (tuple(x.shape), x.is_contiguous(), p.cin))
    if x.dtype != p.dtype or out.dtype != p.dtype:
        raise CobevtHipError("deconv_into: input %s / out %s do not match the plan's %s" % (x.dtype, out.dtype, p.dtype))
    n, h, w, _ = x.shape
    if out.dim() != 4 or tuple(out.shape[:3]) != (n, s * h, s * w) or not out.is_contiguous():
        raise CobevtHipError("deconv_into: `out` must be contiguous (%d, %d, %d, ldc) for a stride-%d deconv of %s, got %s"
                             % (n, s * h, s * w, s, tuple(x.shape), tuple(out.shape)))
    ldc, c_off = int(out.shape[3]), int(c_off)
    if c_off < 0 or c_off % 8 != 0 or ldc % 8 != 0:
        raise CobevtHipError("deconv_into: c_off=%d and the destination's %d channels must be multiples of 8 (16-byte stores)" % (c_off, ldc))
    if c_off + p.cout > ldc:
        raise CobevtHipError("deconv_into: channels [%d, %d) do not fit the destination's %d" % (c_off, c_off + p.cout, ldc))
    if n * h * w * s * s >= 2 ** 31:
        raise CobevtHipError("deconv_into: %d destination pixels overflow the kernel's 32-bit pixel index" % (n * h * w * s * s))
    _need_cuda(x, out)

    def cost():
        esz = 2 if p.code == BF16 else 4
        m = n * h * w
        return 2.0 * m * s * s * p.cout * p.cin, float(esz * (m * p.cin + s * s * p.cout * p.cin + m * s * s * p.cout))

    dims = _ints([p.code, n, h, w, p.cin, p.cout, p.kpad, s, c_off, ldc, p.act])
    with _timed("deconv|s%d %d->%d M=%d" % (s, p.cin, p.cout, n * h * w), cost):
        _L.call("cobevt_deconv_nhwc", _p(x), _p(p.wgt), _p(p.shift), _p(out), dims, _stream())
    return out


def basicblock_fusable(x, plan1, plan2):
    """stride-1 BasicBlock without downsample on 64 / 128 channels: both 3x3 convs in one launch (basicblock.hip)"""
    return (USE_BASICBLOCK and plan1.wfrag is not None and plan2.wfrag is not None and plan1.cin == plan1.cout == plan2.cin
            == plan2.cout and plan1.cout in (64, 128) and plan1.cout <= BASICBLOCK_MAX_C and plan1.act == 1 and plan2.act == 1 and not plan1.upsample
            and not plan2.upsample and plan1.store_mode == 0 and plan2.store_mode == 0 and x.is_contiguous()
            and x.dtype == plan1.dtype and x.numel() < 2 ** 31)


def basicblock(x, plan1, plan2):
    """relu(conv2(relu(conv1(x))) + x) for BN-folded 3x3 plans; x (N,H,W,C) channels-last."""
    _need_cuda(x)
    n, h, w, c = x.shape
    out = torch.empty_like(x)
    dims = _ints([plan1.code, n, h, w, c, BASICBLOCK_TILE_ROWS])

    def cost():
        esz = 2 if plan1.code == BF16 else 4
        return 2.0 * 2 * n * h * w * c * 9 * c, float(2 * x.numel() * esz + 2 * c * 9 * c * esz)

    with _timed("basicblock|%d %dx%dx%d" % (c, n, h, w), cost):
        _L.call("cobevt_basicblock_nhwc", _p(x), _p(plan1.wfrag), _p(plan1.bias), _p(plan2.wfrag), _p(plan2.bias), _p(out), dims, _stream())
    return out


def dsblock_fusable(x, plan1, plan2, plan_ds):
    """layer2's first BasicBlock (64 -> 128, stride 2, 1x1 / stride-2 projection shortcut), bf16: one launch (basicblock.hip)"""
    return (USE_DSBLOCK and x.dtype == torch.bfloat16 and plan1.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()
            and plan1.wfrag is not None and plan2.wfrag is not None and plan_ds.wfrag_rows is not None
            and (plan1.cin, plan1.cout, plan1.stride) == (64, 128, 2) and (plan2.cin, plan2.cout, plan2.stride) == (128, 128, 1)
            and (plan_ds.cin, plan_ds.cout, plan_ds.stride, plan_ds.kp_rows) == (64, 128, 2, 128)
            and plan1.act == 1 and plan2.act == 1 and plan_ds.act == 0 and plan_ds.pre_scale is None and not plan_ds.has_ln
            and not plan1.upsample and not plan2.upsample and plan1.store_mode == 0 and plan2.store_mode == 0
            and x.shape[3] == 64 and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0 and x.numel() < 2 ** 31)


def dsblock(x, plan1, plan2, plan_ds):
    """relu(conv2(relu(conv1/s2(x))) + ds(x)) for BN-folded plans; x (N,H,W,64) channels-last bf16 -> (N,H/2,W/2,128)."""
    _need_cuda(x)
    n, h, w, c = x.shape
    out = torch.empty((n, h // 2, w // 2, 128), dtype=x.dtype, device=x.device)
    dims = _ints([plan1.code, n, h, w, c, 128])

    def cost():
        px = n * (h // 2) * (w // 2)
        return 2.0 * px * 128 * (9 * 64 + 9 * 128 + 64), float(2 * (x.numel() + out.numel()) + 2 * 128 * (9 * 64 + 9 * 128 + 64))

    with _timed("basicblock|%d->128/s2 %dx%dx%d" % (c, n, h // 2, w // 2), cost):
        _L.call("cobevt_dsblock_nhwc", _p(x), _p(plan1.wfrag), _p(plan1.bias), _p(plan2.wfrag), _p(plan2.bias), _p(plan_ds.wfrag_rows),
                _p(plan_ds.bias), _p(out), dims, _stream())
    return out


def conv3_ds_fusable(x, plan1, plan2, plan_ds):
    """The down-sampling BasicBlocks of layer3 / layer4 (stride-2 conv1, 1x1 / stride-2 projection shortcut), bf16: the shortcut rides
    in conv2's launch as extra one-tap channel chunks (cobevt_conv3x3_ds_wfrag_nhwc).  Returns the tile variant, or 0."""
    if not (USE_CONV3_DS and USE_CONV3X3 and USE_CONV3_WFRAG and x.dtype == torch.bfloat16 and plan2.dtype == torch.bfloat16
            and x.dim() == 4 and x.is_contiguous() and plan2.wfrag is not None and plan_ds.wgt_rows is not None
            and plan1.stride == 2 and plan2.stride == 1 and plan_ds.stride == 2 and plan2.cc3 == 64
            and plan1.cout == plan2.cin == plan2.cout == plan_ds.cout and plan_ds.cin == x.shape[3] and x.shape[3] % 64 == 0
            and x.shape[3] <= 256 and plan2.cin % 64 == 0 and plan2.act in (0, 1) and plan_ds.act == 0 and plan_ds.pre_scale is None and not plan_ds.has_ln
            and not plan2.upsample and plan2.store_mode == 0 and plan2.bias is not None and plan_ds.bias is not None
            and x.numel() < 2 ** 31):
        return 0
    n, h, w, _ = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    variant = conv3_variant(n, ho, wo, plan2.cin, plan2.cout, 64, 1)
    mt, code = (variant - 100) // 10, (variant - 100) % 10
    return variant if (variant >= 100 and 3 <= mt <= 5 and code in (0, 1)) else 0


def _conv3_ds_table(plan2, plan_ds):
    """conv2's fragment table with the shortcut's one-tap steps appended per 32-cout tile (cached on plan2, keyed by the shortcut plan)"""
    cached = getattr(plan2, "_ds_fused", None)
    if cached is not None and cached[0] is plan_ds:
        return cached[1]
    coutp, cin, cin2 = plan2.coutp3, plan2.cin, plan_ds.cin
    t = coutp // 32
    main = plan2.wfrag.reshape(t, (cin // 64) * 9, 2048)
    wd = torch.zeros((coutp, cin2), dtype=plan2.wfrag.dtype, device=plan2.wfrag.device)
    wd[:plan_ds.cout] = plan_ds.wgt_rows[:, :cin2]
    extra = wd.reshape(t, 32, cin2 // 64, 4, 2, 8).permute(0, 2, 3, 4, 1, 5).reshape(t, cin2 // 64, 2048)
    table = torch.cat([main, extra], dim=1).contiguous()
    plan2._ds_fused = (plan_ds, table)
    return table


def conv3_ds(y, x, plan2, plan_ds, variant):
    """act(conv2(y) + round(ds(x))) for BN-folded plans (the shortcut rounded to the storage type as its own launch would store it): y (N, H/2, W/2, C) = the block's first convolution's output, x (N, H, W, Cin2) its input."""
    _need_cuda(y, x)
    n, ho, wo, c = y.shape
    _, h, w, cin2 = x.shape
    table = _conv3_ds_table(plan2, plan_ds)
    out = torch.empty((n, ho, wo, plan2.cout), dtype=y.dtype, device=y.device)
    dims = _ints([plan2.code, n, ho, wo, c, plan2.cout, plan2.act, plan2.coutp3, variant, h, w, cin2])

    def cost():
        px = n * ho * wo
        return 2.0 * px * plan2.cout * (9 * c + cin2), float(2 * (y.numel() + px * cin2 + out.numel()) + 2 * plan2.cout * (9 * c + cin2))

    with _timed("conv3x3|%d->%d +ds%d %dx%dx%d" % (c, plan2.cout, cin2, n, ho, wo), cost):
        _L.call("cobevt_conv3x3_ds_wfrag_nhwc", _p(y), _p(x), _p(table), _p(plan2.bias), _p(plan_ds.bias), _p(out), dims, _stream())
    return out


class BottleneckPlan(object):
    """torchvision Bottleneck(128, 32) lowered for cobevt_bottleneck_nhwc: the three convolutions with their eval BatchNorms
    folded, as MFMA A-operand fragments ([.., 64 lanes, 8 values]: lane = 32 * half + output row, the 8 values are the
    contraction slots 8 * half .. + 7 of a 16-wide k-block).  W3's contraction index is stored in the order the kernel's
    accumulator registers hand conv2's result over: slot 8 * half + j of k-block u <-> mid channel 16u + (j & 3) + 8 (j >> 2) +
    4 * half (bottleneck.hip)."""

    def __init__(self, conv1, bn1, conv2, bn2, conv3, bn3, device="cuda"):
        def fold(conv, bn):
            w = conv.weight.detach().double().cpu()
            s, sh = bn_affine(bn)
            b = conv.bias.detach().double().cpu() * s.cpu() + sh.cpu() if conv.bias is not None else sh.cpu()
            return w * s.cpu()[:, None, None, None], b
        w1, b1 = fold(conv1, bn1)
        w2, b2 = fold(conv2, bn2)
        w3, b3 = fold(conv3, bn3)
        mid, cin = w1.shape[0], w1.shape[1]
        ok = (tuple(w1.shape) == (32, 128, 1, 1) and tuple(w2.shape) == (32, 32, 3, 3) and tuple(w3.shape) == (128, 32, 1, 1)
              and conv1.stride == (1, 1) and conv2.stride == (1, 1) and conv3.stride == (1, 1) and conv2.padding == (1, 1))
        if not ok:
            raise CobevtHipError("the fused Bottleneck kernel is built for Bottleneck(128, 32), stride 1 (got %d -> %d)" % (cin, mid))
        lane = torch.arange(64)
        row, half = lane % 32, lane // 32
        j = torch.arange(8)
        # W1 [8 k-groups][64][8]: W1[row][16 g + 8 half + j]
        g = torch.arange(8)
        k1 = 16 * g[:, None, None] + 8 * half[None, :, None] + j[None, None, :]
        f1 = w1[:, :, 0, 0][row[None, :, None].expand(8, 64, 8), k1]
        # W2 [9 taps][2][64][8]: W2[row][16 u + 8 half + j][ky][kx]
        u = torch.arange(2)
        k2 = 16 * u[:, None, None] + 8 * half[None, :, None] + j[None, None, :]
        w2t = w2.reshape(32, 32, 9)
        f2 = torch.stack([w2t[:, :, t][row[None, :, None].expand(2, 64, 8), k2] for t in range(9)])
        # W3 [4 cout tiles][2][64][8]: W3[32 ct + row][16 u + (j & 3) + 8 (j >> 2) + 4 half]
        k3 = 16 * u[:, None, None] + (j & 3)[None, None, :] + 8 * (j >> 2)[None, None, :] + 4 * half[None, :, None]
        f3 = torch.stack([w3[32 * ct:32 * ct + 32, :, 0, 0][row[None, :, None].expand(2, 64, 8), k3] for ct in range(4)])
        bf = lambda t: t.to(torch.float32).to(torch.bfloat16).to(device).contiguous()      # noqa: E731
        self.w1, self.w2, self.w3 = bf(f1), bf(f2), bf(f3)
        self.b1, self.b2, self.b3 = [t.to(torch.float32).to(device).contiguous() for t in (b1, b2, b3)]


def bottleneck_fusable(x):
    return USE_BOTTLENECK and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[3] == 128 and x.is_contiguous()


def bottleneck(x, plan, tile_rows=0):
    """relu(conv3(relu(conv2(relu(conv1(x))))) + x) for a BottleneckPlan; x (N, H, W, 128) channels-last bf16."""
    _need_cuda(x)
    n, h, w, c = x.shape
    out = torch.empty_like(x)
    dims = _ints([BF16, n, h, w, c, 32, tile_rows])

    def cost():
        m = n * h * w
        return 2.0 * m * (128 * 32 + 32 * 32 * 9 + 32 * 128), float(2 * x.numel() * 2 + (128 * 32 * 2 + 32 * 32 * 9) * 2)

    with _timed("bottleneck|%dx%dx%d" % (n, h, w), cost):
        _L.call("cobevt_bottleneck_nhwc", _p(x), _p(plan.w1), _p(plan.w2), _p(plan.w3), _p(plan.b1), _p(plan.b2), _p(plan.b3), _p(out),
                dims, _stream())
    return out


def bottleneck_f32_fusable(x, p1, p2, p3, y1=None):
    """the fp32-storage Bottleneck(128, 32) as one launch (csrc/bottleneck_f32.hip; round 6): the three separate launches' own plans"""
    return (USE_BOTTLENECK_F32 and x.dtype == torch.float32 and x.dim() == 4 and x.shape[3] == 128 and x.is_contiguous() and x.numel() < 2 ** 31
            and p1.code == FP32 and p1.wfrag_rows is not None and (p1.K, p1.cout, p1.kp_rows, p1.act, p1.stride) == (128, 32, 128, 1, 1)
            and not p1.has_ln and p1.pre_scale is None and p1.bias is not None
            and p2.wfrag is not None and (p2.cin, p2.cout, p2.cc3, p2.stride, p2.act) == (32, 32, 32, 1, 1) and not p2.upsample
            and p2.store_mode == 0 and p2.bias is not None
            and p3.wfrag_rows is not None and (p3.K, p3.cout, p3.act, p3.stride) == (32, 128, 1, 1) and not p3.has_ln and p3.pre_scale is None
            and p3.bias is not None
            and (y1 is None or (y1.dtype == torch.float32 and y1.is_contiguous() and tuple(y1.shape) == tuple(x.shape[:3]) + (32,))))


def bottleneck_f32(x, p1, p2, p3, y1=None):
    """relu(conv3(relu(conv2(relu(conv1(x))))) + x) on (N, H, W, 128) fp32 channels-last; y1 = relu(conv1(x)) when the producer made it."""
    _need_cuda(x, y1)
    n, h, w, c = x.shape
    out = torch.empty_like(x)
    dims = _ints([n, h, w, p3.kp_rows // 8 * 64])

    def cost():
        m = n * h * w
        return 2.0 * m * ((0 if y1 is not None else 128 * 32) + 32 * 32 * 9 + 32 * 128), float((2 * x.numel() + (y1.numel() if y1 is not None else 0)) * 4)

    with _timed("bottleneck|%dx%dx%d%s" % (n, h, w, " y1" if y1 is not None else ""), cost):
        _L.call("cobevt_bottleneck_f32_nhwc", _p(x), _p(y1), _p(p1.wfrag_rows), _p(p1.bias), _p(p2.wfrag), _p(p2.bias), _p(p3.wfrag_rows),
                _p(p3.bias), _p(out), dims, _stream())
    return out


def linear(x, plan, residual=None, out=None):
    """x: (..., K) contiguous tokens -> (..., Cout).  A Linear is the 1x1 case of the implicit GEMM; plans built
    with ln=... apply LayerNorm(x) first (fused into the GEMM when the row fits one K-tile).  out: optional
    preallocated contiguous (..., Cout) result buffer in the compute dtype."""
    lead = x.shape[:-1]
    rows = int(math.prod(lead)) if len(lead) else 1
    x4 = x.reshape(1, 1, rows, x.shape[-1])
    r4 = residual.reshape(1, 1, rows, plan.cout) if residual is not None else None
    o4 = None
    if out is not None:
        if tuple(out.shape) != tuple(lead) + (plan.cout,) or not out.is_contiguous() or out.dtype != x.dtype:
            raise CobevtHipError("linear: `out` must be a contiguous %s tensor of dtype %s" % (tuple(lead) + (plan.cout,), x.dtype))
        o4 = out.reshape(1, 1, rows, plan.cout)
    y = conv2d(x4, plan, residual=r4, out=o4)
    return out if out is not None else y.reshape(*lead, plan.cout)


# ----------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta, eps=1e-5, out=None):
    """LayerNorm over the last axis of a contiguous tensor."""
    _need_cuda(x, gamma, beta)
    if not x.is_contiguous():
        raise CobevtHipError("layernorm: input must be contiguous")
    c = x.shape[-1]
    rows = x.numel() // c
    if out is None:
        out = torch.empty_like(x)
    _L.call("cobevt_layernorm", _p(x), _p(gamma), _p(beta), _p(out), dcode(x.dtype), rows, c, float(eps), 1, 0, 0, 0, _stream())
    return out


def mean_layernorm(x, gamma, beta, eps=1e-5):
    """x: (B, L, R, C) contiguous -> LayerNorm(mean over L): (B, R, C)   (SwapFusionEncoder.mlp_head)."""
    _need_cuda(x, gamma, beta)
    b, l, r, c = x.shape
    if not x.is_contiguous():
        raise CobevtHipError("mean_layernorm: input must be contiguous")
    out = torch.empty((b, r, c), device=x.device, dtype=x.dtype)
    _L.call("cobevt_layernorm", _p(x), _p(gamma), _p(beta), _p(out), dcode(x.dtype), b * r, c, float(eps), l, r * c, l * r * c, r,
            _stream())
    return out


def mean_ln_linear(x, plan):
    """x (B, L, R, C) contiguous bf16 -> plan(mean over L) with plan's folded LayerNorm: (B, R, Cout), one launch
    (SwapFusionEncoder.mlp_head, swap_fusion_modules.py:275-281); None when the shape does not fit the kernel."""
    _need_cuda(x)
    b, l, r, c = x.shape
    if not (USE_GEMM_ROWS3 and x.dtype == torch.bfloat16 and x.is_contiguous() and plan.wfrag_rows is not None and plan.kp_rows == 128
            and plan.K == c and c % 8 == 0 and plan.cout % 8 == 0 and plan.cout <= 4096 and l <= 64 and plan.pre_scale is None
            and plan.stride == 1):
        return None
    out = torch.empty((b, r, plan.cout), device=x.device, dtype=x.dtype)
    dims = (ctypes.c_long * 8)(0, b, l, r, c, plan.cout, int(plan.has_ln), plan.act)

    def cost():
        return 2.0 * b * r * c * plan.cout, float((b * l * r * c + b * r * plan.cout + c * plan.cout) * 2)

    with _timed("gemm_rows|mean%d %d->%d M=%d ln" % (l, c, plan.cout, b * r), cost):
        _L.call("cobevt_mean_linear_rows_small_k", _p(x), _p(plan.wfrag_rows), _p(plan.bias), _p(out), dims, ctypes.c_float(plan.ln_eps),
                _stream())
    return out


def tokmap(mode, ncam, hh, ww, w1, w2):
    """Token map tuple for cobevt_window_attention: mode 0 window / 1 grid / 2 stored-partitioned."""
    if hh % w1 or ww % w2:
        raise CobevtHipError("map %dx%d not divisible by window %dx%d" % (hh, ww, w1, w2))
    return (int(mode), int(ncam), int(hh), int(ww), int(w1), int(w2), hh // w1, ww // w2)


def window_attention(q, k, v, out, qmap, kmap, omap, batch, heads, scale, ldq, ldk, ldv, ldo, qoff=0, koff=0, voff=0,
                     ooff=0, bias_table=None, bias_L=1, mask=None, mean_q=False, variant=None, qsplit=None, ksplit=None):
    _need_cuda(q, k, v, out, bias_table, mask)
    code = dcode(q.dtype) | ((ATTN_VARIANT if variant is None else int(variant)) << 8) | \
        ((ATTN_QSPLIT if qsplit is None else int(qsplit)) << 16)
    if k.dtype != q.dtype or v.dtype != q.dtype or out.dtype != q.dtype:
        raise CobevtHipError("window_attention: q/k/v/out dtypes differ")
    L = qmap[6] * qmap[7]
    dims = _ints([code, batch, L, heads, ldq, ldk, ldv, ldo, qoff, koff, voff, ooff,
                  0 if bias_table is None else 1, 0 if bias_table is None else bias_table.shape[0], bias_L,
                  int(mean_q)] + list(qmap) + list(kmap) + list(omap))
    def cost():
        nq = qmap[1] * qmap[4] * qmap[5]
        nk = kmap[1] * kmap[4] * kmap[5]
        esz = q.element_size()
        d = heads * 32
        nbytes = batch * L * (nq + 2 * nk + nq // (qmap[1] if mean_q else 1)) * d * esz
        pairs = nq * nk // (qmap[1] if int(mean_q) == 2 else 1)      # camera-paired: a query copy scores its own camera's keys
        return 4.0 * batch * L * heads * pairs * 32, float(nbytes)

    nq_, nk_ = qmap[1] * qmap[4] * qmap[5], kmap[1] * kmap[4] * kmap[5]
    ks = ATTN_KSPLIT if ksplit is None else int(ksplit)
    # plain bf16 windows of 513 .. 1024 keys (the FAX level-2 / global attention: one whole-map window per agent): K / V resident in LDS,
    # one launch (attention_resident.hip, round 6) instead of the key split + merge of the streaming kernel
    big_resident = (USE_ATTN_BIG_RESIDENT and ksplit is None and q.dtype == torch.bfloat16 and bias_table is None and mask is None and not mean_q
                    and 512 < nk_ <= 1024 and (ATTN_VARIANT if variant is None else int(variant)) == 0 and omap[1] == qmap[1])
    use_ks = (ks > 1 and not big_resident and not mean_q and nk_ >= 1024 and batch * L * heads * ((nq_ + 127) // 128) * ks <= 1024
              and out.is_contiguous() and ldo == out.shape[-1] and ooff == 0 and omap[1] == qmap[1])
    if int(mean_q) == 2:
        # camera-paired (CVT): split only when the caller asks for it - with ksplit=None the OPV2V CVT baselines keep their single-pass launch
        use_ks = ksplit is not None and ks > 1
        if use_ks and not (out.is_contiguous() and ldo == out.shape[-1] and ooff == 0):
            raise CobevtHipError("window_attention: the camera-paired key split writes a contiguous `out` (ldo = width, ooff = 0)")
    # "fp32_fast": the attention launches go to the third library as well (lib.encoder_scope() is a no-op in every other mode) - fp16
    # queries / probabilities against fp16 (hi, lo) keys / values, csrc/attention.hip kStage16
    with _L.encoder_scope(), _timed("attention|B%d L%d h%d Nq%d Nk%d%s" % (batch, L, heads, nq_, nk_, " ks%d" % ks if use_ks else ""), cost):
        if use_ks:
            rows = out.numel() // out.shape[-1]
            part_out = torch.empty((ks, rows, heads * 32), device=out.device, dtype=out.dtype)
            part_lse = torch.empty((ks, rows, heads), device=out.device, dtype=torch.float32)
            _L.call("cobevt_window_attention_ksplit", _p(q), _p(k), _p(v), _p(out), _p(bias_table), _p(mask), _p(part_out), _p(part_lse),
                    dims, ctypes.c_float(scale), ks, rows, _stream())
        else:
            _L.call("cobevt_window_attention", _p(q), _p(k), _p(v), _p(out), _p(bias_table), _p(mask), dims, ctypes.c_float(scale),
                    _stream())
    return out


PAIRED_KSPLIT_MAX = 16      # cobevt_window_attention_ksplit's cap
PAIRED_KSPLIT_WG = 512      # ... and the grid the split count aims at: up to two workgroups per CU


def paired_ksplit(batch, heads, qmap, kmap):
    """Key split for a camera-paired (mean_q = 2) window_attention over whole-map windows: as many splits as keep the grid at or below
    PAIRED_KSPLIT_WG workgroups (batch x heads x 128-query tiles each), at most PAIRED_KSPLIT_MAX and at most one per 64-key tile
    (tiles never mix cameras).  None when the unsplit grid is already that large (no split)."""
    L = qmap[6] * qmap[7]
    wg = batch * L * heads * ((qmap[4] * qmap[5] + 127) // 128)
    tiles = kmap[1] * ((kmap[4] * kmap[5] + 63) // 64)
    ks = min(PAIRED_KSPLIT_MAX, tiles, PAIRED_KSPLIT_WG // wg)
    return ks if ks >= 2 else None


def attention_index_map(tmap, batch, device):
    """int32 (batch, X*Y, ncam*w1*w2): the token -> row map of cobevt_window_attention for one token map (test hook)."""
    L, ntok = tmap[6] * tmap[7], tmap[1] * tmap[4] * tmap[5]
    rows = torch.empty((batch, L, ntok), device=device, dtype=torch.int32)
    _need_cuda(rows)
    _L.call("cobevt_attention_index_map", _ints(tmap), batch, _p(rows), _stream())
    return rows


def attention_bias_index(qmap, kmap, bias_L, device):
    """int32 (Nq, Nk): the relative-position table row the attention kernels use for every (query, key) pair (test hook)."""
    nq, nk = qmap[1] * qmap[4] * qmap[5], kmap[1] * kmap[4] * kmap[5]
    idx = torch.empty((nq, nk), device=device, dtype=torch.int32)
    _need_cuda(idx)
    _L.call("cobevt_attention_bias_index", _ints(qmap), _ints(kmap), int(bias_L), _p(idx), _stream())
    return idx


def agent_max(x):
    """(B, L, ...) contiguous -> max over L: (B, ...)   (F-Cooper max-out, fusion_modules/f_cooper_fuse.py:30-36)"""
    _need_cuda(x)
    if not x.is_contiguous():
        raise CobevtHipError("agent_max: input must be contiguous")
    b, l = x.shape[:2]
    out = torch.empty((b,) + tuple(x.shape[2:]), device=x.device, dtype=x.dtype)
    per = out[0].numel()
    _L.call("cobevt_agent_max", _p(x), _p(out), dcode(x.dtype), b, l, per, _stream())
    return out


def ray_embed(i_inv, e_inv, image_plane, w_img, w_cam, hw, dim, dtype):
    _need_cuda(i_inv, e_inv, image_plane, w_img, w_cam)
    bn = i_inv.shape[0]
    out = torch.empty((bn, hw, dim), device=i_inv.device, dtype=dtype)
    _L.call("cobevt_fax_ray_embed", _p(i_inv), _p(e_inv), _p(image_plane), _p(w_img), _p(w_cam), _p(out), dcode(dtype), bn, hw, dim,
            _stream())
    return out


def batch_broadcast(x):
    """True for expand()-ed views whose leading dimension has stride 0 over one contiguous slice."""
    return x.dim() >= 2 and x.shape[0] > 1 and x.stride(0) == 0 and x[0].is_contiguous()


def bev_embed(e_inv, world, w_bev, b_bev, w_cam, x, n):
    """x: (B, HW, D), or a batch-broadcast view (stride 0 over B) of one (HW, D) prior -> query (B, n, HW, D)"""
    _need_cuda(e_inv, world, w_bev, b_bev, w_cam, x)
    b, hw, d = x.shape
    bcast = batch_broadcast(x)
    if not bcast:
        x = x.contiguous()
    out = torch.empty((b, n, hw, d), device=x.device, dtype=x.dtype)
    _L.call("cobevt_fax_bev_embed", _p(e_inv), _p(world), _p(w_bev), _p(b_bev), _p(w_cam), _p(x), _p(out), dcode(x.dtype), b, n, hw, d,
            int(bcast), _stream())
    return out


def bev_embed_linear(e_inv, world, w_bev, b_bev, w_cam, x, n, plan):
    """plan(bev_embed(...)) : (B, HW, D) -> (B, n, HW, N) without materialising the (B, n, HW, D) query (the dense-row GEMM
    produces its A rows on the fly) when plan is a LayerNorm-folded Linear whose row fits one K-tile; otherwise the two
    launches."""
    b, hw, d = x.shape
    bcast = batch_broadcast(x)
    wave_level = d == 128 and plan.cout == 128 and b * n <= 32           # bev_query.hip's shape (else the call lands in gemm_rows3.hip)
    fused3 = ((USE_EMBED_GEMM3 == 2 or (USE_EMBED_GEMM3 and wave_level)) and USE_GEMM_ROWS3 and plan.code == BF16 and plan.has_ln
              and plan.K == d and d <= 128 and d % 8 == 0
              and plan.kp_rows == 128 and plan.wfrag_rows is not None and hw % 32 == 0 and plan.stride == 1
              and plan.pre_scale is None and plan.act == 0 and plan.cout % 8 == 0 and (bcast or x.is_contiguous()))
    if fused3:
        _need_cuda(e_inv, world, w_bev, b_bev, w_cam, x)
        out = torch.empty((b, n, hw, plan.cout), device=x.device, dtype=x.dtype)
        dims = (ctypes.c_long * 8)(plan.code, b, n, hw, d, plan.cout, 1, int(bcast))

        def cost3():
            m = b * n * hw
            return 2.0 * m * plan.cout * d, float((hw if bcast else x.numel() // d) * d * 2 + plan.cout * d * 2 + out.numel() * 2)

        with _timed("gemm_rows|embed %d->%d M=%d ln r32" % (d, plan.cout, b * n * hw), cost3):
            _L.call("cobevt_bev_embed_linear_rows_small_k", _p(e_inv), _p(world), _p(w_bev), _p(b_bev), _p(w_cam), _p(x),
                    _p(plan.wfrag_rows), _p(plan.bias), _p(out), dims, ctypes.c_float(plan.ln_eps), _stream())
        return out
    fused = (USE_EMBED_GEMM and USE_GEMM_ROWS and plan.has_ln and ln_fusable(plan) and plan.K == d and hw % 128 == 0
             and plan.stride == 1 and plan.pre_scale is None and plan.act == 0 and x.is_contiguous())
    if not fused:
        return linear(bev_embed(e_inv, world, w_bev, b_bev, w_cam, x, n), plan)
    _need_cuda(e_inv, world, w_bev, b_bev, w_cam, x)
    out = torch.empty((b, n, hw, plan.cout), device=x.device, dtype=x.dtype)
    dims = (ctypes.c_long * 8)(plan.code, b, n, hw, d, plan.cout, plan.kp_rows, 1)

    def cost():
        m = b * n * hw
        esz = 2 if plan.code == BF16 else 4
        return 2.0 * m * plan.cout * d, float(x.numel() * esz + plan.cout * d * esz + out.numel() * esz)

    with _timed("gemm_rows|embed %d->%d M=%d ln" % (d, plan.cout, b * n * hw), cost):
        _L.call("cobevt_bev_embed_linear_rows", _p(e_inv), _p(world), _p(w_bev), _p(b_bev), _p(w_cam), _p(x), _p(plan.wgt_rows),
                _p(plan.bias), _p(out), dims, ctypes.c_float(plan.ln_eps), _stream())
    return out


def stem_pool(x, plan):
    """maxpool3x3s2(conv2d(x, plan)) for the ResNet stem plan (7x7 / s2 / pad 3 on the fp32 image, 64 couts, ReLU):
    one launch when the image sides are multiples of 4, else the two kernels."""
    _need_cuda(x)
    n, h, w, cin = x.shape
    fused = (USE_STEM_POOL and USE_STEM and plan.wgt_stem is not None and plan.cout == 64 and plan.act == 1
             and h % 4 == 0 and w % 4 == 0 and x.dtype == torch.float32 and x.is_contiguous())
    if not fused:
        return maxpool3x3s2(conv2d(x, plan))
    out = torch.empty((n, h // 4, w // 4, 64), device=x.device, dtype=plan.dtype)
    dims = _ints([plan.code, n, h, w])

    def cost():
        esz = 2 if plan.code == BF16 else 4
        return 2.0 * n * (h // 2) * (w // 2) * 64 * 147, float(x.numel() * 4 + out.numel() * esz)

    with _timed("stem7x7|pool %dx%dx%d" % (n, h, w), cost):
        _L.call("cobevt_stem_conv7x7s2_pool", _p(x), _p(plan.wgt_stem), _p(plan.bias), _p(out), dims, _stream())
    return out


def stem_pool_u8(x, lut, plan):
    """stem_pool on uint8 camera frames (N, H, W, 3) + the (3, 256) fp32 normalisation table (host/rgb_preprocessor.py): the
    reference's host-side normalisation and the fp32 image upload folded into the stem's gather.  No fallback: the frame sides must
    be multiples of 4 (every OPV2V / nuScenes resolution is)."""
    _need_cuda(x, lut)
    n, h, w, cin = x.shape
    if not (plan.wgt_stem is not None and plan.cout == 64 and plan.act == 1 and h % 4 == 0 and w % 4 == 0 and cin == 3
            and x.dtype == torch.uint8 and x.is_contiguous() and lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256)
            and lut.is_contiguous()):
        raise CobevtHipError("stem_pool_u8: needs contiguous uint8 frames (N, H, W, 3) with H, W multiples of 4, a (3, 256) fp32 table "
                             "and the ResNet stem plan; got %s %s" % (tuple(x.shape), x.dtype))
    out = torch.empty((n, h // 4, w // 4, 64), device=x.device, dtype=plan.dtype)
    dims = _ints([plan.code, n, h, w])

    def cost():
        esz = 2 if plan.code == BF16 else 4
        return 2.0 * n * (h // 2) * (w // 2) * 64 * 147, float(x.numel() + out.numel() * esz)

    with _timed("stem7x7|pool u8 %dx%dx%d" % (n, h, w), cost):
        _L.call("cobevt_stem_conv7x7s2_pool_u8", _p(x), _p(lut), _p(plan.wgt_stem), _p(plan.bias), _p(out), dims, _stream())
    return out


def host_fetch(src_pinned, dst, blocks=0):
    """dst (device) <- src_pinned (pinned host tensor of the same shape / dtype) by a kernel that reads the host buffer over PCIe
    (cobevt_host_fetch): capturable in a HIP graph, runs beside the compute kernels."""
    _need_cuda(dst)
    if src_pinned.is_cuda or not src_pinned.is_pinned():
        raise CobevtHipError("host_fetch: the source must be a pinned host tensor (tensor.pin_memory())")
    nbytes = dst.numel() * dst.element_size()
    if (tuple(src_pinned.shape) != tuple(dst.shape) or src_pinned.dtype != dst.dtype or not src_pinned.is_contiguous() or not dst.is_contiguous()
            or nbytes % 16):
        raise CobevtHipError("host_fetch: contiguous tensors of one shape / dtype, a multiple of 16 bytes")
    _L.call("cobevt_host_fetch", ctypes.c_void_p(src_pinned.data_ptr()), _p(dst), nbytes, int(blocks), _stream())
    return dst


def maxpool3x3s2(x):
    _need_cuda(x)
    n, h, w, c = x.shape
    ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    out = torch.empty((n, ho, wo, c), device=x.device, dtype=x.dtype)
    _L.call("cobevt_maxpool3x3s2", _p(x), _p(out), dcode(x.dtype), n, h, w, c, _stream())
    return out


def to_nhwc(x, dtype):
    """Any (N,C,H,W)-shaped CUDA tensor (arbitrary strides, bf16/fp32) -> contiguous (N,H,W,C) in `dtype`.
    Zero-copy when x already is a channels-last view of the right dtype."""
    _need_cuda(x)
    n, c, h, w = x.shape
    v = x.permute(0, 2, 3, 1)
    if x.dtype == dtype and v.is_contiguous():
        return v
    out = torch.empty((n, h, w, c), device=x.device, dtype=dtype)
    strides = (ctypes.c_long * 4)(*x.stride())
    _L.call("cobevt_to_nhwc", _p(x), dcode(x.dtype), _p(out), dcode(dtype), n, c, h, w, strides, _stream())
    return out


def from_nhwc(x, dtype):
    """Contiguous (N,H,W,C) -> contiguous (N,C,H,W) in `dtype`."""
    _need_cuda(x)
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), device=x.device, dtype=dtype)
    strides = (ctypes.c_long * 4)(*out.stride())
    _L.call("cobevt_from_nhwc", _p(x), dcode(x.dtype), _p(out), dcode(dtype), n, c, h, w, strides, _stream())
    return out


def copy_into_interior(x, dst):
    """dst[:, :h, :w, :] = x for contiguous (N, h, w, C) `x` and a contiguous, larger (N, H, W, C) `dst` of the same dtype - the
    zero-padded key map of a FAX level without image features (fax_modules.py:392-396).  cobevt_from_nhwc with the interior's
    strides: no torch arithmetic on the inference path."""
    _need_cuda(x, dst)
    n, h, w, c = x.shape
    if dst.dtype != x.dtype or not x.is_contiguous() or not dst.is_contiguous() or dst.shape[0] != n or dst.shape[3] != c \
            or dst.shape[1] < h or dst.shape[2] < w:
        raise CobevtHipError("copy_into_interior: dst must be a contiguous (N, >= h, >= w, C) map of x's dtype")
    sN, sH, sW, sC = dst.stride()
    strides = (ctypes.c_long * 4)(sN, sC, sH, sW)                     # (N, C, H, W) order of the C entry point
    _L.call("cobevt_from_nhwc", _p(x), dcode(x.dtype), _p(dst), dcode(dst.dtype), n, c, h, w, strides, _stream())
    return dst


def regroup(x, record_len, max_cav):
    """x: (N, ...) contiguous, record_len int32 device (B,) -> (B, max_cav, ...), mask (B, max_cav) fp32."""
    _need_cuda(x, record_len)
    if record_len.dtype != torch.int32 or not x.is_contiguous():
        raise CobevtHipError("regroup: record_len must be int32 on the device and x contiguous")
    b = record_len.shape[0]
    per = x[0].numel()
    out = torch.empty((b, max_cav) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
    mask = torch.empty((b, max_cav), device=x.device, dtype=torch.float32)
    _L.call("cobevt_regroup", _p(x), _p(record_len), _p(out), _p(mask), dcode(x.dtype), b, max_cav, per, _stream())
    return out, mask


PILLAR_CHANNELS = 64        # the one PFN layer csrc/pillar_vfe.hip implements
PILLAR_MAX_POINTS = 32      # a pillar's points sit on the lanes of one half-wave


def _index_i32(t, what, shape_tail=None):
    """int32 contiguous device index tensor; an int64 one is converted on the device (no host round trip)"""
    if t.dtype == torch.int64:
        t = t.to(torch.int32)
    if t.dtype != torch.int32:
        raise CobevtHipError("%s must be an int32 (or int64) tensor, got %s" % (what, t.dtype))
    if shape_tail is not None and tuple(t.shape[1:]) != shape_tail:
        raise CobevtHipError("%s must have shape (P%s), got %s" % (what, "".join(", %d" % d for d in shape_tail), tuple(t.shape)))
    return t if t.is_contiguous() else t.contiguous()


def _scratch(entry, dims, n=1, packed=False, variant=None):
    """The size question every `*_scratch` entry of the C library answers: dims (a c_long vector, or the one integer the entry takes)
    -> the size, or the n sizes, written through one output word each (packed: through one c_long vector of n)"""
    out = (ctypes.c_long * n)() if packed else [ctypes.c_long(0) for _ in range(n)]
    _L.call(entry, dims, *([out] if packed else [ctypes.byref(v) for v in out]), variant=variant)
    sizes = tuple(int(v) if packed else v.value for v in out)
    return sizes[0] if n == 1 else sizes


def _longs(*vals):
    return (ctypes.c_long * len(vals))(*[int(v) for v in vals])


_WORKSPACES = {}      # family -> {(device,) + key: the default buffer}, for the life of the process
WORKSPACE_ALIGN = 16  # bytes: the strictest start any family demands of a workspace; every default has it
# family -> the arguments its C size formula reads, as the key of its default buffer.  A key that left one out would hand a later call
# a buffer that is too small; one that held more (bev_points' point count, say) would grow a buffer per distinct value.
WORKSPACE_KEYS = {
    "voxelize": lambda m, n, t, max_voxels, nx, ny: (m, n, t, max_voxels, nx, ny),            # voxel_ws_ints (nz = 1)
    "voxelize3d": lambda m, n, t, max_voxels, slots: (m, n, t, max_voxels, slots),            # ... with the table in place of the grid
    "prepare_points": lambda m: (m,),                                                         # cloud_ws_ints
    "sparse": lambda n, shape: (n,) + tuple(shape),                                           # sp_index_ints
    "detect": lambda total: (total,),                                                         # det_ws_bytes
    "bev_points": lambda n, nx, ny: (n, nx, ny),                                              # bev_points_ws_ints: 3 N nx ny
    "sparse_train": lambda dtype, elements: (dtype, elements),                                # sized by its callers
}


def _workspace(what, family, dev, key, need, given, dtype=torch.int32, align=4):
    """The scratch buffer of one operator call: the caller's `workspace=` after its checks, or the family's default.
    A default is one buffer per (family, device, key), made on first use and kept for the life of the process, so that a captured
    graph replays on the buffer it saw; one first made during a capture is cached like any other, which is why the replays and later
    eager calls share it.  `key` must hold every argument the size depends on (tests pin this against the C formulas).  `need`, in
    elements of `dtype`, is a number or - where the C library is to be asked only on a miss or for a given buffer - a callable.
    A default starts on a WORKSPACE_ALIGN boundary whatever the family; a given one must be contiguous `dtype` on `dev`, hold `need`
    elements and start on the family's own `align` bytes."""
    if given is None:
        cache = _WORKSPACES.setdefault(family, {})
        ws = cache.get((dev,) + key)
        if ws is None:
            ws = cache[(dev,) + key] = torch.empty(need() if callable(need) else need, device=dev, dtype=dtype)
            if ws.data_ptr() % WORKSPACE_ALIGN:       # a fresh torch block starts on 64 (host) / 512 (device) bytes: checked, not assumed
                raise CobevtHipError("%s: the allocator returned a workspace off the %d-byte boundary" % (what, WORKSPACE_ALIGN))
        return ws
    need = need() if callable(need) else need
    if given.dtype != dtype or not given.is_contiguous() or given.numel() < need or given.device != dev or given.data_ptr() % align:
        raise CobevtHipError("%s: workspace= must be a contiguous%s %s tensor of at least %d elements on %s"
                             % (what, ", %d-byte aligned" % align if align > given.element_size() else "", str(dtype).split(".")[-1], need, dev))
    return given


_TABLES = {}          # family -> {id(weight): (weakref, version, data_ptr, tables)}
# a family's own dict inside the two registries, under the name its tests clear and look into (a test clears one family, never the registry)
_SPARSE_WS, _SPARSE_TRAIN_WS, _CLOUD_WS = (_WORKSPACES.setdefault(f, {}) for f in ("sparse", "sparse_train", "prepare_points"))
_SPARSE_TRAIN_WEIGHTS, _DECONV_TRAIN_WEIGHTS = (_TABLES.setdefault(f, {}) for f in ("sparse", "deconv"))


def _lowered_tables(family, weight, lower):
    """lower(weight.detach()) -> the operand tables of a training kernel, cached per weight OBJECT on its version counter and address:
    hand over the nn.Parameter itself (a .detach() of it is a new object every time and would never hit).  An entry goes when its
    weight does.  Never cached inside a graph capture: there the lowering is part of the graph, so a replay follows the optimiser."""
    capturing = weight.is_cuda and torch.cuda.is_current_stream_capturing()
    cache = _TABLES.setdefault(family, {})
    key, stamp = id(weight), (weight._version, weight.data_ptr())
    ent = cache.get(key)
    if not capturing and ent is not None and ent[0]() is weight and ent[1:3] == stamp:
        return ent[3]
    tables = lower(weight.detach())
    if not capturing:
        cache[key] = (weakref.ref(weight, lambda _: cache.pop(key, None)),) + stamp + (tables,)
    return tables


def _points_offsets(what, points, point_offsets):
    """the cloud operators' input: points (M, 4) contiguous fp32, point_offsets (N + 1,) int32 / int64 -> (offsets int32, N, M, device)"""
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4 or not points.is_contiguous():
        raise CobevtHipError("%s: points must be contiguous fp32 (M, 4) as [x, y, z, intensity], got %s %s"
                             % (what, points.dtype, tuple(points.shape)))
    offs = _index_i32(point_offsets, what + ": point_offsets")
    if offs.dim() != 1 or offs.shape[0] < 2:
        raise CobevtHipError("%s: point_offsets must be (N + 1,) with N >= 1 agents, got %s" % (what, tuple(offs.shape)))
    return offs, offs.shape[0] - 1, points.shape[0], points.device


class BnTrainMode(object):
    """How a train-mode entry normalises with the BatchNorm1d container `bn` (None: no norm), decided in one place.
    .mode 0: batch statistics (bn.training, or a norm without running statistics); 1: the frozen running statistics, read only;
    2: no norm.  frozen = True / False overrides the container's own choice.  BatchNorm1d(momentum=None) is refused in the constructor,
    which callers run before anything is launched: the `kernels` ("pillar", "sparse") keep an exponential running average.  It reads no
    buffer of a module in train(): it runs several times per layer and step.  .buffers() are the kernel's arguments, .written() follows
    the launch."""
    __slots__ = ("bn", "mode", "_written")

    def __init__(self, bn, kernels, frozen=None):
        self.bn, self.mode, self._written = bn, 2, ()
        if bn is None:
            return
        if frozen is None:
            frozen = not bn.training and bn.track_running_stats and bn.running_mean is not None
        elif frozen and not (bn.track_running_stats and bn.running_mean is not None):
            raise CobevtHipError("the %s training kernels: frozen statistics need a BatchNorm1d with running statistics" % kernels)
        if not frozen and bn.track_running_stats and bn.momentum is None:
            raise CobevtHipError("BatchNorm1d(momentum=None): the %s training kernels keep an exponential running average and need a "
                                 "numeric momentum" % kernels)
        self.mode = 1 if frozen else 0

    def buffers(self):
        """-> (running_mean, running_var, num_batches_tracked, eps, momentum): in mode 0 the three buffers the kernel updates where the
        norm tracks them, in mode 1 the two it reads, None otherwise"""
        bn = self.bn
        if bn is None:
            return None, None, None, 0.0, 0.0
        rm = rv = nbt = None
        if self.mode == 1 or (bn.track_running_stats and bn.running_mean is not None):
            rm, rv = bn.running_mean, bn.running_var
            if self.mode == 0:
                nbt = bn.num_batches_tracked
                self._written = (rm, rv, nbt)
        return rm, rv, nbt, bn.eps, 0.0 if bn.momentum is None else bn.momentum

    def written(self):
        """after the launch: the buffers .buffers() handed out for updating were written through raw pointers, so bump their version
        counters (eval plans folded from the running statistics rebuild, graph fingerprints move)"""
        for t in self._written:
            if t is not None:
                torch.autograd.graph.increment_version(t)


def pillar_args(what, vf, npts, coords, geom, use_absolute_xyz, with_distance, code, grid=None, record_len=None, max_cav=None,
                num_agents=None):
    """What every entry of the pillar front end takes, checked in one place, and the `dims` / `geom` vectors cobevt_pillar_vfe and
    cobevt_pillar_train_* share: voxel_features (P, T <= 32, 4) contiguous fp32, voxel_num_points (P), voxel_coords (P, 4) int32 / int64,
    geom = (voxel x, y, z, offset x, y, z), code = the output's dtype code.  grid None: the rows form (record_len is not used); else
    (ny, nx) with record_len (int32 (B,) on the device) and max_cav, or with num_agents.
    -> (npts, coords as int32, dims, geom, k, record_len | None, (n, b, l)): k = the decorated point's features, n = the bound on the
    batch indices, (b, l) = the regrouped canvas' (B, max_cav), (0, 0) without record_len"""
    _need_cuda(vf, npts, coords, record_len)
    if vf.dtype != torch.float32 or vf.dim() != 3 or not vf.is_contiguous():
        raise CobevtHipError("%s: voxel_features must be contiguous fp32 (P, T, 4)" % what)
    p, t, f = vf.shape
    k = (4 if use_absolute_xyz else 1) + 6 + (1 if with_distance else 0)
    if f != 4 or t < 1 or t > PILLAR_MAX_POINTS:
        raise CobevtHipError("%s: F = 4 point features and 1 <= T <= %d points per pillar are supported, got F = %d, T = %d"
                             % (what, PILLAR_MAX_POINTS, f, t))
    npts = _index_i32(npts, what + ": voxel_num_points", ())
    coords = _index_i32(coords, what + ": voxel_coords", (4,))
    if npts.shape[0] != p or coords.shape[0] != p:
        raise CobevtHipError("%s: voxel_num_points (P) and voxel_coords (P, 4) must match voxel_features' P = %d" % (what, p))
    if len(geom) != 6:
        raise CobevtHipError("%s: geom = (voxel x, y, z, offset x, y, z)" % what)
    n = b = l = ny = nx = 0
    if grid is None:
        record_len = None
    else:
        ny, nx = int(grid[0]), int(grid[1])
        if record_len is not None:
            if record_len.dtype != torch.int32 or record_len.dim() != 1 or not record_len.is_contiguous() or max_cav is None:
                raise CobevtHipError("%s: record_len must be int32 (B,) on the device, with max_cav given" % what)
            # with record_len the slot search already rejects n >= sum(record_len): no second bound unless the caller gives one (a
            # sample with more than max_cav agents pushes later samples' agent indices past B * max_cav)
            n, b, l = 0x7fffffff if num_agents is None else int(num_agents), record_len.shape[0], int(max_cav)
        elif num_agents is None:
            raise CobevtHipError("%s: num_agents (a host integer) is required without record_len" % what)
        else:
            n = int(num_agents)
    dims = _ints([p, t, f, k, int(bool(use_absolute_xyz)), int(bool(with_distance)), code, int(grid is None), n, b, l, ny, nx])
    return npts, coords, dims, (ctypes.c_float * 6)(*[float(v) for v in geom]), k, record_len, (n, b, l)


def _pillar_call(voxel_features, args, w, shift, out, cav):
    npts, coords, dims, g, k, record_len, _ = args
    _need_cuda(w, shift, out)
    if w.dtype != torch.float32 or shift.dtype != torch.float32 or not w.is_contiguous() or not shift.is_contiguous() \
            or tuple(w.shape) != (k, PILLAR_CHANNELS) or tuple(shift.shape) != (PILLAR_CHANNELS,):
        raise CobevtHipError("pillar_vfe: folded weight / shift must be contiguous fp32 (%d, %d) / (%d)" % (k, PILLAR_CHANNELS, PILLAR_CHANNELS))
    _L.call("cobevt_pillar_vfe", _p(voxel_features), _p(npts), _p(coords), _p(w), _p(shift), _p(record_len), _p(out), _p(cav), dims, g,
            _stream())


def _canvas(out, shape, dtype, device, what):
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.device != device:
        raise CobevtHipError("%s: out= must be a contiguous %s tensor of shape %s on %s" % (what, dtype, tuple(shape), device))
    return out


def pillar_vfe_scatter(voxel_features, voxel_num_points, voxel_coords, w, shift, geom, grid, dtype, use_absolute_xyz=True,
                       with_distance=False, record_len=None, max_cav=None, num_agents=None, out=None):
    """PillarVFE (one 64-channel PFN layer) + PointPillarScatter (+ regroup) in one operator (csrc/pillar_vfe.hip).
    voxel_features (P, T <= 32, 4) fp32; voxel_num_points (P); voxel_coords (P, 4) as [n, z, y, x] (int32, or int64: converted on the
    device); w (K, 64) / shift (64) fp32 folded layer; geom = (voxel x, y, z, offset x, y, z); grid = (ny, nx); dtype: the canvas's.
    With record_len (int32 device (B,)) and max_cav: -> canvas (B, max_cav, ny, nx, 64), cav_mask (B, max_cav) fp32 as ops.regroup;
    num_agents (host int, optional) is a further upper bound on the batch indices; by default only record_len bounds them.  Without: -> canvas (num_agents, ny, nx, 64), None.
    Every element of the canvas is written (cells without a pillar and padded agent slots with 0, whatever `out=` held).  Rows with a
    batch index < 0 (the padding convention for a fixed P under graph replay) or >= num_agents, in a slot >= max_cav, with y / x
    outside the grid or voxel_num_points <= 0 are skipped.  No host synchronisation."""
    ny, nx = int(grid[0]), int(grid[1])
    dev = voxel_features.device
    args = pillar_args("pillar_vfe", voxel_features, voxel_num_points, voxel_coords, geom, use_absolute_xyz, with_distance, dcode(dtype),
                       (ny, nx), record_len, max_cav, num_agents)
    k, (n, b, l) = args[4], args[6]
    shape = (b, l, ny, nx, PILLAR_CHANNELS) if record_len is not None else (n, ny, nx, PILLAR_CHANNELS)
    if n < 1 or ny < 1 or nx < 1 or (record_len is not None and (b < 1 or l < 1)):
        raise CobevtHipError("pillar_vfe_scatter: empty canvas %s" % (shape,))
    cav = torch.empty((b, l), device=dev, dtype=torch.float32) if record_len is not None else None
    out = _canvas(out, shape, dtype, dev, "pillar_vfe_scatter")
    pts = voxel_features.shape[0] * voxel_features.shape[1]
    cost = lambda: (2.0 * pts * k * PILLAR_CHANNELS, 16.0 * pts + out.numel() * out.element_size())         # noqa: E731
    with _timed("pillar_vfe|P%d T%d %dx%d" % (voxel_features.shape[0], voxel_features.shape[1], ny, nx), cost):
        _pillar_call(voxel_features, args, w, shift, out, cav)
    return out, cav


def pillar_vfe_rows(voxel_features, voxel_num_points, voxel_coords, w, shift, geom, dtype, use_absolute_xyz=True, with_distance=False):
    """The same layer as dense rows: -> (P, 64) in `dtype`, row p = pillar p (always two-dimensional: the reference's squeeze()
    collapses P = 1).  A pillar with voxel_num_points <= 0 gives a zero row."""
    _need_cuda(voxel_features)
    out = torch.empty((voxel_features.shape[0], PILLAR_CHANNELS), device=voxel_features.device, dtype=dtype)
    if out.numel() == 0:
        dcode(dtype)
        return out
    _pillar_call(voxel_features, pillar_args("pillar_vfe", voxel_features, voxel_num_points, voxel_coords, geom, use_absolute_xyz,
                                             with_distance, dcode(dtype)), w, shift, out, None)
    return out


def scatter_rows(rows, voxel_coords, num_agents, grid, out=None):
    """PointPillarScatter: rows (P, C) bf16 / fp32 contiguous, voxel_coords (P, 4) [n, z, y, x] -> (num_agents, ny, nx, C) channels-last,
    cell z + y * nx + x of agent n; every other element 0.  Rows with n outside [0, num_agents) or y / x outside the grid are skipped."""
    _need_cuda(rows, voxel_coords, out)
    if rows.dim() != 2 or not rows.is_contiguous() or (rows.shape[1] * rows.element_size()) % 16:
        raise CobevtHipError("scatter_rows: rows must be contiguous (P, C) with C * element size a multiple of 16 bytes")
    p, c = rows.shape
    coords = _index_i32(voxel_coords, "scatter_rows: voxel_coords", (4,))
    if coords.shape[0] != p:
        raise CobevtHipError("scatter_rows: voxel_coords must be (P, 4) with P = %d" % p)
    n, ny, nx = int(num_agents), int(grid[0]), int(grid[1])
    if n < 1 or ny < 1 or nx < 1:
        raise CobevtHipError("scatter_rows: empty canvas (%d, %d, %d, %d)" % (n, ny, nx, c))
    out = _canvas(out, (n, ny, nx, c), rows.dtype, rows.device, "scatter_rows")
    _L.call("cobevt_scatter_rows", _p(rows), _p(coords), _p(out), dcode(rows.dtype), p, c, n, ny, nx, _stream())
    return out


def voxel_grid_size(lidar_range, voxel_size):
    """(nx, ny, nz) = round((range_hi - range_lo) / voxel_size) in fp32, as spconv's VoxelGenerator forms it"""
    r = np.asarray(lidar_range, dtype=np.float32).reshape(-1)
    v = np.asarray(voxel_size, dtype=np.float32).reshape(-1)
    if r.shape != (6,) or v.shape != (3,) or not bool(np.all(v > 0)) or not bool(np.all(np.isfinite(r))):
        raise CobevtHipError("voxelize_points: lidar_range = [x0, y0, z0, x1, y1, z1] and voxel_size = [vx, vy, vz] > 0, got %s / %s"
                             % (list(lidar_range), list(voxel_size)))
    return tuple(int(g) for g in np.round((r[3:] - r[:3]) / v).astype(np.int64))


def voxelize_workspace_ints(num_points, num_agents, grid, max_points, max_voxels):
    """int32 elements of voxelize_points' workspace for M points of N agents on an (nx, ny, nz) grid (cobevt_voxelize_scratch)"""
    return _scratch("cobevt_voxelize_scratch", _longs(num_points, num_agents, max_points, max_voxels, grid[0], grid[1], grid[2], 0, 0))


def voxelize_points(points, point_offsets, lidar_range, voxel_size, max_points=32, max_voxels=None, range_mask=False, ego_mask=False,
                    out=None, workspace=None):
    """spconv's points_to_voxel with OpenCOOD's collate (csrc/voxelize.hip), without a host synchronisation.
    points (M, 4) contiguous fp32 [x, y, z, intensity]: the agents' points concatenated, in the ego frame; point_offsets (N + 1,)
    int32 on the device (int64: converted on the device): agent a owns rows offsets[a] .. offsets[a + 1], rows at or past offsets[N]
    are ignored.  Per agent, in input order: points with a non-finite coordinate, outside the optional masks (range_mask:
    pcd_utils.mask_points_by_range's strict inequalities; ego_mask: pcd_utils.mask_ego_points' box) or with floor((p - lo) / voxel)
    (fp32, rounded subtract and divide) outside the grid are dropped; the first kept point of a cell opens a voxel, voxels are numbered
    in order of their first point, at most max_voxels per agent (cells past the cap are dropped with all their points); a voxel keeps the
    first max_points (<= 32) points of its cell.
    -> voxel_features (N max_voxels, T, 4) fp32, voxel_coords (N max_voxels, 4) int32 [a, 0, y, x], voxel_num_points (N max_voxels)
    int32, num_voxels (N,) int32.  Agent a's voxels start at row a * max_voxels.  Rows without a voxel hold voxel_coords [-1, 0, 0, 0]
    and voxel_num_points 0 - the padding rows pillar_vfe_scatter skips - and their voxel_features are NOT written (they keep what
    `out=` held, or are uninitialised): clearing them would cost more than the operator.  out = the four tensors to write into;
    workspace = an int32 tensor of at least voxelize_workspace_ints(...) elements (default: one cached per shape and device).
    Bitwise reproducible: nothing depends on scheduling."""
    return _voxelize("voxelize_points", points, point_offsets, lidar_range, voxel_size, max_points, max_voxels, range_mask, ego_mask, out,
                     workspace, None)


def _voxelize(what, points, point_offsets, lidar_range, voxel_size, max_points, max_voxels, range_mask, ego_mask, out, workspace, slots):
    """voxelize_points (slots None: the dense tables, nz = 1) and voxelize_points_3d (slots: the hash table's entries, 0 = the default)"""
    _need_cuda(points, point_offsets, workspace)
    offs, n, m, dev = _points_offsets(what, points, point_offsets)
    if max_voxels is None or int(max_voxels) < 1:
        raise CobevtHipError("%s: max_voxels (per agent, >= 1) is required" % what)
    nx, ny, nz = voxel_grid_size(lidar_range, voxel_size)
    if slots is None and nz != 1:
        raise CobevtHipError("voxelize_points: the pillar front end implements nz = 1 (one voxel over the height), got grid (%d, %d, %d)"
                             % (nx, ny, nz))
    t, mv = int(max_points), int(max_voxels)
    if t < 1 or t > PILLAR_MAX_POINTS:
        raise CobevtHipError("%s: 1 <= max_points <= T = %d points per voxel are supported, got %d" % (what, PILLAR_MAX_POINTS, t))
    if nx < 1 or ny < 1 or nz < 1:
        raise CobevtHipError("%s: empty grid (%d, %d, %d)" % (what, nx, ny, nz))
    pcap = n * mv
    flags = (int(bool(range_mask)), int(bool(ego_mask)))
    if slots is None:
        dims = (ctypes.c_long * 9)(m, n, t, mv, nx, ny, nz, *flags)
        key, ws_ints = WORKSPACE_KEYS["voxelize"](m, n, t, mv, nx, ny), lambda: voxelize_workspace_ints(m, n, (nx, ny, nz), t, mv)       # noqa: E731
    else:
        dims = (ctypes.c_long * 10)(m, n, t, mv, nx, ny, nz, *flags, slots)
        key, ws_ints = WORKSPACE_KEYS["voxelize3d"](m, n, t, mv, slots), lambda: voxelize3d_workspace_ints(m, n, t, mv, slots)       # noqa: E731
    geom = (ctypes.c_float * 9)(*[float(v) for v in list(lidar_range) + list(voxel_size)])
    # (the 3-D form's workspace starts with the hash table's 64-bit keys)
    workspace = _workspace(what, "voxelize" if slots is None else "voxelize3d", dev, key, ws_ints, workspace, align=4 if slots is None else 8)
    shapes = [((pcap, t, 4), torch.float32), ((pcap, 4), torch.int32), ((pcap,), torch.int32), ((n,), torch.int32)]
    if out is None:
        out = [None] * 4
    elif len(out) != 4:
        raise CobevtHipError("%s: out= is (voxel_features, voxel_coords, voxel_num_points, num_voxels)" % what)
    vf, coords, npts, nvox = [_canvas(o, s, d, dev, what) for o, (s, d) in zip(out, shapes)]
    if slots is None:
        cost = lambda: (0.0, 32.0 * m + 16.0 * m + 16.0 * (n * ny * nx) + 24.0 * pcap)         # noqa: E731
        with _timed("voxelize|M%d N%d T%d %dx%d" % (m, n, t, ny, nx), cost):
            _L.call("cobevt_voxelize_points", _p(points), _p(offs), _p(vf), _p(coords), _p(npts), _p(nvox), _p(workspace), dims, geom, _stream())
    else:
        table = voxelize3d_table_slots(m, slots)
        cost = lambda: (0.0, 32.0 * m + 16.0 * m + 24.0 * table + 24.0 * pcap)                 # noqa: E731
        with _timed("voxelize3d|M%d N%d T%d %dx%dx%d S%d" % (m, n, t, nz, ny, nx, table), cost):
            _L.call("cobevt_voxelize3d_points", _p(points), _p(offs), _p(vf), _p(coords), _p(npts), _p(nvox), _p(workspace), dims, geom,
                    _stream())
    return vf, coords, npts, nvox


def voxelize3d_table_slots(num_points, table_slots=None):
    """entries of voxelize_points_3d's hash table: table_slots, or by default the smallest power of two >= max(2 M, 64), at most 2^31"""
    if table_slots:
        return int(table_slots)
    slots = 64
    while slots < 2 * int(num_points):
        slots *= 2
    return min(slots, 1 << 31)


def voxelize3d_workspace_ints(num_points, num_agents, max_points, max_voxels, table_slots=None):
    """int32 elements of voxelize_points_3d's workspace for M points of N agents (cobevt_voxelize3d_scratch): it follows M, the table
    (table_slots, default: voxelize3d_table_slots) and N max_voxels, not the grid"""
    return _scratch("cobevt_voxelize3d_scratch", _longs(num_points, num_agents, max_points, max_voxels, 1, 1, 1, 0, 0, table_slots or 0))


def voxelize_points_3d(points, point_offsets, lidar_range, voxel_size, max_points=32, max_voxels=None, range_mask=False, ego_mask=False,
                       out=None, workspace=None, table_slots=None):
    """voxelize_points on a 3-D grid (csrc/voxelize.hip, cobevt_voxelize3d_points): the voxel dict of host.MeanVFE / VoxelBackBone8x from
    raw points, without a host synchronisation.  Arguments, drop rules, numbering, cap, padding rows and `out=` exactly as
    voxelize_points; the cell is (z, y, x) with z = floor((p.z - z0) / voxel z) in [0, nz), any nz >= 1 (each of nx, ny, nz <= 2^24).
    -> voxel_features (N max_voxels, T, 4) fp32, voxel_coords (N max_voxels, 4) int32 [a, z, y, x], voxel_num_points, num_voxels (N,);
    on an nz = 1 grid all four equal voxelize_points'.
    The per-cell tables are indexed through an open-addressed hash table of table_slots entries (a power of two > M; default
    voxelize3d_table_slots(M): a load of at most one half), so time and workspace follow M, the table and N max_voxels and not the grid - the
    dense tables of voxelize_points would take 1.48 GB per agent at (1408, 1600, 41).  A smaller table only lengthens the probe
    sequences; the result is the same.  workspace = an int32 tensor of at least voxelize3d_workspace_ints(...) elements on an 8-byte
    boundary (default: one cached per shape and device).  Bitwise reproducible: nothing in the outputs depends on scheduling."""
    slots = 0 if table_slots is None else int(table_slots)
    if table_slots is not None and (slots < 1 or slots & (slots - 1) or slots <= points.shape[0] or slots > 1 << 31):
        raise CobevtHipError("voxelize_points_3d: table_slots must be a power of two above the %d points and at most 2^31, got %r"
                             % (points.shape[0], table_slots))
    return _voxelize("voxelize_points_3d", points, point_offsets, lidar_range, voxel_size, max_points, max_voxels, range_mask, ego_mask,
                     out, workspace, slots)


CLOUD_MAX_BOXES = 128      # ground-truth rows cobevt_prepare_points augments (one thread each of one workgroup)
_WORLD_KEYS = ("flip_x", "flip_y", "rot", "scale")


def prepare_points_workspace_ints(num_points, num_agents=1):
    """int32 elements of prepare_points' workspace for M points of N agents (cobevt_prepare_points_scratch)"""
    return _scratch("cobevt_prepare_points_scratch", _longs(num_points, num_agents, 0, 0, 0, 0, 0, 0, 0, 0))


def rotation_cos_sin(angle):
    """(cos, sin) as common_utils.rotate_points_along_z makes them: torch.cos / torch.sin of the fp32 angle on the CPU"""
    a = torch.tensor([float(angle)], dtype=torch.float64).float()
    return float(torch.cos(a)[0]), float(torch.sin(a)[0])


def prepare_points(points, point_offsets, transforms=None, *, order=None, ego_mask=False, lidar_range=None, world=None, boxes=None,
                   box_mask=None, out=None, workspace=None):
    """Per-agent sensor-frame clouds -> one compact ego-frame cloud (csrc/cloud_prep.hip), without a host synchronisation: what the
    reference's datasets do in NumPy in front of the pre-processors.
    points (M, 4) contiguous fp32 [x, y, z, intensity] and point_offsets (N + 1,) int32 / int64 on the device, as voxelize_points
    takes them (rows at or past offsets[N] are ignored).  Per agent, in input order - with order (M,) int32 / int64 on the device in
    the order points[order[i]]; order must map each agent's row range onto itself, which is not checked (host.shuffle_order makes one):
      1 ego_mask: pcd_utils.mask_ego_points on the sensor-frame point (limits rounded to fp32, voxelize_points' rule);
      2 transforms (N, 4, 4) fp64 on the device (fp32: converted on the device): pcd_utils.lidar_project in fp64 as
        ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]; None skips the stage;
      3 world = dict(flip_x=bool, flip_y=bool, rot=float | None, scale=float | None), always in this order:
        augment_utils.random_flip_along_x (y negated), random_flip_along_y (x negated), global_rotation (x, y, z rounded to fp32,
        x c - y s and x s + y c in fp64 from fp32 values, rounded to fp32), global_scaling (fl32(v * fl32(scale)));
      4 the point is rounded to fp32;
      5 lidar_range = [x0, y0, z0, x1, y1, z1]: pcd_utils.mask_points_by_range on the fp32 OUTPUT point with the limits rounded to
        fp32 (where the reference still holds fp64 points it compares in fp64: a point within half an fp32 ulp of a limit can differ);
      6 the kept points are written densely, in order.
    -> points_out (M, 4) fp32, out_offsets (N + 1,) int32: agent a's points are rows out_offsets[a] .. out_offsets[a + 1]; rows at or
    past out_offsets[N] are NOT written (they keep what `out=` held).  Non-finite values get no rule of their own: a NaN survives the
    ego mask and fails the range mask.
    boxes (G <= 128, 7) and box_mask (G,), both fp32 or both fp64, contiguous, on the device: rows with mask == 1 get stage 3 IN PLACE
    as augment_utils applies it to boxes (flip_x: y and heading negated; flip_y: x negated, heading <- -(h + pi); rot: x, y, z rounded
    to fp32 and rotated, heading += rot; scale: columns 0 .. 5), in fp64 with one rounding to the dtype; other rows are untouched.
    The reference compacts the valid rows to the front and leaves the mask alone, which is the same thing whenever the mask is a
    prefix - and generate_object_center always produces a prefix.
    Every call augments the boxes again: a captured graph that holds the call does so on each replay, so refresh the boxes' buffer
    before a replay (as pipeline.CapturedCall does with its arguments) or keep the boxes out of the captured call.
    out = (points_out, out_offsets) to write into, points_out not overlapping points; workspace = an int32 tensor of at least prepare_points_workspace_ints(M) elements
    whose storage is 8-byte aligned (default: one cached per shape and device).  Bitwise reproducible."""
    _need_cuda(points, point_offsets, transforms, order, boxes, box_mask, workspace, *(out or ()))
    offs, n, m, dev = _points_offsets("prepare_points", points, point_offsets)
    if transforms is not None:
        if transforms.dtype not in (torch.float64, torch.float32) or tuple(transforms.shape) != (n, 4, 4):
            raise CobevtHipError("prepare_points: transforms must be fp64 (or fp32) (N, 4, 4) with N = %d agents, got %s %s"
                                 % (n, transforms.dtype, tuple(transforms.shape)))
        transforms = transforms.to(torch.float64).contiguous()
    if order is not None:
        order = _index_i32(order, "prepare_points: order")
        if tuple(order.shape) != (m,):
            raise CobevtHipError("prepare_points: order must be (M,) with M = %d rows, got %s" % (m, tuple(order.shape)))
    rng = [0.0] * 6
    if lidar_range is not None:
        rng = [float(v) for v in lidar_range]
        if len(rng) != 6 or not all(np.isfinite(rng)):
            raise CobevtHipError("prepare_points: lidar_range = [x0, y0, z0, x1, y1, z1], got %r" % (list(lidar_range),))
    world = dict(world or {})
    if any(k not in _WORLD_KEYS for k in world):
        raise CobevtHipError("prepare_points: world = dict(flip_x, flip_y, rot, scale), got the keys %r" % (sorted(world),))
    rot, scale = world.get("rot"), world.get("scale")
    if (rot is not None and not np.isfinite(float(rot))) or (scale is not None and not np.isfinite(float(scale))):
        raise CobevtHipError("prepare_points: world['rot'] and world['scale'] are finite numbers or None, got %r / %r" % (rot, scale))
    cos, sin = rotation_cos_sin(rot) if rot is not None else (1.0, 0.0)
    g = 0
    if boxes is not None or box_mask is not None:
        if boxes is None or box_mask is None or boxes.dtype not in (torch.float32, torch.float64) or boxes.dim() != 2 \
                or boxes.shape[1] != 7 or not boxes.is_contiguous():
            raise CobevtHipError("prepare_points: boxes must be contiguous fp32 or fp64 (G, 7), with box_mask (G,)")
        g = boxes.shape[0]
        if box_mask.dtype != boxes.dtype:
            raise CobevtHipError("prepare_points: boxes and box_mask must have the same dtype, got %s and %s" % (boxes.dtype, box_mask.dtype))
        if tuple(box_mask.shape) != (g,) or not box_mask.is_contiguous():
            raise CobevtHipError("prepare_points: box_mask must be contiguous (G,) with G = %d, got %s" % (g, tuple(box_mask.shape)))
        if g > CLOUD_MAX_BOXES:
            raise CobevtHipError("prepare_points: at most G = %d boxes are supported, got %d" % (CLOUD_MAX_BOXES, g))
    workspace = _workspace("prepare_points", "prepare_points", dev, WORKSPACE_KEYS["prepare_points"](m),
                           lambda: prepare_points_workspace_ints(m, n), workspace, align=8)
    if out is None:
        out = (None, None)
    elif len(out) != 2:
        raise CobevtHipError("prepare_points: out= is (points_out, out_offsets)")
    pts_out = _canvas(out[0], (m, 4), torch.float32, dev, "prepare_points")
    if m and pts_out.data_ptr() < points.data_ptr() + 16 * m and points.data_ptr() < pts_out.data_ptr() + 16 * m:
        raise CobevtHipError("prepare_points: out= must not overlap points (the scatter launch reads points while it writes out)")
    out_offs = _canvas(out[1], (n + 1,), torch.int32, dev, "prepare_points")
    dims = (ctypes.c_long * 10)(m, n, g, int(bool(ego_mask)), int(lidar_range is not None), int(bool(world.get("flip_x"))),
                                int(bool(world.get("flip_y"))), int(rot is not None), int(scale is not None),
                                int(g > 0 and boxes.dtype == torch.float64))
    geom = (ctypes.c_double * 10)(*(rng + [cos, sin, float(rot or 0.0), float(1.0 if scale is None else scale)]))
    with _timed("prepare_points|M%d N%d G%d" % (m, n, g), lambda: (0.0, 16.0 * m + 16.0 * m + 16.0 * m)):
        _L.call("cobevt_prepare_points", _p(points) if m else None, _p(offs), _p(transforms), _p(order) if m else None,
                _p(pts_out) if m else None, _p(out_offs), _p(boxes) if g else None, _p(box_mask) if g else None, _p(workspace), dims, geom,
                _stream())
    return pts_out, out_offs


# ----------------------------------------------------------------------------------------------
# the sparse 3-D voxel backbone (csrc/sparse_conv.hip): MeanVFE, active-set indices, SubMConv3d / SparseConv3d, dense()
# ----------------------------------------------------------------------------------------------
SPARSE_TILE_ROWS = 32      # output rows of one MFMA tile of cobevt_sparse_conv: the unit that skips absent taps
SPARSE_BLOCK_ROWS = 128    # ... and of one workgroup (four tiles)


def sparse_row_channels(channels, dtype):
    """channels of one feature row as cobevt_sparse_conv reads it: a whole number of 32-byte groups (16 bf16 / 8 fp32)"""
    g = 16 if dcode(dtype) == BF16 else 8
    return (int(channels) + g - 1) // g * g


def mean_vfe(voxel_features, voxel_num_points, voxel_coords=None, dtype=torch.float32, channels=None, out=None):
    """MeanVFE (csrc/sparse_conv.hip) in one launch: voxel_features (P, T, C) contiguous fp32, voxel_num_points (P,) int32 / int64 ->
    (P, channels) in `dtype`: per voxel the sum of its first voxel_num_points point slots, in slot order, divided by
    max(voxel_num_points, 1) - the reference's sum over all T slots whenever the unused ones are zero, which spconv guarantees.
    channels (default C, at most 64) >= C pads every row with zeros: sparse_row_channels(C, dtype) is the row cobevt_sparse_conv reads.
    With voxel_coords (P, 4) the rows with a batch index < 0 (the padding rows of a fixed-size voxel dict) are zero."""
    _need_cuda(voxel_features, voxel_num_points, voxel_coords, out)
    if voxel_features.dtype != torch.float32 or voxel_features.dim() != 3 or not voxel_features.is_contiguous():
        raise CobevtHipError("mean_vfe: voxel_features must be contiguous fp32 (P, T, C), got %s %s" % (voxel_features.dtype, tuple(voxel_features.shape)))
    p, t, c = voxel_features.shape
    cpad = c if channels is None else int(channels)
    if t < 1 or c < 1 or cpad < c or cpad > 64:
        raise CobevtHipError("mean_vfe: T >= 1 point slots and 1 <= C <= channels <= 64 are supported, got T = %d, C = %d, channels = %d" % (t, c, cpad))
    npts = _index_i32(voxel_num_points, "mean_vfe: voxel_num_points")
    if tuple(npts.shape) != (p,):
        raise CobevtHipError("mean_vfe: voxel_num_points must be (P,) with P = %d, got %s" % (p, tuple(npts.shape)))
    coords = None
    if voxel_coords is not None:
        coords = _index_i32(voxel_coords, "mean_vfe: voxel_coords", (4,))
        if coords.shape[0] != p:
            raise CobevtHipError("mean_vfe: voxel_coords must be (P, 4) with P = %d" % p)
    out = _canvas(out, (p, cpad), dtype, voxel_features.device, "mean_vfe")
    dims = (ctypes.c_long * 5)(dcode(dtype), p, t, c, cpad)
    with _timed("mean_vfe|P%d T%d C%d" % (p, t, c), lambda: (float(p * t * c), 4.0 * p * t * c + out.element_size() * p * cpad)):
        _L.call("cobevt_mean_vfe", _p(voxel_features), _p(npts), _p(coords), _p(out), dims, _stream())
    return out


def _sparse_shape(batch_size, spatial_shape, what):
    shape = tuple(int(v) for v in spatial_shape)
    n = int(batch_size)
    if len(shape) != 3 or n < 1 or min(shape) < 1:
        raise CobevtHipError("%s: batch_size >= 1 and spatial_shape = (D, H, W) >= 1 are needed, got %r / %r" % (what, batch_size, list(spatial_shape)))
    return n, shape


def sparse_workspace_ints(batch_size, spatial_shape):
    """int32 elements of one level's index workspace - a bit per cell, a popcount prefix per 32-bit word, the scan's partials - for
    batch_size samples on the sparse shape (D, H, W) (cobevt_sparse_scratch)"""
    n, shape = _sparse_shape(batch_size, spatial_shape, "sparse_workspace_ints")
    return _scratch("cobevt_sparse_scratch", _longs(n, *shape))


def _sparse_ws(workspace, dev, n, shape, what):
    return _workspace(what, "sparse", dev, WORKSPACE_KEYS["sparse"](n, shape), lambda: sparse_workspace_ints(n, shape), workspace, align=16)


def sparse_out_shape(spatial_shape, kernel, stride, padding):
    """the output shape of SparseConv3d: floor((n + 2 p - k) / s) + 1 per axis"""
    return tuple((int(n) + 2 * p - k) // s + 1 for n, k, s, p in zip(spatial_shape, kernel, stride, padding))


def _triple(v):
    return (int(v),) * 3 if isinstance(v, (int, np.integer)) else tuple(int(x) for x in v)


class SparseConvTensor(object):
    """A level of the sparse backbone, the holder the reference gets from spconv:
      features       (capacity, C) in the compute dtype; rows at or past the live count are NOT written
      indices        (capacity, 4) int32 [b, z, y, x], rows ordered by the cell index ((b D + z) H + y) W + x
      num            (2,) int32 ON THE DEVICE: [live rows, rows dropped because the capacity was smaller than the active set]
      spatial_shape  (D, H, W); batch_size
    dense() -> (N, C, D, H, W), zero off the active set.  `workspace` is the level's index (sparse_workspace_ints), `row_map` - only on
    what sparse_index returns - the input row each level row reads its features from."""

    def __init__(self, features, indices, num, spatial_shape, batch_size, workspace, row_map=None):
        self.features, self.indices, self.num = features, indices, num
        self.spatial_shape, self.batch_size = tuple(int(v) for v in spatial_shape), int(batch_size)
        self.workspace, self.row_map = workspace, row_map

    @property
    def capacity(self):
        return int(self.indices.shape[0])

    def dense(self):
        return sparse_dense(self)


def sparse_index(voxel_coords, batch_size, spatial_shape, features=None, capacity=None, workspace=None):
    """The active set of level 0 from voxel_coords (P, 4) int32 / int64 [b, z, y, x] on the sparse shape (D, H, W)
    (cobevt_sparse_index), without a host read and independent of scheduling -> SparseConvTensor whose rows are ordered by cell index.
    Rows with b < 0 (padding rows) or a coordinate outside the shape are ignored; of duplicate cells the lowest input row wins.
    capacity (default P: nothing can be dropped) bounds the rows; cells past it are dropped from the high end of the cell order and
    counted in num[1].  features (P, C) are NOT permuted: the tensor keeps them with row_map (capacity,), and the first convolution
    reads row r of the level from features[row_map[r]].  workspace = an int32 tensor of at least sparse_workspace_ints(...) elements
    (default: one cached per shape and device, so a second index of the same shape replaces the first)."""
    _need_cuda(voxel_coords, features, workspace)
    n, shape = _sparse_shape(batch_size, spatial_shape, "sparse_index")
    coords = _index_i32(voxel_coords, "sparse_index: voxel_coords", (4,))
    p, dev = coords.shape[0], coords.device
    cap = max(p, 1) if capacity is None else int(capacity)
    if cap < 1:
        raise CobevtHipError("sparse_index: capacity must be >= 1, got %d" % cap)
    if features is not None and (features.dim() != 2 or features.shape[0] != p or not features.is_contiguous()):
        raise CobevtHipError("sparse_index: features must be contiguous (P, C) with P = %d, got %s" % (p, tuple(features.shape)))
    workspace = _sparse_ws(workspace, dev, n, shape, "sparse_index")
    indices = torch.empty((cap, 4), device=dev, dtype=torch.int32)
    num = torch.empty((2,), device=dev, dtype=torch.int32)
    source = torch.empty((cap,), device=dev, dtype=torch.int32)
    dims = (ctypes.c_long * 6)(n, shape[0], shape[1], shape[2], p, cap)
    cells = n * shape[0] * shape[1] * shape[2]
    with _timed("sparse_index|P%d N%d %dx%dx%d" % ((p, n) + shape), lambda: (0.0, 32.0 * p + cells / 8.0 * 5 + 20.0 * cap)):
        _L.call("cobevt_sparse_index", _p(coords) if p else None, _p(workspace), _p(indices), _p(num), _p(source), dims, _stream())
    return SparseConvTensor(features, indices, num, shape, n, workspace, row_map=source)


def sparse_downsample(x, kernel, stride, padding, capacity=None, workspace=None):
    """The output level of SparseConv3d(kernel, stride, padding) over the level x (cobevt_sparse_downsample): a cell is active when
    any input of its receptive field is -> SparseConvTensor without features.  capacity: default the provable bound
    min(cells of the output level, outputs one input can mark x x's capacity) - 8 x for kernel 3 / stride 2, 2 x for (3, 1, 1) /
    (2, 1, 1) -, with which nothing can be dropped; a smaller one drops the cells past it from the high end of the cell order."""
    k, s, p = _triple(kernel), _triple(stride), _triple(padding)
    _need_cuda(x.indices, x.num, workspace)
    so = sparse_out_shape(x.spatial_shape, k, s, p)
    if min(so) < 1:
        raise CobevtHipError("sparse_downsample: a %s level has no output under kernel %s, stride %s, padding %s" % (x.spatial_shape, k, s, p))
    n, dev = x.batch_size, x.indices.device
    if capacity is None:
        fan = 1
        for kk, ss in zip(k, s):
            fan *= (kk + ss - 1) // ss
        capacity = min(n * so[0] * so[1] * so[2], fan * x.capacity)
    cap = int(capacity)
    if cap < 1:
        raise CobevtHipError("sparse_downsample: capacity must be >= 1, got %d" % cap)
    workspace = _sparse_ws(workspace, dev, n, so, "sparse_downsample")
    indices = torch.empty((cap, 4), device=dev, dtype=torch.int32)
    num = torch.empty((2,), device=dev, dtype=torch.int32)
    dims = (ctypes.c_long * 15)(n, *(x.spatial_shape + (x.capacity, cap) + k + s + p))
    cells = n * so[0] * so[1] * so[2]
    with _timed("sparse_downsample|%dx%dx%d" % so, lambda: (0.0, 16.0 * x.capacity + cells / 8.0 * 5 + 16.0 * cap)):
        _L.call("cobevt_sparse_downsample", _p(x.indices), _p(x.num), _p(workspace), _p(indices), _p(num), dims, _stream())
    return SparseConvTensor(None, indices, num, so, n, workspace)


class SparseConvPlan(object):
    """spconv's SubMConv3d / SparseConv3d (bias=False) + the eval BatchNorm1d + ReLU that follow it, lowered to cobevt_sparse_conv:
    `wgt` [taps][Cout padded to 32][Cin padded to the 32-byte row] = weight[co, kz, ky, kx, ci] * bn_scale[co] (folded in float64,
    then rounded to the compute dtype), tap = (kz KY + ky) KX + kx, and `shift` fp32 [Cout padded].  weight: (Cout, kz, ky, kx, Cin),
    the spconv 2.x layout; the sum is a cross-correlation (input cell = stride * output cell - padding + tap).  subm: the output set
    is the input set (kernel 3, stride 1, padding 1).  device="cpu" builds the same tensors without a GPU."""

    PAIRS = ((16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128))

    def __init__(self, weight, bn=None, stride=1, padding=0, subm=False, dtype=torch.bfloat16, device="cuda"):
        if weight.dim() != 5:
            raise CobevtHipError("SparseConvPlan: weight must be (Cout, kz, ky, kx, Cin), got %s" % (tuple(weight.shape),))
        cout, kz, ky, kx, cin = (int(d) for d in weight.shape)
        self.kernel, self.stride, self.padding, self.subm = (kz, ky, kx), _triple(stride), _triple(padding), bool(subm)
        self.dtype, self.code = dtype, dcode(dtype)
        if self.subm and (self.kernel, self.stride, self.padding) != ((3, 3, 3), (1, 1, 1), (1, 1, 1)):
            raise CobevtHipError("SparseConvPlan: SubMConv3d is supported with kernel 3, stride 1, padding 1, got %s / %s / %s"
                                 % (self.kernel, self.stride, self.padding))
        if self.kernel not in ((3, 3, 3), (3, 1, 1)) or self.stride not in ((1, 1, 1), (2, 2, 2), (2, 1, 1)) \
                or self.padding not in ((1, 1, 1), (0, 1, 1), (0, 0, 0)) or (self.kernel == (3, 1, 1) and self.padding != (0, 0, 0)):
            raise CobevtHipError("SparseConvPlan: kernel 3 or (3, 1, 1), stride 1, 2 or (2, 1, 1) and padding 1, (0, 1, 1) or 0 are "
                                 "supported, got %s / %s / %s" % (self.kernel, self.stride, self.padding))
        if not ((cin <= 8 and cout == 16) or (cin, cout) in self.PAIRS):
            raise CobevtHipError("SparseConvPlan: %d -> %d channels; supported are <= 8 -> 16 and %s" % (cin, cout, ", ".join("%d -> %d" % p for p in self.PAIRS)))
        w = weight.detach().double().cpu()
        shift = torch.zeros(cout, dtype=torch.float64)
        if bn is not None:
            sc, shift = (t.cpu() for t in bn_affine(bn))
            w = w * sc[:, None, None, None, None]
        self.cin, self.cout, self.taps = cin, cout, kz * ky * kx
        self.cin_pad, self.cout_pad = sparse_row_channels(cin, dtype), (cout + 31) // 32 * 32
        wk = torch.zeros(self.taps, self.cout_pad, self.cin_pad, dtype=torch.float64)
        wk[:, :cout, :cin] = w.permute(1, 2, 3, 0, 4).reshape(self.taps, cout, cin)
        sh = torch.zeros(self.cout_pad, dtype=torch.float64)
        sh[:cout] = shift
        self.wgt = wk.to(torch.float32).to(dtype).to(device).contiguous()
        self.shift = sh.to(torch.float32).to(device).contiguous()


def sparse_conv3d(x, plan, capacity=None, workspace=None, out_level=None):
    """One SubMConv3d / SparseConv3d + BatchNorm + ReLU of the plan over the SparseConvTensor x (cobevt_sparse_conv): one launch,
    output-stationary (no floating-point atomics, bitwise reproducible), taps that no row of a 32-row tile has are skipped.
    x.features (rows, plan.cin_pad) contiguous in plan.dtype.  SubM: the result shares x's indices / num / workspace.  Strided: the
    output level comes from sparse_downsample(x, ..., capacity, workspace) first (two calls), or is `out_level` if the caller has it.
    -> SparseConvTensor with features (capacity, Cout); rows at or past num[0] are not written."""
    p = plan
    f = x.features
    if f is None or f.dim() != 2 or f.shape[1] != p.cin_pad or f.dtype != p.dtype or not f.is_contiguous():
        raise CobevtHipError("sparse_conv3d: x.features must be contiguous (rows, %d) %s for this plan, got %s"
                             % (p.cin_pad, p.dtype, None if f is None else "%s %s" % (f.dtype, tuple(f.shape))))
    _need_cuda(f, x.indices, x.num, x.workspace, x.row_map, p.wgt, p.shift)
    if x.row_map is None and f.shape[0] != x.capacity:
        raise CobevtHipError("sparse_conv3d: x.features has %d rows, the level's capacity is %d" % (f.shape[0], x.capacity))
    if p.subm:
        level = x
    elif out_level is not None:
        level = out_level
        if level.spatial_shape != sparse_out_shape(x.spatial_shape, p.kernel, p.stride, p.padding) or level.batch_size != x.batch_size:
            raise CobevtHipError("sparse_conv3d: out_level is %s, the plan's output on %s is %s"
                                 % (level.spatial_shape, x.spatial_shape, sparse_out_shape(x.spatial_shape, p.kernel, p.stride, p.padding)))
    else:
        level = sparse_downsample(x, p.kernel, p.stride, p.padding, capacity, workspace)
    cap = level.capacity
    out = torch.empty((cap, p.cout), device=f.device, dtype=p.dtype)
    dims = (ctypes.c_long * 18)(p.code, x.batch_size, *(x.spatial_shape + (f.shape[0], cap, p.cin_pad, p.cout) + p.kernel + p.stride + p.padding))

    def cost():       # an upper bound: the live rows and the taps present are known on the device only
        esz = f.element_size()
        return 2.0 * cap * p.taps * p.cin_pad * p.cout, float(esz * (cap * p.taps * p.cin_pad + p.wgt.numel() + cap * p.cout))

    fam = "sparse_conv|%s k%d%d%d s%d%d%d %d->%d %dx%dx%d" % (("subm" if p.subm else "spconv",) + p.kernel + p.stride + (p.cin, p.cout) + level.spatial_shape)
    with _timed(fam, cost):
        _L.call("cobevt_sparse_conv", _p(f), _p(x.workspace), _p(x.num), _p(x.row_map), _p(level.indices), _p(level.num), _p(p.wgt),
                _p(p.shift), _p(out), dims, _stream())
    return SparseConvTensor(out, level.indices, level.num, level.spatial_shape, level.batch_size, level.workspace)


def sparse_dense_nhwc(x):
    """SparseConvTensor -> (N, H, W, C D) in the features' dtype, channel index c D + d, zero off the active set: the NHWC form of
    HeightCompression's dense().view(N, C D, H, W) (cobevt_sparse_dense: a clear launch and a scatter launch)"""
    f = x.features
    if f is None or f.dim() != 2 or f.shape[0] != x.capacity or not f.is_contiguous() or x.row_map is not None:
        raise CobevtHipError("sparse_dense: the tensor needs contiguous features (capacity, C) in the level's row order")
    _need_cuda(f, x.indices, x.num)
    n, (d, h, w), c = x.batch_size, x.spatial_shape, int(f.shape[1])
    out = torch.empty((n, h, w, c * d), device=f.device, dtype=f.dtype)
    dims = (ctypes.c_long * 7)(dcode(f.dtype), n, d, h, w, x.capacity, c)
    with _timed("sparse_dense|%dx%dx%d C%d" % (d, h, w, c), lambda: (0.0, float(f.element_size() * (out.numel() + 2 * f.numel())))):
        _L.call("cobevt_sparse_dense", _p(f), _p(x.indices), _p(x.num), _p(out), dims, _stream())
    return out


def sparse_dense(x):
    """spconv's SparseConvTensor.dense(): (N, C, D, H, W), zero off the active set - a VIEW of sparse_dense_nhwc's memory, laid out so
    that .view(N, C * D, H, W) works on it and is channels-last (what BaseBEVBackbone reads without a copy)"""
    y = sparse_dense_nhwc(x)
    n, h, w, cd = y.shape
    d = x.spatial_shape[0]
    return y.view(n, h, w, cd // d, d).permute(0, 3, 4, 1, 2)


# ---------------------------------------------------------------------------------------------- training of the sparse backbone
# fp32 rows only.  Every row count is a level's device word num[0]; scratch buffers are cached per size, so a captured graph replays
# on the buffers it saw (the launches of one stream use them one after the other).
SPARSE_ROW_CHUNKS = 64     # row chunks of cobevt_sparse_conv_wgrad and of the BatchNorm sums: ceil(ceil(num[0] / 64) / 32) * 32 rows each
SPARSE_TRAIN_PAIRS = ((8, 16),) + SparseConvPlan.PAIRS          # (input row in channels, Cout)
SPARSE_STAT_DOUBLES = SPARSE_ROW_CHUNKS * 2 * 128              # the BatchNorm entries' partials (cobevt_sparse_train_scratch's second size)


def sparse_train_scratch(cin_pad, cout, taps):
    """(floats of the weight gradient's partials = SPARSE_ROW_CHUNKS x taps x Cout padded to 32 x input row, doubles of the
    BatchNorm entries' partials) - independent of every capacity and grid (cobevt_sparse_train_scratch)"""
    return _scratch("cobevt_sparse_train_scratch", _longs(cin_pad, cout, taps), n=2, packed=True)


def _sparse_train_ws(dev, dtype, n):
    """the partial sums of the training kernels (sparse and transposed convolution): one default buffer per dtype and element count"""
    return _workspace("training scratch", "sparse_train", dev, WORKSPACE_KEYS["sparse_train"](dtype, n), n, None, dtype)


def sparse_train_weights(weight):
    """The module weight (Cout, kz, ky, kx, Cin) fp32 -> the two operand tables of the training kernels, UNfolded: forward
    [taps][Cout padded to 32][input row] and transposed [taps][Cin padded to 32][Cout], tap = (kz KY + ky) KX + kx.  Lowered on the
    device by torch ops - no host round trip per optimiser step, unlike SparseConvPlan - and cached per weight object
    (_lowered_tables: hand over the nn.Parameter itself, the detaching is done there)."""
    if weight.dim() != 5 or weight.dtype != torch.float32:
        raise CobevtHipError("sparse_train_weights: weight must be fp32 (Cout, kz, ky, kx, Cin), got %s %s" % (weight.dtype, tuple(weight.shape)))
    cout, kz, ky, kx, cin = (int(d) for d in weight.shape)
    cin_pad = sparse_row_channels(cin, torch.float32)
    if not ((cin <= 8 and cout == 16) or (cin, cout) in SparseConvPlan.PAIRS) or (kz, ky, kx) not in ((3, 3, 3), (3, 1, 1)):
        raise CobevtHipError("sparse_train_weights: %d -> %d channels, kernel %s; supported are <= 8 -> 16 and %s with kernel 3 or (3, 1, 1)"
                             % (cin, cout, (kz, ky, kx), ", ".join("%d -> %d" % p for p in SparseConvPlan.PAIRS)))
    taps = kz * ky * kx

    def lower(w):
        fwd = torch.zeros((taps, (cout + 31) // 32 * 32, cin_pad), device=w.device, dtype=torch.float32)
        fwd[:, :cout, :cin] = w.permute(1, 2, 3, 0, 4).reshape(taps, cout, cin)
        tr = torch.zeros((taps, (cin_pad + 31) // 32 * 32, cout), device=w.device, dtype=torch.float32)
        tr[:, :cin, :] = w.permute(1, 2, 3, 4, 0).reshape(taps, cin, cout)
        return fwd, tr

    return _lowered_tables("sparse", weight, lower)


def _sparse_geometry(kernel, stride, padding, subm, what):
    k, s, p = _triple(kernel), _triple(stride), _triple(padding)
    if subm:
        if (k, s, p) != ((3, 3, 3), (1, 1, 1), (1, 1, 1)):
            raise CobevtHipError("%s: SubMConv3d is supported with kernel 3, stride 1, padding 1, got %s / %s / %s" % (what, k, s, p))
    elif k not in ((3, 3, 3), (3, 1, 1)) or s not in ((1, 1, 1), (2, 2, 2), (2, 1, 1)) or p not in ((1, 1, 1), (0, 1, 1), (0, 0, 0)) \
            or (k == (3, 1, 1) and p != (0, 0, 0)):
        raise CobevtHipError("%s: kernel 3 or (3, 1, 1), stride 1, 2 or (2, 1, 1) and padding 1, (0, 1, 1) or 0 are supported, got %s / %s / %s"
                             % (what, k, s, p))
    return k, s, p


def sparse_conv_raw(x, level, wgt, cout, kernel, stride, padding, subm):
    """z = conv(x): no BatchNorm, no ReLU (cobevt_sparse_conv_raw, the inference kernel with a plain-store epilogue).  x: the input
    SparseConvTensor with fp32 features (rows, input row) (row_map honoured), level: the output level (x itself for SubM), wgt: the
    forward table of sparse_train_weights -> z (level.capacity, cout) fp32, zeros at and past level.num[0]"""
    k, s, p = _sparse_geometry(kernel, stride, padding, subm, "sparse_conv_raw")
    f = _require_f32(x.features, "sparse_conv_raw: x.features", ("rows" if x.row_map is not None else x.capacity, wgt.shape[2]))
    _need_cuda(f, x.workspace, x.num, x.row_map, level.indices, level.num, wgt)
    cap, cin_pad = level.capacity, int(f.shape[1])
    z = torch.empty((cap, cout), device=f.device, dtype=torch.float32)
    dims = (ctypes.c_long * 17)(x.batch_size, *(x.spatial_shape + (f.shape[0], cap, cin_pad, cout) + k + s + p))
    taps = k[0] * k[1] * k[2]
    fam = "sparse_conv_raw|k%d%d%d s%d%d%d %d->%d %dx%dx%d" % (k + s + (cin_pad, cout) + level.spatial_shape)
    with _timed(fam, lambda: (2.0 * cap * taps * cin_pad * cout, 4.0 * (cap * taps * cin_pad + wgt.numel() + cap * cout))):
        _L.call("cobevt_sparse_conv_raw", _p(f), _p(x.workspace), _p(x.num), _p(x.row_map), _p(level.indices), _p(level.num), _p(wgt), _p(z), dims,
                _stream(), variant="")
    return z


def sparse_bn_relu(z, num, gamma, beta, bn=None, frozen=False, eps=1e-3, momentum=0.01, want_y=True):
    """BatchNorm1d + ReLU over the num[0] live rows of z (capacity, C) (cobevt_sparse_bn_relu) -> (stat (4, C) fp32 = [mean, rstd,
    scale, shift], y | None).  bn: the nn.BatchNorm1d whose eps / momentum hold and whose running statistics are updated in place
    (frozen: read instead, nothing updated); its buffers' version counters are bumped, so eval plans folded from them rebuild."""
    _require_f32(z, "sparse_bn_relu: z", ("rows", "C"))
    cap, c = (int(v) for v in z.shape)
    _need_cuda(z, num, gamma, beta)
    mode = BnTrainMode(bn, "sparse", bool(frozen))
    rm, rv, nbt, bn_eps, bn_momentum = mode.buffers()
    if bn is not None:
        eps = bn_eps
        if rm is not None and not frozen:
            momentum = bn_momentum
        _need_cuda(rm, rv, nbt)
    g, b = gamma.detach(), beta.detach()
    for t, what in ((g, "gamma"), (b, "beta"), (rm, "running_mean"), (rv, "running_var")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (c,) or not t.is_contiguous()):
            raise CobevtHipError("sparse_bn_relu: %s must be contiguous fp32 (%d,), got %s %s" % (what, c, t.dtype, tuple(t.shape)))
    if nbt is not None and nbt.dtype != torch.int64:
        raise CobevtHipError("sparse_bn_relu: num_batches_tracked must be int64, got %s" % nbt.dtype)
    doubles = SPARSE_STAT_DOUBLES
    partial = _sparse_train_ws(z.device, torch.float64, doubles)
    stat = torch.empty((4, c), device=z.device, dtype=torch.float32)
    y = torch.empty_like(z) if want_y else None
    dims = (ctypes.c_long * 4)(cap, c, 1 if frozen else 0, doubles)
    with _timed("sparse_bn_relu|C%d" % c, lambda: (4.0 * cap * c, 4.0 * cap * c * (3 if want_y else 1))):
        _L.call("cobevt_sparse_bn_relu", _p(z), _p(num), _p(g), _p(b), _p(rm), _p(rv), _p(nbt), _p(stat), _p(partial), _p(y), dims,
                ctypes.c_float(eps), ctypes.c_float(momentum), _stream(), variant="")
    mode.written()
    return stat, y


def sparse_bn_relu_bwd(dy, y, z, num, gamma, stat, frozen=False):
    """The backward of sparse_bn_relu (cobevt_sparse_bn_relu_bwd) -> (dz (capacity, C), dgamma (C), dbeta (C)); dy at and past num[0]
    is never read, dz there is 0.  frozen: the statistics were constants (no / n terms)."""
    _require_f32(z, "sparse_bn_relu_bwd: z", ("rows", "C"))
    cap, c = (int(v) for v in z.shape)
    _require_f32(dy, "sparse_bn_relu_bwd: dy", (cap, c))
    _require_f32(y, "sparse_bn_relu_bwd: y", (cap, c))
    _need_cuda(dy, y, z, num, gamma, stat)
    doubles = SPARSE_STAT_DOUBLES
    partial = _sparse_train_ws(z.device, torch.float64, doubles)
    dev = z.device
    dz = torch.empty_like(z)
    dgb = torch.empty((2, c), device=dev, dtype=torch.float32)
    coef = torch.empty((3, c), device=dev, dtype=torch.float32)
    dims = (ctypes.c_long * 4)(cap, c, 1 if frozen else 0, doubles)
    with _timed("sparse_bn_relu_bwd|C%d" % c, lambda: (10.0 * cap * c, 4.0 * cap * c * 7)):
        _L.call("cobevt_sparse_bn_relu_bwd", _p(dy), _p(y), _p(z), _p(num), _p(gamma.detach()), _p(stat), _p(partial), _p(dgb[0]), _p(dgb[1]), _p(coef),
                _p(dz), dims, _stream(), variant="")
    return dz, dgb[0], dgb[1]


def sparse_conv_dgrad(dz, x, level, wgt_t, cin, kernel, stride, padding, subm):
    """The input gradient of sparse_conv_raw (cobevt_sparse_conv_dgrad): dz (level.capacity, Cout) by the OUTPUT level's rows, x the
    input level (its indices / num; features not needed), wgt_t the transposed table -> dx (x.capacity, cin), output-stationary over
    the input rows: a row without a contributing output gets exactly 0, rows at and past x.num[0] too."""
    k, s, p = _sparse_geometry(kernel, stride, padding, subm, "sparse_conv_dgrad")
    cout = int(wgt_t.shape[2])
    _require_f32(dz, "sparse_conv_dgrad: dz", (level.capacity, cout))
    if x.row_map is not None:
        raise CobevtHipError("sparse_conv_dgrad: no gradient is offered through a row_map (the input level of the backbone)")
    _need_cuda(dz, level.workspace, level.num, x.indices, x.num, wgt_t)
    dx = torch.empty((x.capacity, cin), device=dz.device, dtype=torch.float32)
    dims = (ctypes.c_long * 17)(x.batch_size, *(x.spatial_shape + (x.capacity, level.capacity, cin, cout) + k + s + p))
    taps = k[0] * k[1] * k[2]
    fam = "sparse_conv_dgrad|k%d%d%d s%d%d%d %d->%d %dx%dx%d" % (k + s + (cin, cout) + level.spatial_shape)
    with _timed(fam, lambda: (2.0 * x.capacity * taps * cin * cout, 4.0 * (x.capacity * taps * cout + wgt_t.numel() + x.capacity * cin))):
        _L.call("cobevt_sparse_conv_dgrad", _p(dz), _p(level.workspace), _p(level.num), _p(x.indices), _p(x.num), _p(wgt_t), _p(dx), dims, _stream(),
                variant="")
    return dx


def sparse_conv_wgrad(x, level, dz, cin, kernel, stride, padding, subm):
    """The weight gradient of sparse_conv_raw (cobevt_sparse_conv_wgrad, two launches): x the input SparseConvTensor with fp32 features
    (row_map honoured), dz (level.capacity, Cout) -> dW (Cout, kz, ky, kx, cin) fp32, the module's layout.  No floating-point atomics:
    SPARSE_ROW_CHUNKS row chunks sized from level.num[0] on the device, added in chunk order in fp64."""
    k, s, p = _sparse_geometry(kernel, stride, padding, subm, "sparse_conv_wgrad")
    f = _require_f32(x.features, "sparse_conv_wgrad: x.features", ("rows" if x.row_map is not None else x.capacity, "C"))
    cin_pad, cout = int(f.shape[1]), int(dz.shape[1]) if dz is not None and dz.dim() == 2 else -1
    _require_f32(dz, "sparse_conv_wgrad: dz", (level.capacity, "C"))
    if (cin_pad, cout) not in SPARSE_TRAIN_PAIRS or not 1 <= cin <= cin_pad or (cin_pad > 8 and cin != cin_pad):
        raise CobevtHipError("sparse_conv_wgrad: %d (row %d) -> %d channels; supported are <= 8 -> 16 and %s"
                             % (cin, cin_pad, cout, ", ".join("%d -> %d" % q for q in SparseConvPlan.PAIRS)))
    _need_cuda(f, x.workspace, x.num, x.row_map, level.indices, level.num, dz)
    taps = k[0] * k[1] * k[2]
    floats = sparse_train_scratch(cin_pad, cout, taps)[0]
    partial = _sparse_train_ws(f.device, torch.float32, floats)
    dw = torch.empty((cout,) + k + (cin,), device=f.device, dtype=torch.float32)
    cap = level.capacity
    dims = (ctypes.c_long * 19)(x.batch_size, *(x.spatial_shape + (f.shape[0], cap, cin, cin_pad, cout) + k + s + p + (floats,)))
    fam = "sparse_conv_wgrad|k%d%d%d s%d%d%d %d->%d %dx%dx%d" % (k + s + (cin_pad, cout) + level.spatial_shape)
    with _timed(fam, lambda: (2.0 * cap * taps * cin_pad * cout, 4.0 * (cap * taps * (cin_pad + cout) + 2 * floats))):
        _L.call("cobevt_sparse_conv_wgrad", _p(f), _p(x.workspace), _p(x.num), _p(x.row_map), _p(level.indices), _p(level.num), _p(dz), _p(partial),
                _p(dw), dims, _stream(), variant="")
    return dw


def sparse_dense_bwd(dcanvas, x, channels):
    """The adjoint of sparse_dense_nhwc (cobevt_sparse_dense_bwd, one gather launch): dcanvas (N, H, W, C D) contiguous fp32 ->
    (x.capacity, C): every live row's cell, 0 at and past x.num[0]"""
    n, (d, h, w), c = x.batch_size, x.spatial_shape, int(channels)
    if dcanvas.dtype != torch.float32 or tuple(dcanvas.shape) != (n, h, w, c * d) or not dcanvas.is_contiguous():
        raise CobevtHipError("sparse_dense_bwd: the gradient must be contiguous fp32 %s, got %s %s" % ((n, h, w, c * d), dcanvas.dtype, tuple(dcanvas.shape)))
    _need_cuda(dcanvas, x.indices, x.num)
    out = torch.empty((x.capacity, c), device=dcanvas.device, dtype=torch.float32)
    dims = (ctypes.c_long * 6)(n, d, h, w, x.capacity, c)
    with _timed("sparse_dense_bwd|%dx%dx%d C%d" % (d, h, w, c), lambda: (0.0, 8.0 * out.numel())):
        _L.call("cobevt_sparse_dense_bwd", _p(dcanvas), _p(x.indices), _p(x.num), _p(out), dims, _stream(), variant="")
    return out


PIL_PRECISION_BITS = 22    # Pillow's 8-bit resample: 32 - 8 - 2 bits of coefficient
PIL_MAX_TAPS = 17          # taps per output index cobevt_resize_pil_u8 takes: a down-scale of at most 8
BEV_MAX_CLASSES = 16       # label bits cobevt_decode_bev unpacks
_PIL_TAPS = {}             # (n_in, n_out) -> (bounds, coeffs), host, read-only
_PIL_TAPS_DEV = {}         # (device, n_in, n_out) -> the same on the device
_PIL_LUT = {}              # device -> ToTensor's byte -> fp32 table


def pil_ksize(n_in, n_out):
    """taps per output index of Pillow's BILINEAR resample from n_in to n_out samples"""
    return 2 * int(math.ceil(1.0 * max(n_in / n_out, 1.0))) + 1


def pil_resize_taps(n_in, n_out):
    """Pillow's tap tables for resampling one axis from n_in to n_out samples with BILINEAR on 8-bit data (Resample.c:
    precompute_coeffs, then normalize_coeffs_8bpc), evaluated in float64 in Pillow's own order of operations.
    -> bounds int32 (n_out, 2) = [first source index, tap count], coeffs int32 (n_out, ksize) in 22-bit fixed point (zero past
    the tap count).  Pure host function; the arrays are cached and read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise CobevtHipError("pil_resize_taps: n_in and n_out must be positive, got %d -> %d" % (n_in, n_out))
    hit = _PIL_TAPS.get((n_in, n_out))
    if hit is not None:
        return hit
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coeffs = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k, ww = [], 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - a if a < 1.0 else 0.0
            k.append(w)
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            coeffs[xx, x] = int(-0.5 + v * (1 << PIL_PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PIL_PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    _PIL_TAPS[(n_in, n_out)] = (bounds, coeffs)
    return bounds, coeffs


def _pil_taps_device(device, n_in, n_out, what):
    key = (device, n_in, n_out)
    hit = _PIL_TAPS_DEV.get(key)
    if hit is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise CobevtHipError("%s: the tap tables for %d -> %d are not on %s yet and cannot be uploaded while a graph is being "
                                 "captured; call once outside the capture" % (what, n_in, n_out, device))
        b, c = pil_resize_taps(n_in, n_out)
        hit = _PIL_TAPS_DEV[key] = (torch.from_numpy(b.copy()).to(device), torch.from_numpy(c.copy()).to(device))
    return hit


def _pil_lut(device, what):
    lut = _PIL_LUT.get(device)
    if lut is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise CobevtHipError("%s: the byte -> fp32 table is not on %s yet and cannot be uploaded while a graph is being captured; "
                                 "call once outside the capture" % (what, device))
        # the very expression torchvision's ToTensor evaluates per byte (img.to(float32).div(255)), on the host: no device division
        lut = _PIL_LUT[device] = torch.arange(256, dtype=torch.float32).div(255).to(device)
    return lut


def resize_pil_bilinear(images_u8, size, top_crop=0, *, dtype=torch.float32, out=None):
    """Image.resize(size, resample=Image.BILINEAR) of Pillow's 8-bit path, the crop of the top rows and ToTensor, for a stack of
    decoded frames in one launch (csrc/image_ingest.hip): the camera side of the nuScenes LoadDataTransform.
    images_u8 (n, H, W, 3) contiguous uint8 on the device (any storage offset); size = (w_resize, h_resize), Pillow's order;
    top_crop rows of the RESIZED image are cut (and never computed).  With h = h_resize - top_crop, w = w_resize:
      dtype=torch.float32 -> (n, 3, h, w) fp32, each byte through the table arange(256) / 255: ToTensor's result, bit for bit;
      dtype=torch.uint8   -> (n, h, w, 3) uint8, the resized bytes themselves.
    Bit-exact with Pillow: integer tap tables from pil_resize_taps (cached on the device per (n_in, n_out), uploaded on first use -
    outside a graph capture), 22-bit fixed-point passes, the horizontal result rounded to a byte before the vertical pass, an axis
    that keeps its size skipped.  A down-scale above 8 on either axis is refused.  No host synchronisation."""
    what = "resize_pil_bilinear"
    _need_cuda(images_u8, out)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or not images_u8.is_contiguous():
        raise CobevtHipError("%s: images_u8 must be contiguous uint8 (n, H, W, 3), got %s %s"
                             % (what, images_u8.dtype, tuple(images_u8.shape)))
    n, hs, ws, ch = images_u8.shape
    if ch != 3:
        raise CobevtHipError("%s: images_u8 must have 3 channels last, got %d" % (what, ch))
    if n < 1 or hs < 1 or ws < 1:
        raise CobevtHipError("%s: images_u8 must not be empty, got %s" % (what, tuple(images_u8.shape)))
    try:
        wr, hr = (int(v) for v in size)
    except (TypeError, ValueError):
        raise CobevtHipError("%s: size = (w_resize, h_resize), got %r" % (what, size))
    if wr < 1 or hr < 1:
        raise CobevtHipError("%s: size = (w_resize, h_resize) must be positive, got %r" % (what, (wr, hr)))
    top = int(top_crop)
    if top < 0 or top >= hr:
        raise CobevtHipError("%s: top_crop must lie in [0, h_resize = %d), got %d" % (what, hr, top))
    if pil_ksize(ws, wr) > PIL_MAX_TAPS or pil_ksize(hs, hr) > PIL_MAX_TAPS:
        raise CobevtHipError("%s: size: a down-scale above 8 on either axis is not supported, got (%d, %d) -> (%d, %d)"
                             % (what, hs, ws, hr, wr))
    if dtype not in (torch.float32, torch.uint8):
        raise CobevtHipError("%s: dtype must be torch.float32 or torch.uint8, got %s" % (what, dtype))
    dev = images_u8.device
    as_u8 = dtype == torch.uint8
    res = _canvas(out, (n, hr - top, wr, 3) if as_u8 else (n, 3, hr - top, wr), dtype, dev, what)
    hb, hc = _pil_taps_device(dev, ws, wr, what) if ws != wr else (None, None)
    vb, vc = _pil_taps_device(dev, hs, hr, what) if hs != hr else (None, None)
    lut = None if as_u8 else _pil_lut(dev, what)
    dims = _ints([n, hs, ws, ch, hr, wr, top, int(as_u8)])
    with _timed("resize_pil|%dx%d>%dx%d" % (hs, ws, hr, wr), lambda: (0.0, 3.0 * n * hs * ws + res.numel() * res.element_size())):
        _L.call("cobevt_resize_pil_u8", _p(images_u8), _p(res), _p(hb), _p(hc), _p(vb), _p(vc), _p(lut), dims, _stream())
    return res


def decode_bev(labels_i32, num_classes, out=None):
    """The bit-packed nuScenes BEV label -> class planes: labels_i32 (n, h, w) contiguous int32 on the device ->
    (n, num_classes <= 16, h, w) fp32 of (x >> c) & 1 - the reference's decode -> * 255 -> uint8 -> ToTensor, exactly 0.0 or 1.0
    (csrc/image_ingest.hip).  One streaming launch, no host synchronisation."""
    what = "decode_bev"
    _need_cuda(labels_i32, out)
    if labels_i32.dtype != torch.int32 or labels_i32.dim() != 3 or not labels_i32.is_contiguous():
        raise CobevtHipError("%s: labels_i32 must be contiguous int32 (n, h, w), got %s %s"
                             % (what, labels_i32.dtype, tuple(labels_i32.shape)))
    if labels_i32.numel() < 1:
        raise CobevtHipError("%s: labels_i32 must not be empty, got %s" % (what, tuple(labels_i32.shape)))
    c = int(num_classes)
    if c < 1 or c > BEV_MAX_CLASSES:
        raise CobevtHipError("%s: num_classes must lie in 1 .. %d, got %d" % (what, BEV_MAX_CLASSES, c))
    n, h, w = labels_i32.shape
    res = _canvas(out, (n, c, h, w), torch.float32, labels_i32.device, what)
    with _timed("decode_bev|C%d" % c, lambda: (0.0, 4.0 * n * h * w * (1 + c))):
        _L.call("cobevt_decode_bev", _p(labels_i32), _p(res), n, h * w, c, _stream())
    return res


DETECT_TOP = 1000          # box_utils.nms_rotated's `top`: the fixed capacity of the detection outputs
DETECT_MAX_CAV = 16


def detect_workspace_bytes(total_anchors):
    """bytes of detect_post_process' / nms_rotated's workspace for `total_anchors` candidates (cobevt_detect_scratch)"""
    return _scratch("cobevt_detect_scratch", int(total_anchors))


def _detect_workspace(workspace, total, dev, what):
    """(asked for its size on every call, in bytes; the buffer is int64 words)"""
    return _workspace(what, "detect", dev, WORKSPACE_KEYS["detect"](total), (detect_workspace_bytes(total) + 7) // 8, workspace, torch.int64, 8)


def _detect_out(out, dev, what):
    shapes = [((DETECT_TOP, 8, 3), torch.float32), ((DETECT_TOP,), torch.float32), ((DETECT_TOP,), torch.int32), ((1,), torch.int32)]
    if out is None:
        out = [None] * 4
    elif len(out) != 4:
        raise CobevtHipError("%s: out= is (boxes, scores, index, count)" % what)
    return [_canvas(o, sh, d, dev, what) for o, (sh, d) in zip(out, shapes)]


def _to_f32(t, dev, what, shape=None):
    """a contiguous fp32 tensor on `dev` CONVERTED from a tensor or an array (an anchor box is numpy float64 in the reference);
    _require_f32 is the form that refuses instead"""
    t = torch.as_tensor(t)
    if not t.is_floating_point():
        raise CobevtHipError("%s must be floating point, got %s" % (what, t.dtype))
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise CobevtHipError("%s must have shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
    return t


def _head_maps(psm, rm, anchors, what, batch=None):
    """checks of one sample's head maps -> (N, H, W, A); psm may be None"""
    if rm.dtype != torch.float32 or rm.dim() != 4 or not rm.is_contiguous():
        raise CobevtHipError("%s: rm must be contiguous fp32 (N, 7A, H, W), got %s %s" % (what, rm.dtype, tuple(rm.shape)))
    n, c7, h, w = rm.shape
    if tuple(anchors.shape[:2]) != (h, w) or anchors.dim() != 4 or anchors.shape[3] != 7 or anchors.shape[2] * 7 != c7 or c7 == 0:
        raise CobevtHipError("%s: anchors must be (H, W, A, 7) with rm (N, 7A, H, W), got %s and %s"
                             % (what, tuple(anchors.shape), tuple(rm.shape)))
    a = anchors.shape[2]
    if n < 1 or h < 1 or w < 1 or (batch is not None and n != batch):
        raise CobevtHipError("%s: batch size %s expected, got rm %s" % (what, ">= 1" if batch is None else batch, tuple(rm.shape)))
    if psm is not None and (psm.dtype != torch.float32 or tuple(psm.shape) != (n, a, h, w) or not psm.is_contiguous()):
        raise CobevtHipError("%s: psm must be contiguous fp32 %s, got %s %s" % (what, (n, a, h, w), psm.dtype, tuple(psm.shape)))
    return n, h, w, a


def delta_to_boxes3d(deltas, anchors):
    """VoxelPostprocessor.delta_to_boxes3d (csrc/detect_post.hip): deltas = the regression map (N, 7A, H, W) contiguous fp32 on the
    device, channel a * 7 + k = delta k of anchor a; anchors (H, W, A, 7) (tensor or array, any float type) -> boxes3d (N, H W A, 7)
    fp32 in (h, w, a) order: x, y = delta * sqrt(a4^2 + a5^2) + anchor, z = delta * a3 + anchor, sizes exp(delta) * anchor, yaw added."""
    _need_cuda(deltas)
    anc = _to_f32(anchors, deltas.device, "delta_to_boxes3d: anchors")
    n, h, w, a = _head_maps(None, deltas, anc, "delta_to_boxes3d")
    out = torch.empty((n, h * w * a, 7), device=deltas.device, dtype=torch.float32)
    _L.call("cobevt_delta_to_boxes3d", _p(deltas), _p(anc), _p(out), n, h, w, a, _stream())
    return out


def _quads(boxes, dev, what):
    """(N, 8, 3) or (N, 4, 2) -> contiguous fp32 (N, 4, 2): corners 0 .. 3 in xy, the polygon common_utils.convert_format builds"""
    b = torch.as_tensor(boxes)
    if b.dim() != 3 or tuple(b.shape[1:]) not in ((8, 3), (4, 2)) or not b.is_floating_point():
        raise CobevtHipError("%s must be floating point (N, 8, 3) or (N, 4, 2), got %s %s" % (what, b.dtype, tuple(b.shape)))
    return b[:, :4, :2].to(device=dev, dtype=torch.float32).contiguous()


def rotated_iou(a, b):
    """Pairwise IoU of convex quads: a (N, 4, 2) / (N, 8, 3), b (M, 4, 2) / (M, 8, 3) on the device (corners 0 .. 3 in xy, either
    winding) -> (N, M) fp64.  The fp32 corners are clipped in fp64 by the device function the NMS mask uses; a pair whose union has no
    area gives 0."""
    _need_cuda(a, b)
    qa = _quads(a, a.device, "rotated_iou: a")
    qb = _quads(b, a.device, "rotated_iou: b")
    out = torch.empty((qa.shape[0], qb.shape[0]), device=a.device, dtype=torch.float64)
    _L.call("cobevt_rotated_iou", _p(qa), _p(qb), _p(out), qa.shape[0], qb.shape[0], _stream())
    return out


def nms_rotated_device(boxes, scores, threshold, out=None, workspace=None):
    """box_utils.nms_rotated without a host read: boxes (N, 8, 3) or (N, 4, 2) and scores (N) on the device -> the fixed-capacity
    (boxes (1000, 8, 3), scores (1000), index (1000) int32 = kept input rows in pick order, count (1) int32); rows past count zero."""
    _need_cuda(boxes, scores, workspace)
    if boxes.dim() != 3 or tuple(boxes.shape[1:]) not in ((8, 3), (4, 2)) or not boxes.is_floating_point():
        raise CobevtHipError("nms_rotated: boxes must be floating point (N, 8, 3) or (N, 4, 2), got %s %s" % (boxes.dtype, tuple(boxes.shape)))
    dev, n = boxes.device, boxes.shape[0]
    b = boxes.to(torch.float32).contiguous()
    sc = _to_f32(scores, dev, "nms_rotated: scores", (n,))
    ws = _detect_workspace(workspace, n, dev, "nms_rotated")
    ob, osc, oi, oc = _detect_out(out, dev, "nms_rotated")
    _L.call("cobevt_nms_rotated", _p(b) if n else None, _p(sc) if n else None, n, b.shape[1] * b.shape[2], float(threshold), _p(ob),
            _p(osc), _p(oi), _p(oc), _p(ws), _stream())
    return ob, osc, oi, oc


def nms_rotated(boxes, scores, threshold):
    """box_utils.nms_rotated: rotated NMS over the 1000 best-scored of N boxes (N, 8, 3) or (N, 4, 2) on the device -> int32 indices
    of the kept boxes, best score first (equal scores: lower index first).  Reads the count back once (one synchronisation);
    nms_rotated_device does not."""
    _, _, index, count = nms_rotated_device(boxes, scores, threshold)
    return index[:int(count.item())].clone()


def detect_post_process(cavs, score_threshold, nms_thresh, order, out=None, workspace=None):
    """VoxelPostprocessor.post_process on the device, without a synchronisation (csrc/detect_post.hip).
    cavs: a sequence of 1 .. 16 (psm, rm, anchors, transformation_matrix): psm (1, A, H, W) and rm (1, 7A, H, W) contiguous fp32 on
    the device, anchors (H, W, A, 7) and the 4 x 4 matrix tensors or arrays (converted to fp32 on the device; give device tensors to
    capture the call in a graph).  order: the box order ('hwl' reads the size columns as [5, 4, 3], any other as they stand).
    -> boxes (1000, 8, 3) fp32, scores (1000) fp32, index (1000) int32 (global anchor index: cav 0's anchors in (h, w, a) order, then
    cav 1's, ...), count (1) int32, in pick order; rows at and past count are zero.  Survivors of score > score_threshold and the
    reference's box filters, the 1000 best of all cavs, rotated NMS (iou > nms_thresh), then the GT_RANGE mask - see cobevt_hip.h.
    out = the four tensors to write into; workspace = an int64 tensor of detect_workspace_bytes(total anchors) bytes."""
    cavs = list(cavs)
    if not 1 <= len(cavs) <= DETECT_MAX_CAV:
        raise CobevtHipError("detect_post_process: 1 .. %d cavs are supported, got %d" % (DETECT_MAX_CAV, len(cavs)))
    if not isinstance(order, str):
        raise CobevtHipError("detect_post_process: order must be a string such as 'hwl' or 'lhw', got %r" % (order,))
    keep, dims, mats, total = [], [], [], 0
    dev = None
    for c, cav in enumerate(cavs):
        if len(cav) != 4:
            raise CobevtHipError("detect_post_process: cav %d must be (psm, rm, anchors, transformation_matrix)" % c)
        psm, rm, anchors, mat = cav
        _need_cuda(psm, rm)
        dev = psm.device if dev is None else dev
        if psm.device != dev or rm.device != dev:
            raise CobevtHipError("detect_post_process: cav %d is on another device" % c)
        anc = _to_f32(anchors, dev, "detect_post_process: anchors of cav %d" % c)
        _, h, w, a = _head_maps(psm, rm, anc, "detect_post_process: cav %d" % c, batch=1)
        mats.append(_to_f32(mat, dev, "detect_post_process: transformation_matrix of cav %d" % c, (4, 4)))
        keep.append((psm, rm, anc))
        dims += [h, w, a]
        total += h * w * a
    if total > 0x7fffffff // 8:
        raise CobevtHipError("detect_post_process: %d anchors are more than the operator indexes" % total)
    matrices = mats[0].reshape(1, 4, 4) if len(mats) == 1 else torch.stack(mats)
    ws = _detect_workspace(workspace, total, dev, "detect_post_process")
    ob, osc, oi, oc = _detect_out(out, dev, "detect_post_process")
    ptrs = [(ctypes.c_void_p * len(cavs))(*[k[j].data_ptr() for k in keep]) for j in range(3)]
    cost = lambda: (0.0, 36.0 * total + 8.0 * DETECT_TOP * 16 + 200.0 * DETECT_TOP)         # noqa: E731
    with _timed("detect_post|cavs%d N%d" % (len(cavs), total), cost):
        _L.call("cobevt_detect_post", ptrs[0], ptrs[1], ptrs[2], _p(matrices), _ints(dims), len(cavs), int(order == "hwl"),
                float(score_threshold), float(nms_thresh), _p(ob), _p(osc), _p(oi), _p(oc), _p(ws), _stream())
    return ob, osc, oi, oc


DETECT_MAX_GT = 128        # ground-truth slots per sample cobevt_detect_targets takes (the reference's max_num is 100)

# ----------------------------------------------------------------------------------------------
# LiDAR BEV maps, the PIXOR formulation (csrc/bev_points.hip, csrc/bev_labels.hip, the bev mode of csrc/detect_post.hip)
# ----------------------------------------------------------------------------------------------
BEV_TARGET_MEAN = (0.008, 0.001, 0.202, 0.2, 0.43, 1.368)          # lidar_bev_postprocessor.py :24-25
BEV_TARGET_STD_DEV = (0.866, 0.5, 0.954, 0.668, 0.09, 0.111)


def _bev_shape(shape, last, what):
    s = tuple(int(v) for v in shape) if np.ndim(shape) == 1 else ()
    if len(s) != 3 or s[0] < 1 or s[1] < 1 or (last is not None and s[2] != last) or s[2] < 2:
        raise CobevtHipError("%s must be (nx, ny, %s) with nx, ny >= 1, got %r" % (what, "C >= 2" if last is None else last, shape))
    return s


def _bev_params(origin_xy, res, downsample_rate, target_mean, target_std_dev, what):
    """the 16 doubles [L1, W1, res, downsample_rate, target_mean (6), target_std_dev (6)] of cobevt_bev_labels / cobevt_bev_post"""
    vals = [float(origin_xy[0]), float(origin_xy[1]), float(res), float(downsample_rate)]
    mean, std = [float(v) for v in np.asarray(target_mean).reshape(-1)], [float(v) for v in np.asarray(target_std_dev).reshape(-1)]
    if len(mean) != 6 or len(std) != 6 or not all(np.isfinite(vals + mean + std)) or any(v == 0.0 for v in std):
        raise CobevtHipError("%s: target_mean and target_std_dev are 6 finite values each, no zero deviation" % what)
    if not (vals[2] > 0.0 and vals[3] > 0.0):
        raise CobevtHipError("%s: res and downsample_rate must be positive, got %r and %r" % (what, res, downsample_rate))
    return (ctypes.c_double * 16)(*(vals + mean + std))


def bev_points_workspace_ints(num_points, num_agents, input_shape):
    """int32 elements of bev_points' workspace for M points of N agents on an (nx, ny, C) map (cobevt_bev_points_scratch)"""
    return _scratch("cobevt_bev_points_scratch", _longs(num_points, num_agents, input_shape[0], input_shape[1], input_shape[2], 0, 0, 0))


def bev_points(points, point_offsets, lidar_range, origin, res, input_shape, range_mask=False, ego_mask=False, channels_last=False,
               out=None, workspace=None):
    """BevPreprocessor.preprocess for N agents, on the device and without a host synchronisation (csrc/bev_points.hip).
    points (M, 4) contiguous fp32 [x, y, z, intensity] and point_offsets (N + 1,) int32 / int64 on the device, as voxelize_points
    takes them; lidar_range = cav_lidar_range (used by range_mask only), origin = (L1, W1, H1), res the cell size, input_shape =
    (nx, ny, C).  -> bev_input (N, C, nx, ny) fp32, or (N, nx, ny, C) with channels_last: channels 0 .. C - 2 the binary occupancy of
    the height slices at trunc(((double)p - origin) / res), channel C - 1 the mean intensity of the cell's points.  Dropped: points
    with a non-finite value, |intensity| >= 256, removed by a mask, or outside [0, nx) x [0, ny) x [0, C - 1) (the reference wraps or
    misplaces those).  Integer atomics only: bitwise identical under any permutation of the points; |mean error| <= 2^-33 + 2^-24 |mean|.
    out = the tensor to write into (the call clears it); workspace = an int32 tensor of at least bev_points_workspace_ints(...)
    elements whose storage is 8-byte aligned (default: one cached per shape and device)."""
    _need_cuda(points, point_offsets, out, workspace)
    offs, n, m, dev = _points_offsets("bev_points", points, point_offsets)
    nx, ny, c = _bev_shape(input_shape, None, "bev_points: input_shape")
    rng, org = [float(v) for v in lidar_range], [float(v) for v in origin]
    if len(rng) != 6 or len(org) != 3 or not all(np.isfinite(rng + org)) or not (float(res) > 0.0 and np.isfinite(float(res))):
        raise CobevtHipError("bev_points: lidar_range = [x0, y0, z0, x1, y1, z1], origin = (L1, W1, H1) and res > 0, got %r / %r / %r"
                             % (list(lidar_range), list(origin), res))
    if n * nx * ny * c > 0x7fffffff // 4:
        raise CobevtHipError("bev_points: %d agents of %d x %d x %d cells are more than the operator indexes" % (n, nx, ny, c))
    dims = (ctypes.c_long * 8)(m, n, nx, ny, c, int(bool(range_mask)), int(bool(ego_mask)), int(bool(channels_last)))
    geom = (ctypes.c_double * 10)(*(rng + org + [float(res)]))
    workspace = _workspace("bev_points", "bev_points", dev, WORKSPACE_KEYS["bev_points"](n, nx, ny),
                           bev_points_workspace_ints(m, n, (nx, ny, c)), workspace, align=8)      # (asked for its size on every call)
    bev = _canvas(out, (n, nx, ny, c) if channels_last else (n, c, nx, ny), torch.float32, dev, "bev_points")
    with _timed("bev_points|M%d N%d %dx%dx%d" % (m, n, nx, ny, c), lambda: (0.0, 16.0 * m + 12.0 * m + 4.0 * n * nx * ny * (c + 6))):
        _L.call("cobevt_bev_points", _p(points) if m else None, _p(offs), _p(bev), _p(workspace), dims, geom, _stream())
    return bev


def bev_labels(gt_box_center, mask, origin_xy, res, downsample_rate, label_shape, target_mean=BEV_TARGET_MEAN,
               target_std_dev=BEV_TARGET_STD_DEV, out=None):
    """LidarBevPostprocessor.generate_label for a batch, on the device and without a synchronisation (csrc/bev_labels.hip).
    gt_box_center (B, max_num, 7) in 'lwh' order and mask (B, max_num), contiguous fp32 on the device, max_num <= 128; origin_xy =
    (L1, W1); label_shape = (lx, ly, 7).  -> label_map (B, 7, lx, ly) fp32, bev_corners (B, max_num, 4, 2) fp32 (valid boxes compacted
    to the front in order, zero rows behind them) and num_valid (B,) int32.  Where boxes overlap the last valid one wins; channels
    1 .. 6 of every pixel are normalised; a box with an edge of squared norm <= 1e-6 marks no pixel - see cobevt_hip.h.  One launch;
    it needs no workspace.  out = the three tensors to write into."""
    lx, ly, _ = _bev_shape(label_shape, 7, "bev_labels: label_shape")
    if gt_box_center.dim() != 3 or gt_box_center.shape[2] != 7:
        raise CobevtHipError("bev_labels: gt_box_center must be (B, max_num, 7), got %s" % (tuple(gt_box_center.shape),))
    b, g = gt_box_center.shape[:2]
    if g > DETECT_MAX_GT:
        raise CobevtHipError("bev_labels: at most %d ground-truth slots per sample are supported, got %d" % (DETECT_MAX_GT, g))
    if b < 1 or b > 65535 or b * lx * ly > 0x7fffffff // 8:
        raise CobevtHipError("bev_labels: %d samples of %d x %d pixels are outside what the operator indexes" % (b, lx, ly))
    _require_f32(gt_box_center, "bev_labels: gt_box_center")
    _require_f32(mask, "bev_labels: mask", (b, g))
    params = _bev_params(origin_xy, res, downsample_rate, target_mean, target_std_dev, "bev_labels")
    dev = gt_box_center.device
    shapes = [((b, 7, lx, ly), torch.float32), ((b, g, 4, 2), torch.float32), ((b,), torch.int32)]
    if out is None:
        out = [None] * 3
    elif len(out) != 3:
        raise CobevtHipError("bev_labels: out= is (label_map, bev_corners, num_valid)")
    _need_cuda(*out)
    label_map, corners, num_valid = [_canvas(o, s, d, dev, "bev_labels") for o, (s, d) in zip(out, shapes)]
    gp = (lambda t: _p(t) if g else None)
    with _timed("bev_labels|B%d G%d %dx%d" % (b, g, lx, ly), lambda: (0.0, 28.0 * b * lx * ly + 60.0 * b * g)):
        _L.call("cobevt_bev_labels", gp(gt_box_center), gp(mask), _p(label_map), gp(corners), _p(num_valid), _ints([b, g, lx, ly]), params,
                _stream())
    return label_map, corners, num_valid


def _bev_post_out(out, dev):
    shapes = [((DETECT_TOP, 4, 2), torch.float32), ((DETECT_TOP,), torch.float32), ((DETECT_TOP,), torch.int32), ((1,), torch.int32)]
    if out is None:
        out = [None] * 4
    elif len(out) != 4:
        raise CobevtHipError("bev_post_process: out= is (boxes, scores, index, count)")
    return [_canvas(o, sh, d, dev, "bev_post_process") for o, (sh, d) in zip(out, shapes)]


def bev_post_process(cavs, origin_xy, res, downsample_rate, score_threshold, nms_thresh, target_mean=BEV_TARGET_MEAN,
                     target_std_dev=BEV_TARGET_STD_DEV, out=None, workspace=None):
    """LidarBevPostprocessor.post_process on the device, without a synchronisation (the bev mode of csrc/detect_post.hip).
    cavs: a sequence of 1 .. 16 (cls, reg, transformation_matrix): cls (1, 1, lx, ly) and reg (1, 6, lx, ly) contiguous fp32 on the
    device, the 4 x 4 matrix a tensor or array (converted to fp32 on the device; give device tensors to capture the call in a graph).
    -> boxes (1000, 4, 2) fp32, scores (1000) fp32, index (1000) int32 (global pixel index: cav 0's pixels in (i, j) order, then cav
    1's, ...), count (1) int32, in pick order; rows at and past count are zero.  Candidates are the pixels with sigmoid(cls) >
    score_threshold and finite decoded values; the 1000 best of all cavs, rotated NMS (iou > nms_thresh), then the GT_RANGE mask on
    the four corners - see cobevt_hip.h.  out = the four tensors to write into; workspace = an int64 tensor of
    detect_workspace_bytes(total pixels) bytes."""
    cavs = list(cavs)
    if not 1 <= len(cavs) <= DETECT_MAX_CAV:
        raise CobevtHipError("bev_post_process: 1 .. %d cavs are supported, got %d" % (DETECT_MAX_CAV, len(cavs)))
    params = _bev_params(origin_xy, res, downsample_rate, target_mean, target_std_dev, "bev_post_process")
    keep, dims, mats, total = [], [], [], 0
    dev = None
    for c, cav in enumerate(cavs):
        if len(cav) != 3:
            raise CobevtHipError("bev_post_process: cav %d must be (cls, reg, transformation_matrix)" % c)
        cls, reg, mat = cav
        _need_cuda(cls, reg)
        dev = cls.device if dev is None else dev
        if cls.device != dev or reg.device != dev:
            raise CobevtHipError("bev_post_process: cav %d is on another device" % c)
        if reg.dtype != torch.float32 or reg.dim() != 4 or reg.shape[0] != 1 or reg.shape[1] != 6 or not reg.is_contiguous() \
                or reg.shape[2] < 1 or reg.shape[3] < 1:
            raise CobevtHipError("bev_post_process: reg of cav %d must be contiguous fp32 (1, 6, lx, ly), got %s %s"
                                 % (c, reg.dtype, tuple(reg.shape)))
        lx, ly = reg.shape[2:]
        if cls.dtype != torch.float32 or tuple(cls.shape) != (1, 1, lx, ly) or not cls.is_contiguous():
            raise CobevtHipError("bev_post_process: cls of cav %d must be contiguous fp32 %s, got %s %s"
                                 % (c, (1, 1, lx, ly), cls.dtype, tuple(cls.shape)))
        mats.append(_to_f32(mat, dev, "bev_post_process: transformation_matrix of cav %d" % c, (4, 4)))
        keep.append((cls, reg))
        dims += [lx, ly]
        total += lx * ly
    if total > 0x7fffffff // 8:
        raise CobevtHipError("bev_post_process: %d pixels are more than the operator indexes" % total)
    matrices = mats[0].reshape(1, 4, 4) if len(mats) == 1 else torch.stack(mats)
    ws = _detect_workspace(workspace, total, dev, "bev_post_process")
    ob, osc, oi, oc = _bev_post_out(out, dev)
    ptrs = [(ctypes.c_void_p * len(cavs))(*[k[j].data_ptr() for k in keep]) for j in range(2)]
    cost = lambda: (0.0, 36.0 * total + 8.0 * DETECT_TOP * 16 + 100.0 * DETECT_TOP)         # noqa: E731
    with _timed("bev_post|cavs%d N%d" % (len(cavs), total), cost):
        _L.call("cobevt_bev_post", ptrs[0], ptrs[1], _p(matrices), _ints(dims), len(cavs), params, float(score_threshold),
                float(nms_thresh), _p(ob), _p(osc), _p(oi), _p(oc), _p(ws), _stream())
    return ob, osc, oi, oc


def _require_f32(t, what, shape=None, dims=None, nonempty=False):
    """a contiguous fp32 device tensor as it stands, or an error: nothing is converted (_to_f32 is the form that converts).  shape:
    the sizes, a name standing for any size - ("rows", 16); dims: the rank alone"""
    _need_cuda(t)
    ok = t is not None and t.dtype == torch.float32 and t.is_contiguous() and (dims is None or t.dim() == dims) \
        and (shape is None or t.dim() == len(shape)) and not (nonempty and min(t.shape) < 1)
    if ok and shape is not None:
        for want, got in zip(shape, t.shape):       # (a plain loop: this runs some eight times per layer of a training step)
            if want != got and not isinstance(want, str):
                ok = False
    if not ok:
        raise CobevtHipError("%s must be contiguous%s fp32%s, got %s"
                             % (what, " non-empty" if nonempty else "", "" if shape is None else " (%s)" % ", ".join(str(v) for v in shape),
                                None if t is None else "%s %s" % (t.dtype, tuple(t.shape))))
    return t


def boxes_standup(boxes):
    """boxes (n, 7) contiguous fp32 on the device, 'hwl' order -> (n, 4) fp32 [x1, y1, x2, y2]: the axis-aligned hull of the four
    rotated footprint corners, box_utils.boxes_to_corners_3d + corner2d_to_standup_box (length = column 5, width = column 4), every
    product and sum a separately rounded fp32 operation (csrc/detect_targets.hip)."""
    if boxes.dim() != 2 or boxes.shape[1] != 7:
        raise CobevtHipError("boxes_standup: boxes must be (n, 7), got %s" % (tuple(boxes.shape),))
    _require_f32(boxes, "boxes_standup: boxes")
    out = torch.empty((boxes.shape[0], 4), device=boxes.device, dtype=torch.float32)
    _L.call("cobevt_boxes_standup", _p(boxes), _p(out), boxes.shape[0], _stream())
    return out


def detect_targets(anchors, anchor_standup, gt_boxes, gt_standup, mask, pos_threshold, neg_threshold):
    """VoxelPostprocessor.generate_label for a batch, on the device and without a synchronisation (csrc/detect_targets.hip).
    anchors (H, W, A, 7) and anchor_standup (H W A, 4); gt_boxes (B, G, 7), gt_standup (B, G, 4), mask (B, G), G <= 128: all
    contiguous fp32 on the device.  A slot is valid when its mask is 1; IoU column k is the k-th valid box and targets come from
    that same box.  -> pos_equal_one (B, H, W, A), neg_equal_one (B, H, W, A), targets (B, H, W, 7A) fp32 and num_pos (B,) int32.
    The IoU is bbox_overlaps' (`+1` convention) on the given standup boxes, bit-identical to the compiled reference's mixed float /
    double arithmetic; the rules are stated in cobevt_hip.h.  Bitwise reproducible."""
    if anchors.dim() != 4 or anchors.shape[3] != 7:
        raise CobevtHipError("detect_targets: anchors must be (H, W, A, 7), got %s" % (tuple(anchors.shape),))
    h, w, a = anchors.shape[:3]
    m = h * w * a
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 7:
        raise CobevtHipError("detect_targets: gt_boxes must be (B, G, 7), got %s" % (tuple(gt_boxes.shape),))
    b, g = gt_boxes.shape[:2]
    if g > DETECT_MAX_GT:
        raise CobevtHipError("detect_targets: at most %d ground-truth slots per sample are supported, got %d" % (DETECT_MAX_GT, g))
    if b < 1 or m < 1 or m * b > 0x7fffffff // 8:
        raise CobevtHipError("detect_targets: %d samples of %d anchors are outside what the operator indexes" % (b, m))
    _require_f32(anchors, "detect_targets: anchors")
    _require_f32(anchor_standup, "detect_targets: anchor_standup", (m, 4))
    _require_f32(gt_boxes, "detect_targets: gt_boxes")
    _require_f32(gt_standup, "detect_targets: gt_standup", (b, g, 4))
    _require_f32(mask, "detect_targets: mask", (b, g))
    dev = anchors.device
    pos = torch.empty((b, h, w, a), device=dev, dtype=torch.float32)
    neg = torch.empty((b, h, w, a), device=dev, dtype=torch.float32)
    targets = torch.empty((b, h, w, 7 * a), device=dev, dtype=torch.float32)
    num_pos = torch.empty((b,), device=dev, dtype=torch.int32)
    ws = torch.empty((b * max(g, 1),), device=dev, dtype=torch.int64)
    gp = (lambda t: _p(t) if g else None)
    with _timed("detect_targets|B%d M%d G%d" % (b, m, g), lambda: (0.0, 16.0 * m * (2 + 9 * b))):
        _L.call("cobevt_detect_targets", _p(anchors), _p(anchor_standup), gp(gt_boxes), gp(gt_standup), gp(mask), float(pos_threshold),
                float(neg_threshold), _p(pos), _p(neg), _p(targets), _p(num_pos), _p(ws), b, h, w, a, g, _stream())
    return pos, neg, targets, num_pos


def pointpillar_loss(psm, rm, pos_equal_one, targets, cls_weight, reg, num_pos=None, want_grad=False):
    """The PointPillar detection loss (upstream OpenCOOD's PointPillarLoss) and, with want_grad, its gradient, in one operator call
    (csrc/detect_targets.hip).  psm (B, A, H, W), rm (B, 7A, H, W) NCHW, pos_equal_one (B, H, W, A), targets (B, H, W, 7A): contiguous
    fp32 on the device; num_pos (B,) int32 from detect_targets, or None to have the positives counted.
    -> (loss (3,) fp32 = [total, conf_loss, reg_loss], d total / d psm or None, d total / d rm or None).  fp32 per element, fp64 sums
    in a fixed order: bitwise reproducible, and the same bits with num_pos given or counted."""
    _require_f32(psm, "pointpillar_loss: psm", dims=4)
    b, a, h, w = psm.shape
    if b < 1 or a < 1 or h < 1 or w < 1 or b * a * h * w > 0x7fffffff // 8:
        raise CobevtHipError("pointpillar_loss: psm %s is outside what the operator indexes" % (tuple(psm.shape),))
    _require_f32(rm, "pointpillar_loss: rm", (b, 7 * a, h, w))
    _require_f32(pos_equal_one, "pointpillar_loss: pos_equal_one", (b, h, w, a))
    _require_f32(targets, "pointpillar_loss: targets", (b, h, w, 7 * a))
    if num_pos is not None:
        _need_cuda(num_pos)
        if num_pos.dtype != torch.int32 or tuple(num_pos.shape) != (b,) or not num_pos.is_contiguous():
            raise CobevtHipError("pointpillar_loss: num_pos must be contiguous int32 (%d,), got %s %s" % (b, num_pos.dtype, tuple(num_pos.shape)))
    dev = psm.device
    loss = torch.empty((3,), device=dev, dtype=torch.float32)
    dpsm = torch.empty_like(psm) if want_grad else None
    drm = torch.empty_like(rm) if want_grad else None
    nblk = ((h * w + 255) // 256) * a * b
    ws = torch.empty((2 * nblk + (b + 1) // 2,), device=dev, dtype=torch.int64)
    with _timed("pointpillar_loss|B%d A%d HW%d" % (b, a, h * w), lambda: (0.0, 4.0 * b * a * h * w * (16 + (8 if want_grad else 0)))):
        _L.call("cobevt_pointpillar_loss", _p(psm), _p(rm), _p(pos_equal_one), _p(targets), _p(num_pos), _p(loss), _p(dpsm), _p(drm),
                _p(ws), b, h, w, a, float(cls_weight), float(reg), _stream())
    return loss, dpsm, drm


def sttf_warp(x, tmat, cav_mask, discrete_ratio, downsample_rate, want_mask=True, record_len=None, max_cav=None):
    """x: (B, L, H, W, C) contiguous ; tmat (B, L, 4, 4) fp32 -> warped (B,L,H,W,C), com_mask (B,H,W,1,L)|None.
    With record_len (int32 device (B,)) x is the un-grouped agent batch (N, H, W, C): regroup + warp in one launch,
    returning (warped, com_mask, cav_mask (B, max_cav))."""
    _need_cuda(x, tmat, cav_mask, record_len)
    if tmat.dtype != torch.float32 or not tmat.is_contiguous() or not x.is_contiguous():
        raise CobevtHipError("sttf_warp: tmat must be contiguous fp32, x contiguous")
    if record_len is not None:
        if record_len.dtype != torch.int32 or x.dim() != 4:
            raise CobevtHipError("sttf_warp: record_len must be int32 on the device and x (N, H, W, C)")
        b, l = record_len.shape[0], int(max_cav)
        _, h, w, c = x.shape
        out = torch.empty((b, l, h, w, c), device=x.device, dtype=x.dtype)
        cav = torch.empty((b, l), device=x.device, dtype=torch.float32)
    else:
        b, l, h, w, c = x.shape
        out = torch.empty_like(x)
        cav = None
    if tuple(tmat.shape[:2]) != (b, l):
        raise CobevtHipError("sttf_warp: tmat must be (B, L, 4, 4)")
    com = torch.empty((b, h, w, 1, l), device=x.device, dtype=torch.float32) if want_mask else None
    _L.call("cobevt_sttf_warp", _p(x), _p(tmat), _p(cav_mask), _p(out), _p(com), _p(record_len), _p(cav), dcode(x.dtype), b, l, h, w, c,
            ctypes.c_float(discrete_ratio), ctypes.c_float(downsample_rate), _stream())
    return (out, com, cav) if record_len is not None else (out, com)


def pairwise_warp(x, pairwise, record_len, max_cav, discrete_ratio, downsample_rate):
    """x (sum(record_len), H, W, C) un-grouped agent maps; pairwise (B, L, L, 4, 4) fp32; record_len device int32 (B,) ->
    nb (B, L, L, H, W, C): nb[b, i, j] = agent j in agent i's frame; roi (B, L, L, H, W) fp32 (v2v_fuse.py:59-103)."""
    _need_cuda(x, pairwise, record_len)
    if record_len.dtype != torch.int32 or x.dim() != 4 or pairwise.dtype != torch.float32:
        raise CobevtHipError("pairwise_warp: record_len int32 on the device, x (N, H, W, C), pairwise fp32")
    b, l = record_len.shape[0], int(max_cav)
    _, h, w, c = x.shape
    if tuple(pairwise.shape) != (b, l, l, 4, 4):
        raise CobevtHipError("pairwise_warp: pairwise must be (B, max_cav, max_cav, 4, 4)")
    nb = torch.empty((b, l, l, h, w, c), device=x.device, dtype=x.dtype)
    roi = torch.empty((b, l, l, h, w), device=x.device, dtype=torch.float32)
    _L.call("cobevt_pairwise_warp", _p(x), _p(pairwise.contiguous()), _p(record_len), _p(nb), _p(roi), dcode(x.dtype), b, l, h, w, c,
            ctypes.c_float(discrete_ratio), ctypes.c_float(downsample_rate), _stream())
    return nb, roi


def agent_message_reduce(msg, ego, roi, record_len, mode):
    """msg (B, L, L, H, W, C), ego (N, H, W, C), roi (B, L, L, H, W) -> (N, H, W, C): mean ('avg') | max over the valid source agents of
    (msg + ego) * roi  (v2v_fuse.py:108-119)"""
    _need_cuda(msg, ego, roi, record_len)
    b, l, _, h, w, c = msg.shape
    out = torch.zeros_like(ego)
    _L.call("cobevt_agent_message_reduce", _p(msg), _p(ego), _p(roi), _p(record_len), _p(out), dcode(msg.dtype), b, l, h * w, c,
            {"avg": 0, "max": 1}[mode], _stream())
    return out


def gru_zero_state(x):
    """(..., 2C) [update | candidate] pre-activations -> (..., C): sigmoid(update) * tanh(candidate)"""
    _need_cuda(x)
    c = x.shape[-1] // 2
    out = torch.empty(x.shape[:-1] + (c,), device=x.device, dtype=x.dtype)
    _L.call("cobevt_gru_zero_state", _p(x), _p(out), dcode(x.dtype), x.numel() // (2 * c), c, _stream())
    return out


def agent_softmax_sum(score, nb, roi, record_len, n_agents, use_mask=True):
    """score (B*L*L*H*W, lds) (column 0), nb (B, L, L, H, W, C), roi -> (n_agents, H, W, C)  (disconet_fuse.py:141-150)"""
    _need_cuda(score, nb, roi, record_len)
    b, l, _, h, w, c = nb.shape
    out = torch.zeros((n_agents, h, w, c), device=nb.device, dtype=nb.dtype)
    _L.call("cobevt_agent_softmax_sum", _p(score), score.shape[-1], _p(nb), _p(roi), _p(record_len), _p(out), dcode(nb.dtype), b, l, h * w,
            c, int(bool(use_mask)), _stream())
    return out


def att_fuse_group_ok(c):
    """csrc/warp_common.hpp's group_ok: 8 channels per lane, a power-of-two group of at most 64 lanes per pixel"""
    g = c >> 3
    return c % 8 == 0 and 1 <= g <= 64 and (g & (g - 1)) == 0


def att_fuse(x, record_len, out=None):
    """AttFusion (fusion_modules/self_attn.py:36-57) in one cobevt_att_fuse_nhwc launch: x (N, H, W, C) contiguous un-grouped agent maps
    in the compute dtype, record_len (B,) int32 on the device -> (B, H, W, C): per pixel the ego's row of the scaled-dot-product
    attention over its sample's agents.  record_len is read on the device (no host synchronisation); a sample whose record_len is
    <= 0 gets zeros.  out=: a contiguous (B, H, W, C) tensor of x's dtype to write into."""
    if x.dim() != 4 or not x.is_contiguous() or min(x.shape) < 1:
        raise CobevtHipError("att_fuse: x must be a contiguous non-empty (N, H, W, C) tensor, got %s (contiguous=%s)"
                             % (tuple(x.shape), x.is_contiguous()))
    code = dcode(x.dtype)
    n, h, w, c = (int(d) for d in x.shape)
    if not att_fuse_group_ok(c):
        raise CobevtHipError("att_fuse: C=%d must be 8 times a power of two, at most 512 (8 channels per lane, one group of lanes per pixel)" % c)
    if record_len.dtype != torch.int32 or record_len.dim() != 1 or not record_len.is_contiguous() or record_len.shape[0] < 1:
        raise CobevtHipError("att_fuse: record_len must be a contiguous int32 (B,) tensor with B >= 1, got %s %s"
                             % (record_len.dtype, tuple(record_len.shape)))
    b = int(record_len.shape[0])
    if b > 65535:
        raise CobevtHipError("att_fuse: %d samples exceed the grid's 65535" % b)
    if out is None:
        out = torch.empty((b, h, w, c), device=x.device, dtype=x.dtype)
    elif tuple(out.shape) != (b, h, w, c) or out.dtype != x.dtype or not out.is_contiguous():
        raise CobevtHipError("att_fuse: out= must be a contiguous %s tensor of shape %s, got %s %s"
                             % (x.dtype, (b, h, w, c), out.dtype, tuple(out.shape)))
    _need_cuda(x, record_len, out)
    esz = 2 if code == BF16 else 4
    cost = lambda: (2.0 * 2 * n * h * w * c, float(esz * (n + b) * h * w * c))         # noqa: E731
    with _timed("att_fuse|N%d B%d HW=%d C=%d" % (n, b, h * w, c), cost):
        _L.call("cobevt_att_fuse_nhwc", _p(x), _p(record_len), _p(out), code, b, n, h * w, c, ctypes.c_float(1.0 / math.sqrt(c)), _stream())
    return out


def att_fuse_bwd(x, record_len, dout):
    """The backward of att_fuse with respect to x in one cobevt_att_fuse_bwd_nhwc launch (fp32 storage only): x (N, H, W, C) contiguous
    fp32, record_len (B,) int32 on the device, dout (B, H, W, C) contiguous fp32 -> dx (N, H, W, C) fp32.  Nothing of the forward is
    kept: the scores are recomputed per pixel.  Every element of dx is written once; rows of agents outside every sample are 0."""
    if x.dim() != 4 or not x.is_contiguous() or min(x.shape) < 1:
        raise CobevtHipError("att_fuse_bwd: x must be a contiguous non-empty (N, H, W, C) tensor, got %s (contiguous=%s)"
                             % (tuple(x.shape), x.is_contiguous()))
    if x.dtype != torch.float32:
        raise CobevtHipError("att_fuse_bwd: fp32 storage only, got %s" % x.dtype)
    n, h, w, c = (int(d) for d in x.shape)
    if not att_fuse_group_ok(c):
        raise CobevtHipError("att_fuse_bwd: C=%d must be 8 times a power of two, at most 512 (8 channels per lane, one group of lanes per pixel)" % c)
    if record_len.dtype != torch.int32 or record_len.dim() != 1 or not record_len.is_contiguous() or record_len.shape[0] < 1:
        raise CobevtHipError("att_fuse_bwd: record_len must be a contiguous int32 (B,) tensor with B >= 1, got %s %s"
                             % (record_len.dtype, tuple(record_len.shape)))
    b = int(record_len.shape[0])
    if b > 65535:
        raise CobevtHipError("att_fuse_bwd: %d samples exceed the grid's 65535" % b)
    if dout.dtype != torch.float32 or tuple(dout.shape) != (b, h, w, c) or not dout.is_contiguous():
        raise CobevtHipError("att_fuse_bwd: dout must be a contiguous fp32 tensor of shape %s, got %s %s" % ((b, h, w, c), dout.dtype, tuple(dout.shape)))
    _need_cuda(x, record_len, dout)
    dx = torch.empty_like(x)
    cost = lambda: (2.0 * 6 * n * h * w * c, 4.0 * (3 * n + b) * h * w * c)         # noqa: E731
    with _timed("att_fuse_bwd|N%d B%d HW=%d C=%d" % (n, b, h * w, c), cost):
        _L.call("cobevt_att_fuse_bwd_nhwc", _p(x), _p(record_len), _p(dout), _p(dx), b, n, h * w, c, ctypes.c_float(1.0 / math.sqrt(c)), _stream(),
                variant="")
    return dx


# ---------------------------------------------------------------------------------------------- typed agent attention (HGTCavAttention)
HGT_MAX_AGENTS = 8         # cobevt_hgt_attention_nhwc refuses more keys per pixel
HgtFold = namedtuple("HgtFold", "w_in b_in w_out b_out num_types heads")
_HGT_FOLDS = {}            # (ids of the parameter objects, dtype, device) -> (weakrefs, stamps, HgtFold)


def _hgt_source(src):
    """module or state dict -> {key: tensor} with the module's own Parameter objects (state_dict() hands out new objects every call)"""
    if isinstance(src, dict):
        return src
    return dict(src.named_parameters())


def _hgt_fold64(sd, ln):
    """the float64 fold: per row type b the rows [Wq_b | R_att[a T + b] Wk_b, a = 0 .. T - 1 | R_msg[a T + b]^T Wv_b, a = 0 .. T - 1] and the
    same for the biases, the LayerNorm affine folded last (W' = W g, b' = b + W beta)"""
    num_types = len([k for k in sd if k.startswith("q_linears.") and k.endswith(".weight")])
    ratt, rmsg = sd["relation_att"].detach().double(), sd["relation_msg"].detach().double()
    if num_types < 1 or ratt.dim() != 4 or ratt.shape != rmsg.shape or ratt.shape[2] != ratt.shape[3]:
        raise CobevtHipError("hgt_fold: not an HGTCavAttention state (q_linears.*, relation_att / relation_msg (R, heads, d, d))")
    if ratt.shape[0] < num_types * num_types:
        raise CobevtHipError("hgt_fold: %d relations cannot serve %d x %d type pairs (index a T + b)" % (ratt.shape[0], num_types, num_types))
    heads, dh = int(ratt.shape[1]), int(ratt.shape[2])
    w_in, b_in, w_out, b_out = [], [], [], []
    for b in range(num_types):
        w = {n: sd["%s_linears.%d.weight" % (n, b)].detach().double() for n in "qkva"}
        bs = {n: sd["%s_linears.%d.bias" % (n, b)].detach().double() for n in "qkva"}
        dim = w["q"].shape[1]
        rows_w, rows_b = [w["q"]], [bs["q"]]
        for name, rel, transpose in (("k", ratt, False), ("v", rmsg, True)):
            for a in range(num_types):
                r = rel[a * num_types + b]                                   # (heads, d, d)
                r = r.transpose(1, 2) if transpose else r
                rows_w.append(torch.einsum("mpq,mqc->mpc", r, w[name].reshape(heads, dh, dim)).reshape(heads * dh, dim))
                rows_b.append(torch.einsum("mpq,mq->mp", r, bs[name].reshape(heads, dh)).reshape(heads * dh))
        wt, bt = torch.cat(rows_w, 0), torch.cat(rows_b, 0)
        if ln is not None:
            g, be = ln.weight.detach().double().to(wt.device), ln.bias.detach().double().to(wt.device)
            bt = bt + wt @ be
            wt = wt * g[None, :]
        w_in.append(wt)
        b_in.append(bt)
        w_out.append(w["a"])
        b_out.append(bs["a"])
    return torch.stack(w_in), torch.stack(b_in), torch.stack(w_out), torch.stack(b_out), num_types, heads


def hgt_fold(module_or_state, ln=None, dtype=torch.float32, device=None):
    """HGTCavAttention's parameters (the module, or a state dict of its 2 + 8 T tensors) -> HgtFold: w_in (T, (1 + 2 T) inner, dim) and
    b_in (T, (1 + 2 T) inner), selected by a ROW's own type b: the query projection, then for every query type a the key projection
    with relation_att[a T + b] folded in and the value projection with relation_msg[a T + b]^T folded in (block-diagonal over the
    heads); ln = the LayerNorm in front, whose affine is folded too.  w_out (T, dim, inner), b_out (T, dim): the a_linears.  Folded in
    float64 on the tensors' own device (CPU tensors work: pure torch), rounded once: weights to `dtype`, biases to fp32.  Cached per
    parameter OBJECTS on their version counters and addresses; never filled inside a stream capture (there the fold is part of the graph)."""
    sd = _hgt_source(module_or_state)
    keys = sorted(k for k in sd if k.startswith(("q_linears.", "k_linears.", "v_linears.", "a_linears.")) or k in ("relation_att", "relation_msg"))
    if "relation_att" not in sd or "relation_msg" not in sd:
        raise CobevtHipError("hgt_fold: relation_att / relation_msg are missing")
    tensors = [sd[k] for k in keys] + ([ln.weight, ln.bias] if ln is not None else [])
    dev = torch.device(device) if device is not None else tensors[0].device
    capturing = tensors[0].is_cuda and torch.cuda.is_current_stream_capturing()
    key = (tuple(id(t) for t in tensors), dtype, str(dev), None if ln is None else float(ln.eps))
    stamp = tuple((t._version, t.data_ptr()) for t in tensors)
    ent = _HGT_FOLDS.get(key)
    if not capturing and ent is not None and ent[1] == stamp and all(r() is t for r, t in zip(ent[0], tensors)):
        return ent[2]
    w_in, b_in, w_out, b_out, num_types, heads = _hgt_fold64(sd, ln)
    fold = HgtFold(w_in.to(torch.float32).to(dtype).to(dev).contiguous(), b_in.to(torch.float32).to(dev).contiguous(),
                   w_out.to(torch.float32).to(dtype).to(dev).contiguous(), b_out.to(torch.float32).to(dev).contiguous(), num_types, heads)
    if not capturing:
        _HGT_FOLDS[key] = ([weakref.ref(t, lambda _, k=key: _HGT_FOLDS.pop(k, None)) for t in tensors], stamp, fold)
    return fold


def typed_linear(x, w, bias, types, rows, residual=None, ln_eps=None, out=None):
    """y[row] = W[t] n(x[row]) + bias[t] (+ residual[row]) in one cobevt_typed_linear launch: x (..., K) contiguous in the compute dtype,
    its rows in G = types.numel() groups of `rows` consecutive rows; t = types[g] clamped to 0 .. T - 1 ON THE DEVICE (int32, no host
    read); w (T, N, K) in x's dtype, bias (T, N) fp32; n = the LayerNorm normalisation with ln_eps (affine folded into w / bias) or the
    identity (ln_eps None).  -> (..., N).  K, N multiples of 32; K <= 512 with ln_eps, <= 1024 without."""
    code = dcode(x.dtype)
    if x.dim() < 2 or not x.is_contiguous() or x.numel() == 0:
        raise CobevtHipError("typed_linear: x must be a contiguous non-empty (..., K) tensor, got %s (contiguous=%s)" % (tuple(x.shape), x.is_contiguous()))
    if w.dim() != 3 or w.dtype != x.dtype or not w.is_contiguous() or w.shape[2] != x.shape[-1]:
        raise CobevtHipError("typed_linear: w must be a contiguous %s (T, N, K=%d) tensor, got %s %s" % (x.dtype, x.shape[-1], w.dtype, tuple(w.shape)))
    t, n, k = (int(d) for d in w.shape)
    if k % 32 or n % 32:
        raise CobevtHipError("typed_linear: K=%d and N=%d must be multiples of 32 (one MFMA tile)" % (k, n))
    if k > (512 if ln_eps is not None else 1024):
        raise CobevtHipError("typed_linear: K=%d exceeds the row tile the kernel keeps in LDS (512 with LayerNorm, 1024 without)" % k)
    if bias.dtype != torch.float32 or tuple(bias.shape) != (t, n) or not bias.is_contiguous():
        raise CobevtHipError("typed_linear: bias must be a contiguous fp32 (%d, %d) tensor, got %s %s" % (t, n, bias.dtype, tuple(bias.shape)))
    if types.dtype != torch.int32 or not types.is_contiguous() or types.numel() < 1:
        raise CobevtHipError("typed_linear: types must be a contiguous non-empty int32 tensor, got %s %s" % (types.dtype, tuple(types.shape)))
    g, rows = int(types.numel()), int(rows)
    m = x.numel() // k
    if rows < 1 or g * rows != m:
        raise CobevtHipError("typed_linear: %d rows are not %d groups of %d rows" % (m, g, rows))
    if g > 65535:
        raise CobevtHipError("typed_linear: %d groups exceed the grid's 65535" % g)
    oshape = tuple(x.shape[:-1]) + (n,)
    for name, tns in (("residual", residual), ("out", out)):
        if tns is not None and (tuple(tns.shape) != oshape or tns.dtype != x.dtype or not tns.is_contiguous()):
            raise CobevtHipError("typed_linear: %s must be a contiguous %s tensor of shape %s, got %s %s" % (name, x.dtype, oshape, tns.dtype, tuple(tns.shape)))
    if ln_eps is not None and not float(ln_eps) >= 0.0:
        raise CobevtHipError("typed_linear: ln_eps=%r must be >= 0" % (ln_eps,))
    _need_cuda(x, w, bias, types, residual, out)
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=x.dtype)
    esz = 2 if code == BF16 else 4
    dims = (ctypes.c_long * 7)(code, g, rows, k, n, t, int(ln_eps is not None))
    cost = lambda: (2.0 * m * n * k, float(esz * (m * k + t * n * k + m * n * (2 if residual is not None else 1))))         # noqa: E731
    with _timed("typed_linear|G%d R=%d K=%d N=%d T=%d" % (g, rows, k, n, t), cost):
        _L.call("cobevt_typed_linear", _p(x), _p(w), _p(bias), _p(types), _p(residual), _p(out), dims, ctypes.c_float(ln_eps or 0.0), _stream())
    return out


def hgt_attention(proj, types, heads, num_types, mask=None, out=None):
    """The per-pixel typed agent attention in one cobevt_hgt_attention_nhwc launch: proj (B, L, H, W, (1 + 2 T) inner) contiguous in the
    compute dtype with rows [q | k'_0 .. k'_(T-1) | v'_0 .. v'_(T-1)] (typed_linear on hgt_fold's w_in), inner = 32 heads; types
    (B, L) int32 on the device (clamped to 0 .. T - 1 there); mask (B, H, W, L) contiguous fp32, 0 = key masked, or None
    -> (B, L, H, W, inner).  A query whose keys are all masked gets zeros."""
    code = dcode(proj.dtype)
    heads, num_types = int(heads), int(num_types)
    if proj.dim() != 5 or not proj.is_contiguous() or proj.numel() == 0:
        raise CobevtHipError("hgt_attention: proj must be a contiguous non-empty (B, L, H, W, C) tensor, got %s (contiguous=%s)"
                             % (tuple(proj.shape), proj.is_contiguous()))
    b, l, h, w, c = (int(d) for d in proj.shape)
    inner = 32 * heads
    if heads < 1 or num_types < 1 or c != (1 + 2 * num_types) * inner:
        raise CobevtHipError("hgt_attention: C=%d is not (1 + 2 T) * 32 heads for T=%d, heads=%d (dim_head = 32)" % (c, num_types, heads))
    if l > HGT_MAX_AGENTS:
        raise CobevtHipError("hgt_attention: %d agents exceed the kernel's %d" % (l, HGT_MAX_AGENTS))
    if heads > 64 or num_types > 64:
        raise CobevtHipError("hgt_attention: heads=%d / T=%d exceed the kernel's 64" % (heads, num_types))
    if b * l > 65535:
        raise CobevtHipError("hgt_attention: %d agent maps exceed the grid's 65535" % (b * l))
    if types.dtype != torch.int32 or not types.is_contiguous() or types.numel() != b * l:
        raise CobevtHipError("hgt_attention: types must be a contiguous int32 tensor of %d elements, got %s %s" % (b * l, types.dtype, tuple(types.shape)))
    if mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != (b, h, w, l) or not mask.is_contiguous()):
        raise CobevtHipError("hgt_attention: mask must be a contiguous fp32 tensor of shape %s, got %s %s" % ((b, h, w, l), mask.dtype, tuple(mask.shape)))
    oshape = (b, l, h, w, inner)
    if out is not None and (tuple(out.shape) != oshape or out.dtype != proj.dtype or not out.is_contiguous()):
        raise CobevtHipError("hgt_attention: out= must be a contiguous %s tensor of shape %s, got %s %s" % (proj.dtype, oshape, out.dtype, tuple(out.shape)))
    _need_cuda(proj, types, mask, out)
    if out is None:
        out = torch.empty(oshape, device=proj.device, dtype=proj.dtype)
    esz = 2 if code == BF16 else 4
    px = b * h * w
    cost = lambda: (4.0 * px * l * l * inner, float(esz * px * l * (inner + 2 * l * inner + inner)))         # noqa: E731
    with _timed("hgt_attention|B%d L%d HW=%d heads=%d T=%d" % (b, l, h * w, heads, num_types), cost):
        _L.call("cobevt_hgt_attention_nhwc", _p(proj), _p(types), _p(mask), _p(out), code, b, l, h * w, heads, num_types,
                ctypes.c_float(32 ** -0.5), _stream())
    return out


# ---------------------------------------------------------------------------------------------- training of the transposed convolution
# fp32 only, the native library (exact fp32 products).  Scratch buffers are cached per size like the sparse path's.
def _deconv_geometry(cin, cout, s, what):
    if not 1 <= s <= DECONV_MAX_STRIDE:
        raise CobevtHipError("%s: stride %d is outside 1 .. %d" % (what, s, DECONV_MAX_STRIDE))
    if cin < 4 or cin % 4 != 0:
        raise CobevtHipError("%s: Cin=%d must be a multiple of 4 for the fp32 kernels" % (what, cin))
    if cout < 32 or cout % 32 != 0:
        raise CobevtHipError("%s: Cout=%d must be a multiple of 32 (one MFMA tile = 32 channels of one tap)" % (what, cout))


def deconv_train_weights(weight):
    """The fp32 master weight (Cin, Cout, s, s) of an nn.ConvTranspose2d(kernel = stride = s, bias=False) -> the two UNfolded operand
    tables of its training kernels: forward [s s Cout][Kpad] with row (dy s + dx) Cout + co = weight[:, co, dy, dx] (DeconvPlan's
    layout without a BatchNorm) and input-gradient rows [Cin][Kpad'] with k = (dy s + dx) Cout + co (the implicit-GEMM rows of the
    weight read as (out = Cin, in = Cout, s, s)); both padded with zero columns to a multiple of 16.  Device permutes - no host round
    trip per optimiser step, unlike DeconvPlan - cached per weight object (_lowered_tables: hand over the nn.Parameter itself)."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.dtype != torch.float32:
        raise CobevtHipError("deconv_train_weights: weight must be fp32 (Cin, Cout, s, s), got %s %s" % (weight.dtype, tuple(weight.shape)))
    cin, cout, s, _ = (int(d) for d in weight.shape)
    _deconv_geometry(cin, cout, s, "deconv_train_weights")
    kf, kd = (cin + 15) // 16 * 16, (s * s * cout + 15) // 16 * 16

    def lower(w):
        fwd = torch.zeros((s * s * cout, kf), device=w.device, dtype=torch.float32)
        fwd[:, :cin] = w.permute(2, 3, 1, 0).reshape(s * s * cout, cin)
        rows = torch.zeros((cin, kd), device=w.device, dtype=torch.float32)
        rows[:, :s * s * cout] = w.permute(0, 2, 3, 1).reshape(cin, s * s * cout)
        return fwd, rows

    return _lowered_tables("deconv", weight, lower)


def deconv_raw(x, wgt, cout, s):
    """z = ConvTranspose2d(kernel = stride = s)(x) without BatchNorm or activation: x (N, H, W, Cin) contiguous fp32, wgt the forward
    table of deconv_train_weights -> z (N, sH, sW, Cout) fp32.  One cobevt_deconv_nhwc launch of the native library (exact fp32) with a
    zero shift, act = 0, c_off = 0."""
    _require_f32(x, "deconv_raw: x", ("N", "H", "W", "C"), nonempty=True)
    n, h, w, cin = (int(d) for d in x.shape)
    cout, s = int(cout), int(s)
    _deconv_geometry(cin, cout, s, "deconv_raw")
    if wgt.dtype != torch.float32 or wgt.dim() != 2 or not wgt.is_contiguous() or wgt.shape[0] != s * s * cout or wgt.shape[1] < cin \
            or wgt.shape[1] % 16:
        raise CobevtHipError("deconv_raw: the weight table must be contiguous fp32 (%d, Kpad >= %d in 16s), got %s %s"
                             % (s * s * cout, cin, wgt.dtype, tuple(wgt.shape)))
    if n * h * w * s * s >= 2 ** 31 - 1:
        raise CobevtHipError("deconv_raw: %d destination pixels overflow the kernel's 32-bit pixel index" % (n * h * w * s * s))
    _need_cuda(x, wgt)
    z = torch.empty((n, s * h, s * w, cout), device=x.device, dtype=torch.float32)
    shift = _zero_shift(x.device, cout)
    dims = _ints([FP32, n, h, w, cin, cout, wgt.shape[1], s, 0, cout, 0])
    m = n * h * w
    with _timed("deconv_raw|s%d %d->%d M=%d" % (s, cin, cout, m), lambda: (2.0 * m * s * s * cout * cin, 4.0 * (m * cin + wgt.numel() + m * s * s * cout))):
        _L.call("cobevt_deconv_nhwc", _p(x), _p(wgt), _p(shift), _p(z), dims, _stream(), variant="")
    return z


_ZERO_SHIFT = {}


def _zero_shift(dev, c):
    """fp32 zeros (c,), never written: the shift operand of the raw transposed convolution"""
    key = (dev, c)
    if key in _ZERO_SHIFT:
        return _ZERO_SHIFT[key]
    z = torch.zeros(c, device=dev, dtype=torch.float32)
    if not (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):       # a capture's allocations belong to its graph
        _ZERO_SHIFT[key] = z
    return z


def deconv_wgrad_chunks(n, h, w, cin, cout, s):
    """cobevt_deconv_wgrad_chunks: the pixel chunks of deconv_wgrad, a pure function of the shape (no device)"""
    rc = _L.load("").cobevt_deconv_wgrad_chunks(_ints([n, h, w, cin, cout, s]))
    if rc < 0:
        raise CobevtHipError("deconv_wgrad: shape N=%d H=%d W=%d Cin=%d Cout=%d s=%d is not served (error %d)" % (n, h, w, cin, cout, s, -rc))
    return int(rc)


def deconv_wgrad(x, dz, s):
    """The weight gradient of deconv_raw (cobevt_deconv_wgrad, two launches): x (N, H, W, Cin), dz (N, sH, sW, Cout) contiguous fp32 ->
    dW (Cin, Cout, s, s) fp32, the ConvTranspose2d layout, written.  No floating-point atomics: pixel chunks added in order in fp64."""
    _require_f32(x, "deconv_wgrad: x", ("N", "H", "W", "C"), nonempty=True)
    n, h, w, cin = (int(d) for d in x.shape)
    s = int(s)
    if dz is None or dz.dim() != 4:
        raise CobevtHipError("deconv_wgrad: dz must be a 4-D tensor")
    cout = int(dz.shape[3])
    _deconv_geometry(cin, cout, s, "deconv_wgrad")
    _require_f32(dz, "deconv_wgrad: dz", (n, s * h, s * w, cout), nonempty=True)
    if n * h * w * s * s >= 2 ** 31 - 1:
        raise CobevtHipError("deconv_wgrad: %d pixels of dz overflow the kernel's 32-bit pixel index" % (n * h * w * s * s))
    _need_cuda(x, dz)
    chunks = deconv_wgrad_chunks(n, h, w, cin, cout, s)
    floats = chunks * s * s * ((cin + 31) // 32 * 32) * cout
    partial = _sparse_train_ws(x.device, torch.float32, floats)
    dw = torch.empty((cin, cout, s, s), device=x.device, dtype=torch.float32)
    m = n * h * w
    with _timed("deconv_wgrad|s%d %d->%d M=%d" % (s, cin, cout, m), lambda: (2.0 * m * s * s * cout * cin, 4.0 * (m * s * s * (cin + cout) + 2 * floats))):
        _L.call("cobevt_deconv_wgrad", _p(x), _p(dz), _p(partial), _p(dw), _ints([n, h, w, cin, cout, s, chunks]), _stream(), variant="")
    return dw


def invert_small(m):
    """Batched inverse of (..., 3, 3) or (..., 4, 4) fp32 matrices on the device."""
    _need_cuda(m)
    d = m.shape[-1]
    x = m.to(torch.float32).contiguous()
    out = torch.empty_like(x)
    _L.call("cobevt_invert_small", _p(x), _p(out), x.numel() // (d * d), d, _stream())
    return out


def resize_nhwc(x, ho, wo, mode):
    """(N,H,W,C) -> (N,ho,wo,C); mode 'nearest' (F.interpolate default) or 'bilinear' (align_corners=True)."""
    _need_cuda(x)
    n, h, w, c = x.shape
    out = torch.empty((n, ho, wo, c), device=x.device, dtype=x.dtype)
    _L.call("cobevt_resize_nhwc", _p(x), _p(out), dcode(x.dtype), n, h, w, c, ho, wo, 0 if mode == "nearest" else 1, _stream())
    return out


def channel_affine(x, scale, shift):
    """x (N, C, ...) contiguous fp32 -> x * scale[c] + shift[c]"""
    _need_cuda(x, scale, shift)
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    out = torch.empty_like(x)
    n, c = x.shape[0], x.shape[1]
    _L.call("cobevt_channel_affine", _p(x), _p(scale), _p(shift), _p(out), n, c, x.numel() // (n * c), _stream())
    return out


def chain_next_fusable(plan_n, c):
    """Can `plan_n` (a Linear / 1x1 conv plan reading C-channel rows) ride at the end of the fused row chain?"""
    return (plan_n is not None and plan_n.wfrag_rows is not None and plan_n.stride == 1 and plan_n.kp_rows == 128 and plan_n.K == c
            and plan_n.cout % 8 == 0 and plan_n.cout <= 768 and plan_n.pre_scale is None and not plan_n.pre_relu
            and plan_n.act <= 2)


def attn_mlp_chain(a, skip, plan_p, plan_1, plan_2, post_ln=None, next_plan=None):
    """out = postLN( y + fc2(GELU(fc1(LN(y)))) ),  y = proj(a) + skip.   a, skip: (..., C) contiguous.
    plan_1 must be built with ln=<prenorm> (affine folded) and act=GELU; post_ln = (gamma, beta, eps) fp32 or None.
    One fused launch in bf16 mode when the shapes fit (C <= 128, hidden <= 256); otherwise three GEMM launches.
    next_plan: the Linear / 1x1-conv plan that consumes `out` next (LayerNorm folded via ln=..., BN folded, act); when
    given the call returns (out, next_plan(out)) - computed inside the same launch when fused."""
    _need_cuda(a, skip)
    c, hd = plan_p.cout, plan_1.cout
    skip_rows = 0
    if skip is not None and batch_broadcast(skip) and skip.shape == a.shape:
        skip_rows = skip[0].numel() // c           # one slice shared by the whole batch: the kernel indexes it modulo
    # fp32 storage (round 6, csrc/row_chain_f32.hip): the C = 128 / hidden 256 chain of every FAX level and of the camera fusion stage
    f32 = a.dtype == torch.float32
    fusable = (USE_ROW_CHAIN and (a.dtype == torch.bfloat16 or (f32 and USE_ROW_CHAIN_F32 and c == 128 and hd == 256 and plan_2.kp_rows == 256))
               and plan_p.wfrag_rows is not None and plan_1.wfrag_rows is not None
               and plan_2.wfrag_rows is not None and plan_2.kp_rows <= 256 and plan_1.has_ln and plan_1.act == 2 and plan_p.act == 0
               and plan_2.act == 0 and not plan_p.has_ln and not plan_2.has_ln and plan_p.K == c and plan_1.K == c
               and plan_2.K == hd and plan_2.cout == c and c <= 128 and c % 8 == 0 and hd <= 256 and hd % 8 == 0
               and plan_p.kp_rows == 128 and plan_1.kp_rows == 128 and a.shape[-1] == c and a.is_contiguous()
               and (skip is None or skip.dtype == a.dtype)
               and (skip is None or skip_rows or (skip.is_contiguous() and skip.shape == a.shape)))
    if not fusable:
        y = linear(a, plan_p, residual=skip.contiguous() if skip is not None else None)
        z = linear(linear(y, plan_1), plan_2, residual=y)
        z = layernorm(z, post_ln[0], post_ln[1], post_ln[2]) if post_ln is not None else z
        return (z, linear(z, next_plan)) if next_plan is not None else z
    m = a.numel() // c
    out = torch.empty_like(a)
    fuse_next = USE_CHAIN_NEXT and chain_next_fusable(next_plan, c)
    nn_ = next_plan.cout if fuse_next else 0
    out_next = torch.empty(a.shape[:-1] + (nn_,), device=a.device, dtype=a.dtype) if fuse_next else None
    dims = _ints([plan_p.code, m, c, hd, plan_2.kp_rows, nn_, int(next_plan.has_ln) if fuse_next else 0,
                  next_plan.act if fuse_next else 0, ROW_CHAIN_ROWS, skip_rows])
    pg, pb, pe = post_ln if post_ln is not None else (None, None, 0.0)

    def cost():
        flops = 2.0 * m * (c * c + 2 * c * hd + c * nn_)
        esz = a.element_size()
        return flops, float((2 * m + (0 if skip is None else skip_rows or m)) * c * esz + m * nn_ * esz + (c * c + 2 * c * hd + c * nn_) * esz)

    with _timed("row_chain|C%d H%d M=%d%s%s" % (c, hd, m, " post" if post_ln is not None else "",
                                                  " +next%d" % nn_ if fuse_next else ""), cost):
        _L.call("cobevt_attn_mlp_chain", _p(a), _p(skip), _p(out), _p(plan_p.wfrag_rows), _p(plan_p.bias), _p(plan_1.wfrag_rows),
                _p(plan_1.bias), _p(plan_2.wfrag_rows), _p(plan_2.bias), _p(pg), _p(pb), _p(next_plan.wfrag_rows) if fuse_next else None,
                _p(next_plan.bias) if fuse_next else None, _p(out_next), dims, ctypes.c_float(plan_1.ln_eps), ctypes.c_float(pe),
                ctypes.c_float(next_plan.ln_eps if fuse_next else 0.0), _stream())
    if next_plan is None:
        return out
    return out, (out_next if fuse_next else linear(out, next_plan))


def proj_chain_fusable(x, plan_p, next_plan, residual):
    c = x.shape[-1]
    return (USE_PROJ_CHAIN and x.dtype == torch.bfloat16 and c == 128 and x.is_contiguous() and plan_p.wfrag_rows is not None
            and plan_p.kp_rows == 128 and plan_p.K == c and plan_p.cout == c and plan_p.act == 0 and not plan_p.has_ln
            and plan_p.stride == 1 and chain_next_fusable(next_plan, c)
            and (residual is None or (residual.is_contiguous() and residual.shape == x.shape and residual.dtype == x.dtype)))


def proj_chain(x, plan_p, next_plan, residual=None, out_next=None):
    """next_plan(plan_p(x) + residual) on (..., 128) rows in one launch (cobevt_proj_chain); plan_p may carry the pre-activation
    BatchNorm -> ReLU of its input, next_plan a folded LayerNorm.  The intermediate map is not materialised."""
    _need_cuda(x, residual)
    c, nn_ = 128, next_plan.cout
    m = x.numel() // c
    if out_next is None:
        out_next = torch.empty(x.shape[:-1] + (nn_,), device=x.device, dtype=x.dtype)
    elif out_next.numel() != m * nn_ or not out_next.is_contiguous() or out_next.dtype != x.dtype:
        raise CobevtHipError("proj_chain: `out_next` must be a contiguous (.., %d) buffer of dtype %s" % (nn_, x.dtype))
    dims = _ints([0, m, c, nn_, int(next_plan.has_ln), next_plan.act, 0, plan_p.pre_relu, 0 if USE_PROJ_CHAIN_WAVE else 1])

    def cost():
        return 2.0 * m * (c * c + c * nn_), float(m * (c * (2 if residual is not None else 1) + nn_) * 2 + (c * c + c * nn_) * 2)

    with _timed("row_chain|proj C%d M=%d +next%d" % (c, m, nn_), cost):
        _L.call("cobevt_proj_chain", _p(x), _p(plan_p.pre_scale), _p(plan_p.pre_shift), _p(residual), _p(plan_p.wfrag_rows),
                _p(plan_p.bias), None, _p(next_plan.wfrag_rows), _p(next_plan.bias), _p(out_next), dims, ctypes.c_float(next_plan.ln_eps),
                _stream())
    return out_next


def proj_chain_kv_fusable(x, plan_key, plan_val, next_key, next_val, residual):
    k = x.shape[-1]
    if not (USE_PROJ_CHAIN_KV and x.dtype == torch.bfloat16 and x.is_contiguous() and k in (256, 384, 512)):
        return False
    for pl in (plan_key, plan_val):
        if pl is None:
            continue
        if not (pl.wfrag_rows is not None and pl.kp_rows == k and pl.K == k and pl.cout == 128 and pl.act == 0 and not pl.has_ln
                and pl.stride == 1):
            return False
    for pn in (next_key, next_val):
        if not (chain_next_fusable(pn, 128) and pn.act == 0):
            return False
    return (plan_val is not None and next_key.cout == next_val.cout and next_key.has_ln == next_val.has_ln and next_key.ln_eps == next_val.ln_eps
            and (residual is None or (plan_key is not None and residual.is_contiguous() and residual.dtype == x.dtype
                                      and tuple(residual.shape) == tuple(x.shape[:-1]) + (128,))))


def proj_chain_kv(x, plan_key, plan_val, next_key, next_val, residual=None, out_k=None, out_v=None):
    """(next_key(plan_key(x) + residual), next_val(plan_val(x))) on (..., K) feature rows, K = 256 / 384 / 512 -> two (..., Nn) maps, ONE
    launch (cobevt_proj_chain_kv); neither 128-channel intermediate map reaches HBM.  plan_key None (`no_image_features`: the key is
    the ray embedding alone, fax_modules.py:392-396) is not served here."""
    _need_cuda(x, residual)
    k, nn_ = x.shape[-1], next_key.cout
    m = x.numel() // k
    outs = []
    for o in (out_k, out_v):
        if o is None:
            o = torch.empty(x.shape[:-1] + (nn_,), device=x.device, dtype=x.dtype)
        elif o.numel() != m * nn_ or not o.is_contiguous() or o.dtype != x.dtype:
            raise CobevtHipError("proj_chain_kv: result buffers must be contiguous (.., %d) of dtype %s" % (nn_, x.dtype))
        outs.append(o)
    ptrs = (ctypes.c_void_p * 18)()
    for s_, (pp, pn, res, o) in enumerate(((plan_key, next_key, residual, outs[0]), (plan_val, next_val, None, outs[1]))):
        vals = (pp.pre_scale, pp.pre_shift, pp.wfrag_rows, pp.bias, res, pn.wfrag_rows, pn.bias, None, o)
        for j, t in enumerate(vals):
            ptrs[9 * s_ + j] = None if t is None else t.data_ptr()
    dims = _ints([0, m, k, nn_, int(next_key.has_ln), 2, plan_key.pre_relu, 0, plan_val.pre_relu, 0])

    def cost():
        return 2.0 * 2 * m * (k * 128 + 128 * nn_), float(m * (k + (128 if residual is not None else 0) + 2 * nn_) * 2 + 2 * (k * 128 + 128 * nn_) * 2)

    with _timed("row_chain|proj kv K%d M=%d +next%d" % (k, m, nn_), cost):
        _L.call("cobevt_proj_chain_kv", _p(x), ptrs, dims, ctypes.c_float(next_key.ln_eps), _stream())
    return outs[0], outs[1]


def swap_stage_fusable(qkv, x, tmap, heads, plan_p, plan_1, plan_2, next_plan, mask):
    """does one SwapFusionBlock half fit the single-launch kernel (cobevt_swap_fusion_stage)?"""
    c = x.shape[-1]
    nk = tmap[1] * tmap[4] * tmap[5]
    return (USE_SWAP_STAGE and x.dtype == torch.bfloat16 and qkv.dtype == torch.bfloat16 and c == 128 and heads == 4
            and tmap[0] in (0, 1) and nk <= 384 and x.is_contiguous() and qkv.is_contiguous() and qkv.shape[-1] == 3 * c
            and plan_p.wfrag_rows is not None and plan_1.wfrag_rows is not None and plan_2.wfrag_rows is not None
            and plan_p.kp_rows == 128 and plan_1.kp_rows == 128 and plan_2.kp_rows in (128, 256) and plan_1.has_ln
            and plan_1.act == 2 and plan_p.act == 0 and plan_2.act == 0 and not plan_p.has_ln and not plan_2.has_ln
            and plan_p.K == c and plan_1.K == c and plan_2.K == plan_1.cout and plan_2.cout == c and plan_1.cout % 8 == 0
            and plan_1.cout <= 256 and plan_p.cout == c
            and (next_plan is None or (chain_next_fusable(next_plan, c) and next_plan.cout <= 384 and next_plan.has_ln
                                       and next_plan.act == 0))
            and (mask is None or (mask.dtype == torch.float32 and mask.is_contiguous())))


SWAP_STAGE_BIAS_FLOATS = 10240     # the kernel copies the relative-position table as a fixed 40-KB image (csrc/swap_stage.hip)


def swap_stage(qkv, x, tmap, batch, heads, scale, bias_table, bias_L, mask, plan_p, plan_1, plan_2, next_plan=None):
    """One SwapFusionBlock half: x (b, l, h, w, 128) + its qkv = to_qkv(LN(x)) (b, l, h, w, 384) -> x_out (and the next
    half's to_qkv(LN(x_out)) when next_plan is given).  bias_table: the flat SWAP_STAGE_BIAS_FLOATS image of
    swap_fusion_modules.Attention.stage_bias_table().  Caller checks swap_stage_fusable() first."""
    _need_cuda(qkv, x, bias_table, mask)
    c, hd = 128, plan_1.cout
    out = torch.empty_like(x)
    nn_ = next_plan.cout if next_plan is not None else 0
    qkv_next = torch.empty(x.shape[:-1] + (nn_,), device=x.device, dtype=x.dtype) if next_plan is not None else None
    bias_rows = (2 * bias_L - 1) * (2 * tmap[4] - 1) * (2 * tmap[5] - 1)
    if bias_table.numel() != SWAP_STAGE_BIAS_FLOATS or bias_table.dtype != torch.float32 or not bias_table.is_contiguous():
        raise CobevtHipError("swap_stage: bias table must be the flat fp32 image of stage_bias_table()")
    dims = _ints([0, batch, c, heads, hd, plan_2.kp_rows, nn_, bias_rows, bias_L])
    m = x.numel() // c
    nk = tmap[1] * tmap[4] * tmap[5]

    def cost():
        flops = 4.0 * m * nk * c + 2.0 * m * (c * c + 2 * c * hd + c * nn_)
        return flops, float(m * (3 * c + 2 * c + nn_) * 2 + (c * c + 2 * c * hd + c * nn_) * 2)

    with _timed("swap_stage|mode%d M=%d Nk%d H%d%s" % (tmap[0], m, nk, hd, " +next%d" % nn_ if nn_ else ""), cost):
        _L.call("cobevt_swap_fusion_stage", _p(qkv), _p(x), _p(out), _p(qkv_next), _ints(tmap), _p(bias_table), _p(mask),
                _p(plan_p.wfrag_rows), _p(plan_p.bias), _p(plan_1.wfrag_rows), _p(plan_1.bias), _p(plan_2.wfrag_rows), _p(plan_2.bias),
                _p(next_plan.wfrag_rows) if next_plan is not None else None, _p(next_plan.bias) if next_plan is not None else None, dims,
                ctypes.c_float(scale), ctypes.c_float(plan_1.ln_eps), ctypes.c_float(next_plan.ln_eps if next_plan is not None else 0.0),
                _stream())
    return out, qkv_next


# ----------------------------------------------------------------------------------------------
# downstream of the hot path: logits -> probabilities / class maps -> per-class pixel counts
# ----------------------------------------------------------------------------------------------
def softmax_argmax(seg_logits):
    """(N, C, H, W) logits -> (softmax(dim=1) fp32 (N, C, H, W), argmax of the probabilities int64 (N, H, W));
    CameraBevPostprocessor.softmax_argmax, camera_bev_postprocessor.py:55-59."""
    _need_cuda(seg_logits)
    if seg_logits.dim() != 4:
        raise CobevtHipError("softmax_argmax expects (N, C, H, W) logits, got %s" % (tuple(seg_logits.shape),))
    x = seg_logits.contiguous()
    n, c, h, w = x.shape
    prob = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
    seg_map = torch.empty((n, h, w), device=x.device, dtype=torch.int64)
    _L.call("cobevt_softmax_argmax", _p(x), _p(prob), _p(seg_map), dcode(x.dtype), n, c, h * w, _stream())
    return prob, seg_map


def seg_class_counts(pred, gt, num_classes):
    """pred, gt: (N, H, W) integer label maps -> (N, num_classes, 3) int64 counts (n_ii, t_i, n_ij) per class - what
    seg_utils.py:25-50 (mean_IU) and :6-21 (mean_precision) reduce their masks to.  Labels outside [0, num_classes)
    raise (the reference would treat them as further classes)."""
    _need_cuda(pred, gt)
    if pred.shape != gt.shape or pred.dim() != 3:
        raise CobevtHipError("seg_class_counts expects two (N, H, W) maps, got %s and %s" % (tuple(pred.shape), tuple(gt.shape)))
    p64, g64 = pred.to(torch.int64).contiguous(), gt.to(torch.int64).contiguous()
    n, h, w = p64.shape
    counts = torch.empty((n, num_classes + 1, 3), device=pred.device, dtype=torch.int64)
    _L.call("cobevt_seg_class_counts", _p(p64), _p(g64), _p(counts), n, h * w, num_classes, _stream())
    host = counts.cpu()
    if int(host[:, num_classes, 0].sum()) or int(host[:, num_classes, 1].sum()):
        raise CobevtHipError("seg_class_counts: labels outside [0, %d)" % num_classes)
    return host[:, :num_classes]


# ----------------------------------------------------------------------------------------------
# MBConv pieces of the nuScenes EfficientNet backbone
# ----------------------------------------------------------------------------------------------
class DepthwisePlan(object):
    """k x k depthwise conv (groups == channels) + folded BatchNorm + activation, TensorFlow-"same" static padding:
    `pad` = (before, after) zero rows / columns, the kernel takes the before part and bounds-checks the rest."""

    def __init__(self, weight, bn=None, stride=1, pad=(0, 0), act=0, dtype=torch.bfloat16, device="cuda"):
        w = weight.detach().double().cpu()                      # (C, 1, k, k)
        c, one, kh, kw = w.shape
        if one != 1 or kh != kw:
            raise CobevtHipError("DepthwisePlan expects a (C, 1, k, k) weight")
        b = torch.zeros(c, dtype=torch.float64)
        if bn is not None:
            s_, sh = bn_affine(bn)
            w = w * s_.cpu()[:, None, None, None]
            b = sh.cpu().double()
        if c % 8 != 0:
            raise CobevtHipError("depthwise conv needs a multiple of 8 channels, got %d" % c)
        self.c, self.k, self.stride, self.act = c, kh, int(stride), int(act)
        self.pad0, self.pad1 = int(pad[0]), int(pad[1])
        self.dtype, self.code = dtype, dcode(dtype)
        self.wgt = w[:, 0].permute(1, 2, 0).reshape(kh * kw, c).to(torch.float32).to(device).contiguous()     # [tap][C]
        self.bias = b.to(torch.float32).to(device).contiguous()

    def out_hw(self, h, w):
        return ((h + self.pad0 + self.pad1 - self.k) // self.stride + 1, (w + self.pad0 + self.pad1 - self.k) // self.stride + 1)


def depthwise_conv(x, plan):
    """x (N, H, W, C) channels-last in plan.dtype -> (N, Ho, Wo, C)"""
    _need_cuda(x)
    n, h, w, c = x.shape
    if c != plan.c or x.dtype != plan.dtype or not x.is_contiguous():
        raise CobevtHipError("depthwise_conv: bad input %s %s for C=%d %s" % (tuple(x.shape), x.dtype, plan.c, plan.dtype))
    ho, wo = plan.out_hw(h, w)
    out = torch.empty((n, ho, wo, c), device=x.device, dtype=plan.dtype)
    dims = _ints([plan.code, n, h, w, c, plan.k, plan.stride, plan.pad0, plan.pad0, ho, wo, plan.act])

    def cost():
        esz = 2 if plan.code == BF16 else 4
        return 2.0 * n * ho * wo * c * plan.k * plan.k, float((x.numel() + out.numel()) * esz)

    with _timed("depthwise|%dx%d s%d C%d %dx%d" % (plan.k, plan.k, plan.stride, c, h, w), cost):
        _L.call("cobevt_depthwise_conv_nhwc", _p(x), _p(plan.wgt), _p(plan.bias), _p(out), dims, _stream())
    return out


def spatial_mean(x):
    """(N, H, W, C) -> (N, C) fp32 mean over the pixels (the squeeze of squeeze-and-excitation), deterministic order"""
    _need_cuda(x)
    n, h, w, c = x.shape
    if not x.is_contiguous():
        raise CobevtHipError("spatial_mean: input must be contiguous channels-last")
    out = torch.empty((n, c), device=x.device, dtype=torch.float32)
    _L.call("cobevt_spatial_mean_nhwc", _p(x), _p(out), dcode(x.dtype), n, h * w, c, _stream())
    return out


def se_gate(mean, w_reduce, b_reduce, w_expand, b_expand):
    """mean (N, C) fp32; w_reduce (Cs, C), b_reduce (Cs,), w_expand (C, Cs), b_expand (C,) fp32 ->
    sigmoid(w_expand . swish(w_reduce . mean + b_reduce) + b_expand)  (N, C) fp32"""
    _need_cuda(mean, w_reduce, b_reduce, w_expand, b_expand)
    n, c = mean.shape
    cs = w_reduce.shape[0]
    if tuple(w_reduce.shape) != (cs, c) or tuple(w_expand.shape) != (c, cs) or b_reduce.numel() != cs or b_expand.numel() != c:
        raise CobevtHipError("se_gate: inconsistent shapes")
    gate = torch.empty((n, c), device=mean.device, dtype=torch.float32)
    _L.call("cobevt_se_gate", _p(mean), _p(w_reduce), _p(b_reduce), _p(w_expand), _p(b_expand), _p(gate), n, c, cs, _stream())
    return gate


def channel_gate(x, gate):
    """x (N, H, W, C) * gate (N, C) fp32 -> (N, H, W, C)"""
    _need_cuda(x, gate)
    n, h, w, c = x.shape
    if tuple(gate.shape) != (n, c) or gate.dtype != torch.float32 or not x.is_contiguous() or not gate.is_contiguous():
        raise CobevtHipError("channel_gate: gate must be (N, C) fp32 for a contiguous (N, H, W, C) map")
    out = torch.empty_like(x)
    _L.call("cobevt_channel_gate_nhwc", _p(x), _p(gate), _p(out), dcode(x.dtype), n, h * w, c, _stream())
    return out


_DEFERRED_LABELS = []


_LABEL_RING = 32


def _label_word(c):
    """The next pinned host word of a ring of _LABEL_RING (entries of _DEFERRED_LABELS are reused round-robin; _check_deferred_labels has
    just read them all).  Pinned memory cannot be allocated while the stream is being captured into a HIP graph: the ring is filled by
    the eager calls before a capture (CapturedTrainStep's warm-up steps); a capture that finds it short skips the copy (None)."""
    global _LABEL_NEXT
    if len(_DEFERRED_LABELS) < _LABEL_RING:
        if torch.cuda.is_current_stream_capturing():
            if not _DEFERRED_LABELS:
                return None
        else:
            _DEFERRED_LABELS.append([torch.zeros(1, dtype=torch.float32).pin_memory(), c])
            return _DEFERRED_LABELS[-1][0]
    _LABEL_NEXT = (_LABEL_NEXT + 1) % len(_DEFERRED_LABELS)
    ent = _DEFERRED_LABELS[_LABEL_NEXT]
    ent[1] = c
    return ent[0]


_LABEL_NEXT = -1


def _check_deferred_labels():
    for word, c in _DEFERRED_LABELS:
        bad = int(word[0])
        if bad:
            word[0] = 0.0
            raise CobevtHipError("weighted_cross_entropy: %d target labels outside [0, %d) in an earlier call (only -100 is ignored)"
                                 % (bad, c))


def check_deferred_label_errors():
    """synchronise and raise if any weighted_cross_entropy call so far saw labels outside [0, C) (other than -100)"""
    torch.cuda.synchronize()
    _check_deferred_labels()


def weighted_cross_entropy(logits, target, weight, want_stats=False):
    """nn.CrossEntropyLoss(weight=weight)(logits (N, C, H, W), target (N, H, W) int64) -> 0-d fp32 tensor on the device
    (vanilla_seg_loss.py:18-23,58-70); forward only."""
    _need_cuda(logits, target)
    if logits.dim() != 4 or tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise CobevtHipError("weighted_cross_entropy expects (N, C, H, W) logits and an (N, H, W) target")
    x, y = logits.contiguous(), target.to(torch.int64).contiguous()
    n, c, h, w = x.shape
    wt = weight.to(device=x.device, dtype=torch.float32).contiguous()
    if wt.numel() != c:
        raise CobevtHipError("weighted_cross_entropy: %d class weights for %d classes" % (wt.numel(), c))
    scratch = torch.empty(3 * n * ((h * w + 4095) // 4096), device=x.device, dtype=torch.float32)
    out = torch.empty(4, device=x.device, dtype=torch.float32)
    _L.call("cobevt_weighted_cross_entropy", _p(x), _p(y), _p(wt), _p(scratch), _p(out), dcode(x.dtype), n, c, h * w, _stream())
    # nn.CrossEntropyLoss raises for targets outside [0, C) other than ignore_index = -100.  Here the count of such labels leaves the
    # device WITHOUT a host sync (a blocking read would drain the launch queue twice per training step): it is copied into a pinned
    # host word behind the kernel and inspected by the following calls (and by check_deferred_label_errors()), so a bad label
    # raises one call late - identically in eager steps and in steps replayed from a captured HIP graph (the copy is a graph node)
    _check_deferred_labels()
    host_word = _label_word(c)
    if host_word is not None:
        host_word.copy_(out[3:4], non_blocking=True)
    return (out[0], out, x, y, wt) if want_stats else out[0]


def iou_counts(pred, label, visibility, label_indices, thresholds, min_visibility):
    """(T, 3) int64 host tensor of (tp, fp, fn) per threshold; nuscenes metrics.py:22-31,56-72.  pred (N, C, hw) fp32 logits on
    the device, label (N, NL, hw), visibility (N, hw) uint8 / None, label_indices: list (length C) of lists of label channels."""
    _need_cuda(pred)
    n, c, hw = pred.shape
    dev = pred.device
    label = label.to(device=dev, dtype=torch.float32).contiguous()
    nl = label.shape[1]
    if len(label_indices) != c or nl > 32 or tuple(label.shape) != (n, nl, hw):
        raise CobevtHipError("iou_counts: %d prediction channels need %d label groups over at most 32 label channels" % (c, c))
    masks = torch.tensor([sum(1 << int(l) for l in group) for group in label_indices], dtype=torch.int64).to(torch.int32).to(dev)
    thr = torch.as_tensor(thresholds, dtype=torch.float32).to(dev).contiguous()
    counts = torch.zeros((thr.numel(), 3), device=dev, dtype=torch.int64)
    vis = None
    mv = -1
    if min_visibility is not None:
        vis = visibility.to(device=dev, dtype=torch.uint8).contiguous()
        mv = int(min_visibility)
    _L.call("cobevt_iou_counts", _p(pred.contiguous()), _p(label), _p(vis), _p(masks), _p(thr), _p(counts), n, c, nl, hw, thr.numel(), mv,
            _stream())
    return counts.cpu()


def sigmoid_focal_loss_mean(pred, label, visibility, label_indices, min_visibility, alpha, gamma):
    """mean sigmoid focal loss over the visible pixels (nuscenes losses.py:27-84, forward).  pred (N, C, hw) fp32 logits on the
    device; label (N, NL, hw); label_indices: list (length C) of label-channel lists, or None = use label channel c as is."""
    _need_cuda(pred)
    n, c, hw = pred.shape
    dev = pred.device
    label = label.to(device=dev, dtype=torch.float32).contiguous()
    nl = label.shape[1]
    soft = label_indices is None
    if (soft and nl != c) or (not soft and len(label_indices) != c) or nl > 32 or tuple(label.shape) != (n, nl, hw):
        raise CobevtHipError("sigmoid_focal_loss_mean: inconsistent prediction / label channels")
    masks = None
    if not soft:
        masks = torch.tensor([sum(1 << int(l) for l in g) for g in label_indices], dtype=torch.int64).to(torch.int32).to(dev)
    vis, mv = None, -1
    if min_visibility is not None:
        vis, mv = visibility.to(device=dev, dtype=torch.uint8).contiguous(), int(min_visibility)
    scratch = torch.empty(2 * n * ((hw + 2047) // 2048), device=dev, dtype=torch.float32)
    out = torch.empty(3, device=dev, dtype=torch.float32)
    _L.call("cobevt_sigmoid_focal_loss", _p(pred.float().contiguous()), _p(label), _p(vis), _p(masks), _p(scratch), _p(out), n, c, nl, hw,
            mv, ctypes.c_float(alpha), ctypes.c_float(gamma), int(soft), _stream())
    return out[0]


# ----------------------------------------------------------------------------------------------
# multi-tensor Adam / AdamW (csrc/train_glue.hip; host/optim.py is the torch.optim.Optimizer in front of it)
# ----------------------------------------------------------------------------------------------
ADAM_MAX_TENSORS = 64      # tensors of one cobevt_multi_adam launch: their pointers travel in the kernel arguments
ADAM_CHUNK = 4096          # elements per workgroup
AdamLaunch = namedtuple("AdamLaunch", "first count chunks")     # tensors [first, first + count) and the chunk count of each


def adam_groups(numels):
    """How the tensors of one param group are dealt to update launches: in order, at most ADAM_MAX_TENSORS per launch, a launch's
    grid (the sum of its chunk counts) below 2^31.  -> [AdamLaunch]; pure, no device."""
    out, first, chunks, total = [], 0, [], 0
    for i, n in enumerate(numels):
        n = int(n)
        if n < 1:
            raise CobevtHipError("adam_groups: tensor %d has %d elements" % (i, n))
        c = (n + ADAM_CHUNK - 1) // ADAM_CHUNK
        if c > 0x7fffffff:
            raise CobevtHipError("adam_groups: tensor %d needs %d chunks, more than one launch can hold" % (i, c))
        if len(chunks) == ADAM_MAX_TENSORS or total + c > 0x7fffffff:
            out.append(AdamLaunch(first, len(chunks), tuple(chunks)))
            first, chunks, total = i, [], 0
        chunks.append(c)
        total += c
    if chunks:
        out.append(AdamLaunch(first, len(chunks), tuple(chunks)))
    return out


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def multi_adam(params, grads, exp_avgs, exp_avg_sqs, steps, coef, lr, beta1, beta2, eps, weight_decay, adamw=True, lr_dev=None,
               grad_scale=None, found_inf=None):
    """One Adam (adamw=False: L2 weight decay) or AdamW step on lists of fp32 contiguous device tensors, in place: `steps` (one fp32
    word each) advance by one, then params / exp_avgs / exp_avg_sqs are updated from grads.  coef: fp32 scratch of >= 4 floats per
    tensor, overwritten.  lr_dev (an fp64 device word) replaces the float `lr` when given - inside a stream capture that is what
    lets a replay follow a scheduler; grad_scale / found_inf are torch.amp.GradScaler's device words (found_inf != 0: nothing moves).
    One prepare launch per 448 tensors + one update launch per 64."""
    n = len(params)
    if n < 1 or not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(steps) == n):
        raise CobevtHipError("multi_adam: five lists of one length >= 1, got %s" % ([len(x) for x in (params, grads, exp_avgs, exp_avg_sqs, steps)],))
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0 and eps >= 0.0 and weight_decay >= 0.0 and (lr_dev is not None or lr >= 0.0)):
        raise CobevtHipError("multi_adam: need 0 <= beta < 1, eps >= 0, weight_decay >= 0, lr >= 0")
    dev = params[0].device
    for i in range(n):
        p = params[i]
        for t, what in ((p, "param"), (grads[i], "grad"), (exp_avgs[i], "exp_avg"), (exp_avg_sqs[i], "exp_avg_sq")):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != dev or t.is_sparse:
                raise CobevtHipError("multi_adam: %s %d must be a dense contiguous fp32 tensor of %d elements on %s, got %s %s on %s"
                                     % (what, i, p.numel(), dev, t.dtype, tuple(t.shape), t.device))
        if steps[i].dtype != torch.float32 or steps[i].numel() != 1 or steps[i].device != dev:
            raise CobevtHipError("multi_adam: step %d must be one fp32 word on %s" % (i, dev))
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.numel() < 4 * n or coef.device != dev:
        raise CobevtHipError("multi_adam: coef must be contiguous fp32 with >= %d elements on %s" % (4 * n, dev))
    for t, what, dt in ((lr_dev, "lr_dev", torch.float64), (grad_scale, "grad_scale", torch.float32), (found_inf, "found_inf", torch.float32)):
        if t is not None and (t.dtype != dt or t.numel() != 1 or t.device != dev):
            raise CobevtHipError("multi_adam: %s must be one %s word on %s" % (what, dt, dev))
    _need_cuda(params[0], coef)
    launches = adam_groups([p.numel() for p in params])
    _L.call("cobevt_adam_prepare", _ptr_array(steps), n, _p(coef), int(bool(adamw)), float(beta1), float(beta2), float(weight_decay),
            float(lr), _p(lr_dev), _p(grad_scale), _p(found_inf), _stream())
    for la in launches:
        sl = slice(la.first, la.first + la.count)
        _L.call("cobevt_multi_adam", _ptr_array(params[sl]), _ptr_array(grads[sl]), _ptr_array(exp_avgs[sl]), _ptr_array(exp_avg_sqs[sl]),
                _longs(*[p.numel() for p in params[sl]]), la.count, ctypes.c_void_p(coef.data_ptr() + 16 * la.first), int(bool(adamw)),
                float(beta1), float(beta2), float(eps), _stream())
