"""The routing table of ops.conv2d / ops.linear and of the training launchers (tests/launch_trace.py case `conv2d_table`): one row per
branch of the routing code.  Data and plan-building calls only; the tensors are zeros, made by the runner.

A conv2d row: name, w = weight shape (2-D: a Linear, run through ops.linear), x = input shape, dt, knobs = ops switches set for the
row, lib = the library variant active while it runs, res = with a residual, out = spatial size of a preallocated (padded) result,
ln / bn / pre_bn = with that layer folded in, and whatever else ops.ConvPlan takes."""
import torch

from cobevt_amd import ops


def row(name, w, x, dt="bf16", knobs=None, lib="", res=False, out=None, ln=False, bn=False, pre_bn=False, **plan):
    return dict(name=name, w=w, x=x, dt=dt, knobs=knobs or {}, lib=lib, res=res, out=out, ln=ln, bn=bn, pre_bn=pre_bn, plan=plan)


def both(name, w, x, **kw):
    return [row("%s.%s" % (name, dt), w, x, dt=dt, **kw) for dt in ("bf16", "fp32")]


S2 = dict(stride=2)
P1 = dict(pad=1)
S2P1 = dict(stride=2, pad=1)
STEM = dict(stride=2, pad=3, smallc=True, act=1, bn=True)

ROWS = (
    # ---- dense rows
    both("rows_ln_k128", (64, 128), (2, 8, 128), ln=True)              # bf16: fused in the small-K kernel; fp32: separate LayerNorm
    + both("rows_ln_k64", (64, 64), (2, 8, 64), ln=True)               # fp32: cobevt_linear_rows with ln = 1
    + both("rows_ln_k256", (64, 256), (2, 8, 256), ln=True)
    + both("rows_plain", (128, 128), (2, 8, 128))
    + both("rows_cout_odd", (12, 64), (2, 8, 64))                      # 12 % 8 != 0, and 6 % 4 != 0 below
    + [row("rows_cout_6.fp32", (6, 64), (2, 8, 64), dt="fp32")]
    + both("rows_cout_4104", (4104, 64), (1, 8, 64))
    + both("rows_s2_res", (128, 64, 1, 1), (1, 8, 8, 64), res=True, **S2)
    + both("rows_s2", (128, 64, 1, 1), (1, 8, 8, 64), **S2)
    + both("rows_s2_strided0", (128, 64, 1, 1), (1, 8, 8, 64), knobs={"GEMM_ROWS3_STRIDED": 0}, **S2)
    + both("rows_max_k128_k256", (64, 256), (2, 8, 256), knobs={"GEMM_ROWS3_MAX_K": 128})
    + both("rows_max_k128_k128", (64, 128), (2, 8, 128), knobs={"GEMM_ROWS3_MAX_K": 128})
    + both("rows_min_m", (64, 128), (2, 8, 128), knobs={"GEMM_ROWS3_MIN_M": 17})
    + both("rows_min_m_reached", (64, 128), (2, 8, 128), knobs={"GEMM_ROWS3_MIN_M": 16})
    + both("rows_rows64", (64, 128), (2, 8, 128), knobs={"GEMM_ROWS3_ROWS64_MIN_M": 1})
    + both("rows_rows64_below", (64, 128), (2, 8, 128), knobs={"GEMM_ROWS3_ROWS64_MIN_M": 17})
    + both("rows2_chunked", (64, 128), (2, 8, 128), knobs={"USE_GEMM_ROWS2": True, "USE_GEMM_ROWS3": False, "USE_GEMM_ROWS3_F32": False})
    + both("rows2_ln", (64, 64), (2, 8, 64), ln=True, knobs={"USE_GEMM_ROWS2": True, "USE_GEMM_ROWS3": False, "USE_GEMM_ROWS3_F32": False})
    + both("rows2_cout_odd", (6, 64), (2, 8, 64), knobs={"USE_GEMM_ROWS2": True, "USE_GEMM_ROWS3": False, "USE_GEMM_ROWS3_F32": False})
    + both("rows2_small_k_first", (64, 128), (2, 8, 128), knobs={"USE_GEMM_ROWS2": True})
    + both("rows_off", (64, 128), (2, 8, 128), knobs={"USE_GEMM_ROWS": False})
    + both("rows_off_ln", (64, 64), (2, 8, 64), ln=True, knobs={"USE_GEMM_ROWS": False})
    + both("rows3_off", (64, 128), (2, 8, 128), knobs={"USE_GEMM_ROWS3": False})
    + both("rows3_f32_off", (64, 128), (2, 8, 128), knobs={"USE_GEMM_ROWS3_F32": False})
    + both("rows_pre_bn", (64, 128, 1, 1), (1, 8, 8, 128), pre_bn=True, pre_relu=True, bn=True, act=1)
    + both("rows_res", (128, 128), (2, 8, 128), res=True)
    + both("rows_out_padded", (64, 128, 1, 1), (1, 8, 8, 128), out=(10, 10))
    + both("rows_out_padded_res", (64, 128, 1, 1), (1, 8, 8, 128), out=(10, 10), res=True)
    + both("rows_out_exact", (64, 128, 1, 1), (1, 8, 8, 128), out=(8, 8))
    # ---- 3x3
    + both("c3_cout32", (32, 64, 3, 3), (1, 16, 16, 64), bn=True, act=1, **P1)        # bf16: 32-cout tiles; fp32: cout < 64, LDS-staged
    + both("c3_cout48", (48, 64, 3, 3), (1, 16, 16, 64), **P1)                        # cout < 64: LDS-staged
    + both("c3_big_grid", (128, 128, 3, 3), (20, 64, 64, 128), **P1)                  # 640 workgroups: LDS-staged
    + both("c3_small_grid", (128, 128, 3, 3), (1, 32, 32, 128), **P1)
    + both("c3_small_grid_no_small_tiles", (128, 128, 3, 3), (1, 32, 32, 128), knobs={"USE_CONV3_SMALL_TILES": False}, **P1)
    + both("c3_cout32_no_small_tiles", (32, 64, 3, 3), (1, 16, 16, 64), knobs={"USE_CONV3_SMALL_TILES": False}, **P1)
    + both("c3_mid_grid", (256, 256, 3, 3), (20, 32, 32, 256), **P1)
    + both("c3_res", (64, 64, 3, 3), (1, 32, 32, 64), res=True, act=1, **P1)
    + both("c3_s2_cout64", (64, 64, 3, 3), (1, 32, 32, 64), **S2P1)
    + both("c3_s2_cout128", (128, 64, 3, 3), (1, 32, 32, 64), **S2P1)
    + both("c3_s2_odd_hw", (128, 64, 3, 3), (2, 31, 33, 64), **S2P1)
    + [row("c3_s2.fp32.lib%s" % (v or "native"), (128, 32, 3, 3), (1, 32, 32, 32), dt="fp32", lib=v, **S2P1) for v in ("", "f32s", "f32h")]
    + [row("c3_s2.bf16.lib%s" % v, (128, 64, 3, 3), (1, 32, 32, 64), lib=v, **S2P1) for v in ("f32s", "f32h")]
    + [row("c3_packed.fp32.lib%s" % (v or "native"), (128, 32, 3, 3), (20, 64, 64, 32), dt="fp32", lib=v, **P1) for v in ("", "f32s", "f32h")]
    + [row("c3_packed_cout64.fp32.lib%s" % (v or "native"), (64, 32, 3, 3), (4, 32, 32, 32), dt="fp32", lib=v, **P1) for v in ("", "f32s", "f32h")]
    + both("c3_s2_off", (128, 64, 3, 3), (1, 32, 32, 64), knobs={"USE_CONV3_S2": False}, **S2P1)
    + both("c3_wfrag_off", (128, 128, 3, 3), (1, 32, 32, 128), knobs={"USE_CONV3_WFRAG": False}, **P1)
    + both("c3_wfrag_off_s2", (128, 64, 3, 3), (1, 32, 32, 64), knobs={"USE_CONV3_WFRAG": False}, **S2P1)
    + both("c3_off", (128, 128, 3, 3), (1, 32, 32, 128), knobs={"USE_CONV3X3": False}, **P1)
    + both("c3_variant150", (128, 128, 3, 3), (1, 32, 32, 128), knobs={"CONV3_VARIANT": 150}, **P1)
    + both("c3_variant150_s2", (128, 64, 3, 3), (1, 32, 32, 64), knobs={"CONV3_VARIANT": 150}, **S2P1)
    + both("c3_variant_lds", (128, 128, 3, 3), (1, 32, 32, 128), knobs={"CONV3_VARIANT": -1}, **P1)       # tools/conv_graph_probe.py's "lds"
    + both("c3_variant_lds_s2", (128, 64, 3, 3), (1, 32, 32, 64), knobs={"CONV3_VARIANT": -1}, **S2P1)
    + both("c3_store_mode1", (64, 64, 3, 3), (1, 16, 16, 64), store_mode=1, **P1)
    + both("c3_upsample", (64, 64, 3, 3), (1, 16, 16, 64), upsample=True, **P1)
    + both("c3_cin96", (64, 96, 3, 3), (1, 16, 16, 96), **P1)                         # 96 = 3 * 32: no fragment table in bf16
    + both("c3_cin48", (64, 48, 3, 3), (1, 16, 16, 48), **P1)                         # ... nor in fp32 (16-channel chunks)
    + both("c3_out_padded", (64, 64, 3, 3), (1, 16, 16, 64), out=(18, 18), **P1)
    + both("c3_pre_bn", (64, 64, 3, 3), (1, 16, 16, 64), pre_bn=True, pre_relu=True, **P1)
    + both("c3_pad0", (64, 64, 3, 3), (1, 16, 16, 64))
    # ---- the others
    + both("head", (3, 64, 3, 3), (1, 16, 16, 64), store_mode=2, **P1)
    + both("head_off", (3, 64, 3, 3), (1, 16, 16, 64), store_mode=2, knobs={"USE_HEAD_CONV": False}, **P1)
    + both("head_cout8", (8, 64, 3, 3), (1, 16, 16, 64), store_mode=2, **P1)
    + both("stem_even", (64, 3, 7, 7), (2, 32, 48, 3), **STEM)
    + both("stem_odd", (64, 3, 7, 7), (2, 33, 47, 3), **STEM)
    + both("stem_off", (64, 3, 7, 7), (2, 32, 48, 3), knobs={"USE_STEM": False}, **STEM)
    + both("smallc_3x3", (32, 3, 3, 3), (1, 16, 16, 3), smallc=True, **P1)
    + both("pad_br", (32, 3, 3, 3), (1, 17, 17, 3), smallc=True, stride=2, pad=0, pad_br=1)
    + both("k5", (32, 32, 5, 5), (1, 16, 16, 32), pad=2)
    + both("store_mode3", (16, 32, 1, 1), (1, 8, 8, 32), store_mode=3)
)

# autograd._igemm_rows(x, w2, cout, cin, kh, kw, bias, stride, pad, ho, wo): (x shape, dtype, cout, kh, stride, pad, with bias)
IGEMM_ROWS = (((2, 8, 8, 16), "bf16", 32, 3, 1, 1, True), ((2, 8, 8, 3), "bf16", 32, 7, 2, 3, False),
              ((2, 8, 8, 16), "fp32", 32, 3, 2, 1, False), ((2, 8, 8, 6), "fp32", 32, 1, 1, 0, True))
# autograd._conv3_strips(x, operand, variant, cout, bias, stride): (x shape, variant, cout, stride, with bias); the operand is
# autograd.conv3_weight_operand's, so its sizes are the training path's own
CONV3_STRIPS = (((2, 16, 16, 64), 113, 128, 1, True), ((2, 16, 16, 64), 0, 128, 1, False), ((2, 15, 17, 64), 151, 64, 2, False))
# autograd._rows_gemm(x2d, frag, n_out, k_in, bias): (rows, n_out, k_in, with bias)
ROWS_GEMM = ((48, 256, 128, True), (7, 64, 512, False))
# Conv2dFn's 3x3 tile choice (n, ho, wo, cin, cout, stride), under CONV3_VARIANT = 0 and (last item) pinned
STRIPS_PLAN = ((1, 32, 32, 128, 128, 1, 0), (20, 64, 64, 128, 128, 1, 0), (5, 64, 64, 128, 32, 1, 0), (20, 32, 32, 128, 256, 2, 0),
               (20, 16, 16, 256, 64, 2, 0), (1, 32, 32, 128, 128, 1, 140), (1, 32, 32, 128, 128, 2, -1))

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


# ---- the routing table of the TRAINING convolutions (tests/launch_trace.py case `train_conv_table`): autograd.Conv2dFn forward and
# backward, one row per branch.  x = channels-last input shape (n, h, w, cin); knobs = autograd.USE_* switches set for the row;
# variant = ops.CONV3_VARIANT; chunks = what the fake library answers to the two *_chunks questions (0 when not named);
# linear = the weight shape (N, K) of a row that goes through autograd.linear_weight instead (x is then (..., K)), and as_conv = the
# 1 x 1 convolution it must arrive as: (h, w, cin, cout) of a one-image map.
def trow(name, x, cout=None, k=1, stride=1, pad=0, dt="bf16", bias=True, x_grad=True, w_grad=True, knobs=None, variant=0, chunks=None,
         linear=None, as_conv=None):
    return dict(name=name, x=x, cout=cout, k=k, stride=stride, pad=pad, dt=dt, bias=bias, x_grad=x_grad, w_grad=w_grad, knobs=knobs or {},
                variant=variant, chunks=chunks or {}, linear=linear, as_conv=as_conv)


def train_conv_args(r):
    """the arguments of autograd.train_conv_route for a row, after the dtype code: (n, h, w, cin, cout, k, stride, pad, x_grad, w_grad)"""
    n, h, w, cin, cout = ((1,) + r["as_conv"]) if r["linear"] else (r["x"] + (r["cout"],))
    return (n, h, w, cin, cout, r["k"], r["stride"], r["pad"], r["x_grad"], r["w_grad"])


X8, X16 = (2, 8, 8), (2, 16, 16)
C3 = dict(k=3, pad=1)
C3S2 = dict(k=3, stride=2, pad=1)
LIN_CHUNKS, C3_CHUNKS = "cobevt_linear_wgrad_chunks", "cobevt_conv_wgrad3_chunks"

TRAIN_ROWS = (
    # ---- forward and input gradient, bf16 (both chunk questions answered 0: the weight gradient falls to the blocked / generic kernel)
    trow("1x1", X8 + (128,), 32),                                                   # the row GEMM both ways; blocked mode 0
    trow("1x1_rows_gemm_off", X8 + (128,), 32, bias=False, knobs={"USE_TRAIN_ROWS_GEMM": False}),
    trow("1x1_cin520", X8 + (520,), 32),                                            # over the 512 cap
    trow("1x1_cout12", X8 + (64,), 12),                                             # 12 % 8 != 0; the bias gradient through cobevt_f64_to_f32
    trow("1x1_s2", X8 + (64,), 128, stride=2),                                      # shortcut conv: zero-stuffed dgrad, blocked mode 1
    trow("3x3", X16 + (64,), 64, **C3),                                             # strips both ways, operands from the paired launch
    trow("3x3_cout32", X16 + (64,), 32, bias=False, **C3),                          # strips forward, implicit-GEMM dgrad
    trow("3x3_cin8", X16 + (8,), 64, **C3),                                         # implicit-GEMM forward, strips dgrad
    trow("3x3_cout48", X16 + (64,), 48, **C3),                                      # forward variant 0: the LDS-staged kernel
    trow("3x3_cin48", X16 + (48,), 64, **C3),                                       # dgrad variant 0
    trow("3x3_s2", X16 + (64,), 128, **C3S2),                                       # stride-2 strips, zero-stuffed dgrad, blocked mode 1
    trow("3x3_strips_off", X16 + (64,), 64, knobs={"USE_TRAIN_STRIPS": False}, **C3),
    trow("3x3_variant140", X16 + (64,), 64, variant=140, **C3),
    trow("stem", X16 + (3,), 64, k=7, stride=2, pad=3),                             # klut gather path (x widened to fp32); blocked mode 2
    trow("5x5", X16 + (64,), 64, k=5, pad=2),                                       # no blocked form: the generic kernel, bf16 code
    trow("3x3_s2_p0", X16 + (64,), 64, k=3, stride=2),
    trow("3x3_x_no_grad", X16 + (64,), 64, x_grad=False, **C3),
    # ---- weight gradient, bf16
    trow("1x1_linear_wgrad", X8 + (128,), 32, chunks={LIN_CHUNKS: 3}),
    trow("3x3_wgrad3", X16 + (64,), 64, chunks={C3_CHUNKS: 4}, **C3),
    trow("3x3_wgrad3_refused", X16 + (64,), 64, chunks={C3_CHUNKS: -4}, **C3),
    trow("3x3_wgrad3_off", X16 + (64,), 64, knobs={"USE_WGRAD3": False}, chunks={C3_CHUNKS: 4}, **C3),
    trow("1x1_wgrad3_off", X8 + (128,), 32, knobs={"USE_WGRAD3": False}, chunks={LIN_CHUNKS: 3}),
    trow("3x3_s2_blocked_strided_off", X16 + (64,), 128, knobs={"USE_WGRAD_BLOCKED_STRIDED": False}, **C3S2),
    trow("3x3_blocked_strided_off", X16 + (64,), 64, knobs={"USE_WGRAD_BLOCKED_STRIDED": False}, **C3),       # mode 0 stays blocked
    trow("3x3_blocked_off", X16 + (64,), 64, knobs={"USE_WGRAD_BLOCKED": False}, **C3),
    trow("1x1_blocked_off", X8 + (128,), 32, knobs={"USE_WGRAD_BLOCKED": False}),
    trow("3x3_w_no_grad", X16 + (64,), 64, w_grad=False, chunks={C3_CHUNKS: 4}, **C3),
    trow("3x3_torch_prep", X16 + (64,), 64, knobs={"USE_TORCH_OPERAND_PREP": True}, **C3),
    trow("3x3_s2_torch_prep", X16 + (64,), 128, knobs={"USE_TORCH_OPERAND_PREP": True}, **C3S2),
    # ---- fp32: conv_weight_rows, the implicit GEMM twice, the generic weight gradient with the fp32 code
    trow("3x3.fp32", X16 + (64,), 64, dt="fp32", chunks={C3_CHUNKS: 4}, **C3),
    trow("1x1.fp32", X8 + (128,), 32, dt="fp32", bias=False, chunks={LIN_CHUNKS: 3}),
    trow("3x3_s2.fp32", X16 + (64,), 128, dt="fp32", **C3S2),
    # ---- autograd.linear_weight: the rows as an H x W map
    trow("linear_1024", (4, 256, 128), linear=(32, 128), as_conv=(4, 256, 128, 32)),
    trow("linear_64", (64, 128), linear=(32, 128), bias=False, as_conv=(4, 16, 128, 32)),
    trow("linear_48", (48, 128), linear=(32, 128), as_conv=(48, 1, 128, 32)),       # no candidate width leaves four map rows
    trow("linear_k6_n5", (16, 6), linear=(5, 6), as_conv=(16, 1, 8, 8)),            # zero-padded to K = N = 8, run again
    trow("linear.fp32", (64, 128), linear=(32, 128), dt="fp32", as_conv=(4, 16, 128, 32)),
)


def plan(r):
    """the ConvPlan of a row, on the CPU"""
    w = r["w"]
    cout, cin = w[0], w[1]
    return ops.ConvPlan(torch.zeros(w), bias=torch.zeros(cout), dtype=DTYPES[r["dt"]], device="cpu",
                        ln=torch.nn.LayerNorm(cin) if r["ln"] else None, bn=torch.nn.BatchNorm2d(cout).eval() if r["bn"] else None,
                        pre_bn=torch.nn.BatchNorm2d(cin).eval() if r["pre_bn"] else None, **r["plan"])
