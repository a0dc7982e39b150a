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


def plan(r):
    """the ConvPlan of a row, on the CPU"""
    w = r["w"]
    cout, cin = w[0], w[1]
    return ops.ConvPlan(torch.zeros(w), bias=torch.zeros(cout), dtype=DTYPES[r["dt"]], device="cpu",
                        ln=torch.nn.LayerNorm(cin) if r["ln"] else None, bn=torch.nn.BatchNorm2d(cout).eval() if r["bn"] else None,
                        pre_bn=torch.nn.BatchNorm2d(cin).eval() if r["pre_bn"] else None, **r["plan"])
