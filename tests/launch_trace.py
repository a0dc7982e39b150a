"""CPU launch traces: which C-ABI entry point a model calls, in which library, with which scalar arguments.

`lib.load` is replaced by a fake library that records every call and answers 0, and the device guards become no-ops, so whole
models run on CPU tensors in seconds and the launch sequence is a pure function of the routing code (ops.conv2d, window_attention,
the *_fusable predicates, the host modules).  tests/test_launch_traces.py replays every case below against its fixture under
tests/golden/launch_traces/; `python tests/launch_trace.py` rewrites the fixtures (gzip of one JSON record per line,
[library variant, symbol, arguments]: `zcat` shows them).

Only lib.load, ops._need_cuda / ops._stream (and the copies autograd binds at import), HipModule._require_inference and
host.training._check are patched, so the same recorder runs on any commit that has those names.
"""
import ctypes
import gzip
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _path in (ROOT, os.path.join(ROOT, "tests", "golden")):       # the package, and the case modules the models are built from
    if _path not in sys.path:
        sys.path.insert(0, _path)

from cobevt_amd import autograd, host, lib, ops, synth  # noqa: E402
from cobevt_amd.host import runtime, training  # noqa: E402
from cobevt_amd.registry import create_model  # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "golden", "launch_traces")
MODES = ("bf16", "fp32", "fp32_split", "fp32_fast")
_STREAM = object()       # what the patched ops._stream returns: dropped from the record

# arguments that legitimately vary, by symbol and position among the recorded arguments: the attention dropout seed word is drawn
# from torch's CPU generator, so it moves with the number of draws made before it and with torch's generator itself
MASKED = {"cobevt_window_attention_lse": (10,), "cobevt_window_attention_bwd": (16,)}


def _value(a):
    """One argument without its address."""
    if a is None:
        return "null"
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, ctypes.Array):
        if issubclass(a._type_, (ctypes.c_void_p, ctypes._Pointer)):
            return ["ptr" if v else "null" for v in a]
        if issubclass(a._type_, ctypes.c_char):
            return "buffer"
        return [_value(v) for v in a]
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    if type(a).__name__ == "CArgObject":        # ctypes.byref(..): an output word
        return "ref"
    raise TypeError("launch_trace: no rule for an argument of type %s" % type(a).__name__)


class Recorder(object):
    """records = [[variant, symbol, [arguments]], ...]; status(name) is what the fake library answers (0 by default)."""

    def __init__(self, status=None):
        self.records = []
        self.status = status or {}

    def load(self, variant=None):
        return _FakeLib(self, lib.get_variant() if variant is None else variant)


class _FakeLib(object):
    def __init__(self, rec, variant):
        self._rec, self._variant = rec, variant

    def __getattr__(self, name):
        if name == "cobevt_strerror":
            return lambda code: b"status %d of the fake library" % code
        if name == "cobevt_abi_version":
            return lambda: 1
        if not name.startswith("cobevt_"):
            raise AttributeError(name)

        def launch(*args):
            vals = [_value(a) for a in args if a is not _STREAM]
            for pos in MASKED.get(name, ()):
                vals[pos] = "masked"
            self._rec.records.append([self._variant, name, vals])
            if name == "cobevt_layernorm_bwd_scratch":
                return 16                         # a size, not a status: a non-empty scratch, so that the launch that follows records a pointer, not null
            return self._rec.status.get(name, 0)
        return launch


def install(setattr_, rec):
    """Route every launch to `rec` and switch the device guards off; setattr_(object, name, value) is pytest's monkeypatch.setattr
    (or plain setattr for the fixture writer, which exits afterwards)."""
    noop = lambda *a, **k: None         # noqa: E731
    stream = lambda: _STREAM            # noqa: E731
    setattr_(lib, "load", rec.load)
    for mod in (ops, autograd):
        setattr_(mod, "_need_cuda", noop)
        setattr_(mod, "_stream", stream)
    setattr_(runtime.HipModule, "_require_inference", noop)
    setattr_(training, "_check", noop)


# ----------------------------------------------------------------------------------------------
# cases: name -> function that runs the model (the recorder is already installed)
# ----------------------------------------------------------------------------------------------
def _corpbevt(mode):
    def run():
        torch.manual_seed(0)
        model = synth.fill_module_(host.CorpBEVT(synth.corpbevt_small_config()), 0).eval()
        batch = synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=0)
        with torch.no_grad(), host.compute_dtype(mode):
            model(batch)
    return run


CVT_KINDS = (("single", "cross_view_transformer", 1), ("swap_fuse", "cross_view_transformer_swap_fuse", 2),
             ("fcooper", "cross_view_transformer_fcooper", 2), ("att_fuse", "cross_view_transformer_att_fuse", 2),
             ("v2vnet", "cross_view_transformer_v2vnet", 2), ("disconet", "cross_view_transformer_disconet", 2))


def _cvt(kind, core, agents, mode):
    def run():
        torch.manual_seed(0)
        model = synth.fill_module_(create_model({"model": {"core_method": core, "args": synth.cvt_small_config(kind)}}), 0).eval()
        batch = synth.opv2v_batch(agents=agents, cams=2, image=128, max_cav=3, seed=0)
        with torch.no_grad(), host.compute_dtype(mode):
            model(batch)
    return run


def _corpbevt_train():
    torch.manual_seed(0)
    model = synth.fill_module_(host.CorpBEVT(synth.corpbevt_small_config()), 0).train()
    batch = synth.opv2v_batch(agents=2, cams=2, image=128, max_cav=3, seed=0)
    with torch.enable_grad(), host.compute_dtype("fp32"):
        model(batch)["dynamic_seg"].float().sum().backward()


def _nuscenes(pyramid, mode):
    """the nuScenes models on fixed backbone feature maps: CVT (cases_nusc_cvt) or the pyramid-axial SinBEVT (synth.nuscenes_config)"""
    def run():
        import cases_nusc_cvt as cc
        from cobevt_amd.host import nuscenes as nu
        torch.manual_seed(0)
        if pyramid:
            c = synth.nuscenes_config()
            feats, image, intr, ext = synth.nuscenes_inputs()
            enc = nu.PyramidAxialEncoder(synth.FeatureMapBackbone(feats), **c["encoder"])
            model = nu.CrossViewTransformer(enc, nu.Decoder(**c["decoder"]), c["dim_last"], c["outputs"])
        else:
            feats, image, intr, ext = cc.inputs()
            model = cc.build(nu, synth.FeatureMapBackbone(feats))
        model = synth.fill_module_(model, 0).eval()
        with torch.no_grad(), host.compute_dtype(mode):
            model({"image": image, "intrinsics": intr, "extrinsics": ext})
    return run


def _point_pillar(mode):
    """inference only: in train() mode host.training.lidar_trains sends CPU tensors to the stand-alone forward, so the training
    graph of the pillar front end cannot be traced here"""
    def run():
        import cases_pillar as cp
        torch.manual_seed(0)
        model = synth.fill_module_(host.PointPillarFuseBEVT(cp.model_args()), 0).eval()
        with torch.no_grad(), host.compute_dtype(mode):
            model({"processed_lidar": cp.voxels(), "record_len": torch.tensor(cp.RECORD_LEN, dtype=torch.int32)})
    return run


def _voxelize():
    import cases_voxel as cv
    import numpy as np
    pts, offs, rng = cv.counts_case()
    # (an explicit workspace: the default one is cached per shape, so only a process's first call would ask for its size)
    ops.voxelize_points(torch.from_numpy(np.ascontiguousarray(pts)), torch.from_numpy(np.asarray(offs, dtype=np.int32)), rng, cv.VOXEL_SIZE,
                        32, 35, workspace=torch.empty(1, dtype=torch.int32))


def _detect_post():
    import cases_detect as cd
    post = host.VoxelPostprocessor(cd.anchor_params(cd.A_GRID, "hwl", 6.0, 4.0), train=False)
    cavs, _ = cd.case_a(post.generate_anchor_box())
    dev_cavs = [tuple(torch.from_numpy(t) for t in cav) for cav in cavs]
    ops.detect_post_process(dev_cavs, cd.SCORE_THRESHOLD, cd.NMS_THRESH, "hwl")


_RECORDER = None        # the Recorder of the trace() that is running


def _note(symbol, *vals):
    """a pseudo-record (no launch): a row boundary or a host-side decision of the conv2d table"""
    _RECORDER.records.append(["", symbol, list(vals)])


def _conv2d_table():
    """every branch of ops.conv2d's routing and the training launchers of autograd.py, one direct call per row of cases_conv on zero
    tensors; each row sets its own switches and library variant and restores them"""
    import cases_conv as cv

    def zeros(shape, dt):
        return torch.zeros(shape, dtype=cv.DTYPES[dt])

    for r in cv.ROWS:
        plan = cv.plan(r)
        old = {k: getattr(ops, k) for k in r["knobs"]}
        old_variant = lib.get_variant()
        x = zeros(r["x"], "fp32" if plan.smallc else r["dt"])
        _note("row", r["name"])
        try:
            for k, v in r["knobs"].items():
                setattr(ops, k, v)
            lib.set_variant(r["lib"])
            if len(r["w"]) == 2:
                ops.linear(x, plan, residual=zeros(r["x"][:-1] + (plan.cout,), r["dt"]) if r["res"] else None)
            else:
                n = r["x"][0]
                ho, wo = plan.out_hw(*r["x"][1:3])
                ops.conv2d(x, plan, residual=zeros((n, ho, wo, plan.cout), r["dt"]) if r["res"] else None,
                           out=zeros((n,) + r["out"] + (plan.cout,), r["dt"]) if r["out"] else None)
        finally:
            lib.set_variant(old_variant)
            for k, v in old.items():
                setattr(ops, k, v)
    # the training launchers, while an fp32-storage library is the active one: they must reach the native library ("") all the same
    old_variant = lib.get_variant()
    lib.set_variant("f32s")
    try:
        for shape, dt, cout, k, stride, pad, has_bias in cv.IGEMM_ROWS:
            _note("row", "autograd._igemm_rows")
            cin = shape[3]
            w2 = zeros((cout, autograd._kpad(k * k * cin, cv.DTYPES[dt])), dt)
            ho, wo = ((s + 2 * pad - k) // stride + 1 for s in shape[1:3])
            autograd._igemm_rows(zeros(shape, dt), w2, cout, cin, k, k, torch.zeros(cout) if has_bias else None, stride, pad, ho, wo)
        for shape, variant, cout, stride, has_bias in cv.CONV3_STRIPS:
            _note("row", "autograd._conv3_strips")
            operand = autograd.conv3_weight_operand(torch.zeros(cout, shape[3], 3, 3), variant, False)     # (one more launch in the trace)
            autograd._conv3_strips(zeros(shape, "bf16"), operand, variant, cout, torch.zeros(cout) if has_bias else None, stride)
        for m, n_out, k_in, has_bias in cv.ROWS_GEMM:
            _note("row", "autograd._rows_gemm")
            autograd._rows_gemm(zeros((m, k_in), "bf16"), zeros((8,), "bf16"), n_out, k_in, torch.zeros(n_out) if has_bias else None)
    finally:
        lib.set_variant(old_variant)
    # Conv2dFn's 3x3 tile choice: ops.conv3_variant on 64-channel chunks (autograd.conv3_strips_plan on the commits that still have it)
    tile_choice = getattr(autograd, "conv3_strips_plan", None) or (
        lambda n, ho, wo, cin, cout, stride: ops.conv3_variant(n, ho, wo, cin, cout, 64, stride))
    for args in cv.STRIPS_PLAN:
        old = ops.CONV3_VARIANT
        try:
            ops.CONV3_VARIANT = args[6]
            _note("Conv2dFn.tile_choice", *(args + (tile_choice(*args[:6]),)))
        finally:
            ops.CONV3_VARIANT = old


def _train_conv_table():
    """every branch of the training convolution's routing (autograd.Conv2dFn forward + backward, autograd.linear_weight), one call per
    row of cases_conv.TRAIN_ROWS on zero tensors; each row sets its own autograd switches, ops.CONV3_VARIANT and the fake library's
    answers to the *_chunks questions, and restores them"""
    import cases_conv as cv
    status = _RECORDER.status
    for r in cv.TRAIN_ROWS:
        dtype = cv.DTYPES[r["dt"]]
        old = {k: getattr(autograd, k) for k in r["knobs"]}
        old_variant, old_status = ops.CONV3_VARIANT, dict(status)
        _note("row", r["name"])
        try:
            for k, v in r["knobs"].items():
                setattr(autograd, k, v)
            ops.CONV3_VARIANT = r["variant"]
            status.update(r["chunks"])
            x = torch.zeros(r["x"], dtype=dtype, requires_grad=r["x_grad"])
            cout = r["linear"][0] if r["linear"] else r["cout"]
            bias = torch.zeros(cout, requires_grad=r["w_grad"]) if r["bias"] else None
            with torch.enable_grad():
                if r["linear"]:
                    y = autograd.linear_weight(x, torch.zeros(r["linear"], requires_grad=r["w_grad"]), bias)
                else:
                    weight = torch.zeros((cout, r["x"][3], r["k"], r["k"]), requires_grad=r["w_grad"])
                    y = autograd.Conv2dFn.apply(x.permute(0, 3, 1, 2), weight, bias, r["stride"], r["pad"])
                if y.requires_grad:
                    y.float().sum().backward()
        finally:
            status.clear()
            status.update(old_status)
            ops.CONV3_VARIANT = old_variant
            for k, v in old.items():
                setattr(autograd, k, v)


CASES = {}
for _mode in MODES:
    CASES["corpbevt_small.%s" % _mode] = _corpbevt(_mode)
    for _kind, _core, _agents in CVT_KINDS:
        CASES["cvt_small_%s.%s" % (_kind, _mode)] = _cvt(_kind, _core, _agents, _mode)
    CASES["nuscenes_cvt.%s" % _mode] = _nuscenes(False, _mode)
    CASES["nuscenes_sinbevt.%s" % _mode] = _nuscenes(True, _mode)
    CASES["point_pillar.%s" % _mode] = _point_pillar(_mode)
CASES["corpbevt_small_train.fp32"] = _corpbevt_train
CASES["voxelize_points"] = _voxelize
CASES["detect_post_process"] = _detect_post
CASES["conv2d_table"] = _conv2d_table
CASES["train_conv_table"] = _train_conv_table


def trace(name, setattr_, status=None):
    global _RECORDER
    rec = _RECORDER = Recorder(status)
    install(setattr_, rec)
    CASES[name]()
    return rec.records


def dumps(records):
    return "".join(json.dumps(r, separators=(",", ":")) + "\n" for r in records)


def fixture_path(name):
    return os.path.join(FIXTURES, name + ".jsonl.gz")


def read_fixture(name):
    with gzip.open(fixture_path(name), "rt") as f:
        return [json.loads(line) for line in f]


if __name__ == "__main__":
    os.makedirs(FIXTURES, exist_ok=True)
    for case in (sys.argv[1:] or sorted(CASES)):
        first = dumps(trace(case, setattr))
        if dumps(trace(case, setattr)) != first:
            raise SystemExit("%s: two runs gave different traces - mask what varies (MASKED) before committing a fixture" % case)
        with open(fixture_path(case), "wb") as f:
            f.write(gzip.compress(first.encode(), mtime=0))         # mtime=0: the same trace gives the same bytes
        print("%-40s %5d launches  %7d bytes" % (case, first.count("\n"), len(first)))
