"""Build libcobevt_hip.so, libcobevt_hip_f32s.so and libcobevt_hip_f32h.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

`python -m cobevt_amd.build` or `__graft_entry__.build()`.

The three libraries export the same C ABI from the same SOURCES and differ in one thing: what an fp32-storage matrix product
becomes.  csrc/f32_matrix.hpp is the only file that says so, and the include graph says which kernels that reaches:
  * a VARIANT source has f32_matrix.hpp in its include closure.  It is compiled three times - natively into csrc/, with the
    second library's -D flag into csrc/f32s/ (two split-bf16 MFMAs per 16-byte piece instead of four v_mfma_f32_32x32x2_f32: the
    "fp32_split" compute mode of host.set_compute_dtype) and with the third's into csrc/f32h/ (ONE fp16 MFMA, the weight operand
    as a single fp16 term: the ResNet encoder's library under "fp32_fast");
  * every other source is SHARED: compiled once into csrc/, without any such flag, and that one object is linked into all three.
Nothing lists the variant sources: variant_sources() derives them from the #include lines (ten of the 44 at present, so a clean
build is 34 + 3 x 10 = 64 hipcc runs), and tests/test_build_plan.py pins the set.

An object is rebuilt when its source or a header in ITS OWN include closure is newer.  Each library links an explicit object
list in SOURCES order, never a directory's contents.  plan() returns all of this without running the compiler.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libcobevt_hip.so")
LIB_F32S = os.path.join(CSRC, "libcobevt_hip_f32s.so")
LIB_F32H = os.path.join(CSRC, "libcobevt_hip_f32h.so")
SOURCES = ["igemm.hip", "conv3x3.hip", "basicblock.hip", "bottleneck.hip", "bottleneck_f32.hip", "gemm_rows.hip", "gemm_rows3.hip", "gemm_rows3_f32.hip", "bev_query.hip", "row_chain.hip", "row_chain_f32.hip", "row_chain64.hip", "ln_linear64.hip", "proj_chain128.hip", "proj_chain_k.hip", "swap_stage.hip", "stem7x7.hip", "attention.hip", "attention_resident.hip", "attention_bwd.hip", "train_rows.hip", "train_glue.hip", "train_prep.hip", "wgrad3.hip", "train_nusc.hip", "train_fax.hip", "elementwise.hip", "pairwise_fusion.hip", "postprocess.hip", "depthwise.hip", "peer_gather.hip", "calibrate.hip", "pillar_vfe.hip", "train_pillar.hip", "voxelize.hip", "detect_post.hip", "sparse_conv.hip", "cloud_prep.hip", "bev_points.hip", "detect_targets.hip", "bev_labels.hip", "image_ingest.hip", "deconv.hip", "att_fuse.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed"]
MAX_JOBS = 16  # hipcc processes at a time

VARIANT_HEADER = "f32_matrix.hpp"
# (library, object subdirectory of csrc/ for the variant sources, their extra flags); the native library first: its objects are the shared ones
LIBRARIES = [(LIB, "", []), (LIB_F32S, "f32s", ["-DCOBEVT_F32_SPLIT=1"]), (LIB_F32H, "f32h", ["-DCOBEVT_F32_SPLIT=2"])]

_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.sep not in cand or os.path.exists(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def include_closure(name, csrc=CSRC):
    """The files of `csrc` that `name` includes with #include "...", transitively (names relative to `csrc`, without `name` itself)."""
    seen, todo = [], [name]
    while todo:
        with open(os.path.join(csrc, todo.pop())) as f:
            for inc in _INCLUDE.findall(f.read()):
                if inc not in seen and os.path.exists(os.path.join(csrc, inc)):
                    seen.append(inc)
                    todo.append(inc)
    return seen


def variant_sources(csrc=CSRC):
    """The sources that are compiled once per library: those whose include closure contains VARIANT_HEADER."""
    return [s for s in SOURCES if VARIANT_HEADER in include_closure(s, csrc)]


def deps(src, csrc=CSRC):
    """What the object of `src` is made from: the source and its own headers, as paths."""
    return [os.path.join(csrc, n) for n in [src] + include_closure(src, csrc)]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _obj(objdir, src):
    return os.path.join(objdir, src.replace(".hip", ".o"))


def plan(force=False):
    """The build without running it: (jobs, links).  jobs = [(source, object path, flags)], one per stale object (every object
    with `force`); links = [(library, its objects in SOURCES order)] for the three libraries."""
    variant = set(variant_sources())
    jobs, links = {}, []          # jobs by object path: a shared object is asked for by all three libraries and built once
    for lib, sub, extra in LIBRARIES:
        objs = []
        for src in SOURCES:
            objdir, flags = (os.path.join(CSRC, sub), FLAGS + extra) if src in variant else (CSRC, FLAGS)
            o = _obj(objdir, src)
            objs.append(o)
            if force or _stale(o, deps(src)):
                jobs[o] = (src, o, flags)
        links.append((lib, objs))
    return list(jobs.values()), links


def _compile(jobs, verbose):
    """Run the (source, object path, flags) jobs, MAX_JOBS at a time."""
    hipcc = _hipcc()

    def run(job):
        src, o, flags = job
        os.makedirs(os.path.dirname(o), exist_ok=True)
        cmd = [hipcc] + flags + ["-c", os.path.join(CSRC, src), "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)

    with ThreadPoolExecutor(MAX_JOBS) as pool:
        for (src, _, _), p in zip(jobs, list(pool.map(run, jobs))):
            if p.returncode != 0:
                raise RuntimeError("hipcc failed for %s:\n%s" % (src, p.stdout.decode(errors="replace")))


def compile_objects(objdir, extra, force, verbose):
    """Compile ALL the sources with the `extra` flags into `objdir` - those whose object there is stale, or every one with `force` -
    and return the object paths in SOURCES order.  Not used by build(): this is for whole-library A/B builds (tools/build_variant.py)."""
    objs = [_obj(objdir, src) for src in SOURCES]
    _compile([(src, o, FLAGS + extra) for src, o in zip(SOURCES, objs) if force or _stale(o, deps(src))], verbose)
    return objs


def build(force=False, verbose=True):
    jobs, links = plan(force)
    _compile(jobs, verbose)
    for lib, objs in links:
        if force or _stale(lib, objs):
            cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
