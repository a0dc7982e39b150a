"""What tools/attn_select_fixture.py and tools/rows_select_fixture.py share when they `record`: a commit's C sources put into a scratch
directory, compiled for the HOST with attn_select_shim.hpp force-included (every kernel launch becomes a printed record), and the
resulting program run twice per environment - the two outputs must be identical.  No GPU involved."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tools", "attn_select_shim.hpp")
WORKTREE = "WORKTREE"       # --rev WORKTREE: the files as they are on disk, committed or not


def checkout(rev, tmp):
    """cobevt_amd/csrc/ and include/ of `rev` under `tmp`; returns the csrc directory there."""
    if rev == WORKTREE:
        listing = [os.path.join(d, f) for d in ("cobevt_amd/csrc", "include") for f in os.listdir(os.path.join(ROOT, d))]
    else:
        listing = subprocess.check_output(["git", "-C", ROOT, "ls-tree", "--name-only", rev, "cobevt_amd/csrc/", "include/"]).decode().split()
    for path in listing:
        if path.endswith((".hip", ".hpp", ".h")):
            dst = os.path.join(tmp, path)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            if rev == WORKTREE:
                shutil.copyfile(os.path.join(ROOT, path), dst)
            else:
                with open(dst, "wb") as f:
                    f.write(subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (rev, path)]))
    return os.path.join(tmp, "cobevt_amd", "csrc")


def build_oracle(tmp, units):
    """Compile every source of `units` host-only with the shim in front, link them into one program and return its path."""
    sys.path.insert(0, ROOT)
    from cobevt_amd.build import _hipcc
    csrc = os.path.join(tmp, "cobevt_amd", "csrc")
    objs = []
    for i, src in enumerate(units):
        objs.append(os.path.join(tmp, "unit%d.o" % i))
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "--offload-host-only", "-std=c++17", "-O1", "-Wno-pass-failed", "-x", "hip",
                               "-include", SHIM, "-I", csrc, "-I", os.path.join(ROOT, "tests"), "-c", src, "-o", objs[-1]])
    exe = os.path.join(tmp, "oracle")
    # a host-only object still names the device image it was not given: left unresolved (null), nothing here launches a kernel
    subprocess.check_call([_hipcc()] + objs + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def run_twice(exe, cases, env_prefix, env):
    """The program's output over `cases` (text on stdin) with every `env_prefix`* variable replaced by `env`; run twice, must agree."""
    e = {k: v for k, v in os.environ.items() if not k.startswith(env_prefix)}
    e.update(env)
    first = subprocess.run([exe], input=cases.encode(), stdout=subprocess.PIPE, env=e, check=True).stdout
    if subprocess.run([exe], input=cases.encode(), stdout=subprocess.PIPE, env=e, check=True).stdout != first:
        raise SystemExit("two runs of the oracle differ")
    return first.decode()
