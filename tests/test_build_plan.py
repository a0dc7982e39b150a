"""CPU: what cobevt_amd/build.py would compile and link, checked on its dry-run plan and its dependency scan - no compiler runs.

The three libraries differ only through csrc/f32_matrix.hpp; a source is built once per library exactly when it includes that
header, every other source once, and an object depends on its own headers only."""
import os
import re

from cobevt_amd import build as b

PKG = os.path.dirname(os.path.abspath(b.__file__))
MACRO = "COBEVT_F32_SPLIT"
VARIANT = {"attention.hip", "basicblock.hip", "bottleneck_f32.hip", "conv3x3.hip", "deconv.hip", "gemm_rows.hip", "gemm_rows3_f32.hip",
           "igemm.hip", "row_chain_f32.hip", "stem7x7.hip"}


def test_variant_sources_are_those_that_include_the_header():
    assert len(b.SOURCES) == 44 and len(set(b.SOURCES)) == 44
    assert set(b.variant_sources()) == VARIANT
    # each of them directly, none through a header that library-independent sources share
    direct = {s for s in b.SOURCES if re.search(r'^\s*#\s*include\s+"%s"' % re.escape(b.VARIANT_HEADER), open(os.path.join(b.CSRC, s)).read(), re.M)}
    assert direct == VARIANT


def test_macro_is_read_by_one_header_and_set_by_the_build_flags():
    mentions = {}
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                path = os.path.join(root, f)
                text = open(path, errors="replace").read()
                if MACRO in text:
                    mentions[os.path.relpath(path, PKG)] = text
    assert set(mentions) == {os.path.join("csrc", b.VARIANT_HEADER), "build.py"}
    text = mentions["build.py"]
    assert text.count(MACRO) == text.count("-D" + MACRO + "=") == 2        # the two -D flags, nothing else


def test_plan_compiles_shared_sources_once_and_variant_sources_per_library():
    jobs, links = b.plan(force=True)
    assert len(jobs) == 64 and len({o for _, o, _ in jobs}) == 64
    assert not any(MACRO in f for f in b.FLAGS)
    by_src = {}
    for src, o, flags in jobs:
        assert flags[:len(b.FLAGS)] == b.FLAGS
        by_src.setdefault(src, []).append((o, flags[len(b.FLAGS):]))
    assert set(by_src) == set(b.SOURCES)
    for src, built in by_src.items():
        name = src.replace(".hip", ".o")
        if src in VARIANT:
            assert built == [(os.path.join(b.CSRC, name), []),
                             (os.path.join(b.CSRC, "f32s", name), ["-DCOBEVT_F32_SPLIT=1"]),
                             (os.path.join(b.CSRC, "f32h", name), ["-DCOBEVT_F32_SPLIT=2"])]
        else:
            assert built == [(os.path.join(b.CSRC, name), [])]

    assert [lib for lib, _ in links] == [b.LIB, b.LIB_F32S, b.LIB_F32H]
    built = {o for _, o, _ in jobs}
    for (lib, objs), sub in zip(links, ("", "f32s", "f32h")):
        assert len(objs) == 44 and set(objs) <= built
        for src, o in zip(b.SOURCES, objs):                                    # SOURCES order, an explicit path per source
            assert o == os.path.join(b.CSRC, sub if src in VARIANT else "", src.replace(".hip", ".o"))
    shared = [[o for src, o in zip(b.SOURCES, objs) if src not in VARIANT] for _, objs in links]
    assert len(shared[0]) == 34 and shared[0] == shared[1] == shared[2]


def _stub_tree(tmp_path):
    """The csrc tree reduced to its #include lines, every file at time 1000 and an object per source at time 2000."""
    objs = {}
    for f in os.listdir(b.CSRC):
        if f.endswith((".hip", ".hpp")):
            lines = [ln for ln in open(os.path.join(b.CSRC, f)).read().split("\n") if re.match(r"\s*#\s*include", ln)]
            (tmp_path / f).write_text("\n".join(lines) + "\n")
            os.utime(tmp_path / f, (1000, 1000))
    for src in b.SOURCES:
        objs[src] = tmp_path / src.replace(".hip", ".o")
        objs[src].write_text("")
        os.utime(objs[src], (2000, 2000))
    return objs


def _stale_after_touching(tmp_path, objs, header):
    os.utime(tmp_path / header, (3000, 3000))
    stale = {src for src in b.SOURCES if b._stale(str(objs[src]), b.deps(src, str(tmp_path)))}
    os.utime(tmp_path / header, (1000, 1000))
    return stale


def test_an_object_is_stale_only_when_one_of_its_own_headers_is_newer(tmp_path):
    objs = _stub_tree(tmp_path)
    assert not any(b._stale(str(objs[src]), b.deps(src, str(tmp_path))) for src in b.SOURCES)
    assert _stale_after_touching(tmp_path, objs, "attn_common.hpp") == {"attention.hip", "attention_resident.hip", "attention_bwd.hip", "swap_stage.hip"}
    assert _stale_after_touching(tmp_path, objs, "pillar_common.hpp") == {"pillar_vfe.hip", "train_pillar.hip"}
    assert _stale_after_touching(tmp_path, objs, b.VARIANT_HEADER) == VARIANT
    assert _stale_after_touching(tmp_path, objs, "common.hpp") == set(b.SOURCES)
    assert _stale_after_touching(tmp_path, objs, "points_common.hpp") == {"voxelize.hip", "bev_points.hip", "cloud_prep.hip"}
    assert _stale_after_touching(tmp_path, objs, "detect_common.hpp") == {"detect_post.hip", "detect_targets.hip", "bev_labels.hip"}
    os.utime(tmp_path / "sparse_conv.hip", (3000, 3000))                       # ... or its source
    assert {src for src in b.SOURCES if b._stale(str(objs[src]), b.deps(src, str(tmp_path)))} == {"sparse_conv.hip"}


def test_a_header_is_shared_and_included_at_the_head_of_a_file():
    """A kernel family lives in a source of its own: a header holds only what at least two sources need, and no source pulls a
    project header in below its first declaration, where what it compiles would depend on the lines above it."""
    closures = {src: b.include_closure(src) for src in b.SOURCES}
    assert sorted(f for f in os.listdir(b.CSRC) if f.endswith(".hip")) == sorted(b.SOURCES)
    for hpp in sorted(f for f in os.listdir(b.CSRC) if f.endswith(".hpp")):
        users = [src for src in b.SOURCES if hpp in closures[src]]
        assert len(users) >= 2, (hpp, users)
    for src in b.SOURCES:
        body = open(os.path.join(b.CSRC, src)).read().partition("namespace cobevt {")[2]     # empty for a source without the namespace
        assert not re.findall(r'^\s*#\s*include\s+"', body, re.M), src
