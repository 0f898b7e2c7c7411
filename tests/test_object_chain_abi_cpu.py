"""The object-chain entry points at the drop-in boundary, without a device: the header declares them, the shared object exports them, the ctypes table binds
them, the three structs have in C the layout the ctypes mirror and the numpy record assume (a C program prints its offsets), the header's constants are the
Python mirror's, every refusal comes before the device is asked for and leaves the outputs untouched, and nothing is computed without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eao_object_update_chain_batch", "eao_object_update_chain", "eao_object_chain_set_profiling", "eao_object_chain_last_kernel_ms"]
DESC = ["points", "map_bad", "cand_bad", "cand_alias", "n_centroids", "class_id", "centroids", "Ryaw", "bi_forest", "prev_cuboid_center"]
RECORD = ["n_final", "forest_status", "removed", "reserved"]
OUT = ["points", "rec", "final", "cuboid", "forest_flags", "scores"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eao_fusion_amd", "csrc")])
    from eao_fusion_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eao_fusion.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(eao_object_(?:update_)?chain[a-z0-9_]*)\s*\(", hdr)) == set(NAMES)
    L = built.load()
    for name in NAMES:
        assert hasattr(L, name) and built.SYMBOLS[name] is not None, name
    assert "object_chain.hip" in open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "Makefile")).read()


def test_record_layouts_c_against_ctypes(built, tmp_path):
    src = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", "#include <eao_fusion.h>", "int main(void) {"]
    for struct, fields in (("eao_object_chain_desc", DESC), ("eao_object_chain_rec", RECORD), ("eao_object_chain_out", OUT)):
        lines.append('    printf("%s %%zu", sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('    printf(" %s:%%zu:%%zu", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (f, struct, f, struct, f))
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])      # (the header is C)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for line, (ct, fields) in zip(got, ((built.ObjectChainDesc, DESC), (built.ObjectChainRec, RECORD), (built.ObjectChainOut, OUT))):
        assert [f for f, _ in ct._fields_] == fields
        want = "%s %d" % (line.split()[0], C.sizeof(ct)) + "".join(" %s:%d:%d" % (f, getattr(ct, f).offset, getattr(ct, f).size) for f in fields)
        assert line == want
    from eao_fusion_amd import object_chain
    assert object_chain.RECORD_DTYPE.itemsize == C.sizeof(built.ObjectChainRec) == 16
    assert [object_chain.RECORD_DTYPE.fields[f][1] for f in RECORD] == [getattr(built.ObjectChainRec, f).offset for f in RECORD]
    import object_chain_reference as Y
    assert Y.RECORD_DTYPE == object_chain.RECORD_DTYPE


def test_constants(built):
    from eao_fusion_amd import object_chain as P
    import object_chain_reference as Y
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    for name, value in (("SKIPPED", P.FOREST_SKIPPED), ("DONE", P.FOREST_DONE), ("FAILED", P.FOREST_FAILED)):
        assert "#define EAO_OBJECT_CHAIN_FOREST_%s %d\n" % (name, value) in hdr, name
        assert getattr(Y, "FOREST_" + name) == value
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_chain_internal.h")).read()
    assert "constexpr int kKernels = %d;" % len(P.KERNELS) in h


def untouched(outs):
    return all(set(np.ascontiguousarray(a).tobytes()) <= {0xAB} for o in outs for a in o.values() if a is not None)


def refusals():
    """(descs, keyword arguments of update_raw) of every refusal that is decided before the device: what the three entries refuse and what the chain adds"""
    import object_chain_scenes as SC
    scenes = SC.scenes()
    base, good = scenes["n_final_31"], scenes["bad_point_first"]

    def edit(key, at, value):
        o = dict(base)
        o[key] = np.array(base[key], np.float64)
        o[key][at] = value
        return o

    n_map = len(base["map_points"])
    wide = dict(scenes["n_final_30"], n_map=65530, n_cand=6)      # the forest may run and the bound exceeds EAO_IFOREST_MAX_POINTS (the counts alone decide)
    bad = [edit("map_points", (5, 2), np.nan), edit("cand_points", (0, 0), np.inf), edit("center", 1, np.nan), edit("sum_pos", 0, -np.inf),
           dict(base, Tcw=[np.inf] + [0.0] * 15), dict(base, fy=np.nan), dict(base, cx=np.inf), dict(base, rmax=np.nan), dict(base, lenth=np.inf), dict(base, width=np.nan),
           dict(base, pose_q=[np.nan, 0, 0, 1]), dict(base, pose_t=[0, 0, np.inf]), dict(base, cuboid_center=[0, np.nan, 0]), dict(base, bounds=[0, 1, 0, 1, np.nan, 1]),
           dict(base, overlap=[0, np.inf, 0]), dict(base, gate=3), dict(base, gate=-1), dict(base, erase=4), dict(base, cols=-1), dict(base, rows=1 << 16),
           dict(base, box_rect=[0, 0, -1, 1]), dict(base, project_rect1=[-(1 << 16), 0, 1, 1]), dict(base, n_map=-1), dict(base, n_cand=-7),
           dict(base, null=("map_points",)), dict(base, null=("map_count",)), dict(base, null=("cand_points",)), dict(base, null=("cand_count",)),
           dict(base, null=("rec",)), dict(base, null=("gate",)), dict(base, null=("target",)), dict(base, null=("count",)), dict(base, null=("list",)),
           dict(base, null=("erased",)), dict(base, null=("survivors",)),
           # the cuboid's
           edit("centroids", (1, 1), np.nan), edit("Ryaw", 4, np.inf), edit("prev_cuboid_center", 2, np.nan), dict(base, n_centroids=-1), dict(base, null=("centroids",)),
           # the chain's own
           dict(base, null=("map_bad",)), dict(base, null=("cand_bad",)), dict(base, null=("chain",)), dict(base, null=("final",)), dict(base, null=("cuboid",)),
           dict(base, null=("forest_flags",)), dict(base, cand_alias=np.full(len(base["cand_points"]), n_map, np.int32)),
           dict(base, cand_alias=np.full(len(base["cand_points"]), -2, np.int32)), wide]
    cases = [([good, b], {}) for b in bad[::2]] + [([b, good], {}) for b in bad[1::2]]
    return cases + [([good], dict(n=-1)), ([good], dict(n=65536))]


def test_arguments_are_checked_before_the_device_is_asked_for(built):
    from eao_fusion_amd import object_chain
    for descs, kw in refusals():
        st, outs = object_chain.update_raw(descs, fill=0xAB, **kw)
        assert st == built.EAO_ERR_INVALID and untouched(outs), (kw, built.load().eao_last_error())
    L = built.load()
    assert L.eao_object_update_chain(None, C.byref(built.ObjectChainOut())) == built.EAO_ERR_INVALID
    assert L.eao_object_update_chain(C.byref(built.ObjectChainDesc()), None) == built.EAO_ERR_INVALID
    assert L.eao_object_update_chain_batch(1, None, C.byref(built.ObjectChainOut())) == built.EAO_ERR_INVALID
    assert L.eao_object_update_chain_batch(1, C.byref(built.ObjectChainDesc()), None) == built.EAO_ERR_INVALID
    assert L.eao_object_update_chain_batch(0, None, None) == built.EAO_OK      # no descs: no device work
    assert L.eao_object_chain_last_kernel_ms(None) == built.EAO_ERR_INVALID
    import object_chain_scenes as SC
    S = SC.scenes()
    # the bound's refusal names the forest; the same counts on a desc whose forest cannot run are no refusal of the bound
    wide = dict(S["n_final_30"], n_map=65530, n_cand=6)
    st, outs = object_chain.update_raw([wide], fill=0xAB)
    assert st == built.EAO_ERR_INVALID and untouched(outs) and b"EAO_IFOREST_MAX_POINTS" in L.eao_last_error()
    # an optional output or input that is NULL is no refusal
    st, _ = object_chain.update_raw([S["alias_null_erases"]], fill=0xAB, want_scores=False)
    assert st != built.EAO_ERR_INVALID


def test_nothing_is_computed_without_a_device(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import object_chain_scenes as SC
    from eao_fusion_amd import object_chain
    st, outs = object_chain.update_raw([SC.scenes()["n_final_31"]], fill=0xAB)
    assert st == built.EAO_ERR_NO_DEVICE and untouched(outs)
    ms = (C.c_float * 6)()
    assert built.load().eao_object_chain_last_kernel_ms(ms) == built.EAO_ERR_INVALID
