"""The numeric steps of Object_Map::DataAssociateUpdate (reference src/Object.cc:1352-1601) chained in one device call -- the point update, the erase of the bad
points, the cuboid and the isolation forest -- through eao_object_update_chain_batch / eao_object_update_chain (csrc/object_chain.hip): the ctypes mirror the
tests and tools/bench_object_chain.py use.

A desc is a dict: the keys of an object_points desc, and map_bad (n_map) and cand_bad (n_cand) uint8 (zeros where missing), cand_alias (n_cand int32, optional),
centroids (m, 3) float32, Ryaw (9,) float32 (the identity where missing), prev_cuboid_center (3,) float64, class_id, bi_forest (1 where missing)."""
import ctypes as C

import numpy as np

from . import _lib, object_cuboid, object_points

FOREST_SKIPPED, FOREST_DONE, FOREST_FAILED = 0, 1, 2
KERNELS = ("k_object_points_match", "k_object_points", "k_object_chain_plan", "k_object_cuboids", "k_iforest_build", "k_iforest_score")

# eao_object_chain_rec (include/eao_fusion.h), field by field
RECORD_DTYPE = np.dtype([("n_final", np.int32), ("forest_status", np.int32), ("removed", np.int32), ("reserved", np.int32)])
assert RECORD_DTYPE.itemsize == 16 == C.sizeof(_lib.ObjectChainRec)

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
_filled = object_points._filled


def lists_of(d):
    """(map_bad, cand_bad, cand_alias or None, centroids) of a desc, contiguous"""
    mp, _, cp, _ = object_points.lists_of(d)
    mb = np.ascontiguousarray(d["map_bad"] if d.get("map_bad") is not None else np.zeros(len(mp)), np.uint8).reshape(-1)
    cb = np.ascontiguousarray(d["cand_bad"] if d.get("cand_bad") is not None else np.zeros(len(cp)), np.uint8).reshape(-1)
    al = None if d.get("cand_alias") is None else np.ascontiguousarray(d["cand_alias"], np.int32).reshape(-1)
    cen = np.ascontiguousarray(d.get("centroids", np.zeros((0, 3))), np.float32).reshape(-1, 3)
    assert len(mb) == len(mp) and len(cb) == len(cp) and (al is None or len(al) == len(cp))
    return mb, cb, al, cen


def _descs(descs, fill, want_scores):
    keep, cd, co = [], (_lib.ObjectChainDesc * max(len(descs), 1))(), (_lib.ObjectChainOut * max(len(descs), 1))()
    for k, d in enumerate(descs):
        pts = object_points.fill_desc(cd[k].points, co[k].points, d, fill, False)
        mb, cb, al, cen = lists_of(d)
        n = len(mb) + len(cb)
        null = d.get("null", ())
        c = cd[k]
        c.map_bad = _lib.ptr(mb) if len(mb) and "map_bad" not in null else None
        c.cand_bad = _lib.ptr(cb) if len(cb) and "cand_bad" not in null else None
        c.cand_alias = _lib.ptr(al) if al is not None and len(al) else None
        c.n_centroids = d.get("n_centroids", len(cen))
        c.centroids = _lib.ptr(cen) if len(cen) and "centroids" not in null else None
        c.Ryaw = (C.c_float * 9)(*np.asarray(d.get("Ryaw", IDENTITY), np.float32).reshape(9).tolist())
        c.prev_cuboid_center = (C.c_double * 3)(*np.asarray(d.get("prev_cuboid_center", np.zeros(3)), np.float64).reshape(3).tolist())
        c.class_id, c.bi_forest = int(d.get("class_id", 0)), int(d.get("bi_forest", 1))
        out = dict(pts[4], chain=_filled(1, RECORD_DTYPE, fill), final=_filled(2 * max(n, 1), np.int32, fill), cuboid=_filled(1, object_cuboid.RECORD_DTYPE, fill),
                   forest_flags=_filled(max(n, 1), np.uint8, fill), scores=_filled(max(n, 1), np.float64, fill) if want_scores else None)
        for f, key in (("rec", "chain"), ("final", "final"), ("cuboid", "cuboid"), ("forest_flags", "forest_flags"), ("scores", "scores")):
            setattr(co[k], f, None if key in null else _lib.ptr(out[key]))
        keep.append((pts, mb, cb, al, cen, out))
    return keep, cd, co


def update_raw(descs, single=False, fill=0, n=None, want_scores=True):
    """(status, [the output buffers of each desc as the call left them, pre-filled with `fill` bytes])"""
    keep, cd, co = _descs(descs, fill, want_scores)
    L = _lib.load()
    st = L.eao_object_update_chain(cd, co) if single else L.eao_object_update_chain_batch(len(descs) if n is None else n, cd, co)
    return st, [k[5] for k in keep]


def trim(desc, out):
    """the written part of a desc's output buffers: what object_points.trim gives (without the positions), and with status DONE chain (a RECORD_DTYPE record),
    final (n_final, 2), cuboid (a record), forest_flags and scores (n_final)"""
    res = object_points.trim(desc, out)
    if res["rec"]["status"] != object_points.DONE:
        return res
    ch = out["chain"][0]
    nf = int(ch["n_final"])
    res.update(chain=ch, final=out["final"][:2 * nf].reshape(-1, 2), cuboid=out["cuboid"][0], forest_flags=out["forest_flags"][:nf])
    if out["scores"] is not None:
        res["scores"] = out["scores"][:nf]
    return res


def update_batch(descs):
    """One library call for all descs: a list of trim()med results."""
    st, outs = update_raw(descs)
    _lib.check(st)
    return [trim(d, o) for d, o in zip(descs, outs)]


def update(desc):
    """One desc through eao_object_update_chain."""
    st, outs = update_raw([desc], single=True)
    _lib.check(st)
    return trim(desc, outs[0])


def set_profiling(on):
    _lib.check(_lib.load().eao_object_chain_set_profiling(1 if on else 0))


def last_kernel_ms():
    """Device time of the chain's kernels (KERNELS) in this thread's last call (after set_profiling(True)); -1 where not measured."""
    ms = (C.c_float * len(KERNELS))()
    _lib.check(_lib.load().eao_object_chain_last_kernel_ms(ms))
    return tuple(float(v) for v in ms)
