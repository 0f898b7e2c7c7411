"""Writes tests/golden/keyframe_database/*.npz from the yardstick (tests/keyframe_database_reference.py): a few scenes of tests/keyframe_database_scenes.py with
their inputs (the ops, the neighbour lists) and the yardstick's results, so that the device test does not depend on the random generator that drew them.

    python tools/gen_golden_keyframe_database.py

pack() / unpack() are the file format; tests/test_gpu_keyframe_database.py reads the files with unpack()."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "keyframe_database")
NAMES = ("first_word_ties", "repeated_query_id", "reloc_stale_score", "reloc_unset_score", "best_keyframe_named_twice", "every_sharer_connected", "places_40")
KINDS = {"add": 0, "erase": 1, "clear": 2}      # a query: 3 + its kind


def _csr(lists, dtype):
    start = np.zeros(len(lists) + 1, np.int64)
    start[1:] = np.cumsum([len(l) for l in lists])
    flat = np.array([x for l in lists for x in l], dtype) if start[-1] else np.zeros(0, dtype)
    return start, flat


def pack(sc, results):
    ops = sc["ops"]
    empty = (np.zeros(0, np.uint32), np.zeros(0))
    kind = np.array([KINDS[op[0]] if op[0] != "query" else 3 + op[1] for op in ops], np.int8)
    ident = np.array([op[1] if op[0] in ("add", "erase") else (op[2] if op[0] == "query" else 0) for op in ops], np.uint64)
    vecs = [op[2] if op[0] == "add" else (op[3] if op[0] == "query" else empty) for op in ops]
    z = dict(n_words=np.int64(sc["n_words"]), op_kind=kind, op_id=ident, op_min_score=np.array([op[5] if op[0] == "query" else 0 for op in ops], np.float32))
    z["vec_start"], z["vec_id"] = _csr([v[0] for v in vecs], np.uint32)
    z["vec_val"] = _csr([v[1] for v in vecs], np.float64)[1]
    z["conn_start"], z["conn_id"] = _csr([op[4] if op[0] == "query" else () for op in ops], np.uint64)
    keys = sorted({op[1] for op in ops if op[0] == "add"})
    z["nb_key"] = np.array(keys, np.uint64)
    z["nb_start"], z["nb_id"] = _csr([list(sc["neighbours"](k)) for k in keys], np.uint64)
    res = [r["res"] for r in results]
    z["raw_start"], z["raw_id"] = _csr([[t[0] for t in r["raw"]] for r in results], np.uint64)
    z["raw_common"] = _csr([[t[1] for t in r["raw"]] for r in results], np.int32)[1]
    z["raw_first"] = _csr([[t[2] for t in r["raw"]] for r in results], np.uint32)[1]
    z["raw_score"] = _csr([[t[3] for t in r["raw"]] for r in results], np.float64)[1]
    z["sharing_start"], z["sharing_id"] = _csr([r["sharing_id"] for r in res], np.uint64)
    z["sharing_words"] = _csr([r["sharing_words"] for r in res], np.int32)[1]
    z["counts"] = np.array([[r["max_common_words"], r["min_common_words"], r["n_scores"], r["used_unset"]] for r in res], np.int32).reshape(-1, 4)
    z["scored_start"], z["scored_id"] = _csr([r["scored_id"] for r in res], np.uint64)
    z["scored_score"] = _csr([r["scored_score"] for r in res], np.float32)[1]
    z["acc_start"], z["acc_score"] = _csr([r["acc_score"] for r in res], np.float32)
    z["best_id"] = _csr([r["best_id"] for r in res], np.uint64)[1]
    z["cand_start"], z["cand_id"] = _csr([r["cand_id"] for r in res], np.uint64)
    return z


def unpack(z):
    """(scene, results) in the layout of keyframe_database_scenes.run"""
    def part(start, flat, i):
        return flat[int(z[start][i]):int(z[start][i + 1])]
    nb = {int(k): [int(x) for x in part("nb_start", z["nb_id"], i)] for i, k in enumerate(z["nb_key"])}
    ops = []
    for i, kind in enumerate(z["op_kind"]):
        bow = (part("vec_start", z["vec_id"], i).copy(), part("vec_start", z["vec_val"], i).copy())
        if kind == 0:
            ops.append(("add", int(z["op_id"][i]), bow))
        elif kind == 1:
            ops.append(("erase", int(z["op_id"][i])))
        elif kind == 2:
            ops.append(("clear",))
        else:
            ops.append(("query", int(kind) - 3, int(z["op_id"][i]), bow, tuple(int(c) for c in part("conn_start", z["conn_id"], i)), float(z["op_min_score"][i])))
    results = []
    for j, op in enumerate(o for o in ops if o[0] == "query"):
        raw = list(zip(*[[x.item() for x in part("raw_start", z[k], j)] for k in ("raw_id", "raw_common", "raw_first", "raw_score")]))
        c = z["counts"][j]
        res = dict(sharing_id=part("sharing_start", z["sharing_id"], j).tolist(), sharing_words=part("sharing_start", z["sharing_words"], j).tolist(),
                   max_common_words=int(c[0]), min_common_words=int(c[1]), n_scores=int(c[2]), used_unset=int(c[3]),
                   scored_id=part("scored_start", z["scored_id"], j).tolist(), scored_score=list(part("scored_start", z["scored_score"], j)),
                   acc_score=list(part("acc_start", z["acc_score"], j)), best_id=part("acc_start", z["best_id"], j).tolist(),
                   cand_id=part("cand_start", z["cand_id"], j).tolist())
        results.append(dict(op=op, raw=raw, res=res))
    return dict(n_words=int(z["n_words"]), ops=ops, neighbours=lambda k: nb.get(int(k), [])), results


def main():
    import keyframe_database_reference as Y
    import keyframe_database_scenes as SC
    os.makedirs(GOLDEN, exist_ok=True)
    for name in NAMES:
        if name == "places_40":
            sc = SC._places(77, 40, 600, 70, 4, 110, 6, erase_every=3)
        else:
            sc = SC.get(name)
        results = SC.run(sc, Y.Database(sc["n_words"]))
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **pack(sc, results))
        back_sc, back = unpack(np.load(path))
        again = SC.run(back_sc, Y.Database(back_sc["n_words"]))      # the file alone reproduces the yardstick's results
        assert [(r["raw"], r["res"]) for r in again] == [(r["raw"], r["res"]) for r in back] == [(list(map(tuple, r["raw"])), r["res"]) for r in results], name
        print("%s: %d ops, %d queries, %d bytes" % (name, len(sc["ops"]), len(results), os.path.getsize(path)))


if __name__ == "__main__":
    main()
