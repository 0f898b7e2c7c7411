"""The yardstick of the chained update of a map object (csrc/object_chain.hip): the composition of the three yardsticks the project already has --
object_points_reference (the change gate, the append, the erase), object_cuboid_reference (ComputeMeanAndStandard with UpdateObjPose) and
isolation_forest_reference (IsolationForestDeleteOutliers) -- in the order of Object_Map::DataAssociateUpdate (reference src/Object.cc:1352-1601).  What is
written here is only what lies between them, in upstream's literal form:

    the alias rule        a list entry that is the very MapPoint of a gated-in candidate shares its object_id_vector with it: step 3 raises the counter
                          (:1492-1502) before step 4 reads it (:1550-1559)
    the bad-point erase   ComputeMeanAndStandard erases the points whose isBad() holds while it iterates (:1003-1024)

A chain desc is an object_points desc with map_bad, cand_bad, cand_alias, centroids, Ryaw, prev_cuboid_center, class_id and bi_forest."""
import numpy as np

import isolation_forest_reference as IF
import object_cuboid_reference as OC
import object_points_reference as OP

f32, f64 = np.float32, np.float64
FOREST_SKIPPED, FOREST_DONE, FOREST_FAILED = 0, 1, 2
RECORD_DTYPE = np.dtype([("n_final", np.int32), ("forest_status", np.int32), ("removed", np.int32), ("reserved", np.int32)])
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], f32)


def bad_flags(desc):
    d = OP.full(desc)
    mb = np.zeros(len(d["map_points"]), np.uint8) if desc.get("map_bad") is None else np.ascontiguousarray(desc["map_bad"], np.uint8).reshape(-1)
    cb = np.zeros(len(d["cand_points"]), np.uint8) if desc.get("cand_bad") is None else np.ascontiguousarray(desc["cand_bad"], np.uint8).reshape(-1)
    assert len(mb) == len(d["map_points"]) and len(cb) == len(d["cand_points"])
    return mb, cb


def raised_counts(desc):
    """map_count as step 4 reads it: upstream's step 3 walks the candidates in order and raises object_id_vector[mnId] of every one its gate lets in; a candidate
    whose MapPoint is list entry k raises the counter that entry k reads"""
    d = OP.full(desc)
    counter = {("map", k): int(c) for k, c in enumerate(d["map_count"])}      # one counter per MapPoint
    alias = desc.get("cand_alias")
    if alias is not None and d["gate"] != OP.GATE_NONE:
        for j, p in enumerate(d["cand_points"]):
            if not OP.gate_of(d, p):
                continue
            if int(alias[j]) >= 0:
                counter[("map", int(alias[j]))] += 1
    return np.array([counter[("map", k)] for k in range(len(d["map_count"]))], np.int32)


def erase_bad(pairs, points, mb, cb):
    """:1003-1024: the erase while iterating"""
    lst = [(int(s), int(i), p) for (s, i), p in zip(pairs, points)]
    at = 0
    while at < len(lst):
        s, i, _ = lst[at]
        if (cb[i] if s else mb[i]):
            del lst[at]
        else:
            at += 1
    return np.array([(s, i) for s, i, _ in lst], np.int32).reshape(-1, 2), np.array([p for _, _, p in lst], f32).reshape(-1, 3)


def forest_of(points, class_id, bi_forest, planted_failure=False):
    """(status, flags, removed, scores) of IsolationForestDeleteOutliers over the final list"""
    n = len(points)
    flags, scores = np.zeros(n, np.uint8), np.full(n, -1.0, f64)
    if not IF.object_runs(bi_forest, class_id, n):
        return FOREST_SKIPPED, flags, 0, scores
    try:
        if planted_failure:
            raise IF.BuildFailed()
        _, sc, _ = IF.forest(points, IF.TREE_COUNT, IF.SEED, n // IF.SAMPLE_DIVISOR)
    except IF.BuildFailed:
        return FOREST_FAILED, flags, 0, scores
    flags = IF.outlier_flags(sc, class_id)
    return FOREST_DONE, flags, int(flags.sum()), np.asarray(sc, f64)


def chain(desc, form="literal"):
    """every output of eao_object_update_chain for one desc.  form: which of the points' and the cuboid's two forms runs (`literal` or `device`)"""
    pd = dict(desc, map_count=raised_counts(desc))
    res = (OP.literal if form == "literal" else OP.device)(pd)
    if int(res["rec"]["status"]) != OP.DONE:
        return res
    mb, cb = bad_flags(desc)
    final, pts = erase_bad(res["survivors"], res["points"], mb, cb)
    del res["points"]
    obj = dict(points=pts, centroids=np.ascontiguousarray(desc.get("centroids", np.zeros((0, 3))), f32).reshape(-1, 3), Ryaw=np.asarray(desc.get("Ryaw", IDENTITY), f32),
               prev_cuboid_center=np.asarray(desc.get("prev_cuboid_center", np.zeros(3)), f64))
    res["final"] = final
    res["cuboid"] = (OC.literal if form == "literal" else OC.device)(obj)
    rec = np.zeros((), RECORD_DTYPE)
    rec["n_final"] = len(final)
    st, flags, removed, scores = forest_of(pts, int(desc.get("class_id", 0)), int(desc.get("bi_forest", 1)))
    rec["forest_status"], rec["removed"] = st, removed
    res["forest_flags"], res["scores"] = flags, scores
    res["chain"] = rec
    return res


def differences(a, b):
    """the names of the outputs in which two results differ"""
    bad = [] if OP.same_record(a["rec"], b["rec"]) else ["rec"]
    if set(a) != set(b):
        return bad + ["keys"]
    for k in a:
        if k == "rec":
            continue
        if k == "cuboid":
            ok = OC.same_records(a[k], b[k])
        elif k == "chain":
            ok = all(int(a[k][f]) == int(b[k][f]) for f in RECORD_DTYPE.names)
        elif k == "scores":
            ok = OP.same_float(np.asarray(a[k], f64), np.asarray(b[k], f64))
        else:
            ok = np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(a[k], b[k])
        if not ok:
            bad.append(k)
    return bad


# ---- tools/object_chain_walk.cpp: its script and the tokens it prints

def final_object(desc, res):
    """the object the cuboid of a result saw"""
    mp, cp = OP.full(desc)["map_points"], OP.full(desc)["cand_points"]
    pts = np.array([cp[i] if s else mp[i] for s, i in res["final"]], f32).reshape(-1, 3)
    return dict(points=pts, centroids=np.ascontiguousarray(desc.get("centroids", np.zeros((0, 3))), f32).reshape(-1, 3), Ryaw=np.asarray(desc.get("Ryaw", IDENTITY), f32),
                prev_cuboid_center=np.asarray(desc.get("prev_cuboid_center", np.zeros(3)), f64))


def walk_script(desc, verb="chain", planted_failure=False):
    mb, cb = bad_flags(desc)
    alias = desc.get("cand_alias")
    cen = np.ascontiguousarray(desc.get("centroids", np.zeros((0, 3))), f32).reshape(-1, 3)
    parts = [OP.walk_script(desc, verb).strip(), str(int(desc.get("class_id", 0))), str(int(desc.get("bi_forest", 1))), str(int(planted_failure)),
             str(int(alias is not None)), str(len(cen)), OP._h32(np.asarray(desc.get("Ryaw", IDENTITY), f32)), OP._h64(np.asarray(desc.get("prev_cuboid_center", np.zeros(3)), f64)),
             OP._h32(cen), OP._ints(mb), OP._ints(cb), OP._ints(alias) if alias is not None else ""]
    return " ".join(p for p in parts if p) + "\n"


def walk_tokens(desc, res, drop=()):
    """a result as the program prints it, token by token (a NaN as `nan`, the zeros of the cuboid's fields in `drop` without their signs)"""
    out = OP.walk_line(dict(res, points=np.zeros((0, 3), f32))).split()
    if int(res["rec"]["status"]) != OP.DONE:
        return out
    ch = res["chain"]
    out += ["|"] + OP._ints(res["final"]).split() + ["||"] + OC.walk_line(res["cuboid"], drop).split()
    out += ["||", str(int(ch["n_final"])), str(int(ch["forest_status"])), str(int(ch["removed"])), "|"] + OP._ints(res["forest_flags"]).split() + ["|"]
    return out + ["nan" if np.isnan(x) else "%016x" % b for x, b in zip(res["scores"], OP._bits(np.asarray(res["scores"], f64)))]


def drop_tokens(tokens, drop):
    """the same dropping applied to the program's tokens"""
    if "||" not in tokens:
        return tokens
    a = tokens.index("||") + 1
    b = a + tokens[a:].index("||")
    return tokens[:a] + OC.drop_line(" ".join(tokens[a:b]), drop).split() + tokens[b:]
