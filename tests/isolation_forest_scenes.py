"""Seeded point sets for Object_Map::IsolationForestDeleteOutliers (reference src/Object.cc:1239-1348, include/isolation_forest.h).  Each scene is the smallest
at which the branch it is named for can still go wrong; tools/gen_golden_isolation_forest.py runs the reference's own header on them and records
tests/golden/isolation_forest/<scene>.npz.  `entry` says which C-ABI entry the scene goes through: "object" = upstream's rule (50 trees, seed 12345, N / 2) via
eao_object_iforest_outliers_batch and the general entry alike, "general" = eao_iforest_scores_batch only."""
import numpy as np

TREE_COUNT, SEED = 50, 12345      # src/Object.cc:1296 (held to the reference text by tests/golden/isolation_forest_constants.json)
# the largest forest whose per-tree working set the build kernel keeps in LDS, and the first that goes through the global workspace
# (csrc/iforest_internal.h lds_plan; the CPU test holds these two to the header's budget)
LDS_EDGE_N, GLOBAL_PATH_N = 3712, 3713


def _cloud(n, seed, far_frac=0.1):
    """a Gaussian cloud (sigma 0.1 around a point a few metres out) with planted far points"""
    rs = np.random.RandomState(seed)
    centre = rs.uniform(-3.0, 3.0, 3)
    p = centre + rs.normal(0.0, 0.1, (n, 3))
    far = max(2, int(round(n * far_frac)))
    idx = rs.choice(n, far, replace=False)
    p[idx] = centre + rs.normal(0.0, 1.0, (far, 3)) * rs.uniform(1.0, 3.0, (far, 1))
    return np.ascontiguousarray(p, np.float32)


def _obj(points, class_id=0, **kw):
    n = len(points)
    return dict(points=np.ascontiguousarray(points, np.float32), tree_count=TREE_COUNT, seed=SEED, sample_size=n // 2, class_id=class_id, entry="object", **kw)


def _gen(points, tree_count, seed, sample_size, **kw):
    return dict(points=np.ascontiguousarray(points, np.float32), tree_count=tree_count, seed=seed, sample_size=sample_size, class_id=0, entry="general", **kw)


def _adjacent(n, seed):
    rs = np.random.RandomState(seed)
    lo = np.float32(1.0e6)
    hi = np.nextafter(lo, np.float32(2.0e6))
    return np.where(rs.randint(0, 2, (n, 3)) == 1, hi, lo).astype(np.float32)


def _four_ulps(n, seed):
    rs = np.random.RandomState(seed)
    base = np.float32(1.0).view(np.uint32)
    return (base + rs.randint(0, 5, (n, 3)).astype(np.uint32)).astype(np.uint32).view(np.float32)


def _flat_y(n, seed):
    p = _cloud(n, seed)
    p[:, 1] = np.float32(0.25)
    return p


def _lattice():
    g = np.arange(4, dtype=np.float32) * np.float32(0.5)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _dup_pairs(seed):
    p = _cloud(25, seed)
    return np.concatenate([p, p])[np.random.RandomState(seed + 1).permutation(50)]


def scenes():
    s = {}
    for i, n in enumerate((30, 31, 64, 65, 128, 129, 300)):
        s["gauss_%d" % n] = _obj(_cloud(n, 100 + i))
    s["adjacent"] = _obj(_adjacent(48, 201))
    s["four_ulps"] = _obj(_four_ulps(64, 202))
    s["flat_y"] = _obj(_flat_y(60, 203))
    s["all_same"] = _obj(np.tile(np.array([[0.5, -1.25, 2.0]], np.float32), (40, 1)))
    s["lattice"] = _obj(_lattice())
    s["dup_pairs"] = _obj(_dup_pairs(204))
    s["class62_60"] = _obj(_cloud(60, 205, far_frac=0.2), class_id=62)
    s["sample_eq_n"] = _gen(_cloud(40, 301), 7, 99, 40)
    s["sample_2"] = _gen(_cloud(40, 302), 7, 4242, 2)
    s["sample_1"] = _gen(_cloud(40, 303), 5, 1, 1)
    s["n2000"] = _obj(_cloud(2000, 401, far_frac=0.05), by_hash=True)
    # the two sides of the LDS budget of the build kernel: 3 trees keep the replay cheap; the stream is held by hash
    s["lds_edge"] = _gen(_cloud(LDS_EDGE_N, 402, far_frac=0.02), 3, 777, LDS_EDGE_N, by_hash=True)
    s["global_path"] = _gen(_cloud(GLOBAL_PATH_N, 403, far_frac=0.02), 3, 778, GLOBAL_PATH_N, by_hash=True)
    return s


def mixed_batch():
    """Objects of one eao_object_iforest_outliers_batch call: (points, class_id, scene whose fixture holds its scores or None when the rules skip it)."""
    s = scenes()
    nan_obj = _cloud(35, 501)
    nan_obj[17, 2] = np.nan
    return [
        (_cloud(29, 502), 0, None),                                   # below the 30-point rule
        (s["gauss_30"]["points"], 0, "gauss_30"),
        (_cloud(40, 503), 75, None),                                  # an exempt class
        (s["gauss_300"]["points"], 0, "gauss_300"),
        (s["class62_60"]["points"], 62, "class62_60"),                # th = 0.65f
        (nan_obj, 0, "refused"),                                      # a NaN coordinate: EAO_ERR_INVALID
    ]
