"""Plain-Python yardstick of the reference's isolation forest (include/isolation_forest.h) as Object_Map::IsolationForestDeleteOutliers uses it
(src/Object.cc:1239-1348), with the libstdc++ (g++ 11) algorithms its result is defined by restated one by one:

  Mt19937                 std::mt19937 (bits/random.tcc: seeding recurrence, twist, tempering)
  uniform_int             uniform_int_distribution's downscaling branch for a 32-bit engine (bits/uniform_int_dist.h _S_nd: multiply, reject low products below
                          -range % range) and the whole-range case (one draw)
  shuffle                 std::shuffle's two-swaps-per-draw path (bits/stl_algo.h: __gen_two_uniform_ints; an even count swaps one element first)
  canonical_float         generate_canonical<float, 24> (bits/random.tcc: one draw converted to float, divided by 2^32, clamped below 1)
  uniform_real            uniform_real_distribution<float>: u * (b - a) + a, rounded operation by operation

The build comes twice: build_tree_sorted follows Node::Build (:165-224) literally, sort included; build_tree is the sort-free form the device uses (minimum, maximum,
partition).  Both emit the preorder node records of Node::Serialize.  tests/test_isolation_forest_reference_cpu.py holds both to the recorded streams of the
reference's own header, byte for byte."""
import math
import struct

import numpy as np

F32 = np.float32
EULER = 0.5772156649      # include/isolation_forest.h:99


class Mt19937:
    N, M = 624, 397

    def __init__(self, seed):
        x = [0] * self.N
        x[0] = seed & 0xFFFFFFFF
        for i in range(1, self.N):
            x[i] = (1812433253 * (x[i - 1] ^ (x[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.x, self.p, self.draws = x, self.N, 0

    def _twist(self):
        x, N, M = self.x, self.N, self.M
        for k in range(N):
            y = (x[k] & 0x80000000) | (x[(k + 1) % N] & 0x7FFFFFFF)
            x[k] = x[(k + M) % N] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.p = 0

    def __call__(self):
        if self.p >= self.N:
            self._twist()
        z = self.x[self.p]
        self.p += 1
        self.draws += 1
        z ^= z >> 11
        z ^= (z << 7) & 0x9D2C5680
        z ^= (z << 15) & 0xEFC60000
        z ^= z >> 18
        return z


def uniform_int(g, a, b):
    """uniform_int_distribution<T>(a, b)(g) over an engine whose range is 2^32 - 1"""
    urange = b - a
    assert 0 <= urange <= 0xFFFFFFFF
    if urange == 0xFFFFFFFF:
        return g() + a
    rng = urange + 1
    product = g() * rng
    low = product & 0xFFFFFFFF
    if low < rng:
        threshold = ((1 << 32) - rng) % rng
        while low < threshold:
            product = g() * rng
            low = product & 0xFFFFFFFF
    return (product >> 32) + a


def shuffle(ids, g):
    n = len(ids)
    if n == 0:
        return
    assert 0xFFFFFFFF // n >= n, "libstdc++ takes its one-swap-per-draw path above 65535 elements"
    i = 1
    if n % 2 == 0:
        j = uniform_int(g, 0, 1)
        ids[i], ids[j] = ids[j], ids[i]
        i += 1
    while i != n:
        swap_range = i + 1
        x = uniform_int(g, 0, swap_range * (swap_range + 1) - 1)
        a, b = x // (swap_range + 1), x % (swap_range + 1)
        ids[i], ids[a] = ids[a], ids[i]
        i += 1
        ids[i], ids[b] = ids[b], ids[i]
        i += 1


def canonical_float(draw):
    r = F32(draw) / F32(4294967296.0)      # (uint64 -> float rounds to nearest even, as the hardware conversion does)
    return np.nextafter(F32(1), F32(0)) if r >= F32(1) else r


def uniform_real(g, a, b):
    with np.errstate(all="ignore"):
        return F32(F32(canonical_float(g()) * F32(F32(b) - F32(a))) + F32(a))


def max_depth(sample_size):
    return int(math.ceil(math.log2(sample_size)))


def tree_seeds(seed, tree_count):
    g = Mt19937(seed)
    return [uniform_int(g, 0, 0xFFFFFFFF) for _ in range(tree_count)]


def sample_ids(tree_seed, n, sample_size):
    g = Mt19937(tree_seed)
    ids = list(range(n))
    shuffle(ids, g)
    return ids[:sample_size], g


class BuildFailed(Exception):
    """Node::Build returned false: the split came out above the maximum, and the right child is an empty range (:167)"""


def build_tree_sorted(points, tree_seed, sample_size):
    """Node::Build as written: recursion, std::sort of the range, linear scan for `middle`.  Returns the preorder records [(dim, split, size)]."""
    ids, g = sample_ids(tree_seed, len(points), sample_size)
    data = [points[i] for i in ids]
    md, out = max_depth(sample_size), []

    def node(first, last, depth):
        if last < first:
            raise BuildFailed()
        rec = [0, F32(0), 0]
        out.append(rec)
        if last - first < 1 or depth >= md:
            rec[2] = last - first + 1
            return
        dim = rec[0] = uniform_int(g, 0, 2)
        data[first:last + 1] = sorted(data[first:last + 1], key=lambda p: p[dim])
        lo, hi = data[first][dim], data[last][dim]
        if lo == hi:
            rec[2] = last - first + 1
            return
        split = rec[1] = uniform_real(g, lo, hi)
        middle = first
        while middle <= last and not data[middle][dim] >= split:
            middle += 1
        if middle == first:
            rec[2] = last - first + 1
            return
        node(first, middle - 1, depth + 1)
        node(middle, last, depth + 1)

    node(0, sample_size - 1, 0)
    return [tuple(r) for r in out]


def build_tree(points, tree_seed, sample_size):
    """The sort-free form: the left child is the set of elements below the split, so minimum, maximum and a partition are enough; an explicit stack of pending
    right children, as the kernel keeps.  Returns (records, right) with right[i] the preorder index of inner node i's right child."""
    ids, g = sample_ids(tree_seed, len(points), sample_size)
    pts = np.asarray(points, F32)[ids]
    md, out, right = max_depth(sample_size), [], []
    stack = [(np.arange(sample_size), 0, -1)]
    while stack:
        idx, depth, parent = stack.pop()
        if parent >= 0:
            right[parent] = len(out)
        while True:
            me, count = len(out), len(idx)
            right.append(0)
            if count == 1 or depth >= md:
                out.append((0, F32(0), count))
                break
            dim = uniform_int(g, 0, 2)
            v = pts[idx, dim]
            lo, hi = v.min(), v.max()
            if lo == hi:
                out.append((dim, F32(0), count))
                break
            split = uniform_real(g, lo, hi)
            left = v < split
            nl = int(left.sum())
            if nl == 0:
                out.append((dim, split, count))
                break
            if nl == count:
                raise BuildFailed()
            out.append((dim, split, 0))
            stack.append((idx[~left], depth + 1, me))
            idx, depth = idx[left], depth + 1
    return out, right


def serialize(trees, sample_size):
    """IsolationForest::Serialize (:532-560): size_t 3, tree count, sample size; per tree size_t 3, sample size, the preorder records."""
    b = [struct.pack("<QII", 3, len(trees), sample_size)]
    for t in trees:
        b.append(struct.pack("<QI", 3, sample_size))
        b.extend(struct.pack("<IfI", int(d), float(s), int(z)) for d, s, z in t)
    return b"".join(b)


def parse(stream):
    """The inverse, as Deserialize reads it (size == 0: inner node).  Returns (sample_size, [(dim[], split[], size[], right[])])."""
    stream = bytes(stream)
    dims, n_trees, sample_size = struct.unpack_from("<QII", stream, 0)
    assert dims == 3
    o, trees = 16, []
    for _ in range(n_trees):
        d, s = struct.unpack_from("<QI", stream, o)
        assert d == 3 and s == sample_size
        o += 12
        dim, split, size = [], [], []
        need = 1      # nodes the records read so far still owe: an inner node owes two children
        while need:
            a, b, c = struct.unpack_from("<IfI", stream, o)
            o += 12
            need += 1 if c == 0 else -1
            dim.append(a), split.append(b), size.append(c)
        trees.append((np.array(dim, np.uint32), np.array(split, F32), np.array(size, np.uint32), _right_children(size)))
    assert o == len(stream)
    return sample_size, trees


def _right_children(size):
    """preorder index of every inner node's right child: the node after its left subtree"""
    n = len(size)
    end = [0] * n      # one past the subtree of node i

    right = np.zeros(n, np.uint32)
    # subtree ends by a reverse scan: a leaf ends at i + 1; an inner node's left child is i + 1, its right child is end[left]
    for i in range(n - 1, -1, -1):
        if size[i]:
            end[i] = i + 1
        else:
            right[i] = end[i + 1]
            end[i] = end[end[i + 1]]
    return right


def c_of(n):
    """CalculateC (:103-118)"""
    if n > 2:
        return 2.0 * (math.log(n - 1) + EULER) - (2.0 * (n - 1)) / float(n)
    return 1.0 if n == 2 else 0.0


def total_path_lengths(points, trees):
    """per point, over the trees in index order: total += double(depth of the leaf) + C(leaf size)  (:272-287, :515-522)"""
    pts = np.asarray(points, F32)
    total = np.zeros(len(pts), np.float64)
    for dim, split, size, right in trees:
        node = np.zeros(len(pts), np.int64)
        depth = np.zeros(len(pts), np.int64)
        live = size[node] == 0
        while live.any():
            k = node[live]
            go_left = pts[live, dim[k]] < split[k]
            node[live] = np.where(go_left, k + 1, right[k])
            depth[live] += 1
            live = size[node] == 0
        c = np.array([c_of(int(s)) for s in size[node]], np.float64)
        total = total + (depth.astype(np.float64) + c)
    return total


def scores_from_totals(total, tree_count, sample_size):
    """(:524-526): pow(2, -(total / trees) / C(sample size)); C = 0 gives NaN, as upstream"""
    c = c_of(sample_size)
    out = np.empty(len(total), np.float64)
    for i, t in enumerate(total):
        avg = float(t) / float(tree_count)
        try:
            x = -avg / c
        except ZeroDivisionError:
            x = float("nan") if avg == 0.0 else -math.inf
        out[i] = math.pow(2.0, x) if not math.isnan(x) else float("nan")
    return out


def forest(points, tree_count, seed, sample_size, sorted_form=False):
    """Build + Serialize + GetAnomalyScores: (stream bytes, scores, total path lengths)"""
    pts = [tuple(F32(c) for c in p) for p in np.asarray(points, F32)]
    if sorted_form:
        trees = [build_tree_sorted(pts, s, sample_size) for s in tree_seeds(seed, tree_count)]
    else:
        trees = [build_tree(np.asarray(points, F32), s, sample_size)[0] for s in tree_seeds(seed, tree_count)]
    stream = serialize(trees, sample_size)
    _, parsed = parse(stream)
    total = total_path_lengths(points, parsed)
    return stream, scores_from_totals(total, tree_count, sample_size), total


# Object_Map::IsolationForestDeleteOutliers' own rules (held to the reference text by tests/golden/isolation_forest_constants.json)
TREE_COUNT, SEED, MIN_POINTS, SAMPLE_DIVISOR = 50, 12345, 30, 2
EXEMPT_CLASSES, THRESHOLD, THRESHOLD_CLASS, THRESHOLD_OF_CLASS = (75, 64, 65), 0.6, 62, 0.65


def object_runs(bi_forest, class_id, n):
    return bool(bi_forest) and class_id not in EXEMPT_CLASSES and n >= MIN_POINTS


def object_threshold(class_id):
    """`float th`, promoted to double in `score > th`"""
    return float(F32(THRESHOLD_OF_CLASS if class_id == THRESHOLD_CLASS else THRESHOLD))


def outlier_flags(scores, class_id):
    return (np.asarray(scores, np.float64) > object_threshold(class_id)).astype(np.uint8)      # (a NaN is not an outlier)
