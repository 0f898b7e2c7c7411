"""Text scenes for tests/cpp/pnp_solver/pnp_solver_driver.cpp: a PnPsolver problem of tests/pnp_solver_scenes.py spread over a frame's match vector together with
entries the constructor must filter (no map point, a bad map point), and the driver's generator restated."""
import numpy as np

LEVEL_SIGMA2 = (1.2 ** (2 * np.arange(8))).astype(np.float32)


class Lcg:
    """standin::Random of the driver: RandomInt(min, max) of a 64-bit LCG"""

    def __init__(self, seed):
        self.state, self.calls = seed, 0

    def random_int(self, lo, hi):
        self.calls += 1
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return lo + (self.state >> 33) % (hi - lo + 1)


def draw_sets(lcg, n, min_set, n_hyp):
    """the sampling loop of iterate (:188-201) with its quirk, over the driver's generator"""
    sets = np.zeros((n_hyp, min_set), np.int32)
    for h in range(n_hyp):
        avail = list(range(n))
        size = n
        for i in range(min_set):
            idx = avail[lcg.random_int(0, size - 1)]
            sets[h, i] = idx
            avail[idx] = avail[size - 1]      # (the buffer keeps its capacity n, as the adapter's does)
            size -= 1
    return sets


def candidate_text(prob, seed=7, extra=0.4):
    """(text, index, n_matches): the n correspondences in order at the positions `index` of a longer match vector; the other entries have no map point or a bad one."""
    rng = np.random.default_rng(seed)
    n = len(prob["sigma2"])
    total = n + int(extra * n) + 2
    index = sorted(rng.choice(total, n, replace=False).tolist())
    octave = np.array([int(np.flatnonzero(LEVEL_SIGMA2 == s)[0]) for s in np.asarray(prob["sigma2"], np.float32)])
    lines = ["%d" % total, " ".join("%.9g" % np.float32(k) for k in prob["K"]), " ".join("%.9g" % s for s in LEVEL_SIGMA2)]
    pos = {p: i for i, p in enumerate(index)}
    for j in range(total):
        if j in pos:
            i = pos[j]
            X, uv = prob["p3d_w"][i], prob["p2d"][i]
            lines.append("0 %.9g %.9g %.9g %.9g %.9g %d" % (X[0], X[1], X[2], uv[0], uv[1], octave[i]))
        else:
            lines.append("%d %.9g %.9g %.9g %.9g %.9g %d" % ((-1 if rng.random() < 0.5 else 1,) + tuple(rng.uniform(-3, 3, 3)) + tuple(rng.uniform(0, 600, 2)) + (int(rng.integers(0, 8)),)))
    return "\n".join(lines) + "\n", index, total
