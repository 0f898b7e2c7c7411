"""Seeded depth images for the plane segmentation tests, rendered analytically to float32.  Each scene names the branch it is there to reach in `claims`;
tests/test_plane_segmentation_reference_cpu.py holds every scene to its claims with the yardstick."""
import numpy as np

import plane_segmentation_reference as R


def _rays(c):
    n = (np.arange(c.width, dtype=np.float64)[None, :] - float(c.cx)) / float(c.fx)
    m = (np.arange(c.height, dtype=np.float64)[:, None] - float(c.cy)) / float(c.fy)
    return n + 0 * m, m + 0 * n


def _plane_depth(c, normal, offset):
    """z of the plane normal . p = offset along every pixel's ray (inf where the ray misses it)"""
    rx, ry = _rays(c)
    den = normal[0] * rx + normal[1] * ry + normal[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = offset / den
    return np.where((den > 1e-9) & (z > 0), z, np.inf), rx, ry


def _cfg(width, height, **kw):
    s = width / 640.0
    return R.default_cfg(width, height, fx=517.306408 * s, fy=516.469215 * s, cx=318.643040 * s, cy=255.313989 * s, **kw)


def _room(c, seed, noise):
    floor, _, _ = _plane_depth(c, (0.0, 1.0, 0.0), 1.1)
    back, _, _ = _plane_depth(c, (0.0, 0.0, 1.0), 3.4)
    left, _, _ = _plane_depth(c, (-1.0, 0.0, 0.15), 1.6)
    z = np.minimum(np.minimum(floor, back), left)
    box, rx, ry = _plane_depth(c, (0.0, 0.0, 1.0), 2.0)
    on = (rx * box > 0.25) & (rx * box < 1.05) & (ry * box > 0.2) & (ry * box < 1.1)
    z = np.where(on & (box < z), box, z)
    rng = np.random.default_rng(seed)
    z = z + noise * z * z * rng.standard_normal(z.shape)
    return z.astype(np.float32)


def _noisy(z, seed, sigma=2e-4):
    """An exact plane has an mse of rounding noise only, and the queue's order would rest on it: the two eigen-solves of the yardstick would then merge in
    different orders.  A fifth of a millimetre of seeded noise gives every block an mse of its own."""
    return z + sigma * np.random.default_rng(seed).standard_normal(z.shape)


def _tilted(c, offset=1.5, normal=(0.1, 0.2, 1.0), seed=5):
    n = np.array(normal) / np.linalg.norm(normal)
    z, _, _ = _plane_depth(c, n, offset)
    return _noisy(z, seed).astype(np.float32)


def scenes():
    out = {}

    def add(name, c, depth, **claims):
        out[name] = dict(cfg=c, depth=np.ascontiguousarray(depth, np.float32), claims=claims)

    c = _cfg(640, 480)
    add("room_vga", c, _room(c, 11, 0.0012), min_planes=3, stopped=True, retaken=True)
    c = _cfg(80, 60, min_support=300)
    add("room_small", c, _room(c, 12, 0.0012), min_planes=1, eroded_planes=True)
    # 65 x 45 and 75 x 55 leave five pixels outside every block (70 x 50 leaves none at window 10: the control).  The fill only starts at a block border, so the
    # last block of the last block row has a hole: its pixels and, through them, the border pixels are claimed by the flood fill alone.
    for w, h in ((70, 50), (65, 45), (75, 55)):
        c = _cfg(w, h, min_support=300)
        d = _tilted(c)
        d[h - h % 10 - 5 if h % 10 else h - 5, w - w % 10 - 5 if w % 10 else w - 5] = 0
        add("ragged_%dx%d" % (w, h), c, d, n_planes=1, ragged_claimed=bool(w % 10))

    # the validity limits: one special value per block of the top row, the rest one plane
    c = _cfg(80, 60, min_support=300)
    d = _tilted(c, 1.5)
    lo, hi = np.float32(0.2), np.float32(4.0)
    special = [lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0)), np.nextafter(hi, np.float32(5)),
               np.float32(0), np.float32(np.nan)]
    for k, v in enumerate(special):
        d[5, 10 * k + 5] = v
    d[15, 5] = np.float32(np.inf)
    d[15, 15] = np.float32(-1.0)
    add("limits", c, d, missing_blocks=[2, 5, 6, 7, 8, 9], n_planes=1)

    # a neighbour difference exactly at T_dz (alpha and tolerance powers of two, so the threshold is exact), and one float beyond
    c = _cfg(80, 60, min_support=300, depth_alpha=0.03125, depth_change_tol=0.015625)
    d = np.full((60, 80), 1.0, np.float64)
    d[:, 40:] = 1.046875                             # |z - zn| = 0.046875 = T_dz(1.0): not a discontinuity (strict >)
    exact = d[:, 39:41].copy()
    d = _noisy(d, 21).astype(np.float32)
    d[:, 39:41] = exact                              # the two columns of the step are exact; the rest carries the noise
    add("tdz_at", c, d, discontinuity_blocks=[])
    d = d.copy()
    d[25, 40] = np.nextafter(np.float32(1.046875), np.float32(2))
    # seen from (25, 39) in block 19 it exceeds T_dz(1.0); from its own side T_dz(1.046875...) is larger and nothing is seen
    add("tdz_beyond", c, d, discontinuity_blocks=[2 * 8 + 3])

    # a step that lies exactly on a block border: only the halo column / row of the next block shows it
    c = _cfg(80, 60, min_support=300)
    d = np.full((60, 80), 1.0, np.float64)
    d[:, 50:] = 1.5
    d[30:, :] += 0.5
    d = _noisy(d, 22).astype(np.float32)
    add("halo", c, d, discontinuity_blocks=sorted(set([r * 8 + 4 for r in range(6)] + [2 * 8 + k for k in range(8)])))

    # nothing: every block has a hole
    c = _cfg(80, 60, min_support=300)
    d = _tilted(c)
    d[4::10, 4::10] = 0
    add("no_plane", c, d, n_planes=0)
    c = _cfg(80, 60, min_support=300)
    add("one_plane", c, _tilted(c), n_planes=1, n_voxels_min=2)

    # a cluster that is large enough and eroded completely: a strip one block high, every block of which has a black neighbour
    c = _cfg(80, 60, min_support=800)
    d = _tilted(c)
    d[0:20, :] = 0
    d[30:60, :] = 0
    add("eroded", c, d, n_first=1, n_planes=0)

    # two coplanar regions either side of a black strip one block wide whose middle rows are valid: the flood fill meets itself there
    c = _cfg(120, 60, min_support=300)
    d = _tilted(c, 1.5, (0.0, 0.0, 1.0))
    d[0:25, 50:70] = 0
    d[35:60, 50:70] = 0
    add("coplanar_strip", c, d, n_first=2, n_planes=1, connects=True)

    # a table top 10 cm above the floor: parallel, closer than 0.2: PlaneNotSeen drops the smaller
    c = _cfg(160, 120, min_support=600)
    floor, rx, ry = _plane_depth(c, (0.0, 0.6, 0.8), 1.6)
    table, _, _ = _plane_depth(c, (0.0, 0.6, 0.8), 1.5)
    d = _noisy(np.where(rx * table > 0.05, table, floor), 23)
    add("table", c, d.astype(np.float32), n_planes=2, n_kept=1)

    # coef[3] < 0 before the flip: unreachable.  The fit turns the normal so that n . c <= 0 with the very products -(n . c) repeats, so d >= 0 for every input
    # (DESIGN.md section 4k); every scene's claim includes that nothing flips.
    # one voxel: the principal point left of and above the image, so x, y, z > 0 everywhere, and a leaf larger than the scene
    c = _cfg(40, 30, min_support=100, leaf=np.float32(5.0))
    c.cx, c.cy = np.float32(-1.0), np.float32(-1.0)
    add("one_voxel", c, _tilted(c), n_planes=1, n_voxels=1)

    # points exactly on a voxel face: a fronto-parallel wall at about 1.25 m with 0.2 mm of noise, of which two pixels are exactly 1.25f.  1.25f * 20 = 25 is
    # exact in float, so floor() decides ON the face between cells 24 and 25 along z and the point belongs to the upper one; the noisy neighbours fall on
    # either side, so both cells are occupied.
    c = _cfg(80, 60, min_support=300)
    d = _tilted(c, 1.25, (0.0, 0.0, 1.0), seed=31)
    d[33, 47] = np.float32(1.25)
    d[12, 20] = np.float32(1.25)
    add("voxel_face", c, d, n_planes=1, on_face=[33 * 80 + 47, 12 * 80 + 20])
    return out


SMALL = [k for k, v in scenes().items() if v["cfg"].width * v["cfg"].height <= 160 * 120]
