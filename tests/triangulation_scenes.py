"""Small scenes for the triangulation loop of LocalMapping::CreateNewMapPoints (tests/triangulation_reference.py is the yardstick, tests/test_gpu_triangulation.py the
consumer).  A scene is a current keyframe, n_nb neighbours, the match table a search would return, and CLAIMS: per kind of pair the verdict the yardstick must give
every pair of that kind, and -- fixed numbers, written beside each scene from its design -- how many pairs of that kind the scene holds at least
(tests/test_triangulation_reference_cpu.py holds every scene to them: a scene that loses a kind to the generator's relabelling fails there).

Every keypoint of keyframe 1 is the image of one world point; a pair's KIND decides how the neighbour's keypoint is made:
  good          the same point seen from the neighbour, pixel noise, an octave consistent with the two distances
  diverge       the neighbour's keypoint lies beyond the image of the ray's point at infinity: the rays meet behind both cameras          -> BEHIND_1
  behind2       the rays meet in front of camera 1 and behind camera 2 (a neighbour that moved forward past a near point)                -> BEHIND_2
  reproj1 / 2   an offset across the epipolar line, octaves chosen so that only keyframe 1's (only keyframe 2's) chi2 gate is exceeded    -> REPROJ_1 / REPROJ_2
  right1        stereo on side 1, the right-image coordinate 3.5 sigma off while the left error passes 5.991                              -> REPROJ_1
  mbf2          stereo on side 2, its right-image coordinate made with the neighbour's OWN mbf: upstream predicts it with keyframe 1's (:410) -> REPROJ_2
  scale_lo / hi octaves five levels apart, either way                                                                                       -> SCALE
  lowpar        (scenes with a tiny baseline, no stereo)                                                                                    -> LOW_PARALLAX
  unproj1 / 2   baseline below mb, stereo on side 1 (or on both: the `else if` of :317) / on side 2 only                                   -> UNPROJECTED_1 / _2
  nodepth       as unproj1 with mvDepth <= 0                                                                                                -> NO_DEPTH
"""
import numpy as np

import triangulation_reference as Y

f32, f64 = np.float32, np.float64
NLEVELS, SCALE = 8, 1.2
SF = (f32(SCALE) ** np.arange(NLEVELS)).astype(f32)
S2 = (SF * SF).astype(f32)


def _rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Rx @ Ry


def make_camera(center, yaw=0.0, pitch=0.0, fx=520.0, fy=515.0, cx=320.0, cy=240.0, mb=0.08):
    """A keyframe's record as LocalMapping reads it: Rcw, tcw, Ow in float32 (Ow rounded on its own, as KeyFrame::SetPose stores it), mbf = mb * fx."""
    R = _rot(yaw, pitch)
    Ow = np.asarray(center, f64)
    return dict(Rcw=R.astype(f32), tcw=(-R @ Ow).astype(f32), Ow=Ow.astype(f32), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy),
                invfx=f32(1.0 / fx), invfy=f32(1.0 / fy), mb=f32(mb), mbf=f32(mb * fx))


def _proj(cam, P):
    """float64 pinhole image of world points P (n, 3): u, v, z"""
    Pc = P @ cam["Rcw"].astype(f64).T + cam["tcw"].astype(f64)
    z = Pc[:, 2]
    return f64(cam["fx"]) * Pc[:, 0] / z + f64(cam["cx"]), f64(cam["fy"]) * Pc[:, 1] / z + f64(cam["cy"]), z


def _frame(n):
    return dict(kp_x=np.zeros(n, f32), kp_y=np.zeros(n, f32), kp_octave=np.zeros(n, np.int32), u_right=np.full(n, -1, f32), depth=np.full(n, -1, f32),
                scale_factors=SF.copy(), level_sigma2=S2.copy(), nlevels=NLEVELS)


def _keyframe1(rng, cam1, n1, stereo_frac, near_frac, noise):
    """n1 world points in front of camera 1 (depth 4..10 m; a share `near_frac` at 1.3..2.3 m close to the axis) and their keypoints."""
    z = rng.uniform(4.0, 10.0, n1)
    x, y = rng.uniform(-0.45, 0.45, n1) * z, rng.uniform(-0.35, 0.35, n1) * z
    near = rng.random(n1) < near_frac
    z[near] = rng.uniform(1.3, 2.3, near.sum())
    x[near], y[near] = rng.uniform(-0.12, 0.12, near.sum()) * z[near], rng.uniform(-0.12, 0.12, near.sum()) * z[near]
    Pc = np.stack([x, y, z], 1)
    Pw = (Pc - cam1["tcw"].astype(f64)) @ cam1["Rcw"].astype(f64)      # Rwc (Pc - tcw)
    K = _frame(n1)
    K["kp_octave"] = rng.integers(0, NLEVELS, n1).astype(np.int32)
    u, v, zz = _proj(cam1, Pw)
    s = SF[K["kp_octave"]].astype(f64)
    K["kp_x"], K["kp_y"] = (u + noise * s * rng.normal(size=n1)).astype(f32), (v + noise * s * rng.normal(size=n1)).astype(f32)
    st = rng.random(n1) < stereo_frac
    K["u_right"] = np.where(st, K["kp_x"].astype(f64) - f64(cam1["mbf"]) / zz + 0.3 * noise * rng.normal(size=n1), -1).astype(f32)
    K["depth"] = np.where(st, zz, -1).astype(f32)
    return K, Pw, near


def _octave_for(o1, ratio):
    """the level of keyframe 2 whose scale factor ratio sf1 / sf2 is nearest to dist2 / dist1"""
    want = np.log(SF[o1].astype(f64) / ratio) / np.log(SCALE)
    return np.clip(np.rint(want), 0, NLEVELS - 1).astype(np.int32)


def _neighbour(rng, cam1, K1, Pw, near, cam2, n2, n_pairs, kinds, noise, stereo2, mbf_for_ur2=None, reserved=None, rest="good"):
    """One neighbour keyframe, its row of the match table and the kind of every pair.  kinds: {kind: share of the pairs}; the others are of kind `rest`.
    reserved: {kind: mask of the keypoints of keyframe 1 that were prepared for it} -- no other kind pairs them."""
    n1 = len(K1["kp_x"])
    K2 = _frame(n2)
    K2["kp_x"], K2["kp_y"] = rng.uniform(0, 640, n2).astype(f32), rng.uniform(0, 480, n2).astype(f32)
    K2["kp_octave"] = rng.integers(0, NLEVELS, n2).astype(np.int32)
    row = np.full(n1, -1, np.int32)
    kind_of = {}
    if n_pairs == 0:
        return K2, row, kind_of
    st1 = K1["u_right"] >= 0
    o1_all = K1["kp_octave"]
    want = []
    for kind, share in kinds.items():
        want += [kind] * max(1, int(round(share * n_pairs))) if share > 0 else []
    want = want[:n_pairs] + [rest] * max(0, n_pairs - len(want))
    ok_for = {
        "good": ~near, "diverge": ~near, "behind2": near, "reproj1": ~near & (o1_all <= 1), "reproj2": ~near & (o1_all == NLEVELS - 1), "right1": ~near & st1,
        "mbf2": ~near, "scale_lo": ~near & (o1_all >= 6), "scale_hi": ~near & (o1_all <= 1), "lowpar": ~near & ~st1, "unproj1": ~near & st1,
        "unproj2": ~near & ~st1, "nodepth": ~near & st1, "good_mono1": ~near & ~st1, "good_stereo1": ~near & st1, "other": ~near,
    }
    held = np.zeros(n1, bool)
    for kind, mask in (reserved or {}).items():
        held |= mask
    for kind in ok_for:
        ok_for[kind] = (reserved[kind] if reserved and kind in reserved else ok_for[kind] & ~held)
    free = np.ones(n1, bool)
    idx2s = rng.permutation(n2)[:n_pairs]
    u_all, v_all, z_all = _proj(cam2, Pw)
    O1, O2 = cam1["Ow"].astype(f64), cam2["Ow"].astype(f64)
    for kind, i2 in zip(want, idx2s):
        cand = np.nonzero(free & ok_for[kind])[0]
        if len(cand) == 0:
            kind, cand = "other", np.nonzero(free & ok_for["other"])[0]
        i1 = int(rng.choice(cand))
        free[i1] = False
        row[i1] = i2
        kind_of[i1] = kind
        P = Pw[i1]
        o1 = int(o1_all[i1])
        d1, d2 = np.linalg.norm(P - O1), np.linalg.norm(P - O2)
        o2 = int(_octave_for(o1, d2 / d1))
        if kind in ("good", "good_mono1", "good_stereo1", "mbf2", "right1"):      # a level at the end of the pyramid: no consistent octave exists on the other side
            ro, rf = f64(SF[o1]) / f64(SF[o2]), 1.5 * SCALE
            if (d2 / d1) * rf < ro * 1.06 or (d2 / d1) * 1.06 > ro * rf:
                kind = kind_of[i1] = "other"
        u, v, z = u_all[i1], v_all[i1], z_all[i1]
        # the epipolar direction at (u, v): towards the image of the ray's far end
        far = O1 + 1e7 * (P - O1) / d1
        uf, vf, _ = _proj(cam2, far[None])
        e = np.array([uf[0] - u, vf[0] - v])
        ne = max(np.linalg.norm(e), 1e-9)
        across = np.array([-e[1], e[0]]) / ne
        if kind == "diverge":
            u, v = uf[0] + 0.6 * e[0] + 3.0 * e[0] / ne, vf[0] + 0.6 * e[1] + 3.0 * e[1] / ne
        elif kind == "reproj1":
            o2 = NLEVELS - 1
            u, v = u + 9.0 * SF[o1] * across[0], v + 9.0 * SF[o1] * across[1]
        elif kind == "reproj2":
            o2 = 0
            u, v = u + 11.0 * across[0], v + 11.0 * across[1]
        elif kind == "scale_lo":
            o2 = o1 - 5
        elif kind == "scale_hi":
            o2 = o1 + 5
        s = f64(SF[o2])
        if kind in ("good", "good_mono1", "good_stereo1", "right1", "mbf2", "scale_lo", "scale_hi", "unproj1", "unproj2", "nodepth", "lowpar", "other"):
            u, v = u + noise * s * rng.normal(), v + noise * s * rng.normal()
        K2["kp_x"][i2], K2["kp_y"][i2], K2["kp_octave"][i2] = f32(u), f32(v), o2
        is_st2 = (stereo2 and kind not in ("lowpar", "unproj1", "nodepth")) or kind in ("mbf2", "unproj2")
        if kind in ("diverge", "behind2"):
            is_st2 = False
        if is_st2:
            mbf = f64(cam2["mbf"]) if kind == "mbf2" else f64(mbf_for_ur2 if mbf_for_ur2 is not None else cam1["mbf"])
            K2["u_right"][i2] = f32(f64(K2["kp_x"][i2]) - mbf / z)
            K2["depth"][i2] = f32(z)
            if not K2["u_right"][i2] >= 0:      # off the right image: upstream's bStereo2 is false for it
                K2["u_right"][i2], K2["depth"][i2] = f32(-1), f32(-1)
                kind_of[i1] = "other"
    return K2, row, kind_of


# the verdicts a kind may end at (`diverge`: the rays meet behind camera 1, now and then only behind camera 2); kind `other` claims nothing
EXPECT = {"good": (Y.TRIANGULATED,), "good_mono1": (Y.TRIANGULATED,), "good_stereo1": (Y.TRIANGULATED,), "diverge": (Y.BEHIND_1, Y.BEHIND_2), "behind2": (Y.BEHIND_2,),
          "reproj1": (Y.REPROJ_1,), "reproj2": (Y.REPROJ_2,), "right1": (Y.REPROJ_1,), "mbf2": (Y.REPROJ_2,), "scale_lo": (Y.SCALE,), "scale_hi": (Y.SCALE,),
          "lowpar": (Y.LOW_PARALLAX,), "unproj1": (Y.UNPROJECTED_1,), "unproj2": (Y.UNPROJECTED_2,), "nodepth": (Y.NO_DEPTH,)}


def _assemble(name, K1, cam1, nbs, claims, friendly=True, notes=""):
    return dict(name=name, K1=K1, cam1=cam1, K2s=[n[0] for n in nbs], cams2=[n[1] for n in nbs],
                match12=np.stack([n[2] for n in nbs]) if nbs else np.zeros((0, len(K1["kp_x"])), np.int32), kinds=[n[3] for n in nbs],
                ratio_factor=Y.ratio_factor(SCALE), claims=claims, friendly=friendly, notes=notes)


# what wide_mono's two kinds of neighbour hold by design: 257 pairs sideways -> round(0.06 * 257) = 15 diverging, 13 + 13 reprojection outliers, 10 + 10 octave
# pairs; 65 pairs forward -> round(0.25 * 65) = 16 behind camera 2 and 3 diverging; the rest good, less the few whose level lies at an end of the pyramid
WIDE_MONO_CLAIMS = {"good": 230, "diverge": 18, "reproj1": 13, "reproj2": 13, "scale_lo": 10, "scale_hi": 10, "behind2": 16}


def wide_mono(seed=11, n1=1000, pairs=(257, 0, 65), origin=(0.0, 0.0, 0.0), name="wide_mono", claims=WIDE_MONO_CLAIMS):
    """Monocular on both sides, baselines of 0.6..1.2 m sideways and one neighbour 3 m FORWARD (the near points lie behind it); different intrinsics per keyframe;
    an empty row between two populated ones; every rejecting gate of a triangulated point but the right-image ones."""
    rng = np.random.default_rng(seed)
    O = np.asarray(origin, f64)
    cam1 = make_camera(O, 0.02, -0.01)
    K1, Pw, near = _keyframe1(rng, cam1, n1, 0.0, 0.12, 0.5)
    nbs = []
    mism = {"diverge": 0.06, "reproj1": 0.05, "reproj2": 0.05, "scale_lo": 0.04, "scale_hi": 0.04}
    for k, npairs in enumerate(pairs):
        forward = k % 3 == 2
        if forward:
            cam2 = make_camera(O + _rot(0.02, -0.01).T @ np.array([0.15, 0.05, 3.0]), 0.0, 0.0, fx=500.0 + 7 * k, fy=505.0, cx=315.0, cy=236.0 + k)
            kinds = {"behind2": 0.25, "diverge": 0.05}
        else:
            cam2 = make_camera(O + np.array([0.6 + 0.15 * (k % 4), 0.1 * ((k % 3) - 1), 0.05 * k]), 0.02 - 0.03 * (k % 3), 0.01, fx=500.0 + 7 * k, fy=505.0, cx=315.0,
                               cy=236.0 + k)
            kinds = mism
        K2, row, kind_of = _neighbour(rng, cam1, K1, Pw, near, cam2, n1 + 37 - 5 * (k % 7), npairs, kinds, 0.5, stereo2=False)
        nbs.append((K2, cam2, row, kind_of))
    return _assemble(name, K1, cam1, nbs, dict(claims))


def stereo_mix(seed=21, n1=333):
    """Stereo keypoints on 60 % of keyframe 1.  Neighbour 0 / 1 / 2: baseline 0.4 mb with stereo on side 1 only / side 2 only / both (the two unprojection
    branches and the `else if` of :317, slots with mvDepth <= 0, mvKeys != mvKeysUn); neighbour 3: 0.9 m away, stereo on both sides, another mbf than keyframe 1
    (:410 decides verdicts), right-image errors that fail 7.8 while the left passes 5.991."""
    rng = np.random.default_rng(seed)
    cam1 = make_camera((0.3, -0.2, 0.1), -0.01, 0.015, mb=0.08)
    K1, Pw, near = _keyframe1(rng, cam1, n1, 0.6, 0.0, 0.15)
    K1["raw_x"] = (K1["kp_x"] + f32(0.3) * np.sin(np.arange(n1)).astype(f32)).astype(f32)
    K1["raw_y"] = (K1["kp_y"] - f32(0.2) * np.cos(np.arange(n1)).astype(f32)).astype(f32)
    # keypoints of keyframe 1 prepared for one kind: mvDepth <= 0 under a valid uRight; a right-image coordinate 3.5 sigma of its level off
    st = np.nonzero(K1["u_right"] >= 0)[0]
    pick = rng.permutation(st)
    reserved = {"nodepth": np.zeros(n1, bool), "right1": np.zeros(n1, bool)}
    reserved["nodepth"][pick[:8]] = True
    reserved["right1"][pick[8:24]] = True
    for j, i1 in enumerate(pick[:8]):
        K1["depth"][i1] = f32(0.0) if j % 2 else f32(-1.0)
    for i1 in pick[8:24]:
        K1["u_right"][i1] = f32(K1["u_right"][i1] + 3.5 * SF[K1["kp_octave"][i1]])
    nbs = []
    short = np.array([0.032, 0.0, 0.0])
    specs = [(64, {"unproj1": 0.8, "nodepth": 0.1, "lowpar": 0.1}, False), (63, {"unproj2": 0.8, "lowpar": 0.2}, False), (65, {"unproj1": 1.0}, True)]
    for k, (npairs, kinds, stereo2) in enumerate(specs):
        cam2 = make_camera(np.array([0.3, -0.2, 0.1]) + short * (1 if k != 1 else -1), -0.01, 0.015, fx=522.0, fy=515.0, cx=321.0, cy=240.0, mb=0.08)
        K2, row, kind_of = _neighbour(rng, cam1, K1, Pw, near, cam2, n1 + 11 + k, npairs, kinds, 0.15, stereo2=stereo2, reserved=reserved, rest="other")
        if k == 2:      # stereo on both sides: every paired keypoint of the neighbour is stereo too
            for i1 in np.nonzero(row >= 0)[0]:
                i2 = row[i1]
                _, _, z = _proj(cam2, Pw[i1][None])
                K2["u_right"][i2], K2["depth"][i2] = f32(f64(K2["kp_x"][i2]) - f64(cam2["mbf"]) / z[0]), f32(z[0])
        K2["raw_x"], K2["raw_y"] = (K2["kp_x"] + f32(0.25)).astype(f32), (K2["kp_y"] - f32(0.15)).astype(f32)
        nbs.append((K2, cam2, row, kind_of))
    cam2 = make_camera((1.2, -0.15, 0.1), -0.04, 0.01, fx=530.0, fy=520.0, cx=318.0, cy=243.0, mb=0.3)      # mbf 159 against keyframe 1's 41.6
    K2, row, kind_of = _neighbour(rng, cam1, K1, Pw, near, cam2, n1 + 5, 64, {"mbf2": 0.25, "right1": 0.2, "good_mono1": 0.2}, 0.15, stereo2=True, reserved=reserved)
    nbs.append((K2, cam2, row, kind_of))
    # by design: 51 + 65 unprojections from keyframe 1, 50 from keyframe 2, 6 slots without depth, 6 + 13 low-parallax pairs; of neighbour 3's 16 + 13 + 13 + 22
    # a few leave their kind (no consistent octave, a right coordinate off the image)
    return _assemble("stereo_mix", K1, cam1, nbs, {"unproj1": 116, "unproj2": 50, "nodepth": 6, "lowpar": 19, "mbf2": 12, "right1": 10, "good_mono1": 10, "good": 15})


def low_parallax(seed=31, n1=130, n_pairs=64):
    """A 2 cm baseline without stereo: every pair ends at `No stereo and very low parallax`."""
    rng = np.random.default_rng(seed)
    cam1 = make_camera((0.0, 0.0, 0.0))
    K1, Pw, near = _keyframe1(rng, cam1, n1, 0.0, 0.0, 0.2)
    cam2 = make_camera((0.02, 0.0, 0.0))
    K2, row, kind_of = _neighbour(rng, cam1, K1, Pw, near, cam2, n1 + 3, n_pairs, {"lowpar": 1.0}, 0.2, stereo2=False)
    return _assemble("low_parallax", K1, cam1, [(K2, cam2, row, kind_of)], {"lowpar": n_pairs})


def single_pair(seed=41, n1=65):
    rng = np.random.default_rng(seed)
    cam1 = make_camera((0.0, 0.0, 0.0))
    K1, Pw, near = _keyframe1(rng, cam1, n1, 0.0, 0.0, 0.3)
    cam2 = make_camera((0.8, 0.0, 0.0), -0.02)
    K2, row, kind_of = _neighbour(rng, cam1, K1, Pw, near, cam2, n1 + 1, 1, {}, 0.3, stereo2=False)
    return _assemble("single_pair", K1, cam1, [(K2, cam2, row, kind_of)], {"good": 1})


TWENTY_PAIRS = (257, 0, 1, 63, 64, 65, 0, 257, 65, 1, 64, 63, 257, 0, 65, 64, 1, 63, 257, 65)


def twenty(seed=51, n1=1100):
    """Twenty neighbours of a 1100-keypoint keyframe (two workgroups per neighbour, the last one partly filled), 100 m from the origin."""
    # by design: four sideways neighbours of 257 pairs (as wide_mono's), five forward ones of 65 (16 behind camera 2, 3 diverging each), five sideways ones of
    # 63..65 (4 + 3 + 3 + 3 + 3 each), three of one pair (the first kind of their list)
    claims = {"good": 1200, "diverge": 4 * 15 + 5 * 3 + 5 * 4 + 2, "reproj1": 4 * 13 + 5 * 3, "reproj2": 4 * 13 + 5 * 3, "scale_lo": 4 * 10 + 5 * 3, "scale_hi": 4 * 10 + 5 * 3,
              "behind2": 5 * 16 + 1}
    return wide_mono(seed, n1, TWENTY_PAIRS, origin=(100.0, -60.0, 40.0), name="twenty", claims=claims)


def nan_row(seed=61, n1=70):
    """stereo_mix's first neighbour in small, with one NaN keypoint coordinate in keyframe 1 (the pair falls through :323, :344 and :348 to `continue`) and one NaN
    mvKeys coordinate on an unprojecting slot (the point is NaN and, as upstream's comparisons are written, passes every gate)."""
    rng = np.random.default_rng(seed)
    cam1 = make_camera((0.0, 0.0, 0.0))
    K1, Pw, near = _keyframe1(rng, cam1, n1, 1.0, 0.0, 0.3)
    cam2 = make_camera((0.04, 0.0, 0.0))
    K2, row, kind_of = _neighbour(rng, cam1, K1, Pw, near, cam2, n1 + 2, 10, {"unproj1": 1.0}, 0.3, stereo2=False)
    paired = np.nonzero(row >= 0)[0]
    K1["raw_x"], K1["raw_y"] = K1["kp_x"].copy(), K1["kp_y"].copy()
    K1["kp_x"][paired[0]] = np.nan
    K1["raw_x"][paired[1]] = np.nan
    kind_of[int(paired[0])] = "nan_kp"
    kind_of[int(paired[1])] = "nan_raw"
    sc = _assemble("nan_row", K1, cam1, [(K2, cam2, row, kind_of)], {"unproj1": 8}, friendly=False)
    sc["nan_slots"] = (int(paired[0]), int(paired[1]))
    return sc


def all_scenes():
    """Every scene once (module-level cache: the tests share them and leave them unchanged)."""
    global _CACHE
    if _CACHE is None:
        scs = [wide_mono(), stereo_mix(), low_parallax(), single_pair(), twenty(), nan_row()]
        _CACHE = {sc["name"]: sc for sc in scs}
    return _CACHE


_CACHE = None

# what the scenes must reach between them, at least (tests/test_triangulation_reference_cpu.py)
MIN_PER_VERDICT = {Y.TRIANGULATED: 500, Y.UNPROJECTED_1: 80, Y.UNPROJECTED_2: 40, Y.LOW_PARALLAX: 64, Y.BEHIND_1: 30, Y.BEHIND_2: 20, Y.REPROJ_1: 30, Y.REPROJ_2: 30,
                   Y.SCALE: 30, Y.NO_DEPTH: 4, Y.EMPTY: 10000}


def sized(n_pairs, seed=71):
    """wide_mono with ONE neighbour of n_pairs pairs over 1000 keypoints: the size sequence 257 -> 0 -> 1 -> 65 -> 257 of the GPU test."""
    return wide_mono(seed + n_pairs, 1000, (n_pairs,), name="sized_%d" % n_pairs, claims={})
