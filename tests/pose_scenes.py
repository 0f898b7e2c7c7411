"""PoseOptimization problems on which the LM REJECTS trials and on which rounds 2-4 differ from round 1 -- what eao_fusion_amd.synth.synth_pose (points 2 - 6 m in
front of the camera, a start within one degree) never produces.  numpy only; used by tests/test_pose_scenes_cpu.py (the oracle alone), tests/test_gpu_pose_rounds.py
(the device against the oracle) and tools/pose_round_bands.py (the bounds).

  far_off     the start 20 - 35 degrees and 0.8 - 1.2 m off the true pose, depths 0.3 - 6 m, outlier shares 0 / 0.1 / 0.3, monocular shares 0 / 0.3 / 1; n on both
              sides of every launch-geometry boundary of csrc/pose.hip (pose_class: 256, 512, 1024; 2048 for the global-memory variant; 63 / 64 / 65 for the first
              wave).  Seeds picked on the CPU (tools/pose_round_bands.py --search prints the candidates).
  scattered   synth_pose(n, seed, outlier_frac=0) with every observation replaced by a uniform draw over the 640 x 480 image: nearly every edge is excluded after
              round 1, rounds 2 - 4 run on 0, 1 or 2 edges (g2o makes no iteration without a level-0 edge; one or two edges leave H rank-deficient).
  boundary    n + planes on either side of the `< 10` break behind round 1 (src/Optimizer.cc, edges().size() < 10), and n = 3.
  zero_depth  a map point in the camera's plane z = 0: chi2 is inf and rho NaN from the first pass on.

A trace is four optimize() calls laid end to end; trace["round_start"] cuts it.  An iteration (round, k) is DECIDED when its trial count is the same in the oracle's
run on the problem and in its twelve runs on one-ulp perturbations of the inputs (perturbed()); a round is compared up to its first undecided iteration."""
import numpy as np

from eao_fusion_amd import synth

# launch geometry of the register kernels (csrc/pose.hip pose_threads, kPoseCand): retrials are evaluated in batches of min(4, waves)
POSE_CAND = 4
LM_MAX_TRIALS = 10


def waves(n):
    return 4 if n > 192 else max(1, (n + 63) // 64)


def far_off(n, seed, outlier_frac, mono_frac):
    rng = np.random.default_rng(seed)
    pts = np.empty((n, 3))
    pts[:, 2] = rng.uniform(0.3, 6.0, n)
    pts[:, 0] = rng.uniform(-0.45, 0.45, n) * pts[:, 2]
    pts[:, 1] = rng.uniform(-0.35, 0.35, n) * pts[:, 2]
    Rcw, tcw = synth._rot(0.03, -0.05, 0.02), np.array([0.1, -0.05, 0.2])
    Xc = pts @ Rcw.T + tcw
    octave = rng.integers(0, 8, size=n)
    inv_sigma2 = (np.float32(1.0) / (np.float32(1.2) ** (2 * octave)).astype(np.float32)).astype(np.float32)
    u = synth.FX * Xc[:, 0] / Xc[:, 2] + synth.CX
    v = synth.FY * Xc[:, 1] / Xc[:, 2] + synth.CY
    ur = u - synth.BF / Xc[:, 2]
    noise = rng.normal(0, 1.0, size=(n, 3)) * (1.2 ** octave)[:, None]
    out = rng.random(n) < outlier_frac
    noise[out, :2] += rng.uniform(10, 40, size=(int(out.sum()), 2)) * rng.choice([-1, 1], size=(int(out.sum()), 2))
    obs = np.stack([u + noise[:, 0], v + noise[:, 1], np.maximum(ur + noise[:, 0] + 0.3 * noise[:, 2], 0.0)], axis=1)
    obs[rng.random(n) < mono_frac, 2] = -1.0
    axis = rng.normal(0, 1, 3)
    axis *= np.deg2rad(rng.uniform(20.0, 35.0)) / np.linalg.norm(axis)
    d = synth._rot(*axis)
    off = rng.normal(0, 1, 3)
    off *= rng.uniform(0.8, 1.2) / np.linalg.norm(off)
    T = np.eye(4)
    T[:3, :3] = d @ Rcw
    T[:3, 3] = d @ tcw + off
    return dict(Tcw=T.astype(np.float32), points=pts.astype(np.float32), obs=obs.astype(np.float32), inv_sigma2=inv_sigma2,
                fx=np.float32(synth.FX), fy=np.float32(synth.FY), cx=np.float32(synth.CX), cy=np.float32(synth.CY), bf=np.float32(synth.BF))


def scattered(n, seed):
    p = synth.synth_pose(n=n, seed=seed, outlier_frac=0.0)
    rng = np.random.default_rng(seed + 77000)
    obs = p["obs"].copy()
    stereo = obs[:, 2] >= 0
    obs[:, 0] = rng.uniform(0, 640, n)
    obs[:, 1] = rng.uniform(0, 480, n)
    ur = np.maximum(obs[:, 0] - rng.uniform(5, 30, n), 0).astype(np.float32)
    obs[stereo, 2] = ur[stereo]
    p["obs"] = obs
    return p


def boundary(n, n_planes, seed):
    return synth.synth_pose(n=n, seed=seed, n_planes=n_planes)


def zero_depth():
    """the identity start pose and map point 0 in the camera's plane z = 0 (tests/pnp_solver_scenes.py has the same for PnP): its projection is infinite, chi2 is inf from
    the first pass on, rho is NaN in every iteration -- ten iterations of one rejected trial each, nothing accepted, and a round 1 that excludes every edge.  Kept because
    the oracle's trace and outlier table are the same, bit for bit, in all thirteen runs (tests/test_pose_scenes_cpu.py)."""
    p = synth.synth_pose(n=40, seed=4610, outlier_frac=0.0)
    p["Tcw"] = np.eye(4, dtype=np.float32)
    p["points"][0, 2] = 0.0
    return p


# A far_off or scattered candidate is ADMITTED when the oracle's thirteen runs agree on its outlier table and round structure and their chi2 / lambda differ by at
# most these figures (relative) on its decided iterations: a scene whose own one-ulp band is of order one says nothing about a second implementation.
ADMIT_CHI2_SPREAD = 1e-3
ADMIT_LAMBDA_SPREAD = 1e-2
# The search (tools/pose_round_bands.py --search): far_off seeds 5000 .. 5007 for every n x outlier share x monocular share below, 720 candidates, 715 with stable tables, 464
# admitted with chi2 spread <= 1e-4; two per n with different shares, ranked by what their decided prefixes hold.  scattered seeds 0 .. 59 per n, 240 candidates.
FAR_OFF_N = (63, 64, 65, 256, 257, 512, 513, 1024, 1025, 2100)      # (the second sweep adds 200: four waves, one edge per thread)
SCATTERED_N = (12, 30, 64, 200)
# far_off: (n, seed, outlier share, monocular share)
FAR_OFF = [(63, 5001, 0.0, 0.3), (63, 5005, 0.1, 1.0), (64, 5006, 0.0, 0.3), (64, 5006, 0.0, 1.0), (65, 5000, 0.3, 0.0), (65, 5001, 0.3, 1.0),
           (256, 5004, 0.1, 1.0), (256, 5000, 0.0, 0.0), (257, 5000, 0.0, 0.3), (257, 5007, 0.1, 0.3), (512, 5003, 0.1, 1.0), (512, 5004, 0.1, 0.0),
           (513, 5002, 0.1, 0.0), (513, 5002, 0.1, 0.3), (1024, 5007, 0.0, 0.0), (1024, 5004, 0.0, 1.0), (1025, 5005, 0.0, 1.0), (1025, 5006, 0.1, 0.0),
           (2100, 5002, 0.0, 0.3), (2100, 5002, 0.0, 1.0)]
# ... and five on which the kernel's kRefresh pass decides the outlier table: round 1 ends on an accepted retrial in front of the end of its candidate batch, and a
# build that keeps the residuals of the batch's last candidate instead excludes other edges (a round that leaves two edges in either way does not show whether the pass
# ran).  Second sweep of the search: seeds 5072 .. 5271 at six four-wave sizes, 10800 candidates; a scratch build without the pass differs from the kernel on 40 of
# them, 25 of those are admitted.
FAR_OFF += [(200, 5139, 0.0, 0.3), (256, 5102, 0.1, 1.0), (257, 5163, 0.0, 1.0), (513, 5165, 0.0, 0.0), (513, 5256, 0.1, 1.0)]
# scattered: (n, seed).  Level-0 edges in rounds 2 / 3 / 4: (12, 10) (30, 2) (64, 20) (200, 28) none at all -- the input pose comes back; (12, 23) 2 / 1 / 1; (12, 30) 2 / 2 / 2;
# (30, 23) and (200, 11) 0 / 1 / 1 -- an edge excluded after round 1 is taken back in at the start pose after a round 2 without iterations; (64, 5) 1 / 1 / 1
SCATTERED = [(12, 10), (12, 23), (12, 30), (30, 2), (30, 23), (64, 5), (64, 20), (200, 11), (200, 28)]
ALL_EXCLUDED = [(12, 10), (30, 2), (64, 20), (200, 28)]
# boundary: (n, planes, seed)
BOUNDARY = [(3, 0, 4601), (9, 0, 4602), (10, 0, 4603), (7, 2, 4604), (7, 3, 4605)]


def all_scenes():
    out = {}
    for a in FAR_OFF:
        out["far_off n=%d seed=%d out=%g mono=%g" % a] = ("far_off", far_off, a)
    for a in SCATTERED:
        out["scattered n=%d seed=%d" % a] = ("scattered", scattered, a)
    for a in BOUNDARY:
        out["boundary n=%d planes=%d seed=%d" % a] = ("boundary", boundary, a)
    out["zero_depth"] = ("zero_depth", zero_depth, ())
    return out


def build(name):
    family, fn, args = all_scenes()[name]
    return fn(*args)


def expected_rounds(prob):
    """the `< 10` rule: one optimize() call when points + planes < 10, four otherwise (none below three points)"""
    n, m = len(prob["points"]), len(prob.get("plane_world", ()))
    return 0 if n < 3 else 1 if n + m < 10 else 4


# ---------------------------------------------------------------------------------------------------------------------- the thirteen runs
def _shift(a, towards):
    """every float32 entry one ulp towards +-inf; an entry does not leave zero or cross it"""
    b = np.nextafter(a, np.float32(towards)).astype(np.float32)
    return np.where((a == 0) | (np.sign(b) != np.sign(a)), a, b)


def perturbed(prob):
    """the twelve one-ulp perturbations of tests/test_gpu_lm_conditioning.py: points / observations / pose shifted up, shifted down, and six draws with a random
    direction per entry of all three.  The monocular marker (ur < 0) and the pose's bottom row stay."""
    arrays = ("points", "obs", "Tcw")

    def fixed(q):
        q["obs"][:, 2] = np.where(prob["obs"][:, 2] < 0, prob["obs"][:, 2], q["obs"][:, 2])
        q["Tcw"][3, :] = prob["Tcw"][3, :]
        return q

    for arr in arrays:
        for towards in (np.inf, -np.inf):
            q = dict(prob, obs=prob["obs"].copy(), Tcw=prob["Tcw"].copy())
            q[arr] = _shift(prob[arr], towards)
            yield fixed(q)
    for s in range(6):
        rs = np.random.default_rng(9000 + s)
        q = dict(prob)
        for arr in arrays:
            up = rs.integers(0, 2, size=prob[arr].shape).astype(bool)
            q[arr] = np.where(up, _shift(prob[arr], np.inf), _shift(prob[arr], -np.inf)).astype(np.float32)
        yield fixed(q)


def oracle_runs(O, prob):
    return [O.pose_optimization(prob)] + [O.pose_optimization(q) for q in perturbed(prob)]


def rounds_of(trace):
    """[(first, last + 1)] trace indices of each optimize() call"""
    rs = [int(x) for x in trace["round_start"]]
    return list(zip(rs, rs[1:] + [len(trace["trials"])]))


def tables_agree(runs):
    """same outlier (and plane) table, return value and round structure in all runs"""
    b = runs[0]
    for r in runs[1:]:
        if not (np.array_equal(r["outlier"], b["outlier"]) and r["n_inliers"] == b["n_inliers"] and len(r["trace"]["round_start"]) == len(b["trace"]["round_start"])):
            return False
        if "plane_outlier" in b and not np.array_equal(r["plane_outlier"], b["plane_outlier"]):
            return False
        if [e > s for s, e in rounds_of(r["trace"])] != [e > s for s, e in rounds_of(b["trace"])]:      # a round without iterations is one in every run
            return False
    return True


def decided(runs):
    """per round of the base run: the number of leading iterations whose trial count is the same in all runs"""
    base = rounds_of(runs[0]["trace"])
    out = []
    for rd, (s, e) in enumerate(base):
        k = 0
        while s + k < e:
            q = runs[0]["trace"]["trials"][s + k]
            ok = True
            for r in runs[1:]:
                rr = rounds_of(r["trace"])
                if rd >= len(rr) or rr[rd][0] + k >= rr[rd][1] or r["trace"]["trials"][rr[rd][0] + k] != q:
                    ok = False
                    break
            if not ok:
                break
            k += 1
        out.append(k)
    return out


CHI2_FLOOR = 1e-6      # chi2 differences are taken relative to max(chi2, this): the floor tests/test_gpu_lm.py's _check_trace stops at.  A round on one or two edges fits them
                       # exactly and its chi2 (1e-28, say) is rounding noise of the solve


def chi2_rel_of(a, ref):
    return abs(a - ref) / max(abs(ref), CHI2_FLOOR)


def lam_rel(a, ref):
    return abs(a - ref) / max(abs(ref), 1e-300)


def spread(runs, dec):
    """largest relative spread of chi2 and of lambda over the decided iterations, base run against each other run"""
    sc, sl = 0.0, 0.0
    base = rounds_of(runs[0]["trace"])
    t0 = runs[0]["trace"]
    for r in runs[1:]:
        rr = rounds_of(r["trace"])
        for rd, k in enumerate(dec):
            for i in range(k):
                a, b = base[rd][0] + i, rr[rd][0] + i
                for key, relf in (("chi2", chi2_rel_of), ("lam", lam_rel)):
                    x, ref = r["trace"][key][b], t0[key][a]
                    if np.isfinite(x) and np.isfinite(ref):
                        d = relf(x, ref)
                    else:                       # (zero_depth) values that are not finite have no spread when they are the same value, an infinite one otherwise
                        d = 0.0 if (np.isnan(x) and np.isnan(ref)) or x == ref else np.inf
                    if key == "chi2":
                        sc = max(sc, d)
                    else:
                        sl = max(sl, d)
    return sc, sl


def lambda_spread_at(runs, rd, i):
    """the oracle's own lambda spread at decided iteration i of round rd"""
    t0, s0 = runs[0]["trace"], rounds_of(runs[0]["trace"])[rd][0]
    return max(lam_rel(r["trace"]["lam"][rounds_of(r["trace"])[rd][0] + i], t0["lam"][s0 + i]) for r in runs[1:])


def pose_excess(T, ref, start):
    """|T - ref| beyond two float32 ulps of the largest entry (the allowance of tests/test_gpu_lm.py's _check_updates: the outputs are float32), relative to the
    largest update |ref - start|"""
    ref64 = ref.astype(np.float64)
    upd = max(np.abs(ref64 - start.astype(np.float64)).max(), 1e-6)
    ulp = float(np.spacing(np.abs(ref).max().astype(np.float32)))
    return max(float(np.abs(T.astype(np.float64) - ref64).max()) - 2 * ulp, 0.0) / upd


def pose_band(runs, prob):
    """the oracle's own band on the pose: the largest pose_excess of its perturbed runs against its base run"""
    return max(pose_excess(r["Tcw"], runs[0]["Tcw"], prob["Tcw"]) for r in runs[1:])


def accepted(trace, s, i):
    """did iteration s + i of the round that begins at s end on an ACCEPTED trial?  After q - 1 rejections lambda stands at 2 * 4 * ... times its value before the
    iteration; an accepted trial multiplies it by at most 2 / 3, a rejected one by the next power of two.  Unknown (None) at a round's first iteration: lambda_0 is not
    in the trace."""
    if i == 0:
        return None
    q = int(trace["trials"][s + i])
    before = trace["lam"][s + i - 1]
    for j in range(q - 1):
        before *= 2.0 ** (j + 1)
    return bool(trace["lam"][s + i] < before)


def stats(name_n, runs, dec):
    """what the decided prefixes of one scene hold: iterations with 2 - 5 and with 6 - 9 trials, rounds that end on an accepted retrial that is not the last of its
    candidate batch (the kernel then re-evaluates that pose: kRefresh), decided iterations with more than one trial per round"""
    t = runs[0]["trace"]
    nb = min(POSE_CAND, waves(name_n))
    batched = name_n <= 2048          # (the global-memory variant beyond evaluates its trials one by one)
    few = many = refresh = 0
    per_round = [0, 0, 0, 0]
    refresh_rounds = []
    for rd, ((s, e), k) in enumerate(zip(rounds_of(t), dec)):
        for i in range(k):
            q = int(t["trials"][s + i])
            few += 2 <= q <= 5
            many += 6 <= q <= 9
            per_round[rd] += q > 1
        if k == e - s and k > 0:          # the round's last iteration is decided
            q = int(t["trials"][e - 1])
            if batched and q > 1 and accepted(t, s, k - 1):
                first = 2 + ((q - 2) // nb) * nb                      # the batch that holds trial q: trials first .. first + size - 1
                size = min(nb, LM_MAX_TRIALS - (first - 1))
                if q < first + size - 1:
                    refresh += 1
                    refresh_rounds.append(rd + 1)
    return dict(few=few, many=many, refresh=refresh, per_round=per_round, refresh_rounds=refresh_rounds)


def _close(a, ref, rel, relf):
    """a value that is not finite must be the same value on both sides"""
    if not (np.isfinite(a) and np.isfinite(ref)):
        return (np.isnan(a) and np.isnan(ref)) or a == ref
    return relf(a, ref) <= rel


def compare_rounds(trace, ref, dec, chi2_rel, lambda_rel):
    """`trace` against the oracle's `ref` on the decided iterations `dec` of ref: the same rounds (a round without iterations is one on both sides), the same trial
    counts, chi2 and lambda within the bounds.  Returns the list of differences (empty: agreement) and the largest chi2 / lambda differences seen."""
    bad, worst_c, worst_l = [], 0.0, 0.0
    ra, rb = rounds_of(trace), rounds_of(ref)
    if len(ra) != len(rb):
        return ["%d rounds, the oracle %d" % (len(ra), len(rb))], worst_c, worst_l
    for rd, ((s, e), (so, eo)) in enumerate(zip(ra, rb)):
        if (e > s) != (eo > so):
            bad.append("round %d: %d iterations, the oracle %d" % (rd + 1, e - s, eo - so))
            continue
        for i in range(dec[rd]):
            if s + i >= e:
                bad.append("round %d ends after %d iterations, the oracle's decided prefix has %d" % (rd + 1, e - s, dec[rd]))
                break
            if int(trace["trials"][s + i]) != int(ref["trials"][so + i]):
                bad.append("round %d iteration %d: %d trials, the oracle %d" % (rd + 1, i, trace["trials"][s + i], ref["trials"][so + i]))
                break
            c, co, lm, lo = trace["chi2"][s + i], ref["chi2"][so + i], trace["lam"][s + i], ref["lam"][so + i]
            if np.isfinite(c) and np.isfinite(co):
                worst_c = max(worst_c, chi2_rel_of(c, co))
            if np.isfinite(lm) and np.isfinite(lo):
                worst_l = max(worst_l, lam_rel(lm, lo))
            if not _close(c, co, chi2_rel, chi2_rel_of):
                bad.append("round %d iteration %d: chi2 %r, the oracle %r" % (rd + 1, i, c, co))
            if not _close(lm, lo, lambda_rel, lam_rel):
                bad.append("round %d iteration %d: lambda %r, the oracle %r" % (rd + 1, i, lm, lo))
    return bad, worst_c, worst_l
