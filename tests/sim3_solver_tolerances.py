"""The bounds of the Sim3Solver parity tests (tests/test_gpu_sim3_solver.py imports every number it uses from here; it carries no literal tolerance of its own).
All three are the `constant` lines of profiles/sim3_solver_bands.txt, written by tools/sim3_solver_bands.py from the yardstick alone
(tests/test_sim3_solver_reference_cpu.py keeps this file equal to that one and holds the two conditions on the friendly families)."""

# Relative eigen-gap (l1 - l2) / (|l1| + |l4|) of Horn's N below which a hypothesis is "ill-conditioned": a float32 eigen solve returns the eigenvector to about
# eps32 / gap, 6e-5 at this value -- below it two eigen solves return different answers, not different roundings of one.  Such a hypothesis is not compared with the
# yardstick's transform; its flags are still held, bit for bit, to CheckInliers on the device's own transform.
GAP_MIN = 1.000e-03

# |dT| / max |T| of T12 and T21 on conditioned hypotheses: the largest spread between yardstick variants (float64 eigh against float32 Jacobi; inputs under
# ulp_perturbed seeds 0..3) over all families, times lm_tolerances.CHAOTIC_BANDS_ALLOWED = 4 -- one float-rounding choice on the device (a cyclic Jacobi in double) may
# differ from both variants.
T12_REL = 1.723e-04

# (hypothesis, correspondence) pairs whose error lies closer than this to its gate, relative to the gate, are left out when flags are compared against the yardstick's
# OWN transform: the largest |d err| / gate between the same variants over pairs near their gate, times 4.
MARGIN_REL = 1.990e-02

# the conditions the scenes are held to (not measurements): share of conditioned hypotheses in every friendly family, share of pairs inside MARGIN_REL
CONDITIONED_MIN_SHARE = 0.90
IN_MARGIN_MAX_SHARE = 0.01
