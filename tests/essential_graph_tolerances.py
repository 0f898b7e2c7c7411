"""The bounds of the OptimizeEssentialGraph parity tests that lm_tolerances.py does not already hold (tests/test_gpu_essential_graph.py imports every number it
uses from there and from here; it carries no literal tolerance of its own).

The pose bound is lm_tolerances.UPDATE_REL times the largest |yardstick - input| over the graph: the yardstick's own band under a one-ulp change of its inputs or a
permuted elimination order is 8.1e-6 of the update at most (profiles/essential_graph_bands.txt, written by tools/essential_graph_bands.py), so no case is banded."""
from lm_tolerances import CHAOTIC_BANDS_ALLOWED

# chi2 of the last iteration, relative: the bound is not known in advance, so it is the yardstick's own relative spread ON THE CASE UNDER TEST over ulp_perturbed
# seeds 0..3 and a permuted elimination order (the fifth column of profiles/essential_graph_bands.txt, copied here case by case;
# tests/test_essential_graph_reference_cpu.py keeps the table equal to that file) times CHAOTIC_BANDS_ALLOWED.  The cases with a free scale stop after the one
# Gauss-Newton step that a perturbation moves by ~1e-6; those with a fixed scale end at the noise floor, where the yardstick agrees with itself to ~1e-11.
CHI2_LAST_SPREAD = {
    "dup2-fs0": 2.914e-13,
    "dup2-fs1": 1.272e-13,
    "ring9-fs0": 6.198e-07,
    "ring9-fs1": 5.327e-12,
    "ring10-fs0": 1.598e-06,
    "ring10-fs1": 3.393e-11,
    "ring65-fs0": 8.724e-07,
    "ring65-fs1": 1.131e-11,
    "ring66-fs0": 8.528e-07,
    "ring66-fs1": 5.406e-12,
    "ring40-fs0": 1.218e-06,
    "ring40-fs1": 2.510e-11,
    "reversed-fs0": 1.244e-06,
    "reversed-fs1": 4.919e-12,
    "fixed_middle-fs0": 5.857e-07,
    "fixed_middle-fs1": 1.197e-11,
    "fixed_last-fs0": 9.899e-07,
    "fixed_last-fs1": 2.021e-12,
    "hub-fs0": 2.042e-07,
    "hub-fs1": 9.686e-13,
    "edges63-fs0": 4.260e-07,
    "edges63-fs1": 3.301e-12,
    "edges64-fs0": 5.406e-07,
    "edges64-fs1": 2.781e-12,
    "edges65-fs0": 9.083e-07,
    "edges65-fs1": 1.618e-11,
    "edges257-fs0": 3.487e-07,
    "edges257-fs1": 1.855e-12,
    "isolated-fs0": 1.090e-06,
    "isolated-fs1": 1.075e-11,
    "drift_small-fs0": 2.657e-06,
    "drift_small-fs1": 1.178e-11,
    "drift_large-fs0": 5.050e-06,
    "drift_large-fs1": 3.179e-11,
    "unit_scale-fs0": 1.366e-06,
    "unit_scale-fs1": 1.301e-12,
    "scale_drift-fs0": 1.105e-06,
    "scale_drift-fs1": 7.638e-12,
    "star-fs0": 4.937e-14,
    "star-fs1": 1.148e-14,
    "straddle_far-fs0": 1.172e-06,
    "straddle_far-fs1": 4.153e-12,
    "ring300-fs0": 4.049e-06,
    "ring300-fs1": 1.337e-11,
}


def chi2_last_rel(case_id):
    return CHAOTIC_BANDS_ALLOWED * CHI2_LAST_SPREAD[case_id]


# Tiw and Xw_corrected against their recomputation in numpy from the device's own Scw: the double arithmetic is far below a float32 ulp, only a rounding straddle differs
DERIVED_FLOAT_ULPS = 1
