"""The bounds of the triangulation parity tests (tests/test_gpu_triangulation.py imports every number it uses from here; it carries no literal tolerance of its
own).  They are the `constant` lines of profiles/triangulation_bands.txt, written by tools/triangulation_bands.py from the yardstick alone
(tests/test_triangulation_reference_cpu.py keeps this file equal to that one and to the probe, and holds the condition on the friendly scenes)."""

# |dX| / |X - Ow1| of an accepted point against the yardstick's: the largest movement between yardstick variants (float64 eigh against OpenCV's float32 one-sided
# Jacobi; every float input one ulp up or down, seeds 0..3) over the friendly scenes, times 4 -- the device sums A^T A and the dot products in its own order and
# solves with a cyclic Jacobi in double, which may differ from both variants.  The scene 100 m from the origin sets it: a float32 coordinate of 100 resolves 8e-6.
X3D_REL = 7.772e-04

# The same, from each friendly scene's own rows of that file.  The scenes at the origin spread some 50 times less than the far one, and a summation in float in place
# of double would pass them at X3D_REL: every comparison of a scene that has an entry here uses it (X3D_REL remains for scenes the probe does not measure).
# low_parallax accepts no pair, so nothing of it is compared.
X3D_REL_BY_SCENE = {"wide_mono": 2.527e-05, "stereo_mix": 1.125e-05, "low_parallax": 0.000e+00, "single_pair": 8.604e-06, "twenty": 7.772e-04}


def x3d_rel(scene):
    return X3D_REL_BY_SCENE.get(scene, X3D_REL)

# A pair whose yardstick margin to ANY comparison upstream evaluates for it (parallax, depth, reprojection, scale; relative, as gates_after_point and
# point_and_branch define them) is smaller than this is left out of the verdict parity: the largest movement of such a margin between the same variants, times 4.
# The replay of the device's own points through gates_after_point leaves nothing out.
MARGIN_REL = 2.526e-03

# the condition the friendly scenes are held to (not a measurement): share of their pairs inside MARGIN_REL of a comparison
IN_MARGIN_MAX_SHARE = 0.01
