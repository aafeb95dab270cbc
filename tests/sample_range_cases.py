"""The cases the exact sampler and the exact marginals share between tests/test_class_sample_range_cpu.py and tests/test_gpu_class_sample_range.py at
the bottom of float64's range, as range_cases.py keeps the samplers': data and the few lines that turn a case into inputs, no tests, no fixtures.

A case is one call: a shape (code, L, lds_width), the rows of tests/test_class_law_range_cpu.py at that shape (both, the tied one first), one step of
a ladder of the tied row -- "row": the row's own, its total normal, subnormal, and past the last positive double; "class": its costliest class's, on
which every class is normal at step 0 and that class alone is subnormal at step 260 --, and the form of the weights: "w4" the four weights, "site" one
table for both rows, "rows" one table per syndrome (the second row's at the step before, so that the rows differ).  Its PREMISE is what the CPU test
asserts of the twin on it, so that the GPU file cannot go vacuous: the ranges the tied row's z crosses, and whether the host path answers for row 0 --
per class (every-class mode, class_marginals, exact_error_counts) and per row (posterior mode, posterior_marginals)."""
import numpy as np

TORIC, XZZX, ROTATED, PLANAR = 0, 1, 2, 3
K = 256
SEED = 20261021
# (code, L, lds_width): nothing held twice; toric L = 3 at width 6 holds seven generators and takes the pick kernel over partials and the combine over
# held assignments
SHAPES = [(ROTATED, 3, 0), (XZZX, 3, 0), (TORIC, 3, 6)]
STEPS = (("class", 0), ("class", 260), ("row", 0), ("row", 260), ("row", 300))  # the ladder's quantity at 1e-250, 1e-315 and 1e-325
FORMS = ("w4", "site", "rows")
CASES = [(code, L, lds_width, ladder, step, form) for code, L, lds_width in SHAPES for ladder, step in STEPS for form in FORMS]
# (ladder, step) -> (the ranges of the tied row's z, answered per class, answered per row)
PREMISE = {("class", 0): ({"normal"}, True, True), ("class", 260): ({"normal", "subnormal"}, False, True),
           ("row", 0): ({"normal", "zero"}, False, True), ("row", 260): ({"subnormal", "zero"}, False, False), ("row", 300): ({"zero"}, False, False)}
# the torus' sixteen classes spread over more costs: at a row total of 1e-250 some are subnormal already
PREMISE_OF = {TORIC: {**PREMISE, ("row", 0): ({"normal", "subnormal", "zero"}, False, True)}}


def premise_of(case):
    return PREMISE_OF.get(case[0], PREMISE)[case[3], case[4]]


def nq_of(code, L):
    return (2 if code in (TORIC, PLANAR) else 1) * L * L


def weights_of(case, ladders, w4_of):
    """(w, wq) of a case: w float64[4] with wq None, or wq float64[nq, 4] / [2, nq, 4] with w None.  ladders: {"row", "class"} -> the p of every step of
    that ladder of the tied row; w4_of: p -> the four weights"""
    code, L, _, ladder, step, form = case
    ladder_p = ladders[ladder]
    w4 = np.asarray(w4_of(ladder_p[step]), dtype=np.float64)
    if form == "w4":
        return w4, None
    if form == "site":
        return None, np.broadcast_to(w4, (nq_of(code, L), 4)).copy()
    other = np.asarray(w4_of(ladder_p[max(step - 1, 0)]), dtype=np.float64)
    return None, np.stack([np.broadcast_to(w4, (nq_of(code, L), 4)), np.broadcast_to(other, (nq_of(code, L), 4))]).copy()


def ranges_of(z):
    return {"normal" if v >= 2.0 ** -1022 else "subnormal" if v > 0 else "zero" for v in np.asarray(z, dtype=np.float64).reshape(-1).tolist()}
