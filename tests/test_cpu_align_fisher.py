"""The noise floor of the oracle's Gauss-Newton chi2 / H and the sensitivity of the H check
(no GPU): what tests/test_gpu_align_fisher.py's tolerances rest on.

H = sum over the features in bounds in the last residual pass of J_f^T J_f with J from the
reference patches only (oracle/align.c:232-236), so two correct implementations that agree on
n_visible differ in H by f32 summation order.  The floor is the oracle against itself with the
features permuted (kps / xyz / usable consistently; 3 fixed permutations per case).

Measured (all of _align_cases' SINGLE / GENERIC / BATCH cases, 30 runs):
  H floor    max 2.50e-5 (generic single frame, 1,863 features); <= 960 features 1.26e-5; batch 1.49e-5
  chi2 floor max 9.59e-6 (single frame seed 2)
  -> H_TOL = 4 x 2.5e-5 = 1.0e-4, CHI2_TOL = 4 x 1.0e-5 = 4.0e-5; the cap 1 / (2 n_visible) is
     >= 2.68e-4 in every case.
Sensitivity: one visible feature cleared, 8 per case by a fixed RNG: 230 of the 240 removals move H
by more than H_TOL, at least 5 of the 8 in every case (the others are weak-gradient features whose
J^T J is below the summation noise, which no tolerance above the floor can see).
"""
import numpy as np
import pytest

import _align_cases as A

PERM_SEEDS = (101, 202, 303)
N_SENS = 8


def _all_cases():
    for name, kw in A.SINGLE_CASES + A.GENERIC_CASES:
        yield name, A.single_inputs(**kw)
    for name, kw in A.BATCH_CASES:
        for p, c in enumerate(A.batch_inputs(**kw)):
            yield f"{name}[{p}]", c


@pytest.fixture(scope="module")
def runs():
    return [(name, c, A.oracle_run(c)) for name, c in _all_cases()]


def test_oracle_gn_floor_fits_the_tolerances(runs):
    h_floor = c_floor = 0.0
    for name, c, o in runs:
        H0 = np.array(o.H[:])
        assert np.array_equal(H0.reshape(6, 6), H0.reshape(6, 6).T), name  # the oracle's own H is symmetric
        for s in PERM_SEEDS:
            p = np.random.default_rng(s).permutation(len(c["kps"]))
            r = A.oracle_run(c, c["kps"][p], c["xyz"][p], c["usable"][p])
            assert r.n_visible == o.n_visible, name
            h_floor = max(h_floor, A.h_dev(r.H[:], H0))
            c_floor = max(c_floor, A.chi2_dev(r.chi2, o.chi2))
        # half an average feature's share of H
        assert A.H_TOL <= 1.0 / (2 * o.n_visible), f"{name}: H_TOL {A.H_TOL} over the cap at n_visible {o.n_visible}"
    print(f"oracle floors over {len(runs)} runs: H {h_floor:.3e}, chi2 {c_floor:.3e}")
    # the recorded floors are what was measured (and not stale by more than 2x)
    assert A.H_FLOOR / 2 <= h_floor <= A.H_FLOOR, h_floor
    assert A.CHI2_FLOOR / 2 <= c_floor <= A.CHI2_FLOOR, c_floor
    assert A.H_TOL == 4 * A.H_FLOOR and A.CHI2_TOL == 4 * A.CHI2_FLOOR and A.CHI2_TOL <= 1e-3


def test_h_tolerance_sees_one_feature(runs):
    """Clearing one visible feature moves H by more than H_TOL for most features."""
    seen = tried = 0
    for name, c, o in runs:
        lv = c["pyr_ref"][c["min_level"]]
        vis = np.flatnonzero(A.in_border(c["kps"], c["usable"], lv.shape[1], lv.shape[0],
                                         c["orc"].inv_scale[c["min_level"]]))
        hit = 0
        for i in np.random.default_rng(7).choice(vis, N_SENS, replace=False):
            u = c["usable"].copy()
            u[i] = 0
            hit += A.h_dev(A.oracle_run(c, usable=u).H[:], o.H[:]) > A.H_TOL
        assert hit >= 5, f"{name}: only {hit} of {N_SENS} single-feature removals exceed H_TOL"
        seen += hit
        tried += N_SENS
    print(f"single-feature removals above H_TOL: {seen} of {tried}")
    assert seen >= 0.8 * tried, (seen, tried)


def test_case_sets_reach_the_out_of_bounds_h(runs):
    """oob_last (features of the last level's set out of the current image in the last residual
    pass) is 0 in some and > 0 in other cases of each family: both H sources of the kernels."""
    oob = {name: A.case_oob(c, o) for name, c, o in runs}
    print("oob_last:", {k: v for k, v in oob.items() if v})
    assert (oob["s0x3"], oob["s1x3"], oob["s2x4"]) == (1, 1, 6)
    for fam in ("s", "g", "b"):
        vals = [v for k, v in oob.items() if k.startswith(fam)]
        assert min(vals) == 0 and max(vals) > 0, (fam, vals)
    assert max(v for k, v in oob.items() if k.startswith("b31s8")) > 0
    assert max(v for k, v in oob.items() if k.startswith("bgens8")) > 0
