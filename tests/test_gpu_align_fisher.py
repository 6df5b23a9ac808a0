"""Gauss-Newton SparseImgAlign's chi2 and H (the Fisher information getFisherInformation() returns,
SparseImageAlign.h:62-66) on the GPU against the oracle, on every kernel path.

chi2 lands in every result slot (header word 9) and H is the last linearisation's J^T J; neither is
a by-product of the pose.  The register kernel keeps a small state machine for which H that is
(csrc/align.hip AlignPairLds::hsrc / Hpk / Hvis / out_it): Hvis when every feature stayed inside the
level in the last residual pass, Hvis less the out-of-bounds features' H_f (Hpk) when one left;
sparse_align_generic holds its own copy.  A wrong source or a stale iteration's H leaves the pose
and n_visible as they are, so every case here computes `oob_last` (the features of the last level's
set that the last pass found out of the image) and each family asserts it has cases with
oob_last == 0 and with oob_last > 0.

Tolerances (tests/_align_cases.py, measured by tests/test_cpu_align_fisher.py on the oracle alone):
H_TOL = 1.0e-4 on max_ij |dH_ij| / sqrt(H_ii H_jj) (4 x the oracle's permutation floor 2.5e-5; below
half an average feature's share 1 / (2 n_visible) >= 2.68e-4), CHI2_TOL = 4.0e-5 relative (4 x the
floor 1.0e-5).  H must be exactly symmetric and n_visible equal.

Observed on the MI355X (worst over the family; each test prints its figures under -s):
    single frame (9 cases)   chi2 6.7e-6   H 1.65e-5    oob_last 1, 1, 6 at s0x3, s1x3, s2x4
    generic path (2 cases)   chi2 1.45e-5  H 3.19e-5    oob_last 4 at g6x4
    batch (19 pairs)         chi2 1.47e-5  H 3.53e-5    oob_last 2, 4, 1, 6 at b31s8 and 7, 8 at bgens8
"""
import numpy as np
import pytest

import _align_cases as A
import _scenes as S
from test_gpu_align import POSE_TOL, align_case
from test_gpu_align_batch import run_batch_align

pytestmark = pytest.mark.gpu


def check_record(what, chi2, H, n_visible, ores):
    """chi2, all 36 entries of H, H's symmetry and n_visible against the oracle's result."""
    H = np.asarray(H, np.float32).reshape(6, 6)
    assert n_visible == ores.n_visible, f"{what}: n_visible {n_visible} vs {ores.n_visible}"
    assert np.array_equal(H, H.T), f"{what}: H is not symmetric"
    dc, dh = A.chi2_dev(chi2, ores.chi2), A.h_dev(H, ores.H[:])
    print(f"{what}: n_visible {n_visible}, chi2 dev {dc:.2e}, H dev {dh:.2e}")
    assert dc <= A.CHI2_TOL, f"{what}: chi2 {chi2} vs {ores.chi2} (relative {dc:.2e})"
    assert dh <= A.H_TOL, f"{what}: H differs from the oracle's by {dh:.2e} (normalised)"
    return dc, dh


# oob_last of every single-frame case on the oracle (tests/test_cpu_align_fisher.py asserts that each
# family has both kinds): 0 -> the result's H is Hvis (hsrc = 0), > 0 -> Hvis less the lost features' H_f
SINGLE_OOB = {"s0": 0, "s1": 0, "s2": 0, "s3": 0, "s0x3": 1, "s1x3": 1, "s2x4": 6, "s5u30": 0, "s7l22": 0}
GENERIC_OOB = {"g6": 0, "g6x4": 4}


def run_single(gpu, name, kw, want_oob):
    res, ores, _, case = align_case(gpu, full=True, **kw)
    check_record(name, res.chi2, res.H[:], res.n_visible, ores)
    gq, gt = res.T_cur_ref.as_arrays()
    assert S.se3_log_inf(gq, gt, np.array(ores.T.q[:]), np.array(ores.T.t[:])) <= POSE_TOL, name
    oob = A.case_oob(case, ores)
    print(f"{name}: oob_last {oob}")
    assert oob == want_oob, f"{name}: oob_last {oob}, expected {want_oob}: the case no longer reaches its H source"


def test_single_case_sets_cover_both_h_sources():
    assert set(SINGLE_OOB) == {n for n, _ in A.SINGLE_CASES} and set(GENERIC_OOB) == {n for n, _ in A.GENERIC_CASES}
    for fam in (SINGLE_OOB, GENERIC_OOB):
        assert min(fam.values()) == 0 and max(fam.values()) > 0


@pytest.mark.parametrize("name,kw", A.SINGLE_CASES, ids=[n for n, _ in A.SINGLE_CASES])
def test_gn_chi2_and_fisher_single_frame(gpu, name, kw):
    """k_sparse_align_reg through ygzfe_sparse_align (<= 960 features): small and large motions,
    30 % usable, a single level."""
    run_single(gpu, name, kw, SINGLE_OOB[name])


@pytest.mark.parametrize("name,kw", A.GENERIC_CASES, ids=[n for n, _ in A.GENERIC_CASES])
def test_gn_chi2_and_fisher_generic_path(gpu, name, kw):
    """sparse_align_generic (~1,900 features > 960): its own H copy, with and without a lost feature."""
    run_single(gpu, name, kw, GENERIC_OOB[name])


def test_gn_no_usable_point_leaves_the_oracles_record(gpu):
    """No usable map point: the record equals whatever the oracle leaves.  That is H all zero,
    n_visible 0 and chi2 = NaN (not the reset value 1e10: the first pass divides a zero sum by zero
    measurements, the all-zero system solves to x = 0, which is no rollback, and the loop ends on
    |x| <= eps with chi2_ = 0 / 0; NLSSolver_impl.hpp:18-91)."""
    res, ores, _ = align_case(gpu, 6, n_usable_frac=0.0)
    print(f"no usable point: GPU chi2 {res.chi2}, oracle chi2 {ores.chi2}")
    assert ores.n_visible == 0 and not np.any(np.array(ores.H[:]))
    assert res.n_visible == 0
    assert res.chi2 == ores.chi2 or (np.isnan(res.chi2) and np.isnan(ores.chi2)), (res.chi2, ores.chi2)
    assert np.array_equal(np.array(res.H[:], np.float32), np.zeros(36, np.float32))


# batches whose pairs all keep every feature in the last pass, and batches with a pair that loses one
BATCH_ALL_IN = ("b31", "b20", "bgen")
BATCH_SOME_OUT = ("b31s8", "bgens8")


@pytest.mark.parametrize("name,kw", A.BATCH_CASES, ids=[n for n, _ in A.BATCH_CASES])
def test_gn_chi2_and_fisher_batch(gpu, name, kw):
    """ygzfe_batch_sparse_align's [P, 45] records (q, t, n_visible, chi2, H): levels 3..1 at strides
    1 and 8, levels 2..0 (the level-0 register kernel), the over-960 generic batch at both strides,
    partially usable map points."""
    _, nvis, rec, ores, cases = run_batch_align(gpu, full=True, **kw)
    worst_c = worst_h = 0.0
    oob = []
    for p, (o, c) in enumerate(zip(ores, cases)):
        dc, dh = check_record(f"{name}[{p}]", rec[p, 8], rec[p, 9:45], int(nvis[p]), o)
        oob.append(A.case_oob(c, o))
        worst_c, worst_h = max(worst_c, dc), max(worst_h, dh)
    print(f"{name}: worst chi2 dev {worst_c:.2e}, worst H dev {worst_h:.2e}, oob_last {oob}")
    if name in BATCH_SOME_OUT:
        assert max(oob) > 0, f"{name}: no pair lost a feature in its last residual pass"
    if name in BATCH_ALL_IN:
        assert max(oob) == 0, (name, oob)
