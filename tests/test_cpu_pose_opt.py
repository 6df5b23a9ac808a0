"""The restatement of Optimizer::PoseOptimization (tests/_pose_opt.py) held from the sides that need no
GPU, and the conditions on the fixed cases that keep tests/test_gpu_pose_opt.py honest.

Measured floors (the restatement against itself under three edge permutations and two other summation
orders, worst over the cases; the asserted constants are these figures rounded up):
  pose (se3-log inf-norm of the double pose)   POSE_FLOOR = 2.2e-14   -> POSE_TOL  = 8.8e-14
  per-round chi2, relative                     CHI2_FLOOR = 1.9e-11   -> CHI2_RTOL = 7.6e-11
CHI2_ATOL = 1e-10 stands beside CHI2_RTOL because a round's chi2 can be a rounding residue (a mono
problem of 3 points has 6 equations for 6 unknowns and ends near 1e-28; the last round of the 'far'
case ends near 1e-19): the sums that form it start near 1e4..1e5, where one ulp is ~1e-11."""
import numpy as np
import pytest

import _pose_opt as P


def _sys_at(sc, R, huber):
    """b and H of the level-0 edges of the last round at the result pose."""
    pr = sc["present"].astype(bool)
    idx = np.nonzero(pr)[0]
    E = P._Edges(sc["cam"], sc["bf"], sc["kps_xy"][idx], sc["octave"][idx], sc["u_right"][idx], sc["xw"][idx],
                 sc["inv_level_sigma2"], set())
    act = ~R.outlier_rounds[-2][idx] if R.rounds > 1 else np.ones(len(idx), bool)
    e0, e1, e2, chi2, xyz = E.errors(R.q, R.t)
    w = E.robust(chi2, huber)[1][act]
    J = E.jacobians(xyz)[:, :, act]
    H = np.einsum("rik,k,rjk->ij", J, w * E.s[act], J)
    b = -np.einsum("rik,k,rk->i", J, w * E.s[act], np.stack([e0, e1, e2])[:, act])
    return H, b


GRID = [c for c in P.CASE_IDS if c not in P.SPECIAL]


@pytest.mark.parametrize("cid", [c for c in GRID if int(c.split("-")[1]) >= 63])
def test_planted_truth_is_recovered(cid):
    """Inlier noise <= 0.5 px, outliers >= 30 px off: the final flags are the planted ones and the pose is
    within the noise-implied bound: a pixel error of e moves a point at depth z by e z / f, so the pose
    cannot be further off than noise * z_max / f (12 m / 457 px) in translation, noise / f in rotation,
    each taken with a factor 4 for the conditioning of 6 DoF over the image."""
    sc, R = P.case(cid)
    pr = sc["present"].astype(bool)
    assert sc["noise"] <= 0.5
    assert np.array_equal(R.outlier[pr].astype(bool), sc["planted"][pr])
    assert R.n_inliers == int((~sc["planted"][pr]).sum())
    bound = 4 * sc["noise"] * 12.0 / 457.0
    assert P.se3_log_inf(R.q, R.t, sc["q_gt"], sc["t_gt"]) <= bound


@pytest.mark.parametrize("cid", ["mono-255", "stereo-256", "mixed-1000", "mixed-2500"])
def test_first_order_optimality(cid):
    sc, R = P.case(cid)
    H, b = _sys_at(sc, R, huber=False)       # the last round runs without the kernel
    assert np.abs(b).max() <= 1e-6 * np.abs(H).max()


def test_preconditions_of_the_gpu_cases():
    rejected = recovered = three_bad = ten_iters = one_round = empty = False
    for cid in P.CASE_IDS:
        sc, R = P.case(cid)
        th = np.where(sc["u_right"] < 0, np.float64(P.TH_MONO), np.float64(P.TH_STEREO))
        for chi in R.edge_chi2:
            ok = ~np.isnan(chi)
            assert np.all(np.abs(chi[ok] - th[ok]) >= 1e-5), cid
        rejected |= sum(R.rejected) > 0
        if R.rounds > 1:
            recovered |= bool(np.any(R.outlier_rounds[0] & ~R.outlier_rounds[-1]))
        three_bad |= "nbad" in R.stops
        ten_iters |= 10 in R.iters
        one_round |= 3 <= R.n_corr < 10 and R.rounds == 1
        empty |= R.rounds == 4 and R.iters[1:] == [0, 0, 0]
    assert rejected and recovered and three_bad and ten_iters and one_round and empty
    sc, R = P.case("far")
    assert sum(R.rejected) > 0 and 10 in R.iters and np.any(R.outlier_rounds[0] & ~R.outlier_rounds[-1])


def test_floor():
    """iters[] / rejected[] / flags of every case depend neither on the edge order nor on how the sums are
    formed (np.sum, reversed, or the lane / butterfly / wave tree of a strided workgroup loop), and the
    tolerances of the GPU test are at least 4 x the worst difference that a mere reordering of the sums
    makes.  A seed at which the counts move under any of these is not a case: the device cannot be asked
    to reproduce a count that the restatement itself does not keep."""
    worst_pose = worst_chi = 0.0
    for cid in P.CASE_IDS:
        sc, R = P.case(cid)
        runs = [(P.permuted(sc, ps), "numpy") for ps in (1, 2, 3)]
        runs += [(dict(sc, perm=np.arange(len(sc["present"]))), o) for o in ("tree", "reverse")]
        runs += [(P.permuted(sc, 1), "tree")]
        for sp, order in runs:
            Rp = P.pose_optimization(*P.call_args(sp), order=order)
            assert (Rp.rounds, Rp.iters, Rp.rejected) == (R.rounds, R.iters, R.rejected), (cid, order)
            assert np.array_equal(Rp.outlier, R.outlier[sp["perm"]]), (cid, order)
            worst_pose = max(worst_pose, P.se3_log_inf(Rp.q, Rp.t, R.q, R.t))
            for a, b in zip(Rp.chi2, R.chi2):
                if abs(a - b) > P.CHI2_ATOL:
                    worst_chi = max(worst_chi, abs(a - b) / abs(b))
    print("floors: pose", worst_pose, "chi2 (relative, beyond CHI2_ATOL)", worst_chi)
    assert worst_pose <= P.POSE_FLOOR and worst_chi <= P.CHI2_FLOOR
    assert 4 * P.POSE_FLOOR <= P.POSE_TOL and 4 * P.CHI2_FLOOR <= P.CHI2_RTOL


def _differs(R, M):
    if not np.array_equal(R.outlier, M.outlier):
        return True
    return P.se3_log_inf(M.q, M.t, R.q, R.t) > 100 * P.POSE_TOL


@pytest.mark.parametrize("mut", ["no_huber", "huber_round4", "right_update", "chain_rounds", "no_rho_eps"])
def test_mutation_shows_on_a_case(mut):
    for cid in ("far", "mixed-255", "stereo-64", "mixed-63", "stereo-3"):
        sc, R = P.case(cid)
        if _differs(R, P.pose_optimization(*P.call_args(sc), mut=(mut,))):
            return
    pytest.fail(f"mutation {mut} changes neither a flag nor the pose on any case")


def _one_edge(stereo, tx):
    """One edge seen from the double pose (identity rotation, translation (tx, 0, 0)): no optimisation runs."""
    xw = np.array([[0.3, -0.2, 5.0]], np.float32)
    fx, fy, cx, cy = P.CAM
    u, v = fx * 0.3 / 5.0 + cx, fy * -0.2 / 5.0 + cy
    obs = np.array([[u + 2.3, v + 1.2]], np.float32)
    ur = np.array([u - P.BF / 5.0 + 1.1 if stereo else -1.0], np.float32)
    chis = []
    for mut in ((), ("double_invz",)):
        E = P._Edges(P.CAM, P.BF, obs, np.array([0]), ur, xw, P.INV_LEVEL_SIGMA2, set(mut))
        chis.append(E.errors(np.array([0.0, 0.0, 0.0, 1.0]), np.array([tx, 0.0, 0.0]))[3][0])
    return chis, np.array([stereo])


def _cross(stereo, th):
    """The translation at which the edge's chi2 (float invz) crosses th, by bisection on the double pose."""
    lo, hi = 0.0, 0.02
    assert _one_edge(stereo, lo)[0][0] > th > _one_edge(stereo, hi)[0][0]
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _one_edge(stereo, mid)[0][0] > th:
            lo = mid
        else:
            hi = mid
    return lo


def test_double_threshold_mutation_on_a_crafted_edge():
    """(double)5.991f is 5.99100017..., so a chi2 between 5.991 and that is an inlier by the reference's float
    compare and an outlier by a double one.  The window is 1.75e-7 wide and no edge of the scenes falls into it,
    so the edge is crafted, as the issue foresees: one mono edge whose chi2 is brought to the middle of the
    window by bisection on the translation of the (double) pose it is classified at."""
    target = 0.5 * (5.991 + float(np.float64(P.TH_MONO)))
    tx = _cross(False, target)
    (chi, _), stereo = _one_edge(False, tx)
    assert 5.991 < chi < float(np.float64(P.TH_MONO))
    chi = np.array([chi])
    assert not P.classify(chi, stereo)[0] and P.classify(chi, stereo, ("double_threshold",))[0]


def test_double_invz_mutation_on_a_crafted_edge():
    """The float invz of the stereo edge (.cpp:309) moves its chi2 by ~1e-6 relative, which changes no flag of
    the scenes; so the edge is crafted: one stereo edge brought to the threshold by bisection on the pose's
    translation, where rounding invz to float or not decides the flag."""
    th = float(np.float64(P.TH_STEREO))
    tx = _cross(True, th)
    differ = 0
    for k in range(-200, 201):
        (cf, cd), stereo = _one_edge(True, tx + k * 1e-10)
        differ += P.classify(np.array([cf]), stereo)[0] != P.classify(np.array([cd]), stereo)[0]
    (cf, cd), _ = _one_edge(True, tx)
    assert cf != cd and differ > 0, (cf, cd, differ)
