"""Gauss-Newton SparseImgAlign cases shared by tests/test_cpu_align_fisher.py (the oracle's own
noise floor, no GPU) and tests/test_gpu_align_fisher.py (the kernels' chi2 / H against the oracle).

The inputs are built on the CPU only: the oracle's extraction is bit-identical to the GPU's
(tests/test_gpu_extract.py), so `single_inputs` / `batch_inputs` give the very keypoints that
test_gpu_align.align_case / test_gpu_align_batch.run_batch_align hand to the kernels.

Why H can be compared tightly.  In the reference (and oracle/align.c:232-236) the Jacobians come
from the reference patches only and the weights are unit, so H = sum_f J_f^T J_f depends on the
pose only through the SET of features in bounds in the last residual pass.  With equal n_visible
the GPU's H and the oracle's differ by f32 summation order alone.  That floor is measured on the
oracle itself by permuting the features (test_cpu_align_fisher.py), with 3 fixed permutations per case.
Largest figures per family (H deviations are max_ij |dH_ij| / sqrt(H_ii H_jj), chi2 deviations
|dchi2| / max(1, |chi2|)):

    case family                                    H floor   chi2 floor   n_visible
    single frame, <= 960 features (9 cases)        1.26e-5   9.59e-6      289 .. 937
    single frame, generic (2 cases)                2.50e-5   9.24e-6      1863, 1867
    batch pairs (19 pairs of 6 batches)            1.49e-5   8.76e-6      379 .. 1869

H_TOL = 4 x 2.5e-5 = 1.0e-4 stays under 1 / (2 n_visible) >= 2.68e-4 (half an average feature's
share of H) for every case.  Sensitivity: clearing one visible feature (8 per case, fixed RNG) moves
H by more than H_TOL for 230 of the 240 features tried (the others are weak-gradient features whose
J^T J is below the summation noise); every case has at least 5 of its 8 above it.
"""
import numpy as np

import _oracle as O
import _scenes as S

BORDER = 3  # patch half size 2 + 1 (SparseImageAlign.cc:64, oracle/align.c:280)
XI = np.array([0.012, -0.006, 0.009, 0.0025, -0.002, 0.0015], np.float32)  # test_gpu_align_batch.XI

# Largest floors measured on the oracle (see the table above) and the tolerances derived from them.
H_FLOOR = 2.5e-5
CHI2_FLOOR = 1.0e-5
H_TOL = 4 * H_FLOOR         # 4 x the floor: the kernels' other reduction tree and fused products
CHI2_TOL = 4 * CHI2_FLOOR   # tightened from the project's 1e-3 (test_gpu_align_lm.py); the GPU meets it


def h_dev(H, H_ref):
    """max_ij |H_ij - Href_ij| / sqrt(Href_ii Href_jj); 0 for two all-zero matrices."""
    H = np.asarray(H, np.float64).reshape(6, 6)
    R = np.asarray(H_ref, np.float64).reshape(6, 6)
    d = np.sqrt(np.abs(np.diag(R)))
    n = np.outer(d, d)
    diff = np.abs(H - R)
    if not n.any():
        return float(diff.max())  # an all-zero reference: any nonzero entry is a deviation
    assert (n > 0).all(), "reference H has a zero diagonal entry"
    return float((diff / n).max())


def chi2_dev(c, c_ref):
    return abs(float(c) - float(c_ref)) / max(1.0, abs(float(c_ref)))


def in_border(kps, usable, w, h, inv_scale):
    """Usable keypoints that pass the reference border test of a level (oracle/align.c:291-293)."""
    s = np.float32(inv_scale)
    ui = np.floor(kps["x"].astype(np.float32) * s).astype(np.int64)
    vi = np.floor(kps["y"].astype(np.float32) * s).astype(np.int64)
    ok = (ui - BORDER >= 0) & (vi - BORDER >= 0) & (ui + BORDER < w) & (vi + BORDER < h)
    return ok & (np.asarray(usable) != 0)


def oob_last(kps, usable, n_visible, w, h, inv_scale):
    """Features of the last level's set that the last residual pass found out of the current image."""
    return int(in_border(kps, usable, w, h, inv_scale).sum()) - int(n_visible)


def oracle_run(c, kps=None, xyz=None, usable=None):
    """The oracle's Gauss-Newton run on case c (optionally with replaced feature arrays)."""
    return O.sparse_align(c["pyr_ref"], c["pyr_cur"], c["orc"].inv_scale, c["ocam"],
                          c["kps"] if kps is None else kps, c["xyz"] if xyz is None else xyz,
                          c["usable"] if usable is None else usable, c["max_level"], c["min_level"],
                          O.se3_from((0, 0, 0, 1), (0, 0, 0)))


def case_oob(c, ores):
    lv = c["pyr_ref"][c["min_level"]]
    return oob_last(c["kps"], c["usable"], ores.n_visible, lv.shape[1], lv.shape[0], c["orc"].inv_scale[c["min_level"]])


def single_inputs(seed, n_usable_frac=1.0, max_level=3, min_level=1, motion_scale=1.0, nfeatures=None):
    """test_gpu_align.align_case's inputs, built with the oracle's extraction."""
    sc = S.PlaneScene(seed)
    W, H, nf, sf, nl, ini, mn = S.CONFIGS["C2"]
    nf = nfeatures or nf
    orc = O.OrbOracle(nf, sf, nl, ini, mn)
    q_ref = S.quat_from_rotvec([0.01, -0.02, 0.005]).astype(np.float32)
    t_ref = np.array([0.05, -0.03, 0.02], np.float32)
    v, w = S.motion(seed, motion_scale)
    q_d = S.quat_from_rotvec(w)
    q_cur, t_cur = S.se3_mul(q_d, v, q_ref.astype(np.float64), t_ref.astype(np.float64))
    f_ref = sc.render(q_ref, t_ref, seed * 2 + 1)
    f_cur = sc.render(q_cur.astype(np.float32), t_cur.astype(np.float32), seed * 2 + 2)
    pyr_ref, pyr_cur = orc.pyramid(f_ref), orc.pyramid(f_cur)
    kps, _ = orc.extract(pyr_ref)
    Pw, ok = sc.map_points(q_ref, t_ref, kps)
    xyz = np.array([S.quat_rot(q_ref.astype(np.float64), p) + t_ref for p in Pw], np.float32)
    rng = np.random.default_rng(seed)
    usable = (ok.astype(bool) & (rng.random(len(kps)) < n_usable_frac)).astype(np.uint8)
    return {"pyr_ref": pyr_ref, "pyr_cur": pyr_cur, "orc": orc, "ocam": O.Cam(*sc.cam), "kps": kps, "xyz": xyz,
            "usable": usable, "max_level": max_level, "min_level": min_level}


def batch_inputs(F, stride, max_level, min_level, usable_frac=1.0, seed=11, nfeatures=None):
    """test_gpu_align_batch.run_batch_align's pairs (k, k + 1), built with the oracle's extraction."""
    import ygzfe
    W, H, nf, sf, nl, ini, mn = S.CONFIGS["C2"]
    nf = nfeatures or nf
    sc = S.PlaneScene(seed, W, H)
    orc = O.OrbOracle(nf, sf, nl, ini, mn)
    poses = [ygzfe.trajectory_pose(k * stride, XI) for k in range(F)]
    pyrs = [orc.pyramid(sc.render(q, t, noise_seed=k)) for k, (q, t) in enumerate(poses)]
    rng = np.random.default_rng(seed)
    cases = []
    for p in range(F - 1):
        q, t = poses[p]
        kps, _ = orc.extract(pyrs[p])
        Pw, ok = sc.map_points(q, t, kps)
        xyz = np.array([S.quat_rot(q.astype(np.float64), w) + t for w in Pw], np.float32)
        usable = (ok.astype(bool) & (rng.random(len(kps)) < usable_frac)).astype(np.uint8)
        cases.append({"pyr_ref": pyrs[p], "pyr_cur": pyrs[p + 1], "orc": orc, "ocam": O.Cam(*sc.cam), "kps": kps,
                      "xyz": xyz, "usable": usable, "max_level": max_level, "min_level": min_level})
    return cases


# (name, single_inputs kwargs): the register kernel's single-frame cases (<= 960 features) ...
SINGLE_CASES = [
    ("s0", dict(seed=0)), ("s1", dict(seed=1)), ("s2", dict(seed=2)), ("s3", dict(seed=3)),
    ("s0x3", dict(seed=0, motion_scale=3.0)), ("s1x3", dict(seed=1, motion_scale=3.0)),
    ("s2x4", dict(seed=2, motion_scale=4.0)),
    ("s5u30", dict(seed=5, n_usable_frac=0.3)),
    ("s7l22", dict(seed=7, max_level=2, min_level=2)),
]
# ... and sparse_align_generic's (ORBextractor(2000): ~1,900 features)
GENERIC_CASES = [
    ("g6", dict(seed=6, nfeatures=2000)),
    ("g6x4", dict(seed=6, nfeatures=2000, motion_scale=4.0)),  # oob_last 0 at scales 1 and 2, 1 at 3, 4 at 4
]
# (name, batch_inputs kwargs): ygzfe_batch_sparse_align
BATCH_CASES = [
    ("b31", dict(F=6, stride=1, max_level=3, min_level=1)),
    # 8x the per-frame motion: at stride 4 no pair loses a feature in its last residual pass on the oracle
    ("b31s8", dict(F=5, stride=8, max_level=3, min_level=1)),
    ("b20", dict(F=3, stride=1, max_level=2, min_level=0)),
    ("bgen", dict(F=4, stride=1, max_level=3, min_level=1, nfeatures=2000, seed=5)),
    ("bgens8", dict(F=3, stride=8, max_level=3, min_level=1, nfeatures=2000, seed=5)),
    ("bpart", dict(F=4, stride=2, max_level=3, min_level=1, usable_frac=0.4, seed=3)),
]
