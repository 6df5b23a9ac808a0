"""numpy float64 restatement of Optimizer::PoseOptimization(Frame*) (Optimizer.cc:1656-1842)
with the pieces of g2o and Sophus it runs, written from those sources:

  edges      types_six_dof_expmap.h:154-215, .cpp:272-377 (mono / stereo, OnlyPose)
  Huber      core/robust_kernel_impl.cpp:78-91, core/base_unary_edge.hpp:43-72
  LM         core/optimization_algorithm_levenberg.cpp:61-189, core/sparse_optimizer.cpp:354-419
  solver     solvers/linear_solver_dense.h:65-113 (LDL^T, isPositive)
  update     types_six_dof_expmap.h:81-85, sophus/se3.hpp:407-428, so3.hpp:426-456

Two things of the reference that a reader may not expect are kept:
  * an inlier edge's chi2 at the classification is the one of the last
    computeActiveErrors, i.e. at the last LM trial's pose even when that trial was
    rejected and the estimate restored; only outlier edges are recomputed (:1789-1791);
  * every round restarts from the input pose (:1779).
Where the restatement has to define what the sources leave open it says so: a failed
factorisation leaves x = 0 (Eigen would leave the previous x), and a round with no
level-0 edge runs no iteration (g2o's optimize returns -1 there) and reports iters 0.
With fewer than 3 correspondences nothing is written, flags included (the library's rule).

`mut` names a deliberate mistake, for the mutation tests of test_cpu_pose_opt.py.
"""
import numpy as np

DELTA_MONO = float(np.float32(np.sqrt(5.991)))      # const float deltaMono = sqrt(5.991)
DELTA_STEREO = float(np.float32(np.sqrt(7.815)))
TH_MONO = np.float32(5.991)
TH_STEREO = np.float32(7.815)
F64_MAX = np.finfo(np.float64).max
MUTATIONS = ("no_huber", "huber_round4", "right_update", "chain_rounds", "double_invz", "double_threshold",
             "no_rho_eps")


class Result:
    """The fields of ygzfe_pose_opt_result, the flags, and every edge's chi2 at each classification."""

    def __init__(self):
        self.q = np.zeros(4)
        self.t = np.zeros(3)
        self.T_q = np.zeros(4, np.float32)
        self.T_t = np.zeros(3, np.float32)
        self.n_corr = 0
        self.n_inliers = 0
        self.rounds = 0
        self.iters = [0, 0, 0, 0]
        self.rejected = [0, 0, 0, 0]
        self.chi2 = [0.0, 0.0, 0.0, 0.0]
        self.outlier = None          # uint8 [n], the caller's values where nothing is written
        self.edge_chi2 = []          # per round: float64 [n] (nan for absent rows)
        self.outlier_rounds = []     # per round: bool [n]
        self.stops = [None] * 4      # per round: 'trials', 'rho0', 'nbad', 'iters', 'none'
        self.min_margin = np.inf     # min over the LM trials of |currentChi - tempChi| / currentChi
        self.last_system = None      # (H 6x6, b 6) of the last buildSystem of the last round


def quat_normalize(q):
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def quat_rotate(q, X, Y, Z):
    """Eigen's Quaternion::_transformVector: v + w * uv + vec x uv with uv = 2 vec x v."""
    qx, qy, qz, qw = q
    ux, uy, uz = qy * Z - qz * Y, qz * X - qx * Z, qx * Y - qy * X
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return ((X + qw * ux) + (qy * uz - qz * uy), (Y + qw * uy) + (qz * ux - qx * uz),
            (Z + qw * uz) + (qx * uy - qy * ux))


def quat_matrix(q):
    a, b, c, w = q
    tx, ty, tz = 2 * a, 2 * b, 2 * c
    twx, twy, twz, txx, txy, txz = tx * w, ty * w, tz * w, tx * a, ty * a, tz * a
    tyy, tyz, tzz = ty * b, tz * b, tz * c
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def se3_exp(upsilon, omega):
    """SE3d::exp (se3.hpp:407-428) over SO3d::expAndTheta (so3.hpp:426-456), as written."""
    theta_sq = omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]
    theta = np.sqrt(theta_sq)
    half = 0.5 * theta
    small = theta < 1e-10
    if small:
        po4 = theta_sq * theta_sq
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * po4
        real = 1.0 - 0.5 * theta_sq + (1.0 / 384.0) * po4
    else:
        imag = np.sin(half) / theta
        real = np.cos(half)
    q = quat_normalize(np.array([imag * omega[0], imag * omega[1], imag * omega[2], real]))
    if small:
        V = quat_matrix(q)
    else:
        O = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
        V = (np.eye(3) + (1.0 - np.cos(theta)) / theta_sq * O) + (theta - np.sin(theta)) / (theta_sq * theta) * (O @ O)
    return q, V @ upsilon


def se3_mul(qa, ta, qb, tb):
    """SE3Group::operator* (se3.hpp:160-197, :239-271): t = ta + Ra tb, q = normalised qa qb."""
    r = quat_rotate(qa, tb[0], tb[1], tb[2])
    return quat_normalize(quat_mul(qa, qb)), np.array([r[0] + ta[0], r[1] + ta[1], r[2] + ta[2]])


def oplus(x, q, t, right=False):
    """VertexSE3Expmap::oplusImpl: update = (x[3:6], x[0:3]); estimate <- exp(update) * estimate."""
    qe, te = se3_exp(x[3:6], x[0:3])
    if right:
        return se3_mul(q, t, qe, te)
    return se3_mul(qe, te, q, t)


class _Edges:
    def __init__(self, cam, bf, kps_xy, octave, u_right, xw, inv_level_sigma2, mut):
        f64 = np.float64
        self.fx, self.fy, self.cx, self.cy = (f64(np.float32(v)) for v in cam)
        self.bf = f64(np.float32(bf))
        self.X = xw[:, 0].astype(np.float32).astype(f64)
        self.Y = xw[:, 1].astype(np.float32).astype(f64)
        self.Z = xw[:, 2].astype(np.float32).astype(f64)
        self.ox = kps_xy[:, 0].astype(np.float32).astype(f64)
        self.oy = kps_xy[:, 1].astype(np.float32).astype(f64)
        self.ur = u_right.astype(np.float32).astype(f64)
        self.stereo = ~(u_right.astype(np.float32) < 0)     # mvuRight[i] < 0 is mono (:1700)
        self.s = np.asarray(inv_level_sigma2, np.float32)[octave].astype(f64)
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.mut = mut

    def transform(self, q, t):
        x, y, z = quat_rotate(q, self.X, self.Y, self.Z)
        return x + t[0], y + t[1], z + t[2]

    def errors(self, q, t):
        """computeError of both edge types -> (e0, e1, e2, chi2); e2 = 0 for mono edges."""
        x, y, z = self.transform(q, t)
        with np.errstate(all="ignore"):
            m0 = self.ox - ((x / z) * self.fx + self.cx)
            m1 = self.oy - ((y / z) * self.fy + self.cy)
            invz = 1.0 / z
            if "double_invz" not in self.mut:
                invz = invz.astype(np.float32).astype(np.float64)   # const float invz = 1.0f / z (.cpp:309)
            px = x * invz * self.fx + self.cx
            py = y * invz * self.fy + self.cy
            pr = px - self.bf * invz
            e0 = np.where(self.stereo, self.ox - px, m0)
            e1 = np.where(self.stereo, self.oy - py, m1)
            e2 = np.where(self.stereo, self.ur - pr, 0.0)
            s = self.s
            chi2 = np.where(self.stereo, e0 * (s * e0) + e1 * (s * e1) + e2 * (s * e2), e0 * (s * e0) + e1 * (s * e1))
        return e0, e1, e2, chi2, (x, y, z)

    def robust(self, chi2, use):
        """RobustKernelHuber::robustify -> rho0, rho1 (or the plain chi2, 1)."""
        if not use:
            return chi2, np.ones_like(chi2)
        with np.errstate(all="ignore"):
            dsqr = self.delta * self.delta
            sq = np.sqrt(chi2)
            inl = chi2 <= dsqr
            rho0 = np.where(inl, chi2, 2 * sq * self.delta - dsqr)
            rho1 = np.where(inl, 1.0, self.delta / sq)
        return rho0, rho1

    def jacobians(self, xyz):
        x, y, z = xyz
        with np.errstate(all="ignore"):
            invz = 1.0 / z
            invz_2 = invz * invz
            J = np.zeros((3, 6) + x.shape)
            J[0, 0] = x * y * invz_2 * self.fx
            J[0, 1] = -(1 + (x * x * invz_2)) * self.fx
            J[0, 2] = y * invz * self.fx
            J[0, 3] = -invz * self.fx
            J[0, 5] = x * invz_2 * self.fx
            J[1, 0] = (1 + y * y * invz_2) * self.fy
            J[1, 1] = -x * y * invz_2 * self.fy
            J[1, 2] = -x * invz * self.fy
            J[1, 4] = -invz * self.fy
            J[1, 5] = y * invz_2 * self.fy
            J[2, 0] = J[0, 0] - self.bf * y * invz_2
            J[2, 1] = J[0, 1] + self.bf * x * invz_2
            J[2, 2] = J[0, 2]
            J[2, 3] = J[0, 3]
            J[2, 5] = J[0, 5] - self.bf * invz_2
            J[2][:, ~self.stereo] = 0.0
        return J


def ldlt_solve(A, b):
    """Unpivoted LDL^T of the 6x6 system; False (and x = 0) on a non-positive pivot."""
    n = 6
    L = np.eye(n)
    d = np.zeros(n)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = A[j, j]
            for m in range(j):
                dj -= L[j, m] * L[j, m] * d[m]
            d[j] = dj
            if dj <= 0.0:
                ok = False
            for i in range(j + 1, n):
                v = A[i, j]
                for m in range(j):
                    v -= L[i, m] * L[j, m] * d[m]
                L[i, j] = v / dj
        if not ok:
            return False, np.zeros(n)
        y = np.zeros(n)
        for i in range(n):
            v = b[i]
            for m in range(i):
                v -= L[i, m] * y[m]
            y[i] = v
        y = y / d
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            v = y[i]
            for m in range(i + 1, n):
                v -= L[m, i] * x[m]
            x[i] = v
    return True, x


def tree_sum(v, rows, n, lanes=256, wave=64):
    """Sum of v (last axis: one value per edge, edge k being row rows[k] of n) in another fixed order: lane
    l adds rows l, l + lanes, ... in turn, the lanes of a wave are combined by an xor butterfly, the waves
    in turn -- the order of a strided loop over a workgroup followed by a wave and an LDS reduction."""
    v = np.asarray(v, np.float64)
    k = -(-max(n, 1) // lanes)
    full = np.zeros(v.shape[:-1] + (k * lanes,))
    full[..., rows] = v
    full = full.reshape(v.shape[:-1] + (k, lanes))
    acc = np.zeros(v.shape[:-1] + (lanes,))
    for i in range(k):
        acc = acc + full[..., i, :]
    acc = acc.reshape(v.shape[:-1] + (lanes // wave, wave))
    lane = np.arange(wave)
    m = wave // 2
    while m >= 1:
        acc = acc + acc[..., lane ^ m]
        m //= 2
    out = acc[..., 0, 0]
    for w in range(1, lanes // wave):
        out = out + acc[..., w, 0]
    return out


def classify(chi, stereo, mut=()):
    """const float chi2 = e->chi2(); chi2 > chi2Mono[it] (Optimizer.cc:1793-1795, :1817-1819): a float compare."""
    if "double_threshold" in mut:
        return chi > np.where(stereo, 7.815, 5.991)
    return chi.astype(np.float32) > np.where(stereo, TH_STEREO, TH_MONO).astype(np.float32)


def pose_optimization(cam, bf, T_init, kps_xy, octave, u_right, xw, present, inv_level_sigma2, outlier_in=None,
                      mut=(), order="numpy"):
    """cam = (fx, fy, cx, cy); T_init = (q xyzw [4], t [3]) float32; kps_xy [n,2]; octave [n]; u_right [n] or
    None; xw [n,3]; present [n].  Returns a Result.
    order: how the sums over the edges are formed, 'numpy' (np.sum / einsum), 'reverse' (np.sum over the
    reversed edges) or 'tree' (tree_sum); the result must not depend on it beyond rounding."""
    mut = set(mut)
    assert mut <= set(MUTATIONS)
    n = len(present)
    present = np.asarray(present).astype(bool)
    kps_xy = np.asarray(kps_xy, np.float32).reshape(n, 2)
    xw = np.asarray(xw, np.float32).reshape(n, 3)
    octave = np.asarray(octave, np.int64)
    u_right = np.full(n, -1.0, np.float32) if u_right is None else np.asarray(u_right, np.float32)
    R = Result()
    R.outlier = np.zeros(n, np.uint8) if outlier_in is None else np.array(outlier_in, np.uint8)
    q_in = np.asarray(T_init[0], np.float32)
    t_in = np.asarray(T_init[1], np.float32)
    R.T_q, R.T_t = q_in.copy(), t_in.copy()
    R.q, R.t = q_in.astype(np.float64), t_in.astype(np.float64)
    R.n_corr = int(present.sum())
    if R.n_corr < 3:
        return R
    idx = np.nonzero(present)[0]
    if np.any(octave[idx] < 0) or np.any(octave[idx] >= len(inv_level_sigma2)):
        raise ValueError("octave out of range")
    E = _Edges(cam, bf, kps_xy[idx], octave[idx], u_right[idx], xw[idx], inv_level_sigma2, mut)
    m = len(idx)
    q0 = quat_normalize(q_in.astype(np.float64))   # mTcw.cast<double>() through the SO3d constructor
    t0 = t_in.astype(np.float64)
    outl = np.zeros(m, bool)
    q, t = q0, t0

    def esum(v, act):
        if order == "tree":
            return tree_sum(v, idx[act], n)
        if order == "reverse":
            return np.sum(v[..., ::-1], axis=-1)
        return np.sum(v, axis=-1)
    n_bad = 0
    for rnd in range(4):
        use_huber = (rnd < 3 or "huber_round4" in mut) and "no_huber" not in mut
        if not ("chain_rounds" in mut and rnd > 0):
            q, t = q0, t0                                             # :1779
        act = ~outl
        ql, tl = q, t               # the pose of the last computeActiveErrors
        iters = rejected = 0
        last_chi = 0.0
        stop = "none"
        if act.any():
            lam = ni = 0.0
            lm_bad = 0
            stop = "iters"
            for it in range(10):
                with np.errstate(all="ignore"):
                    e0, e1, e2, chi2, xyz = E.errors(q, t)
                    ql, tl = q, t
                    rho0, rho1 = E.robust(chi2, use_huber)
                    cur = ini = last_chi = float(esum(rho0[act], act))
                    J = E.jacobians(xyz)[:, :, act]
                    s, w = E.s[act], rho1[act]
                    err = np.stack([e0, e1, e2])[:, act]
                    if order == "numpy":
                        H = np.einsum("rik,k,rjk->ij", J, w * s, J)
                        b = -np.einsum("rik,k,rk->i", J, w * s, err)
                    else:
                        ws = w * s
                        Ht = (J[0][:, None] * ws * J[0][None] + J[1][:, None] * ws * J[1][None]
                              + J[2][:, None] * ws * J[2][None])
                        bt = w * (J[0] * (s * err[0]) + J[1] * (s * err[1]) + J[2] * (s * err[2]))
                        H, b = esum(Ht, act), -esum(bt, act)
                R.last_system = (H, b)
                if it == 0:                                           # computeLambdaInit, std::max as written
                    mx = 0.0
                    for j in range(6):
                        h = abs(H[j, j])
                        mx = mx if h < mx else h
                    lam, ni, lm_bad = 1e-5 * mx, 2.0, 0
                qmax = 0
                rho = 0.0
                while True:
                    ok, x = ldlt_solve(H + lam * np.eye(6), b)
                    with np.errstate(all="ignore"):
                        qt, tt = oplus(x, q, t, right="right_update" in mut)
                        _, _, _, chi2t, _ = E.errors(qt, tt)
                        ql, tl = qt, tt
                        temp = last_chi = float(esum(E.robust(chi2t, use_huber)[0][act], act))
                        if not ok:
                            temp = F64_MAX
                        if np.isfinite(temp) and cur > 0:
                            R.min_margin = min(R.min_margin, abs(cur - temp) / cur)
                        scale = 0.0
                        for j in range(6):
                            scale += x[j] * (lam * x[j] + b[j])
                        if "no_rho_eps" not in mut:
                            scale += 1e-3
                        rho = float(np.float64(cur - temp) / np.float64(scale))
                    if rho > 0 and np.isfinite(temp):
                        alpha = 1. - (2 * rho - 1) ** 3
                        alpha = min(alpha, 2. / 3.)
                        lam *= max(1. / 3., alpha)
                        ni = 2.0
                        cur = temp
                        q, t = qt, tt
                    else:
                        lam *= ni
                        ni *= 2
                        rejected += 1
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                iters += 1
                if qmax == 10:
                    stop = "trials"
                    break
                if rho == 0:
                    stop = "rho0"
                    break
                if (ini - cur) * 1e3 < ini:
                    lm_bad += 1
                else:
                    lm_bad = 0
                if lm_bad >= 3:
                    stop = "nbad"
                    break
        # classification (:1783-1830)
        with np.errstate(all="ignore"):
            chi_in = E.errors(ql, tl)[3]
            chi_out = E.errors(q, t)[3]
            chi = np.where(outl, chi_out, chi_in)
            outl = classify(chi, E.stereo, mut)
        n_bad = int(outl.sum())
        full = np.full(n, np.nan)
        full[idx] = chi
        R.edge_chi2.append(full)
        fo = np.zeros(n, bool)
        fo[idx] = outl
        R.outlier_rounds.append(fo)
        R.iters[rnd], R.rejected[rnd], R.chi2[rnd], R.stops[rnd] = iters, rejected, last_chi, stop
        R.rounds = rnd + 1
        if m < 10:                                                    # optimizer.edges().size() < 10
            break
    R.outlier[idx] = outl
    R.q, R.t = np.array(q, np.float64), np.array(t, np.float64)
    R.T_q, R.T_t = R.q.astype(np.float32), R.t.astype(np.float32)
    R.n_inliers = R.n_corr - n_bad
    return R


# ------------------------------------------------------------------ SE3 helpers for the tests
def quat_from_rotvec(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.array([0.5 * w[0], 0.5 * w[1], 0.5 * w[2], 1.0])
    return np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]])


def se3_log_inf(qa, ta, qb, tb):
    """inf-norm of log(A * B^-1) as (rotation vector, translation difference in A's frame)."""
    qa = quat_normalize(np.asarray(qa, np.float64))
    qb = quat_normalize(np.asarray(qb, np.float64))
    qbi = np.array([-qb[0], -qb[1], -qb[2], qb[3]])
    qd = quat_mul(qa, qbi)
    if qd[3] < 0:
        qd = -qd
    nv = np.linalg.norm(qd[:3])
    rot = 2.0 * qd[:3] if nv < 1e-12 else 2.0 * np.arctan2(nv, qd[3]) * qd[:3] / nv
    r = quat_rotate(qd, *np.asarray(tb, np.float64))
    dt = np.asarray(ta, np.float64) - np.array(r)
    with np.errstate(all="ignore"):
        return float(max(np.max(np.abs(rot)), np.max(np.abs(dt))))


# ------------------------------------------------------------------ scenes
INV_LEVEL_SIGMA2 = np.array([1.0 / (1.2 ** (2 * l)) for l in range(4)], np.float32)
CAM = (458.654, 457.296, 367.215, 248.375)
BF = 47.9


def make_scene(seed, n, stereo_share=0.0, outlier_share=0.15, noise=0.5, present_share=0.9, init_rot=0.02,
               init_trans=0.05, outlier_px=30.0):
    """A pinhole camera, points in front of it, pixel noise (uniform within +-noise), a planted share of
    gross outliers (>= outlier_px away), an optional stereo share, octaves 0..3, a ground-truth pose and
    a perturbed initial pose.  Returns a dict of call arguments and the planted truth."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CAM
    q_gt = quat_normalize(quat_from_rotvec(rng.uniform(-0.3, 0.3, 3)))
    t_gt = rng.uniform(-1.0, 1.0, 3)
    # points in the camera frame, then to the world: Xw = R^T (Xc - t)
    u = rng.uniform(20, 2 * cx - 20, n)
    v = rng.uniform(20, 2 * cy - 20, n)
    z = rng.uniform(2.0, 12.0, n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    qi = np.array([-q_gt[0], -q_gt[1], -q_gt[2], q_gt[3]])
    d = Xc - t_gt
    xw = np.stack(quat_rotate(qi, d[:, 0], d[:, 1], d[:, 2]), 1).astype(np.float32)
    # observations of the float32 points under the truth
    xc = np.stack(quat_rotate(q_gt, *xw.astype(np.float64).T), 1) + t_gt
    pu = xc[:, 0] / xc[:, 2] * fx + cx
    pv = xc[:, 1] / xc[:, 2] * fy + cy
    pr = pu - BF / xc[:, 2]
    planted = rng.random(n) < outlier_share
    if n >= 3:
        planted[:3] = False
    ang = rng.uniform(0, 2 * np.pi, n)
    mag = rng.uniform(outlier_px, 3 * outlier_px, n)
    du = rng.uniform(-noise, noise, n) + np.where(planted, mag * np.cos(ang), 0.0)
    dv = rng.uniform(-noise, noise, n) + np.where(planted, mag * np.sin(ang), 0.0)
    dr = rng.uniform(-noise, noise, n) + np.where(planted, mag * np.cos(ang), 0.0)
    kps_xy = np.stack([pu + du, pv + dv], 1).astype(np.float32)
    stereo = rng.random(n) < stereo_share
    u_right = np.where(stereo, np.maximum(pr + dr, 0.0), -1.0).astype(np.float32)
    octave = rng.integers(0, 4, n).astype(np.int32)
    present = rng.random(n) < present_share
    if n >= 3:
        present[:3] = True
    if present_share >= 1.0:
        present[:] = True
    q_init, t_init = se3_mul(quat_from_rotvec(rng.uniform(-1, 1, 3) * init_rot), rng.uniform(-1, 1, 3) * init_trans,
                             q_gt, t_gt)
    return dict(cam=CAM, bf=BF, T_init=(q_init.astype(np.float32), t_init.astype(np.float32)), kps_xy=kps_xy,
                octave=octave, u_right=u_right, xw=xw, present=present.astype(np.uint8),
                inv_level_sigma2=INV_LEVEL_SIGMA2, planted=planted, q_gt=q_gt, t_gt=t_gt, noise=noise)


def call_args(sc):
    return (sc["cam"], sc["bf"], sc["T_init"], sc["kps_xy"], sc["octave"], sc["u_right"], sc["xw"], sc["present"],
            sc["inv_level_sigma2"])


def permuted(sc, seed):
    p = np.random.default_rng(seed).permutation(len(sc["present"]))
    out = dict(sc)
    for k in ("kps_xy", "octave", "u_right", "xw", "present", "planted"):
        out[k] = sc[k][p]
    out["perm"] = p
    return out


# ------------------------------------------------------------------ the fixed cases of the CPU and GPU tests
SIZES = (3, 9, 10, 63, 64, 65, 255, 256, 257, 1000, 2500)
KINDS = (("mono", 0.0), ("stereo", 1.0), ("mixed", 0.4))
# seeds chosen in test_cpu_pose_opt.py's preconditions: 'far' starts 0.8 rad / 2 m off, runs all 10
# iterations of a round, rejects LM trials and re-admits edges that round 1 called outliers;
# 'empty_round' starts so far off that round 1 leaves no inlier and rounds 2-4 have nothing to optimise
SPECIAL = {"far": dict(seed=10, n=120, stereo_share=0.3, init_rot=0.8, init_trans=2.0),
           "empty_round": dict(seed=8, n=120, stereo_share=0.3, init_rot=0.8, init_trans=2.0)}
CASE_IDS = [f"{k}-{n}" for n in SIZES for k, _ in KINDS] + list(SPECIAL)
_cache = {}


# per case: the first seed of a fixed sequence at which the restatement's flags are the planted ones and
# its iters[] / rejected[] are the same under edge permutations and under the other summation orders of
# pose_optimization(order=...) (most seeds of a mono case are not: once chi2 has converged to rounding,
# whether a further LM trial lowers it is decided by the summation order)
SEEDS = {'mono-3': 9003, 'stereo-3': 1013, 'mixed-3': 2007, 'mono-9': 2009, 'stereo-9': 3019, 'mixed-9': 1013,
         'mono-10': 2010, 'stereo-10': 2020, 'mixed-10': 2014, 'mono-63': 51063, 'stereo-63': 3073,
         'mixed-63': 2067, 'mono-64': 64064, 'stereo-64': 1074, 'mixed-64': 1068, 'mono-65': 101065,
         'stereo-65': 1075, 'mixed-65': 2069, 'mono-255': 519255, 'stereo-255': 2265, 'mixed-255': 2259,
         'mono-256': 194256, 'stereo-256': 1266, 'mixed-256': 7260, 'mono-257': 102257, 'stereo-257': 1267,
         'mixed-257': 9261, 'mono-1000': 54000, 'stereo-1000': 2010, 'mixed-1000': 2004, 'mono-2500': 84500,
         'stereo-2500': 3510, 'mixed-2500': 3504}
# the mono cases of these sizes start further off (no seed of the default start qualified in 600..800)
CASE_KW = {'mono-63': dict(init_rot=0.3, init_trans=0.8), 'mono-64': dict(init_rot=0.15, init_trans=0.4),
           'mono-65': dict(init_rot=0.15, init_trans=0.4), 'mono-257': dict(init_rot=0.15, init_trans=0.4)}


def case_scene(cid):
    if cid in SPECIAL:
        return make_scene(**SPECIAL[cid])
    kind, n = cid.split("-")
    return make_scene(SEEDS[cid], int(n), stereo_share=dict(KINDS)[kind], **CASE_KW.get(cid, {}))


def case(cid):
    """(scene, restatement result), computed once per process and shared; callers must not modify them."""
    if cid not in _cache:
        sc = case_scene(cid)
        _cache[cid] = (sc, pose_optimization(*call_args(sc)))
    return _cache[cid]


# Floors measured by test_cpu_pose_opt.py::test_floor (the restatement against itself under three edge
# permutations and two other summation orders, worst over CASE_IDS) and the tolerances derived from them (4 x floor, rounded up).
POSE_FLOOR, CHI2_FLOOR = 2.2e-14, 1.9e-11
POSE_TOL, CHI2_RTOL = 8.8e-14, 7.6e-11
CHI2_ATOL = 1e-10
