// poseopt.hip — Optimizer::PoseOptimization(Frame*) (Optimizer.cc:1656-1842) in one launch.
//
// One workgroup per problem: the 4 rounds, g2o's Levenberg-Marquardt
// (optimization_algorithm_levenberg.cpp:61-189) with its trial loop, the Huber kernel,
// Sophus's SE3 exponential applied on the left (types_six_dof_expmap.h:81-85) and the
// inlier / outlier classification after each round.  FP64 like g2o; the inputs are the
// reference's floats widened to double.
//
// Threads own edge rows in a strided loop; a row's float inputs are gathered once into
// LDS with their outlier flag (rows past kPoCache, 1792, are gathered again from global in every
// pass, up to ~440 passes, and keep their flag in the output array; the output array is otherwise
// only written).  The 21 + 6 + 1 sums go lane
// (row order) -> wave (xor butterfly) -> waves (LDS, wave order): no floating-point
// atomics, so a result does not depend on scheduling.  Thread 0 runs the 6x6 LDL^T, the
// trial logic and the exponential and publishes the poses and one control word through
// LDS; every loop exit is taken on that word (or on a reduced count) after a barrier, so
// all barriers are workgroup-uniform, and every loop has a fixed bound (4 x 10 x 10).
#include <float.h>

#include "kernels.hpp"

namespace ygzfe {
namespace {

constexpr int kPoThreads = 256;
constexpr int kPoWaves = kPoThreads / 64;
constexpr int kPoCache = 1792;  // edge rows kept in LDS (32 B each, 56 KB)
constexpr int kPoSums = 28;     // upper H (21), b (6), robust chi2 (1)

enum { kPoAbsent = 0, kPoMono = 1, kPoStereo = 2, kPoBadOctave = 3 };
enum { kCtlNextIter = 0, kCtlNextTrial = 1, kCtlStop = 2 };

struct PoEdge {
    float X, Y, Z, ox, oy, ur, s;
    int kind;
    bool out;  // mvbOutlier / level 1, kept beside the kind in LDS for cached rows
};

struct PoArgs {
    const int32_t *ptr;
    const ygzfe_camera *cam;
    const float *bf;
    const ygzfe_se3 *T_init;
    const ygzfe_kp *kps;
    const float *u_right;
    const float *xw;
    const uint8_t *present;
    const float *inv_sigma2;
    int n_levels;
    uint8_t *outlier;
    ygzfe_pose_opt_result *res;
};

struct PoCam {
    double fx, fy, cx, cy, bf;
};

__device__ inline PoEdge po_gather(const PoArgs &a, int row) {
    PoEdge e;
    e.X = e.Y = e.Z = e.ox = e.oy = e.ur = e.s = 0.f;
    e.kind = kPoAbsent;
    e.out = false;
    if (!a.present[row]) return e;
    const ygzfe_kp k = a.kps[row];
    if (k.octave < 0 || k.octave >= a.n_levels) {
        e.kind = kPoBadOctave;
        return e;
    }
    e.X = a.xw[3 * (size_t)row];
    e.Y = a.xw[3 * (size_t)row + 1];
    e.Z = a.xw[3 * (size_t)row + 2];
    e.ox = k.x;
    e.oy = k.y;
    e.s = a.inv_sigma2[k.octave];
    const float ur = a.u_right ? a.u_right[row] : -1.f;
    e.ur = ur;
    e.kind = (ur < 0) ? kPoMono : kPoStereo;  // Optimizer.cc:1700
    return e;
}

// SE3d * point: Eigen's Quaternion::_transformVector, then + translation (se3.hpp:257)
__device__ inline void po_transform(const double *T, double X, double Y, double Z, double &x, double &y, double &z) {
    const double qx = T[0], qy = T[1], qz = T[2], qw = T[3];
    double ux = qy * Z - qz * Y, uy = qz * X - qx * Z, uz = qx * Y - qy * X;
    ux += ux;
    uy += uy;
    uz += uz;
    x = (X + qw * ux) + (qy * uz - qz * uy) + T[4];
    y = (Y + qw * uy) + (qz * ux - qx * uz) + T[5];
    z = (Z + qw * uz) + (qx * uy - qy * ux) + T[6];
}

// computeError + chi2 (types_six_dof_expmap.h:165-201, .cpp:297-315); returns the edge's
// dimension, err[] = obs - cam_project(T * Xw)
__device__ inline double po_error(const PoEdge &e, const PoCam &c, double x, double y, double z, double err[3]) {
    const double s = (double)e.s;
    if (e.kind == kPoMono) {
        err[0] = (double)e.ox - ((x / z) * c.fx + c.cx);
        err[1] = (double)e.oy - ((y / z) * c.fy + c.cy);
        err[2] = 0.0;
        return err[0] * (s * err[0]) + err[1] * (s * err[1]);
    }
    const float invz_f = (float)(1.0 / z);  // .cpp:309: const float invz = 1.0f / trans_xyz[2]
    const double invz = (double)invz_f;
    const double px = x * invz * c.fx + c.cx;
    const double py = y * invz * c.fy + c.cy;
    const double pr = px - c.bf * invz;
    err[0] = (double)e.ox - px;
    err[1] = (double)e.oy - py;
    err[2] = (double)e.ur - pr;
    return err[0] * (s * err[0]) + err[1] * (s * err[1]) + err[2] * (s * err[2]);
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho0, rho1
__device__ inline void po_huber(double e2, double delta, double &rho0, double &rho1) {
    const double dsqr = delta * delta;
    if (e2 <= dsqr) {
        rho0 = e2;
        rho1 = 1.0;
    } else {
        const double sq = sqrt(e2);
        rho0 = 2 * sq * delta - dsqr;
        rho1 = delta / sq;
    }
}

__device__ inline double po_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// lane -> wave -> waves, in a fixed order; dst[0..K) is valid for every thread afterwards
template <int K>
__device__ inline void po_block_sum(double (&acc)[K], double *s_part, double *dst) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = po_wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_part[wave * kPoSums + k] = acc[k];
    }
    __syncthreads();
    if (tid < K) {
        double s = s_part[tid];
        for (int w = 1; w < kPoWaves; ++w) s += s_part[w * kPoSums + tid];
        dst[tid] = s;
    }
    __syncthreads();
}

// (H + lambda I) x = b by an unpivoted LDL^T; a non-positive pivot fails the trial
// (linear_solver_dense.h:107-112) and leaves x = 0.  A NaN pivot compares false and
// goes through, as Eigen's sign test does.
__device__ inline bool po_solve(const double *Hb, double lambda, double x[6]) {
    double A[6][6], d[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) A[i][j] = A[j][i] = Hb[k];
    for (int i = 0; i < 6; ++i) A[i][i] += lambda;
    bool ok = true;
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
        for (int m = 0; m < j; ++m) dj -= A[j][m] * A[j][m] * d[m];
        d[j] = dj;
        if (dj <= 0.0) ok = false;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int m = 0; m < j; ++m) v -= A[i][m] * A[j][m] * d[m];
            A[i][j] = v / dj;
        }
    }
    if (!ok) {
        for (int i = 0; i < 6; ++i) x[i] = 0.0;
        return false;
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = Hb[21 + i];
        for (int m = 0; m < i; ++m) v -= A[i][m] * y[m];
        y[i] = v;
    }
    for (int i = 0; i < 6; ++i) y[i] /= d[i];
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int m = i + 1; m < 6; ++m) v -= A[m][i] * x[m];
        x[i] = v;
    }
    return true;
}

__device__ inline void po_quat_normalize(double q[4]) {
    const double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= len;
}

// Tn = SE3d::exp((upsilon, omega)) * T with x = (omega, upsilon) (oplusImpl,
// types_six_dof_expmap.h:81-85; se3.hpp:407-428, so3.hpp:426-456 and the normalising
// product, se3.hpp:160-197)
__device__ inline void po_oplus(const double x[6], const double *T, double *Tn) {
    const double wx = x[0], wy = x[1], wz = x[2], ux = x[3], uy = x[4], uz = x[5];
    const double theta_sq = wx * wx + wy * wy + wz * wz;
    const double theta = sqrt(theta_sq);
    const double half = 0.5 * theta;
    const bool small = theta < 1e-10;
    double imag, real;
    if (small) {
        const double po4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * po4;
        real = 1.0 - 0.5 * theta_sq + (1.0 / 384.0) * po4;  // as written at so3.hpp:441-443
    } else {
        imag = sin(half) / theta;
        real = cos(half);
    }
    double qe[4] = {imag * wx, imag * wy, imag * wz, real};
    po_quat_normalize(qe);  // the SO3Group(Quaternion) constructor
    // V
    double V[3][3];
    if (small) {
        const double a = qe[0], b = qe[1], c = qe[2], w = qe[3];  // so3.matrix()
        const double tx = 2 * a, ty = 2 * b, tz = 2 * c;
        const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * a, txy = ty * a, txz = tz * a;
        const double tyy = ty * b, tyz = tz * b, tzz = tz * c;
        V[0][0] = 1 - (tyy + tzz); V[0][1] = txy - twz; V[0][2] = txz + twy;
        V[1][0] = txy + twz; V[1][1] = 1 - (txx + tzz); V[1][2] = tyz - twx;
        V[2][0] = txz - twy; V[2][1] = tyz + twx; V[2][2] = 1 - (txx + tyy);
    } else {
        const double O[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
        const double c1 = (1.0 - cos(theta)) / theta_sq, c2 = (theta - sin(theta)) / (theta_sq * theta);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double o2 = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
                V[i][j] = ((i == j ? 1.0 : 0.0) + c1 * O[i][j]) + c2 * o2;
            }
    }
    const double te[3] = {V[0][0] * ux + V[0][1] * uy + V[0][2] * uz, V[1][0] * ux + V[1][1] * uy + V[1][2] * uz,
                          V[2][0] * ux + V[2][1] * uy + V[2][2] * uz};
    // translation += so3_e * t, then the quaternion product and its normalisation
    const double Te[7] = {qe[0], qe[1], qe[2], qe[3], te[0], te[1], te[2]};
    po_transform(Te, T[4], T[5], T[6], Tn[4], Tn[5], Tn[6]);
    const double ax = qe[0], ay = qe[1], az = qe[2], aw = qe[3], bx = T[0], by = T[1], bz = T[2], bw = T[3];
    double q[4] = {aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                   aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz};
    po_quat_normalize(q);
    Tn[0] = q[0];
    Tn[1] = q[1];
    Tn[2] = q[2];
    Tn[3] = q[3];
}

__global__ __launch_bounds__(kPoThreads) void k_pose_opt(PoArgs a) {
    __shared__ float4 s_e0[kPoCache], s_e1[kPoCache];  // (X, Y, Z, ox), (oy, ur, s, kind)
    __shared__ double s_part[kPoWaves * kPoSums];
    __shared__ double s_H[kPoSums], s_chi[2];
    __shared__ double s_T[7], s_Tt[7], s_Tl[7];  // estimate, trial, pose of the last computeActiveErrors
    __shared__ int s_ctl;

    const int p = blockIdx.x, tid = threadIdx.x;
    const int base = a.ptr[p], n = a.ptr[p + 1] - base;
    ygzfe_pose_opt_result *res = a.res + p;
    const ygzfe_camera cf = a.cam[p];
    PoCam cam;
    cam.fx = cf.fx;
    cam.fy = cf.fy;
    cam.cx = cf.cx;
    cam.cy = cf.cy;
    cam.bf = a.bf[p];
    const double delta_mono = (double)(float)sqrt(5.991);
    const double delta_stereo = (double)(float)sqrt(7.815);  // Optimizer.cc:1689-1690

    auto edge_at = [&](int i) -> PoEdge {
        if (i < kPoCache) {
            const float4 u = s_e0[i], v = s_e1[i];
            PoEdge e;
            e.X = u.x; e.Y = u.y; e.Z = u.z; e.ox = u.w;
            e.oy = v.x; e.ur = v.y; e.s = v.z;
            const int k = __float_as_int(v.w);
            e.kind = k & 3;
            e.out = (k & 4) != 0;
            return e;
        }
        PoEdge e = po_gather(a, base + i);
        e.out = e.kind != kPoAbsent && a.outlier[base + i] != 0;
        return e;
    };

    // gather, nInitialCorrespondences, octave check
    {
        double acc[2] = {0.0, 0.0};
        for (int i = tid; i < n; i += kPoThreads) {
            const PoEdge e = po_gather(a, base + i);
            if (i < kPoCache) {
                s_e0[i] = make_float4(e.X, e.Y, e.Z, e.ox);
                s_e1[i] = make_float4(e.oy, e.ur, e.s, __int_as_float(e.kind));
            }
            if (e.kind == kPoBadOctave) acc[1] += 1.0;
            else if (e.kind != kPoAbsent) acc[0] += 1.0;
        }
        po_block_sum<2>(acc, s_part, s_chi);
    }
    const int n_bad_octave = (int)s_chi[1];
    const int n_corr = (int)s_chi[0];
    if (n_bad_octave > 0) {  // uniform
        if (tid == 0) {
            const ygzfe_se3 Tb = a.T_init[p];
            res->T_cw = Tb;
            for (int i = 0; i < 4; ++i) res->q[i] = (double)Tb.q[i];
            for (int i = 0; i < 3; ++i) res->t[i] = (double)Tb.t[i];
            res->n_corr = n_corr;
            res->n_inliers = 0;
            res->rounds = -1;
            for (int r = 0; r < 4; ++r) {
                res->iters[r] = 0;
                res->rejected[r] = 0;
                res->chi2[r] = 0.0;
            }
        }
        return;
    }
    const ygzfe_se3 Tf = a.T_init[p];
    if (n_corr < 3) {  // uniform; Optimizer.cc:1767
        if (tid == 0) {
            res->T_cw = Tf;
            for (int i = 0; i < 4; ++i) res->q[i] = (double)Tf.q[i];
            for (int i = 0; i < 3; ++i) res->t[i] = (double)Tf.t[i];
            res->n_corr = n_corr;
            res->n_inliers = 0;
            res->rounds = 0;
            for (int r = 0; r < 4; ++r) {
                res->iters[r] = 0;
                res->rejected[r] = 0;
                res->chi2[r] = 0.0;
            }
        }
        return;
    }
    // mTcw.cast<double>(): the SO3d constructor normalises
    double T0[7];
    {
        double q[4] = {(double)Tf.q[0], (double)Tf.q[1], (double)Tf.q[2], (double)Tf.q[3]};
        po_quat_normalize(q);
        T0[0] = q[0]; T0[1] = q[1]; T0[2] = q[2]; T0[3] = q[3];
        T0[4] = Tf.t[0]; T0[5] = Tf.t[1]; T0[6] = Tf.t[2];
    }
    for (int i = tid; i < n; i += kPoThreads)
        if (edge_at(i).kind != kPoAbsent) a.outlier[base + i] = 0;  // mvbOutlier[i] = false (:1702, :1730)

    int n_bad = 0, rounds = 0;
    // thread 0's LM state
    double lambda = 0.0, ni = 2.0, cur_chi = 0.0, last_chi = 0.0;
    int lm_bad = 0;
    for (int r = 0; r < 4; ++r) {
        const bool robust = r < 3;  // setRobustKernel(0) after it == 2 (:1804, :1828)
        const int n_active = n_corr - n_bad;
        int iters = 0, rejected = 0;
        if (tid == 0) {
            for (int i = 0; i < 7; ++i) s_T[i] = s_Tl[i] = T0[i];  // :1779
            last_chi = 0.0;
        }
        __syncthreads();
        // initializeOptimization(0) with no level-0 edge leaves nothing to optimise
        for (int it = 0; n_active > 0 && it < 10; ++it) {
            // computeActiveErrors + buildSystem at the estimate
            double T[7];
            for (int i = 0; i < 7; ++i) T[i] = s_T[i];
            double acc[kPoSums];
#pragma unroll
            for (int k = 0; k < kPoSums; ++k) acc[k] = 0.0;
            for (int i = tid; i < n; i += kPoThreads) {
                const PoEdge e = edge_at(i);
                if (e.kind == kPoAbsent || e.out) continue;
                double x, y, z, err[3];
                po_transform(T, e.X, e.Y, e.Z, x, y, z);
                const double e2 = po_error(e, cam, x, y, z, err);
                double rho0 = e2, rho1 = 1.0;
                if (robust) po_huber(e2, e.kind == kPoMono ? delta_mono : delta_stereo, rho0, rho1);
                // linearizeOplus (.cpp:272-295, :347-377), columns (omega, upsilon)
                const double invz = 1.0 / z, invz_2 = invz * invz;
                double J[3][6];
                J[0][0] = x * y * invz_2 * cam.fx;
                J[0][1] = -(1 + (x * x * invz_2)) * cam.fx;
                J[0][2] = y * invz * cam.fx;
                J[0][3] = -invz * cam.fx;
                J[0][4] = 0;
                J[0][5] = x * invz_2 * cam.fx;
                J[1][0] = (1 + y * y * invz_2) * cam.fy;
                J[1][1] = -x * y * invz_2 * cam.fy;
                J[1][2] = -x * invz * cam.fy;
                J[1][3] = 0;
                J[1][4] = -invz * cam.fy;
                J[1][5] = y * invz_2 * cam.fy;
                const int dim = e.kind == kPoMono ? 2 : 3;
                if (dim == 3) {
                    J[2][0] = J[0][0] - cam.bf * y * invz_2;
                    J[2][1] = J[0][1] + cam.bf * x * invz_2;
                    J[2][2] = J[0][2];
                    J[2][3] = J[0][3];
                    J[2][4] = 0;
                    J[2][5] = J[0][5] - cam.bf * invz_2;
                } else {
                    for (int c = 0; c < 6; ++c) J[2][c] = 0;
                }
                // constructQuadraticForm (base_unary_edge.hpp:56-66): rho' Omega, no second-order term
                const double s = (double)e.s, ws = rho1 * s;
                int k = 0;
#pragma unroll
                for (int c = 0; c < 6; ++c) {
#pragma unroll
                    for (int d = c; d < 6; ++d, ++k)
                        acc[k] += J[0][c] * ws * J[0][d] + J[1][c] * ws * J[1][d] + J[2][c] * ws * J[2][d];
                    acc[21 + c] -= rho1 * (J[0][c] * (s * err[0]) + J[1][c] * (s * err[1]) + J[2][c] * (s * err[2]));
                }
                acc[27] += rho0;
            }
            po_block_sum<kPoSums>(acc, s_part, s_H);
            int q_trials = 0;
            double ini_chi = 0.0, rho = 0.0;
            if (tid == 0) {
                cur_chi = ini_chi = last_chi = s_H[27];
                for (int i = 0; i < 7; ++i) s_Tl[i] = s_T[i];
                if (it == 0) {  // computeLambdaInit, std::max's NaN behaviour kept
                    const int diag[6] = {0, 6, 11, 15, 18, 20};
                    double mx = 0.0;
                    for (int j = 0; j < 6; ++j) {
                        const double h = fabs(s_H[diag[j]]);
                        mx = (h < mx) ? mx : h;
                    }
                    lambda = 1e-5 * mx;
                    ni = 2.0;
                    lm_bad = 0;
                }
            }
            for (int trial = 0; trial < 10; ++trial) {  // maxTrialsAfterFailure
                bool ok = true;
                double xs[6];
                if (tid == 0) {
                    ok = po_solve(s_H, lambda, xs);
                    double Tn[7];
                    po_oplus(xs, s_T, Tn);
                    for (int i = 0; i < 7; ++i) s_Tt[i] = s_Tl[i] = Tn[i];
                }
                __syncthreads();
                double Tt[7];
                for (int i = 0; i < 7; ++i) Tt[i] = s_Tt[i];
                double chi[1] = {0.0};
                for (int i = tid; i < n; i += kPoThreads) {
                    const PoEdge e = edge_at(i);
                    if (e.kind == kPoAbsent || e.out) continue;
                    double x, y, z, err[3];
                    po_transform(Tt, e.X, e.Y, e.Z, x, y, z);
                    const double e2 = po_error(e, cam, x, y, z, err);
                    double rho0 = e2, rho1 = 1.0;
                    if (robust) po_huber(e2, e.kind == kPoMono ? delta_mono : delta_stereo, rho0, rho1);
                    chi[0] += rho0;
                }
                po_block_sum<1>(chi, s_part, s_chi);
                if (tid == 0) {
                    double temp = s_chi[0];
                    last_chi = temp;
                    if (!ok) temp = DBL_MAX;
                    double scale = 0.0;
                    for (int j = 0; j < 6; ++j) scale += xs[j] * (lambda * xs[j] + s_H[21 + j]);
                    scale += 1e-3;
                    rho = (cur_chi - temp) / scale;
                    if (rho > 0 && isfinite(temp)) {
                        double alpha = 2 * rho - 1;
                        alpha = 1. - alpha * alpha * alpha;
                        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
                        const double sf = 1. / 3. < alpha ? alpha : 1. / 3.;
                        lambda *= sf;
                        ni = 2;
                        cur_chi = temp;
                        for (int i = 0; i < 7; ++i) s_T[i] = s_Tt[i];
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        ++rejected;
                    }
                    ++q_trials;
                    int ctl = kCtlNextIter;
                    if (rho < 0 && q_trials < 10) {
                        ctl = kCtlNextTrial;
                    } else {
                        ++iters;
                        if (q_trials == 10 || rho == 0) {
                            ctl = kCtlStop;
                        } else {
                            if ((ini_chi - cur_chi) * 1e3 < ini_chi) ++lm_bad;  // "Stop criterium (Raul)"
                            else lm_bad = 0;
                            if (lm_bad >= 3) ctl = kCtlStop;
                        }
                    }
                    s_ctl = ctl;
                }
                __syncthreads();
                if (s_ctl != kCtlNextTrial) break;  // uniform: read from LDS after the barrier
            }
            if (s_ctl == kCtlStop) break;  // uniform
            __syncthreads();               // s_ctl is rewritten only after every thread has read it
        }
        __syncthreads();

        // classification (:1783-1830): an outlier edge's error is recomputed at the estimate,
        // an inlier edge keeps the error of the last computeActiveErrors (the last trial's pose)
        double Tc[7], Tl[7];
        for (int i = 0; i < 7; ++i) {
            Tc[i] = s_T[i];
            Tl[i] = s_Tl[i];
        }
        double bad[1] = {0.0};
        for (int i = tid; i < n; i += kPoThreads) {
            const PoEdge e = edge_at(i);
            if (e.kind == kPoAbsent) continue;
            const bool out = e.out;
            double x, y, z, err[3];
            po_transform(out ? Tc : Tl, e.X, e.Y, e.Z, x, y, z);
            const float chi2 = (float)po_error(e, cam, x, y, z, err);
            const bool now_out = chi2 > (e.kind == kPoMono ? 5.991f : 7.815f);
            a.outlier[base + i] = now_out ? 1 : 0;
            if (i < kPoCache) s_e1[i].w = __int_as_float(e.kind | (now_out ? 4 : 0));
            if (now_out) bad[0] += 1.0;
        }
        po_block_sum<1>(bad, s_part, s_chi);
        n_bad = (int)s_chi[0];
        rounds = r + 1;
        if (tid == 0) {
            res->iters[r] = iters;
            res->rejected[r] = rejected;
            res->chi2[r] = last_chi;
        }
        if (n_corr < 10) break;  // optimizer.edges().size() < 10 (:1832), uniform
        __syncthreads();
    }
    if (tid == 0) {
        for (int r = rounds; r < 4; ++r) {
            res->iters[r] = 0;
            res->rejected[r] = 0;
            res->chi2[r] = 0.0;
        }
        for (int i = 0; i < 4; ++i) {
            res->q[i] = s_T[i];
            res->T_cw.q[i] = (float)s_T[i];
        }
        for (int i = 0; i < 3; ++i) {
            res->t[i] = s_T[4 + i];
            res->T_cw.t[i] = (float)s_T[4 + i];
        }
        res->n_corr = n_corr;
        res->n_inliers = n_corr - n_bad;
        res->rounds = rounds;
    }
}

}  // namespace

hipError_t launch_pose_opt(int n_problems, const int32_t *ptr, const ygzfe_camera *cam, const float *bf,
                           const ygzfe_se3 *T_init, const ygzfe_kp *kps, const float *u_right, const float *xw,
                           const uint8_t *present, const float *inv_sigma2, int n_levels, uint8_t *outlier,
                           ygzfe_pose_opt_result *res, hipStream_t st) {
    if (n_problems <= 0) return hipSuccess;
    PoArgs a{ptr, cam, bf, T_init, kps, u_right, xw, present, inv_sigma2, n_levels, outlier, res};
    hipLaunchKernelGGL(k_pose_opt, dim3(n_problems), dim3(kPoThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace ygzfe
