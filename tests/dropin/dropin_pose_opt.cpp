// The reference's call site of Optimizer::PoseOptimization (Tracking.cc:2212-2239) over the test
// stubs of Frame / MapPoint, with the drop-in body (compat/dropin/Optimizer_pose_gpu.inc), against a
// plain C++ double restatement of Optimizer.cc:1656-1842 with the g2o / Sophus pieces it runs
// (test only; sums in row order).  --time: median ms of the drop-in call and of the restatement on
// one core, for a 1,000-edge frame and for 32 candidates (one batch launch against 32 CPU runs).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <random>
#include <set>
#include <vector>

#include "Frame.h"
#include "MapPoint.h"
#include "OptimizerGPU.h"

namespace ygz {
static std::mutex g_map_mutex;  // the stub MapPoint has no mGlobalMutex
#define YGZFE_POSE_GATHER_MUTEX g_map_mutex
class Optimizer {
public:
    int static PoseOptimization(Frame *pFrame);  // Optimizer.h:37
};
#include "Optimizer_pose_gpu.inc"
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
bool Frame::mbNeedUndistort = false;
long unsigned int Frame::nNextId = 0;
}  // namespace ygz
using namespace ygz;

// ------------------------------------------------------------------ restatement (double)
struct Pose { double q[4], t[3]; };
static void qnorm(double *q) {
    const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q[i] /= l;
}
static void rot(const double *q, const double *v, double *o) {
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux += ux; uy += uy; uz += uz;
    o[0] = (v[0] + q[3] * ux) + (q[1] * uz - q[2] * uy);
    o[1] = (v[1] + q[3] * uy) + (q[2] * ux - q[0] * uz);
    o[2] = (v[2] + q[3] * uz) + (q[0] * uy - q[1] * ux);
}
static Pose oplus(const double *x, const Pose &T) {  // exp((x[3:6], x[0:3])) * T
    const double w[3] = {x[0], x[1], x[2]}, u[3] = {x[3], x[4], x[5]};
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2), half = 0.5 * th;
    double imag, real;
    const bool small = th < 1e-10;
    if (small) {
        const double p4 = th2 * th2;
        imag = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * p4;
        real = 1.0 - 0.5 * th2 + (1.0 / 384.0) * p4;
    } else {
        imag = std::sin(half) / th;
        real = std::cos(half);
    }
    Pose E;
    E.q[0] = imag * w[0]; E.q[1] = imag * w[1]; E.q[2] = imag * w[2]; E.q[3] = real;
    qnorm(E.q);
    double V[3][3];
    if (small) {
        for (int c = 0; c < 3; c++) {
            double e[3] = {0, 0, 0}, o[3];
            e[c] = 1;
            rot(E.q, e, o);
            for (int r = 0; r < 3; r++) V[r][c] = o[r];
        }
    } else {
        const double O[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
        const double c1 = (1.0 - std::cos(th)) / th2, c2 = (th - std::sin(th)) / (th2 * th);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double o2 = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
                V[i][j] = ((i == j ? 1.0 : 0.0) + c1 * O[i][j]) + c2 * o2;
            }
    }
    for (int i = 0; i < 3; i++) E.t[i] = V[i][0] * u[0] + V[i][1] * u[1] + V[i][2] * u[2];
    Pose R;
    double r[3];
    rot(E.q, T.t, r);
    for (int i = 0; i < 3; i++) R.t[i] = r[i] + E.t[i];
    const double *a = E.q, *b = T.q;
    R.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    R.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    R.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    R.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    qnorm(R.q);
    return R;
}
struct Edge { double X[3], ox, oy, ur, s; bool stereo; int row; };
struct Cam { double fx, fy, cx, cy, bf; };
static double edge_err(const Edge &e, const Cam &c, const Pose &T, double *err, double *xyz) {
    double p[3];
    rot(T.q, e.X, p);
    for (int i = 0; i < 3; i++) p[i] += T.t[i];
    if (xyz) memcpy(xyz, p, sizeof(p));
    if (!e.stereo) {
        err[0] = e.ox - ((p[0] / p[2]) * c.fx + c.cx);
        err[1] = e.oy - ((p[1] / p[2]) * c.fy + c.cy);
        err[2] = 0;
        return err[0] * (e.s * err[0]) + err[1] * (e.s * err[1]);
    }
    const float invz_f = 1.0f / p[2];
    const double invz = invz_f, px = p[0] * invz * c.fx + c.cx, py = p[1] * invz * c.fy + c.cy;
    err[0] = e.ox - px;
    err[1] = e.oy - py;
    err[2] = e.ur - (px - c.bf * invz);
    return err[0] * (e.s * err[0]) + err[1] * (e.s * err[1]) + err[2] * (e.s * err[2]);
}
static void huber(double e2, double delta, double &r0, double &r1) {
    const double d2 = delta * delta;
    if (e2 <= d2) { r0 = e2; r1 = 1; } else { const double sq = std::sqrt(e2); r0 = 2 * sq * delta - d2; r1 = delta / sq; }
}
static bool solve6(const double H[6][6], const double *b, double lambda, double *x) {
    double L[6][6] = {{0}}, d[6];
    bool ok = true;
    for (int j = 0; j < 6; j++) {
        double dj = H[j][j] + lambda;
        for (int m = 0; m < j; m++) dj -= L[j][m] * L[j][m] * d[m];
        d[j] = dj;
        if (dj <= 0.0) ok = false;
        for (int i = j + 1; i < 6; i++) {
            double v = H[i][j];
            for (int m = 0; m < j; m++) v -= L[i][m] * L[j][m] * d[m];
            L[i][j] = v / dj;
        }
    }
    if (!ok) { for (int i = 0; i < 6; i++) x[i] = 0; return false; }
    double y[6];
    for (int i = 0; i < 6; i++) { double v = b[i]; for (int m = 0; m < i; m++) v -= L[i][m] * y[m]; y[i] = v; }
    for (int i = 0; i < 6; i++) y[i] /= d[i];
    for (int i = 5; i >= 0; i--) { double v = y[i]; for (int m = i + 1; m < 6; m++) v -= L[m][i] * x[m]; x[i] = v; }
    return true;
}
struct RefResult { Pose T; int n_corr, n_inliers; std::vector<uint8_t> outlier; double min_gap; };
static double robust_chi(const std::vector<Edge> &E, const std::vector<uint8_t> &outl, const Cam &c, const Pose &T,
                         bool use_huber, double dm, double ds) {
    double sum = 0, err[3];
    for (size_t k = 0; k < E.size(); k++) {
        if (outl[k]) continue;
        double e2 = edge_err(E[k], c, T, err, nullptr), r0 = e2, r1 = 1;
        if (use_huber) huber(e2, E[k].stereo ? ds : dm, r0, r1);
        sum += r0;
    }
    return sum;
}
static RefResult ref_pose_opt(Frame *F) {
    RefResult R;
    const Cam c = {Frame::fx, Frame::fy, Frame::cx, Frame::cy, F->mbf};
    std::vector<Edge> E;
    for (int i = 0; i < F->N; i++) {
        MapPoint *mp = F->mvpMapPoints[i];
        if (!mp) continue;
        Edge e;
        const Vector3f X = mp->GetWorldPos();
        for (int k = 0; k < 3; k++) e.X[k] = X[k];
        e.ox = F->mvKeys[i].pt.x; e.oy = F->mvKeys[i].pt.y; e.ur = F->mvuRight[i];
        e.stereo = !(F->mvuRight[i] < 0);
        e.s = F->mvInvLevelSigma2[F->mvKeys[i].octave];
        e.row = i;
        E.push_back(e);
    }
    R.n_corr = (int)E.size();
    R.n_inliers = 0;
    R.min_gap = 1e300;
    R.outlier.assign(F->N, 2);
    Pose T0;
    T0.q[0] = F->mTcw.unit_quaternion().x(); T0.q[1] = F->mTcw.unit_quaternion().y();
    T0.q[2] = F->mTcw.unit_quaternion().z(); T0.q[3] = F->mTcw.unit_quaternion().w();
    for (int k = 0; k < 3; k++) T0.t[k] = F->mTcw.translation()[k];
    R.T = T0;
    if (R.n_corr < 3) return R;
    qnorm(T0.q);
    const double dm = (double)(float)std::sqrt(5.991), ds = (double)(float)std::sqrt(7.815);
    std::vector<uint8_t> outl(E.size(), 0);
    Pose T = T0;
    int nbad = 0;
    for (int rnd = 0; rnd < 4; rnd++) {
        const bool hub = rnd < 3;
        T = T0;
        Pose Tl = T;
        size_t nact = 0;
        for (size_t k = 0; k < E.size(); k++) nact += !outl[k];
        double lambda = 0, ni = 2;
        int lm_bad = 0;
        for (int it = 0; nact > 0 && it < 10; it++) {
            double H[6][6] = {{0}}, b[6] = {0}, cur = 0;
            for (size_t k = 0; k < E.size(); k++) {
                if (outl[k]) continue;
                double err[3], p[3];
                const double e2 = edge_err(E[k], c, T, err, p);
                double r0 = e2, r1 = 1;
                if (hub) huber(e2, E[k].stereo ? ds : dm, r0, r1);
                cur += r0;
                const double x = p[0], y = p[1], invz = 1.0 / p[2], iz2 = invz * invz;
                double J[3][6] = {{0}};
                J[0][0] = x * y * iz2 * c.fx; J[0][1] = -(1 + (x * x * iz2)) * c.fx; J[0][2] = y * invz * c.fx;
                J[0][3] = -invz * c.fx; J[0][5] = x * iz2 * c.fx;
                J[1][0] = (1 + y * y * iz2) * c.fy; J[1][1] = -x * y * iz2 * c.fy; J[1][2] = -x * invz * c.fy;
                J[1][4] = -invz * c.fy; J[1][5] = y * iz2 * c.fy;
                if (E[k].stereo) {
                    J[2][0] = J[0][0] - c.bf * y * iz2; J[2][1] = J[0][1] + c.bf * x * iz2; J[2][2] = J[0][2];
                    J[2][3] = J[0][3]; J[2][5] = J[0][5] - c.bf * iz2;
                }
                const double ws = r1 * E[k].s;
                for (int a = 0; a < 6; a++) {
                    for (int d = 0; d < 6; d++)
                        H[a][d] += J[0][a] * ws * J[0][d] + J[1][a] * ws * J[1][d] + J[2][a] * ws * J[2][d];
                    b[a] -= r1 * (J[0][a] * (E[k].s * err[0]) + J[1][a] * (E[k].s * err[1]) + J[2][a] * (E[k].s * err[2]));
                }
            }
            Tl = T;
            const double ini = cur;
            if (it == 0) {
                double mx = 0;
                for (int j = 0; j < 6; j++) { const double h = std::fabs(H[j][j]); mx = (h < mx) ? mx : h; }
                lambda = 1e-5 * mx; ni = 2; lm_bad = 0;
            }
            int qmax = 0;
            double rho = 0;
            do {
                double x[6];
                const bool ok = solve6(H, b, lambda, x);
                const Pose Tt = oplus(x, T);
                double temp = robust_chi(E, outl, c, Tt, hub, dm, ds);
                Tl = Tt;
                if (!ok) temp = DBL_MAX;
                double scale = 0;
                for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                scale += 1e-3;
                rho = (cur - temp) / scale;
                if (rho > 0 && std::isfinite(temp)) {
                    double alpha = 1. - std::pow(2 * rho - 1, 3);
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha);
                    ni = 2; cur = temp; T = Tt;
                } else {
                    lambda *= ni; ni *= 2;
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0) break;
            if ((ini - cur) * 1e3 < ini) lm_bad++; else lm_bad = 0;
            if (lm_bad >= 3) break;
        }
        nbad = 0;
        for (size_t k = 0; k < E.size(); k++) {
            double err[3];
            const double chi = edge_err(E[k], c, outl[k] ? T : Tl, err, nullptr);
            const double th = E[k].stereo ? (double)7.815f : (double)5.991f;
            R.min_gap = std::min(R.min_gap, std::fabs(chi - th));
            outl[k] = (float)chi > (E[k].stereo ? 7.815f : 5.991f);
            nbad += outl[k];
        }
        if (E.size() < 10) break;
    }
    for (size_t k = 0; k < E.size(); k++) R.outlier[E[k].row] = outl[k];
    R.T = T;
    R.n_inliers = R.n_corr - nbad;
    return R;
}

// ------------------------------------------------------------------ scenes over the stubs
struct Scene { Frame F; std::vector<MapPoint> pts; };
static double uni(std::mt19937 &g, double a, double b) { return a + (b - a) * (g() / 4294967296.0); }
static void make_scene(Scene &S, unsigned seed, int n, double stereo_share, double init_rot, double init_trans) {
    std::mt19937 g(seed);
    Frame::fx = 458.654f; Frame::fy = 457.296f; Frame::cx = 367.215f; Frame::cy = 248.375f;
    Frame &F = S.F;
    F.mbf = 47.9f;
    F.N = n;
    F.mvInvLevelSigma2.clear();
    for (int l = 0; l < 4; l++) F.mvInvLevelSigma2.push_back((float)(1.0 / std::pow(1.2, 2 * l)));
    double w[6];
    for (int i = 0; i < 3; i++) w[i] = uni(g, -0.3, 0.3);
    for (int i = 3; i < 6; i++) w[i] = uni(g, -1, 1);
    Pose I = {{0, 0, 0, 1}, {0, 0, 0}};
    Pose gt = oplus(w, I);
    S.pts.assign(n, MapPoint());
    F.mvKeys.assign(n, cv::KeyPoint());
    F.mvuRight.assign(n, -1.f);
    F.mvpMapPoints.assign(n, nullptr);
    F.mvbOutlier.assign(n, false);
    const double qi[4] = {-gt.q[0], -gt.q[1], -gt.q[2], gt.q[3]};
    for (int i = 0; i < n; i++) {
        const double u = uni(g, 20, 714), v = uni(g, 20, 476), z = uni(g, 2, 12);
        const double d[3] = {(u - Frame::cx) / Frame::fx * z - gt.t[0], (v - Frame::cy) / Frame::fy * z - gt.t[1], z - gt.t[2]};
        double Xw[3];
        rot(qi, d, Xw);
        S.pts[i].mWorldPos = Vector3f((float)Xw[0], (float)Xw[1], (float)Xw[2]);
        const double Xf[3] = {S.pts[i].mWorldPos[0], S.pts[i].mWorldPos[1], S.pts[i].mWorldPos[2]};
        double pc[3];
        rot(gt.q, Xf, pc);
        for (int k = 0; k < 3; k++) pc[k] += gt.t[k];
        const double pu = pc[0] / pc[2] * Frame::fx + Frame::cx, pv = pc[1] / pc[2] * Frame::fy + Frame::cy;
        const bool planted = i >= 3 && uni(g, 0, 1) < 0.15;
        const double ang = uni(g, 0, 6.283185307), mag = uni(g, 30, 90);
        const double du = uni(g, -0.5, 0.5) + (planted ? mag * std::cos(ang) : 0);
        const double dv = uni(g, -0.5, 0.5) + (planted ? mag * std::sin(ang) : 0);
        const double dr = uni(g, -0.5, 0.5) + (planted ? mag * std::cos(ang) : 0);
        F.mvKeys[i].pt.x = (float)(pu + du);
        F.mvKeys[i].pt.y = (float)(pv + dv);
        F.mvKeys[i].octave = (int)(g() % 4);
        if (uni(g, 0, 1) < stereo_share) F.mvuRight[i] = (float)std::max(pu - F.mbf / pc[2] + dr, 0.0);
        if (i < 3 || uni(g, 0, 1) < 0.9) F.mvpMapPoints[i] = &S.pts[i];
        F.mvbOutlier[i] = (i % 3) == 0;  // stale flags: rows without a map point must keep them
    }
    double dx[6];
    for (int i = 0; i < 3; i++) dx[i] = uni(g, -1, 1) * init_rot;
    for (int i = 3; i < 6; i++) dx[i] = uni(g, -1, 1) * init_trans;
    const Pose T0 = oplus(dx, gt);
    F.mTcw = SE3f(Eigen::Quaternionf((float)T0.q[3], (float)T0.q[0], (float)T0.q[1], (float)T0.q[2]),
                  Vector3f((float)T0.t[0], (float)T0.t[1], (float)T0.t[2]));
}

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

static void check_case(const char *name, unsigned seed, int n, double ss, double rot0, double tr0) {
    Scene S;
    make_scene(S, seed, n, ss, rot0, tr0);
    Frame &mCurrentFrame = S.F;
    const RefResult R = ref_pose_opt(&mCurrentFrame);
    const std::vector<bool> before = mCurrentFrame.mvbOutlier;
    CHECK(R.min_gap >= 1e-5, "%s: an edge sits %.2e from a threshold (choose another seed)", name, R.min_gap);
    // Tracking.cc:2212-2239
    std::set<MapPoint *> mvpDirectMapPointsCache;
    for (int i = 0; i < mCurrentFrame.N; i++)
        if (mCurrentFrame.mvpMapPoints[i]) mvpDirectMapPointsCache.insert(mCurrentFrame.mvpMapPoints[i]);
    const bool mbOnlyTracking = false;
    const int ret = Optimizer::PoseOptimization(&mCurrentFrame);
    int mnMatchesInliers = 0;
    for (int i = 0; i < mCurrentFrame.N; i++) {
        if (mCurrentFrame.mvpMapPoints[i]) {
            if (!mCurrentFrame.mvbOutlier[i]) {
                if (!mbOnlyTracking) {
                    if (mCurrentFrame.mvpMapPoints[i]->Observations() > 0)
                        mnMatchesInliers++;
                } else
                    mnMatchesInliers++;
            } else {
                auto iter = mvpDirectMapPointsCache.find(mCurrentFrame.mvpMapPoints[i]);
                if (iter != mvpDirectMapPointsCache.end())
                    mvpDirectMapPointsCache.erase(iter);
            }
        }
    }
    CHECK(ret == R.n_inliers, "%s: return %d, restatement %d", name, ret, R.n_inliers);
    int flag_diff = 0, stale_diff = 0;
    for (int i = 0; i < mCurrentFrame.N; i++) {
        if (R.outlier[i] == 2 || R.n_corr < 3) stale_diff += mCurrentFrame.mvbOutlier[i] != before[i];
        else flag_diff += mCurrentFrame.mvbOutlier[i] != (R.outlier[i] != 0);
    }
    CHECK(flag_diff == 0, "%s: %d flags differ", name, flag_diff);
    CHECK(stale_diff == 0, "%s: %d rows without a map point were written", name, stale_diff);
    CHECK(R.n_corr < 3 || mnMatchesInliers == R.n_inliers, "%s: mnMatchesInliers %d", name, mnMatchesInliers);
    CHECK(R.n_corr < 3 || (int)mvpDirectMapPointsCache.size() == R.n_inliers, "%s: cache %zu", name, mvpDirectMapPointsCache.size());
    // SetPose(estimate.cast<float>()): the float pose of the double estimate, one float ulp allowed
    const float got[7] = {mCurrentFrame.mTcw.unit_quaternion().x(), mCurrentFrame.mTcw.unit_quaternion().y(),
                          mCurrentFrame.mTcw.unit_quaternion().z(), mCurrentFrame.mTcw.unit_quaternion().w(),
                          mCurrentFrame.mTcw.translation()[0], mCurrentFrame.mTcw.translation()[1],
                          mCurrentFrame.mTcw.translation()[2]};
    double worst = 0;
    for (int k = 0; k < 7; k++) {
        const double want = k < 4 ? R.T.q[k] : R.T.t[k - 4];
        worst = std::max(worst, std::fabs((double)got[k] - (double)(float)want) / std::max(1.0, std::fabs(want)));
    }
    CHECK(worst <= 1.2e-7, "%s: float pose differs by %.3e", name, worst);
    printf("%-28s n_corr %4d inliers %4d (restatement %4d) float-pose diff %.1e  %s\n", name, R.n_corr, ret, R.n_inliers,
           worst, g_fail ? "FAILED" : "ok");
}

template <class Fn>
static double median_ms(int reps, Fn fn) {
    std::vector<double> v;
    for (int i = 0; i < reps; i++) {
        const auto a = std::chrono::steady_clock::now();
        fn();
        v.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count());
    }
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

#define HIPCHK(x) do { if ((x) != hipSuccess) { printf("FAILED hip call %s\n", #x); return 1; } } while (0)
static int run_time() {
    Scene S;
    make_scene(S, 77, 1000, 0.4, 0.02, 0.05);
    const SE3f T0 = S.F.mTcw;
    const double gpu_ms = median_ms(31, [&] { S.F.mTcw = T0; Optimizer::PoseOptimization(&S.F); });
    S.F.mTcw = T0;
    const double cpu_ms = median_ms(31, [&] { S.F.mTcw = T0; ref_pose_opt(&S.F); });
    printf("TIMING pose_optimization_1000 dropin_call_ms %.3f cpu_restatement_ms %.3f\n", gpu_ms, cpu_ms);
    // 32 relocalisation candidates: one batch launch on device-resident arrays against 32 CPU runs
    const int P = 32;
    std::vector<Scene> C(P);
    std::vector<gpu::PoseProblem> pr(P);
    std::vector<int32_t> ptr(1, 0);
    std::vector<ygzfe_camera> cam;
    std::vector<float> bf, ur, xw;
    std::vector<ygzfe_se3> Ti;
    std::vector<ygzfe_kp> kps;
    std::vector<uint8_t> present;
    for (int p = 0; p < P; p++) {
        make_scene(C[p], 100 + p, 300 + 20 * p, 0.4, 0.02, 0.05);
        gpu::GatherPoseProblem(&C[p].F, pr[p]);
        ptr.push_back(ptr.back() + C[p].F.N);
        cam.push_back(pr[p].cam); bf.push_back(pr[p].bf); Ti.push_back(pr[p].T);
        kps.insert(kps.end(), pr[p].kps.begin(), pr[p].kps.end());
        ur.insert(ur.end(), pr[p].u_right.begin(), pr[p].u_right.end());
        xw.insert(xw.end(), pr[p].xw.begin(), pr[p].xw.end());
        present.insert(present.end(), pr[p].present.begin(), pr[p].present.end());
    }
    const int n = ptr.back();
    const std::vector<float> &sig = C[0].F.mvInvLevelSigma2;
    void *d_ptr, *d_cam, *d_bf, *d_T, *d_kps, *d_ur, *d_xw, *d_pr, *d_sig, *d_out, *d_res;
#define UP(d, v) HIPCHK(hipMalloc(&d, v.size() * sizeof(v[0]))); HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice))
    UP(d_ptr, ptr); UP(d_cam, cam); UP(d_bf, bf); UP(d_T, Ti); UP(d_kps, kps); UP(d_ur, ur); UP(d_xw, xw); UP(d_pr, present);
    UP(d_sig, sig);
    HIPCHK(hipMalloc(&d_out, n));
    HIPCHK(hipMalloc(&d_res, P * sizeof(ygzfe_pose_opt_result)));
    int rc = 0;
    const double batch_ms = median_ms(31, [&] {
        rc |= ygzfe_pose_optimization_batch(dropin::device(), P, (const int32_t *)d_ptr, (const ygzfe_camera *)d_cam,
                                            (const float *)d_bf, (const ygzfe_se3 *)d_T, (const ygzfe_kp *)d_kps,
                                            (const float *)d_ur, (const float *)d_xw, (const uint8_t *)d_pr,
                                            (const float *)d_sig, (int)sig.size(), (uint8_t *)d_out,
                                            (ygzfe_pose_opt_result *)d_res, nullptr);
        (void)hipStreamSynchronize(nullptr);
    });
    CHECK(rc == 0, "batch launch: %s", ygzfe_last_error());
    std::vector<ygzfe_pose_opt_result> res(P);
    HIPCHK(hipMemcpy(res.data(), d_res, P * sizeof(res[0]), hipMemcpyDeviceToHost));
    int inl_diff = 0;
    std::vector<RefResult> refs(P);
    const double cpu32_ms = median_ms(5, [&] { for (int p = 0; p < P; p++) refs[p] = ref_pose_opt(&C[p].F); });
    for (int p = 0; p < P; p++) inl_diff += res[p].n_inliers != refs[p].n_inliers;
    CHECK(inl_diff == 0, "%d batch problems differ from the restatement in n_inliers", inl_diff);
    printf("TIMING pose_optimization_batch_32 (%d edges) batch_ms %.3f cpu_32_sequential_ms %.3f\n", n, batch_ms, cpu32_ms);
    for (void *d : {d_ptr, d_cam, d_bf, d_T, d_kps, d_ur, d_xw, d_pr, d_sig, d_out, d_res}) (void)hipFree(d);
    return 0;
}

int main(int argc, char **argv) {
    check_case("mixed-1000", 11, 1000, 0.4, 0.02, 0.05);
    check_case("mono-300", 12, 300, 0.0, 0.02, 0.05);
    check_case("stereo-257", 13, 257, 1.0, 0.02, 0.05);
    check_case("mixed-9 (one round)", 14, 9, 0.4, 0.02, 0.05);
    check_case("mixed-2 (nothing written)", 15, 2, 0.5, 0.02, 0.05);
    check_case("mixed-120 far start", 16, 120, 0.3, 0.3, 0.8);
    if (argc > 1 && !strcmp(argv[1], "--time") && run_time()) g_fail++;
    printf(g_fail ? "FAILED\n" : "OK\n");
    return g_fail ? 1 : 0;
}
