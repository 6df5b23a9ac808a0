// The reference's call site of ORBmatcher::SearchForTriangulation (LocalMapping.cc:1037-1042) over a test stub
// of KeyFrame, with the drop-in body (compat/dropin/ORBmatcher_mapping_gpu.inc), per neighbour and through
// gpu::SearchForTriangulationAll, against a plain C++ restatement of ORBmatcher.cc:597-746 inside this program
// (test only; built with -ffp-contract=off).  --time: median ms of the drop-in calls and of the restatement
// on one core, for one neighbour and for 20 neighbours of ~1,000-keypoint keyframes.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "KeyFrame.h"
#include "ORBmatcher.h"
#include "ORBmatcherMappingGPU.h"

namespace ygz {
#include "ORBmatcher_mapping_gpu.inc"
}  // namespace ygz
using namespace ygz;

typedef std::vector<std::pair<size_t, size_t> > Pairs;
static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

// ------------------------------------------------------------------ restatement of ORBmatcher.cc:597-746
static int popcount256(const uint8_t *a, const uint8_t *b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

static bool on_epipolar_line(const cv::KeyPoint &kp1, const cv::KeyPoint &kp2, const Matrix3f &F12, KeyFrame *pKF2) {  // :136-153
    const float a = kp1.pt.x * F12(0, 0) + kp1.pt.y * F12(1, 0) + F12(2, 0);
    const float b = kp1.pt.x * F12(0, 1) + kp1.pt.y * F12(1, 1) + F12(2, 1);
    const float c = kp1.pt.x * F12(0, 2) + kp1.pt.y * F12(1, 2) + F12(2, 2);
    const float num = a * kp2.pt.x + b * kp2.pt.y + c;
    const float den = a * a + b * b;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return dsqr < 3.84 * pKF2->mvLevelSigma2[kp2.octave];
}

static int ref_search(KeyFrame *pKF1, KeyFrame *pKF2, const Matrix3f &F12, Pairs &pairs, bool only_stereo, bool check_ori) {
    const Vector3f C2 = pKF2->GetRotation() * pKF1->GetCameraCenter() + pKF2->GetTranslation();
    const float invz = 1.0f / C2[2];
    const float ex = pKF2->fx * C2[0] * invz + pKF2->cx, ey = pKF2->fy * C2[1] * invz + pKF2->cy;
    int nmatches = 0;
    std::vector<int> m12(pKF1->N, -1);
    std::vector<int> hist[30];
    auto it1 = pKF1->mFeatVec.begin(), it2 = pKF2->mFeatVec.begin();
    while (it1 != pKF1->mFeatVec.end() && it2 != pKF2->mFeatVec.end()) {
        if (it1->first < it2->first) { it1 = pKF1->mFeatVec.lower_bound(it2->first); continue; }
        if (it2->first < it1->first) { it2 = pKF2->mFeatVec.lower_bound(it1->first); continue; }
        for (size_t p1 = 0; p1 < it1->second.size(); p1++) {
            const size_t idx1 = it1->second[p1];
            if (pKF1->GetMapPoint(idx1)) continue;
            const bool stereo1 = pKF1->mvuRight[idx1] >= 0;
            if (only_stereo && !stereo1) continue;
            const cv::KeyPoint &kp1 = pKF1->mvKeys[idx1];
            int best_dist = 50, best = -1;
            for (size_t p2 = 0; p2 < it2->second.size(); p2++) {
                const size_t idx2 = it2->second[p2];
                if (pKF2->GetMapPoint(idx2)) continue;  // vbMatched2 is never set in this reference
                const bool stereo2 = pKF2->mvuRight[idx2] >= 0;
                if (only_stereo && !stereo2) continue;
                const int dist = popcount256(pKF1->mDescriptors.ptr<uint8_t>((int)idx1), pKF2->mDescriptors.ptr<uint8_t>((int)idx2));
                if (dist > 50 || dist > best_dist) continue;
                const cv::KeyPoint &kp2 = pKF2->mvKeys[idx2];
                if (!stereo1 && !stereo2) {
                    const float dx = ex - kp2.pt.x, dy = ey - kp2.pt.y;
                    if (dx * dx + dy * dy < 100 * pKF2->mvScaleFactors[kp2.octave]) continue;
                }
                if (on_epipolar_line(kp1, kp2, F12, pKF2)) { best = (int)idx2; best_dist = dist; }
            }
            if (best < 0) continue;
            m12[idx1] = best;
            nmatches++;
            if (check_ori) {
                float rot = kp1.angle - pKF2->mvKeys[best].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)std::round(rot * (1.0f / 30));
                if (bin == 30) bin = 0;
                hist[bin].push_back((int)idx1);
            }
        }
        ++it1;
        ++it2;
    }
    if (check_ori) {
        int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;  // ComputeThreeMaxima :1471-1502
        for (int i = 0; i < 30; i++) {
            const int s = (int)hist[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
            else if (s > max3) { max3 = s; i3 = i; }
        }
        if (max2 < 0.1f * (float)max1) i2 = i3 = -1;
        else if (max3 < 0.1f * (float)max1) i3 = -1;
        for (int i = 0; i < 30; i++) {
            if (i == i1 || i == i2 || i == i3) continue;
            for (size_t j = 0; j < hist[i].size(); j++) { m12[hist[i][j]] = -1; nmatches--; }
        }
    }
    pairs.clear();
    for (size_t i = 0; i < m12.size(); i++)
        if (m12[i] >= 0) pairs.push_back(std::make_pair(i, (size_t)m12[i]));
    return nmatches;
}

// ------------------------------------------------------------------ scene
static const float kFx = 458.654f, kFy = 457.296f, kCx = 367.215f, kCy = 248.375f;  // EuRoC cam0

static Matrix3f mul(const Matrix3f &a, const Matrix3f &b) {
    Matrix3f r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r(i, j) = a(i, 0) * b(0, j) + a(i, 1) * b(1, j) + a(i, 2) * b(2, j);
    return r;
}

// LocalMapping::ComputeF12 (LocalMapping.cc:1294-1308): K1^-T [t12]x R12 K2^-1
static Matrix3f compute_f12(KeyFrame *k1, KeyFrame *k2) {
    const Matrix3f R1w = k1->GetRotation(), R2w = k2->GetRotation();
    const Vector3f t1w = k1->GetTranslation(), t2w = k2->GetTranslation();
    const Matrix3f R12 = mul(R1w, R2w.transpose());
    const Vector3f rt = R12 * t2w, t12(t1w[0] - rt[0], t1w[1] - rt[1], t1w[2] - rt[2]);
    Matrix3f tx, K1iT, K2i;
    tx(0, 1) = -t12[2]; tx(0, 2) = t12[1]; tx(1, 0) = t12[2]; tx(1, 2) = -t12[0]; tx(2, 0) = -t12[1]; tx(2, 1) = t12[0];
    K1iT(0, 0) = 1 / k1->fx; K1iT(1, 1) = 1 / k1->fy; K1iT(2, 0) = -k1->cx / k1->fx; K1iT(2, 1) = -k1->cy / k1->fy; K1iT(2, 2) = 1;
    K2i(0, 0) = 1 / k2->fx; K2i(1, 1) = 1 / k2->fy; K2i(0, 2) = -k2->cx / k2->fx; K2i(1, 2) = -k2->cy / k2->fy; K2i(2, 2) = 1;
    return mul(mul(K1iT, tx), mul(R12, K2i));
}

struct World {
    std::vector<Vector3f> pts;
    std::vector<std::vector<uint8_t> > desc;
    std::vector<float> angle;
    std::vector<unsigned> node;
};
static MapPoint g_some_map_point;

// a keyframe at pose T_cw: the world points it sees (each with a few descriptor bits flipped and pixel noise of
// its octave), now and then a twin with the same descriptor next to it (equal distances in one node), and
// unrelated keypoints, some angles turned by 90 or 150 degrees; about half with a map point, a third stereo; the node lists in shuffled order
static void make_keyframe(KeyFrame &kf, const World &w, const SE3f &T, int n_target, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    kf = KeyFrame();
    kf.fx = kFx; kf.fy = kFy; kf.cx = kCx; kf.cy = kCy;
    kf.mTcw = T;
    for (int l = 0; l < 4; l++) { kf.mvScaleFactors.push_back((float)(1 << l)); kf.mvLevelSigma2.push_back((float)(1 << (2 * l))); }
    std::vector<std::vector<uint8_t> > rows;
    std::vector<unsigned> nodes;
    auto add = [&](float x, float y, int oct, float ang, const std::vector<uint8_t> &d, unsigned node) {
        kf.mvKeys.push_back(cv::KeyPoint(cv::Point2f(x, y), 31.f * (1 << oct), ang, 10.f, oct));
        kf.mvuRight.push_back(U(rng) < 0.35f ? x - 20.f : -1.f);
        kf.mvpMapPoints.push_back(U(rng) < 0.5f ? &g_some_map_point : NULL);
        rows.push_back(d);
        nodes.push_back(node);
    };
    for (size_t i = 0; i < w.pts.size() && (int)rows.size() < n_target * 3 / 4; i++) {
        const Vector3f Pc = T * w.pts[i];
        if (Pc[2] < 0.5f) continue;
        const int oct = (int)(U(rng) * 4) & 3;
        const float s = 0.6f * (1 << oct);
        const float x = kFx * Pc[0] / Pc[2] + kCx + (U(rng) - 0.5f) * s, y = kFy * Pc[1] / Pc[2] + kCy + (U(rng) - 0.5f) * s;
        if (x < 0 || x >= 752 || y < 0 || y >= 480) continue;
        std::vector<uint8_t> d = w.desc[i];
        for (int f = (int)(U(rng) * 12); f > 0; f--) { const int b = (int)(U(rng) * 256) & 255; d[b >> 3] ^= (uint8_t)(1 << (b & 7)); }
        const float turn = U(rng);  // now and then a keypoint turned away: rotation bins the three maxima drop
        add(x, y, oct, std::fmod(w.angle[i] + U(rng) * 8.f + (turn < 0.04f ? 90.f : turn < 0.08f ? 150.f : 0.f), 360.f), d, w.node[i]);
        if (U(rng) < 0.08f) add(x + 0.25f, y, oct, w.angle[i], d, w.node[i]);  // the twin
    }
    while ((int)rows.size() < n_target) {
        std::vector<uint8_t> d(32);
        for (int b = 0; b < 32; b++) d[b] = (uint8_t)(rng() & 255);
        add(U(rng) * 752, U(rng) * 480, (int)(U(rng) * 4) & 3, U(rng) * 360.f, d, (unsigned)(rng() % 120));
    }
    kf.N = (int)rows.size();
    kf.mDescriptors.create(kf.N, 32, CV_8U);
    std::vector<unsigned> order(kf.N);
    for (int i = 0; i < kf.N; i++) { order[i] = i; memcpy(kf.mDescriptors.ptr<uint8_t>(i), rows[i].data(), 32); }
    std::shuffle(order.begin(), order.end(), rng);
    for (int i = 0; i < kf.N; i++) kf.mFeatVec[nodes[order[i]]].push_back(order[i]);
}

struct Scene {
    KeyFrame kf1;
    std::vector<KeyFrame> nb;
    std::vector<KeyFrame *> pnb;
    std::vector<Matrix3f> F12;
};
static void make_scene(Scene &S, int n_nb, int n_kp, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    World w;
    for (int i = 0; i < 4 * n_kp; i++) {
        w.pts.push_back(Vector3f(U(rng) * 3.5f, U(rng) * 2.3f, 4.f + U(rng) * 1.5f));
        std::vector<uint8_t> d(32);
        for (int b = 0; b < 32; b++) d[b] = (uint8_t)(rng() & 255);
        w.desc.push_back(d);
        w.angle.push_back((U(rng) + 1.f) * 170.f);
        w.node.push_back((unsigned)(rng() % 100) * 3 + 1);
    }
    make_keyframe(S.kf1, w, SE3f(), n_kp, seed * 31 + 1);
    S.nb.resize(n_nb);
    for (int k = 0; k < n_nb; k++) {
        const float ax = 0.03f * U(rng), ay = 0.03f * U(rng), az = 0.03f * U(rng), nq = std::sqrt(1 + ax * ax + ay * ay + az * az);
        // every third neighbour moves mostly forward: its epipole lies inside the image
        const Vector3f t = k % 3 == 0 ? Vector3f(0.02f * U(rng), 0.02f * U(rng), -0.25f) : Vector3f(0.25f * U(rng), 0.15f * U(rng), 0.05f * U(rng));
        make_keyframe(S.nb[k], w, SE3f(Eigen::Quaternionf(1 / nq, ax / nq, ay / nq, az / nq), t), n_kp - 7 * k, seed * 31 + 2 + k);
    }
    for (int k = 0; k < n_nb; k++) {
        S.pnb.push_back(&S.nb[k]);
        S.F12.push_back(compute_f12(&S.kf1, &S.nb[k]));
    }
}

static bool same(const Pairs &a, const Pairs &b) { return a == b; }

// LocalMapping.cc:1037-1042 for every neighbour, per neighbour and through SearchForTriangulationAll
static void run_case(const char *name, int n_nb, int n_kp, unsigned seed, bool only_stereo, bool check_ori, int min_matches) {
    Scene S;
    make_scene(S, n_nb, n_kp, seed);
    ORBmatcher matcher(0.6, check_ori);
    KeyFrame *mpCurrentKeyFrame = &S.kf1;
    int total = 0, worst = 1 << 30;
    std::vector<Pairs> want(n_nb);
    std::vector<int> want_n(n_nb);
    for (int i = 0; i < n_nb; i++) {
        KeyFrame *pKF2 = S.pnb[i];
        Matrix3f F12 = S.F12[i];
        vector<pair<size_t, size_t> > vMatchedIndices;
        const int got = matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, only_stereo);
        want_n[i] = ref_search(mpCurrentKeyFrame, pKF2, F12, want[i], only_stereo, check_ori);
        CHECK(got == want_n[i], "%s neighbour %d: returned %d, restatement %d", name, i, got, want_n[i]);
        CHECK(same(vMatchedIndices, want[i]), "%s neighbour %d: pairs differ (%zu against %zu)", name, i, vMatchedIndices.size(), want[i].size());
        CHECK((int)want[i].size() == want_n[i], "%s neighbour %d: nmatches against pairs", name, i);
        total += want_n[i];
        worst = std::min(worst, want_n[i]);
    }
    std::vector<Pairs> all;
    const std::vector<int> n_all = gpu::SearchForTriangulationAll(mpCurrentKeyFrame, S.pnb, S.F12, only_stereo, all, check_ori);
    CHECK(n_all == want_n, "%s: SearchForTriangulationAll return values", name);
    for (int i = 0; i < n_nb; i++) CHECK(same(all[i], want[i]), "%s neighbour %d: SearchForTriangulationAll pairs differ", name, i);
    CHECK(n_nb == 0 || worst >= min_matches, "%s: only %d matches on some neighbour (the case tests little)", name, worst);
    printf("%-28s %2d neighbours x %4d keypoints: %5d matches (min %d per neighbour) %s\n", name, n_nb, n_kp, total,
           n_nb ? worst : 0, g_fail ? "FAILED" : "ok");
}

template <class Fn>
static double median_ms(int reps, Fn fn) {
    std::vector<double> v;
    for (int r = 0; r < reps; r++) {
        const auto a = std::chrono::steady_clock::now();
        fn();
        v.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count());
    }
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

static void run_time() {
    Scene S;
    make_scene(S, 20, 1000, 77);
    ORBmatcher matcher(0.6, false);
    Pairs p;
    std::vector<Pairs> all;
    int sink = 0;
    auto one_gpu = [&] { Matrix3f F = S.F12[0]; sink += matcher.SearchForTriangulation(&S.kf1, S.pnb[0], F, p, false); };
    auto all_gpu = [&] { sink += gpu::SearchForTriangulationAll(&S.kf1, S.pnb, S.F12, false, all)[0]; };
    for (int i = 0; i < 5; i++) { one_gpu(); all_gpu(); }  // warm-up: uploads, staging, code objects
    const double g1 = median_ms(51, one_gpu);
    const double c1 = median_ms(21, [&] { sink += ref_search(&S.kf1, S.pnb[0], S.F12[0], p, false, false); });
    printf("TIMING search_for_triangulation_1 (%d x %d keypoints) dropin_call_ms %.3f cpu_restatement_ms %.3f\n", S.kf1.N, S.nb[0].N, g1, c1);
    const double g20 = median_ms(51, all_gpu);
    const double s20 = median_ms(21, [&] { for (int k = 0; k < 20; k++) { Matrix3f F = S.F12[k]; sink += matcher.SearchForTriangulation(&S.kf1, S.pnb[k], F, p, false); } });
    const double c20 = median_ms(11, [&] { for (int k = 0; k < 20; k++) sink += ref_search(&S.kf1, S.pnb[k], S.F12[k], p, false, false); });
    printf("TIMING search_for_triangulation_batch_20 batch_ms %.3f dropin_20_calls_ms %.3f cpu_20_sequential_ms %.3f (sink %d)\n", g20, s20, c20, sink);
}

int main(int argc, char **argv) {
    run_case("mapping-10", 10, 1000, 3, false, false, 30);       // CreateNewMapPoints: matcher(0.6, false), bOnlyStereo false
    run_case("mapping-10 checkOri", 10, 1000, 4, false, true, 30);
    run_case("mapping-3 onlyStereo", 3, 1000, 5, true, true, 1);
    run_case("mono-20 small", 20, 300, 6, false, false, 5);
    run_case("one neighbour, odd size", 1, 333, 7, false, true, 5);
    run_case("no neighbour", 0, 100, 8, false, false, 0);
    if (argc > 1 && !strcmp(argv[1], "--time")) run_time();
    printf(g_fail ? "FAILED\n" : "OK\n");
    return g_fail ? 1 : 0;
}
