// LocalMapping::SearchInNeighbors' two Fuse phases (LocalMapping.cc:1262-1306) over test stubs of KeyFrame and
// MapPoint (tests/dropin/stubs_fuse), run twice on two identical copies of a synthetic map: with the drop-in
// (compat/dropin/ORBmatcherFuseGPU.h: gpu::FuseAll for the forward phase, ORBmatcher::Fuse for the backward one) and
// with a plain C++ restatement of ORBmatcher.cc:748-886 inside this program (test only; -ffp-contract=off).  The
// complete final state is compared: every keyframe's mvpMapPoints, every point's bad flag, observations and
// descriptor, and the nFused returns.  One crafted map has a Replace in target 0 that changes a candidate's
// descriptor before target 1.  --time: the drop-in against the restatement on one core.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "KeyFrame.h"
#include "ORBmatcher.h"
#include "ORBmatcherFuseGPU.h"

namespace ygz {
#include "ORBmatcher_fuse_gpu.inc"
}  // namespace ygz
using namespace ygz;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)
static long g_ref_pairs = 0, g_ref_survivors = 0;

// ------------------------------------------------------------------ restatement of ORBmatcher.cc:748-886
static int ref_fuse(KeyFrame *pKF, const std::vector<MapPoint *> &points, float th) {
    const Matrix3f Rcw = pKF->GetRotation();
    const Vector3f tcw = pKF->GetTranslation(), Ow = pKF->GetCameraCenter();
    int nFused = 0;
    for (size_t i = 0; i < points.size(); i++) {
        MapPoint *pMP = points[i];
        if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        g_ref_pairs++;
        const Vector3f Pw = pMP->GetWorldPos();
        const Vector3f Pc = Rcw * Pw + tcw;
        if (Pc[2] < 0.0f) continue;
        const float invz = 1 / Pc[2];
        const float u = pKF->fx * (Pc[0] * invz) + pKF->cx, v = pKF->fy * (Pc[1] * invz) + pKF->cy;
        if (!pKF->IsInImage(u, v)) continue;
        const float ur = u - pKF->mbf * invz;
        const Vector3f PO = Pw - Ow;
        const float dist3D = PO.norm();
        if (dist3D < pMP->GetMinDistanceInvariance() || dist3D > pMP->GetMaxDistanceInvariance()) continue;
        const Vector3f Pn = pMP->GetNormal();
        if (PO[0] * Pn[0] + PO[1] * Pn[1] + PO[2] * Pn[2] < 0.5 * dist3D) continue;
        const int level = pMP->PredictScale(dist3D, pKF);
        g_ref_survivors++;
        const std::vector<size_t> cand = pKF->GetFeaturesInArea(u, v, th * pKF->mvScaleFactors[level]);
        const cv::Mat dMP = pMP->GetDescriptor();
        int bestDist = 256, bestIdx = -1;
        for (size_t c = 0; c < cand.size(); c++) {
            const size_t idx = cand[c];
            const cv::KeyPoint &kp = pKF->mvKeys[idx];
            if (kp.octave < level - 1 || kp.octave > level) continue;
            const float ex = u - kp.pt.x, ey = v - kp.pt.y;
            if (pKF->mvuRight[idx] >= 0) {
                const float er = ur - pKF->mvuRight[idx];
                if ((ex * ex + ey * ey + er * er) * pKF->mvInvLevelSigma2[kp.octave] > 7.8) continue;
            } else if ((ex * ex + ey * ey) * pKF->mvInvLevelSigma2[kp.octave] > 5.99) {
                continue;
            }
            const int d = gpu::fuse_distance(dMP.ptr<uint8_t>(0), pKF->mDescriptors.ptr<uint8_t>((int)idx));
            if (d < bestDist) bestDist = d, bestIdx = (int)idx;
        }
        if (bestDist <= 50) {
            MapPoint *in = pKF->GetMapPoint(bestIdx);
            if (in) {
                if (!in->isBad()) {
                    if (in->Observations() > pMP->Observations()) pMP->Replace(in);
                    else in->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, bestIdx);
                pKF->AddMapPoint(pMP, bestIdx);
            }
            nFused++;
        }
    }
    return nFused;
}

// ------------------------------------------------------------------ a synthetic map
struct World {
    std::vector<std::unique_ptr<KeyFrame> > kfs;  // [0] the current keyframe, the rest its targets
    std::vector<std::unique_ptr<MapPoint> > pts;
    MapPoint *new_point() {
        pts.emplace_back(new MapPoint());
        pts.back()->mnId = (long)pts.size() - 1;
        return pts.back().get();
    }
};

static const int kLevels = 8;
static void init_keyframe(KeyFrame &K, long id, const SE3f &Tcw) {
    K.mnId = id;
    K.mTcw = Tcw;
    K.fx = K.fy = 458.0f;
    K.cx = 376.0f;
    K.cy = 240.0f;
    K.mbf = 458.0f * 0.11f;
    K.mnMinX = 0.f, K.mnMaxX = 752.f, K.mnMinY = 0.f, K.mnMaxY = 480.f;
    K.mnScaleLevels = kLevels;
    K.mfLogScaleFactor = std::log(1.2f);
    float s = 1.f;
    for (int l = 0; l < kLevels; l++, s *= 1.2f) K.mvScaleFactors.push_back(s), K.mvInvLevelSigma2.push_back(1.0f / (s * s));
}
static void finish_keyframe(KeyFrame &K, const std::vector<std::vector<uint8_t> > &desc) {
    K.N = (int)K.mvKeys.size();
    K.mDescriptors.create(std::max(K.N, 1), 32, CV_8U);
    for (int i = 0; i < K.N; i++) std::memcpy(K.mDescriptors.ptr<uint8_t>(i), desc[i].data(), 32);
    K.mvpMapPoints.resize(K.N, nullptr);
    K.AssignFeaturesToGrid();
}
static void observe(MapPoint *p, KeyFrame *K, size_t idx) {
    p->AddObservation(K, idx);
    K->AddMapPoint(p, idx);
}

// n_kf keyframes around the origin looking at n_land landmarks 4-8 m ahead; each keyframe sees a landmark as one
// keypoint (noisy position, a few descriptor bits flipped), and the keyframes that see it share one of two map
// points or leave the keypoint free: duplicates to Replace and free keypoints to AddObservation.
static void build_world(World &W, unsigned seed, int n_kf, int n_land) {
    std::mt19937 rng(seed);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    auto gauss = [&](float s) { return std::normal_distribution<float>(0.f, s)(rng); };
    std::vector<Vector3f> land(n_land);
    std::vector<std::vector<uint8_t> > base(n_land, std::vector<uint8_t>(32));
    std::vector<int> oct(n_land);
    for (int l = 0; l < n_land; l++) {
        land[l] = Vector3f(uni(-5.f, 5.f), uni(-3.f, 3.f), uni(4.f, 8.f));
        for (int b = 0; b < 32; b++) base[l][b] = (uint8_t)(rng() & 255);
        oct[l] = (int)(rng() % 4);
    }
    std::vector<MapPoint *> group(2 * (size_t)n_land, nullptr);
    for (int k = 0; k < n_kf; k++) {
        const float ax = uni(-0.04f, 0.04f), ay = uni(-0.04f, 0.04f), az = uni(-0.02f, 0.02f);
        const float nq = std::sqrt(1.f + (ax * ax + ay * ay + az * az) / 4);
        const SE3f T(Eigen::Quaternionf(1.f / nq, ax / 2 / nq, ay / 2 / nq, az / 2 / nq),
                     Vector3f(uni(-0.4f, 0.4f), uni(-0.3f, 0.3f), uni(-0.3f, 0.3f)));
        W.kfs.emplace_back(new KeyFrame());
        KeyFrame &K = *W.kfs.back();
        init_keyframe(K, k, T);
        std::vector<std::vector<uint8_t> > desc;
        std::vector<int> seen;
        for (int l = 0; l < n_land; l++) {
            const Vector3f Pc = T * land[l];
            const float u = K.fx * Pc[0] / Pc[2] + K.cx + gauss(0.6f), v = K.fy * Pc[1] / Pc[2] + K.cy + gauss(0.6f);
            if (!(u >= 2 && u < 750 && v >= 2 && v < 478) || rng() % 8 == 0) continue;
            K.mvKeys.push_back(cv::KeyPoint(cv::Point2f(u, v), 31.f, 0.f, 1.f, oct[l]));
            K.mvuRight.push_back(rng() % 2 ? u - K.mbf / Pc[2] + gauss(0.4f) : -1.f);
            std::vector<uint8_t> d = base[l];
            for (int f = (int)(rng() % 9); f > 0; f--) d[rng() % 32] ^= (uint8_t)(1u << (rng() % 8));
            desc.push_back(d);
            seen.push_back(l);
        }
        for (int c = 0; c < n_land / 4; c++) {  // clutter
            K.mvKeys.push_back(cv::KeyPoint(cv::Point2f(uni(2, 750), uni(2, 478)), 31.f, 0.f, 1.f, (int)(rng() % 4)));
            K.mvuRight.push_back(-1.f);
            std::vector<uint8_t> d(32);
            for (int b = 0; b < 32; b++) d[b] = (uint8_t)(rng() & 255);
            desc.push_back(d);
        }
        finish_keyframe(K, desc);
        const Vector3f Ow = K.GetCameraCenter();
        for (size_t i = 0; i < seen.size(); i++) {
            const unsigned r = rng() % 10;
            if (r < 4) continue;  // a free keypoint
            MapPoint *&p = group[2 * (size_t)seen[i] + (r & 1)];
            if (!p) {
                p = W.new_point();
                p->mWorldPos = land[seen[i]] + Vector3f(gauss(0.004f), gauss(0.004f), gauss(0.004f));
                const Vector3f PO = p->mWorldPos - Ow;
                const float d = PO.norm();
                p->mNormalVector = Vector3f(PO[0] / d, PO[1] / d, PO[2] / d);
                p->mfMaxDistance = d * K.mvScaleFactors[oct[seen[i]]];
                p->mfMinDistance = p->mfMaxDistance / K.mvScaleFactors[kLevels - 1];
            }
            observe(p, &K, i);
        }
    }
    for (size_t i = 0; i < W.pts.size(); i++) W.pts[i]->ComputeDistinctiveDescriptors();
}

// The crafted map: current keyframe C (id 0) holds point A; target T0 holds point B at the keypoint A matches, with
// as many observations, so B->Replace(A) runs and A's descriptor is recomputed from C's and T0's keypoints (C's
// wins: least median, first on ties) instead of the one it carried; target T1's keypoint is within TH_LOW of the
// carried descriptor only, so a stale search would fuse there and the reference does not.
static std::vector<uint8_t> bits(int from, int n) {
    std::vector<uint8_t> d(32, 0);
    for (int b = from; b < from + n; b++) d[b / 8] |= (uint8_t)(1u << (b % 8));
    return d;
}
static void build_crafted(World &W) {
    const Vector3f P(0.f, 0.f, 5.f);
    const std::vector<uint8_t> carried = bits(0, 0), in_c = bits(0, 40), in_t0 = bits(0, 20), in_t1 = bits(100, 30);
    const std::vector<uint8_t> kd[3] = {in_c, in_t0, in_t1};
    for (int k = 0; k < 3; k++) {
        W.kfs.emplace_back(new KeyFrame());
        KeyFrame &K = *W.kfs.back();
        init_keyframe(K, k, SE3f(Eigen::Quaternionf(), Vector3f(0.05f * k, 0.f, 0.f)));
        const Vector3f Pc = K.mTcw * P;
        K.mvKeys.push_back(cv::KeyPoint(cv::Point2f(K.fx * Pc[0] / Pc[2] + K.cx, K.fy * Pc[1] / Pc[2] + K.cy), 31.f, 0.f, 1.f, 0));
        K.mvuRight.push_back(-1.f);
        finish_keyframe(K, std::vector<std::vector<uint8_t> >(1, kd[k]));
    }
    for (int j = 0; j < 2; j++) {  // A in C, B in T0
        MapPoint *p = W.new_point();
        p->mWorldPos = P;
        p->mNormalVector = Vector3f(0.f, 0.f, 1.f);
        p->mfMaxDistance = 5.0f;
        p->mfMinDistance = 5.0f / W.kfs[0]->mvScaleFactors[kLevels - 1];
        observe(p, W.kfs[j].get(), 0);
        p->mDescriptor.create(1, 32, CV_8U);
        std::memcpy(p->mDescriptor.data, (j == 0 ? carried : in_t0).data(), 32);
    }
}

// ------------------------------------------------------------------ SearchInNeighbors' two phases
struct Outcome {
    std::vector<int> forward;
    int backward = 0;
    long pairs = 0, host_pairs = 0;
    double fwd_ms = 0, bwd_ms = 0, pack_ms = 0, call_ms = 0, replay_ms = 0;
};
enum Mode { REF, DROPIN_BATCH, DROPIN_EACH };

static Outcome search_in_neighbors(World &W, Mode mode) {
    Outcome o;
    KeyFrame *cur = W.kfs[0].get();
    std::vector<KeyFrame *> targets;
    for (size_t k = 1; k < W.kfs.size(); k++) targets.push_back(W.kfs[k].get());
    ORBmatcher matcher;
    const long p0 = gpu::fuse_stats().pairs, h0 = gpu::fuse_stats().host_pairs;
    const std::vector<MapPoint *> matches = cur->GetMapPointMatches();  // :1262
    double t = gpu::fuse_now_ms();
    if (mode == DROPIN_BATCH) {
        o.forward = gpu::FuseAll(targets, matches, 3.0f);
        o.pack_ms = gpu::fuse_stats().pack_ms, o.call_ms = gpu::fuse_stats().call_ms, o.replay_ms = gpu::fuse_stats().replay_ms;
    } else {
        for (size_t k = 0; k < targets.size(); k++)
            o.forward.push_back(mode == REF ? ref_fuse(targets[k], matches, 3.0f) : matcher.Fuse(targets[k], matches));
    }
    o.fwd_ms = gpu::fuse_now_ms() - t;
    std::vector<MapPoint *> cands;  // :1283-1303
    std::vector<uint8_t> taken(W.pts.size(), 0);
    for (size_t k = 0; k < targets.size(); k++) {
        const std::vector<MapPoint *> mps = targets[k]->GetMapPointMatches();
        for (size_t i = 0; i < mps.size(); i++) {
            MapPoint *p = mps[i];
            if (!p || p->isBad() || taken[p->mnId]) continue;
            taken[p->mnId] = 1;
            cands.push_back(p);
        }
    }
    t = gpu::fuse_now_ms();
    o.backward = mode == REF ? ref_fuse(cur, cands, 3.0f) : matcher.Fuse(cur, cands);
    o.bwd_ms = gpu::fuse_now_ms() - t;
    o.pairs = gpu::fuse_stats().pairs - p0;
    o.host_pairs = gpu::fuse_stats().host_pairs - h0;
    return o;
}

static void compare(const char *name, World &A, World &B, const Outcome &a, const Outcome &b) {
    const int before = g_fail;
    CHECK(a.forward == b.forward && a.backward == b.backward, "%s: nFused differ", name);
    for (size_t k = 0; k < A.kfs.size(); k++)
        for (int i = 0; i < A.kfs[k]->N; i++) {
            const MapPoint *x = A.kfs[k]->mvpMapPoints[i], *y = B.kfs[k]->mvpMapPoints[i];
            if ((x ? x->mnId : -1) != (y ? y->mnId : -1)) {
                CHECK(false, "%s: keyframe %zu slot %d: point %ld vs %ld", name, k, i, x ? x->mnId : -1, y ? y->mnId : -1);
                break;
            }
        }
    CHECK(A.pts.size() == B.pts.size(), "%s: point counts", name);
    for (size_t i = 0; i < A.pts.size() && i < B.pts.size(); i++) {
        MapPoint &x = *A.pts[i], &y = *B.pts[i];
        bool same = x.mbBad == y.mbBad && x.nObs == y.nObs && x.mObservations.size() == y.mObservations.size() &&
                    std::memcmp(x.mDescriptor.data, y.mDescriptor.data, 32) == 0 &&
                    (x.mpReplaced ? x.mpReplaced->mnId : -1) == (y.mpReplaced ? y.mpReplaced->mnId : -1);
        MapPoint::Observations_t::iterator ix = x.mObservations.begin(), iy = y.mObservations.begin();
        for (; same && ix != x.mObservations.end(); ++ix, ++iy)
            same = ix->first->mnId == iy->first->mnId && ix->second == iy->second;
        if (!same) {
            CHECK(false, "%s: point %zu differs", name, i);
            break;
        }
    }
    int fused = a.backward, bad = 0;
    for (size_t k = 0; k < a.forward.size(); k++) fused += a.forward[k];
    for (size_t i = 0; i < A.pts.size(); i++) bad += A.pts[i]->mbBad;
    printf("%s: %s, %d fused, %d points replaced, %ld pairs replayed, host pairs %ld\n", name,
           g_fail == before ? "state equal" : "MISMATCH", fused, bad, a.pairs, a.host_pairs);
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char **argv) {
    const bool timing = argc > 1 && !std::strcmp(argv[1], "--time");
    const struct { const char *name; unsigned seed; int n_kf, n_land; Mode mode; } cases[] = {
        {"map-4 batched", 11, 4, 500, DROPIN_BATCH},
        {"map-4 per target", 11, 4, 500, DROPIN_EACH},
        {"map-9 batched", 12, 9, 700, DROPIN_BATCH},
        {"one target", 13, 2, 300, DROPIN_BATCH},
        {"no target", 14, 1, 100, DROPIN_BATCH},
    };
    for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); c++) {
        World A, B;
        build_world(A, cases[c].seed, cases[c].n_kf, cases[c].n_land);
        build_world(B, cases[c].seed, cases[c].n_kf, cases[c].n_land);
        const Outcome a = search_in_neighbors(A, cases[c].mode), b = search_in_neighbors(B, REF);
        compare(cases[c].name, A, B, a, b);
    }
    {
        World A, B, S;
        build_crafted(A);
        build_crafted(B);
        const Outcome a = search_in_neighbors(A, DROPIN_BATCH), b = search_in_neighbors(B, REF);
        compare("crafted replace", A, B, a, b);
        CHECK(a.host_pairs >= 1, "crafted: no pair took the host path");
        CHECK(b.forward.size() == 2 && b.forward[0] == 1 && b.forward[1] == 0, "crafted: the reference fuses in T0 only");
        CHECK(A.pts[1]->mbBad && std::memcmp(A.pts[0]->mDescriptor.data, bits(0, 40).data(), 32) == 0,
              "crafted: B replaced, A's descriptor recomputed");
    }
    if (timing) {
        const int n_targets = 20, reps = 5;
        std::vector<double> df, rf, db, rb, pk, cl, rp;
        long pairs = 0, survivors = 0, host = 0;
        for (int r = 0; r < reps + 1; r++) {  // the first repetition warms up
            World A, B;
            build_world(A, 100 + r, n_targets + 1, 1000);
            build_world(B, 100 + r, n_targets + 1, 1000);
            const Outcome a = search_in_neighbors(A, DROPIN_BATCH);
            g_ref_pairs = g_ref_survivors = 0;
            const Outcome b = search_in_neighbors(B, REF);
            if (r == 0) continue;
            df.push_back(a.fwd_ms), rf.push_back(b.fwd_ms), db.push_back(a.bwd_ms), rb.push_back(b.bwd_ms);
            pk.push_back(a.pack_ms), cl.push_back(a.call_ms), rp.push_back(a.replay_ms);
            pairs = g_ref_pairs, survivors = g_ref_survivors, host = a.host_pairs;
        }
        printf("TIMING fuse_forward_%d dropin_ms %.3f ref_ms %.3f (pack %.3f, call %.3f, replay %.3f)\n", n_targets,
               median(df), median(rf), median(pk), median(cl), median(rp));
        printf("TIMING fuse_backward dropin_ms %.3f ref_ms %.3f\n", median(db), median(rb));
        printf("TIMING fuse pairs (both phases, last map) %ld, survivors of the projection %ld, host pairs %ld\n", pairs,
               survivors, host);
    }
    printf(g_fail ? "%d FAILED\n" : "OK\n", g_fail);
    return g_fail ? 1 : 0;
}
