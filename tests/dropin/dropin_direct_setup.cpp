// Tracking::SearchLocalPointsDirect with the per-point set-up on the device
// (compat/dropin/Tracking_direct_gpu.inc built with -DYGZFE_DIRECT_DEVICE_SETUP) over the test
// stubs of Frame / KeyFrame / MapPoint, on a local map of 130 keyframes.
//
// Expected values come from a host loop written here: the cull, the keyframe choice and
// T_ref * P_w in the float32 sequence stated in include/ygzfe.h (this file is compiled with
// -ffp-contract=off), feeding the existing ygzfe_search_local_points_direct.  The appended
// mvKeys / mvpMapPoints / mvMatchedFrom, the resulting cache set and what isInFrustum leaves in
// the MapPoints must be bit-equal.  --time prints the wall time of the default body (host set-up)
// and of the device set-up body on the same case.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "Common.h"
#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "TrackingDirectGPU.h"

#ifndef YGZFE_DIRECT_DEVICE_SETUP
#error "build with -DYGZFE_DIRECT_DEVICE_SETUP"
#endif

namespace ygz {
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
long unsigned int Frame::nNextId = 0;
bool Frame::mbNeedUndistort = false;

struct Tracking {
    ORBextractor *mpORBextractorLeft = nullptr;
    Frame mCurrentFrame;
    std::vector<MapPoint *> mvpLocalMapPoints;
    set<MapPoint *> mvpDirectMapPointsCache;
    int mnCacheHitTh = 150;
    KeyFrame *mpLastKeyFrame = nullptr;
    std::vector<MapPoint *> mvpNextLocalMapPoints;  // what the UpdateLocalMap stub installs
    int nUpdateLocalMap = 0;
    void UpdateLocalMap() {
        mvpLocalMapPoints = mvpNextLocalMapPoints;
        nUpdateLocalMap++;
    }
    void SearchLocalPointsDirect();           // the device set-up body
    void SearchLocalPointsDirectHostSetup();  // the default body, for --time
    vector<std::pair<KeyFrame *, size_t> > SelectNearestKeyframe(const std::map<KeyFrame *, size_t> &observations,
                                                                 int n) {
        vector<std::pair<KeyFrame *, size_t> > s;
        for (auto &o : observations)
            if (!o.first->isBad() && o.first != mpLastKeyFrame) s.push_back(make_pair(o.first, o.second));
        sort(s.begin(), s.end(), [](const pair<KeyFrame *, size_t> &a, const pair<KeyFrame *, size_t> &b) {
            return a.first->mnId > b.first->mnId;
        });
        if ((int)s.size() > n) s.resize(n);
        return s;
    }
    explicit Tracking(int nLevels) { mpORBextractorLeft = new ORBextractor(1000, 2.0f, nLevels, 20, 7); }
    ~Tracking() { delete mpORBextractorLeft; }
};
#include "Tracking_direct_gpu.inc"
// the default body under another name
#pragma push_macro("YGZFE_DIRECT_DEVICE_SETUP")
#undef YGZFE_DIRECT_DEVICE_SETUP
#define SearchLocalPointsDirect SearchLocalPointsDirectHostSetup
#include "Tracking_direct_gpu.inc"
#undef SearchLocalPointsDirect
#pragma pop_macro("YGZFE_DIRECT_DEVICE_SETUP")
}  // namespace ygz

using namespace ygz;

static int fails = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        std::printf(__VA_ARGS__);                       \
        std::printf(" %s\n", (cond) ? "ok" : "FAILED"); \
        if (!(cond)) fails++;                           \
    } while (0)

static cv::Mat synth(int W, int H, unsigned seed, int dx, int dy) {
    cv::Mat img(H, W, CV_8U);
    std::memset(img.data, 128, (size_t)W * H);
    unsigned s = seed;
    auto rnd = [&](int n) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)n); };
    for (int r = 0; r < 900; r++) {
        const int x0 = rnd(W + 40) - 20, y0 = rnd(H + 40) - 20, w = 4 + rnd(40), h = 4 + rnd(40), v = rnd(256);
        for (int y = y0; y < y0 + h; y++)
            for (int x = x0; x < x0 + w; x++) {
                const int xx = x + dx, yy = y + dy;
                if (xx >= 0 && yy >= 0 && xx < W && yy < H) img.data[(size_t)yy * W + xx] = (uint8_t)v;
            }
    }
    for (int i = 0; i < W * H; i++) {
        const int v = img.data[i] + (int)(((uint32_t)(i + seed) * 2654435761u) >> 30) - 1;
        img.data[i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
    return img;
}

// ((R[i][0] * P0 + R[i][1] * P1) + R[i][2] * P2) + t_i
static void rt(const float *R, const float *t, const float *P, float *o) {
    for (int i = 0; i < 3; i++) o[i] = ((R[3 * i] * P[0] + R[3 * i + 1] * P[1]) + R[3 * i + 2] * P[2]) + t[i];
}

struct Track {
    bool in_view = false;
    float x = 0, y = 0, xr = 0, cos = 0;
    bool operator==(const Track &o) const {
        return in_view == o.in_view && (!in_view || (x == o.x && y == o.y && xr == o.xr && cos == o.cos));
    }
};
static Track track_of(const MapPoint &mp) {
    Track t;
    t.in_view = mp.mbTrackInView;
    t.x = mp.mTrackProjX;
    t.y = mp.mTrackProjY;
    t.xr = mp.mTrackProjXR;
    t.cos = mp.mTrackViewCos;
    return t;
}

struct Want {
    std::vector<cv::KeyPoint> keys;
    std::vector<MapPoint *> mps;
    std::vector<int> from;
    std::set<MapPoint *> cache;
    int local_runs = 0, culled = 0;
};

// the stated arithmetic on the host: true when the point is in view, with (u, v, u_r, cos)
static bool in_frustum(const ygzfe_direct_view &V, MapPoint *mp, Track &tr) {
    tr = Track();
    const float P[3] = {mp->mWorldPos[0], mp->mWorldPos[1], mp->mWorldPos[2]};
    float Pc[3];
    rt(V.R, V.t, P, Pc);
    if (Pc[2] < 0.0f) return false;
    const float invz = 1.0f / Pc[2];
    const float u = ((Frame::fx * Pc[0]) * invz) + Frame::cx, v = ((Frame::fy * Pc[1]) * invz) + Frame::cy;
    if (u < V.min_x || u > V.max_x) return false;
    if (v < V.min_y || v > V.max_y) return false;
    const float PO[3] = {P[0] - V.Ow[0], P[1] - V.Ow[1], P[2] - V.Ow[2]};
    const float dist = std::sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]);
    if (dist < 0.8f * mp->mfMinDistance || dist > 1.2f * mp->mfMaxDistance) return false;
    const float cosv = ((PO[0] * mp->mNormalVector[0] + PO[1] * mp->mNormalVector[1]) + PO[2] * mp->mNormalVector[2]) / dist;
    if (cosv < V.view_cos_limit) return false;
    if (!std::isfinite(u) || !std::isfinite(v) || !std::isfinite(dist) || !std::isfinite(cosv)) return false;
    tr.in_view = true;
    tr.x = u;
    tr.y = v;
    tr.xr = u - V.mbf * invz;
    tr.cos = cosv;
    return true;
}

int main(int argc, char **argv) {
    const bool timing = argc > 1 && std::strcmp(argv[1], "--time") == 0;
    const int W = 752, H = 480, nl = 4, NK = 130;
    Frame::fx = 458.654f;
    Frame::fy = 457.296f;
    Frame::cx = 367.215f;
    Frame::cy = 248.375f;
    Frame::invfx = 1.f / Frame::fx;
    Frame::invfy = 1.f / Frame::fy;
    const float Z = 3.0f;
    Tracking T(nl);
    const cv::Mat im0 = synth(W, H, 7u, 0, 0), im1 = synth(W, H, 7u, 2, -1);
    Frame last(im0, T.mpORBextractorLeft);
    last.ExtractFeatures();

    // the local map of tests/dropin/dropin_calls.cpp's 130-keyframe case: shifted images of the
    // plane (image shift (dx, dy) <=> T_cw translation (dx Z / fx, dy Z / fy, 0)), kfs[2] the last
    // keyframe, one keyframe bad; plus points that the distance, viewing-angle and depth rules cull
    std::vector<KeyFrame> kfs(NK);
    std::vector<Frame> kframes;
    kframes.reserve(NK);
    auto shift = [](int k, int c) {
        static const int s3[3][2] = {{0, 0}, {-1, 1}, {3, 2}};
        return k < 3 ? s3[k][c] : (c == 0 ? (k * 5) % 9 - 4 : (k * 3) % 7 - 3);
    };
    for (int k = 0; k < NK; k++) {
        cv::Mat kim = k == 0 ? im0 : synth(W, H, 7u, shift(k, 0), shift(k, 1));
        if (k >= 3) kim.data[k] ^= 0x5A;  // every keyframe's pyramid distinct
        kframes.push_back(Frame(kim, T.mpORBextractorLeft));
        kfs[k].mvImagePyramid = kframes[k].mvImagePyramid;
        kfs[k].mvScaleFactors = kframes[k].mvScaleFactors;
        kfs[k].mTcw = SE3f(Eigen::Quaternionf(), Vector3f(shift(k, 0) * Z / Frame::fx, shift(k, 1) * Z / Frame::fy, 0.f));
        kfs[k].mnId = 10 + (k * 37) % NK;  // not monotone in the table order
    }
    T.mpLastKeyFrame = &kfs[2];
    kfs[40].mbBad = true;
    std::vector<MapPoint> dm;
    dm.reserve(2 * last.N);
    for (int i = 0; i < last.N; i++)
        for (int c = 0; c < 1 + (i % 3 == 0); c++) {
            const cv::KeyPoint &kp = last.mvKeys[i];
            MapPoint mp;
            const float u = kp.pt.x + 0.6f * c, v = kp.pt.y - 0.4f * c;
            mp.mWorldPos = Vector3f((u - Frame::cx) / Frame::fx * Z, (v - Frame::cy) / Frame::fy * Z, Z);
            const size_t j = dm.size();
            mp.mbBad = (j % 23) == 11;
            mp.mfMinDistance = 1.0f;
            mp.mfMaxDistance = (j % 17) == 3 ? 2.0f : 6.0f;      // 1.2 * 2 < dist: too far
            if (j % 31 == 9) mp.mfMinDistance = 5.0f;            // 0.8 * 5 > dist: too near
            if (j % 19 == 5) mp.mNormalVector = Vector3f(1.f, 0.f, 0.f);  // viewing cosine < 0.5
            if (j % 29 == 7) mp.mWorldPos[2] = -Z;               // behind the camera
            dm.push_back(mp);
        }
    for (size_t j = 0; j < dm.size(); j++) {
        MapPoint &mp = dm[j];
        const int oc = (int)(j % 3);
        for (int k = 0; k < NK; k++) {
            if (k == 0 && j % 5 == 1) continue;
            if (k == 1 && j % 4 == 2) continue;
            if (k >= 3 && (j / 2 + 7 * (size_t)k) % 26 != 0) continue;
            const Vector3f pc = kfs[k].mTcw * mp.mWorldPos;
            cv::KeyPoint kp(cv::Point2f(Frame::fx * pc[0] / pc[2] + Frame::cx, Frame::fy * pc[1] / pc[2] + Frame::cy),
                            31.f * kfs[k].mvScaleFactors[oc], -1, 0, oc);
            mp.mObservations[&kfs[k]] = kfs[k].mvKeys.size();
            kfs[k].mvKeys.push_back(kp);
        }
    }
    // the frame being tracked: the plane shifted by (2, -1) px and turned by 2 mrad about the axis
    T.mCurrentFrame = Frame(im1, T.mpORBextractorLeft);
    T.mCurrentFrame.mbf = 40.f;
    T.mCurrentFrame.SetPose(SE3f(Eigen::Quaternionf(std::cos(0.001f), 0.f, 0.f, std::sin(0.001f)),
                                 Vector3f(2 * Z / Frame::fx, -1 * Z / Frame::fy, 0.f)));
    Frame &C = T.mCurrentFrame;
    dropin::PyramidPool &pool = dropin::PyramidPool::instance();

    // one phase of the host loop: the stated set-up, then the existing call
    auto host_phase = [&](const std::vector<MapPoint *> &pts, int n_cache, int th, std::vector<int> &status, Want &w,
                          std::vector<Track> &tracks) {
        ygzfe_direct_view V;
        gpu::DirectMapBatch::fill_view(C, V);
        std::vector<int32_t> ip(1, 0), ri;
        std::vector<ygzfe_kp> kp;
        std::vector<float> pt, proj;
        std::vector<ygzfe_se3> tcr;
        std::vector<long> ids;
        std::vector<const ygzfe_frame *> refs;
        std::map<KeyFrame *, int> slot;
        for (size_t i = 0; i < pts.size(); i++) {
            proj.push_back(tracks[i].x);
            proj.push_back(tracks[i].y);
            for (auto &ob : T.SelectNearestKeyframe(pts[i]->GetObservations(), 5)) {
                KeyFrame *kf = ob.first;
                if (!slot.count(kf)) {
                    ygzfe_frame *f = pool.find_or_upload(kf->mvImagePyramid);
                    if (!f) return -1;
                    pool.pin(f, 1);
                    slot[kf] = (int)refs.size();
                    refs.push_back(f);
                }
                const SE3f pose = kf->GetPose();
                const Eigen::Matrix3f R = pose.rotationMatrix();
                const float tt[3] = {pose.translation()[0], pose.translation()[1], pose.translation()[2]};
                const float P[3] = {pts[i]->mWorldPos[0], pts[i]->mWorldPos[1], pts[i]->mWorldPos[2]};
                float p[3];
                rt(R.m, tt, P, p);
                ri.push_back(slot[kf]);
                kp.push_back(*dropin::as_kp(&kf->mvKeys[ob.second]));
                for (int q = 0; q < 3; q++) pt.push_back(p[q]);
                tcr.push_back(gpu::to_se3(C.mTcw * pose.inverse()));
                ids.push_back((long)kf->mnId);
            }
            ip.push_back((int32_t)ri.size());
        }
        const int n = (int)pts.size();
        std::vector<float> px(2 * n + 2);
        std::vector<int32_t> m(n + 1), st(n + 1);
        int cs = 0, ran = 0;
        ygzfe_frame *cf = pool.find_or_upload(C.mvImagePyramid);
        const ygzfe_camera cam{Frame::fx, Frame::fy, Frame::cx, Frame::cy};
        const int rc = cf ? ygzfe_search_local_points_direct(refs.data(), (int)refs.size(), cf, &cam, n_cache, n - n_cache,
                                                             ip.data(), ri.data(), kp.data(), pt.data(), tcr.data(),
                                                             proj.data(), 20.f, 5, th, px.data(), m.data(), st.data(),
                                                             &cs, &ran)
                          : -1;
        for (const ygzfe_frame *f : refs) pool.pin(f, -1);
        if (rc != YGZFE_OK) return -1;
        status.assign(st.begin(), st.end());
        for (int i = 0; i < n; i++)
            if (st[i] == YGZFE_DIRECT_MATCHED) {
                w.keys.push_back(cv::KeyPoint(cv::Point2f(px[2 * i], px[2 * i + 1]), 7, -1, 0, 0));
                w.mps.push_back(pts[i]);
                w.from.push_back((int)ids[m[i]]);
            }
        return cs;
    };
    // Tracking.cc:2258-2410 over the host loop; expect[mp] = what isInFrustum leaves in the MapPoint
    auto expected = [&](const std::set<MapPoint *> &cache0, const std::vector<MapPoint *> &local, int th,
                        std::map<MapPoint *, Track> &expect) {
        ygzfe_direct_view V;
        gpu::DirectMapBatch::fill_view(C, V);
        Want w;
        w.cache = cache0;
        std::vector<MapPoint *> pts;
        std::vector<Track> tracks;
        for (auto it = w.cache.begin(); it != w.cache.end();) {
            Track tr;
            const bool bad = (*it)->isBad();
            const bool in = !bad && in_frustum(V, *it, tr);
            if (!bad) expect[*it] = tr;
            if (!in) { it = w.cache.erase(it); w.culled++; continue; }
            pts.push_back(*it);
            tracks.push_back(tr);
            ++it;
        }
        std::vector<int> st;
        const int cnt = host_phase(pts, (int)pts.size(), th, st, w, tracks);
        if (cnt < 0) { w.local_runs = -1; return w; }
        for (size_t i = 0; i < pts.size(); i++)
            if (st[i] == YGZFE_DIRECT_FAILED) w.cache.erase(pts[i]);
        if (cnt > th) return w;
        w.local_runs = 1;
        pts.clear();
        tracks.clear();
        for (MapPoint *mp : local) {
            if (w.cache.count(mp) || mp->isBad()) continue;
            Track tr;
            const bool in = in_frustum(V, mp, tr);
            expect[mp] = tr;
            if (!in) { w.culled++; continue; }
            pts.push_back(mp);
            tracks.push_back(tr);
        }
        const size_t before = w.mps.size();
        if (host_phase(pts, 0, th, st, w, tracks) < 0) { w.local_runs = -1; return w; }
        for (size_t i = before; i < w.mps.size(); i++) w.cache.insert(w.mps[i]);
        return w;
    };

    std::set<MapPoint *> cache0;
    std::vector<MapPoint *> local;
    for (size_t j = 0; j < dm.size(); j++) {
        if (j % 2 == 0) cache0.insert(&dm[j]);
        local.push_back(&dm[j]);
    }
    auto reset = [&](int th) {
        C.mvKeys.clear();
        C.mvpMapPoints.clear();
        C.mvDepth.clear();
        C.mvbOutlier.clear();
        C.mvMatchedFrom.clear();
        C.N = 0;
        T.mvpDirectMapPointsCache = cache0;
        T.mvpLocalMapPoints.clear();
        T.mvpNextLocalMapPoints = local;
        T.mnCacheHitTh = th;
        T.nUpdateLocalMap = 0;
    };
    for (int th : {1 << 30, 150}) {
        std::map<MapPoint *, Track> expect;
        const Want w = expected(cache0, local, th, expect);
        for (MapPoint &mp : dm) {  // stale values that the call must overwrite or leave
            mp.mbTrackInView = true;
            mp.mTrackProjX = mp.mTrackProjY = mp.mTrackProjXR = mp.mTrackViewCos = -7.f;
        }
        reset(th);
        T.SearchLocalPointsDirect();
        bool same = w.local_runs >= 0 && (size_t)C.N == w.keys.size() && C.mvKeys.size() == w.keys.size() &&
                    C.mvpMapPoints == w.mps && C.mvMatchedFrom == w.from && T.mvpDirectMapPointsCache == w.cache &&
                    T.nUpdateLocalMap == w.local_runs && (int)C.mvuRight.size() == C.N &&
                    C.mvDepth.size() == w.keys.size();
        for (size_t i = 0; same && i < w.keys.size(); i++)
            same = C.mvKeys[i].pt.x == w.keys[i].pt.x && C.mvKeys[i].pt.y == w.keys[i].pt.y &&
                   C.mvKeys[i].size == 7.f && C.mvKeys[i].angle == -1.f;
        CHECK(same && w.keys.size() > 100 && w.culled > 30,
              "SearchLocalPointsDirect() device set-up [%d keyframes, mnCacheHitTh %d]: %zu points tracked (host loop "
              "%zu), %d culled, local map %s, cache %zu -> %zu", NK, th, C.mvKeys.size(), w.keys.size(), w.culled,
              w.local_runs ? "searched" : "skipped", cache0.size(), T.mvpDirectMapPointsCache.size());
        int tested = 0, in_view = 0, bad = 0;
        for (MapPoint &mp : dm) {
            auto it = expect.find(&mp);
            if (it == expect.end()) {  // never reached isInFrustum: untouched
                if (!(mp.mbTrackInView && mp.mTrackProjX == -7.f)) bad++;
                continue;
            }
            tested++;
            in_view += it->second.in_view;
            if (!(track_of(mp) == it->second)) bad++;
        }
        CHECK(bad == 0 && in_view > 100 && tested > in_view,
              "  mbTrackInView / mTrackProjX / mTrackProjY / mTrackProjXR / mTrackViewCos of %d points (%d in view) "
              "bit-equal, the others untouched", tested, in_view);
    }

    if (timing) {
        // the same case through both bodies, alternating, after a warm-up (pool, staging, keypoints)
        auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        std::vector<double> th_, td_;
        gpu::DirectStats sh, sd;  // means: pyramid-pool lookups / uploads, the C-ABI call
        for (int r = 0; r < 35; r++) {
            if (r == 5) sh = sd = gpu::DirectStats();
            reset(150);
            gpu::direct_stats() = sh;
            auto t0 = std::chrono::steady_clock::now();
            T.SearchLocalPointsDirectHostSetup();
            const double a = gpu::ms_since(t0);
            sh = gpu::direct_stats();
            reset(150);
            gpu::direct_stats() = sd;
            t0 = std::chrono::steady_clock::now();
            T.SearchLocalPointsDirect();
            const double b = gpu::ms_since(t0);
            sd = gpu::direct_stats();
            if (r >= 5) {
                th_.push_back(a);
                td_.push_back(b);
            }
        }
        std::printf("TIMING search_local_points_direct_130kf host_setup_ms %.4f device_setup_ms %.4f points %zu "
                    "(medians of 30 alternating runs)\n", median(th_), median(td_), local.size() + cache0.size());
        std::printf("TIMING   host_setup: pool_ms %.4f c_abi_ms %.4f | device_setup: pool_ms %.4f c_abi_ms %.4f "
                    "(means; pool = pyramid lookups and uploads, device set-up: keypoint uploads not included)\n",
                    sh.pool_ms / 30, sh.call_ms / 30, sd.pool_ms / 30, sd.call_ms / 30);
    }
    if (fails) std::printf("%d FAILED\n", fails);
    else std::printf("OK\n");
    return fails ? 1 : 0;
}
