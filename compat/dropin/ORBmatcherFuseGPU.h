// ORBmatcherFuseGPU.h — ORBmatcher::Fuse (the projection search of LocalMapping::SearchInNeighbors) on the GPU,
// read through the reference's own KeyFrame / MapPoint members.
//
//   Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th)      ORBmatcher.cc:748-886
//
// ORBmatcher.cc includes ORBmatcher_fuse_gpu.inc in place of that body, so SearchInNeighbors
// (LocalMapping.cc:1228-1326) compiles and runs unchanged: one device call per target keyframe, and the backward
// phase is that call.  gpu::FuseAll searches every target of the forward phase in ONE call
// (ygzfe_fuse_search_batch) and then replays the targets in order.
//
// The split.  The search of a (keyframe, point) pair (:764-866) reads the keyframe and the point only; all pairs go
// to the device at once.  What follows it (:868-882: Replace, AddObservation, AddMapPoint) is sequential and stays
// here: the pairs are replayed keyframe by keyframe and point by point, `!pMP`, isBad() and IsInKeyFrame(pKF)
// checked live, then :868-882 applied with the device's bestIdx / bestDist.
//
// Stale descriptors.  MapPoint::Replace ends with ComputeDistinctiveDescriptors() on the surviving point
// (MapPoint.cc:185), so a point that survives a Replace in one target may carry another descriptor into the next.
// The replay compares pMP->GetDescriptor() with the 32 bytes it uploaded; where they differ (or where the pair was
// not searched because the point was in the keyframe when the call was packed) it searches that one pair here, with
// the scalar loop below.  Nothing else a pair reads changes during Fuse (positions, normals, distance ranges and
// the keyframes' keypoints stay), so the result equals the reference's whatever the batching.
//
// MapPoint needs two one-line accessors for the raw distance range, `float GetMinDistance()` and
// `float GetMaxDistance()` (mfMinDistance / mfMaxDistance are private, and the invariance getters scale them).
#ifndef YGZFE_ORBMATCHER_FUSE_GPU_H_
#define YGZFE_ORBMATCHER_FUSE_GPU_H_

#include <chrono>
#include <cstring>
#include <vector>

#include "ORBmatcherGPU.h"

namespace ygz {
namespace gpu {

// the views of one mapping thread's Fuse calls: view k holds target k
inline MatchView &fuse_view(size_t slot) {
    static thread_local std::vector<MatchView *> v;  // kept for the thread's lifetime
    while (v.size() <= slot) v.push_back(new MatchView((int)v.size()));
    return *v[slot];
}

// pairs replayed, and those searched on the host (stale descriptor), since the thread started
struct FuseStats {
    long pairs = 0, host_pairs = 0;
    double pack_ms = 0, call_ms = 0, replay_ms = 0;  // of the last FuseAll
};
inline FuseStats &fuse_stats() {
    static thread_local FuseStats s;
    return s;
}

inline double fuse_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline int fuse_distance(const uint8_t *a, const uint8_t *b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// :764-866 for one pair with the point's current descriptor: the drop-in's own scalar loop
template <class KeyFrameT, class MapPointT>
inline void fuse_search_host(KeyFrameT *pKF, MapPointT *pMP, const float th, int &bestIdx, int &bestDist) {
    bestIdx = -1;
    bestDist = 256;
    const Matrix3f Rcw = pKF->GetRotation();
    const Vector3f tcw = pKF->GetTranslation(), Ow = pKF->GetCameraCenter();
    const Vector3f p3Dw = pMP->GetWorldPos();
    const Vector3f p3Dc = Rcw * p3Dw + tcw;
    if (p3Dc[2] < 0.0f) return;
    const float invz = 1 / p3Dc[2];
    const float x = p3Dc[0] * invz, y = p3Dc[1] * invz;
    const float u = pKF->fx * x + pKF->cx, v = pKF->fy * y + pKF->cy;
    if (!pKF->IsInImage(u, v)) return;
    const float ur = u - pKF->mbf * invz;
    const Vector3f PO = p3Dw - Ow;
    const float dist3D = PO.norm();
    if (dist3D < pMP->GetMinDistanceInvariance() || dist3D > pMP->GetMaxDistanceInvariance()) return;
    const Vector3f Pn = pMP->GetNormal();
    if (((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2]) < 0.5f * dist3D) return;
    const float ratio = pMP->GetMaxDistance() / dist3D;
    if (!(dist3D > 0.0f && std::isfinite(dist3D) && ratio > 0.0f && std::isfinite(ratio))) return;  // as the device
    const int level = pMP->PredictScale(dist3D, pKF);
    const float radius = th * pKF->mvScaleFactors[level];
    const std::vector<size_t> vIndices = pKF->GetFeaturesInArea(u, v, radius);
    const cv::Mat dMP = pMP->GetDescriptor();
    for (size_t k = 0; k < vIndices.size(); k++) {
        const size_t idx = vIndices[k];
        const cv::KeyPoint &kp = pKF->mvKeys[idx];
        if (kp.octave < level - 1 || kp.octave > level) continue;
        const float ex = u - kp.pt.x, ey = v - kp.pt.y;
        if (pKF->mvuRight[idx] >= 0) {
            const float er = ur - pKF->mvuRight[idx];
            const float e2 = (ex * ex + ey * ey) + er * er;
            if (e2 * pKF->mvInvLevelSigma2[kp.octave] > 7.8) continue;
        } else {
            const float e2 = ex * ex + ey * ey;
            if (e2 * pKF->mvInvLevelSigma2[kp.octave] > 5.99) continue;
        }
        const int dist = fuse_distance(dMP.ptr<uint8_t>(0), pKF->mDescriptors.template ptr<uint8_t>((int)idx));
        if (dist < bestDist) {
            bestDist = dist;
            bestIdx = (int)idx;
        }
    }
    if (bestDist > kTH_LOW) bestIdx = -1;
}

// :868-882 with the pair's search result
template <class KeyFrameT, class MapPointT>
inline int fuse_apply(KeyFrameT *pKF, MapPointT *pMP, int bestIdx, int bestDist) {
    if (bestDist > kTH_LOW || bestIdx < 0) return 0;
    MapPointT *pMPinKF = pKF->GetMapPoint(bestIdx);
    if (pMPinKF) {
        if (!pMPinKF->isBad()) {
            if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
            else pMPinKF->Replace(pMP);
        }
    } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
    }
    return 1;
}

// Fuse(vpTargetKFs[k], vpMapPoints, th) for every k in order, the searches in one device call.  Returns the nFused
// of each target.  The level tables are those of the first target: the keyframes of a map share the extractor.
template <class KeyFrameT, class MapPointT>
std::vector<int> FuseAll(const std::vector<KeyFrameT *> &vpTargetKFs, const std::vector<MapPointT *> &vpMapPoints,
                         const float th = 3.0f) {
    const int nkf = (int)vpTargetKFs.size(), nall = (int)vpMapPoints.size();
    std::vector<int> nFused(nkf, 0);
    FuseStats &S = fuse_stats();
    if (nkf == 0) return nFused;
    const double t0 = fuse_now_ms();
    // the points that can take part: present and not bad now (a bad point stays bad)
    std::vector<int> slot(nall, -1);
    std::vector<float> world, normal, mind, maxd;
    std::vector<uint8_t> desc;
    int npts = 0;
    for (int i = 0; i < nall; i++) {
        MapPointT *pMP = vpMapPoints[i];
        if (!pMP || pMP->isBad()) continue;
        slot[i] = npts++;
        const Vector3f P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
        for (int c = 0; c < 3; c++) world.push_back(P[c]), normal.push_back(Pn[c]);
        mind.push_back(pMP->GetMinDistance());
        maxd.push_back(pMP->GetMaxDistance());
        const cv::Mat d = pMP->GetDescriptor();
        desc.insert(desc.end(), d.ptr<uint8_t>(0), d.ptr<uint8_t>(0) + 32);
    }
    std::vector<ygzfe_match_frame *> frames(nkf);
    std::vector<float> view(20 * (size_t)nkf);
    std::vector<uint8_t> skip((size_t)nkf * npts + 1, 0);
    bool ok = true;
    for (int k = 0; k < nkf && ok; k++) {
        KeyFrameT *pKF = vpTargetKFs[k];
        const ygzfe_bounds b = {pKF->mnMinX, pKF->mnMaxX, pKF->mnMinY, pKF->mnMaxY};
        ok = fuse_view(k).set(pKF->mvKeys, pKF->mDescriptors, pKF->N,
                              (int)pKF->mvuRight.size() >= pKF->N && pKF->N > 0 ? pKF->mvuRight.data() : nullptr, b);
        frames[k] = fuse_view(k).get();
        const Matrix3f R = pKF->GetRotation();
        const Vector3f t = pKF->GetTranslation(), Ow = pKF->GetCameraCenter();
        float *w = &view[20 * (size_t)k];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) w[3 * r + c] = R(r, c);
        for (int c = 0; c < 3; c++) w[9 + c] = t[c], w[12 + c] = Ow[c];
        w[15] = pKF->fx, w[16] = pKF->fy, w[17] = pKF->cx, w[18] = pKF->cy, w[19] = pKF->mbf;
        for (int i = 0; i < nall; i++)
            if (slot[i] >= 0 && vpMapPoints[i]->IsInKeyFrame(pKF)) skip[(size_t)k * npts + slot[i]] = 1;
    }
    std::vector<int32_t> bi((size_t)nkf * npts + 1, -1), bd((size_t)nkf * npts + 1, 256);
    const double t1 = fuse_now_ms();
    KeyFrameT *pKF0 = vpTargetKFs[0];
    if (!ok || ygzfe_fuse_search_batch(nkf, frames.data(), view.data(), npts, world.data(), normal.data(), mind.data(),
                                       maxd.data(), desc.data(), skip.data(), th, pKF0->mvScaleFactors.data(),
                                       pKF0->mvInvLevelSigma2.data(), pKF0->mnScaleLevels, pKF0->mfLogScaleFactor, 1,
                                       bi.data(), bd.data()) != YGZFE_OK) {
        failed("Fuse");
        return nFused;
    }
    const double t2 = fuse_now_ms();
    for (int k = 0; k < nkf; k++) {  // the reference's order: keyframe by keyframe, point by point
        KeyFrameT *pKF = vpTargetKFs[k];
        for (int i = 0; i < nall; i++) {
            MapPointT *pMP = vpMapPoints[i];
            if (!pMP) continue;                                   // :767
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;  // :770, live
            const size_t p = (size_t)k * npts + slot[i];
            int bestIdx = bi[p], bestDist = bd[p];
            S.pairs++;
            const cv::Mat d = pMP->GetDescriptor();
            if (skip[p] || std::memcmp(d.ptr<uint8_t>(0), &desc[32 * (size_t)slot[i]], 32) != 0) {
                fuse_search_host(pKF, pMP, th, bestIdx, bestDist);  // the descriptor changed since the upload
                S.host_pairs++;
            }
            nFused[k] += fuse_apply(pKF, pMP, bestIdx, bestDist);
        }
    }
    const double t3 = fuse_now_ms();
    S.pack_ms = t1 - t0;
    S.call_ms = t2 - t1;
    S.replay_ms = t3 - t2;
    return nFused;
}

// the reference's signature: one keyframe (also the backward phase of SearchInNeighbors)
template <class KeyFrameT, class MapPointT>
int Fuse(KeyFrameT *pKF, const std::vector<MapPointT *> &vpMapPoints, const float th) {
    return FuseAll(std::vector<KeyFrameT *>(1, pKF), vpMapPoints, th)[0];
}

}  // namespace gpu
}  // namespace ygz

#endif
