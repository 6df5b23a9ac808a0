// Tracking_direct_gpu.inc — Tracking::SearchLocalPointsDirect (Tracking.cc:2258-2410)
// with its per-point FindDirectProjection / Align2D loops on the GPU.
// Tracking.cc: include TrackingDirectGPU.h, delete the body of
// SearchLocalPointsDirect and, inside `namespace ygz { ... }`,
// `#include "Tracking_direct_gpu.inc"`.  Tracking.h and every caller
// (TrackLocalMapDirect, Tracking.cc:2201) stay unchanged.
//
// The loops keep the reference's host-side filters and order; the two phases
// each make one GPU call (cache with the 5-px coverage grid replayed on the
// device, then -- only if the cache hit <= mnCacheHitTh points -- the local map).
//
// -DYGZFE_DIRECT_DEVICE_SETUP (opt-in) selects the body that also runs the per-point
// set-up on the device: the host gathers the raw local map (no isInFrustum, no
// SelectNearestKeyframe, no sort) and ygzfe_search_local_map_direct does the rest.  The cull
// then follows the float32 sequence stated in include/ygzfe.h, not Eigen's evaluation order.
#ifdef YGZFE_DIRECT_DEVICE_SETUP
void Tracking::SearchLocalPointsDirect() {
    const int grid_size = 5;   // Tracking.cc:2261
    const float border = 20;   // Tracking.cc:2295-2298
    gpu::DirectMapBatch batch;
    batch.clear();
    std::vector<MapPoint *> points;
    for (MapPoint *mp: mvpDirectMapPointsCache) {  // :2269-2275, the filters on the device
        batch.add_point(mp, mp->isBad(), mpLastKeyFrame, mCurrentFrame);
        points.push_back(mp);
    }
    int cntSuccess = 0;
    if (!points.empty()) {
        const bool ran = batch.run(mCurrentFrame, (int)points.size(), grid_size, mnCacheHitTh, border);
        for (size_t i = 0; i < points.size(); i++) {
            MapPoint *mp = points[i];
            const int st = ran ? batch.status((int)i) : YGZFE_DIRECT_GRID_SKIP;  // a failed call keeps the cache
            if (ran) batch.write_track((int)i, mp, mCurrentFrame);
            if (st == YGZFE_DIRECT_MATCHED) {  // :2300-2326
                mCurrentFrame.mvMatchedFrom.push_back(batch.matched_kf_id((int)i));
                mCurrentFrame.mvKeys.push_back(cv::KeyPoint(cv::Point2f(batch.px((int)i, 0), batch.px((int)i, 1)), 7, -1, 0, 0));
                mCurrentFrame.mvpMapPoints.push_back(mp);
                mCurrentFrame.mvDepth.push_back(-1);
                mCurrentFrame.mvbOutlier.push_back(false);
                cntSuccess++;
            } else if (st == YGZFE_DIRECT_FAILED || st == YGZFE_DIRECT_CULLED) {  // :2271-2275, :2327-2330
                mvpDirectMapPointsCache.erase(mp);
            }
        }
    }

    if (cntSuccess > mnCacheHitTh) {  // :2334-2340
        mCurrentFrame.N = mCurrentFrame.mvKeys.size();
        mCurrentFrame.mvuRight.resize(mCurrentFrame.N, -1);
        return;
    }

    UpdateLocalMap();  // :2344

    batch.clear();
    points.clear();
    for (MapPoint *mp: mvpLocalMapPoints) {  // :2348-2361
        const bool skip = mvpDirectMapPointsCache.find(mp) != mvpDirectMapPointsCache.end() || mp->isBad();
        batch.add_point(mp, skip, mpLastKeyFrame, mCurrentFrame);
        points.push_back(mp);
    }
    if (!points.empty() && batch.run(mCurrentFrame, 0, grid_size, mnCacheHitTh, border)) {
        for (size_t i = 0; i < points.size(); i++) {
            MapPoint *mp = points[i];
            batch.write_track((int)i, mp, mCurrentFrame);
            if (batch.status((int)i) != YGZFE_DIRECT_MATCHED) continue;  // rejected (:2402-2405)
            mCurrentFrame.mvMatchedFrom.push_back(batch.matched_kf_id((int)i));  // :2378-2401
            mCurrentFrame.mvKeys.push_back(cv::KeyPoint(cv::Point2f(batch.px((int)i, 0), batch.px((int)i, 1)), 7, -1, 0, 0));
            mCurrentFrame.mvpMapPoints.push_back(mp);
            mCurrentFrame.mvDepth.push_back(-1);
            mCurrentFrame.mvbOutlier.push_back(false);
            mvpDirectMapPointsCache.insert(mp);
        }
    }

    mCurrentFrame.N = mCurrentFrame.mvKeys.size();  // :2408-2409
    mCurrentFrame.mvuRight.resize(mCurrentFrame.N, -1);
}
#else
void Tracking::SearchLocalPointsDirect() {
    const int grid_size = 5;   // Tracking.cc:2261
    const float border = 20;   // Tracking.cc:2295-2298
    gpu::DirectBatch batch;
    batch.clear();
    std::vector<MapPoint *> points;
    for (auto iter = mvpDirectMapPointsCache.begin(); iter != mvpDirectMapPointsCache.end();) {
        MapPoint *mp = *iter;
        if (mp->isBad() || mCurrentFrame.isInFrustum(mp, 0.5) == false) {  // :2271-2275
            iter = mvpDirectMapPointsCache.erase(iter);
            continue;
        }
        batch.add_point(mp, SelectNearestKeyframe(mp->GetObservations(), 5), mCurrentFrame);
        points.push_back(mp);
        ++iter;
    }
    int cntSuccess = 0;
    if (!points.empty()) {
        const bool ran = batch.run(mCurrentFrame, (int)points.size(), grid_size, mnCacheHitTh, border);
        for (size_t i = 0; i < points.size(); i++) {
            MapPoint *mp = points[i];
            const int st = ran ? batch.status((int)i) : YGZFE_DIRECT_GRID_SKIP;  // a failed call keeps the cache
            if (st == YGZFE_DIRECT_MATCHED) {  // :2300-2326
                mCurrentFrame.mvMatchedFrom.push_back(batch.matched_kf_id((int)i));
                mCurrentFrame.mvKeys.push_back(cv::KeyPoint(cv::Point2f(batch.px((int)i, 0), batch.px((int)i, 1)), 7, -1, 0, 0));
                mCurrentFrame.mvpMapPoints.push_back(mp);
                mCurrentFrame.mvDepth.push_back(-1);
                mCurrentFrame.mvbOutlier.push_back(false);
                cntSuccess++;
            } else if (st == YGZFE_DIRECT_FAILED) {  // :2327-2330
                mvpDirectMapPointsCache.erase(mp);
            }
        }
    }

    if (cntSuccess > mnCacheHitTh) {  // :2334-2340
        mCurrentFrame.N = mCurrentFrame.mvKeys.size();
        mCurrentFrame.mvuRight.resize(mCurrentFrame.N, -1);
        return;
    }

    UpdateLocalMap();  // :2344

    batch.clear();
    points.clear();
    for (MapPoint *mp: mvpLocalMapPoints) {  // :2348-2361
        if (mvpDirectMapPointsCache.find(mp) != mvpDirectMapPointsCache.end())
            continue;
        if (mp->isBad())
            continue;
        if (mCurrentFrame.isInFrustum(mp, 0.5) == false)
            continue;
        batch.add_point(mp, SelectNearestKeyframe(mp->GetObservations(), 5), mCurrentFrame);
        points.push_back(mp);
    }
    if (!points.empty() && batch.run(mCurrentFrame, 0, grid_size, mnCacheHitTh, border)) {
        for (size_t i = 0; i < points.size(); i++) {
            if (batch.status((int)i) != YGZFE_DIRECT_MATCHED) continue;  // rejected (:2402-2405)
            MapPoint *mp = points[i];
            mCurrentFrame.mvMatchedFrom.push_back(batch.matched_kf_id((int)i));  // :2378-2401
            mCurrentFrame.mvKeys.push_back(cv::KeyPoint(cv::Point2f(batch.px((int)i, 0), batch.px((int)i, 1)), 7, -1, 0, 0));
            mCurrentFrame.mvpMapPoints.push_back(mp);
            mCurrentFrame.mvDepth.push_back(-1);
            mCurrentFrame.mvbOutlier.push_back(false);
            mvpDirectMapPointsCache.insert(mp);
        }
    }

    mCurrentFrame.N = mCurrentFrame.mvKeys.size();  // :2408-2409
    mCurrentFrame.mvuRight.resize(mCurrentFrame.N, -1);
}
#endif
