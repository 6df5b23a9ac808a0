// Test stub of the reference's KeyFrame for ORBmatcher::Fuse: the members Fuse (ORBmatcher.cc:748-886) reads, the
// grid with GetFeaturesInArea / IsInImage, and the map-point slots MapPoint::Replace edits.  Written for the test.
#pragma once
#include <algorithm>

#include "Common.h"
#include "MapPoint.h"

namespace ygz {
class KeyFrame {
public:
    static const int kCols = 64, kRows = 48;
    long mnId = 0;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys;
    std::vector<float> mvuRight;  // negative: monocular keypoint
    cv::Mat mDescriptors;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2;
    float mfLogScaleFactor = 0.f;
    int mnScaleLevels = 0;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f, mbf = 0.f;
    float mnMinX = 0.f, mnMaxX = 0.f, mnMinY = 0.f, mnMaxY = 0.f;
    float mfGridElementWidthInv = 0.f, mfGridElementHeightInv = 0.f;
    std::vector<std::vector<std::vector<size_t> > > mGrid;
    SE3f mTcw;

    Matrix3f GetRotation() { return mTcw.rotationMatrix(); }
    Vector3f GetTranslation() { return mTcw.translation(); }
    Vector3f GetCameraCenter() { return mTcw.inverse().translation(); }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = nullptr; }
    bool IsInImage(const float &x, const float &y) const { return x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY; }

    // the grid of the frame the keyframe was made from: cell = round((x - min) * inv), outside: no cell
    void AssignFeaturesToGrid() {
        mfGridElementWidthInv = (float)kCols / (mnMaxX - mnMinX);
        mfGridElementHeightInv = (float)kRows / (mnMaxY - mnMinY);
        mGrid.assign(kCols, std::vector<std::vector<size_t> >(kRows));
        for (int i = 0; i < N; i++) {
            const int px = (int)std::round((mvKeys[i].pt.x - mnMinX) * mfGridElementWidthInv);
            const int py = (int)std::round((mvKeys[i].pt.y - mnMinY) * mfGridElementHeightInv);
            if (px < 0 || px >= kCols || py < 0 || py >= kRows) continue;
            mGrid[px][py].push_back((size_t)i);
        }
    }

    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const {
        std::vector<size_t> out;
        const int x0 = std::max(0, (int)std::floor((x - mnMinX - r) * mfGridElementWidthInv));
        const int x1 = std::min(kCols - 1, (int)std::ceil((x - mnMinX + r) * mfGridElementWidthInv));
        const int y0 = std::max(0, (int)std::floor((y - mnMinY - r) * mfGridElementHeightInv));
        const int y1 = std::min(kRows - 1, (int)std::ceil((y - mnMinY + r) * mfGridElementHeightInv));
        if (x0 >= kCols || x1 < 0 || y0 >= kRows || y1 < 0) return out;
        for (int ix = x0; ix <= x1; ix++)
            for (int iy = y0; iy <= y1; iy++)
                for (size_t j = 0; j < mGrid[ix][iy].size(); j++) {
                    const cv::KeyPoint &kp = mvKeys[mGrid[ix][iy][j]];
                    if (std::fabs(kp.pt.x - x) < r && std::fabs(kp.pt.y - y) < r) out.push_back(mGrid[ix][iy][j]);
                }
        return out;
    }
};

inline bool KeyFrameById::operator()(const KeyFrame *a, const KeyFrame *b) const { return a->mnId < b->mnId; }

inline int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF) {
    const float ratio = mfMaxDistance / currentDist;
    int nScale = (int)std::ceil(std::log(ratio) / pKF->mfLogScaleFactor);  // float log, float divide
    if (nScale < 0) nScale = 0;
    else if (nScale >= pKF->mnScaleLevels) nScale = pKF->mnScaleLevels - 1;
    return nScale;
}

inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx) {
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs += pKF->mvuRight[idx] >= 0 ? 2 : 1;
}

// the descriptor, among those of the observing keypoints, with the least median distance to the others
inline void MapPoint::ComputeDistinctiveDescriptors() {
    if (mbBad || mObservations.empty()) return;
    std::vector<const uint8_t *> d;
    for (Observations_t::iterator it = mObservations.begin(); it != mObservations.end(); ++it)
        d.push_back(it->first->mDescriptors.ptr<uint8_t>((int)it->second));
    const size_t n = d.size();
    int best_median = 1 << 30;
    size_t best = 0;
    for (size_t i = 0; i < n; i++) {
        std::vector<int> dist(n);
        for (size_t j = 0; j < n; j++) {
            int s = 0;
            for (int b = 0; b < 32; b++) s += __builtin_popcount((unsigned)(d[i][b] ^ d[j][b]));
            dist[j] = s;
        }
        std::sort(dist.begin(), dist.end());
        const int median = dist[(n - 1) / 2];
        if (median < best_median) best_median = median, best = i;
    }
    cv::Mat m(1, 32, CV_8U);
    std::memcpy(m.data, d[best], 32);
    mDescriptor = m;
}

inline void MapPoint::Replace(MapPoint *pMP) {
    if (pMP->mnId == mnId) return;
    const Observations_t obs = mObservations;
    mObservations.clear();
    mbBad = true;
    mpReplaced = pMP;
    for (Observations_t::const_iterator it = obs.begin(); it != obs.end(); ++it) {
        KeyFrame *pKF = it->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(it->second, pMP);
            pMP->AddObservation(pKF, it->second);
        } else {
            pKF->EraseMapPointMatch(it->second);
        }
    }
    pMP->IncreaseFound(mnFound);
    pMP->IncreaseVisible(mnVisible);
    pMP->ComputeDistinctiveDescriptors();
}
}  // namespace ygz
