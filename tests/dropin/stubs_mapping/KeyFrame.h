// Test stub of the reference's KeyFrame for the mapping-side search: the members
// ORBmatcher::SearchForTriangulation (ORBmatcher.cc:597-746) reads.  Written for the test; it comes before
// tests/dropin/stubs on the include path, whose KeyFrame stub serves the tracking-side programs.
#pragma once
#include "Common.h"
#include "MapPoint.h"

namespace ygz {
class KeyFrame {
public:
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys;
    std::vector<float> mvuRight;  // negative: monocular keypoint
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<float> mvScaleFactors, mvLevelSigma2;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
    SE3f mTcw;
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    Matrix3f GetRotation() { return mTcw.rotationMatrix(); }
    Vector3f GetTranslation() { return mTcw.translation(); }
    Vector3f GetCameraCenter() { return mTcw.inverse().translation(); }
};
}  // namespace ygz
