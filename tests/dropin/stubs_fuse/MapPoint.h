// Test stub of the reference's MapPoint for ORBmatcher::Fuse: the members Fuse (ORBmatcher.cc:748-886) reads and
// the map surgery it calls (AddObservation, Replace with ComputeDistinctiveDescriptors).  Written for the test; it
// comes before tests/dropin/stubs on the include path.  The member functions that need KeyFrame are defined at the
// end of this directory's KeyFrame.h.
#pragma once
#include "Common.h"

namespace ygz {
class KeyFrame;
struct KeyFrameById {  // observations in keyframe-id order, so two copies of a map behave alike
    bool operator()(const KeyFrame *a, const KeyFrame *b) const;
};
class MapPoint {
public:
    typedef std::map<KeyFrame *, size_t, KeyFrameById> Observations_t;
    long mnId = 0;
    Vector3f mWorldPos;
    Vector3f mNormalVector{0.f, 0.f, 1.f};
    cv::Mat mDescriptor;
    float mfMaxDistance = 0.f, mfMinDistance = 0.f;
    bool mbBad = false;
    int nObs = 0, mnVisible = 1, mnFound = 1;
    MapPoint *mpReplaced = nullptr;
    Observations_t mObservations;

    Vector3f GetWorldPos() { return mWorldPos; }
    Vector3f GetNormal() { return mNormalVector; }
    bool isBad() { return mbBad; }
    int Observations() { return nObs; }
    Observations_t GetObservations() { return mObservations; }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistance() { return mfMaxDistance; }  // the raw values (the drop-in's two accessors)
    float GetMinDistance() { return mfMinDistance; }
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    void IncreaseFound(int n = 1) { mnFound += n; }
    int PredictScale(const float &currentDist, KeyFrame *pKF);
    void AddObservation(KeyFrame *pKF, size_t idx);
    void Replace(MapPoint *pMP);
    void ComputeDistinctiveDescriptors();
};
}  // namespace ygz
