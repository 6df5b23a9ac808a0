// Test stub of the reference's ORBmatcher.h for Fuse: the constructor and the declaration of Fuse with the
// reference's signature (ORBmatcher.h:166).  Written for the test.
#pragma once
#include "Common.h"
#include "KeyFrame.h"

namespace ygz {
class ORBmatcher {
public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    int Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th = 3.0);

private:
    float mfNNratio;
    bool mbCheckOrientation;
};
}  // namespace ygz
