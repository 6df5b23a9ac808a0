// Test stub of the reference's ORBmatcher.h for the mapping-side search: the constructor, the members and the
// declaration of SearchForTriangulation with the reference's signature (ORBmatcher.h:146-150).  Written for the test.
#pragma once
#include "Common.h"
#include "KeyFrame.h"

namespace ygz {
class ORBmatcher {
public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, Matrix3f &F12,
                               std::vector<std::pair<size_t, size_t> > &vMatchedPairs, const bool bOnlyStereo);

private:
    float mfNNratio;
    bool mbCheckOrientation;
};
}  // namespace ygz
