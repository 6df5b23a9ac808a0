// ORBmatcher_mapping_gpu.inc — ORBmatcher::SearchForTriangulation on the GPU.
// ORBmatcher.cc: delete the body of this member function and, inside `namespace ygz { ... }`,
// `#include "ORBmatcher_mapping_gpu.inc"` (after including ORBmatcherMappingGPU.h).  ORBmatcher.h
// and LocalMapping.cc stay unchanged; INTEGRATION.md shows the batched form of the call site.
int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, Matrix3f &F12,
                                       vector<pair<size_t, size_t> > &vMatchedPairs, const bool bOnlyStereo) {
    return gpu::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, mbCheckOrientation);  // :597-746
}
