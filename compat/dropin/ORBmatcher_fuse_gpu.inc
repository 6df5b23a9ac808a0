// ORBmatcher_fuse_gpu.inc — ORBmatcher::Fuse(pKF, vpMapPoints, th) on the GPU.
// ORBmatcher.cc: delete the body of this member function and, inside `namespace ygz { ... }`,
// `#include "ORBmatcher_fuse_gpu.inc"` (after including ORBmatcherFuseGPU.h).  ORBmatcher.h and
// LocalMapping.cc stay unchanged; INTEGRATION.md shows the batched form of SearchInNeighbors' forward phase.
int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th) {
    return gpu::Fuse(pKF, vpMapPoints, th);  // :748-886
}
