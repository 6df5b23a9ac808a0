// Optimizer_pose_gpu.inc — Optimizer::PoseOptimization(Frame*) on the GPU.
// Optimizer.cc: `#include "OptimizerGPU.h"` at the top, delete the body of
// PoseOptimization (Optimizer.cc:1656-1842) and, inside `namespace ygz { ... }`,
// `#include "Optimizer_pose_gpu.inc"`.  Optimizer.h and every caller stay unchanged.
// The gather still runs under MapPoint::mGlobalMutex, as the reference's does (:1694).
#ifndef YGZFE_POSE_GATHER_MUTEX
#define YGZFE_POSE_GATHER_MUTEX MapPoint::mGlobalMutex
#endif
int Optimizer::PoseOptimization(Frame *pFrame) {
    return gpu::PoseOptimization(pFrame, [] { return unique_lock<mutex>(YGZFE_POSE_GATHER_MUTEX); });
}
