// OptimizerGPU.h — Optimizer::PoseOptimization(Frame*) on the GPU, read through the
// reference's own Frame / MapPoint members.
//
// Optimizer.cc includes Optimizer_pose_gpu.inc in place of the body of
//   int Optimizer::PoseOptimization(Frame *pFrame)                     Optimizer.cc:1656-1842
// Optimizer.h and every caller (Tracking.cc:1030, 1186, 1229, 1921, 1937, 1951, 2212) stay unchanged.
// The gather of mvKeys / mvuRight / GetWorldPos() runs under MapPoint::mGlobalMutex as
// the reference's edge set-up does (Optimizer.cc:1694); the whole optimisation (4 rounds
// of Levenberg-Marquardt, the classification) is one GPU call, ygzfe_pose_optimization;
// mvbOutlier and the pose are written back as the reference writes them.
#ifndef YGZFE_OPTIMIZER_GPU_H_
#define YGZFE_OPTIMIZER_GPU_H_

#include <cstdint>
#include <type_traits>
#include <vector>

#include "ygzfe_dropin.h"

namespace ygz {
namespace gpu {

// One problem's packed inputs: PoseOptimization(Frame*) and, for Relocalization's
// candidates, the rows of a batch.
struct PoseProblem {
    ygzfe_camera cam;
    float bf;
    ygzfe_se3 T;
    std::vector<ygzfe_kp> kps;
    std::vector<float> u_right, xw;
    std::vector<uint8_t> present;
};

// Optimizer.cc:1677-1764 without the g2o objects.  The caller holds MapPoint::mGlobalMutex.
template <class FrameT>
inline void GatherPoseProblem(FrameT *pFrame, PoseProblem &P) {
    const int N = pFrame->N;
    P.cam.fx = pFrame->fx;
    P.cam.fy = pFrame->fy;
    P.cam.cx = pFrame->cx;
    P.cam.cy = pFrame->cy;
    P.bf = pFrame->mbf;
    P.T.q[0] = pFrame->mTcw.unit_quaternion().x();
    P.T.q[1] = pFrame->mTcw.unit_quaternion().y();
    P.T.q[2] = pFrame->mTcw.unit_quaternion().z();
    P.T.q[3] = pFrame->mTcw.unit_quaternion().w();
    for (int k = 0; k < 3; k++) P.T.t[k] = pFrame->mTcw.translation()[k];
    P.kps.resize(N);
    P.u_right.resize(N);
    P.xw.assign(3 * (size_t)N, 0.f);
    P.present.assign(N, 0);
    for (int i = 0; i < N; i++) {
        ygzfe_kp &k = P.kps[i];
        k.x = pFrame->mvKeys[i].pt.x;
        k.y = pFrame->mvKeys[i].pt.y;
        k.size = k.angle = k.response = 0.f;
        k.octave = pFrame->mvKeys[i].octave;
        k.class_id = -1;
        P.u_right[i] = pFrame->mvuRight[i];
        auto *pMP = pFrame->mvpMapPoints[i];
        if (!pMP) continue;
        P.present[i] = 1;
        const auto Xw = pMP->GetWorldPos();
        for (int c = 0; c < 3; c++) P.xw[3 * (size_t)i + c] = Xw[c];
    }
}

// Optimizer.cc:1767-1841 on the device; writes mvbOutlier and the pose, returns the inlier count.
template <class FrameT>
inline int ApplyPoseResult(FrameT *pFrame, const PoseProblem &P, const ygzfe_pose_opt_result &r,
                           const std::vector<uint8_t> &outlier) {
    if (r.rounds <= 0) return 0;  // fewer than 3 correspondences (:1767): pose untouched
    for (int i = 0; i < pFrame->N; i++)
        if (P.present[i]) pFrame->mvbOutlier[i] = outlier[i] != 0;
    typedef typename std::decay<decltype(pFrame->mTcw)>::type SE3;
    typedef typename std::decay<decltype(pFrame->mTcw.unit_quaternion())>::type Quat;
    typedef typename std::decay<decltype(pFrame->mTcw.translation())>::type Vec;
    pFrame->SetPose(SE3(Quat(r.T_cw.q[3], r.T_cw.q[0], r.T_cw.q[1], r.T_cw.q[2]),
                        Vec(r.T_cw.t[0], r.T_cw.t[1], r.T_cw.t[2])));
    return r.n_inliers;
}

template <class FrameT, class Lock>
inline int PoseOptimization(FrameT *pFrame, Lock &&lock_global_mutex) {
    PoseProblem P;
    {
        auto lock = lock_global_mutex();  // unique_lock<mutex>(MapPoint::mGlobalMutex), Optimizer.cc:1694
        (void)lock;
        GatherPoseProblem(pFrame, P);
    }
    std::vector<uint8_t> outlier(P.present.size(), 0);
    ygzfe_pose_opt_result r;
    const int rc = ygzfe_pose_optimization(dropin::device(), &P.cam, P.bf, &P.T, pFrame->N, P.kps.data(),
                                           P.u_right.data(), P.xw.data(), P.present.data(),
                                           pFrame->mvInvLevelSigma2.data(), (int)pFrame->mvInvLevelSigma2.size(),
                                           outlier.data(), &r);
    if (rc != YGZFE_OK) {
        dropin::log_once("PoseOptimization", dropin::last_error());
        return 0;
    }
    return ApplyPoseResult(pFrame, P, r, outlier);
}

}  // namespace gpu
}  // namespace ygz
#endif
