// api_poseopt.cpp — pose-only optimisation, on device pointers and on host arrays.
#include <string.h>

#include "host.hpp"

// ------------------------------------------------------------------ pose-only optimisation
// Optimizer::PoseOptimization (Optimizer.cc:1656-1842), poseopt.hip
int ygzfe_pose_optimization_batch(int device, int n_problems, const int32_t *d_problem_ptr,
                                  const ygzfe_camera *d_cam, const float *d_bf, const ygzfe_se3 *d_T_init,
                                  const ygzfe_kp *d_kps, const float *d_u_right, const float *d_xw,
                                  const uint8_t *d_present, const float *d_inv_level_sigma2, int n_levels,
                                  uint8_t *d_outlier, ygzfe_pose_opt_result *d_results, void *stream) {
    if (n_problems < 0 || n_levels <= 0 ||
        (n_problems > 0 && (!d_problem_ptr || !d_cam || !d_bf || !d_T_init || !d_kps || !d_xw || !d_present ||
                            !d_inv_level_sigma2 || !d_outlier || !d_results))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    if (n_problems == 0) return YGZFE_OK;
    YGZ_TRY(ensure_device(device));
    YGZ_HIP(launch_pose_opt(n_problems, d_problem_ptr, d_cam, d_bf, d_T_init, d_kps, d_u_right, d_xw, d_present,
                            d_inv_level_sigma2, n_levels, d_outlier, d_results, (hipStream_t)stream));
    return YGZFE_OK;
}

int ygzfe_pose_optimization(int device, const ygzfe_camera *cam, float bf, const ygzfe_se3 *T_cw_init, int n,
                            const ygzfe_kp *kps, const float *u_right, const float *xw, const uint8_t *present,
                            const float *inv_level_sigma2, int n_levels, uint8_t *outlier_out,
                            ygzfe_pose_opt_result *result) {
    if (!cam || !T_cw_init || !result || n < 0 || n_levels <= 0 || !inv_level_sigma2 ||
        (n > 0 && (!kps || !xw || !present || !outlier_out))) {
        set_error("invalid argument");
        return YGZFE_EINVAL;
    }
    for (int i = 0; i < n; i++)
        if (present[i] && (kps[i].octave < 0 || kps[i].octave >= n_levels)) {
            set_error("row %d: octave %d outside [0, %d)", i, kps[i].octave, n_levels);
            return YGZFE_EINVAL;
        }
    StagingLease S;
    YGZ_TRY(S.acquire(device));
    // in: [problem_ptr 2][cam][bf][T_init][inv_sigma2][kps][xw][u_right][present]  out: [result][outlier]
    const size_t rows = (size_t)(n > 0 ? n : 1);
    const int32_t ptr[2] = {0, n};
    BlockLayout in{16}, out{16};
    const size_t o_ptr = in.take(sizeof(ptr)), o_cam = in.take(sizeof(*cam)), o_bf = in.take(sizeof(bf));
    const size_t o_T = in.take(sizeof(*T_cw_init)), o_sig = in.take(n_levels, 4), o_kps = in.take(rows, sizeof(*kps));
    const size_t o_xw = in.take(rows, 12), o_ur = in.take(rows, 4), o_pr = in.take(rows), in_bytes = in.size();
    const size_t o_res = out.take(sizeof(ygzfe_pose_opt_result)), o_flags = out.take(rows), out_bytes = out.size();
    YGZ_TRY(S.reserve(in_bytes, out_bytes));
    uint8_t *h = S->hin.as<uint8_t>(), *d = S->dev.as<uint8_t>();
    memcpy(h + o_ptr, ptr, sizeof(ptr));
    memcpy(h + o_cam, cam, sizeof(*cam));
    memcpy(h + o_bf, &bf, sizeof(bf));
    memcpy(h + o_T, T_cw_init, sizeof(*T_cw_init));
    memcpy(h + o_sig, inv_level_sigma2, (size_t)n_levels * 4);
    if (n > 0) {
        memcpy(h + o_kps, kps, (size_t)n * sizeof(ygzfe_kp));
        memcpy(h + o_xw, xw, (size_t)n * 12);
        if (u_right) memcpy(h + o_ur, u_right, (size_t)n * 4);
        memcpy(h + o_pr, present, (size_t)n);
    }
    YGZ_TRY(S.upload(in_bytes));
    uint8_t *dout = d + in_bytes;
    YGZ_TRY(ygzfe_pose_optimization_batch(
        device, 1, at<const int32_t>(d, o_ptr), at<const ygzfe_camera>(d, o_cam), at<const float>(d, o_bf),
        at<const ygzfe_se3>(d, o_T), at<const ygzfe_kp>(d, o_kps), u_right ? at<const float>(d, o_ur) : nullptr,
        at<const float>(d, o_xw), d + o_pr, at<const float>(d, o_sig), n_levels, dout + o_flags,
        at<ygzfe_pose_opt_result>(dout, o_res), S->stream));
    YGZ_TRY(S.download(in_bytes, out_bytes));
    memcpy(result, S->hout.as<uint8_t>() + o_res, sizeof(*result));
    if (result->rounds > 0) {  // mvbOutlier is written where a map point is present only
        const uint8_t *flags = S->hout.as<uint8_t>() + o_flags;
        for (int i = 0; i < n; i++)
            if (present[i]) outlier_out[i] = flags[i];
    }
    return YGZFE_OK;
}
