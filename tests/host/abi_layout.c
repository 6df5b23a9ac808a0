/* Layout of every public struct of include/ygzfe.h that the Python binding mirrors: one line
 * "struct size" per struct and one line "struct.field offset size" per field (nested ygzfe_se3
 * members also by their dotted leaves).  tests/test_cpu_abi.py compares the output with the
 * ctypes.Structure classes and the numpy dtypes of ygzfe/__init__.py. */
#include <stddef.h>
#include <stdio.h>

struct ygzfe_align_result; /* ygzfe_batch_pack_slots names it before the header defines it (a C warning) */
#include "ygzfe.h"

#define S(s) printf("%s %zu\n", #s, sizeof(ygzfe_##s))
#define F(s, f) printf("%s.%s %zu %zu\n", #s, #f, offsetof(ygzfe_##s, f), sizeof(((ygzfe_##s *)0)->f))

int main(void) {
    S(kp); F(kp, x); F(kp, y); F(kp, size); F(kp, angle); F(kp, response); F(kp, octave); F(kp, class_id);
    S(orb_params); F(orb_params, nfeatures); F(orb_params, scale_factor); F(orb_params, nlevels);
    F(orb_params, ini_th_fast); F(orb_params, min_th_fast); F(orb_params, blur_variant);
    S(camera); F(camera, fx); F(camera, fy); F(camera, cx); F(camera, cy);
    S(se3); F(se3, q); F(se3, t);
    S(bounds); F(bounds, min_x); F(bounds, max_x); F(bounds, min_y); F(bounds, max_y);
    S(match_query); F(match_query, u); F(match_query, v); F(match_query, radius); F(match_query, u_right);
    F(match_query, min_level); F(match_query, max_level); F(match_query, angle); F(match_query, flags);
    S(align_result); F(align_result, T_cur_ref); F(align_result, T_cur_ref.q); F(align_result, T_cur_ref.t);
    F(align_result, n_visible); F(align_result, chi2); F(align_result, H);
    S(direct_view); F(direct_view, R); F(direct_view, t); F(direct_view, Ow); F(direct_view, min_x);
    F(direct_view, max_x); F(direct_view, min_y); F(direct_view, max_y); F(direct_view, view_cos_limit);
    F(direct_view, mbf);
    S(direct_keyframes); F(direct_keyframes, n_kf); F(direct_keyframes, ref); F(direct_keyframes, kf_id);
    F(direct_keyframes, kf_excluded); F(direct_keyframes, T_rw); F(direct_keyframes, T_cr);
    S(direct_candidates); F(direct_candidates, n_cache); F(direct_candidates, n_local); F(direct_candidates, world);
    F(direct_candidates, normal); F(direct_candidates, min_dist); F(direct_candidates, max_dist);
    F(direct_candidates, skip); F(direct_candidates, obs_ptr); F(direct_candidates, obs_kf);
    F(direct_candidates, obs_kp);
    S(direct_map_result); F(direct_map_result, status); F(direct_map_result, px_out); F(direct_map_result, matched_kf);
    F(direct_map_result, matched_kp); F(direct_map_result, proj); F(direct_map_result, view_cos);
    F(direct_map_result, dist);
    S(pose_opt_result); F(pose_opt_result, T_cw); F(pose_opt_result, T_cw.q); F(pose_opt_result, T_cw.t);
    F(pose_opt_result, q); F(pose_opt_result, t); F(pose_opt_result, n_corr); F(pose_opt_result, n_inliers);
    F(pose_opt_result, rounds); F(pose_opt_result, iters); F(pose_opt_result, rejected); F(pose_opt_result, chi2);
    return 0;
}
