"""The C prototypes behind ygzfe, declared once, as `function=return kind:parameter kinds` entries.

Kinds: p any pointer (c_void_p: None, an int address, a c_void_p, byref(...), a ctypes array), s const char *,
i int / int32_t, f float, z size_t, d double, Q uint64_t, v a void return.  YGZFE holds exactly the prototypes of
include/ygzfe.h, in its order and without their ygzfe_ prefix (tests/test_cpu_abi.py parses the header against it);
SYNTH and SYNTH_HIP are the only declaration of what synth/synth.c and synth/plane_points.hip export (ygzs_).
"""
import ctypes as C

KINDS = {"p": C.c_void_p, "s": C.c_char_p, "i": C.c_int, "f": C.c_float, "z": C.c_size_t, "d": C.c_double,
         "Q": C.c_uint64, "v": None}

YGZFE = """
    last_error=s: device_count=i: extractor_create=i:pip extractor_destroy=v:p extractor_levels=i:pppppp
    extractor_features_per_level=i:pp extractor_dso_grid=i:ppp orb_plan=i:piippppp orb_plan_choices=i:piipp
    frame_create=i:piip frame_destroy=v:p compute_pyramid=i:pppi compute_pyramid_device=i:pppip frame_level=i:pipppi frame_set_level=i:pipi
    frame_levels=i:piipp frame_set_levels=i:piipp extract=i:ppipiipp detect_and_compute=i:pppipipp
    batch_create=i:piiiip batch_destroy=v:p batch_info=i:pppp batch_frames=i:pp batch_bind_buffers=i:ppppp
    batch_upload=i:ppi batch_extract=i:pip batch_extract_split=i:pipp batch_check=i:p batch_match=i:pipppppp
    batch_result=i:pipipp batch_device_results=i:ppppp batch_level=i:piipppp batch_read_level=i:piiipi
    batch_stats=i:pipp slot_bytes=z:i batch_pack_slots=i:piipipzp batch_timing=i:pippi batch_stream=p:p
    descriptor_distance=i:pp hamming_best2_device=i:pipipppp hamming_best2=i:ipipippp hamming_csr=i:ipipippp
    match_frame_create=i:ip match_frame_destroy=v:p match_frame_set=i:pppipp match_frame_stats=i:pp
    match_frame_resolve_stats=i:pp match_frame_from_batch=i:ppip search_projection_best=i:pppipiipp
    search_projection_ratio=i:pppipfpp search_for_initialization=i:pppifipp search_by_bow=i:pppipppipppfipp
    search_for_triangulation_batch=i:ppipppipppppppppppiiipp search_for_triangulation=i:ppipppppipppppppiiipp
    predict_scale_thresholds=i:fip fuse_search_batch=i:ippippppppfppifipp fuse_search=i:ppippppppfppifipp
    sparse_align=i:ppppppiiipp sparse_align_begin=i:ppppppiiip sparse_align_end=i:pp sparse_align_method=i:ppppppiiipip
    extractor_align_probe=i:ppp batch_sparse_align=i:pipppppiippp fast10_detect=i:ipiiipiiipip
    debug_dso_cells=i:ipiiiip align2d_batch=i:piippipp align2d_image=i:ipiiippipp
    find_direct_projection_batch=i:pppippppppp search_direct_batch=i:pippippppppfpp
    search_local_points_direct=i:pippiippppppfiippppp frame_set_keypoints=i:ppi frame_keypoint_count=i:p
    search_local_map_direct=i:pppppifiippp pose_optimization=i:ipfpipppppipp pose_optimization_batch=i:iipppppppppippp
    stereo_matches=i:ppppippiffpp batch_stereo=i:pippffppp stereo_from_rgbd=i:ipiiipifpp batch_stereo_rgbd=i:pipzifppp
    vocab_create=i:iiiiiippppp vocab_load_text=i:isp vocab_load_binary=i:isp vocab_destroy=v:p vocab_info=i:ppppppp
    bow_transform=i:ppiippp compute_bow=i:ppiipppppp batch_compute_bow=i:ppiippppppp undistort_create=i:ippiiip
    undistort_destroy=v:p undistort_maps=i:ppp undistort_apply_device=i:ppzipziip
    undistort_apply_f32_device=i:ppzipziip undistort_image=i:ppipi undistort_depth=i:ppipi
    compute_pyramid_undistorted=i:ppppi batch_undistort_device=i:pppzip batch_upload_undistorted=i:pppi
"""
SYNTH = "texture=v:Qiip render_plane=v:piiddpppiiQip backproject_plane=i:pppffdp trajectory_pose=v:ippp"
SYNTH_HIP = "plane_points=i:piiipppfpp render_plane_device=i:piiddppppiiiipzp"


def table(prefix, entries):
    """{function: kinds} of one of the blocks above."""
    return {prefix + e.split("=")[0]: e.split("=")[1] for e in entries.split()}


def declare(path, prefix, entries):
    """Load the library at `path` and set restype and argtypes of every function of `entries`: the one place that
    assigns them.  A function the library lacks is an AttributeError here, not at its first call."""
    lib = C.CDLL(path)
    for name, kinds in table(prefix, entries).items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = KINDS[kinds[0]], [KINDS[k] for k in kinds[2:]]
    return lib
