"""ygzfe — Python view of the MI355X front-end C ABI (include/ygzfe.h).

Mirrors the reference's hot-path interfaces so tests read like the reference:
  ORBextractor      ORBextractor.h:37-192   (ctor, operator(), ComputePyramid, getters)
  Frame             Frame::mvImagePyramid   (device-resident pyramid)
  ORBmatcher        ORBmatcher.h:38-178     (DescriptorDistance, dense / windowed search)
  SparseImgAlign    SparseImageAlign.h:37-60 (run)
  Align2D / FindDirectProjection            Align.h:20-26, ORBmatcher.cc:1573-1602
  Batch             many frames resident in HBM (bench / multi-GPU path)

All compute runs in lib/libygzfe.so on the GPU; there is no CPU fallback: the
module raises if the library or a HIP device is missing.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("YGZFE_LIB") or os.path.join(PKG_ROOT, "lib", "libygzfe.so")  # YGZFE_LIB: A/B builds
SYNTH_PATH = os.path.join(PKG_ROOT, "lib", "libygzsynth.so")
SYNTH_HIP_PATH = os.path.join(PKG_ROOT, "lib", "libygzsynth_hip.so")

MAX_LEVELS = 16
ORBSLAM_KEYPOINT, FAST_KEYPOINT, DSO_KEYPOINT = 0, 1, 2
BLUR_CV4, BLUR_CV3 = 0, 1
OK, EINVAL, EHIP, ECAP, ENOMEM, ESTATE = 0, -1, -2, -3, -4, -5

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class YgzfeError(RuntimeError):
    pass


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("blur_variant", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class SE3(C.Structure):
    _fields_ = [("q", C.c_float * 4), ("t", C.c_float * 3)]

    @staticmethod
    def make(q=(0, 0, 0, 1), t=(0, 0, 0)):
        s = SE3()
        for i in range(4):
            s.q[i] = float(q[i])
        for i in range(3):
            s.t[i] = float(t[i])
        return s

    def as_arrays(self):
        return np.array(self.q[:], np.float32), np.array(self.t[:], np.float32)


class AlignResult(C.Structure):
    _fields_ = [("T_cur_ref", SE3), ("n_visible", C.c_int32), ("chi2", C.c_float), ("H", C.c_float * 36)]


SE3_DTYPE = np.dtype([("q", "<f4", 4), ("t", "<f4", 3)])
ALIGN_RESULT_DTYPE = np.dtype([("q", "<f4", 4), ("t", "<f4", 3), ("n_visible", "<i4"), ("chi2", "<f4"),
                               ("H", "<f4", 36)])

_lib = None


def _load(path, prefix, entries, hint=""):
    if not os.path.exists(path):
        raise YgzfeError(f"{path} missing: run `make -C orb-ygz-slam_amd`{hint}")
    return _abi.declare(path, prefix, entries)


def lib():
    """Load libygzfe.so; raise loudly when it is absent (no fallback)."""
    global _lib
    if _lib is None:
        # torch ships its own libamdhip64.so.7; whichever copy loads first
        # serves the whole process, and torch refuses to run on a runtime it
        # was not built with.  Load torch's first so device pointers and
        # streams can be shared with it later in the same process.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = _load(LIB_PATH, "ygzfe_", _abi.YGZFE, " (or __graft_entry__.build())")
    return _lib


def _check(rc, what=""):
    if rc != OK:
        msg = lib().ygzfe_last_error().decode(errors="replace")
        raise YgzfeError(f"{what} failed ({rc}): {msg}")
    return rc


def _p(a):
    return C.c_void_p(a.ctypes.data)


def device_count():
    return lib().ygzfe_device_count()


def slot_bytes(kp_cap):
    """Bytes of one offline-sequence result slot (ygzfe_slot_bytes)."""
    return int(lib().ygzfe_slot_bytes(kp_cap))


def orb_plan(nfeatures, scale_factor, nlevels, ini_th=20, min_th=7, width=752, height=480, blur=BLUR_CV4):
    """Host-only extraction plan (ygzfe_orb_plan): level sizes, budgets, FAST cells, umax."""
    p = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th, blur)
    w, h, b, nc = (np.zeros(nlevels, np.int32) for _ in range(4))
    um = np.zeros(16, np.int32)
    _check(lib().ygzfe_orb_plan(C.byref(p), width, height, _p(w), _p(h), _p(b), _p(nc), _p(um)), "orb_plan")
    return {"sizes": list(zip(w.tolist(), h.tolist())), "budget": b.tolist(), "ncells": nc.tolist(),
            "umax": um.tolist()}


PLAN_LEVEL_FIELDS = ("n_ini", "oct_rb", "ncells", "fast_rw", "fast_rh", "node_class", "fast_S", "fast_R",
                     "sort0_keys_batch", "sort0_keys_single")


def orb_plan_choices(nfeatures, scale_factor, nlevels, ini_th=20, min_th=7, width=752, height=480, blur=BLUR_CV4):
    """Host-only (ygzfe_orb_plan_choices): what the launchers choose from the plan.  "levels": one dict of
    PLAN_LEVEL_FIELDS per level, plus "fast" = (S, R) of the level's own FAST launch (None without cells);
    "merged_fast": (S, R) of the single-frame path's one FAST launch (None without cells); "octree_groups"."""
    p = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th, blur)
    lv = np.zeros((nlevels, len(PLAN_LEVEL_FIELDS)), np.int32)
    pl = np.zeros(3, np.int32)
    _check(lib().ygzfe_orb_plan_choices(C.byref(p), width, height, _p(lv), _p(pl)), "orb_plan_choices")
    levels = [dict(zip(PLAN_LEVEL_FIELDS, row)) for row in lv.tolist()]
    for d in levels:
        d["fast"] = (d["fast_S"], d["fast_R"]) if d["ncells"] else None
    return {"levels": levels, "merged_fast": (int(pl[0]), int(pl[1])) if pl[0] else None, "octree_groups": int(pl[2])}


def _created(what, *args):
    """The handle that ygzfe_<what>(*args, &handle) makes."""
    h = C.c_void_p()
    _check(getattr(lib(), "ygzfe_" + what)(*args, C.byref(h)), what)
    return h


class _Handle:
    """Owner of the C handle .h (a c_void_p) that the function named _destroy frees.  Whoever destroys the handle
    through lib() directly sets .h to None."""
    _destroy = None

    def __del__(self):
        if getattr(self, "h", None) and self.h.value and _lib is not None:
            getattr(_lib, self._destroy)(self.h)
            self.h = None


class Frame(_Handle):
    """Device-resident pyramid (Frame::mvImagePyramid)."""
    _destroy = "ygzfe_frame_destroy"

    def __init__(self, extractor, width, height):
        self.ex = extractor
        self.width, self.height = width, height
        self.h = _created("frame_create", extractor.h, width, height)

    def level(self, l):
        w, h = C.c_int(), C.c_int()
        _check(lib().ygzfe_frame_level(self.h, l, C.byref(w), C.byref(h), None, 0), "frame_level")
        out = np.zeros((h.value, w.value), np.uint8)
        _check(lib().ygzfe_frame_level(self.h, l, None, None, _p(out), w.value), "frame_level")
        return out

    def levels(self):
        return [self.level(l) for l in range(self.ex.nlevels)]

    def set_level(self, l, img):
        img = np.ascontiguousarray(img, np.uint8)
        _check(lib().ygzfe_frame_set_level(self.h, l, _p(img), img.shape[1]), "frame_set_level")

    def set_levels(self, imgs, first=0):
        """Upload levels [first, first + len(imgs)) of a host pyramid in one DMA (ygzfe_frame_set_levels)."""
        imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
        src = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        strides = (C.c_int * len(imgs))(*[im.shape[1] for im in imgs])
        _check(lib().ygzfe_frame_set_levels(self.h, first, len(imgs), src, strides), "frame_set_levels")

    def set_keypoints(self, kps):
        """A keyframe's mvKeys, resident with the frame (read by search_local_map_direct)."""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        _check(lib().ygzfe_frame_set_keypoints(self.h, _p(kps), len(kps)), "frame_set_keypoints")

    def keypoint_count(self):
        """Keypoints set with set_keypoints, or -1 when none were."""
        return int(lib().ygzfe_frame_keypoint_count(self.h))


class ORBextractor(_Handle):
    """ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) (ORBextractor.h:53-57)."""
    _destroy = "ygzfe_extractor_destroy"

    def __init__(self, nfeatures=500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, device=0,
                 blur=BLUR_CV4):
        self.params = OrbParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, blur)
        self.nlevels = nlevels
        self.h = _created("extractor_create", C.byref(self.params), device)

    # getters (ORBextractor.h:87-109)
    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return self.params.scale_factor

    def _levels(self):
        arrs = [np.zeros(MAX_LEVELS, np.float32) for _ in range(4)]
        _check(lib().ygzfe_extractor_levels(self.h, None, *[_p(a) for a in arrs]), "levels")
        return [a[:self.nlevels] for a in arrs]

    def GetScaleFactors(self):
        return self._levels()[0]

    def GetInverseScaleFactors(self):
        return self._levels()[1]

    def GetScaleSigmaSquares(self):
        return self._levels()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._levels()[3]

    def FeaturesPerLevel(self):
        out = np.zeros(MAX_LEVELS, np.int32)
        _check(lib().ygzfe_extractor_features_per_level(self.h, _p(out)), "features_per_level")
        return out[:self.nlevels].tolist()

    @property
    def dso_grid(self):
        g = C.c_int32()
        _check(lib().ygzfe_extractor_dso_grid(self.h, C.byref(g), None), "dso_grid")
        return g.value

    @dso_grid.setter
    def dso_grid(self, v):
        g = C.c_int32(v)
        _check(lib().ygzfe_extractor_dso_grid(self.h, None, C.byref(g)), "dso_grid")

    def ComputePyramid(self, image, frame=None):
        """Frame::ComputeImagePyramid -> a device Frame holding mvImagePyramid."""
        image = np.ascontiguousarray(image, np.uint8)
        H, W = image.shape
        frame = frame if frame is not None else Frame(self, W, H)
        _check(lib().ygzfe_compute_pyramid(self.h, frame.h, _p(image), W), "compute_pyramid")
        return frame

    def extract(self, frame, method=ORBSLAM_KEYPOINT, existing=None, cap=None):
        """operator()(Frame*, keypoints, descriptors, method) (ORBextractor.cc:1031-1127).

        Returns (keypoints[KP_DTYPE], descriptors uint8[n,32]); rows of `existing`
        come first (their angles are recomputed in DSO mode, as the reference does)."""
        existing = np.zeros(0, KP_DTYPE) if existing is None else np.ascontiguousarray(existing, KP_DTYPE)
        ne = len(existing)
        cap = cap or (ne + 8192)
        kps = np.zeros(cap, KP_DTYPE)
        kps[:ne] = existing
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        rc = lib().ygzfe_extract(self.h, frame.h, method, _p(kps), ne, cap, _p(desc), C.byref(n))
        if rc == ECAP:
            return self.extract(frame, method, existing, cap=n.value)
        _check(rc, "extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors) (ORBextractor.cc:970-1028)."""
        frame = self.ComputePyramid(image)
        return self.extract(frame, ORBSLAM_KEYPOINT)


def debug_dso_cells(img, g, barrier, device=0):
    """The DSO_KEYPOINT cell kernel's own FAST-10 pass (ygzfe_debug_dso_cells): for each g x g
    cell of the grid, row-major, the cell-relative corners in raster order (int16[n, 2] (x, y)),
    from one pass at `barrier` over the kernel's scan region; border cells are empty."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    ncells = (H // g) * (W // g)
    flags = np.zeros((max(ncells, 1), g, g), np.uint8)
    _check(lib().ygzfe_debug_dso_cells(device, _p(img), W, H, int(g), int(barrier), _p(flags)), "debug_dso_cells")
    out = []
    for k in range(ncells):
        ys, xs = np.nonzero(flags[k])  # raster order (row-major nonzero)
        out.append(np.stack([xs, ys], 1).astype(np.int16))
    return out


def fast10_detect(img, barrier, rois, sse=True, cap=None, device=0):
    """Thirdparty/fast FAST-10 on the GPU (ygzfe_fast10_detect): fast_corner_detect_10_sse2 (sse) or
    fast_corner_detect_10 over each ROI (x0, y0, w, h) of `img` -> list of int16[n, 2] (x, y) corner
    arrays, ROI-relative and in the reference's raster order.  `cap` (corners per ROI) defaults to
    1 << 16 bounded by the largest ROI's pixel count; when a ROI holds more, the call is repeated
    once with the cap the first call's counts report (ygzfe.h: ECAP, counts = corners found)."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    rois = np.ascontiguousarray(rois, np.int32).reshape(-1, 4)
    n = len(rois)
    area = max(1, int((rois[:, 2].clip(0) * rois[:, 3].clip(0)).max())) if n else 1
    retry = cap is None
    cap = min(area, 1 << 16) if cap is None else cap
    while True:
        xy = np.zeros((max(n, 1), cap, 2), np.int16)
        counts = np.zeros(max(n, 1), np.int32)
        rc = lib().ygzfe_fast10_detect(device, _p(img), W, H, W, _p(rois), n, int(barrier), int(bool(sse)), _p(xy),
                                       cap, _p(counts))
        if rc == ECAP and retry:
            retry = False
            cap = int(counts.max())
            continue
        _check(rc, "fast10_detect")
        break
    return [xy[r, :counts[r]].copy() for r in range(n)]


class Undistort(_Handle):
    """Frame::ComputeImagePyramid's undistortion (Frame.cc:775-790): the CV_16SC2
    initUndistortRectifyMap maps, built on the device once per camera, and the
    INTER_LINEAR remap applied per frame."""
    _destroy = "ygzfe_undistort_destroy"

    def __init__(self, cam, dist, width, height, device=0):
        cam = cam if isinstance(cam, Camera) else Camera(*[float(c) for c in cam])
        d = np.ascontiguousarray(dist, np.float32).ravel()
        self.width, self.height, self.device = width, height, device
        self.h = _created("undistort_create", device, C.byref(cam), _p(d) if len(d) else None, len(d), width, height)

    def maps(self):
        """(map1 int16[H, W, 2], map2 uint16[H, W]) -- OpenCV's CV_16SC2 + CV_16UC1 pair."""
        m1 = np.zeros((self.height, self.width, 2), np.int16)
        m2 = np.zeros((self.height, self.width), np.uint16)
        _check(lib().ygzfe_undistort_maps(self.h, _p(m1), _p(m2)), "undistort_maps")
        return m1, m2

    def apply_device(self, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_images, stream=None):
        _check(lib().ygzfe_undistort_apply_device(self.h, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride,
                                                  n_images, stream), "undistort_apply")

    def apply_f32_device(self, d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_images, stream=None):
        """remap of n CV_32F device images (pitch / stride in floats): Frame.cc:799-804."""
        _check(lib().ygzfe_undistort_apply_f32_device(self.h, d_src, src_pitch, src_stride, d_dst, dst_pitch,
                                                      dst_stride, n_images, stream), "undistort_apply_f32")

    def remap_image(self, image):
        """cv::remap(mImGray / mImRight, ..., INTER_LINEAR) on a host u8 image (Frame.cc:786-797)."""
        image = np.ascontiguousarray(image, np.uint8)
        out = np.zeros_like(image)
        _check(lib().ygzfe_undistort_image(self.h, _p(image), image.shape[1], _p(out), out.shape[1]), "undistort_image")
        return out

    def remap_depth(self, depth):
        """cv::remap(mImDepth, ..., INTER_LINEAR) on a host CV_32F depth image (Frame.cc:799-804)."""
        depth = np.ascontiguousarray(depth, np.float32)
        out = np.zeros_like(depth)
        _check(lib().ygzfe_undistort_depth(self.h, _p(depth), depth.shape[1], _p(out), out.shape[1]), "undistort_depth")
        return out

    def ComputePyramid(self, extractor, image, frame=None):
        """ComputeImagePyramid with mDistCoef != 0: remap(image) -> level 0 -> levels."""
        image = np.ascontiguousarray(image, np.uint8)
        H, W = image.shape
        frame = frame if frame is not None else Frame(extractor, W, H)
        _check(lib().ygzfe_compute_pyramid_undistorted(extractor.h, frame.h, self.h, _p(image), W),
               "compute_pyramid_undistorted")
        return frame


class ORBmatcher:
    """Hamming hot subset of ORBmatcher (ORBmatcher.h:38-178)."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.nnratio, self.checkOri, self.device = nnratio, checkOri, device

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().ygzfe_descriptor_distance(_p(a), _p(b))

    def best2(self, query, train):
        q = np.ascontiguousarray(query, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
        nq = len(q)
        bi = np.zeros(nq, np.int32)
        bd = np.zeros(nq, np.int32)
        sd = np.zeros(nq, np.int32)
        _check(lib().ygzfe_hamming_best2(self.device, _p(q), nq, _p(t), len(t), _p(bi), _p(bd), _p(sd)),
               "hamming_best2")
        return bi, bd, sd

    def window_distances(self, query, train, row_ptr, cand):
        q = np.ascontiguousarray(query, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        cand = np.ascontiguousarray(cand, np.int32)
        out = np.zeros(max(1, len(cand)), np.int32)
        _check(lib().ygzfe_hamming_csr(self.device, _p(q), len(q), _p(t), len(t), _p(row_ptr), _p(cand), _p(out)),
               "hamming_csr")
        return out[:len(cand)]


MATCH_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("u_right", "<f4"),
                              ("min_level", "<i4"), ("max_level", "<i4"), ("angle", "<f4"), ("flags", "<i4")])
MQ_VALID, MQ_BLOCKS, MQ_STEREO = 1, 2, 4


class Bounds(C.Structure):
    """Frame::mnMinX / mnMaxX / mnMinY / mnMaxY (Frame.cc:501-507)."""
    _fields_ = [("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class MatchFrame(_Handle):
    """The searched Frame's state on the device (mvKeys, mDescriptors, mvuRight, bounds;
    the 64 x 48 grid of AssignFeaturesToGrid is built there)."""
    _destroy = "ygzfe_match_frame_destroy"

    def __init__(self, device=0):
        self.h = _created("match_frame_create", device)
        self.n = 0

    def set(self, kps, desc, u_right=None, bounds=(0.0, 752.0, 0.0, 480.0)):
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        b = Bounds(*[float(x) for x in bounds])
        _check(lib().ygzfe_match_frame_set(self.h, _p(kps), _p(desc), len(kps), None if ur is None else _p(ur),
                                           C.byref(b)), "match_frame_set")
        self.n = len(kps)
        return self

    def rescans(self):
        """Queries of the last search whose top-K candidates the sequential skips used up."""
        r = C.c_int()
        _check(lib().ygzfe_match_frame_stats(self.h, C.byref(r)), "match_frame_stats")
        return r.value

    def resolve_passes(self):
        """Parallel-resolve passes of the last search (-1: the serial replay decided)."""
        r = C.c_int()
        _check(lib().ygzfe_match_frame_resolve_stats(self.h, C.byref(r)), "match_frame_resolve_stats")
        return r.value

    def from_batch(self, batch, frame, bounds=(0.0, 752.0, 0.0, 480.0)):
        b = Bounds(*[float(x) for x in bounds])
        _check(lib().ygzfe_match_frame_from_batch(self.h, batch.h, frame, C.byref(b)), "match_frame_from_batch")
        return self


def search_projection_best(cur, queries, q_desc, blocked=None, th_dist=100, check_ori=True):
    """SearchByProjection(CurrentFrame, LastFrame | pKF, ...) (ORBmatcher.cc:1218-1469):
    -> (train_match int32[cur.n]: -1 untouched / -2 NULLed by the rotation check / query, nmatches)."""
    q = np.ascontiguousarray(queries, MATCH_QUERY_DTYPE)
    d = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
    bl = None if blocked is None else np.ascontiguousarray(blocked, np.uint8)
    out = np.zeros(max(cur.n, 1), np.int32)
    nm = C.c_int()
    _check(lib().ygzfe_search_projection_best(cur.h, _p(q), _p(d), len(q), None if bl is None else _p(bl), th_dist,
                                              int(check_ori), _p(out), C.byref(nm)), "search_projection_best")
    return out[:cur.n], nm.value


def search_projection_ratio(F, queries, q_desc, blocked=None, nnratio=0.6):
    """SearchByProjection(F, vpMapPoints, th, checkLevel) (ORBmatcher.cc:43-126) -> (train_match, nmatches)."""
    q = np.ascontiguousarray(queries, MATCH_QUERY_DTYPE)
    d = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
    bl = None if blocked is None else np.ascontiguousarray(blocked, np.uint8)
    out = np.zeros(max(F.n, 1), np.int32)
    nm = C.c_int()
    _check(lib().ygzfe_search_projection_ratio(F.h, _p(q), _p(d), len(q), None if bl is None else _p(bl), nnratio,
                                               _p(out), C.byref(nm)), "search_projection_ratio")
    return out[:F.n], nm.value


def search_for_initialization(F1, F2, prev_matched, window_size=100, nnratio=0.9, check_ori=True):
    """SearchForInitialization (ORBmatcher.cc:375-478) -> (vnMatches12, nmatches, vbPrevMatched updated)."""
    prev = np.ascontiguousarray(prev_matched, np.float32).reshape(-1, 2).copy()
    m12 = np.zeros(max(F1.n, 1), np.int32)
    nm = C.c_int()
    _check(lib().ygzfe_search_for_initialization(F1.h, F2.h, _p(prev), window_size, nnratio, int(check_ori),
                                                 _p(m12), C.byref(nm)), "search_for_initialization")
    return m12[:F1.n], nm.value, prev


def search_by_bow(kf, F, kf_usable, fv_kf, fv_f, nnratio=0.7, check_ori=False):
    """SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:155-263).  fv_* = (nodes, ptr, feats)
    node-sorted CSR FeatureVectors -> (f_match int32[F.n]: KF index or -1, nmatches)."""
    us = np.ascontiguousarray(kf_usable, np.uint8)
    kn, kp, kfe = (np.ascontiguousarray(a, np.int32) for a in fv_kf)
    fn, fp, ffe = (np.ascontiguousarray(a, np.int32) for a in fv_f)
    out = np.zeros(max(F.n, 1), np.int32)
    nm = C.c_int()
    _check(lib().ygzfe_search_by_bow(kf.h, F.h, _p(us), len(kn), _p(kn), _p(kp), _p(kfe), len(fn), _p(fn), _p(fp),
                                     _p(ffe), nnratio, int(check_ori), _p(out), C.byref(nm)), "search_by_bow")
    return out[:F.n], nm.value


def _fv(fv):
    """(nodes, ptr, feats) of a FeatureVector as int32 arrays; ptr of an empty one is [0]."""
    nodes, ptr, feats = (np.ascontiguousarray(a, np.int32).ravel() for a in fv)
    return nodes, (ptr if len(ptr) else np.zeros(1, np.int32)), feats


def search_for_triangulation_batch(kf1, kf2s, has_mp1, fv1, has_mp2s, fv2s, F12s, epipoles, level_sigma2,
                                   scale_factors, only_stereo=False, check_ori=True):
    """SearchForTriangulation (ORBmatcher.cc:597-746) of keyframe kf1 against every neighbour of kf2s in one call
    (LocalMapping::CreateNewMapPoints).  has_mp*: GetMapPoint(i) != NULL; fv* = (nodes, ptr, feats) node-sorted CSR
    FeatureVectors; F12s [n_nb, 3, 3]; epipoles [n_nb, 2] = (ex, ey) of :603-609.
    -> (matches12 int32[n_nb, kf1.n]: KF2 index or -1, nmatches int32[n_nb])."""
    n_nb = len(kf2s)
    hm1 = np.ascontiguousarray(has_mp1, np.uint8)
    n1, p1, f1 = _fv(fv1)
    hm2 = [np.ascontiguousarray(a, np.uint8).ravel() for a in has_mp2s]
    fvs = [_fv(fv) for fv in fv2s]
    if not (len(hm2) == len(fvs) == n_nb):
        raise ValueError("one has_mp2 and one FeatureVector per neighbour")
    cat = lambda xs, dt: np.concatenate([np.zeros(0, dt)] + list(xs)).astype(dt)  # noqa: E731
    mp2_ptr = np.concatenate([[0], np.cumsum([len(a) for a in hm2])]).astype(np.int32)
    fv2_ptr = np.concatenate([[0], np.cumsum([len(n) for n, _, _ in fvs])]).astype(np.int32)
    feat_off = np.concatenate([[0], np.cumsum([len(f) for _, _, f in fvs])]).astype(np.int64)
    ptr2 = cat([[0]] + [p[1:len(n) + 1] + feat_off[k] for k, (n, p, _) in enumerate(fvs)], np.int32)
    nodes2, feats2 = cat([n for n, _, _ in fvs], np.int32), cat([f for _, _, f in fvs], np.int32)
    hm2c = cat(hm2, np.uint8)
    F = np.ascontiguousarray(F12s, np.float32).reshape(n_nb, 9)
    ep = np.ascontiguousarray(epipoles, np.float32).reshape(n_nb, 2)
    sig, sc = np.ascontiguousarray(level_sigma2, np.float32), np.ascontiguousarray(scale_factors, np.float32)
    if len(sig) != len(sc):
        raise ValueError("level_sigma2 and scale_factors differ in length")
    hs = (C.c_void_p * max(n_nb, 1))(*[f.h.value for f in kf2s])
    m12 = np.full((n_nb, kf1.n), -2, np.int32)  # -2: not written (an error return leaves the outputs alone)
    nm = np.full(n_nb, -2, np.int32)
    _check(lib().ygzfe_search_for_triangulation_batch(
        kf1.h, _p(hm1), len(n1), _p(n1), _p(p1), _p(f1), n_nb, hs, _p(mp2_ptr), _p(hm2c), _p(fv2_ptr), _p(nodes2),
        _p(ptr2), _p(feats2), _p(F), _p(ep), _p(sig), _p(sc), len(sig), int(only_stereo), int(check_ori), _p(m12),
        _p(nm)), "search_for_triangulation_batch")
    return m12, nm


def search_for_triangulation(kf1, kf2, has_mp1, fv1, has_mp2, fv2, F12, epipole, level_sigma2, scale_factors,
                             only_stereo=False, check_ori=True):
    """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORBmatcher.cc:597-746) for one neighbour
    -> (matches12 int32[kf1.n]: KF2 index or -1, nmatches)."""
    hm1, hm2 = np.ascontiguousarray(has_mp1, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
    n1, p1, f1 = _fv(fv1)
    n2, p2, f2 = _fv(fv2)
    F, ep = np.ascontiguousarray(F12, np.float32).reshape(9), np.ascontiguousarray(epipole, np.float32).reshape(2)
    sig, sc = np.ascontiguousarray(level_sigma2, np.float32), np.ascontiguousarray(scale_factors, np.float32)
    if len(sig) != len(sc):
        raise ValueError("level_sigma2 and scale_factors differ in length")
    m12 = np.full(kf1.n, -2, np.int32)
    nm = np.full(1, -2, np.int32)
    _check(lib().ygzfe_search_for_triangulation(
        kf1.h, _p(hm1), len(n1), _p(n1), _p(p1), _p(f1), kf2.h, _p(hm2), len(n2), _p(n2), _p(p2), _p(f2), _p(F), _p(ep),
        _p(sig), _p(sc), len(sig), int(only_stereo), int(check_ori), _p(m12), _p(nm)), "search_for_triangulation")
    return m12, int(nm[0])


def predict_scale_thresholds(log_scale_factor, n_levels):
    """MapPoint::PredictScale (MapPoint.cc:343-357) as a table (host only): float32[n_levels - 1], thr[L-1] = the
    smallest positive float r with ceil(logf(r) / log_scale_factor) >= L; the level of a ratio is the number of
    thresholds <= ratio."""
    thr = np.zeros(16, np.float32)
    _check(lib().ygzfe_predict_scale_thresholds(float(log_scale_factor), int(n_levels), _p(thr)),
           "predict_scale_thresholds")
    return thr[:n_levels - 1].copy()


def fuse_search_batch(kfs, views, world, normal, min_dist, max_dist, desc, scale_factors, inv_level_sigma2,
                      log_scale_factor, skip=None, th=3.0, check_reproj=True, best_idx=None, best_dist=None):
    """The search of ORBmatcher::Fuse (ORBmatcher.cc:748-866) for every (keyframe, map point) pair in one call
    (LocalMapping::SearchInNeighbors).  kfs: MatchFrames; views [n_kf, 20] = Rcw row-major, tcw, Ow, fx, fy, cx, cy,
    bf; world / normal [n_pts, 3]; min_dist / max_dist the raw mfMinDistance / mfMaxDistance; desc [n_pts, 32];
    skip [n_kf, n_pts] or None; check_reproj=False is the Sim3 form's search.
    -> (best_idx int32[n_kf, n_pts]: the keypoint when bestDist <= 50 else -1, best_dist int32[n_kf, n_pts]:
    the distance, 256 when no candidate was kept).  best_idx / best_dist: arrays to write instead of new ones."""
    n_kf = len(kfs)
    w = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
    n_pts = len(w)
    nrm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    mn, mx = np.ascontiguousarray(min_dist, np.float32).ravel(), np.ascontiguousarray(max_dist, np.float32).ravel()
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    vw = np.ascontiguousarray(views, np.float32).reshape(-1, 20)
    sc, sig = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(inv_level_sigma2, np.float32)
    if not (len(nrm) == len(mn) == len(mx) == len(d) == n_pts) or len(vw) != n_kf or len(sc) != len(sig):
        raise ValueError("fuse_search_batch: array lengths disagree")
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n_kf, n_pts)
    hs = (C.c_void_p * max(n_kf, 1))(*[f.h.value for f in kfs])
    bi = np.full((n_kf, n_pts), -2, np.int32) if best_idx is None else best_idx  # -2: not written
    bd = np.full((n_kf, n_pts), -2, np.int32) if best_dist is None else best_dist
    assert bi.dtype == bd.dtype == np.int32 and bi.size == bd.size == n_kf * n_pts and bi.flags.c_contiguous
    _check(lib().ygzfe_fuse_search_batch(n_kf, hs, _p(vw), n_pts, _p(w), _p(nrm), _p(mn), _p(mx), _p(d),
                                         None if sk is None else _p(sk), float(th), _p(sc), _p(sig), len(sc),
                                         float(log_scale_factor), int(check_reproj), _p(bi), _p(bd)),
           "fuse_search_batch")
    return bi, bd


def fuse_search(kf, view, world, normal, min_dist, max_dist, desc, scale_factors, inv_level_sigma2, log_scale_factor,
                skip=None, th=3.0, check_reproj=True):
    """ORBmatcher::Fuse's search for one keyframe -> (best_idx int32[n_pts], best_dist int32[n_pts])."""
    w = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
    n_pts = len(w)
    nrm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    mn, mx = np.ascontiguousarray(min_dist, np.float32).ravel(), np.ascontiguousarray(max_dist, np.float32).ravel()
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    vw = np.ascontiguousarray(view, np.float32).reshape(20)
    sc, sig = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(inv_level_sigma2, np.float32)
    if not (len(nrm) == len(mn) == len(mx) == len(d) == n_pts) or len(sc) != len(sig):
        raise ValueError("fuse_search: array lengths disagree")
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n_pts)
    bi, bd = np.full(n_pts, -2, np.int32), np.full(n_pts, -2, np.int32)
    _check(lib().ygzfe_fuse_search(kf.h, _p(vw), n_pts, _p(w), _p(nrm), _p(mn), _p(mx), _p(d),
                                   None if sk is None else _p(sk), float(th), _p(sc), _p(sig), len(sc),
                                   float(log_scale_factor), int(check_reproj), _p(bi), _p(bd)), "fuse_search")
    return bi, bd


class SparseImgAlign:
    """SparseImgAlign(n_levels, min_level, n_iter=10, method=GaussNewton) (SparseImageAlign.h:37-60)."""
    GaussNewton, LevenbergMarquardt = 0, 1  # NLLSSolver's methods (NLSSolver.h:40-43)

    def __init__(self, max_level, min_level, n_iter=10, method=0):
        self.max_level, self.min_level, self.method = max_level, min_level, int(method)

    def run(self, ref_frame, cur_frame, cam, kps, xyz_ref, usable, T_init):
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        xyz = np.ascontiguousarray(xyz_ref, np.float32).reshape(-1, 3)
        us = np.ascontiguousarray(usable, np.uint8)
        res = AlignResult()
        _check(lib().ygzfe_sparse_align_method(ref_frame.h, cur_frame.h, C.byref(cam), _p(kps), _p(xyz), _p(us),
                                               len(kps), self.max_level, self.min_level, C.byref(T_init),
                                               self.method, C.byref(res)),
               "sparse_align")
        return res


def align2d_batch(cur_frame, level, patches_with_border, patches, px, n_iter=10):
    pwb = np.ascontiguousarray(patches_with_border, np.uint8).reshape(-1, 100)
    p = np.ascontiguousarray(patches, np.uint8).reshape(-1, 64)
    px = np.ascontiguousarray(px, np.float32).reshape(-1, 2).copy()
    conv = np.zeros(len(px), np.uint8)
    _check(lib().ygzfe_align2d_batch(cur_frame.h, level, len(px), _p(pwb), _p(p), n_iter, _p(px), _p(conv)),
           "align2d_batch")
    return conv.astype(bool), px


def align2d_image(img, patch_with_border, patch, px, n_iter=10, device=0):
    """Align2D(const cv::Mat &cur_img, ...) (Align.cc:8-105) on a host image, whose rows may be
    `img.strides[0]` > width bytes apart -> (converged, px float32[2])."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img, np.uint8)
    pwb = np.ascontiguousarray(patch_with_border, np.uint8).reshape(100)
    p = np.ascontiguousarray(patch, np.uint8).reshape(64)
    px = np.array(px, np.float32).reshape(2)
    conv = np.zeros(1, np.uint8)
    _check(lib().ygzfe_align2d_image(device, _p(img), img.shape[1], img.shape[0], img.strides[0], _p(pwb), _p(p),
                                     n_iter, _p(px), _p(conv)), "align2d_image")
    return bool(conv[0]), px


def find_direct_projection_batch(ref_frames, cur_frame, cam, ref_index, kp_ref, pt_ref, T_cr, px):
    refs = (C.c_void_p * len(ref_frames))(*[f.h.value for f in ref_frames])
    ref_index = np.ascontiguousarray(ref_index, np.int32)
    kp_ref = np.ascontiguousarray(kp_ref, KP_DTYPE)
    pt_ref = np.ascontiguousarray(pt_ref, np.float32).reshape(-1, 3)
    T_cr = np.ascontiguousarray(T_cr, SE3_DTYPE)
    px = np.ascontiguousarray(px, np.float32).reshape(-1, 2).copy()
    n = len(px)
    lvl = np.zeros(n, np.int32)
    ok = np.zeros(n, np.uint8)
    _check(lib().ygzfe_find_direct_projection_batch(refs, cur_frame.h, C.byref(cam), n, _p(ref_index), _p(kp_ref),
                                                    _p(pt_ref), _p(T_cr), _p(px), _p(lvl), _p(ok)),
           "find_direct_projection_batch")
    return px, lvl, ok.astype(bool)


def stereo_matches(left_frame, right_frame, kl, dl, kr, dr, mb, mbf):
    """Frame::ComputeStereoMatches (Frame.cc:509-682) -> (mvuRight, mvDepth), float32[nl], -1 = none."""
    kl = np.ascontiguousarray(kl, KP_DTYPE)
    kr = np.ascontiguousarray(kr, KP_DTYPE)
    dl = np.ascontiguousarray(dl, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(dr, np.uint8).reshape(-1, 32)
    ur = np.zeros(len(kl), np.float32)
    dep = np.zeros(len(kl), np.float32)
    _check(lib().ygzfe_stereo_matches(left_frame.h, right_frame.h, _p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr),
                                      mb, mbf, _p(ur), _p(dep)), "stereo_matches")
    return ur, dep


def stereo_from_rgbd(im_depth, kps, mbf, device=0):
    """Frame::ComputeStereoFromRGBD (Frame.cc:684-700) -> (mvuRight, mvDepth)."""
    im = np.ascontiguousarray(im_depth, np.float32)
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    ur = np.zeros(len(kps), np.float32)
    dep = np.zeros(len(kps), np.float32)
    _check(lib().ygzfe_stereo_from_rgbd(device, _p(im), im.shape[1], im.shape[0], im.shape[1], _p(kps), len(kps), mbf,
                                        _p(ur), _p(dep)), "stereo_from_rgbd")
    return ur, dep


class Vocabulary(_Handle):
    """ORBVocabulary = TemplatedVocabulary<FORB::TDescriptor, FORB> (Thirdparty/DBoW2) in HBM."""
    _destroy = "ygzfe_vocab_destroy"

    def __init__(self, handle, device):
        self.h, self.device = handle, device
        v = [C.c_int() for _ in range(6)]
        _check(lib().ygzfe_vocab_info(self.h, *[C.byref(x) for x in v]), "vocab_info")
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = [x.value for x in v]

    @classmethod
    def from_arrays(cls, k, L, scoring, weighting, parent, is_leaf, desc, weight, device=0):
        parent = np.ascontiguousarray(parent, np.int32)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float64)
        return cls(_created("vocab_create", device, k, L, scoring, weighting, len(parent), _p(parent), _p(is_leaf),
                            _p(desc), _p(weight)), device)

    @classmethod
    def load_text(cls, path, device=0):
        """loadFromTextFile (TemplatedVocabulary.h:1362)."""
        return cls(_created("vocab_load_text", device, str(path).encode()), device)

    @classmethod
    def load_binary(cls, path, device=0):
        """loadFromBinaryFile (TemplatedVocabulary.h:1478)."""
        return cls(_created("vocab_load_binary", device, str(path).encode()), device)

    def transform_each(self, desc, levelsup=4):
        """transform(feature, word, weight, &nid, levelsup) per descriptor -> (word, weight, nid)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        w = np.zeros(n, np.int32)
        wt = np.zeros(n, np.float64)
        nid = np.zeros(n, np.int32)
        _check(lib().ygzfe_bow_transform(self.h, _p(d), n, levelsup, _p(w), _p(wt), _p(nid)), "bow_transform")
        return w, wt, nid

    def transform(self, desc, levelsup=4):
        """Frame::ComputeBoW -> (BowVector {word: value}, FeatureVector {node: [features]}), as
        (words int32[], values float64[]) and (nodes int32[], features int32[]) in map order."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        m = max(n, 1)
        bw, bv = np.zeros(m, np.int32), np.zeros(m, np.float64)
        fn, ff = np.zeros(m, np.int32), np.zeros(m, np.int32)
        nw, nf = C.c_int(), C.c_int()
        _check(lib().ygzfe_compute_bow(self.h, _p(d), n, levelsup, _p(bw), _p(bv), C.byref(nw), _p(fn), _p(ff),
                                       C.byref(nf)), "compute_bow")
        return (bw[:nw.value].copy(), bv[:nw.value].copy()), (fn[:nf.value].copy(), ff[:nf.value].copy())


def search_direct_batch(ref_frames, cur_frame, cam, item_ptr, ref_index, kp_ref, pt_ref, T_cr, px_proj, border=20.0):
    """Tracking::SearchLocalPointsDirect's per-point search (Tracking.cc:2337-2395), batched:
    point i tries items [item_ptr[i], item_ptr[i+1]) (its keyframes in SelectNearestKeyframe
    order) with FindDirectProjection from px_proj[i] and keeps the first converged pixel inside
    the border.  Returns (px_out float32[n,2], matched_item int32[n], -1 = no match)."""
    refs = (C.c_void_p * max(1, len(ref_frames)))(*[f.h.value for f in ref_frames])
    item_ptr = np.ascontiguousarray(item_ptr, np.int32)
    n = len(item_ptr) - 1
    ref_index = np.ascontiguousarray(ref_index, np.int32)
    kp_ref = np.ascontiguousarray(kp_ref, KP_DTYPE)
    pt_ref = np.ascontiguousarray(pt_ref, np.float32).reshape(-1, 3)
    T_cr = np.ascontiguousarray(T_cr, SE3_DTYPE)
    px_proj = np.ascontiguousarray(px_proj, np.float32).reshape(-1, 2)
    px_out = np.zeros((max(n, 0), 2), np.float32)
    matched = np.zeros(max(n, 0), np.int32)
    _check(lib().ygzfe_search_direct_batch(refs, len(ref_frames), cur_frame.h, C.byref(cam), n, _p(item_ptr),
                                           _p(ref_index), _p(kp_ref), _p(pt_ref), _p(T_cr), _p(px_proj), border,
                                           _p(px_out), _p(matched)), "search_direct_batch")
    return px_out, matched


DIRECT_FAILED, DIRECT_MATCHED, DIRECT_GRID_SKIP, DIRECT_NOT_RUN = 0, 1, 2, 3


def search_local_points_direct(ref_frames, cur_frame, cam, n_cache, item_ptr, ref_index, kp_ref, pt_ref, T_cr,
                               px_proj, border=20.0, grid_size=5, cache_hit_th=150):
    """Tracking::SearchLocalPointsDirect (Tracking.cc:2258-2410) whole: points [0, n_cache) are the
    cache (5-px coverage grid, replayed in order), the rest the local-map points (searched only
    when the cache gave <= cache_hit_th successes).  Returns (px_out float32[n,2], matched_item
    int32[n], status int32[n] (DIRECT_*), cache_success, local_ran)."""
    refs = (C.c_void_p * max(1, len(ref_frames)))(*[f.h.value for f in ref_frames])
    item_ptr = np.ascontiguousarray(item_ptr, np.int32)
    n = len(item_ptr) - 1
    ref_index = np.ascontiguousarray(ref_index, np.int32)
    kp_ref = np.ascontiguousarray(kp_ref, KP_DTYPE)
    pt_ref = np.ascontiguousarray(pt_ref, np.float32).reshape(-1, 3)
    T_cr = np.ascontiguousarray(T_cr, SE3_DTYPE)
    px_proj = np.ascontiguousarray(px_proj, np.float32).reshape(-1, 2)
    px_out = np.zeros((max(n, 0), 2), np.float32)
    matched = np.zeros(max(n, 0), np.int32)
    status = np.zeros(max(n, 0), np.int32)
    cs, lr = C.c_int(), C.c_int()
    _check(lib().ygzfe_search_local_points_direct(refs, len(ref_frames), cur_frame.h, C.byref(cam), int(n_cache),
                                                  n - int(n_cache), _p(item_ptr), _p(ref_index), _p(kp_ref),
                                                  _p(pt_ref), _p(T_cr), _p(px_proj), border, int(grid_size),
                                                  int(cache_hit_th), _p(px_out), _p(matched), _p(status),
                                                  C.byref(cs), C.byref(lr)), "search_local_points_direct")
    return px_out, matched, status, cs.value, bool(lr.value)


DIRECT_CULLED = 4
DIRECT_MAX_SEL = 8


class DirectView(C.Structure):
    """The current frame's side of Frame::isInFrustum: mRcw (row-major), mtcw, mOw, the image
    bounds, the viewing-cosine limit and mbf."""
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("Ow", C.c_float * 3), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("view_cos_limit", C.c_float),
                ("mbf", C.c_float)]

    @staticmethod
    def make(R, t, Ow, bounds, view_cos_limit=0.5, mbf=0.0):
        v = DirectView()
        v.R[:] = [float(x) for x in np.asarray(R, np.float32).reshape(9)]
        v.t[:] = [float(x) for x in np.asarray(t, np.float32).reshape(3)]
        v.Ow[:] = [float(x) for x in np.asarray(Ow, np.float32).reshape(3)]
        v.min_x, v.max_x, v.min_y, v.max_y = (float(np.float32(b)) for b in bounds)
        v.view_cos_limit, v.mbf = float(np.float32(view_cos_limit)), float(np.float32(mbf))
        return v


class _DirectKeyframes(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("ref", C.c_void_p), ("kf_id", C.c_void_p), ("kf_excluded", C.c_void_p),
                ("T_rw", C.c_void_p), ("T_cr", C.c_void_p)]


class _DirectCandidates(C.Structure):
    _fields_ = [("n_cache", C.c_int32), ("n_local", C.c_int32), ("world", C.c_void_p), ("normal", C.c_void_p),
                ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("skip", C.c_void_p), ("obs_ptr", C.c_void_p),
                ("obs_kf", C.c_void_p), ("obs_kp", C.c_void_p)]


class _DirectMapResult(C.Structure):
    _fields_ = [("status", C.c_void_p), ("px_out", C.c_void_p), ("matched_kf", C.c_void_p),
                ("matched_kp", C.c_void_p), ("proj", C.c_void_p), ("view_cos", C.c_void_p), ("dist", C.c_void_p)]


def search_local_map_direct(kf_frames, cur_frame, cam, view, kf_id, kf_excluded, T_rw, T_cr, n_cache, world, normal,
                            min_dist, max_dist, skip, obs_ptr, obs_kf, obs_kp, n_sel=5, border=20.0, grid_size=5,
                            cache_hit_th=150):
    """Tracking::SearchLocalPointsDirect from the raw local map (ygzfe_search_local_map_direct): the
    frustum cull, the choice of the n_sel keyframes of largest kf_id per point, T_ref * P_w, the item
    search and the replay all on the device.  kf_frames: the keyframe table's frames, each with
    set_keypoints() done; kf_id int64[n_kf], kf_excluded uint8[n_kf], T_rw float32[n_kf, 12] (R
    row-major, t), T_cr SE3_DTYPE[n_kf].  Candidates (the first n_cache are the cache): world /
    normal float32[n, 3], min_dist / max_dist float32[n], skip uint8[n], observations in CSR form
    (obs_kf a table row, obs_kp a keypoint index of that keyframe).  Returns a dict of the
    per-candidate arrays status (DIRECT_*), px_out, matched_kf, matched_kp, proj, view_cos, dist,
    and (cache_success, local_ran)."""
    n_kf = len(kf_frames)
    refs = (C.c_void_p * max(1, n_kf))(*[f.h.value for f in kf_frames])
    kf_id = np.ascontiguousarray(kf_id, np.int64)
    kf_excluded = np.ascontiguousarray(kf_excluded, np.uint8)
    T_rw = np.ascontiguousarray(T_rw, np.float32).reshape(-1, 12)
    T_cr = np.ascontiguousarray(T_cr, SE3_DTYPE)
    if not (len(kf_id) == len(kf_excluded) == len(T_rw) == len(T_cr) == n_kf):
        raise YgzfeError("search_local_map_direct: keyframe table arrays differ in length")
    world = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
    normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    min_dist = np.ascontiguousarray(min_dist, np.float32)
    max_dist = np.ascontiguousarray(max_dist, np.float32)
    skip = np.ascontiguousarray(skip, np.uint8)
    obs_ptr = np.ascontiguousarray(obs_ptr, np.int32)
    obs_kf = np.ascontiguousarray(obs_kf, np.int32)
    obs_kp = np.ascontiguousarray(obs_kp, np.int32)
    n = len(world)
    if not (len(normal) == len(min_dist) == len(max_dist) == len(skip) == n and len(obs_ptr) == n + 1
            and len(obs_kf) == len(obs_kp) and (n == 0 or len(obs_kf) >= obs_ptr.max())):
        raise YgzfeError("search_local_map_direct: candidate arrays differ in length")
    res = {"status": np.zeros(n, np.int32), "px_out": np.zeros((n, 2), np.float32),
           "matched_kf": np.full(n, -1, np.int32), "matched_kp": np.full(n, -1, np.int32),
           "proj": np.zeros((n, 3), np.float32), "view_cos": np.zeros(n, np.float32), "dist": np.zeros(n, np.float32)}
    kfs = _DirectKeyframes(n_kf, C.cast(refs, C.c_void_p), _p(kf_id), _p(kf_excluded), _p(T_rw), _p(T_cr))
    cand = _DirectCandidates(int(n_cache), n - int(n_cache), _p(world), _p(normal), _p(min_dist), _p(max_dist),
                             _p(skip), _p(obs_ptr), _p(obs_kf), _p(obs_kp))
    out = _DirectMapResult(*[_p(res[k]) for k in ("status", "px_out", "matched_kf", "matched_kp", "proj", "view_cos",
                                                   "dist")])
    cs, lr = C.c_int(), C.c_int()
    _check(lib().ygzfe_search_local_map_direct(cur_frame.h, C.byref(cam), C.byref(view), C.byref(kfs), C.byref(cand),
                                               int(n_sel), border, int(grid_size), int(cache_hit_th), C.byref(out),
                                               C.byref(cs), C.byref(lr)), "search_local_map_direct")
    return res, cs.value, bool(lr.value)


class Batch(_Handle):
    """Frames resident in HBM, one launch per stage (the bench / multi-GPU path)."""
    _destroy = "ygzfe_batch_destroy"

    def __init__(self, params_or_extractor_args, device, width, height, max_frames):
        p = params_or_extractor_args
        if not isinstance(p, OrbParams):
            p = OrbParams(*p)
        self.params = p
        self.device, self.width, self.height, self.max_frames = device, width, height, max_frames
        self.h = _created("batch_create", C.byref(p), device, width, height, max_frames)
        pitch, cap, nl = C.c_size_t(), C.c_int(), C.c_int()
        _check(lib().ygzfe_batch_info(self.h, C.byref(pitch), C.byref(cap), C.byref(nl)), "batch_info")
        self.frame_pitch, self.kp_cap, self.nlevels = pitch.value, cap.value, nl.value

    @property
    def stream(self):
        return lib().ygzfe_batch_stream(self.h)

    def frames_ptr(self):
        """Device pointer of the pyramid slots (frame i level 0 at + i * frame_pitch)."""
        p = C.c_void_p()
        _check(lib().ygzfe_batch_frames(self.h, C.byref(p)), "batch_frames")
        return p.value

    def upload(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        _check(lib().ygzfe_batch_upload(self.h, _p(frames), len(frames)), "batch_upload")

    def upload_undistorted(self, und, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        _check(lib().ygzfe_batch_upload_undistorted(self.h, und.h, _p(frames), len(frames)), "upload_undistorted")

    def undistort_device(self, und, d_raw, raw_pitch, n_frames, stream=None):
        _check(lib().ygzfe_batch_undistort_device(self.h, und.h, d_raw, raw_pitch, n_frames, stream), "batch_undistort")

    def bind(self, pyramids=0, kps=0, desc=0, counts=0):
        _check(lib().ygzfe_batch_bind_buffers(self.h, pyramids or None, kps or None, desc or None, counts or None),
               "bind")

    def extract(self, n_frames, stream=None):
        _check(lib().ygzfe_batch_extract(self.h, n_frames, stream), "batch_extract")

    def extract_split(self, n_frames, kp_stream, desc_stream):
        _check(lib().ygzfe_batch_extract_split(self.h, n_frames, kp_stream, desc_stream), "batch_extract_split")

    def check(self):
        _check(lib().ygzfe_batch_check(self.h), "batch_check")

    def result(self, i):
        kps = np.zeros(self.kp_cap, KP_DTYPE)
        desc = np.zeros((self.kp_cap, 32), np.uint8)
        n = C.c_int()
        _check(lib().ygzfe_batch_result(self.h, i, _p(kps), self.kp_cap, _p(desc), C.byref(n)), "batch_result")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def level_size(self, level):
        w, h, st = C.c_int(), C.c_int(), C.c_int()
        _check(lib().ygzfe_batch_level(self.h, 0, level, None, C.byref(w), C.byref(h), C.byref(st)), "batch_level")
        return w.value, h.value

    def stats(self, n_frames):
        """Per-level totals over frames [0, n) of the last extract: (FAST candidates, octree keypoints)."""
        cand = np.zeros(self.nlevels, np.int64)
        sel = np.zeros(self.nlevels, np.int64)
        _check(lib().ygzfe_batch_stats(self.h, n_frames, _p(cand), _p(sel)), "batch_stats")
        return cand, sel

    def read_level(self, i, level, blurred=False):
        """Host copy of pyramid level `level` of frame i (or its 7x7 blurred copy)."""
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        _check(lib().ygzfe_batch_read_level(self.h, i, level, int(bool(blurred)), _p(out), w), "batch_read_level")
        return out

    def match(self, n_pairs, d_qframe, d_tframe, d_bi, d_bd, d_sd, stream=None):
        _check(lib().ygzfe_batch_match(self.h, n_pairs, d_qframe, d_tframe, d_bi, d_bd, d_sd, stream), "batch_match")

    def sparse_align(self, n_pairs, d_ref_idx, d_cur_idx, d_xyz, d_usable, cam, max_level, min_level, d_T_init,
                     d_out, stream=None):
        _check(lib().ygzfe_batch_sparse_align(self.h, n_pairs, d_ref_idx, d_cur_idx, d_xyz, d_usable, C.byref(cam),
                                              max_level, min_level, d_T_init, d_out, stream), "batch_sparse_align")

    def stereo(self, n_pairs, d_left_idx, d_right_idx, mb, mbf, d_u_right, d_depth, stream=None):
        _check(lib().ygzfe_batch_stereo(self.h, n_pairs, d_left_idx, d_right_idx, mb, mbf, d_u_right, d_depth, stream),
               "batch_stereo")

    def stereo_rgbd(self, n_frames, d_depth_images, depth_pitch, stride, mbf, d_u_right, d_depth, stream=None):
        _check(lib().ygzfe_batch_stereo_rgbd(self.h, n_frames, d_depth_images, depth_pitch, stride, mbf, d_u_right,
                                             d_depth, stream), "batch_stereo_rgbd")

    def compute_bow(self, vocab, n_frames, levelsup, d_bow_words, d_bow_values, d_n_words, d_fv_nodes, d_fv_feats,
                    d_n_fv, stream=None):
        _check(lib().ygzfe_batch_compute_bow(self.h, vocab.h, n_frames, levelsup, d_bow_words, d_bow_values, d_n_words,
                                             d_fv_nodes, d_fv_feats, d_n_fv, stream), "batch_compute_bow")

    def pack_slots(self, frame_begin, n_frames, d_align, global_first, d_slots, slot_pitch, stream=None):
        """Device-side packing of the offline sequence mode's per-frame result slots
        (ygzfe_batch_pack_slots; layout in include/ygzfe.h and ygzfe.dist)."""
        _check(lib().ygzfe_batch_pack_slots(self.h, frame_begin, n_frames, d_align or None, global_first, d_slots,
                                            slot_pitch, stream), "batch_pack_slots")

    def timing(self, enable=True):
        ms = (C.c_float * 16)()
        names = (C.c_char_p * 16)()
        n = lib().ygzfe_batch_timing(self.h, int(enable), ms, names, 16)
        return {names[i].decode(): ms[i] for i in range(n)}


# ---------------------------------------------------------------- synthetic inputs (tests / bench)
_synth = None


def synth():
    global _synth
    if _synth is None:
        _synth = _load(SYNTH_PATH, "ygzs_", _abi.SYNTH)
    return _synth


def synth_texture(seed, W, H):
    out = np.zeros((H, W), np.uint8)
    synth().ygzs_texture(seed, W, H, _p(out))
    return out


EUROC_CAM = (458.654, 457.296, 367.215, 248.375)


def trajectory_pose(k, xi):
    q = np.zeros(4, np.float32)
    t = np.zeros(3, np.float32)
    xi = np.ascontiguousarray(xi, np.float32)
    synth().ygzs_trajectory_pose(k, _p(xi), _p(q), _p(t))
    return q, t


def render_plane(tex, texel, plane_z, cam, q_cw, t_cw, W, H, noise_seed=0, noise_amp=2):
    tex = np.ascontiguousarray(tex, np.uint8)
    out = np.zeros((H, W), np.uint8)
    camv = np.array(cam, np.float32)
    synth().ygzs_render_plane(_p(tex), tex.shape[1], tex.shape[0], texel, plane_z, _p(camv),
                              _p(np.ascontiguousarray(q_cw, np.float32)), _p(np.ascontiguousarray(t_cw, np.float32)),
                              W, H, noise_seed, noise_amp, _p(out))
    return out


def backproject_plane(cam, q_cw, t_cw, uv, plane_z):
    camv = np.array(cam, np.float32)
    q = np.ascontiguousarray(q_cw, np.float32)
    t = np.ascontiguousarray(t_cw, np.float32)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    out = np.zeros((len(uv), 3), np.float32)
    ok = np.zeros(len(uv), np.uint8)
    P = np.zeros(3, np.float32)
    for i, (u, v) in enumerate(uv):
        ok[i] = synth().ygzs_backproject_plane(_p(camv), _p(q), _p(t), u, v, plane_z, _p(P))
        out[i] = P
    return out, ok


_synth_hip = None


def _synth_hip_lib():
    global _synth_hip
    if _synth_hip is None:
        lib()  # torch's HIP runtime first (see lib())
        _synth_hip = _load(SYNTH_HIP_PATH, "ygzs_", _abi.SYNTH_HIP)
    return _synth_hip


def render_plane_device(d_tex, tex_w, tex_h, texel, plane_z, cam, d_q, d_t, d_seeds, n_frames, W, H, d_out, pitch,
                        noise_amp=2, stream=None):
    """The synthetic plane sequence rendered on the device (synth/plane_points.hip):
    frame i (pose d_q[i], d_t[i], noise seed d_seeds[i]) -> d_out + i * pitch."""
    c = (C.c_float * 4)(*[float(v) for v in cam])
    rc = _synth_hip_lib().ygzs_render_plane_device(d_tex, tex_w, tex_h, texel, plane_z, c, d_q, d_t, d_seeds, n_frames,
                                                   W, H, noise_amp, d_out, pitch, stream)
    if rc != 0:
        raise YgzfeError("render_plane_device launch failed")


def plane_points_device(d_kps, cap, n_frames, cam, d_r3, d_cz, plane_z, d_xyz, stream=None):
    """Synthetic map points for bench.py: back-project every keypoint of frame i
    onto the plane Z_w = plane_z (one fused HIP pass; synth/plane_points.hip)."""
    c = (C.c_float * 4)(*[float(v) for v in cam])
    rc = _synth_hip_lib().ygzs_plane_points(d_kps, KP_DTYPE.itemsize // 4, cap, n_frames, c, d_r3, d_cz, plane_z, d_xyz,
                                            stream)
    if rc != 0:
        raise YgzfeError("plane_points launch failed")


# ------------------------------------------------------------------ pose-only optimisation
class PoseOptResult(C.Structure):
    """ygzfe_pose_opt_result (Optimizer::PoseOptimization, Optimizer.cc:1656-1842)."""
    _fields_ = [("T_cw", SE3), ("q", C.c_double * 4), ("t", C.c_double * 3), ("n_corr", C.c_int32),
                ("n_inliers", C.c_int32), ("rounds", C.c_int32), ("iters", C.c_int32 * 4),
                ("rejected", C.c_int32 * 4), ("chi2", C.c_double * 4)]


POSE_OPT_RESULT_DTYPE = np.dtype({"names": ["Tq", "Tt", "q", "t", "n_corr", "n_inliers", "rounds", "iters", "rejected",
                                            "chi2"],
                                  "formats": [("<f4", 4), ("<f4", 3), ("<f8", 4), ("<f8", 3), "<i4", "<i4", "<i4",
                                              ("<i4", 4), ("<i4", 4), ("<f8", 4)],
                                  "offsets": [0, 16, 32, 64, 88, 92, 96, 100, 116, 136], "itemsize": 168})


def pose_optimization(cam, bf, T_cw_init, kps, xw, present, inv_level_sigma2, u_right=None, outlier=None, device=0):
    """Optimizer::PoseOptimization(Frame*) on the device.  kps: KP_DTYPE rows (mvKeys), xw [n,3] world
    points, present [n] (mvpMapPoints[i] != NULL), u_right: mvuRight or None (all mono), outlier: the
    caller's mvbOutlier (rows without a map point keep their value; default zeros).
    -> (PoseOptResult, outlier uint8 [n])."""
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    n = len(kps)
    xw = np.ascontiguousarray(xw, np.float32).reshape(n, 3)
    pr = np.ascontiguousarray(present, np.uint8)
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    out = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8)
    if len(pr) != n or len(out) != n or (ur is not None and len(ur) != n):
        raise YgzfeError("pose_optimization: array lengths differ")
    res = PoseOptResult()
    _check(lib().ygzfe_pose_optimization(device, C.byref(cam), bf, C.byref(T_cw_init), n, _p(kps),
                                         None if ur is None else _p(ur), _p(xw), _p(pr), _p(sig), len(sig), _p(out),
                                         C.byref(res)), "pose_optimization")
    return res, out


def pose_optimization_batch(problem_ptr, cam, bf, T_init, kps, u_right, xw, present, inv_level_sigma2, outlier,
                            results=None, device=0):
    """Many PoseOptimization problems in one launch on torch.cuda.current_stream(); every argument is a
    torch device tensor (u_right may be None) and nothing synchronises.  problem_ptr: int32 [P+1] CSR
    over the edge rows; cam: float32 [P,4]; bf: float32 [P]; T_init: float32 [P,7] (q xyzw, t); kps: uint8
    [n,28] (KP_DTYPE bytes); xw: float32 [n,3]; present, outlier: uint8 [n]; inv_level_sigma2: float32
    [n_levels].  outlier is written in place; -> results, uint8 [P, 168] (view with POSE_OPT_RESULT_DTYPE)."""
    import torch
    P = int(problem_ptr.numel()) - 1
    tensors = [problem_ptr, cam, bf, T_init, kps, xw, present, inv_level_sigma2, outlier] + \
        ([] if u_right is None else [u_right])
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous():
            raise YgzfeError("pose_optimization_batch takes contiguous device tensors")
    want = [(problem_ptr, torch.int32), (cam, torch.float32), (bf, torch.float32), (T_init, torch.float32),
            (kps, torch.uint8), (xw, torch.float32), (present, torch.uint8), (inv_level_sigma2, torch.float32),
            (outlier, torch.uint8)] + ([] if u_right is None else [(u_right, torch.float32)])
    if any(t.dtype != d for t, d in want):
        raise YgzfeError("pose_optimization_batch: wrong tensor dtype")
    n = int(present.numel())
    if (P < 0 or cam.numel() != 4 * P or bf.numel() != P or T_init.numel() != 7 * P or kps.numel() != 28 * n or
            xw.numel() != 3 * n or outlier.numel() != n or (u_right is not None and u_right.numel() != n)):
        raise YgzfeError("pose_optimization_batch: tensor shapes differ")
    if results is None:
        results = torch.zeros((max(P, 0), POSE_OPT_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=present.device)
    elif results.numel() != P * POSE_OPT_RESULT_DTYPE.itemsize or results.dtype != torch.uint8:
        raise YgzfeError("pose_optimization_batch: results must be uint8 [P, 168]")
    vp = torch.Tensor.data_ptr
    stream = torch.cuda.current_stream(present.device).cuda_stream
    _check(lib().ygzfe_pose_optimization_batch(device, P, vp(problem_ptr), vp(cam), vp(bf), vp(T_init), vp(kps),
                                               None if u_right is None else vp(u_right), vp(xw), vp(present),
                                               vp(inv_level_sigma2), int(inv_level_sigma2.numel()), vp(outlier),
                                               vp(results), stream), "pose_optimization_batch")
    return results
