"""FindDirectProjection / Align2D inputs under real viewpoint change, and an independent
restatement of the warp (GetWarpAffineMatrix, GetBestSearchLevel, WarpAffine) in numpy.

Views.  The keyframe K0 sits at PlaneScene's identity pose (fronto-parallel, plane depth
PLANE_Z everywhere); K1 is K0 rolled 90 deg about the optical axis.  The current frames are
PlaneScene.render from poses with a real warp, `s` = keyframe depth / current depth:

    zoom<s>     s in ZOOMS[cfg]: D = s^2 * scale[octave]^2 climbs the search levels
    cap         s = 16: D is still above 3 at the top level
    zoomout     s = 0.4: D < 1, the patch's footprint in the reference level is ~25 px
    roll30/90/180, roll90zoom (90 deg and s = 1.9): large off-diagonals in A
    oblique     35 deg yaw, anisotropic A

A = d(current level-0 px) / d(reference level-`octave` px), so D = det A carries
scale[octave]^2 on top of s^2: with the x2.0 pyramid the search level at the identity already
equals the octave (the scenes of _scenes.direct_scene reach it that way, always with A ~ scale * I).
Octaves are drawn from [0, nlevels - 1 - level(s^2)] so that, outside `cap`, the search level is
the level GetBestSearchLevel wants and not the cap (`cap` draws from all octaves).

Shrunk parameters (the texture is 13.3 m x 10 m around the optical axis of K0): the oblique
camera looks at the plane point in front of K0 from 2 m, not from PLANE_Z = 3 m, because at
3 m the far image edge (74 deg off the plane normal) leaves the texture.  Every other view
renders whole; test_cpu_direct_views.py asserts it (view_in_texture).

Two pyramid configurations: CONFIGS["sf20"] = 752x480, x2.0, 4 levels and CONFIGS["sf12"] =
641x479, x1.2, 8 levels (odd level widths).

Reference keypoints: a jittered grid in keyframe pixels over what the current frame sees of
the keyframe, out to KF_MARGIN px beyond the keyframe's own edges (patches partly and wholly
outside the level), a random octave each.  pt_ref = the plane point in the keyframe's frame,
T_cr from the poses, px0 = the true projection + U(-1.5, 1.5) px * scale[expected level].
True projections stay inside the current frame (CUR_MARGIN = 0): with a 30 px margin beyond it the
items that can never converge took the oracle's own end-to-end convergence on the x1.2 roll views
to 0.45 .. 0.51 of the fully-inside items, at the 0.5 the test asks; inside the frame it is 0.53 ..
0.90 on every view (the x1.2 pyramid converges least: its patches come from levels up to 1.73 x
blurrier than the search level).  Guesses still leave the frame through px0's noise.

The restatement follows ORBmatcher.cc:1525-1602, ORBmatcher.h:226-252 and Frame.h:170-191 (not
oracle/align.c): warp_matrix and best_search_level in float64; warp_patch takes the sample
positions in float32, the type the reference computes them in (Matrix2f / Vector2f: a float64
position moves a sample by ~1e-4 px and a byte with it), the bilinear weights in double and
the uchar cast truncating.  `mut` names a deliberate mistake (MUTATIONS) for the mutation
tests of test_cpu_direct_views.py.
"""
import ctypes as C
import functools

import numpy as np

import _oracle as O
import _scenes as S
import ygzfe

CONFIGS = {"sf20": (752, 480, 2.0, 4), "sf12": (641, 479, 1.2, 8)}
SCENE_SEED = 11
KF_MARGIN = 40      # px beyond the keyframe's edges that reference keypoints reach
CUR_MARGIN = 0      # true projections stay inside the current frame; px0's noise still takes guesses out of it
N_TARGET = 260
# sf20: D = s^2 gives levels 0, 1, 1, 2, 3 at octave 0; sf12 (D / 1.44 per level): 0, 1, 2, 3, 4, 5, 6, 7
ZOOMS = {"sf20": (1.5, 1.9, 2.5, 4.0, 8.0), "sf12": (1.5, 1.9, 2.2, 2.7, 3.3, 4.0, 5.0, 6.0)}
MUTATIONS = ("transpose_A", "swap_R_offdiag", "no_search_scale", "level_from_octave")

# Worst |A_oracle - warp_matrix| over every item of every view of both configurations (float32
# against float64 evaluation of the same expressions; measured by
# test_cpu_direct_views.py::test_oracle_A_against_float64, which prints it) and the tolerance
# derived from it: 4 x floor, the convention of _pose_opt.py.
A_FLOOR = 2.3e-4   # the cap views (|A| ~ 128); 2e-5 .. 6e-5 on the views with |A| ~ 1
A_TOL = 4 * A_FLOOR


def view_names(cfg):
    return [f"zoom{s:g}" for s in ZOOMS[cfg]] + ["cap", "zoomout", "roll30", "roll90", "roll180", "roll90zoom",
                                                  "oblique"]


def _zoom_of(name):
    if name.startswith("zoom") and name != "zoomout":
        return float(name[4:])
    return {"cap": 16.0, "zoomout": 0.4, "roll90zoom": 1.9}.get(name, 1.0)


def _stable_seed(*parts):
    h = 2166136261
    for ch in "/".join(str(p) for p in parts).encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def view_pose(cfg, name):
    """T_cw of the current frame (float64 quaternion xyzw, translation); world = K0's frame."""
    rng = np.random.default_rng(_stable_seed("pose", cfg, name))
    jit = S.quat_from_rotvec(rng.uniform(-0.01, 0.01, 3))
    tj = np.append(rng.uniform(-0.02, 0.02, 2), 0.0)
    s = _zoom_of(name)
    if name == "oblique":
        q = S.quat_mul(jit, S.quat_from_rotvec([0.0, np.deg2rad(35.0), 0.0]))
        qi, _ = S.se3_inv(q, np.zeros(3))
        centre = np.array([0.0, 0.0, S.PLANE_Z]) - 2.0 * S.quat_rot(qi, np.array([0.0, 0.0, 1.0]))
        return q, -S.quat_rot(q, centre) + tj
    roll = {"roll30": 30.0, "roll90": 90.0, "roll180": 180.0, "roll90zoom": 90.0}.get(name, 0.0)
    q = S.quat_mul(jit, S.quat_from_rotvec([0.0, 0.0, np.deg2rad(roll)]))
    return q, tj + np.array([0.0, 0.0, -(S.PLANE_Z - S.PLANE_Z / s)])


KF_POSES = ((np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)),                     # K0
            (S.quat_from_rotvec([0.0, 0.0, np.pi / 2]), np.zeros(3)))           # K1: rolled 90 deg


def pyramid_scales(cfg):
    """mvScaleFactors, mvInvScaleFactors, mvInvLevelSigma2 (ORBextractor.cc:412-427), float32."""
    _, _, sf, nl = CONFIGS[cfg]
    scale = np.ones(nl, np.float32)
    for i in range(1, nl):
        scale[i] = scale[i - 1] * np.float32(sf)
    sigma2 = scale * scale
    return scale, np.float32(1.0) / scale, np.float32(1.0) / sigma2


@functools.lru_cache(maxsize=None)
def _scene(cfg):
    W, H, _, _ = CONFIGS[cfg]
    return S.PlaneScene(SCENE_SEED, W, H)


def cam32(cfg):
    """The intrinsics as the float32 values the C structs hold, in float64."""
    return np.array(_scene(cfg).cam, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def keyframe_image(cfg, k):
    q, t = KF_POSES[k]
    img = _scene(cfg).render(q.astype(np.float32), t.astype(np.float32), 100 + k)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def current_image(cfg, name):
    q, t = view_pose(cfg, name)
    img = _scene(cfg).render(q.astype(np.float32), t.astype(np.float32), _stable_seed("noise", name) % 1000)
    img.setflags(write=False)
    return img


def view_in_texture(cfg, name):
    """Whether every corner ray of the current frame meets the plane inside the texture."""
    W, H, _, _ = CONFIGS[cfg]
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
    P = S.backproject_plane_np(cam32(cfg), view_pose(cfg, name), corners)
    tx, ty = P[:, 0] / S.TEXEL + S.TEX_W * 0.5, P[:, 1] / S.TEXEL + S.TEX_H * 0.5
    return bool((tx >= 0).all() and (ty >= 0).all() and (tx < S.TEX_W - 1).all() and (ty < S.TEX_H - 1).all())


def _outline(W, H, m, k=12):
    xs, ys = np.linspace(-m, W + m, k), np.linspace(-m, H + m, k)
    return np.concatenate([np.stack([xs, np.full(k, -m)], 1), np.stack([xs, np.full(k, H + m)], 1),
                           np.stack([np.full(k, -m), ys], 1), np.stack([np.full(k, W + m), ys], 1)])


def expected_level_of_zoom(cfg, s):
    _, _, _, nl = CONFIGS[cfg]
    inv_s2 = float(pyramid_scales(cfg)[2][1])
    D, lvl = s * s, 0
    while D > 3.0 and lvl < nl - 1:
        lvl, D = lvl + 1, D * inv_s2
    return lvl


@functools.lru_cache(maxsize=None)
def view_items(cfg, name, k=0):
    """The items of one view against keyframe k: dict of kps (ygzfe.KP_DTYPE), pt_ref f32[n, 3],
    T_cr (ygzfe.SE3_DTYPE), px0 f32[n, 2], px_true f64[n, 2], ref_index i32[n] (all k)."""
    W, H, sf, nl = CONFIGS[cfg]
    cam = cam32(cfg)
    scale = pyramid_scales(cfg)[0]
    rng = np.random.default_rng(_stable_seed("items", cfg, name, k))
    kf, cur = KF_POSES[k], view_pose(cfg, name)
    # what the current frame (and CUR_MARGIN around it) sees, in keyframe pixels
    Pw = S.backproject_plane_np(cam, cur, _outline(W, H, CUR_MARGIN))
    uvk, _ = S.project(cam, kf[0], kf[1], Pw)
    lo = np.maximum(uvk.min(0), [-KF_MARGIN, -KF_MARGIN])
    hi = np.minimum(uvk.max(0), [W + KF_MARGIN, H + KF_MARGIN])
    step = float(np.sqrt(np.prod(hi - lo) / N_TARGET))
    gx, gy = np.meshgrid(np.arange(lo[0] + step / 2, hi[0], step), np.arange(lo[1] + step / 2, hi[1], step))
    uv = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.3 * step, 0.3 * step, (gx.size, 2))
    uv = uv.astype(np.float32).astype(np.float64)          # the keypoint as the reference holds it
    Pw = S.backproject_plane_np(cam, kf, uv)
    px_true, Pc = S.project(cam, cur[0], cur[1], Pw)
    keep = ((Pc[:, 2] > 0) & (px_true[:, 0] > -CUR_MARGIN) & (px_true[:, 0] < W + CUR_MARGIN) &
            (px_true[:, 1] > -CUR_MARGIN) & (px_true[:, 1] < H + CUR_MARGIN))
    uv, Pw, px_true = uv[keep], Pw[keep], px_true[keep]
    if len(uv) > 300:
        sel = np.sort(rng.permutation(len(uv))[:300])
        uv, Pw, px_true = uv[sel], Pw[sel], px_true[sel]
    n = len(uv)
    top = nl - 1 if name == "cap" else nl - 1 - expected_level_of_zoom(cfg, _zoom_of(name))
    kps = np.zeros(n, ygzfe.KP_DTYPE)
    kps["x"], kps["y"] = uv[:, 0], uv[:, 1]
    kps["octave"] = rng.integers(0, top + 1, n)
    kps["size"] = 31.0 * scale[kps["octave"]]
    kps["angle"] = -1.0
    pt_ref = np.array([S.quat_rot(kf[0], p) + kf[1] for p in Pw], np.float32)
    qi, ti = S.se3_inv(*kf)
    qcr, tcr = S.se3_mul(cur[0], cur[1], qi, ti)
    T_cr = np.zeros(n, ygzfe.SE3_DTYPE)
    T_cr["q"], T_cr["t"] = qcr, tcr
    A = warp_matrix(cam, T_cr["q"][0], T_cr["t"][0], pt_ref, uv, scale[kps["octave"]])
    sl = best_search_level(A, nl - 1, pyramid_scales(cfg)[2][1])
    px0 = (px_true + rng.uniform(-1.5, 1.5, (n, 2)) * scale[sl][:, None].astype(np.float64)).astype(np.float32)
    return {"cfg": cfg, "view": name, "kps": kps, "pt_ref": pt_ref, "T_cr": T_cr, "px0": px0, "px_true": px_true,
            "ref_index": np.full(n, k, np.int32)}


# ------------------------------------------------------------------ the restatement
def _qrot(q, v):
    """Eigen QuaternionBase::_transformVector on rows of v, float64."""
    q = np.asarray(q, np.float64)
    uv = 2.0 * np.cross(q[:3], v)
    return v + q[3] * uv + np.cross(q[:3], uv)


def warp_matrix(cam, q_cr, t_cr, pt_ref, px_ref, level_scale, mut=()):
    """GetWarpAffineMatrix (ORBmatcher.cc:1525-1547) for n items at once -> A[n, 2, 2], float64.
    pt_ref[n, 3], px_ref[n, 2], level_scale[n] = mvScaleFactors[octave]."""
    fx, fy, cx, cy = (float(c) for c in cam)
    pt_ref = np.asarray(pt_ref, np.float64).reshape(-1, 3)
    px_ref = np.asarray(px_ref, np.float64).reshape(-1, 2)
    ls = np.asarray(level_scale, np.float64).reshape(-1)
    depth = pt_ref[:, 2]
    half = 4.0  # WarpHalfPatchSize

    def pixel2camera(px):  # Frame.h:185-191, depth that of pt_ref
        return np.stack([(px[:, 0] - cx) * depth / fx, (px[:, 1] - cy) * depth / fy, depth], 1)

    def world2pixel(p):    # Frame.h:170-183 with T_c_w = TCR
        c = _qrot(q_cr, p) + np.asarray(t_cr, np.float64)
        return np.stack([fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy], 1)

    du = pixel2camera(px_ref + np.stack([half * ls, 0 * ls], 1))
    dv = pixel2camera(px_ref + np.stack([0 * ls, half * ls], 1))
    pc, pu, pv = world2pixel(pt_ref), world2pixel(du), world2pixel(dv)
    A = np.zeros((len(pt_ref), 2, 2))
    A[:, :, 0] = (pu - pc) / half   # ACR.col(0)
    A[:, :, 1] = (pv - pc) / half   # ACR.col(1)
    if "transpose_A" in mut:
        A = A.transpose(0, 2, 1).copy()
    return A


def search_level_D(A, max_level, inv_sigma2_1):
    """The determinants GetBestSearchLevel compares with 3.0: D[n, max_level + 1], D[:, k] = det A *
    inv_sigma2_1^k in float32 steps as the reference multiplies them."""
    A = np.asarray(A)
    D = (A[:, 0, 0] * A[:, 1, 1] - A[:, 1, 0] * A[:, 0, 1]).astype(np.float32)
    out = [D]
    for _ in range(max_level):
        out.append(out[-1] * np.float32(inv_sigma2_1))
    return np.stack(out, 1)


def best_search_level(A, max_level, inv_sigma2_1, mut=(), octave=None):
    """GetBestSearchLevel (ORBmatcher.h:226-238) on A[n, 2, 2] -> int level per item."""
    if "level_from_octave" in mut:
        return np.asarray(octave).astype(np.int64)
    A = np.asarray(A, np.float64)
    D = A[:, 0, 0] * A[:, 1, 1] - A[:, 1, 0] * A[:, 0, 1]
    lvl = np.zeros(len(A), np.int64)
    for _ in range(max_level):
        go = (D > 3.0) & (lvl < max_level)
        lvl += go
        D = np.where(go, D * float(inv_sigma2_1), D)
    return lvl


def warp_patch(A, img, px_ref, scale_ref, scale_search, half_patch=5, mut=()):
    """WarpAffine (ORBmatcher.cc:1549-1571) + GetBilateralInterpUchar (ORBmatcher.h:241-252) of one item:
    A float32[2, 2] -> (patch uint8[2 hp, 2 hp], the float64 samples, the mask of samples outside)."""
    f32 = np.float32
    A = np.asarray(A, f32)
    det = A[0, 0] * A[1, 1] - A[1, 0] * A[0, 1]           # Eigen 2x2 inverse: cofactors * (1 / det)
    inv = f32(1.0) / det
    R00, R01, R10, R11 = A[1, 1] * inv, -A[0, 1] * inv, -A[1, 0] * inv, A[0, 0] * inv
    if "swap_R_offdiag" in mut:
        R01, R10 = R10, R01
    pr = np.asarray(px_ref, f32) / f32(scale_ref)        # px_ref_pyr
    g = np.arange(2 * half_patch) - half_patch
    ppx, ppy = np.meshgrid(g.astype(f32), g.astype(f32))    # px_patch(x - hp, y - hp), rows = y
    if "no_search_scale" not in mut:
        ppx, ppy = ppx * f32(scale_search), ppy * f32(scale_search)
    qx = (R00 * ppx + R01 * ppy) + pr[0]
    qy = (R10 * ppx + R11 * ppy) + pr[1]
    assert qx.dtype == f32 and qy.dtype == f32
    h, w = img.shape
    outside = (qx < 0) | (qy < 0) | (qx >= w - 1) | (qy >= h - 1) | ~np.isfinite(qx) | ~np.isfinite(qy)
    X, Y = np.where(outside, 0.0, qx.astype(np.float64)), np.where(outside, 0.0, qy.astype(np.float64))
    xx, yy = X - np.floor(X), Y - np.floor(Y)
    ix, iy = X.astype(np.int64), Y.astype(np.int64)
    im = img.astype(np.float64)
    val = ((1 - xx) * (1 - yy) * im[iy, ix] + xx * (1 - yy) * im[iy, ix + 1] + (1 - xx) * yy * im[iy + 1, ix] +
           xx * yy * im[iy + 1, ix + 1])
    val = np.where(outside, 0.0, val)
    return val.astype(np.uint8), val, outside        # float64 -> uint8 truncates


# ------------------------------------------------------------------ the oracle, item by item
class OracleView:
    """The oracle's pyramids and level tables of one configuration, as ctypes arrays."""

    def __init__(self, cfg):
        W, H, sf, nl = CONFIGS[cfg]
        self.cfg, self.nl = cfg, nl
        self.orc = O.OrbOracle(1000, sf, nl, 20, 7)
        self.scale, self.inv_scale, self.inv_sigma2 = self.orc.scale, self.orc.inv_scale, self.orc.inv_sigma2
        self.sc = (C.c_float * 16)(*self.scale.tolist())
        self.isc = (C.c_float * 16)(*self.inv_scale.tolist())
        self.cam = O.Cam(*_scene(cfg).cam)
        self._pyr = {}

    def pyramid(self, key, img=None):
        """Pyramid of keyframe k (key = int), of a view's current frame (key = name) or of `img`."""
        if key not in self._pyr:
            if img is None:
                img = keyframe_image(self.cfg, key) if isinstance(key, int) else current_image(self.cfg, key)
            self._pyr[key] = self.orc.pyramid(img)
        return self._pyr[key]

    @staticmethod
    def _ptrs(levels):
        return ((C.c_void_p * 16)(*[l.ctypes.data for l in levels]), (C.c_int * 16)(*[l.shape[1] for l in levels]),
                (C.c_int * 16)(*[l.shape[0] for l in levels]))

    def warp_matrices(self, it):
        """ygzo_warp_affine_matrix per item -> A float32[n, 2, 2] (rows of the matrix)."""
        n = len(it["kps"])
        A = np.zeros((n, 4), np.float32)
        for i in range(n):
            T = O.se3_from(it["T_cr"]["q"][i], it["T_cr"]["t"][i])
            kp = it["kps"][i]
            O.lib().ygzo_warp_affine_matrix(C.byref(self.cam), C.byref(T), O._p(it["pt_ref"][i]), C.c_float(kp["x"]),
                                            C.c_float(kp["y"]), C.c_float(self.scale[kp["octave"]]), O._p(A[i]))
        return A.reshape(n, 2, 2)

    def search_levels(self, A):
        return np.array([O.lib().ygzo_best_search_level(O._p(np.ascontiguousarray(a, np.float32)), self.nl - 1,
                                                        C.c_float(self.inv_sigma2[1])) for a in A], np.int64)

    def warp(self, A, ref_levels, kp, sl):
        """ygzo_warp_affine of one item -> uint8[10, 10]."""
        lv = ref_levels[kp["octave"]]
        out = np.zeros(100, np.uint8)
        O.lib().ygzo_warp_affine(O._p(np.ascontiguousarray(A, np.float32)), O._p(lv), lv.shape[1], lv.shape[0],
                                 lv.shape[1], C.c_float(kp["x"]), C.c_float(kp["y"]),
                                 C.c_float(self.scale[kp["octave"]]), C.c_float(self.scale[sl]), 5, O._p(out))
        return out.reshape(10, 10)

    def find_direct(self, it, ref_pyramids, cur_levels, px0=None):
        """ygzo_find_direct_projection per item -> (px f32[n, 2], level i32[n], ok bool[n]);
        ref_pyramids = the keyframes' level lists, indexed by it["ref_index"]."""
        n = len(it["kps"])
        px = np.array(it["px0"] if px0 is None else px0, np.float32).reshape(n, 2).copy()
        lvl, ok = np.zeros(n, np.int32), np.zeros(n, bool)
        refs = [self._ptrs(p) for p in ref_pyramids]
        cp, cw, ch = self._ptrs(cur_levels)
        for i in range(n):
            rp, rw, rh = refs[it["ref_index"][i]]
            T = O.se3_from(it["T_cr"]["q"][i], it["T_cr"]["t"][i])
            sl = C.c_int()
            ok[i] = bool(O.lib().ygzo_find_direct_projection(
                C.byref(self.cam), rp, rw, rh, cp, cw, ch, self.nl, self.sc, self.isc, C.c_float(self.inv_sigma2[1]),
                C.byref(T), O._p(it["pt_ref"][i]), O._p(it["kps"][i:i + 1]), O._p(px[i]), C.byref(sl)))
            lvl[i] = sl.value
        return px, lvl, ok


@functools.lru_cache(maxsize=None)
def oracle_view(cfg):
    return OracleView(cfg)


def restated_find_direct(cfg, it, cur_name, mut=()):
    """FindDirectProjection with the warp from the restatement (under `mut`) and the oracle's Align2D
    -> (px f32[n, 2], level, ok, fully_inside)."""
    ov = oracle_view(cfg)
    _, _, _, nl = CONFIGS[cfg]
    scale, inv_scale, inv_s2 = pyramid_scales(cfg)
    n = len(it["kps"])
    uv = np.stack([it["kps"]["x"], it["kps"]["y"]], 1)
    oc = it["kps"]["octave"]
    A = warp_matrix(cam32(cfg), it["T_cr"]["q"][0], it["T_cr"]["t"][0], it["pt_ref"], uv, scale[oc], mut)
    sl = best_search_level(A, nl - 1, inv_s2[1], mut, oc)
    cur = ov.pyramid(cur_name)
    px, ok, inside = np.zeros((n, 2), np.float32), np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        ref = ov.pyramid(int(it["ref_index"][i]))[oc[i]]
        pb, _, outside = warp_patch(A[i], ref, uv[i], scale[oc[i]], scale[sl[i]], 5, mut)
        inside[i] = not outside.any()
        pxs = it["px0"][i] * inv_scale[sl[i]]
        ok[i], q = O.align2d(cur[sl[i]], pb.reshape(-1), pb[1:9, 1:9].reshape(-1), pxs)
        px[i] = q * scale[sl[i]]
    return px, sl, ok, inside


def end_to_end(px, ok, inside, it):
    """The end-to-end figures of one view: (share of the fully-inside items that converged, median
    distance to the true projection of the converged ones after and before, level-0 px)."""
    sel = ok & inside
    conv = float(ok[inside].mean()) if inside.any() else 0.0
    if not sel.any():
        return conv, np.inf, 0.0
    after = np.linalg.norm(px[sel].astype(np.float64) - it["px_true"][sel], axis=1)
    before = np.linalg.norm(it["px0"][sel].astype(np.float64) - it["px_true"][sel], axis=1)
    return conv, float(np.median(after)), float(np.median(before))


def end_to_end_passes(figs):
    conv, after, before = figs
    return conv >= 0.5 and after < before


# ------------------------------------------------------------------ Align2D on a host image
WINDOW_HALF = 24   # ygzfe_align2d_image sends the 48 x 48 window around the estimate up first
# Seeds of walk_case found by a search over 400 of them (the oracle traced with n_iter = 1..10):
# low-contrast patches whose trajectory leaves the first window but stays inside the image (the
# call's second pass on the whole image), and one that leaves the image (the loop breaks).
WALK_OUT_SEEDS = (1, 16, 25, 28, 52, 57)
OUT_OF_IMAGE_SEEDS = (18,)   # walk_case(seed, edge=True)


@functools.lru_cache(maxsize=None)
def host_image():
    """A 641 x 479 view into a 700 x 500 host image: stride 700 > w."""
    big = S.frame(21, 700, 500)
    return big[7:7 + 479, 13:13 + 641]


def walk_case(seed, edge=False):
    """A low-contrast 10 x 10 patch (grey 100 + U{0..c-1}, c in 2..5: a small H, long steps) and a guess
    in the middle of host_image() (edge: 8..30 px from its left edge) -> (pwb uint8[10, 10], px f32[2])."""
    rng = np.random.default_rng(9000 + seed)
    c = int(rng.integers(2, 6))
    pwb = (100 + rng.integers(0, c, (10, 10))).astype(np.uint8)
    px = np.array([rng.uniform(200, 440), rng.uniform(150, 330)], np.float32)
    if edge:
        px[0] = np.float32(rng.uniform(8, 30))
    return pwb, px


def align2d_trace(img, pwb, px):
    """The oracle's Align2D after 1..10 iterations -> [(converged, px)] * 10."""
    img = np.ascontiguousarray(img)
    return [O.align2d(img, pwb.reshape(-1), np.ascontiguousarray(pwb[1:9, 1:9]).reshape(-1), px, k)
            for k in range(1, 11)]


def walk_kind(img, px, trace):
    """What the first iteration that does not start inside the first window meets: "walk_out" (inside
    the image: the second pass), "out_of_image" (the loop breaks), else "conv" / "nan" / "stays"."""
    h, w = img.shape
    cu, cv = int(np.floor(px[0])), int(np.floor(px[1]))
    x0, y0 = max(cu - WINDOW_HALF, 0), max(cv - WINDOW_HALF, 0)
    x1, y1 = min(cu + WINDOW_HALF, w), min(cv + WINDOW_HALF, h)
    for ok, q in trace[:9]:   # the state that iterations 2..10 start from
        if ok:
            return "conv"
        if not np.isfinite(q).all():
            return "nan"
        ur, vr = int(np.floor(q[0])), int(np.floor(q[1]))
        if ur < 4 or vr < 4 or ur >= w - 4 or vr >= h - 4:
            return "out_of_image"
        if ur - 4 < x0 or vr - 4 < y0 or ur + 4 >= x1 or vr + 4 >= y1:
            return "walk_out"
    return "stays"
