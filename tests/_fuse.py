"""The search of ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:748-866; KeyFrame::GetFeaturesInArea,
KeyFrame.cc:774-809; MapPoint::PredictScale, MapPoint.cc:343-357) restated in plain Python / numpy, in two forms,
and the inputs its tests share.

* `fuse_loops`: the reference's loops as written (the cell walk of GetFeaturesInArea into vIndices, then the running
  bestDist with `dist < bestDist`), float32 arithmetic with each operation rounded once, the gates in double.
* `fuse_closed`: per pair the argmin of the (distance, cell, index) key over every keypoint of the keyframe that
  passes the predicates: what ygzfe_fuse_search_batch computes.

PredictScale is ceil(logf(ratio) / lsf) with libm's logf through ctypes: neither np.log (numpy's own float32 path)
nor the library's threshold table, which these restatements are there to check.

A case is a dict: kfs = [dict(kps, desc, ur (or None), bounds (min_x, max_x, min_y, max_y), view float32[20])],
world, normal float32[n, 3], min_dist, max_dist float32[n] (raw), desc uint8[n, 32], skip uint8[n_kf, n] or None, th,
scale, isig float32[n_levels], lsf float32, check_reproj.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

import ygzfe
import _scenes as S

F32 = np.float32
TH_LOW = 50
COLS, ROWS = 64, 48
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]


def logf(x):
    return F32(_libm.logf(float(F32(x))))


def predict_scale(ratio, lsf, n_levels):
    """MapPoint::PredictScale, or None where the reference would convert a non-finite float to int."""
    with np.errstate(all="ignore"):
        v = np.ceil(logf(ratio) / F32(lsf))
    if not np.isfinite(v):
        return None
    return int(min(max(int(v), 0), n_levels - 1))


def _round_half_away(v):
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def grid_of(kf):
    """Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:314-330, 483-493): (inv_w, inv_h, cell id per keypoint
    (ix * ROWS + iy, -1 outside), {cell: ascending indices})."""
    if "_grid" not in kf:
        mnx, mxx, mny, mxy = (F32(b) for b in kf["bounds"])
        inv_w, inv_h = F32(COLS) / (mxx - mnx), F32(ROWS) / (mxy - mny)
        cell = np.full(len(kf["kps"]), -1, np.int64)
        cells = {}
        for i, kp in enumerate(kf["kps"]):
            px = _round_half_away(float((F32(kp["x"]) - mnx) * inv_w))
            py = _round_half_away(float((F32(kp["y"]) - mny) * inv_h))
            if 0 <= px < COLS and 0 <= py < ROWS:
                cell[i] = px * ROWS + py
                cells.setdefault(int(cell[i]), []).append(i)
        kf["_grid"] = (inv_w, inv_h, cell, cells)
    return kf["_grid"]


def project(case, k, i):
    """:768-811 for pair (k, i): None where culled, else dict(u, v, ur, dist, ratio, level, radius)."""
    kf = case["kfs"][k]
    vw = np.asarray(kf["view"], F32)
    R, t, Ow = vw[:9].reshape(3, 3), vw[9:12], vw[12:15]
    fx, fy, cx, cy, bf = vw[15:20]
    P = np.asarray(case["world"][i], F32)
    with np.errstate(all="ignore"):
        Pc = [((R[j, 0] * P[0] + R[j, 1] * P[1]) + R[j, 2] * P[2]) + t[j] for j in range(3)]
        if Pc[2] < 0:
            return None
        invz = F32(1) / Pc[2]
        x, y = Pc[0] * invz, Pc[1] * invz
        u, v = fx * x + cx, fy * y + cy
        mnx, mxx, mny, mxy = (F32(b) for b in kf["bounds"])
        if not (u >= mnx and u < mxx and v >= mny and v < mxy):
            return None
        ur = u - bf * invz
        PO = P - Ow
        dist = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2])
        mn, mx = F32(case["min_dist"][i]), F32(case["max_dist"][i])
        if dist < F32(0.8) * mn or dist > F32(1.2) * mx:
            return None
        n = np.asarray(case["normal"][i], F32)
        if float((PO[0] * n[0] + PO[1] * n[1]) + PO[2] * n[2]) < 0.5 * float(dist):
            return None
        ratio = mx / dist
    if not (np.isfinite(dist) and dist > 0 and np.isfinite(ratio) and ratio > 0):
        return None  # the documented deviation
    level = predict_scale(ratio, case["lsf"], len(case["scale"]))
    if level is None:
        return None
    return {"u": u, "v": v, "ur": ur, "dist": dist, "ratio": ratio, "level": level,
            "radius": F32(case["th"]) * F32(case["scale"][level])}


def _cell_range(kf, u, v, r):
    """:778-792: (x0, x1, y0, y1) or None."""
    inv_w, inv_h, _, _ = grid_of(kf)
    mnx, _, mny, _ = (F32(b) for b in kf["bounds"])
    x0 = max(0, int(np.floor((u - mnx - r) * inv_w)))
    if x0 >= COLS:
        return None
    x1 = min(COLS - 1, int(np.ceil((u - mnx + r) * inv_w)))
    if x1 < 0:
        return None
    y0 = max(0, int(np.floor((v - mny - r) * inv_h)))
    if y0 >= ROWS:
        return None
    y1 = min(ROWS - 1, int(np.ceil((v - mny + r) * inv_h)))
    if y1 < 0:
        return None
    return x0, x1, y0, y1


def _gate(case, kf, q, idx):
    """:833-860 for candidate idx: the octave filter and the reprojection gate."""
    kp = kf["kps"][idx]
    lvl = int(kp["octave"])
    if lvl < q["level"] - 1 or lvl > q["level"]:
        return False
    if not case["check_reproj"]:
        return True
    ex, ey = q["u"] - F32(kp["x"]), q["v"] - F32(kp["y"])
    isig = F32(case["isig"][lvl])
    if kf["ur"] is not None and kf["ur"][idx] >= 0:
        er = q["ur"] - F32(kf["ur"][idx])
        e2 = (ex * ex + ey * ey) + er * er
        return not float(e2 * isig) > 7.8
    e2 = ex * ex + ey * ey
    return not float(e2 * isig) > 5.99


def _dist(case, kf, i, idx):
    return int(_POP[np.asarray(case["desc"][i], np.uint8) ^ np.asarray(kf["desc"][idx], np.uint8)].sum())


def _pair_loops(case, k, i):
    kf = case["kfs"][k]
    q = project(case, k, i)
    if q is None:
        return -1, 256
    rng = _cell_range(kf, q["u"], q["v"], q["radius"])
    indices = []
    if rng is not None:
        cells = grid_of(kf)[3]
        for ix in range(rng[0], rng[1] + 1):
            for iy in range(rng[2], rng[3] + 1):
                for j in cells.get(ix * ROWS + iy, ()):
                    dx, dy = F32(kf["kps"][j]["x"]) - q["u"], F32(kf["kps"][j]["y"]) - q["v"]
                    if abs(dx) < q["radius"] and abs(dy) < q["radius"]:
                        indices.append(j)
    best_dist, best_idx = 256, -1
    for idx in indices:
        if not _gate(case, kf, q, idx):
            continue
        d = _dist(case, kf, i, idx)
        if d < best_dist:
            best_dist, best_idx = d, idx
    return (best_idx if best_dist <= TH_LOW else -1), best_dist


def _pair_closed(case, k, i):
    kf = case["kfs"][k]
    q = project(case, k, i)
    if q is None or len(kf["kps"]) == 0:
        return -1, 256
    rng = _cell_range(kf, q["u"], q["v"], q["radius"])
    if rng is None:
        return -1, 256
    cell = grid_of(kf)[2]
    ix, iy = cell // ROWS, cell % ROWS
    x, y = kf["kps"]["x"].astype(F32), kf["kps"]["y"].astype(F32)
    ok = (cell >= 0) & (ix >= rng[0]) & (ix <= rng[1]) & (iy >= rng[2]) & (iy <= rng[3])
    ok &= (np.abs(x - q["u"]) < q["radius"]) & (np.abs(y - q["v"]) < q["radius"])
    keys = [(_dist(case, kf, i, int(j)), int(cell[j]), int(j)) for j in np.flatnonzero(ok) if _gate(case, kf, q, int(j))]
    if not keys:
        return -1, 256
    d, _, j = min(keys)
    return (j if d <= TH_LOW else -1), d


def _run(case, pair):
    n_kf, n = len(case["kfs"]), len(case["world"])
    bi, bd = np.full((n_kf, n), -1, np.int32), np.full((n_kf, n), 256, np.int32)
    for k in range(n_kf):
        for i in range(n):
            if case["skip"] is not None and case["skip"][k, i]:
                continue
            bi[k, i], bd[k, i] = pair(case, k, i)
    return bi, bd


def fuse_loops(case):
    """-> (best_idx int32[n_kf, n_pts], best_dist int32[n_kf, n_pts]) by the reference's loops."""
    return _run(case, _pair_loops)


def fuse_closed(case):
    return _run(case, _pair_closed)


def with_flags(case, check_reproj=None, skip=None, kfs=None):
    out = dict(case)
    if check_reproj is not None:
        out["check_reproj"] = bool(check_reproj)
    if skip is not None:
        out["skip"] = np.asarray(skip, np.uint8)
    if kfs is not None:
        out["kfs"] = [case["kfs"][k] for k in kfs]
        if out["skip"] is not None:
            out["skip"] = out["skip"][list(kfs)]
    return out


def gpu_call(case, frames=None):
    """The case through ygzfe.fuse_search_batch (frames: MatchFrames already set, else made here)."""
    frames = frames or [ygzfe.MatchFrame(0).set(kf["kps"], kf["desc"], kf["ur"], kf["bounds"]) for kf in case["kfs"]]
    views = np.array([kf["view"] for kf in case["kfs"]], F32).reshape(-1, 20)
    return ygzfe.fuse_search_batch(frames, views, case["world"], case["normal"], case["min_dist"], case["max_dist"],
                                   case["desc"], case["scale"], case["isig"], case["lsf"], skip=case["skip"],
                                   th=case["th"], check_reproj=case["check_reproj"])


# ------------------------------------------------------------------------------------------ the C2 scene
def _rot(q):
    return np.stack([S.quat_rot(np.asarray(q, np.float64), e) for e in np.eye(3)], 1)


def view_of(cam, pose, bf):
    """view[20] of a keyframe at T_cw = pose: Rcw, tcw, Ow = -Rcw' tcw, fx, fy, cx, cy, bf."""
    R, t = _rot(pose[0]), np.asarray(pose[1], np.float64)
    return np.concatenate([R.ravel(), t, -R.T @ t, cam, [bf]]).astype(F32)


@functools.lru_cache(maxsize=None)
def c2_scene(seed=0, n_points=400):
    """Three target keyframes of the textured plane (752 x 480, oracle extraction; the second with u_right) and about
    n_points map points seen from two of them: positions jittered off the plane, the normal and the distance range
    as MapPoint::UpdateNormalAndDepth leaves them, the descriptor of the observing keypoint a few bits apart."""
    p = S.match_pair("C2", seed)
    sc, rng = p["sc"], np.random.default_rng(8800 + seed)
    nl = S.CONFIGS["C2"][4]
    scale = np.asarray(p["scale"], F32)[:nl]
    cam = np.asarray(sc.cam, np.float64)
    bf = float(F32(cam[0]) * F32(0.11))
    v, w = S.motion(seed + 31, 3.0)
    pose2 = (S.quat_from_rotvec(w), v)
    img2 = sc.render(pose2[0].astype(F32), pose2[1].astype(F32), 3 * seed + 9)
    (k2, d2), _ = S._oracle_extract("C2", img2)
    poses = [p["poses"][0], p["poses"][1], pose2]
    frames = [(p["k0"], p["d0"]), (p["k1"], p["d1"]), (k2, d2)]
    bounds = (0.0, float(p["W"]), 0.0, float(p["H"]))
    kfs = []
    for k, ((kps, desc), pose) in enumerate(zip(frames, poses)):
        ur = None
        if k == 1:  # depth ~ 3 m: disparity bf / 3, half the keypoints stereo
            ur = np.where(rng.random(len(kps)) < 0.5, kps["x"] - F32(bf / 3.0) + rng.normal(0, 0.4, len(kps)),
                          -1.0).astype(F32)
        kfs.append({"kps": kps, "desc": desc, "ur": ur, "bounds": bounds, "view": view_of(cam, pose, bf)})
    world, normal, mn, mx, desc = [], [], [], [], []
    for k, share in ((0, 0.6), (2, 0.4)):
        kps, dsc = frames[k]
        pick = rng.choice(len(kps), int(n_points * share), replace=False)
        uv = np.stack([kps["x"][pick], kps["y"][pick]], 1).astype(np.float64)
        Pw = S.backproject_plane_np(cam, poses[k], uv) + rng.normal(0, 0.004, (len(pick), 3))
        Ow = kfs[k]["view"][12:15].astype(np.float64)
        PO = Pw - Ow
        dist = np.linalg.norm(PO, axis=1)
        world.append(Pw)
        normal.append(PO / dist[:, None])
        far = dist * scale[kps["octave"][pick]]
        mx.append(far)
        mn.append(far / scale[nl - 1])
        dd = dsc[pick].copy()
        for r in range(len(pick)):
            for b in rng.integers(0, 256, rng.integers(0, 9)):
                dd[r, b // 8] ^= np.uint8(1 << (b % 8))
        desc.append(dd)
    return {"kfs": kfs, "world": np.concatenate(world).astype(F32), "normal": np.concatenate(normal).astype(F32),
            "min_dist": np.concatenate(mn).astype(F32), "max_dist": np.concatenate(mx).astype(F32),
            "desc": np.concatenate(desc), "skip": None, "th": 3.0, "scale": scale,
            "isig": (F32(1) / (scale * scale)).astype(F32), "lsf": F32(np.log(2.0)), "check_reproj": True}


# ------------------------------------------------------------------------------------------ crafted rows
SCALE4 = np.array([1, 2, 4, 8], F32)
BOUNDS = (0.0, 752.0, 0.0, 480.0)
MAX_FOR_LEVEL = {0: 2.0, 1: 4.0, 2: 6.0, 3: 16.0}  # with dist 2: ratio 1, 2, 3, 8


def kps_of(xy, octave=0):
    k = np.zeros(len(xy), ygzfe.KP_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy, F32).T
    k["octave"], k["size"] = octave, 31.0
    return k


def desc_of(bits):
    """One descriptor per entry: the first `bits` bits set (so `bits` from the all-zero descriptor)."""
    d = np.zeros((len(bits), 32), np.uint8)
    for i, b in enumerate(bits):
        d[i] = np.packbits(np.arange(256) < b)
    return d


def point(u, v, level=0, dist=2.0, z=1.0, **kw):
    """A map point that the unit camera (fx = fy = 1, cx = cy = 0, R = I, t = 0) projects to exactly (u, v): P =
    (u z, v z, z), with Ow placed so that PO = (0, 0, dist) exactly, normal (0, 0, 1), all-zero descriptor."""
    out = {"P": (u * z, v * z, z), "dist": dist, "max": MAX_FOR_LEVEL[level], "min": 0.1, "normal": (0, 0, 1),
           "bits": 0}
    out.update(kw)
    return out


def crafted(xy, octave, bits, pts, ur=None, bf=0.0, th=3.0, check_reproj=True, isig=None, bounds=BOUNDS):
    """One keyframe with the unit camera, keypoints xy / octave / descriptors `bits` from zero, against pts."""
    kf = {"kps": kps_of(xy, octave), "desc": desc_of(bits), "ur": None if ur is None else np.asarray(ur, F32),
          "bounds": bounds}
    # Ow is an argument of its own: every crafted point shares P - Ow = (0, 0, dist) only when there is one point,
    # so each point gets its own keyframe row over the same keypoints
    case = {"kfs": [], "world": np.array([q["P"] for q in pts], F32).reshape(-1, 3),
            "normal": np.array([q["normal"] for q in pts], F32).reshape(-1, 3),
            "min_dist": np.array([q["min"] for q in pts], F32), "max_dist": np.array([q["max"] for q in pts], F32),
            "desc": desc_of([q["bits"] for q in pts]), "th": th, "scale": SCALE4,
            "isig": np.asarray([1, 0.25, 0.0625, 0.015625] if isig is None else isig, F32), "lsf": logf(2.0),
            "check_reproj": check_reproj}
    for q in pts:
        P = np.asarray(q["P"], F32)
        Ow = np.array([P[0], P[1], P[2] - F32(q["dist"])], F32)
        assert P[2] - Ow[2] == F32(q["dist"]), "the crafted distance is not exact"
        view = np.concatenate([np.eye(3).ravel(), [0, 0, 0], Ow, [1, 1, 0, 0, bf]]).astype(F32)
        case["kfs"].append(dict(kf, view=view))
    n = len(pts)
    case["skip"] = (1 - np.eye(n, dtype=np.uint8)) if n > 1 else None  # point i against its own row only
    return case


def diag(res):
    """The (row i, point i) entries of a crafted case's result."""
    bi, bd = res
    return [int(bi[i, i]) for i in range(bi.shape[1])], [int(bd[i, i]) for i in range(bd.shape[1])]


def around(limit):
    """The largest float32 <= limit (a double) and the next one up."""
    lo = F32(limit)
    if float(lo) > limit:
        lo = np.nextafter(lo, F32(0))
    return lo, np.nextafter(lo, F32(np.inf))


def factor_hitting(c, target):
    """A float32 m with float32(c) * m == target exactly (searched around target / c), or None."""
    m = F32(target) / F32(c)
    for cand in [m] + [f(m) for f in (lambda a: np.nextafter(a, F32(0)), lambda a: np.nextafter(a, F32(np.inf)))]:
        if F32(c) * cand == F32(target):
            return cand
    return None


def crafted_cases(level2_threshold=None):
    """name -> (case, expected best_idx per point, expected best_dist per point).  Cells are 11.75 x 10 px; a
    keypoint's cell is round(x / 11.75), round(y / 10).  level2_threshold: the float32 ratio at which PredictScale
    first gives 2 (found by the caller with logf; the table is not used here)."""
    out = {}
    # equal distances in two cells: index 1 at x = 99 (cell 8) comes before index 0 at x = 101 (cell 9)
    out["tie_two_cells"] = (crafted([(101, 100), (99, 100)], 0, [7, 7], [point(100, 100)]), [1], [7])
    # equal distances in one cell: the lower index
    out["tie_one_cell"] = (crafted([(101, 100), (102, 100), (100, 101)], 0, [9, 7, 7], [point(100, 100)]), [1], [7])
    # predicted level 2: octaves 0 .. 3, the best descriptor at level + 1, the next at level - 2
    out["level_filter"] = (crafted([(101, 100), (100, 101), (99, 100), (100, 99)], [0, 1, 2, 3], [3, 20, 10, 0],
                                   [point(100, 100, 2)]), [2], [10])
    # predicted level 0: only octave 0
    out["level_zero"] = (crafted([(101, 100), (100, 101)], [1, 0], [0, 12], [point(100, 100, 0)]), [1], [12])
    if level2_threshold is not None:  # ratio = max / 1: at the threshold level 2 (octaves 1, 2), below it level 1
        T = F32(level2_threshold)
        at = point(100, 100, dist=1.0, max=T, min=0.1)
        below = point(100, 100, dist=1.0, max=np.nextafter(T, F32(0)), min=0.1)
        out["ratio_at_threshold"] = (crafted([(101, 100), (100, 101)], [2, 0], [0, 5], [at, below]), [0, 1], [0, 5])
    # the mono gate: e2 = 1 against inv sigma2 just under / over 5.99; accepted without the gate
    lo, hi = around(5.99)
    mono = dict(xy=[(101, 100)], octave=0, bits=[4], pts=[point(100, 100)])
    out["mono_gate_under"] = (crafted(isig=[lo, 1, 1, 1], **mono), [0], [4])
    out["mono_gate_over"] = (crafted(isig=[hi, 1, 1, 1], **mono), [-1], [256])
    out["mono_gate_off"] = (crafted(isig=[hi, 1, 1, 1], check_reproj=False, **mono), [0], [4])
    # the stereo gate: ex = ey = 0, er = 1 (bf = 0: ur = u = 100, u_right = 99) against 7.8
    lo, hi = around(7.8)
    st = dict(xy=[(100, 100)], octave=0, bits=[4], pts=[point(100, 100)], ur=[99.0])
    out["stereo_gate_under"] = (crafted(isig=[lo, 1, 1, 1], **st), [0], [4])
    out["stereo_gate_over"] = (crafted(isig=[hi, 1, 1, 1], **st), [-1], [256])
    out["stereo_gate_off"] = (crafted(isig=[hi, 1, 1, 1], check_reproj=False, **st), [0], [4])
    # TH_LOW
    out["dist_50"] = (crafted([(101, 100)], 0, [50], [point(100, 100)]), [0], [50])
    out["dist_51"] = (crafted([(101, 100)], 0, [51], [point(100, 100)]), [-1], [51])
    # frustum and bounds
    near = dict(xy=[(1, 100), (751, 100)], octave=0, bits=[3, 3])
    out["behind"] = (crafted(pts=[point(100, 100, z=-1.0)], **near), [-1], [256])
    out["depth_zero"] = (crafted(pts=[point(1, 1, P=(1, 1, 0)), point(0, 0, P=(0, 0, 0))], **near), [-1, -1], [256, 256])
    out["u_at_bounds"] = (crafted(pts=[point(0, 100), point(752, 100)], **near), [0, -1], [3, 256])
    m08, m12 = factor_hitting(0.8, 2.0), None
    for d in (2.0, 3.0, 1.5, 2.5, 1.75, 2.25, 3.5):
        m12 = factor_hitting(1.2, d)
        if m12 is not None:
            break
    assert m08 is not None and m12 is not None
    out["dist_at_range_ends"] = (crafted([(101, 100)], 0, [3], [point(100, 100, min=m08),
                                                                 point(100, 100, dist=d, max=m12, min=0.1),
                                                                 point(100, 100, min=2.6)]),
                                 [0, 0, -1], [3, 3, 256])
    out["view_cos"] = (crafted([(101, 100)], 0, [3], [point(100, 100, normal=(0, 0, 0.5)),
                                                       point(100, 100, normal=(0, 0, np.nextafter(F32(0.5), F32(0))))]),
                       [0, -1], [3, 256])
    # |dx| == r is outside (radius 3)
    out["dx_equals_r"] = (crafted([(103, 100), (102, 100), (100, 97)], 0, [0, 9, 0], [point(100, 100)]), [1], [9])
    # windows: > 64 cells (radius 60: 12 x 13 cells), partly outside the grid, empty
    far = [(45, 50), (155, 150), (100, 100), (159.5, 40.5), (161, 100)]
    out["wide_window"] = (crafted(far, 0, [9, 8, 30, 7, 0], [point(100, 100)], th=60.0, check_reproj=False), [3], [7])
    out["window_at_corner"] = (crafted([(1, 1), (3, 2)], 0, [9, 4], [point(2, 2)], th=30.0, check_reproj=False),
                               [1], [4])
    out["empty_window"] = (crafted([(300, 300)], 0, [0], [point(100, 100)]), [-1], [256])
    # a keypoint outside the bounds has no cell: never a candidate
    out["no_cell"] = (crafted([(-7, 100), (2, 100)], 0, [0, 6], [point(0.5, 100)], th=10.0, check_reproj=False), [1], [6])
    return out


def level_threshold(lsf, L):
    """The smallest positive float32 ratio with ceil(logf(ratio) / lsf) >= L, by bisection over the bit patterns
    with logf itself (the tests' own search, independent of ygzfe_predict_scale_thresholds)."""
    reach = lambda b: bool(np.ceil(logf(np.array([b], np.uint32).view(F32)[0]) / F32(lsf)) >= L)  # noqa: E731
    lo, hi = 1, 0x7F7FFFFF
    if not reach(hi):
        return F32(np.inf)
    if reach(lo):
        return np.array([lo], np.uint32).view(F32)[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if reach(mid) else (mid, hi)
    return np.array([hi], np.uint32).view(F32)[0]
