"""Raw local maps for ygzfe.search_local_map_direct and a float32 restatement of its set-up.

map_scene(): a local map on the textured plane -- keyframe images and poses, shuffled
non-monotone kf_ids, per-point world points / normals / distance ranges, per-keyframe
keypoint tables (the points' projections, random octaves) and unordered observation lists
of 0..9 keyframes per point -- with extra candidates that each cull rule of
Frame::isInFrustum (Frame.cc:363-422) rejects.

restate(): the arithmetic stated in include/ygzfe.h, every operation an explicit float32
operation in the stated order, and SelectNearestKeyframe (Tracking.cc:2412-2432); returns
the per-candidate outputs and the compacted CSR items in the format of
ygzfe.search_local_points_direct.  restate64(): the same formulas in float64 with the margin
of every comparison.  expand(): a compact result mapped back to candidate rows.
"""
import numpy as np

import ygzfe
from _scenes import PlaneScene, backproject_plane_np, motion, project, quat_from_rotvec, quat_rot, se3_inv, se3_mul

F = np.float32
CULLED = 4
# why a candidate left (restate()["rule"]); 0 = in view
IN_VIEW, SKIP, BEHIND, MIN_X, MAX_X, MIN_Y, MAX_Y, NEAR, FAR, VIEW_COS, NOT_FINITE = range(11)
CULL_RULES = (BEHIND, MIN_X, MAX_X, MIN_Y, MAX_Y, NEAR, FAR, VIEW_COS)


def rot_matrix(q):
    return np.stack([quat_rot(q, e) for e in np.eye(3)], 1)


def map_scene(seed, n_kf=10, max_obs=9, W=752, H=480, nlevels=4, scale_factor=2.0, n_points=None, cluster=2,
              n_special=8, skip_frac=0.1, cache_frac=0.6, render=True):
    """The raw local map.  Candidates: a jittered pixel grid of keyframe 0 on the plane (with
    `cluster` neighbours within +-1.2 px after each, so points share cells of the 5-px coverage
    grid), and n_special candidates per cull rule (behind the camera, outside each bound, too
    near, too far, viewing cosine below 0.5) scattered among them.  Two keyframes are excluded
    (one as bad, one as the last keyframe).  The first cache_frac of the rows are the cache."""
    rng = np.random.default_rng(4000 + seed)
    sc = PlaneScene(seed, W, H)
    poses = [(quat_from_rotvec(rng.uniform(-0.01, 0.01, 3)), rng.uniform(-0.04, 0.04, 3)) for _ in range(n_kf)]
    v, w = motion(seed)
    qc, tc = se3_mul(quat_from_rotvec(w), v, *poses[0])
    imgs = cur = None
    if render:
        imgs = [sc.render(q.astype(F), t.astype(F), seed * 16 + k) for k, (q, t) in enumerate(poses)]
        cur = sc.render(qc.astype(F), tc.astype(F), seed * 16 + 15)
    gx, gy = np.meshgrid(np.arange(6, W - 6, 22), np.arange(6, H - 6, 22))
    uv = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64) + rng.uniform(-3, 3, (gx.size, 2))
    if n_points is not None:
        uv = uv[rng.permutation(len(uv))[:n_points]]
    if cluster:
        uv = np.concatenate([uv[:, None, :], uv[:, None, :] + rng.uniform(-1.2, 1.2, (len(uv), cluster, 2))],
                            1).reshape(-1, 2)
    n_reg, m = len(uv), n_special
    # candidates outside each bound: plane points seen at pixels outside the current image
    cur_pose = (qc, tc)
    out_uv = np.concatenate([
        np.stack([rng.uniform(-60, -5, m), rng.uniform(40, H - 40, m)], 1),
        np.stack([rng.uniform(W + 5, W + 60, m), rng.uniform(40, H - 40, m)], 1),
        np.stack([rng.uniform(40, W - 40, m), rng.uniform(-60, -5, m)], 1),
        np.stack([rng.uniform(40, W - 40, m), rng.uniform(H + 5, H + 60, m)], 1)])
    in_uv = np.stack([rng.uniform(60, W - 60, 4 * m), rng.uniform(60, H - 60, 4 * m)], 1)  # near, far, cos, behind
    Pw = np.concatenate([backproject_plane_np(sc.cam, poses[0], uv), backproject_plane_np(sc.cam, cur_pose, out_uv),
                         backproject_plane_np(sc.cam, cur_pose, in_uv)])
    n = len(Pw)
    Rc = rot_matrix(qc)
    Ow = -(Rc.T @ tc)
    behind = np.arange(n - m, n)
    Pw[behind] = Ow + (Pw[behind] - Ow) * -rng.uniform(0.3, 1.0, (m, 1))  # mirrored through the camera centre
    PO = Pw - Ow
    dist = np.linalg.norm(PO, axis=1)
    normal = PO / dist[:, None] + rng.uniform(-0.05, 0.05, (n, 3))
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    min_dist, max_dist = dist * rng.uniform(0.3, 0.7, n), dist * rng.uniform(1.5, 3.0, n)
    s0 = n_reg + 4 * m
    min_dist[s0:s0 + m] = dist[s0:s0 + m] * rng.uniform(1.5, 2.0, m)           # 0.8 * min > dist
    max_dist[s0 + m:s0 + 2 * m] = dist[s0 + m:s0 + 2 * m] * rng.uniform(0.4, 0.7, m)  # 1.2 * max < dist
    for i in range(s0 + 2 * m, s0 + 3 * m):  # the normal turned 65..85 degrees away from the ray
        axis = np.cross(PO[i], rng.normal(size=3))
        axis /= np.linalg.norm(axis)
        normal[i] = quat_rot(quat_from_rotvec(axis * rng.uniform(np.radians(65), np.radians(85))), PO[i] / dist[i])
    # the special candidates land at random places among the regular ones
    key = np.concatenate([np.arange(n_reg, dtype=np.float64), rng.uniform(0, n_reg, n - n_reg)])
    order = np.argsort(key, kind="stable")
    Pw, normal, min_dist, max_dist = Pw[order], normal[order], min_dist[order], max_dist[order]
    skip = (rng.random(n) < skip_frac).astype(np.uint8)
    # keyframe table
    kf_id = (rng.permutation(n_kf) * 7 + 100 + rng.integers(0, 7, n_kf)).astype(np.int64)
    kf_excluded = np.zeros(n_kf, np.uint8)
    if n_kf >= 3:
        kf_excluded[rng.permutation(n_kf)[:2]] = 1
    T_rw = np.zeros((n_kf, 12), F)
    T_cr = np.zeros(n_kf, ygzfe.SE3_DTYPE)
    kp_tables, kp_row = [], np.zeros((n_kf, n), np.int32)
    for k, (q, t) in enumerate(poses):
        T_rw[k, :9] = rot_matrix(q).reshape(9)
        T_rw[k, 9:] = t
        qi, ti = se3_inv(q, t)
        T_cr["q"][k], T_cr["t"][k] = se3_mul(qc, tc, qi, ti)
        with np.errstate(all="ignore"):
            px, _ = project(sc.cam, q, t, Pw)
        perm = rng.permutation(n)  # point i's keypoint in keyframe k is row perm[i]
        kps = np.zeros(n, ygzfe.KP_DTYPE)
        kps["x"][perm], kps["y"][perm] = (np.nan_to_num(px[:, j], nan=0.0, posinf=0.0, neginf=0.0) for j in (0, 1))
        kps["octave"] = rng.integers(0, nlevels, n)
        kps["size"] = 31.0 * scale_factor ** kps["octave"]
        kps["angle"] = -1.0
        kp_tables.append(kps)
        kp_row[k] = perm
    obs_ptr, obs_kf, obs_kp = [0], [], []
    for i in range(n):
        for k in rng.permutation(n_kf)[:min(int(rng.integers(0, max_obs + 1)), n_kf)]:
            obs_kf.append(k)
            obs_kp.append(kp_row[k, i])
        obs_ptr.append(len(obs_kf))
    view = {"R": Rc.astype(F).reshape(9), "t": tc.astype(F), "Ow": Ow.astype(F),
            "bounds": (F(0), F(W), F(0), F(H)), "limit": F(0.5), "mbf": F(sc.cam[0] * 0.110073)}
    return {"scene": sc, "kf_images": imgs, "cur_image": cur, "view": view, "kf_id": kf_id, "kf_excluded": kf_excluded,
            "T_rw": T_rw, "T_cr": T_cr, "kp_tables": kp_tables, "n_cache": int(cache_frac * n),
            "world": Pw.astype(F), "normal": normal.astype(F), "min_dist": min_dist.astype(F),
            "max_dist": max_dist.astype(F), "skip": skip, "obs_ptr": np.array(obs_ptr, np.int32),
            "obs_kf": np.array(obs_kf, np.int32), "obs_kp": np.array(obs_kp, np.int32)}


def gpu_view(m):
    v = m["view"]
    return ygzfe.DirectView.make(v["R"], v["t"], v["Ow"], v["bounds"], v["limit"], v["mbf"])


def call_args(m):
    """The array arguments of ygzfe.search_local_map_direct after (kf_frames, cur_frame, cam, view)."""
    return (m["kf_id"], m["kf_excluded"], m["T_rw"], m["T_cr"], m["n_cache"], m["world"], m["normal"], m["min_dist"],
            m["max_dist"], m["skip"], m["obs_ptr"], m["obs_kf"], m["obs_kp"])


def _rt(R, t, P):
    """((R[i][0] * P0 + R[i][1] * P1) + R[i][2] * P2) + t_i, float32, one rounding per operation."""
    R, t, P = np.asarray(R, F).reshape(3, 3), np.asarray(t, F), np.asarray(P, F)
    return np.stack([((R[i, 0] * P[..., 0] + R[i, 1] * P[..., 1]) + R[i, 2] * P[..., 2]) + t[i] for i in range(3)], -1)


def select(obs_kf, obs_kp, kf_id, kf_excluded, n_sel):
    """SelectNearestKeyframe: the observations of keyframes not excluded, the n_sel of largest
    kf_id, in descending kf_id order."""
    el = [(int(kf_id[s]), int(s), int(q)) for s, q in zip(obs_kf, obs_kp) if not kf_excluded[s]]
    el.sort(key=lambda e: -e[0])
    return [(s, q) for _, s, q in el[:n_sel]]


def restate(m, cam, n_sel=5):
    v = m["view"]
    fx, fy, cx, cy = (F(c) for c in cam)
    min_x, max_x, min_y, max_y = v["bounds"]
    P, N = m["world"], m["normal"]
    n = len(P)
    with np.errstate(all="ignore"):
        Pc = _rt(v["R"], v["t"], P)
        invz = F(1.0) / Pc[:, 2]
        u = ((fx * Pc[:, 0]) * invz) + cx
        vv = ((fy * Pc[:, 1]) * invz) + cy
        PO = P - v["Ow"][None, :]
        dist = np.sqrt((PO[:, 0] * PO[:, 0] + PO[:, 1] * PO[:, 1]) + PO[:, 2] * PO[:, 2])
        vc = ((PO[:, 0] * N[:, 0] + PO[:, 1] * N[:, 1]) + PO[:, 2] * N[:, 2]) / dist
        ur = u - v["mbf"] * invz
        lo, hi = F(0.8) * m["min_dist"], F(1.2) * m["max_dist"]
    assert all(a.dtype == F for a in (Pc, invz, u, vv, dist, vc, ur, lo, hi))
    rule = np.zeros(n, np.int32)
    tests = [(SKIP, m["skip"] != 0), (BEHIND, Pc[:, 2] < 0), (MIN_X, u < min_x), (MAX_X, u > max_x),
             (MIN_Y, vv < min_y), (MAX_Y, vv > max_y), (NEAR, dist < lo), (FAR, dist > hi), (VIEW_COS, vc < v["limit"]),
             (NOT_FINITE, ~(np.isfinite(u) & np.isfinite(vv) & np.isfinite(dist) & np.isfinite(vc)))]
    for code, hit in tests:  # the first rule that rejects, in the reference's order
        rule[(rule == 0) & hit] = code
    culled = rule != 0
    z = np.zeros(n, F)
    out = {"culled": culled, "rule": rule, "proj": np.where(culled[:, None], F(0), np.stack([u, vv, ur], 1)),
           "view_cos": np.where(culled, z, vc), "dist": np.where(culled, z, dist)}
    rows = np.flatnonzero(~culled)
    item_ptr, ref_index, item_kp, kps, pt_ref, n_elig = [0], [], [], [], [], np.zeros(n, np.int32)
    for i in rows:
        a, b = m["obs_ptr"][i], m["obs_ptr"][i + 1]
        n_elig[i] = sum(1 for s in m["obs_kf"][a:b] if not m["kf_excluded"][s])
        for s, q in select(m["obs_kf"][a:b], m["obs_kp"][a:b], m["kf_id"], m["kf_excluded"], n_sel):
            ref_index.append(s)
            item_kp.append(q)
            kps.append(m["kp_tables"][s][q:q + 1])
            pt_ref.append(_rt(m["T_rw"][s, :9], m["T_rw"][s, 9:], P[i]))
        item_ptr.append(len(ref_index))
    ref_index = np.array(ref_index, np.int32)
    out.update(rows=rows, n_cache=int((rows < m["n_cache"]).sum()), n_eligible=n_elig,
               item_ptr=np.array(item_ptr, np.int32), ref_index=ref_index, item_kp=np.array(item_kp, np.int32),
               kps=np.concatenate(kps) if kps else np.zeros(0, ygzfe.KP_DTYPE),
               pt_ref=np.array(pt_ref, F).reshape(-1, 3), T_cr=m["T_cr"][ref_index],
               px_proj=np.stack([u, vv], 1)[rows])
    return out


def items_of(r):
    """restate()'s compact items as the array arguments of search_local_points_direct after n_cache."""
    return r["item_ptr"], r["ref_index"], r["kps"], r["pt_ref"], r["T_cr"], r["px_proj"]


def expand(r, n, px, matched, status):
    """A result of search_local_points_direct over restate()'s compact points, on candidate rows:
    (status with CULLED, px_out, matched_kf, matched_kp)."""
    st = np.full(n, CULLED, np.int32)
    pxo = np.zeros((n, 2), F)
    mkf, mkp = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    rows = r["rows"]
    st[rows] = status
    pxo[rows] = px
    hit = matched >= 0
    mkf[rows[hit]] = r["ref_index"][matched[hit]]
    mkp[rows[hit]] = r["item_kp"][matched[hit]]
    return st, pxo, mkf, mkp


def restate64(m, cam):
    """The same formulas in float64 on the same inputs: (in_view, u, v, the smallest margin |a - b|
    over the comparisons a candidate reaches)."""
    v = m["view"]
    fx, fy, cx, cy = (float(c) for c in cam)
    min_x, max_x, min_y, max_y = (float(b) for b in v["bounds"])
    P, N = m["world"].astype(np.float64), m["normal"].astype(np.float64)
    R, t, Ow = v["R"].astype(np.float64).reshape(3, 3), v["t"].astype(np.float64), v["Ow"].astype(np.float64)
    with np.errstate(all="ignore"):
        Pc = P @ R.T + t
        invz = 1.0 / Pc[:, 2]
        u, vv = fx * Pc[:, 0] * invz + cx, fy * Pc[:, 1] * invz + cy
        PO = P - Ow
        dist = np.sqrt((PO * PO).sum(1))
        vc = (PO * N).sum(1) / dist
        lo, hi = 0.8 * m["min_dist"].astype(np.float64), 1.2 * m["max_dist"].astype(np.float64)
    margins = [Pc[:, 2], u - min_x, max_x - u, vv - min_y, max_y - vv, dist - lo, hi - dist, vc - float(v["limit"])]
    alive = m["skip"] == 0
    margin = np.full(len(P), np.inf)
    for g in margins:  # a comparison counts only for candidates that reach it
        with np.errstate(all="ignore"):
            margin = np.where(alive, np.minimum(margin, np.abs(g)), margin)
            alive = alive & (g >= 0)
    finite = np.isfinite(u) & np.isfinite(vv) & np.isfinite(dist) & np.isfinite(vc)
    return alive & finite, u, vv, margin
