"""ORBmatcher::SearchForTriangulation (ORBmatcher.cc:597-746, CheckDistEpipolarLine :136-153) restated in
plain Python / numpy, in two forms, and the inputs its tests share.

* `search_loops`: the reference's loops as written (running bestDist, `dist > bestDist` skips, an equal distance
  replaces), float32 arithmetic with each operation rounded once, the last comparison in double.
* `search_closed`: per KF1 feature the smallest accepted distance, among equal distances the last position in the
  node's list: what ygzfe_search_for_triangulation_batch computes.  This reference never writes vbMatched2, so the
  two agree; tests/test_cpu_triangulation.py checks that they do.

A case is a dict: k1, d1, ur1 (or None), has_mp1, fv1 = (nodes, ptr, feats), nbs = [dict(k2, d2, ur2, has_mp2, fv2,
F12 float32[3, 3], ep float32[2])], sigma2, scale (float32 per level).
"""
import functools

import numpy as np

import ygzfe
import _scenes as S

TH_LOW, HISTO = 50, 30
F32 = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(d1, d2):
    """DescriptorDistance of every (row of d1, row of d2): int32 [n1, n2]."""
    d1, d2 = np.asarray(d1, np.uint8).reshape(-1, 32), np.asarray(d2, np.uint8).reshape(-1, 32)
    out = np.zeros((len(d1), len(d2)), np.int32)
    for r in range(0, len(d1), 128):
        out[r:r + 128] = _POP[d1[r:r + 128, None, :] ^ d2[None, :, :]].sum(2, dtype=np.int32)
    return out


def epipolar_ok(x1, y1, x2, y2, F, sigma2):
    """CheckDistEpipolarLine (:136-153): float32, the comparison in double (3.84 is a double literal)."""
    x1, y1, x2, y2 = F32(x1), F32(y1), F32(x2), F32(y2)
    a = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]
    b = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
    c = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if den == 0:
        return False
    with np.errstate(all="ignore"):
        dsqr = num * num / den
    return bool(float(dsqr) < 3.84 * float(sigma2))


def _accepted(case, nb, D, idx1, idx2, stereo1):
    """Every test of the inner loop (:657-685) that does not involve bestDist."""
    if nb["has_mp2"][idx2]:
        return False
    stereo2 = nb["ur2"] is not None and bool(nb["ur2"][idx2] >= 0)
    if case["only_stereo"] and not stereo2:
        return False
    if D[idx1, idx2] > TH_LOW:
        return False
    kp2 = nb["k2"][idx2]
    if not stereo1 and not stereo2:
        distex, distey = nb["ep"][0] - kp2["x"], nb["ep"][1] - kp2["y"]
        if distex * distex + distey * distey < F32(100) * case["scale"][kp2["octave"]]:
            return False
    kp1 = case["k1"][idx1]
    return epipolar_ok(kp1["x"], kp1["y"], kp2["x"], kp2["y"], nb["F12"], case["sigma2"][kp2["octave"]])


def _shared_nodes(fv1, fv2):
    """The lower-bound merge of :630-716: (position in fv1, position in fv2) of every shared node."""
    n1, n2 = np.asarray(fv1[0]), np.asarray(fv2[0])
    i = j = 0
    while i < len(n1) and j < len(n2):
        if n1[i] == n2[j]:
            yield i, j
            i, j = i + 1, j + 1
        elif n1[i] < n2[j]:
            i += int(np.searchsorted(n1[i:], n2[j], "left"))
        else:
            j += int(np.searchsorted(n2[j:], n1[i], "left"))


def _rot_bin(a1, a2):
    rot = F32(a1) - F32(a2)
    if rot < 0.0:
        rot = rot + F32(360.0)
    v = float(rot * (F32(1.0) / F32(HISTO)))
    b = int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)  # std::round: halves away from zero
    return 0 if b == HISTO else b


def _three_maxima(counts):
    """ComputeThreeMaxima (:1471-1502)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(HISTO):
        s = counts[i]
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif max3 < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _orientation(case, nb, m12, order):
    """:696-705 and :718-734 over the matches in the order the loops found them."""
    hist = [[] for _ in range(HISTO)]
    for idx1 in order:
        hist[_rot_bin(case["k1"][idx1]["angle"], nb["k2"][m12[idx1]]["angle"])].append(idx1)
    keep = _three_maxima([len(h) for h in hist])
    n = len(order)
    for i in range(HISTO):
        if i in keep:
            continue
        for idx1 in hist[i]:
            m12[idx1] = -1
            n -= 1
    return n


def _search(case, nb, closed):
    D = nb["D"] if "D" in nb else hamming(case["d1"], nb["d2"])
    n1 = len(case["k1"])
    m12 = np.full(n1, -1, np.int32)
    order = []
    (_, ptr1, feats1), (_, ptr2, feats2) = case["fv1"], nb["fv2"]
    for i, j in _shared_nodes(case["fv1"], nb["fv2"]):
        list2 = [int(v) for v in feats2[ptr2[j]:ptr2[j + 1]]]
        for idx1 in (int(v) for v in feats1[ptr1[i]:ptr1[i + 1]]):
            if case["has_mp1"][idx1]:
                continue
            stereo1 = case["ur1"] is not None and bool(case["ur1"][idx1] >= 0)
            if case["only_stereo"] and not stereo1:
                continue
            if closed:  # argmin over (distance, -position) of the accepted candidates
                ok = [(int(D[idx1, idx2]), -pos) for pos, idx2 in enumerate(list2)
                      if _accepted(case, nb, D, idx1, idx2, stereo1)]
                best = list2[-min(ok)[1]] if ok else -1
            else:  # :651-689
                best_dist, best = TH_LOW, -1
                for idx2 in list2:
                    if D[idx1, idx2] > TH_LOW or D[idx1, idx2] > best_dist:
                        continue
                    if _accepted(case, nb, D, idx1, idx2, stereo1):
                        best, best_dist = idx2, int(D[idx1, idx2])
            if best >= 0:
                m12[idx1] = best
                order.append(idx1)
    n = _orientation(case, nb, m12, order) if case["check_ori"] else len(order)
    return m12, n


def search_loops(case):
    """-> (matches12 int32[n_nb, n1], nmatches int32[n_nb]) by the reference's loops."""
    r = [_search(case, nb, False) for nb in case["nbs"]]
    return np.array([m for m, _ in r], np.int32).reshape(len(r), len(case["k1"])), np.array([n for _, n in r], np.int32)


def search_closed(case):
    r = [_search(case, nb, True) for nb in case["nbs"]]
    return np.array([m for m, _ in r], np.int32).reshape(len(r), len(case["k1"])), np.array([n for _, n in r], np.int32)


def with_flags(case, only_stereo, check_ori):
    return dict(case, only_stereo=bool(only_stereo), check_ori=bool(check_ori))


# ------------------------------------------------------------------------------------------ FeatureVectors
def csr(node, order=None):
    """(nodes, ptr, feats) of per-feature node ids; feats of a node in `order` (default: index order)."""
    node = np.asarray(node, np.int64)
    order = np.arange(len(node)) if order is None else np.asarray(order)
    order = order[np.argsort(node[order], kind="stable")]
    nodes, counts = np.unique(node[order], return_counts=True)
    return nodes.astype(np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order.astype(np.int32)


N_WORDS = 40


def word_nodes(desc):
    """The nearest of N_WORDS fixed random descriptors (the first on ties): descriptors a few bits apart share a
    node, as under a vocabulary; _scenes.feature_vector's two raw bytes split four matching pairs in five."""
    words = np.random.default_rng(4040).integers(0, 256, (N_WORDS, 32), dtype=np.uint8)
    return hamming(desc, words).argmin(1) * 5 + 2


# ------------------------------------------------------------------------------------------ the C2 scene
def rot_matrix(q):
    return np.stack([S.quat_rot(np.asarray(q, np.float64), e) for e in np.eye(3)], 1)


def fundamental(cam, pose1, pose2):
    """LocalMapping::ComputeF12 (LocalMapping.cc:1294-1308) and the epipole of :603-609 from the true poses T_cw,
    float64 then float32: x1' F12 x2 = 0."""
    fx, fy, cx, cy = cam
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    R1, t1 = rot_matrix(pose1[0]), np.asarray(pose1[1], np.float64)
    R2, t2 = rot_matrix(pose2[0]), np.asarray(pose2[1], np.float64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)
    C2 = R2 @ (-R1.T @ t1) + t2
    ep = np.array([fx * C2[0] / C2[2] + cx, fy * C2[1] / C2[2] + cy])
    return F12.astype(np.float32), ep.astype(np.float32)


@functools.lru_cache(maxsize=None)
def c2_scene(seed=0, n_nb=3):
    """KF1 = frame 0 of S.match_pair("C2", seed); n_nb neighbours of the same PlaneScene at other poses (oracle
    extraction).  About half the features of every frame already have a map point, a third carry a u_right."""
    p = S.match_pair("C2", seed)
    sc, rng = p["sc"], np.random.default_rng(9100 + seed)
    nl = S.CONFIGS["C2"][4]
    scale = np.asarray(p["scale"], np.float32)[:nl]
    case = {"k1": p["k0"], "d1": p["d0"], "scale": scale, "sigma2": (scale * scale).astype(np.float32),
            "has_mp1": (rng.random(len(p["k0"])) < 0.5).astype(np.uint8),
            "ur1": np.where(rng.random(len(p["k0"])) < 0.35, p["k0"]["x"] - 20.0, -1.0).astype(np.float32),
            "fv1": csr(word_nodes(p["d0"]), rng.permutation(len(p["k0"]))), "nbs": [], "only_stereo": False,
            "check_ori": True}
    for k in range(n_nb):
        v, w = S.motion(seed + 10 * (k + 1), 2.0 + k)
        if k == 0:  # mostly forward: the epipole lies in the image, so the mono-mono distance rule bites
            v = v * np.array([0.25, 0.25, 2.0])
        pose = (S.quat_from_rotvec(w), v)
        img = sc.render(pose[0].astype(np.float32), pose[1].astype(np.float32), 3 * seed + 5 + k)
        (k2, d2), _ = S._oracle_extract("C2", img)
        F12, ep = fundamental(sc.cam, p["poses"][0], pose)
        case["nbs"].append({"k2": k2, "d2": d2, "F12": F12, "ep": ep, "D": hamming(p["d0"], d2),
                            "has_mp2": (rng.random(len(k2)) < 0.5).astype(np.uint8),
                            "ur2": np.where(rng.random(len(k2)) < 0.35, k2["x"] - 20.0, -1.0).astype(np.float32),
                            "fv2": csr(word_nodes(d2), rng.permutation(len(k2)))})
    return case


# ------------------------------------------------------------------------------------------ crafted rows
def _kps(xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), ygzfe.KP_DTYPE)
    k["x"], k["y"] = np.asarray(xy, np.float32).T
    k["octave"], k["angle"], k["size"] = octave, angle, 31.0
    return k


def _desc(bits):
    """One descriptor per entry: the first `bits` bits set."""
    d = np.zeros((len(bits), 32), np.uint8)
    for i, b in enumerate(bits):
        d[i] = np.packbits(np.arange(256) < b)
    return d


# l = x1' F = (a, b, c) with a = F[0,0] x1 + F[1,0] y1 + F[2,0]: F_VERTICAL gives a = 1, b = 0, c = -100, the line
# x2 = 100 whatever (x1, y1) is: num = x2 - 100, den = 1, dsqr = (x2 - 100)^2
F_VERTICAL = np.array([[0, 0, 0], [0, 0, 0], [1, 0, -100]], np.float32)


def sigma2_where_float_and_double_disagree():
    """A float32 sigma2 near 1 / 3.84 at which dsqr = 1 passes `dsqr < 3.84 * sigma2` in double and fails it when
    the product is rounded to float32 first (found by a search over adjacent float32 values)."""
    s = F32(1.0 / 3.84)
    for _ in range(64):
        s = np.nextafter(s, F32(0))
    for _ in range(128):
        dbl = 1.0 < 3.84 * float(s)
        flt = bool(F32(1.0) < F32(3.84) * s)
        if dbl != flt:
            return s, dbl, flt
        s = np.nextafter(s, F32(1))
    raise AssertionError("no float32 near 1/3.84 separates the two evaluations")


def _crafted(name, k1, d1, k2, d2, list1=None, list2=None, nodes1=None, nodes2=None, F12=F_VERTICAL, ep=(5000, 5000),
             ur1=None, ur2=None, has_mp1=None, has_mp2=None, sigma2=(1, 4, 16, 64), only_stereo=False):
    n1, n2 = len(k1), len(k2)
    fv1 = csr(np.zeros(n1) if nodes1 is None else nodes1, list1)
    fv2 = csr(np.zeros(n2) if nodes2 is None else nodes2, list2)
    nb = {"k2": k2, "d2": d2, "F12": np.asarray(F12, np.float32), "ep": np.asarray(ep, np.float32),
          "has_mp2": np.zeros(n2, np.uint8) if has_mp2 is None else np.asarray(has_mp2, np.uint8),
          "ur2": None if ur2 is None else np.asarray(ur2, np.float32), "fv2": fv2}
    return {"name": name, "k1": k1, "d1": d1, "ur1": None if ur1 is None else np.asarray(ur1, np.float32),
            "has_mp1": np.zeros(n1, np.uint8) if has_mp1 is None else np.asarray(has_mp1, np.uint8), "fv1": fv1,
            "nbs": [nb], "sigma2": np.asarray(sigma2, np.float32), "scale": np.array([1, 2, 4, 8], np.float32),
            "only_stereo": only_stereo, "check_ori": False}


def crafted_cases():
    """name -> (case, expected matches12 row of the one neighbour).  Every KF1 keypoint is (10, 20); with F_VERTICAL
    a KF2 keypoint passes the epipolar test at octave 0 when (x2 - 100)^2 < 3.84."""
    k1, d1 = _kps([(10, 20)]), _desc([0])
    out = {}
    # two identical descriptors in one node, listed 2, 0, 1: the last position (index 1) wins, not the largest index
    out["tie_last_position"] = (_crafted("tie", k1, d1, _kps([(100, 1), (100, 2), (100, 3)]), _desc([7, 7, 7]),
                                         list2=[2, 0, 1]), [1])
    # the closer candidate lies off the line, the farther one on it
    out["closer_fails_epipolar"] = (_crafted("epi", k1, d1, _kps([(103, 1), (101, 2)]), _desc([3, 30])), [1])
    # TH_LOW: 50 is accepted, 51 is not
    out["dist_50"] = (_crafted("d50", k1, d1, _kps([(100, 1)]), _desc([50])), [0])
    out["dist_51"] = (_crafted("d51", k1, d1, _kps([(100, 1)]), _desc([51])), [-1])
    # mono-mono within 100 * scale of the epipole: (100 - 100)^2 + (1 - 8)^2 = 49 < 100
    near = dict(k2=_kps([(100, 1)]), d2=_desc([5]), ep=(100, 8))
    out["epipole_mono_mono"] = (_crafted("ep-mm", k1, d1, **near), [-1])
    out["epipole_one_stereo"] = (_crafted("ep-st", k1, d1, ur2=[90.0], **near), [0])
    # only_stereo: a mono KF1 feature is left out, a mono candidate is passed over for a farther stereo one
    two1 = (_kps([(10, 20), (10, 21)]), _desc([0, 1]))
    out["only_stereo"] = (_crafted("os", *two1, _kps([(100, 1), (100, 2)]), _desc([2, 20]), ur1=[-1.0, 4.0],
                                   ur2=[-1.0, 90.0], only_stereo=True), [-1, 1])
    out["only_stereo_off"] = (_crafted("os-off", *two1, _kps([(100, 1), (100, 2)]), _desc([2, 20]), ur1=[-1.0, 4.0],
                                       ur2=[-1.0, 90.0]), [0, 0])
    # F12 = 0: den == 0 rejects everything
    out["den_zero"] = (_crafted("den0", k1, d1, _kps([(100, 1)]), _desc([5]), F12=np.zeros((3, 3))), [-1])
    # nodes 4, 7, 9 against 4, 6, 9: KF1's node 7 and KF2's node 6 have no partner (both lower_bound branches)
    out["node_one_side"] = (_crafted("nodes", _kps([(10, 20), (10, 21), (10, 22)]), _desc([0, 0, 0]),
                                     _kps([(100, 1), (100, 2), (100, 3)]), _desc([9, 1, 4]), nodes1=[4, 7, 9],
                                     nodes2=[4, 6, 9]), [0, -1, 2])
    # a map point on either side
    out["has_map_point"] = (_crafted("mp", *two1, _kps([(100, 1), (100, 2)]), _desc([2, 20]), has_mp1=[1, 0],
                                     has_mp2=[1, 0]), [-1, 1])
    # dsqr = 1 (x2 = 101: num = 1, den = 1) against a sigma2 where only the double comparison passes
    s, dbl, flt = sigma2_where_float_and_double_disagree()
    out["double_comparison"] = (_crafted("dbl", k1, d1, _kps([(101, 1)]), _desc([5]), sigma2=(s, 4, 16, 64)),
                                [0 if dbl else -1])
    return out
