"""ygzfe.search_local_map_direct: the frustum cull, the keyframe choice and the item list on the
GPU, against the float32 restatement of tests/_direct_map.py (bit-exact) and, from the
restatement's compacted items, against the existing search_local_points_direct and the oracle."""
import functools

import numpy as np
import pytest

import _direct_map as DM
import _oracle as O
import _scenes as S

pytestmark = pytest.mark.gpu

C2 = S.CONFIGS["C2"]


@functools.lru_cache(maxsize=None)
def _case(seed, **kw):
    """A scene, its restatement and the oracle's result per threshold: computed once, never changed."""
    m = DM.map_scene(seed, **kw)
    return m, DM.restate(m, m["scene"].cam), {}


def _frames(gpu, m):
    W, H, nf, sf, nl, ini, mn = C2
    ex = gpu.ORBextractor(nf, sf, nl, ini, mn)
    kf_fr = [ex.ComputePyramid(im) for im in m["kf_images"]]
    for f, kps in zip(kf_fr, m["kp_tables"]):
        assert f.keypoint_count() == -1
        f.set_keypoints(kps)
        assert f.keypoint_count() == len(kps)
    return ex, kf_fr, ex.ComputePyramid(m["cur_image"])


def _oracle(m, r, oracle_cache, th):
    if th not in oracle_cache:
        W, H, nf, sf, nl, ini, mn = C2
        orc = O.OrbOracle(nf, sf, nl, ini, mn)
        kl, cl = [orc.pyramid(im) for im in m["kf_images"]], orc.pyramid(m["cur_image"])
        oracle_cache[th] = O.search_local_points_direct(orc, kl, cl, O.Cam(*m["scene"].cam), r["n_cache"],
                                                        *DM.items_of(r), cache_hit_th=th)
    return oracle_cache[th]


def _check(gpu, m, r, oracle_cache, kf_fr, cur_fr, th, n_sel=5, with_oracle=True):
    """The device set-up path against the restatement, then against the existing call and the
    oracle fed with the restatement's items.  Returns the candidate-row result."""
    cam = m["scene"].camera()
    n = len(m["world"])
    res, cs, ran = gpu.search_local_map_direct(kf_fr, cur_fr, cam, DM.gpu_view(m), *DM.call_args(m), n_sel=n_sel,
                                               cache_hit_th=th)
    assert np.array_equal(res["status"] == gpu.DIRECT_CULLED, r["culled"])
    iv = ~r["culled"]
    for k in ("proj", "view_cos", "dist"):
        assert res[k][iv].tobytes() == r[k][iv].tobytes(), k
    refs = [("existing call", gpu.search_local_points_direct(kf_fr, cur_fr, cam, r["n_cache"], *DM.items_of(r),
                                                             cache_hit_th=th))]
    if with_oracle:
        refs.append(("oracle", _oracle(m, r, oracle_cache, th)))
    for name, (px, matched, status, rcs, rran) in refs:
        st, pxo, mkf, mkp = DM.expand(r, n, px, matched, status)
        assert np.array_equal(res["status"], st), (name, th)
        assert res["px_out"].tobytes() == pxo.tobytes(), (name, th)
        assert np.array_equal(res["matched_kf"], mkf) and np.array_equal(res["matched_kp"], mkp), (name, th)
        assert (cs, ran) == (rcs, rran), (name, th)
    return res, cs, ran


@pytest.mark.parametrize("seed", [0, 2])
def test_local_map_direct_bitexact(gpu, seed):
    """10 keyframes with shuffled kf_ids (one excluded as bad, one as the last keyframe: with 0..9
    observations per point, only a table of more than 7 keyframes lets a point have more than 5
    eligible ones), clustered points, ~10 % skipped, and candidates that each cull rule rejects."""
    m, r, oc = _case(seed)
    ex, kf_fr, cur_fr = _frames(gpu, m)
    assert m["kf_excluded"].sum() == 2 and (np.diff(m["kf_id"]) < 0).any() and (np.diff(m["kf_id"]) > 0).any()
    assert 0.05 <= m["skip"].mean() <= 0.15
    for rule in DM.CULL_RULES:
        assert (r["rule"] == rule).sum() >= 5, rule
    iv = ~r["culled"]
    assert (r["n_eligible"][iv] > 5).mean() >= 0.2
    none = iv & (r["n_eligible"] == 0)
    assert none.any()
    seen = set()
    for th in (10 ** 6, 20):
        res, cs, ran = _check(gpu, m, r, oc, kf_fr, cur_fr, th)
        seen.add(ran)
        # without an eligible observation: FAILED, unless the grid skipped the cache row first or
        # the local phase did not run
        nc = m["n_cache"]
        st_c, st_l = res["status"][:nc][none[:nc]], res["status"][nc:][none[nc:]]
        assert np.isin(st_c, (gpu.DIRECT_FAILED, gpu.DIRECT_GRID_SKIP)).all() and (st_c == gpu.DIRECT_FAILED).any()
        assert len(st_l) and (st_l == (gpu.DIRECT_FAILED if ran else gpu.DIRECT_NOT_RUN)).all()
        cache = iv[:m["n_cache"]]
        assert (res["status"][:m["n_cache"]][cache] == gpu.DIRECT_GRID_SKIP).mean() >= 0.1
        assert (res["status"] == gpu.DIRECT_MATCHED).sum() > 200
    assert seen == {True, False}


def _tiny(gpu):
    """One keyframe image at the identity pose, also the current image; a table of 4 rows on it."""
    W, H, nf, sf, nl, ini, mn = C2
    sc = S.PlaneScene(2)
    img = sc.render(np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32), 1)
    ex = gpu.ORBextractor(nf, sf, nl, ini, mn)
    kf, cur = ex.ComputePyramid(img), ex.ComputePyramid(img)
    fx, fy, cx, cy = sc.cam
    kps = np.zeros(3, gpu.KP_DTYPE)
    kps["x"], kps["y"], kps["size"], kps["angle"] = cx, cy, 31.0, -1.0
    kf.set_keypoints(kps)
    n_kf = 4
    T_rw = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(np.float32), (n_kf, 1))
    T_cr = np.zeros(n_kf, gpu.SE3_DTYPE)
    T_cr["q"][:, 3] = 1.0
    tab = dict(kf_frames=[kf] * n_kf, kf_id=np.array([40, 90, 70, 10], np.int64),
               kf_excluded=np.array([0, 1, 0, 0], np.uint8), T_rw=T_rw, T_cr=T_cr)
    return sc, ex, cur, tab


def _tiny_call(gpu, sc, cur, tab, world, bounds=None, n_sel=5, min_dist=0.0, obs=None, **kw):
    W, H = C2[:2]
    world = np.asarray(world, np.float32).reshape(-1, 3)
    n = len(world)
    view = gpu.DirectView.make(np.eye(3), np.zeros(3), np.zeros(3), bounds or (0, W, 0, H), 0.5, 40.0)
    normal = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    obs = obs if obs is not None else [[(0, 0)]] * n
    obs_ptr = np.cumsum([0] + [len(o) for o in obs]).astype(np.int32)
    flat = [p for o in obs for p in o]
    obs_kf = np.array([p[0] for p in flat], np.int32)
    obs_kp = np.array([p[1] for p in flat], np.int32)
    return gpu.search_local_map_direct(tab["kf_frames"], cur, sc.camera(), view, tab["kf_id"], tab["kf_excluded"],
                                       tab["T_rw"], tab["T_cr"], kw.pop("n_cache", n), world, normal,
                                       np.full(n, min_dist, np.float32), np.full(n, 100.0, np.float32),
                                       kw.pop("skip", np.zeros(n, np.uint8)), obs_ptr, obs_kf, obs_kp, n_sel=n_sel,
                                       cache_hit_th=10 ** 6, **kw)


def test_local_map_direct_boundaries(gpu):
    """T_cw = identity and P = (0, 0, z) project to (cx, cy) exactly: a bound equal to it keeps the
    point, the next float32 past it culls it.  P == Ow gives NaN everywhere and is culled (the
    stated deviation); a slightly negative Pc_z is culled; n_sel = 1 keeps the largest eligible id."""
    sc, ex, cur, tab = _tiny(gpu)
    W, H = C2[:2]
    fx, fy, cx, cy = (np.float32(c) for c in sc.cam)
    up, down = (lambda x: np.nextafter(x, np.float32(np.inf))), (lambda x: np.nextafter(x, np.float32(-np.inf)))
    P = [[0, 0, 3.0]]
    full = (np.float32(0), np.float32(W), np.float32(0), np.float32(H))
    cases = [(0, cx, up(cx)), (1, cx, down(cx)), (2, cy, up(cy)), (3, cy, down(cy))]
    for slot, keep, cull in cases:
        for value, want_culled in ((keep, False), (cull, True)):
            b = list(full)
            b[slot] = value
            res, _, _ = _tiny_call(gpu, sc, cur, tab, P, bounds=tuple(b))
            assert (res["status"][0] == gpu.DIRECT_CULLED) == want_culled, (slot, value)
            if not want_culled:
                assert res["proj"][0, 0] == cx and res["proj"][0, 1] == cy
                assert res["dist"][0] == np.float32(3.0) and res["view_cos"][0] == np.float32(1.0)
                assert res["proj"][0, 2] == cx - np.float32(40.0) * (np.float32(1.0) / np.float32(3.0))
    # rows: a regular point, P == Ow, Pc_z slightly negative (min_dist 0: only the stated rule rejects)
    res, cs, ran = _tiny_call(gpu, sc, cur, tab, [[0, 0, 3.0], [0, 0, 0], [0, 0, -1e-6]])
    assert res["status"].tolist() == [gpu.DIRECT_MATCHED, gpu.DIRECT_CULLED, gpu.DIRECT_CULLED]
    assert res["matched_kf"].tolist() == [0, -1, -1] and res["matched_kp"].tolist() == [0, -1, -1]
    assert cs == 1 and ran
    # n_sel = 1: ids 40, 90 (excluded), 70, 10 -> row 2, whatever the order of the list
    for obs in ([(0, 1), (1, 0), (2, 2), (3, 0)], [(3, 0), (2, 2), (1, 0), (0, 1)], [(2, 2), (0, 1)]):
        res, _, _ = _tiny_call(gpu, sc, cur, tab, P, n_sel=1, obs=[obs])
        assert res["status"][0] == gpu.DIRECT_MATCHED
        assert (res["matched_kf"][0], res["matched_kp"][0]) == (2, 2)


def test_local_map_direct_scan_crosses_blocks(gpu):
    """> 2,500 candidates (11 set-up workgroups: item_ptr is a scan across them) with a cache
    phase of > 2,048 rows both before and after the cull (two replay chunks)."""
    m, r, oc = _case(4, n_kf=4, max_obs=4, cluster=4, cache_frac=0.7)
    assert len(m["world"]) >= 2500 and m["n_cache"] > 2048 and r["n_cache"] > 2048
    ex, kf_fr, cur_fr = _frames(gpu, m)
    res, cs, ran = _check(gpu, m, r, oc, kf_fr, cur_fr, 10 ** 6)
    assert (res["status"][2048:m["n_cache"]] == gpu.DIRECT_GRID_SKIP).any()
    assert r["item_ptr"][-1] > 2000


def test_local_map_direct_edges(gpu):
    sc, ex, cur, tab = _tiny(gpu)
    # no candidates
    res, cs, ran = _tiny_call(gpu, sc, cur, tab, np.zeros((0, 3)))
    assert len(res["status"]) == 0 and cs == 0 and ran
    # every candidate culled: no item exists on the device
    P = np.tile(np.array([[0, 0, 3.0]], np.float32), (300, 1))
    res, cs, ran = _tiny_call(gpu, sc, cur, tab, P, skip=np.ones(300, np.uint8))
    assert (res["status"] == gpu.DIRECT_CULLED).all() and cs == 0 and ran
    assert (res["matched_kf"] == -1).all() and (res["px_out"] == 0).all()
    # a keyframe table of one row
    m, r, oc = _case(3, n_kf=1, max_obs=1, n_points=40, cluster=1, n_special=5)
    _, kf_fr, cur_fr = _frames(gpu, m)
    res, _, _ = _check(gpu, m, r, oc, kf_fr, cur_fr, 10 ** 6)
    assert (res["status"] == gpu.DIRECT_MATCHED).any()
    # the host checks
    one = [[0, 0, 3.0]]
    with pytest.raises(gpu.YgzfeError):
        _tiny_call(gpu, sc, cur, tab, one, obs=[[(4, 0)]])      # obs_kf out of range
    with pytest.raises(gpu.YgzfeError):
        _tiny_call(gpu, sc, cur, tab, one, obs=[[(0, 3)]])      # obs_kp past the keypoint count
    with pytest.raises(gpu.YgzfeError):
        _tiny_call(gpu, sc, cur, tab, one, n_sel=9)
    with pytest.raises(gpu.YgzfeError):
        _tiny_call(gpu, sc, cur, tab, one, n_sel=0)
    bare = dict(tab, kf_frames=[ex.ComputePyramid(sc.render(np.array([0, 0, 0, 1], np.float32),
                                                            np.zeros(3, np.float32), 1))] * 4)
    with pytest.raises(gpu.YgzfeError):
        _tiny_call(gpu, sc, cur, bare, one)                     # a keyframe without keypoints
    with pytest.raises(gpu.YgzfeError):
        bad = np.zeros(1, gpu.KP_DTYPE)
        bad["octave"] = 4
        tab["kf_frames"][0].set_keypoints(bad)                  # an octave outside the pyramid
    assert tab["kf_frames"][0].keypoint_count() == 3
    res, cs, ran = _tiny_call(gpu, sc, cur, tab, one)
    assert res["status"].tolist() == [gpu.DIRECT_MATCHED] and cs == 1
