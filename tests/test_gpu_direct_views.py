"""FindDirectProjection (find_direct_wave of csrc/align.hip, behind find_direct_projection_batch and
search_direct_batch) against the oracle, bit for bit, on the views of tests/_direct_views.py: zooms
that climb every search level and hit the cap, a zoom-out whose patches leave the reference level,
rolls and an oblique view with A far from the identity.  tests/test_cpu_direct_views.py pins the
oracle itself on the same items.
"""
import functools

import numpy as np
import pytest

import _direct_views as V
import _oracle as O
import _scenes as S

pytestmark = pytest.mark.gpu


class Rig:
    """One configuration's extractor, device keyframes and oracle pyramids."""

    def __init__(self, gpu, cfg):
        W, H, sf, nl = V.CONFIGS[cfg]
        self.gpu, self.cfg, self.nl = gpu, cfg, nl
        self.ex = gpu.ORBextractor(1000, sf, nl, 20, 7)
        self.ov = V.oracle_view(cfg)
        self.kf = [self.ex.ComputePyramid(V.keyframe_image(cfg, k)) for k in (0, 1)]
        self.kf_levels = [self.ov.pyramid(k) for k in (0, 1)]
        self.cam = V._scene(cfg).camera()
        self._cur = {}

    def current(self, name):
        if name not in self._cur:
            self._cur[name] = self.ex.ComputePyramid(V.current_image(self.cfg, name))
        return self._cur[name], self.ov.pyramid(name)

    def both(self, it, name, px0=None, kf=None, kf_levels=None):
        """(GPU, oracle) results of the items `it` on view `name`: each (px, level, ok)."""
        cur, cur_levels = self.current(name)
        px0 = it["px0"] if px0 is None else px0
        got = self.gpu.find_direct_projection_batch(kf or self.kf, cur, self.cam, it["ref_index"], it["kps"],
                                                    it["pt_ref"], it["T_cr"], px0)
        want = self.ov.find_direct(it, kf_levels or self.kf_levels, cur_levels, px0)
        return got, want


_rigs = {}


@pytest.fixture
def rig(gpu, request):
    cfg = request.param
    if cfg not in _rigs:
        _rigs[cfg] = Rig(gpu, cfg)
    return _rigs[cfg]


def assert_same(got, want, nan_rows=None):
    """px, level and ok equal bit for bit; NaN pixels are accepted on `nan_rows` only."""
    (gpx, glv, gok), (opx, olv, ook) = got, want
    assert np.array_equal(glv, olv), np.nonzero(glv != olv)[0][:8]
    assert np.array_equal(gok, ook), np.nonzero(gok != ook)[0][:8]
    nan = np.isnan(opx).any(1)
    if nan_rows is None:
        nan_rows = np.zeros(len(opx), bool)
    assert not (nan & ~nan_rows).any(), "NaN outside the singular rows"
    assert np.array_equal(gpx[~nan_rows].view(np.uint32), opx[~nan_rows].view(np.uint32))
    assert np.array_equal(gpx[nan_rows], opx[nan_rows], equal_nan=True)


def oracle_patches(cfg, it, levels):
    """The oracle's warped 10 x 10 patch of every item."""
    ov = V.oracle_view(cfg)
    A = ov.warp_matrices(it)
    sl = ov.search_levels(A)
    return [ov.warp(A[i], levels[it["ref_index"][i]], kp, sl[i]) for i, kp in enumerate(it["kps"])]


def singular_rows(cfg, it, levels):
    """Items whose H = sum J J^T (Align.cc:37-64) has a float32 cofactor determinant of 0: a flat patch,
    or one whose gradients all point one way.  H's entries are exact in float32 (multiples of 1/4 below 2^22)."""
    f32 = np.float32
    out = []
    for pb in oracle_patches(cfg, it, levels):
        b = pb.astype(np.float64)
        J = np.stack([0.5 * (b[1:9, 2:10] - b[1:9, 0:8]), 0.5 * (b[2:10, 1:9] - b[0:8, 1:9]), np.ones((8, 8))])
        H = np.einsum("ayx,byx->ab", J, J).astype(f32)
        c0 = H[1, 1] * H[2, 2] - H[1, 2] * H[2, 1]
        c1 = H[2, 1] * H[0, 2] - H[2, 2] * H[0, 1]
        c2 = H[0, 1] * H[1, 2] - H[0, 2] * H[1, 1]
        det = f32(f32(c0 * H[0, 0]) + f32(c1 * H[1, 0])) + f32(c2 * H[2, 0])
        out.append(det == 0)
    return np.array(out, bool)


def flat_rows(cfg, it, levels):
    return np.array([pb.min() == pb.max() for pb in oracle_patches(cfg, it, levels)], bool)


def concat(items):
    keys = ("kps", "pt_ref", "T_cr", "px0", "px_true", "ref_index")
    return {k: np.concatenate([it[k] for it in items]) for k in keys}


VIEW_CASES = [(cfg, name) for cfg in V.CONFIGS for name in V.view_names(cfg)]


@pytest.mark.parametrize("rig,name", VIEW_CASES, indirect=["rig"], ids=[f"{c}-{n}" for c, n in VIEW_CASES])
def test_view_bitexact(rig, name):
    it = V.view_items(rig.cfg, name)
    got, want = rig.both(it, name)
    print(rig.cfg, name, "levels", np.bincount(want[1], minlength=rig.nl).tolist(), "converged", int(want[2].sum()),
          "of", len(want[2]))
    assert_same(got, want, singular_rows(rig.cfg, it, rig.kf_levels))
    if name != "cap":
        assert want[2].mean() > 0.3   # the comparison is of alignments that work


@pytest.mark.parametrize("rig", list(V.CONFIGS), indirect=True)
def test_mixed_keyframes_bitexact(rig):
    """One call over K0 and K1 with interleaved ref_index; n around the wave (1 item) and workgroup (4)."""
    name = "roll30"
    a, b = V.view_items(rig.cfg, name, 0), V.view_items(rig.cfg, name, 1)
    m = min(len(a["kps"]), len(b["kps"]))
    both = concat([a, b])
    order = np.stack([np.arange(m), len(a["kps"]) + np.arange(m)], 1).ravel()   # K0, K1, K0, K1, ...
    for n in (1, 3, 4, 5, 257):
        it = {k: v[order[:n]] for k, v in both.items()}
        assert n < 2 or set(it["ref_index"][:2]) == {0, 1}
        got, want = rig.both(it, name)
        assert len(got[0]) == n
        assert_same(got, want, singular_rows(rig.cfg, it, rig.kf_levels))


@pytest.mark.parametrize("rig", list(V.CONFIGS), indirect=True)
def test_border_at_search_level(rig):
    """Guesses on the first-out and first-in columns and rows of the search level (floor(u * inv_scale[sl])
    = 3, 4, w - 5, w - 4; Align.cc:56-59) for items with sl in {1, 2, 3}: the first iteration breaks
    exactly where the oracle's does."""
    name = "zoom1.9"
    it = V.view_items(rig.cfg, name)
    _, cur_levels = rig.current(name)
    sl_all = rig.ov.search_levels(rig.ov.warp_matrices(it))
    isc, sc = rig.ov.inv_scale, rig.ov.scale
    rows, px0, stops = [], [], []
    for sl in (1, 2, 3):
        idx = np.nonzero(sl_all == sl)[0][:8]
        assert len(idx) == 8, sl
        h, w = cur_levels[sl].shape
        cells = [(c, h // 2, c < 4 or c >= w - 4) for c in (3, 4, w - 5, w - 4)] + \
                [(w // 2, r, r < 4 or r >= h - 4) for r in (3, 4, h - 5, h - 4)]
        for i, (cx, cy, stop) in zip(idx, cells):
            g = np.array([(cx + 0.5) * sc[sl], (cy + 0.5) * sc[sl]], np.float32)
            q = g * isc[sl]   # the kernel's and the oracle's float32 product
            assert (int(np.floor(q[0])), int(np.floor(q[1]))) == (cx, cy)
            rows.append(i), px0.append(g), stops.append(stop)
    sub = {k: v[rows] for k, v in it.items() if k not in ("cfg", "view")}
    px0, stops = np.array(px0, np.float32), np.array(stops)
    got, want = rig.both(sub, name, px0)
    assert_same(got, want)
    sls = want[1]
    assert set(sls) == {1, 2, 3}
    untouched = np.array([np.array_equal(want[0][i], (px0[i] * isc[sls[i]]) * sc[sls[i]]) for i in range(len(px0))])
    assert np.array_equal(untouched, stops), (untouched, stops)   # in: the estimate moved; out: it did not
    assert not want[2][stops].any()


@pytest.mark.parametrize("rig", list(V.CONFIGS), indirect=True)
def test_flat_patches(rig):
    """A flat reference patch (wholly outside its level, or over a uniform area of the keyframe) has a
    singular H: not converged, and the pixel (NaN when the first iteration ran) equals the oracle's."""
    name, W, H = "roll30", *V.CONFIGS[rig.cfg][:2]
    it = V.view_items(rig.cfg, name)
    flat = flat_rows(rig.cfg, it, rig.kf_levels)
    assert flat.sum() >= 3
    outside = {k: v[flat] for k, v in it.items() if k not in ("cfg", "view")}
    got, want = rig.both(outside, name)
    assert_same(got, want, np.ones(flat.sum(), bool))
    assert not got[2].any()
    # uniform blocks painted into K0 around four octave-0, level-0 items well inside the image
    x, y = it["kps"]["x"], it["kps"]["y"]
    cand = (it["kps"]["octave"] == 0) & (x > 60) & (x < W - 60) & (y > 60) & (y < H - 60)
    cand &= rig.ov.search_levels(rig.ov.warp_matrices(it)) == 0
    inblock = np.zeros(len(x), bool)
    inblock[np.nonzero(cand)[0][:4]] = True
    assert inblock.sum() == 4
    img = V.keyframe_image(rig.cfg, 0).copy()
    for j, i in enumerate(np.nonzero(inblock)[0]):
        img[int(y[i]) - 25:int(y[i]) + 25, int(x[i]) - 25:int(x[i]) + 25] = 60 + 40 * j
    painted, painted_levels = rig.ex.ComputePyramid(img), rig.ov.pyramid("painted", img)
    sub = {k: v[inblock] for k, v in it.items() if k not in ("cfg", "view")}
    assert flat_rows(rig.cfg, sub, [painted_levels]).all()
    got, want = rig.both(sub, name, kf=[painted], kf_levels=[painted_levels])
    assert_same(got, want, np.ones(inblock.sum(), bool))
    assert not got[2].any() and np.isnan(got[0]).any()


@functools.lru_cache(maxsize=None)
def search_scene(cfg, name="roll90zoom", seed=5):
    """SearchLocalPointsDirect's local-map items on one current view: every point of the K0 and K1
    item sets of the view observed by a random ordered subset of {K0, K1} (same plane point, the
    keypoint in that keyframe with its own octave), px_proj = true projection + U(-1.5, 1.5) px."""
    rng = np.random.default_rng(seed)
    a = V.view_items(cfg, name, 0)
    W, H, sf, nl = V.CONFIGS[cfg]
    cam = V.cam32(cfg)
    scale = V.pyramid_scales(cfg)[0]
    cur = V.view_pose(cfg, name)
    Pw = S.backproject_plane_np(cam, V.KF_POSES[0], np.stack([a["kps"]["x"], a["kps"]["y"]], 1).astype(np.float64))
    item_ptr, ref_index, kps, pt_ref, T_cr = [0], [], [], [], []
    for i in range(len(Pw)):
        for k in rng.permutation(2)[:int(rng.integers(0, 4))]:
            q, t = V.KF_POSES[k]
            px_k, Pc = S.project(cam, q, t, Pw[i:i + 1])
            kp = np.zeros(1, a["kps"].dtype)
            kp["x"], kp["y"] = px_k[0]
            kp["octave"] = int(rng.integers(0, nl))
            kp["size"], kp["angle"] = 31.0 * scale[kp["octave"][0]], -1.0
            qi, ti = S.se3_inv(q, t)
            T = np.zeros(1, a["T_cr"].dtype)
            T["q"], T["t"] = S.se3_mul(cur[0], cur[1], qi, ti)
            ref_index.append(k), kps.append(kp), pt_ref.append(Pc[0]), T_cr.append(T)
        item_ptr.append(len(ref_index))
    px_proj = (a["px_true"] + rng.uniform(-1.5, 1.5, a["px_true"].shape)).astype(np.float32)
    return (np.array(item_ptr, np.int32), np.array(ref_index, np.int32), np.concatenate(kps),
            np.array(pt_ref, np.float32), np.concatenate(T_cr), px_proj)


@pytest.mark.parametrize("rig", list(V.CONFIGS), indirect=True)
def test_search_direct_batch_views(rig):
    """search_direct_batch (k_direct_items) on a rolled and zoomed current frame, several observations
    per point over K0 and K1: matches and pixels bit-exact with the oracle's sequential loop, as in
    test_gpu_align.py::test_search_direct_batch_bitexact."""
    name = "roll90zoom"
    args = search_scene(rig.cfg, name)
    cur, cur_levels = rig.current(name)
    px, m = rig.gpu.search_direct_batch(rig.kf, cur, rig.cam, *args)
    opx, om = O.search_direct(rig.ov.orc, rig.kf_levels, cur_levels, rig.ov.cam, *args)
    assert np.array_equal(m, om)
    assert np.array_equal(px.view(np.uint32), opx.view(np.uint32))
    item_ptr, ref_index = args[0], args[1]
    hit, has_obs = m >= 0, np.diff(item_ptr) > 0
    assert not hit[~has_obs].any()
    assert hit[has_obs].mean() > 0.3, hit[has_obs].mean()
    assert (m[hit] > item_ptr[:-1][hit]).any()              # some fall back to a later keyframe
    assert set(ref_index[m[hit]]) == {0, 1}                 # and both keyframes give matches
    assert (np.diff(item_ptr) >= 2).sum() > 50
