"""GPU stereo vs the oracle.

Frame::ComputeStereoMatches (Frame.cc:509-682): row-band Hamming, 11x11 SAD
sliding window + parabola, median outlier cut — mvuRight / mvDepth bit-exact.
Frame::ComputeStereoFromRGBD (Frame.cc:684-700): bit-exact.
"""
import numpy as np
import pytest

import _oracle as O
import _scenes as S

pytestmark = pytest.mark.gpu


def _extract_pair(gpu, cfg, d):
    W, H, nf, sf, nl, ini, mn = cfg
    ex_l = gpu.ORBextractor(nf, sf, nl, ini, mn)
    ex_r = gpu.ORBextractor(nf, sf, nl, ini, mn)  # the stereo Frame's two extractors
    fl, fr = ex_l.ComputePyramid(d["left"]), ex_r.ComputePyramid(d["right"])
    kl, dl = ex_l.extract(fl)
    kr, dr = ex_r.extract(fr)
    return ex_l, ex_r, fl, fr, kl, dl, kr, dr


@pytest.mark.parametrize("cfg,seed", [("C2", 0), ("C2", 1), ("C1", 2), ("C4", 3)])
def test_stereo_matches_bitexact(gpu, cfg, seed):
    W, H, nf, sf, nl, ini, mn = S.CONFIGS[cfg]
    d = S.stereo_scene(seed, W, H)
    ex_l, ex_r, fl, fr, kl, dl, kr, dr = _extract_pair(gpu, S.CONFIGS[cfg], d)
    ur, dep = gpu.stereo_matches(fl, fr, kl, dl, kr, dr, d["mb"], d["mbf"])
    orc = O.OrbOracle(nf, sf, nl, ini, mn)
    our, odep, osad = O.stereo_matches(orc, orc.pyramid(d["left"]), orc.pyramid(d["right"]), kl, dl, kr, dr, d["mb"],
                                       d["mbf"])
    assert np.array_equal(ur, our)
    assert np.array_equal(dep, odep)
    ok = dep > 0
    assert ok.mean() > 0.3, ok.mean()
    # the recovered depth is the plane's depth at the keypoint (sanity of the restatement)
    sc = d["scene"]
    Pw, _ = sc.map_points(d["pose"][0].astype(np.float32), d["pose"][1].astype(np.float32), kl[ok])
    Pc = np.array([S.quat_rot(d["pose"][0], p) + d["pose"][1] for p in Pw])
    rel = np.abs(dep[ok] - Pc[:, 2]) / Pc[:, 2]
    assert np.median(rel) < 0.05, np.median(rel)
    assert (osad[ok] >= 0).all() and (osad[~ok] == -1).all()


def test_stereo_edges(gpu):
    W, H, nf, sf, nl, ini, mn = S.CONFIGS["C2"]
    d = S.stereo_scene(4, W, H)
    ex_l, ex_r, fl, fr, kl, dl, kr, dr = _extract_pair(gpu, S.CONFIGS["C2"], d)
    orc = O.OrbOracle(nf, sf, nl, ini, mn)
    ll, rl = orc.pyramid(d["left"]), orc.pyramid(d["right"])
    # no left keypoints, no right keypoints, one left keypoint
    ur, dep = gpu.stereo_matches(fl, fr, kl[:0], dl[:0], kr, dr, d["mb"], d["mbf"])
    assert len(ur) == 0
    ur, dep = gpu.stereo_matches(fl, fr, kl, dl, kr[:0], dr[:0], d["mb"], d["mbf"])
    assert (ur == -1).all() and (dep == -1).all()
    for sl in (slice(0, 1), slice(0, 7), slice(3, 300)):
        ur, dep = gpu.stereo_matches(fl, fr, kl[sl], dl[sl], kr, dr, d["mb"], d["mbf"])
        our, odep, _ = O.stereo_matches(orc, ll, rl, kl[sl], dl[sl], kr, dr, d["mb"], d["mbf"])
        assert np.array_equal(ur, our) and np.array_equal(dep, odep)
    # identical images: disparities ~0 (clamped to 0.01 px, Frame.cc:661-664), all SADs 0, so the
    # median cut (SAD >= 2.1 x 0) drops every match, as in the reference
    ur, dep = gpu.stereo_matches(fl, fl, kl, dl, kl, dl, d["mb"], d["mbf"])
    our, odep, _ = O.stereo_matches(orc, ll, ll, kl, dl, kl, dl, d["mb"], d["mbf"])
    assert np.array_equal(ur, our) and np.array_equal(dep, odep)
    with pytest.raises(gpu.YgzfeError):
        gpu.stereo_matches(fl, fr, kl, dl, kr, dr, 0.0, d["mbf"])


def test_batch_stereo_matches_single(gpu):
    import torch
    W, H, nf, sf, nl, ini, mn = S.CONFIGS["C2"]
    scenes = [S.stereo_scene(10 + i, W, H) for i in range(3)]
    frames = np.stack([im for d in scenes for im in (d["left"], d["right"])])
    b = gpu.Batch((nf, sf, nl, ini, mn, 0), 0, W, H, len(frames))
    b.upload(frames)
    b.extract(len(frames))
    b.check()
    cap = b.kp_cap
    dev = torch.device("cuda", 0)
    li = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
    ri = torch.tensor([1, 3, 5], dtype=torch.int32, device=dev)
    ur = torch.zeros((3, cap), dtype=torch.float32, device=dev)
    dep = torch.zeros((3, cap), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.stereo(3, li.data_ptr(), ri.data_ptr(), scenes[0]["mb"], scenes[0]["mbf"], ur.data_ptr(), dep.data_ptr())
    b.check()
    ur, dep = ur.cpu().numpy(), dep.cpu().numpy()
    ex = gpu.ORBextractor(nf, sf, nl, ini, mn)
    for p, d in enumerate(scenes):
        kl, dl = b.result(2 * p)
        kr, dr = b.result(2 * p + 1)
        fl, fr = ex.ComputePyramid(d["left"]), ex.ComputePyramid(d["right"])
        sur, sdep = gpu.stereo_matches(fl, fr, kl, dl, kr, dr, d["mb"], d["mbf"])
        n = len(kl)
        assert np.array_equal(ur[p, :n], sur) and np.array_equal(dep[p, :n], sdep)
        assert (dep[p, :n] > 0).mean() > 0.3


def test_stereo_from_rgbd_bitexact(gpu):
    W, H, nf, sf, nl, ini, mn = S.CONFIGS["C4"]
    rng = np.random.default_rng(7)
    img = S.frame(7, W, H)
    ex = gpu.ORBextractor(nf, sf, nl, ini, mn)
    kps, _ = ex.extract(ex.ComputePyramid(img))
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.2] = 0.0  # holes
    mbf = 40.0  # TUM1.yaml Camera.bf
    ur, dep = gpu.stereo_from_rgbd(depth, kps, mbf)
    our, odep = O.stereo_from_rgbd(depth, kps, mbf)
    assert np.array_equal(ur, our) and np.array_equal(dep, odep)
    assert (dep > 0).mean() > 0.6


# ------------------------------------------------------------------------------------------------------------------
# Crafted one-rule cases and the random sweep of tests/_stereo.py (tests/test_cpu_stereo.py shows, without a GPU,
# that each case lands in the branch it names and which mutation of the restatement each one exposes).
import ctypes as C  # noqa: E402

import _stereo as ST  # noqa: E402

SENTINEL = np.float32(-77.25)
_pairs = {}


def _frames(gpu, geom):
    """(extractor, left frame, right frame, oracle) of a geometry, made once."""
    if geom.name not in _pairs:
        nf, sf, nl, ini, mn = geom.extractor_args
        assert gpu.orb_plan(nf, sf, nl, ini, mn, geom.W, geom.H)["sizes"] == geom.sizes
        ex = gpu.ORBextractor(nf, sf, nl, ini, mn)
        _pairs[geom.name] = (ex, gpu.Frame(ex, geom.W, geom.H), gpu.Frame(ex, geom.W, geom.H),
                             O.OrbOracle(nf, sf, nl, ini, mn))
    return _pairs[geom.name]


def _oracle(orc, case):
    return O.stereo_matches(orc, case["left"], case["right"], case["kl"], case["dl"], case["kr"], case["dr"],
                            float(case["mb"]), float(case["mbf"]))


def _gpu_case(gpu, case):
    ex, fl, fr, orc = _frames(gpu, case["geom"])
    assert [l.shape[::-1] for l in case["left"]] == case["geom"].sizes
    fl.set_levels(case["left"])
    fr.set_levels(case["right"])
    ur, dep = gpu.stereo_matches(fl, fr, case["kl"], case["dl"], case["kr"], case["dr"], float(case["mb"]),
                                 float(case["mbf"]))
    return ur, dep, _oracle(orc, case)


@pytest.mark.parametrize("geometry", sorted(ST.GEOMETRIES))
def test_stereo_crafted_cases(gpu, geometry):
    n = 0
    for name, case in ST.crafted_cases().items():
        if case["geom"].name != geometry:
            continue
        n += 1
        ur, dep, (our, odep, _) = _gpu_case(gpu, case)
        assert np.array_equal(ur, our) and np.array_equal(dep, odep), name
        for il, code in enumerate(case["codes"]):       # what the case itself states
            if code not in ("KEPT", "KEPT_CLAMPED"):
                assert ur[il] == -1 and dep[il] == -1, (name, il, code)
        for il, (u, d, _) in case["values"].items():
            assert ur[il] == np.float32(u) and dep[il] == np.float32(d), (name, il)
    assert n >= 20


def test_stereo_set_levels_is_set_level(gpu):
    """Frame.set_levels (one DMA) leaves the pyramid Frame.set_level writes level by level."""
    case = ST.crafted_cases()["inexact_scale_products"]
    ex, fl, fr, _ = _frames(gpu, case["geom"])
    fl.set_levels(case["left"])
    for l, img in enumerate(case["right"]):
        fr.set_level(l, img)
    assert all(np.array_equal(a, b) for a, b in zip(fl.levels(), case["left"]))
    assert all(np.array_equal(a, b) for a, b in zip(fr.levels(), case["right"]))
    fl.set_levels(case["right"][2:5], first=2)
    assert all(np.array_equal(a, b) for a, b in zip(fl.levels(), case["left"][:2] + case["right"][2:5] + case["left"][5:]))


@pytest.mark.parametrize("geometry", sorted(ST.GEOMETRIES))
def test_stereo_random_sweep(gpu, geometry):
    kept = 0
    for seed in ST.RANDOM_SEEDS:
        ur, dep, (our, odep, _) = _gpu_case(gpu, ST.random_case(seed, geometry))
        assert np.array_equal(ur, our) and np.array_equal(dep, odep), seed
        kept += int((dep > 0).sum())
    assert kept >= 20 * len(ST.RANDOM_SEEDS)


def _bound_batch(gpu, geom, frames, max_frames):
    """A batch of the geometry whose pyramids, keypoints, descriptors and counts are caller-owned torch buffers,
    filled from `frames` = [(levels, kps, desc)]; rows past a frame's count hold other, valid keypoints."""
    import torch
    nf, sf, nl, ini, mn = geom.extractor_args
    b = gpu.Batch((nf, sf, nl, ini, mn, 0), 0, geom.W, geom.H, max_frames)
    cap = b.kp_cap
    base = b.frames_ptr()
    off = []
    for l in range(geom.nlevels):
        p = C.c_void_p()
        assert gpu.lib().ygzfe_batch_level(b.h, 0, l, C.byref(p), None, None, None) == gpu.OK
        off.append(p.value - base)
    rng = np.random.default_rng(3)
    pyr = rng.integers(0, 256, (max_frames, b.frame_pitch), dtype=np.uint8)
    kps = np.zeros((max_frames, cap), gpu.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, geom.W, kps.shape), rng.uniform(0, geom.H, kps.shape)
    kps["octave"] = rng.integers(0, geom.nlevels, kps.shape)
    desc = rng.integers(0, 256, (max_frames, cap, 32), dtype=np.uint8)
    counts = np.zeros(max_frames, np.int32)
    for f, (levels, k, d) in enumerate(frames):
        assert len(k) <= cap
        for l, img in enumerate(levels):
            assert img.shape[::-1] == geom.sizes[l] and off[l] + img.size <= b.frame_pitch
            pyr[f, off[l]:off[l] + img.size] = img.ravel()
        kps[f, :len(k)], desc[f, :len(k)], counts[f] = k, d, len(k)
    dev = torch.device("cuda", 0)
    t = dict(pyr=torch.from_numpy(pyr).to(dev), kps=torch.from_numpy(kps.view(np.uint8).reshape(max_frames, -1)).to(dev),
             desc=torch.from_numpy(desc).to(dev), counts=torch.from_numpy(counts).to(dev))
    torch.cuda.synchronize()
    b.bind(pyramids=t["pyr"].data_ptr(), kps=t["kps"].data_ptr(), desc=t["desc"].data_ptr(),
           counts=t["counts"].data_ptr())
    return b, t, kps, counts


def test_batch_stereo_crafted(gpu):
    """ygzfe_batch_stereo on caller-owned buffers: counts far apart, an empty left and an empty right frame, a frame
    that is left in one pair and right in another, a pair listed twice, a frame against itself; rows past the left
    count keep what the caller wrote."""
    import torch
    geom = ST.GEOMETRIES["x2"]
    r0, r1 = ST.random_case(0, "x2"), ST.random_case(1, "x2")
    small = ST.crafted_cases()["disparity_zero_clamped"]
    frames = [(r0["left"], r0["kl"], r0["dl"]), (r0["right"], r0["kr"], r0["dr"]),
              (small["left"], small["kl"], small["dl"]), (small["right"], small["kr"], small["dr"]),
              (r1["left"], r1["kl"][:0], r1["dl"][:0]), (r1["right"], r1["kr"][:40], r1["dr"][:40])]
    b, t, _, counts = _bound_batch(gpu, geom, frames, len(frames))
    assert counts.tolist() == [300, len(r0["kr"]), len(small["kl"]), len(small["kr"]), 0, 40] and len(small["kl"]) < 10
    pairs = [(0, 1), (2, 3), (2, 1), (0, 3), (4, 1), (0, 4), (1, 0), (0, 1), (0, 0), (5, 5), (4, 4)]
    cap, dev = b.kp_cap, torch.device("cuda", 0)
    li = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=dev)
    ri = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=dev)
    ur = torch.full((len(pairs), cap), float(SENTINEL), dtype=torch.float32, device=dev)
    dep = torch.full((len(pairs), cap), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.stereo(len(pairs), li.data_ptr(), ri.data_ptr(), float(geom.mb), float(geom.mbf), ur.data_ptr(), dep.data_ptr())
    b.check()
    torch.cuda.synchronize()
    ur, dep = ur.cpu().numpy(), dep.cpu().numpy()
    orc = O.OrbOracle(*geom.extractor_args)
    kept = 0
    for p, (l, r) in enumerate(pairs):
        (ll, kl, dl), (rl, kr, dr) = frames[l], frames[r]
        our, odep, _ = O.stereo_matches(orc, ll, rl, kl, dl, kr, dr, float(geom.mb), float(geom.mbf))
        n = len(kl)
        assert np.array_equal(ur[p, :n], our) and np.array_equal(dep[p, :n], odep), (p, l, r)
        assert (ur[p, n:] == SENTINEL).all() and (dep[p, n:] == SENTINEL).all(), (p, l, r)
        kept += int((odep > 0).sum())
    assert np.array_equal(ur[0], ur[7]) and np.array_equal(dep[0], dep[7])
    assert kept > 60
    del b


RGBD_VALUES = np.array([0.0, -1.5, np.nan, np.inf, 1e-40, 0.75, 2.5, 3.0e3], np.float32)   # 1e-40: a denormal
PAD = np.float32(5.0)   # in the padding: a depth the kernel would accept, were it to read there


def _rgbd_image(rng, W, H, stride, tail):
    """A depth image of RGBD_VALUES in a buffer of H * stride + tail floats whose padding holds PAD."""
    buf = np.full(H * stride + tail, PAD, np.float32)
    img = RGBD_VALUES[rng.integers(0, len(RGBD_VALUES), (H, W))]
    rows = buf[:H * stride].reshape(H, stride)
    rows[:, :W] = img
    return buf, img


def _rgbd_keypoints(gpu, rng, W, H, n):
    """n keypoints: the edges first (W - 0.5 and H - 0.5 are the last column and row, W and H are outside, -0.5
    truncates to 0 and is inside, -1.0 is outside), then random positions."""
    edge = [(W - 0.5, 3.0), (3.0, H - 0.5), (W - 0.5, H - 0.5), (float(W), 3.0), (3.0, float(H)), (-0.5, 3.0),
            (3.0, -0.5), (-0.5, -0.5), (-1.0, 3.0), (3.0, -1.0), (0.0, 0.0), (float(W), H - 0.5), (W - 0.5, float(H))]
    k = np.zeros(n, gpu.KP_DTYPE)
    k["x"], k["y"] = rng.uniform(0, W, n), rng.uniform(0, H, n)
    m = min(n, len(edge))
    k["x"][:m], k["y"][:m] = [e[0] for e in edge[:m]], [e[1] for e in edge[:m]]
    return k


def test_batch_stereo_rgbd(gpu):
    import torch
    geom = ST.GEOMETRIES["x2"]
    W, H = geom.W, geom.H
    nf, sf, nl, ini, mn = geom.extractor_args
    b = gpu.Batch((nf, sf, nl, ini, mn, 0), 0, W, H, 4)
    cap = b.kp_cap
    rng = np.random.default_rng(11)
    counts = np.array([0, 1, cap // 2, cap], np.int32)
    kps = np.stack([_rgbd_keypoints(gpu, rng, W, H, cap) for _ in range(4)])
    kps[1][0] = kps[1][2]       # the one keypoint of frame 1: the last pixel
    stride, tail = W + 5, 7
    imgs = [_rgbd_image(rng, W, H, stride, tail) for _ in range(4)]
    pitch = H * stride + tail
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(np.stack([i[0] for i in imgs])).to(dev)
    d_kps = torch.from_numpy(kps.view(np.uint8).reshape(4, -1)).to(dev)
    d_cnt = torch.from_numpy(counts).to(dev)
    ur = torch.full((4, cap), float(SENTINEL), dtype=torch.float32, device=dev)
    dep = torch.full((4, cap), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.bind(kps=d_kps.data_ptr(), counts=d_cnt.data_ptr())
    mbf = 40.0
    with pytest.raises(gpu.YgzfeError):
        b.stereo_rgbd(5, d_img.data_ptr(), pitch, stride, mbf, ur.data_ptr(), dep.data_ptr())      # > max_frames
    with pytest.raises(gpu.YgzfeError):
        b.stereo_rgbd(4, d_img.data_ptr(), pitch, W - 1, mbf, ur.data_ptr(), dep.data_ptr())       # stride < width
    b.stereo_rgbd(4, d_img.data_ptr(), pitch, stride, mbf, ur.data_ptr(), dep.data_ptr(), b.stream)
    b.check()
    torch.cuda.synchronize()
    ur, dep = ur.cpu().numpy(), dep.cpu().numpy()
    seen = set()
    for f in range(4):
        n = counts[f]
        our, odep = O.stereo_from_rgbd(imgs[f][1], kps[f][:n], mbf)
        assert np.array_equal(ur[f, :n], our) and np.array_equal(dep[f, :n], odep), f
        assert (ur[f, n:] == SENTINEL).all() and (dep[f, n:] == SENTINEL).all(), f
        assert not (odep == PAD).any()
        seen |= set(odep.tolist())
    assert {-1.0, 0.75, 2.5, 3.0e3, float("inf"), float(np.float32(1e-40))} <= seen
    del b


def test_stereo_from_rgbd_padded_rows(gpu):
    """ygzfe_stereo_from_rgbd with stride > width; the buffer ends with the last row's `width` floats."""
    W, H, stride = 88, 64, 101
    rng = np.random.default_rng(12)
    buf, img = _rgbd_image(rng, W, H, stride, 0)
    buf = buf[:(H - 1) * stride + W].copy()
    kps = _rgbd_keypoints(gpu, rng, W, H, 400)
    ur, dep = np.full(400, SENTINEL, np.float32), np.full(400, SENTINEL, np.float32)
    mbf = 40.0
    rc = gpu.lib().ygzfe_stereo_from_rgbd(0, gpu._p(buf), W, H, stride, gpu._p(kps), len(kps), mbf, gpu._p(ur),
                                          gpu._p(dep))
    assert rc == gpu.OK
    our, odep = O.stereo_from_rgbd(img, kps, mbf)
    assert np.array_equal(ur, our) and np.array_equal(dep, odep)
    assert not (dep == PAD).any()
    assert {-1.0, 0.75, float("inf"), float(np.float32(1e-40))} <= set(dep.tolist())
    assert gpu.lib().ygzfe_stereo_from_rgbd(0, gpu._p(buf), W, H, W - 1, gpu._p(kps), len(kps), mbf, gpu._p(ur),
                                            gpu._p(dep)) == gpu.EINVAL
