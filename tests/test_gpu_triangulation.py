"""ygzfe_search_for_triangulation(_batch) against the restatement of ORBmatcher::SearchForTriangulation
(tests/_triangulation.py; its two forms are compared in tests/test_cpu_triangulation.py): matches12 and nmatches
bit-exact on the three-neighbour C2 scene and on every crafted row, the batch against single calls, empty inputs,
uploads still in flight, repeat calls and refused arguments."""
import numpy as np
import pytest

import _triangulation as T

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, 752.0, 0.0, 480.0)
FLAGS = [(False, True), (False, False), (True, True), (True, False)]  # (only_stereo, check_ori)


def frames_of(gpu, case):
    kf1 = gpu.MatchFrame(0).set(case["k1"], case["d1"], case["ur1"], BOUNDS)
    return kf1, [gpu.MatchFrame(0).set(nb["k2"], nb["d2"], nb["ur2"], BOUNDS) for nb in case["nbs"]]


def batch(gpu, case, kf1, kf2s, nbs=None):
    nbs = case["nbs"] if nbs is None else nbs
    return gpu.search_for_triangulation_batch(
        kf1, kf2s, case["has_mp1"], case["fv1"], [nb["has_mp2"] for nb in nbs], [nb["fv2"] for nb in nbs],
        [nb["F12"] for nb in nbs], [nb["ep"] for nb in nbs], case["sigma2"], case["scale"], case["only_stereo"],
        case["check_ori"])


def single(gpu, case, kf1, kf2, nb):
    return gpu.search_for_triangulation(kf1, kf2, case["has_mp1"], case["fv1"], nb["has_mp2"], nb["fv2"], nb["F12"],
                                        nb["ep"], case["sigma2"], case["scale"], case["only_stereo"], case["check_ori"])


@pytest.fixture(scope="module")
def scene(gpu):
    case = T.c2_scene(0)
    want = {fl: T.search_loops(T.with_flags(case, *fl)) for fl in FLAGS}
    kf1, kf2s = frames_of(gpu, case)
    return case, want, kf1, kf2s


@pytest.mark.parametrize("only_stereo,check_ori", FLAGS)
def test_scene_bit_exact_and_batch_equals_single_calls(gpu, scene, only_stereo, check_ori):
    base, want, kf1, kf2s = scene
    case = T.with_flags(base, only_stereo, check_ori)
    wm, wn = want[(only_stereo, check_ori)]
    m12, n = batch(gpu, case, kf1, kf2s)
    print("nmatches", n.tolist(), "want", wn.tolist())
    assert m12.dtype == np.int32 and m12.shape == wm.shape
    assert np.array_equal(n, wn) and np.array_equal(m12, wm)
    for k, nb in enumerate(case["nbs"]):
        ms, ns = single(gpu, case, kf1, kf2s[k], nb)
        assert ns == wn[k] and np.array_equal(ms, wm[k])
    m2, n2 = batch(gpu, case, kf1, kf2s)  # a second call: identical
    assert np.array_equal(m2, m12) and np.array_equal(n2, n)


CRAFTED = T.crafted_cases()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_row(gpu, name):
    case, want = CRAFTED[name]
    kf1, kf2s = frames_of(gpu, case)
    wm, wn = T.search_loops(case)
    assert wm.tolist() == [want]
    m12, n = batch(gpu, case, kf1, kf2s)
    assert np.array_equal(m12, wm) and np.array_equal(n, wn)
    ms, ns = single(gpu, case, kf1, kf2s[0], case["nbs"][0])
    assert np.array_equal(ms, wm[0]) and ns == wn[0]


def test_crafted_rows_with_the_orientation_check(gpu):
    """Four matches whose rotation bins are 0, 0, 0 and 6: ComputeThreeMaxima keeps bin 0 alone (1 < 0.1 * 3 fails,
    so bin 6 stays) -- and with eleven in bin 0 the single one goes (1 < 1.1)."""
    for n0, keeps in ((3, True), (11, False)):
        n = n0 + 1
        k1 = T._kps([(10, 20 + i) for i in range(n)], angle=200.0)
        k2 = T._kps([(100, 1 + i) for i in range(n)], angle=200.0)
        k2["angle"][n0] = 20.0  # rot = 180 -> bin 6
        d = np.zeros((n, 32), np.uint8)
        d[:, 0] = np.arange(n)  # distinct nodes keep the pairs apart
        case = T._crafted("ori", k1, d, k2, d, nodes1=np.arange(n), nodes2=np.arange(n))
        case["check_ori"] = True
        wm, wn = T.search_loops(case)
        assert wn.tolist() == [n if keeps else n0] and (wm[0, n0] == n0) == keeps
        kf1, kf2s = frames_of(gpu, case)
        m12, nm = batch(gpu, case, kf1, kf2s)
        assert np.array_equal(m12, wm) and np.array_equal(nm, wn)


def test_empty_inputs(gpu, scene):
    base, want, kf1, kf2s = scene
    case = T.with_flags(base, False, True)
    wm, wn = want[(False, True)]
    n1 = len(case["k1"])
    # no neighbour
    m12, n = batch(gpu, case, kf1, [], nbs=[])
    assert m12.shape == (0, n1) and n.shape == (0,)
    # an empty KF1
    e1 = gpu.MatchFrame(0).set(case["k1"][:0], case["d1"][:0], None, BOUNDS)
    empty_fv = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    ecase = dict(case, k1=case["k1"][:0], d1=case["d1"][:0], ur1=None, has_mp1=np.zeros(0, np.uint8), fv1=empty_fv)
    m12, n = batch(gpu, ecase, e1, kf2s)
    assert m12.shape == (3, 0) and n.tolist() == [0, 0, 0]
    # an empty neighbour in the middle of a batch: the others as before
    e2 = gpu.MatchFrame(0).set(case["k1"][:0], case["d1"][:0], None, BOUNDS)
    enb = dict(case["nbs"][1], k2=case["k1"][:0], d2=case["d1"][:0], ur2=None, has_mp2=np.zeros(0, np.uint8),
               fv2=empty_fv)
    m12, n = batch(gpu, case, kf1, [kf2s[0], e2, kf2s[2]], nbs=[case["nbs"][0], enb, case["nbs"][2]])
    assert n.tolist() == [wn[0], 0, wn[2]] and (m12[1] == -1).all()
    assert np.array_equal(m12[0], wm[0]) and np.array_equal(m12[2], wm[2])
    # empty FeatureVectors: on KF1, then on every neighbour
    m12, n = batch(gpu, dict(case, fv1=empty_fv), kf1, kf2s)
    assert (m12 == -1).all() and m12.shape == wm.shape and n.tolist() == [0, 0, 0]
    m12, n = batch(gpu, case, kf1, kf2s, nbs=[dict(nb, fv2=empty_fv) for nb in case["nbs"]])
    assert (m12 == -1).all() and n.tolist() == [0, 0, 0]
    ms, ns = single(gpu, case, kf1, kf2s[0], dict(case["nbs"][0], fv2=empty_fv))
    assert (ms == -1).all() and ns == 0


def test_uploads_in_flight(gpu, scene):
    """The call right after MatchFrame.set on every frame (the uploads are asynchronous, each on its frame's
    stream), then one neighbour set again with other content."""
    base, want, _, _ = scene
    case = T.with_flags(base, False, True)
    wm, wn = want[(False, True)]
    kf1, kf2s = frames_of(gpu, case)
    m12, n = batch(gpu, case, kf1, kf2s)
    assert np.array_equal(m12, wm) and np.array_equal(n, wn)
    # neighbour 1 becomes a copy of neighbour 2 (content, map points, FeatureVector, geometry)
    nb2 = case["nbs"][2]
    kf2s[1].set(nb2["k2"], nb2["d2"], nb2["ur2"], BOUNDS)
    m12, n = batch(gpu, case, kf1, kf2s, nbs=[case["nbs"][0], nb2, nb2])
    assert n.tolist() == [wn[0], wn[2], wn[2]]
    assert np.array_equal(m12[0], wm[0]) and np.array_equal(m12[1], wm[2]) and np.array_equal(m12[2], wm[2])


def raw_single(gpu, case, kf1, kf2, nb, m12, nm):
    """ygzfe_search_for_triangulation itself, with the caller's output arrays -> its return code."""
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    keep = [i32(a) for a in case["fv1"]] + [i32(a) for a in nb["fv2"]] + [
        f32(nb["F12"]), f32(nb["ep"]), f32(case["sigma2"]), f32(case["scale"]),
        np.ascontiguousarray(case["has_mp1"], np.uint8), np.ascontiguousarray(nb["has_mp2"], np.uint8)]
    n1, p1, f1, n2, p2, f2, F, ep, sig, sc, hm1, hm2 = (gpu._p(a) for a in keep)
    return gpu.lib().ygzfe_search_for_triangulation(
        kf1.h, hm1, len(keep[0]), n1, p1, f1, kf2.h, hm2, len(keep[3]), n2, p2, f2, F, ep, sig, sc, len(keep[8]),
        int(case["only_stereo"]), int(case["check_ori"]), gpu._p(m12), gpu._p(nm))


def test_bad_arguments_leave_the_outputs_unwritten(gpu, scene):
    base, want, kf1, kf2s = scene
    case = T.with_flags(base, False, True)
    nb = case["nbs"][1]

    def refused(c, n):
        m12, nm = np.full(len(c["k1"]), -7, np.int32), np.full(1, -7, np.int32)
        assert raw_single(gpu, c, kf1, kf2s[1], n, m12, nm) == gpu.EINVAL
        assert (m12 == -7).all() and nm[0] == -7, "outputs were written"
        with pytest.raises(gpu.YgzfeError):
            single(gpu, c, kf1, kf2s[1], n)

    # an octave >= n_levels on the neighbour: as many levels given as its highest octave
    top = int(nb["k2"]["octave"].max())
    assert top >= 1
    refused(dict(case, sigma2=case["sigma2"][:top], scale=case["scale"][:top]), nb)
    # a KF2 feature index out of range, a negative one
    for bad in (len(nb["k2"]), -1):
        feats = nb["fv2"][2].copy()
        feats[7] = bad
        refused(case, dict(nb, fv2=(nb["fv2"][0], nb["fv2"][1], feats)))
    # a KF1 feature index out of range, and a KF1 feature listed twice
    feats = case["fv1"][2].copy()
    feats[-1] = len(case["k1"])
    refused(dict(case, fv1=(case["fv1"][0], case["fv1"][1], feats)), nb)
    feats = case["fv1"][2].copy()
    feats[0] = feats[1]
    refused(dict(case, fv1=(case["fv1"][0], case["fv1"][1], feats)), nb)
    # the same arrays unbroken: accepted, and the result as before
    wm, wn = want[(False, True)]
    m12, nm = np.full(len(case["k1"]), -7, np.int32), np.full(1, -7, np.int32)
    assert raw_single(gpu, case, kf1, kf2s[1], nb, m12, nm) == gpu.OK
    assert np.array_equal(m12, wm[1]) and nm[0] == wn[1]
