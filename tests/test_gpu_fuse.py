"""ygzfe_fuse_search_batch / ygzfe_fuse_search on the GPU: best_idx and best_dist bit-exact against the loops of
tests/_fuse.py (ORBmatcher.cc:748-866 as written, PredictScale through libm's logf) on the C2 scene and on crafted
rows of a few keypoints each."""
import numpy as np
import pytest

import ygzfe
import _fuse as FU

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def scene():
    case = FU.c2_scene(0)
    frames = [ygzfe.MatchFrame(0).set(kf["kps"], kf["desc"], kf["ur"], kf["bounds"]) for kf in case["kfs"]]
    return case, frames, {True: FU.fuse_loops(case), False: FU.fuse_loops(FU.with_flags(case, check_reproj=False))}


@pytest.mark.parametrize("reproj", [True, False])
def test_scene_matches_the_loops(scene, reproj):
    case, frames, want = scene
    gi, gd = FU.gpu_call(FU.with_flags(case, check_reproj=reproj), frames)
    assert np.array_equal(gi, want[reproj][0]) and np.array_equal(gd, want[reproj][1])


def test_batch_equals_single_calls_and_repeats(scene):
    case, frames, want = scene
    gi, gd = FU.gpu_call(case, frames)
    ri, rd = FU.gpu_call(case, frames)
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd)
    for k, (kf, f) in enumerate(zip(case["kfs"], frames)):
        si, sd = ygzfe.fuse_search(f, kf["view"], case["world"], case["normal"], case["min_dist"], case["max_dist"],
                                   case["desc"], case["scale"], case["isig"], case["lsf"], th=case["th"])
        assert np.array_equal(si, gi[k]) and np.array_equal(sd, gd[k])
        assert np.array_equal(si, want[True][0][k])


def test_skip_is_honoured(scene):
    case, frames, want = scene
    skip = (np.random.default_rng(3).random(want[True][0].shape) < 0.4).astype(np.uint8)
    gi, gd = FU.gpu_call(FU.with_flags(case, skip=skip), frames)
    assert np.array_equal(gi, np.where(skip, -1, want[True][0])) and np.array_equal(gd, np.where(skip, 256, want[True][1]))
    assert (want[True][0][skip == 1] >= 0).any()


CASES = FU.crafted_cases(FU.level_threshold(FU.logf(2.0), 2))


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_row(name):
    case, want_idx, want_dist = CASES[name]
    got = FU.gpu_call(case)
    loops = FU.fuse_loops(case)
    assert np.array_equal(got[0], loops[0]) and np.array_equal(got[1], loops[1])
    assert FU.diag(got) == (want_idx, want_dist)


def _args(case, frames):
    views = np.array([kf["view"] for kf in case["kfs"]], F32).reshape(-1, 20)
    return (frames, views, case["world"], case["normal"], case["min_dist"], case["max_dist"], case["desc"],
            case["scale"], case["isig"], case["lsf"])


def test_degenerate_shapes(scene):
    case, frames, want = scene
    empty = ygzfe.MatchFrame(0).set(FU.kps_of([]), np.zeros((0, 32), np.uint8), None, FU.BOUNDS)
    kfs = [case["kfs"][0], dict(case["kfs"][1], kps=FU.kps_of([]), desc=np.zeros((0, 32), np.uint8), ur=None)]
    gi, gd = FU.gpu_call(dict(case, kfs=kfs), [frames[0], empty])  # a keyframe with no keypoints, in a batch
    assert np.array_equal(gi[0], want[True][0][0]) and np.all(gi[1] == -1) and np.all(gd[1] == 256)
    a = _args(case, frames)
    bi, bd = ygzfe.fuse_search_batch([], np.zeros((0, 20), F32), *a[2:])  # n_kf == 0
    assert bi.shape == (0, len(case["world"])) and bd.size == 0
    z3, z1 = np.zeros((0, 3), F32), np.zeros(0, F32)
    bi, bd = ygzfe.fuse_search_batch(frames, a[1], z3, z3, z1, z1, np.zeros((0, 32), np.uint8), *a[7:])  # n_pts == 0
    assert bi.shape == (3, 0)


def test_refused_arguments_leave_the_outputs_alone(scene):
    case, frames, _ = scene
    a = _args(case, frames)
    n = len(case["world"])

    def refused(*args, **kw):
        bi, bd = np.full((len(args[0]), n), -7, np.int32), np.full((len(args[0]), n), -7, np.int32)
        with pytest.raises(ygzfe.YgzfeError):
            ygzfe.fuse_search_batch(*args, best_idx=bi, best_dist=bd, **kw)
        assert np.all(bi == -7) and np.all(bd == -7)

    refused(*a[:7], np.ones(17, F32), np.ones(17, F32), case["lsf"])          # n_levels 17
    refused(*a[:7], np.zeros(0, F32), np.zeros(0, F32), case["lsf"])          # n_levels 0
    for lsf in (0.0, -0.5, float("nan"), float("inf")):
        refused(*a[:9], lsf)
    top = max(int(kf["kps"]["octave"].max()) for kf in case["kfs"])               # an octave outside [0, n_levels)
    assert top >= 1
    refused(*a[:7], case["scale"][:top], case["isig"][:top], case["lsf"])
    lib = ygzfe.lib()
    bi = np.full(n, -7, np.int32)
    rc = lib.ygzfe_fuse_search(frames[0].h, None, n, ygzfe._p(a[2]), ygzfe._p(a[3]), ygzfe._p(a[4]), ygzfe._p(a[5]),
                               ygzfe._p(a[6]), None, 3.0, ygzfe._p(a[7]), ygzfe._p(a[8]), 4, float(case["lsf"]), 1,
                               ygzfe._p(bi), ygzfe._p(bi))
    assert rc == ygzfe.EINVAL and np.all(bi == -7)                               # null view
    rc = lib.ygzfe_fuse_search(None, ygzfe._p(a[1]), n, ygzfe._p(a[2]), ygzfe._p(a[3]), ygzfe._p(a[4]),
                               ygzfe._p(a[5]), ygzfe._p(a[6]), None, 3.0, ygzfe._p(a[7]), ygzfe._p(a[8]), 4,
                               float(case["lsf"]), 1, ygzfe._p(bi), ygzfe._p(bi))
    assert rc == ygzfe.EINVAL and np.all(bi == -7)                               # null keyframe
    if ygzfe.device_count() > 1:
        other = ygzfe.MatchFrame(1).set(case["kfs"][1]["kps"], case["kfs"][1]["desc"], None, FU.BOUNDS)
        refused([frames[0], other, frames[2]], *a[1:])
