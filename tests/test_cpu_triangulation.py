"""The restatement of ORBmatcher::SearchForTriangulation (tests/_triangulation.py) against itself, without a GPU:
the reference's sequential loops and the closed form the device computes (smallest accepted distance, last list
position among equals) agree on every input the GPU tests use, the C2 scene really matches, and every crafted
row decides what it is meant to decide."""
import numpy as np
import pytest

import _triangulation as T

FLAGS = [(False, True), (False, False), (True, True), (True, False)]  # (only_stereo, check_ori)


@pytest.mark.parametrize("only_stereo,check_ori", FLAGS)
def test_loops_and_closed_form_agree_on_the_scene(only_stereo, check_ori):
    case = T.with_flags(T.c2_scene(0), only_stereo, check_ori)
    m_l, n_l = T.search_loops(case)
    m_c, n_c = T.search_closed(case)
    assert np.array_equal(m_l, m_c) and np.array_equal(n_l, n_c)
    assert np.array_equal((m_l >= 0).sum(1), n_l)


def test_the_scene_really_matches():
    case = T.c2_scene(0)
    assert len(case["nbs"]) == 3
    for f in [case["has_mp1"]] + [nb["has_mp2"] for nb in case["nbs"]]:
        assert 0.4 < f.mean() < 0.6, "about half the features already have a map point"
    m12, n = T.search_loops(case)
    print("matches per neighbour:", n.tolist())
    assert (n > 30).all()
    for row, nb in zip(m12, case["nbs"]):  # only features without a map point, on either side
        i1 = np.nonzero(row >= 0)[0]
        assert not case["has_mp1"][i1].any() and not nb["has_mp2"][row[i1]].any()
    # the first neighbour's epipole lies in the image: the mono-mono distance rule has keypoints to reject
    ex, ey = case["nbs"][0]["ep"]
    assert 0 < ex < 752 and 0 < ey < 480
    # with only_stereo fewer, but some, remain, and every one joins two stereo keypoints
    ms, ns = T.search_loops(T.with_flags(case, True, True))
    assert (ns > 0).all() and (ns < n).all()
    for row, nb in zip(ms, case["nbs"]):
        i1 = np.nonzero(row >= 0)[0]
        assert (case["ur1"][i1] >= 0).all() and (nb["ur2"][row[i1]] >= 0).all()


CRAFTED = T.crafted_cases()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_row(name):
    case, want = CRAFTED[name]
    for search in (T.search_loops, T.search_closed):
        m12, n = search(case)
        assert m12.tolist() == [want], name
        assert n.tolist() == [sum(v >= 0 for v in want)]


def test_crafted_rows_change_when_their_rule_is_broken():
    """Each row against the neighbouring rule: the pairs differ in exactly the rule's input."""
    r = {k: T.search_closed(c)[0][0].tolist() for k, (c, _) in CRAFTED.items()}
    assert r["tie_last_position"] == [1]  # the first position would give 2, the largest index 2, the smallest 0
    tie = CRAFTED["tie_last_position"][0]
    assert tie["nbs"][0]["fv2"][2].tolist() == [2, 0, 1]
    assert r["closer_fails_epipolar"] == [1]  # without the epipolar test: 0, the closer one
    D = T.hamming(CRAFTED["closer_fails_epipolar"][0]["d1"], CRAFTED["closer_fails_epipolar"][0]["nbs"][0]["d2"])
    assert D[0, 0] < D[0, 1] <= T.TH_LOW
    assert T.hamming(CRAFTED["dist_50"][0]["d1"], CRAFTED["dist_50"][0]["nbs"][0]["d2"])[0, 0] == 50
    assert T.hamming(CRAFTED["dist_51"][0]["d1"], CRAFTED["dist_51"][0]["nbs"][0]["d2"])[0, 0] == 51
    assert r["dist_50"] != r["dist_51"]
    assert r["epipole_mono_mono"] != r["epipole_one_stereo"]
    assert r["only_stereo"] != r["only_stereo_off"]
    assert r["den_zero"] == [-1]


def test_float_and_double_comparisons_disagree_at_the_chosen_sigma2():
    s, dbl, flt = T.sigma2_where_float_and_double_disagree()
    assert s.dtype == np.float32 and dbl != flt
    assert dbl == (1.0 < 3.84 * float(s)) and flt == bool(np.float32(1.0) < np.float32(3.84) * s)
    case, want = CRAFTED["double_comparison"]
    # the row's dsqr is exactly 1: x2 = 101 on the line x2 = 100 with den = 1
    assert case["nbs"][0]["k2"]["x"][0] == 101 and want == [0 if dbl else -1]
    assert T.search_loops(case)[0].tolist() == [want]
