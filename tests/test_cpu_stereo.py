"""Frame::ComputeStereoMatches without a GPU: the restatement of tests/_stereo.py against oracle/stereo.c bit for bit,
the crafted cases against the outcome they are named for, the random sweep's coverage of every outcome, and every
mutation of the restatement against the crafted case that shows it."""
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import _stereo as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-ygz-slam_amd")
F32 = np.float32
CASES = ST.crafted_cases()

# every outcome code and the crafted cases that pin it (checked by test_codes_are_pinned)
PINNED_BY = {
    "ROW_OUT": ["u_negative_and_rows_out"],
    "U_NEG": ["u_negative_and_rows_out"],
    "NO_CAND": ["band_lo_o0", "band_hi_o0", "band_lo_o1", "band_hi_o1", "band_lo_o7", "band_hi_o7", "octave_d-2",
                "octave_d+2", "u_at_min", "u_at_max", "hamming_100"],
    "ORB_TH": ["hamming_75", "hamming_99", "median_no_match"],
    "LEFT_WIN_OUT": ["left_window_left_past", "left_window_right_past", "left_window_top_past",
                     "left_window_bottom_past", "u_negative_and_rows_out"],
    "SLIDE_OUT": ["slide_left_past", "slide_right_past", "top_level_slide_9", "top_level_slide_11",
                  "left_window_left"],
    "SLIDE_END": ["min_at_-5", "min_at_+5", "median_no_match"],
    "DISP_RANGE": ["disparity_negative", "disparity_at_max_and_under"],
    "CUT": ["median_odd", "median_even", "median_repeats", "median_low_byte", "median_high"],
    "KEPT": ["hamming_74", "octave_d-1", "octave_d+0", "octave_d+1", "left_window_right", "left_window_top",
             "left_window_bottom", "slide_left", "slide_right", "top_level_slide_10", "min_at_-4", "min_at_+4",
             "two_equal_minima", "three_equal_minima", "round_half_uL", "round_half_vL", "round_half_uR0",
             "tie_lanes_strides", "tie_lower_index_higher_lane", "smaller_distance_later",
             "disparity_at_max_and_under", "median_single_largest_sad", "inexact_scale_products"],
    "KEPT_CLAMPED": ["disparity_zero_clamped"],
}
# every mutation and a crafted case whose u_right, depth or sad it changes
KILLED_BY = {
    "band_swapped": "band_lo_o7", "octave_pm2": "octave_d+2", "u_excl_lo": "u_at_min", "u_excl_hi": "u_at_max",
    "th_le_75": "hamming_75", "hamming_tie_last": "tie_lanes_strides", "sad_tie_last": "three_equal_minima",
    "rint": "round_half_uR0", "slide_endu_gt": "top_level_slide_11", "slide_end_kept": "min_at_+5",
    "no_clamp": "disparity_zero_clamped", "median_lo": "median_even", "cut_le": "median_odd",
    "fma": "inexact_scale_products",
}


def oracle_run(case):
    g = case["geom"]
    orc = O.OrbOracle(*g.extractor_args)
    return O.stereo_matches(orc, case["left"], case["right"], case["kl"], case["dl"], case["kr"], case["dr"],
                            float(case["mb"]), float(case["mbf"]))


def same(res, u, d, s):
    return np.array_equal(res.u_right, u) and np.array_equal(res.depth, d) and np.array_equal(res.sad, s)


@pytest.fixture(scope="module")
def ygzfe():
    if not os.path.exists(os.path.join(PKG, "lib", "libygzfe.so")):  # hipcc cross-compiles for gfx950 without a GPU
        subprocess.check_call(["make", "-s", "-C", PKG])
    import ygzfe as m
    return m


@pytest.mark.parametrize("name", sorted(ST.GEOMETRIES))
def test_geometry_is_the_extractors(ygzfe, name):
    g = ST.GEOMETRIES[name]
    orc = O.OrbOracle(*g.extractor_args)
    assert orc.level_sizes(g.W, g.H) == g.sizes
    assert np.array_equal(orc.scale, g.scale) and np.array_equal(orc.inv_scale, g.inv_scale)
    nf, sf, nl, ini, mn = g.extractor_args
    assert ygzfe.orb_plan(nf, sf, nl, ini, mn, g.W, g.H)["sizes"] == g.sizes     # frame creation takes the size
    assert float(g.max_d) == {"x2": 32.0, "x1.2": 80.0}[name]
    if name == "x2":    # the top level's one legal slide position
        assert [c for c in range(g.sizes[2][0]) if c - 10 >= 0 and c + 11 < g.sizes[2][0]] == [10]


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_case(name):
    """The restatement equals the oracle bit for bit (sad included), every left keypoint lands in the branch the
    case names, and the values the case states in closed form are the ones computed."""
    case = CASES[name]
    res = ST.run(case)
    assert same(res, *oracle_run(case))
    assert res.code == case["codes"]
    for il, (u, d, s) in case["values"].items():
        assert res.u_right[il] == F32(u) and res.depth[il] == F32(d) and res.sad[il] == s, (name, il)
    for il, code in enumerate(res.code):
        if code not in ("KEPT", "KEPT_CLAMPED"):
            assert res.u_right[il] == -1 and res.depth[il] == -1 and res.sad[il] == -1


def test_codes_are_pinned():
    assert set(PINNED_BY) == set(ST.CODES)
    for code, names in PINNED_BY.items():
        for n in names:
            assert code in CASES[n]["codes"], (code, n)
    assert set(sum(PINNED_BY.values(), [])) <= set(CASES)


@pytest.mark.parametrize("geometry", sorted(ST.GEOMETRIES))
def test_random_sweep(geometry):
    """Bit-exact agreement with the oracle on every seed, and (a condition on the inputs) every outcome code
    occurs over the seeds, with every octave on both sides."""
    seen = set()
    g = ST.GEOMETRIES[geometry]
    for seed, (case, res) in zip(ST.RANDOM_SEEDS, ST.random_cases(geometry)):
        assert same(res, *oracle_run(case)), seed
        seen |= set(res.code)
        assert set(case["kl"]["octave"]) == set(case["kr"]["octave"]) == set(range(g.nlevels))
        assert len(case["kl"]) == 300 and len(case["kr"]) >= 300
    assert seen == set(ST.CODES), set(ST.CODES) - seen


@pytest.mark.parametrize("mut", ST.MUTATIONS)
def test_mutation_shows_on_a_crafted_case(mut):
    name = KILLED_BY[mut]
    base, got = ST.run(CASES[name]), ST.run(CASES[name], mut=(mut,))
    assert not same(got, base.u_right, base.depth, base.sad), f"{mut} changes nothing on {name}"


def test_every_mutation_has_its_case():
    assert set(KILLED_BY) == set(ST.MUTATIONS)


def test_cut_constant_is_2p1f():
    """Why there is no `2.1f * median` mutation: 1.5f * 1.4f is the float 2.1f."""
    assert F32(F32(1.5) * F32(1.4)) == F32(2.1)


def test_clamp_literals_agree():
    """Why there is no `uL - 0.01f` mutation: for every uL a clamped keypoint can have (its window is inside its
    level, so 4.5 <= uL < 4096) the float form equals float(double(uL) - 0.01).  Per binade the offset of uL - 0.01
    from the float grid is one number; it is checked for every binade, on its first and last floats and on 10^5
    random ones."""
    rng = np.random.default_rng(5)
    for e in range(2, 12):
        lo, hi = F32(2.0 ** e), np.nextafter(F32(2.0 ** (e + 1)), F32(0))
        first = lo.view(np.uint32) + np.arange(0, 64, dtype=np.uint32)
        last = hi.view(np.uint32) - np.arange(0, 64, dtype=np.uint32)
        rnd = rng.integers(int(lo.view(np.uint32)), int(hi.view(np.uint32)) + 1, 100000).astype(np.uint32)
        u = np.concatenate([first, last, rnd]).view(F32)
        assert np.array_equal((u.astype(np.float64) - 0.01).astype(F32), u - F32(0.01)), e


def test_median_sets():
    """The preconditions of the median-cut cases, in the restatement's own float32."""
    th = lambda m: F32(F32(F32(1.5) * F32(1.4)) * F32(m))     # noqa: E731
    assert th(10) == 21 and th(4200) == 8820                   # a SAD exactly at the threshold is cut (strict <)
    for name, sads in ST.MEDIAN_SETS.items():
        res = ST.run(CASES[name])
        assert sorted(res.sad[res.sad >= 0].tolist() + [s for s in sads if not F32(s) < th(res.median)]) \
            == sorted(sads), name
        assert res.median == sorted(sads)[len(sads) // 2]
    assert len(ST.MEDIAN_SETS["median_odd"]) % 2 == 1 and len(ST.MEDIAN_SETS["median_even"]) % 2 == 0
    s = sorted(ST.MEDIAN_SETS["median_low_byte"])
    k = len(s) // 2
    assert s[k - 1] >> 8 == s[k] >> 8 == s[k + 1] >> 8 and s[k - 1] < s[k] < s[k + 1]
    for other in (s[k - 1], s[k + 1]):  # a select that took a neighbour of the median would cut other rows
        assert [F32(v) < th(other) for v in s] != [F32(v) < th(s[k]) for v in s]
    assert max(ST.MEDIAN_SETS["median_high"]) > 4095 and min(ST.MEDIAN_SETS["median_high"]) > 255
    big = ST.run(CASES["median_single_largest_sad"])
    assert big.sad.tolist() == [58650] and big.median == 58650 and big.code == ["KEPT"]
    none = ST.run(CASES["median_no_match"])
    assert none.median is None and (none.sad == -1).all()


def test_clamped_match_survives():
    case = CASES["disparity_zero_clamped"]
    res = ST.run(case)
    assert res.median > 0 and res.code.count("KEPT_CLAMPED") == 2
    for il, code in enumerate(res.code):
        if code == "KEPT_CLAMPED":
            u_l = case["kl"]["x"][il]
            assert res.depth[il] == F32(case["mbf"] / F32(0.01))
            assert res.u_right[il] == F32(np.float64(u_l) - 0.01)


def test_delta_half():
    """deltaR is exactly +0.5 where the right neighbour equals the minimum; -0.5 only under the tie mutation."""
    assert ST.run(CASES["two_equal_minima"]).delta[0] == F32(0.5)
    assert ST.run(CASES["three_equal_minima"]).delta[0] == F32(0.5)
    assert ST.run(CASES["two_equal_minima"], mut=("sad_tie_last",)).delta[0] == F32(-0.5)
