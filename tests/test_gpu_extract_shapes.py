"""GPU ORB extraction vs the CPU oracle across plan shapes: every FAST cell kernel instance in both
launch forms, octree root columns 1..8 and aspect ratios, feature budgets around every node-pool
boundary, every octree sort stage of the batch path, FAST thresholds and tiny levels.

Every case compares the pyramid levels, the ygzfe_kp rows field by field and the descriptors byte
for byte with OrbOracle.extract on the oracle's own pyramid (no tolerance), through the single-frame
path (ORBextractor.extract: one merged FAST launch, 8,192-key first octree stage) and through a
Batch (one FAST launch per level, node-pool classes in launch groups).  Before it compares, a case
asserts from ygzfe.orb_plan_choices (the launchers' own chooser functions, no GPU) that its plan is
the one its name says, and from the oracle that it is not vacuous: every level with cells yields a
keypoint and the frame at least MIN_TOTAL (unless the budget or the design of the case bounds it).
The CPU half (plan + oracle) of every case is `cpu_half`, so the cases can be checked without a GPU.
"""
import functools

import numpy as np
import pytest

import _oracle as O
import _scenes as S
import ygzfe
from test_gpu_extract import assert_kps_equal

MIN_TOTAL = 20


def case(size, orb, img=("frame", 0), min_total=MIN_TOTAL, **expect):
    nf, sf, nl = orb[:3]
    ini, mn = orb[3:] if len(orb) > 3 else (20, 7)
    return dict(size=size, orb=(nf, sf, nl, ini, mn), img=img, min_total=min_total, expect=expect)


# expect: merged = (S, R) of the single-frame FAST launch; fast = per-level (S, R) of the batch path
# (None: no cells); n_ini, classes per level; groups = octree launch groups
CASES = {
    # --- 1. every reachable k_fast_cells<S, R>, one level of 2 x 2 cells (64, 64: a lone 57-px column)
    "fast_36_40": case((92, 92), (100, 1.2, 1), ("frame", 43), merged=(36, 40), fast=[(36, 40)]),
    "fast_40_40": case((93, 92), (100, 1.2, 1), ("frame", 47), merged=(40, 40), fast=[(40, 40)]),
    "fast_40_48": case((92, 101), (100, 1.2, 1), ("frame", 3), merged=(40, 48), fast=[(40, 48)]),
    "fast_40_56": case((92, 117), (100, 1.2, 1), ("frame", 4), merged=(40, 56), fast=[(40, 56)]),
    "fast_48_48": case((101, 92), (100, 1.2, 1), ("frame", 5), merged=(48, 48), fast=[(48, 48)]),
    "fast_56_56": case((117, 92), (100, 1.2, 1), ("frame", 6), merged=(56, 56), fast=[(56, 56)]),
    "fast_64_64": case((89, 92), (100, 1.2, 1), ("frame", 7), merged=(64, 64), fast=[(64, 64)]),
    # the merged instance larger than some level's own
    "fast_merged_3_levels": case((160, 120), (100, 1.2, 3), ("frame", 8), merged=(56, 56),
                                 fast=[(40, 56), (40, 40), (56, 56)], n_ini=[1, 1, 2]),
    "fast_merged_8_levels": case((256, 192), (200, 1.2, 8), ("frame", 9), merged=(56, 56),
                                 fast=[(40, 40), (40, 40), (48, 48), (48, 48), (40, 40), (48, 48), (56, 56), None],
                                 n_ini=[1, 1, 1, 1, 1, 2, 2, 2]),
    # --- 2. root columns and aspect ratio
    "roots_3": case((176, 80), (100, 1.2, 1), ("frame", 10), n_ini=[3], oct_rb=[2]),
    "roots_4": case((224, 80), (100, 1.2, 1), ("frame", 11), n_ini=[4], oct_rb=[2]),
    "roots_5": case((272, 80), (100, 1.2, 1), ("frame", 12), n_ini=[5], oct_rb=[3]),
    "roots_8": case((416, 80), (150, 1.2, 1), ("frame", 13), n_ini=[8], oct_rb=[3]),
    "roots_7_then_8": case((480, 96), (200, 1.2, 2), ("frame", 14), n_ini=[7, 8], oct_rb=[3, 3]),
    "roots_portrait_clamped_to_1": case((64, 200), (100, 1.2, 1), ("frame", 15), n_ini=[1], oct_rb=[0]),
    # texture in the third of 8 root columns only: the other roots are empty nodes
    "roots_8_one_column_textured": case((416, 80), (150, 1.2, 1), ("paste", 16, 2, 8), n_ini=[8], oct_rb=[3]),
    # --- 3. budgets and node pools
    # budget-bound totals: at least one keypoint per level with cells is all a budget of 0 or 1 admits
    "budget_0_8_levels": case((256, 192), (0, 1.2, 8), ("frame", 17), min_total=7, budgets=[0] * 8),
    "budget_1_8_levels": case((256, 192), (1, 1.2, 8), ("frame", 17), min_total=7, budgets=[0] * 7 + [1]),
    "budget_30_8_levels": case((256, 192), (30, 1.2, 8), ("frame", 17), budgets=[7, 5, 5, 4, 3, 3, 2, 1]),
    "pool_need_256": case((200, 160), (236, 1.2, 1), ("noise", 18, 1.0), classes=[256]),
    "pool_need_257": case((200, 160), (237, 1.2, 1), ("noise", 18, 1.0), classes=[512]),
    "pool_need_512": case((200, 160), (492, 1.2, 1), ("noise", 18, 1.0), classes=[512]),
    "pool_need_513": case((200, 160), (493, 1.2, 1), ("noise", 18, 1.0), classes=[1024]),
    "pool_need_1024": case((200, 160), (1004, 1.2, 1), ("noise", 18, 1.0), classes=[1024]),
    "pool_need_1025": case((200, 160), (1005, 1.2, 1), ("noise", 18, 1.0), classes=[2048]),
    "pool_2048": case((200, 160), (1500, 1.2, 1), ("noise", 18, 1.0), classes=[2048]),
    # classes down and back up (a flipped n_ini lifts level 4): four launch groups, side streams
    "pool_classes_down_and_up": case((200, 100), (1392, 1.01, 6), ("frame", 19), groups=4,
                                     classes=[512, 512, 512, 256, 512, 256], n_ini=[2, 2, 2, 2, 3, 3]),
    # far more features asked for than the image holds: the tree ends with every node a singleton
    "budget_above_image": case((96, 72), (2000, 1.2, 1), ("frame", 48), classes=[2048], all_candidates_kept=True),
    # --- 5. thresholds
    "th_ini_equals_min": case((160, 120), (200, 1.2, 3, 7, 7), ("frame", 21)),
    "th_min_1": case((160, 120), (200, 1.2, 3, 20, 1), ("frame", 22)),
    "th_ini_255": case((160, 120), (200, 1.2, 3, 255, 7), ("frame", 23), ini_finds_nothing=True),
    "th_low_contrast": case((256, 192), (200, 1.2, 3, 20, 7), ("low", 55), ini_finds_nothing=True),
    "odd_641x479_c1": case((641, 479), (500, 1.2, 8), ("frame", 25)),
}
# designed-empty: no level has a FAST cell (97x61: a candidate area of 65 x 29 is under one cell row;
# 30x20: no candidate area at all, the levels csrc/plan.cpp gives one root and empty code tables)
EMPTY_CASES = {
    "tiny_97x61": case((97, 61), (500, 1.2, 4), ("frame", 11), min_total=0),
    "tiny_30x20": case((30, 20), (1000, 2.0, 4), ("frame", 11), min_total=0),
}


def make_image(kind, W, H):
    name, seed = kind[0], kind[1]
    if name == "frame":
        return S.frame(seed, W, H)
    if name == "low":  # S.frame squeezed into 12 grey levels: no pixel pair differs by the initial threshold
        return (120 + S.frame(seed, W, H).astype(np.int32) * 12 // 256).astype(np.uint8)
    if name == "paste":  # a flat image with texture in column kind[2] of kind[3] equal columns of the candidate area
        img = np.full((H, W), 128, np.uint8)
        cw = (W - 32) // kind[3]
        x0 = 16 + kind[2] * cw + 2
        img[:, x0:x0 + cw - 4] = S.frame(seed, W, H)[:, x0:x0 + cw - 4]
        return img
    if name == "noise":  # uniform noise over the top fraction kind[2] of a flat image
        img = np.full((H, W), 128, np.uint8)
        rows = int(round(H * kind[2]))
        img[:rows] = np.random.default_rng(seed).integers(0, 256, (rows, W), dtype=np.uint8)
        return img
    if name == "flat":
        return np.full((H, W), 77, np.uint8)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(orb, kind, W, H):
    """(image, oracle pyramid, oracle keypoints, oracle descriptors, candidates per level); shared, never modified."""
    orc = O.OrbOracle(*orb)
    img = make_image(kind, W, H)
    lv = orc.pyramid(img)
    kr, dr = orc.extract(lv)
    ncand = [orc.octree_level(lv[l], l)[1] for l in range(orb[2])]
    for a in (img, kr, dr, *lv):
        a.setflags(write=False)
    return img, lv, kr, dr, ncand


def second_frame(kind):
    return (kind[0], kind[1] + 100) + tuple(kind[2:])


def check_plan(c):
    """The case reaches what its name says: asked of the launchers' chooser functions."""
    (W, H), orb, e = c["size"], c["orb"], c["expect"]
    ch = ygzfe.orb_plan_choices(*orb, W, H)
    lv = ch["levels"]
    if "merged" in e:
        assert ch["merged_fast"] == e["merged"]
    if "fast" in e:
        assert [l["fast"] for l in lv] == e["fast"]
    for key, field in (("n_ini", "n_ini"), ("oct_rb", "oct_rb"), ("classes", "node_class")):
        if key in e:
            assert [l[field] for l in lv] == e[key], key
    if "groups" in e:
        assert ch["octree_groups"] == e["groups"]
    if "budgets" in e:
        assert ygzfe.orb_plan(*orb, W, H)["budget"] == e["budgets"]
    return ch


def cpu_half(c):
    """Plan and oracle assertions of a case (no GPU): its plan is the named one and the oracle's output is
    not vacuous.  Returns (choices, reference)."""
    (W, H), orb, e = c["size"], c["orb"], c["expect"]
    ch = check_plan(c)
    ref = reference(orb, c["img"], W, H)
    img, lv, kr, dr, ncand = ref
    per_level = np.bincount(kr["octave"], minlength=orb[2])
    for l, d in enumerate(ch["levels"]):
        if c["min_total"] > 0 and d["ncells"] > 0:
            assert per_level[l] >= 1, f"level {l} yields no keypoint"
        if d["ncells"] == 0:
            assert ncand[l] == 0 and per_level[l] == 0
    assert len(kr) >= c["min_total"], len(kr)
    if c["min_total"] == 0:
        assert len(kr) == 0 and all(d["ncells"] == 0 for d in ch["levels"])
    if e.get("all_candidates_kept"):
        assert len(kr) == sum(ncand) < orb[0]
    if e.get("ini_finds_nothing"):  # every corner comes from the per-cell retry at min_th
        hi = O.OrbOracle(orb[0], orb[1], orb[2], orb[3], 255)
        assert sum(hi.octree_level(lv[l], l)[1] for l in range(orb[2])) == 0 and len(kr) >= MIN_TOTAL
    if "classes" in e and c["img"][0] == "noise":  # the pool is filled: more candidates than the budget
        assert ncand[0] > orb[0] and len(kr) >= orb[0]
    if c["img"][0] == "paste":  # every keypoint in the one textured root column
        col = ((kr["x"] - 16) / ((W - 32) / c["img"][3])).astype(int)
        assert set(col.tolist()) == {c["img"][2]}
    return ch, ref


def compare_single(gpu, orb, ref, what):
    img, lv, kr, dr, _ = ref
    ex = gpu.ORBextractor(*orb)
    fr = ex.ComputePyramid(img)
    for l, (g, r) in enumerate(zip(fr.levels(), lv)):
        assert g.shape == r.shape and np.array_equal(g, r), f"{what} level {l}"
    kg, dg = ex.extract(fr)
    assert_kps_equal(kg, kr, what)
    assert np.array_equal(dg, dr), f"{what}: {np.count_nonzero((dg != dr).any(1))} descriptor rows differ"


def compare_batch(gpu, orb, size, refs, what):
    W, H = size
    b = gpu.Batch((*orb, 0), 0, W, H, len(refs))
    b.upload(np.stack([r[0] for r in refs]))
    b.extract(len(refs))
    b.check()
    for i, (img, lv, kr, dr, _) in enumerate(refs):
        for l in range(orb[2]):
            assert np.array_equal(b.read_level(i, l), lv[l]), f"{what} frame {i} level {l}"
        kg, dg = b.result(i)
        assert_kps_equal(kg, kr, f"{what} frame {i}")
        assert np.array_equal(dg, dr), f"{what} frame {i}: {np.count_nonzero((dg != dr).any(1))} descriptor rows differ"


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["single", "batch"])
@pytest.mark.parametrize("name", list(CASES) + list(EMPTY_CASES))
def test_extract_shape(gpu, name, path):
    c = {**CASES, **EMPTY_CASES}[name]
    _, ref = cpu_half(c)
    if path == "single":
        compare_single(gpu, c["orb"], ref, name)
    else:
        (W, H) = c["size"]
        compare_batch(gpu, c["orb"], c["size"], [ref, reference(c["orb"], second_frame(c["img"]), W, H)], name)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["single", "batch"])
def test_aspect_past_8_roots_is_refused(gpu, path):
    """400x70: a candidate area of 368 x 38 asks for 10 root columns; the plan holds 8."""
    with pytest.raises(gpu.YgzfeError, match="initial octree nodes"):
        gpu.orb_plan_choices(100, 1.2, 1, 20, 7, 400, 70)
    with pytest.raises(gpu.YgzfeError):
        if path == "single":
            gpu.ORBextractor(100, 1.2, 1, 20, 7).ComputePyramid(S.frame(0, 400, 70))
        else:
            gpu.Batch((100, 1.2, 1, 20, 7, 0), 0, 400, 70, 2)


# --- 4. octree sort stages of the batch path: k_octree_sort (NK0 keys), k_octree_sort_q<., 4096> (the 256
# class only), k_octree_sort_q<., 8192>, k_octree_global, taken as a task's candidate count overflows each.
# One plan cannot hold a 256-class level dense enough for the last stage under a 1,024-class one (budgets
# shrink with the level, and so do the levels), so two plans of the same eight frames: both levels of the
# 256 class, both of the 1,024 class.
STAGE_SIZE = (416, 416)
STAGE_FRAMES = [("flat", 0), ("frame", 30), ("noise", 31, 0.05), ("noise", 32, 0.2), ("noise", 33, 0.45),
                ("noise", 34, 0.75), ("noise", 35, 1.0), ("frame", 36)]
STAGE_PLANS = {"class_256": ((400, 1.2, 2, 20, 7), 256, 1024), "class_1024": ((1100, 1.2, 2, 20, 7), 1024, 4096)}


def stage_ranges(nk0):
    return [(0, 0), (1, nk0), (nk0 + 1, 4096), (4097, 8192), (8193, 65535)]


def stage_cpu_half(plan):
    """Both levels are of the plan's class, and on each level the oracle's candidate counts of the eight frames
    fall into every range between the stages' capacities."""
    orb, cls, nk0 = STAGE_PLANS[plan]
    W, H = STAGE_SIZE
    ch = ygzfe.orb_plan_choices(*orb, W, H)
    assert [l["node_class"] for l in ch["levels"]] == [cls, cls]
    assert [l["sort0_keys_batch"] for l in ch["levels"]] == [nk0, nk0]
    assert [l["sort0_keys_single"] for l in ch["levels"]] == [8192, 8192]
    refs = [reference(orb, k, W, H) for k in STAGE_FRAMES]
    for l in range(2):
        counts = [r[4][l] for r in refs]
        for lo, hi in stage_ranges(nk0):
            if lo <= hi:
                assert any(lo <= n <= hi for n in counts), f"level {l}: no task with {lo}..{hi} candidates in {counts}"
    assert sum(len(r[2]) for r in refs) >= 6 * orb[0] // 2
    return refs


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(STAGE_PLANS))
def test_octree_sort_stages_batch(gpu, plan):
    refs = stage_cpu_half(plan)
    compare_batch(gpu, STAGE_PLANS[plan][0], STAGE_SIZE, refs, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(STAGE_PLANS))
def test_octree_sort_stages_single(gpu, plan):
    """The same frames one by one through the single-frame path (8,192 keys, then the global stage)."""
    for i, ref in enumerate(stage_cpu_half(plan)):
        compare_single(gpu, STAGE_PLANS[plan][0], ref, f"{plan} frame {i}")


# --- 6. DSO_KEYPOINT at an odd size
@pytest.mark.gpu
def test_extract_dso_odd_size_and_state(gpu):
    """test_gpu_extract.py::test_extract_dso_bitexact_and_state at 641x479 with the C1 parameters: the grid
    state mnGridSize carries across three frames (ORBextractor.cc:1295,1380)."""
    W, H, orb = 641, 479, (500, 1.2, 8, 20, 7)
    ex = gpu.ORBextractor(*orb)
    orc = O.OrbOracle(*orb)
    for seed in (4, 5, 6):
        img = S.frame(seed, W, H)
        lv = orc.pyramid(img)
        base, _ = orc.extract(lv)
        existing = base[:60].copy()
        kg, dg = ex.extract(ex.ComputePyramid(img), method=gpu.DSO_KEYPOINT, existing=existing)
        kr, dr, _ = orc.extract_dso(lv, existing=existing)
        assert len(kr) > 60 + MIN_TOTAL
        assert_kps_equal(kg, kr, f"dso seed {seed}")
        assert np.array_equal(dg, dr)
        assert ex.dso_grid == orc.o.dso_grid
