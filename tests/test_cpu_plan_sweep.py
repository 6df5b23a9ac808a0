"""csrc/plan.cpp and the launchers' choices from a plan, without a GPU.

* tests/host/plan_sweep.cpp links plan.cpp alone and runs build_plan over image sizes 8..140 on
  each side (plus large and extreme-aspect sizes), scale factors 1.05 / 1.2 / 1.5 / 2.0, 1 to 16
  levels and budgets 0 to 2000, checking the invariants the kernels rely on.  It is built with
  AddressSanitizer and UBSan (hipcc, the flags on the host side: common.hpp needs the HIP headers)
  and run as a child process, so a level smaller than its border must be planned without a
  division by zero, an out-of-range float-to-int cast or a count of leading zeros of 0.
* ygzfe_orb_plan_choices reports what the launchers of extract.hip choose (the chooser functions
  themselves are called): which k_fast_cells<S, R> instances any level size can reach, and the
  plans tests/test_gpu_extract_shapes.py relies on.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-ygz-slam_amd")
CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(ROOT, "tests", "host", "plan_sweep.cpp")

# YGZ_FAST_SHAPES of csrc/extract.hip
INSTANCES = [(36, 40), (40, 40), (40, 48), (40, 56), (48, 48), (56, 56), (64, 64), (72, 72)]


@pytest.fixture(scope="module")
def ygzfe():
    if not os.path.exists(os.path.join(PKG, "lib", "libygzfe.so")):  # hipcc cross-compiles for gfx950 without a GPU
        subprocess.check_call(["make", "-s", "-C", PKG])
    import ygzfe as m
    return m


def test_plan_sweep_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "plan_sweep")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-x", "hip", os.path.join(CSRC, "plan.cpp"), SRC,
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 violations" in r.stdout.splitlines()[-1]


def test_reachable_fast_instances(ygzfe):
    """Every level size from 62 to 400 on each side, as a one-level plan: the k_fast_cells<S, R>
    instance of the level's launch.  A larger level has 12 or more cells across, of at most 34 + 6
    pixels; a smaller one has no cell.  (72, 72) is instantiated but no level size selects it: the
    largest ROI side is 59, a lone cell clipped to the border (the widest unclipped is 45 + 6)."""
    seen, roi = {}, 0
    for W in range(62, 401):
        for H in range(62, 401):
            try:
                lv = ygzfe.orb_plan_choices(100, 1.2, 1, 20, 7, W, H)["levels"][0]
            except ygzfe.YgzfeError:  # more than 8 root columns
                assert not (W - 32 < 8.5 * (H - 32)), (W, H)
                continue
            assert lv["ncells"] > 0, (W, H)
            seen.setdefault(lv["fast"], (W, H))
            roi = max(roi, lv["fast_rw"], lv["fast_rh"])
    print("reachable instances, first size:", sorted(seen.items()), "largest ROI side:", roi)
    assert roi == 59
    assert sorted(seen) == INSTANCES[:-1]
    assert (72, 72) not in seen


def test_choices_of_known_plans(ygzfe):
    """The three benchmark configurations: what the merged and the per-level launches run."""
    c1 = ygzfe.orb_plan_choices(500, 1.2, 8, 20, 7, 640, 480)
    assert c1["merged_fast"] == (48, 48) and [l["n_ini"] for l in c1["levels"]] == [1] * 8
    assert {l["node_class"] for l in c1["levels"]} == {256} and c1["octree_groups"] == 1
    assert [l["sort0_keys_batch"] for l in c1["levels"]] == [1024] * 8
    assert [l["sort0_keys_single"] for l in c1["levels"]] == [8192] * 8
    c2 = ygzfe.orb_plan_choices(1000, 2.0, 4, 20, 7, 752, 480)
    assert c2["merged_fast"] == (40, 56) and [l["n_ini"] for l in c2["levels"]] == [2, 2, 2, 2]
    assert [l["oct_rb"] for l in c2["levels"]] == [1, 1, 1, 1]
    assert [l["node_class"] for l in c2["levels"]] == [1024, 512, 256, 256] and c2["octree_groups"] == 3
    assert c2["levels"][3]["ncells"] == 0 and c2["levels"][3]["fast"] is None
    assert [l["sort0_keys_batch"] for l in c2["levels"]] == [4096, 4096, 1024, 1024]
    c4 = ygzfe.orb_plan_choices(2000, 1.2, 8, 20, 7, 640, 480)
    assert c4["merged_fast"] == (48, 48) and [l["node_class"] for l in c4["levels"]] == [512] * 4 + [256] * 4
    with pytest.raises(ygzfe.YgzfeError):
        ygzfe.orb_plan_choices(100, 1.2, 1, 20, 7, 400, 70)  # 10 root columns
    tiny = ygzfe.orb_plan_choices(1000, 2.0, 4, 20, 7, 30, 20)  # no level has a candidate area
    assert tiny["merged_fast"] is None and all(l["n_ini"] == 1 and l["ncells"] == 0 for l in tiny["levels"])
