"""Optimizer::PoseOptimization(Frame*) with the drop-in body (compat/dropin/Optimizer_pose_gpu.inc) at the
reference's call site (Tracking.cc:2212-2239) over the stubs of Frame / MapPoint, against the plain C++
double restatement inside tests/dropin/dropin_pose_opt.cpp: return value, mvbOutlier (rows without a map
point untouched), the float pose, mnMatchesInliers and the cache set; the comparison runs in the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dropin_body_matches_the_cpp_restatement(gpu):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "dropin_pose_opt"])
    r = subprocess.run([os.path.join(ROOT, "compat", "build", "dropin_pose_opt"), "--time"], capture_output=True,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "FAILED" not in r.stdout
    for line in ("mixed-1000", "mixed-2 (nothing written)", "TIMING pose_optimization_1000 dropin_call_ms",
                 "TIMING pose_optimization_batch_32"):
        assert line in r.stdout
