"""ORBmatcher::SearchForTriangulation with the drop-in body (compat/dropin/ORBmatcher_mapping_gpu.inc) at the
reference's call site (LocalMapping.cc:1037-1042) over a stub KeyFrame, per neighbour and through
gpu::SearchForTriangulationAll, against the plain C++ restatement inside tests/dropin/dropin_triangulation.cpp:
return values and vMatchedPairs; the comparison runs in the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dropin_body_matches_the_cpp_restatement(gpu):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "dropin_triangulation"])
    r = subprocess.run([os.path.join(ROOT, "compat", "build", "dropin_triangulation"), "--time"], capture_output=True,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "FAILED" not in r.stdout
    for line in ("mapping-10 checkOri", "mapping-3 onlyStereo", "no neighbour",
                 "TIMING search_for_triangulation_1 ", "TIMING search_for_triangulation_batch_20 batch_ms"):
        assert line in r.stdout
