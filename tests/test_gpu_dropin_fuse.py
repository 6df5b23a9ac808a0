"""ORBmatcher::Fuse with the drop-in body (compat/dropin/ORBmatcher_fuse_gpu.inc) and gpu::FuseAll at the reference's
call sites (LocalMapping::SearchInNeighbors, LocalMapping.cc:1262-1306) over stub KeyFrames and MapPoints
(tests/dropin/stubs_fuse), against the plain C++ restatement inside tests/dropin/dropin_fuse.cpp: the complete final
state of the map and the nFused returns; the comparison runs in the program."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dropin_fuse_matches_the_cpp_restatement(gpu):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "dropin_fuse"])
    r = subprocess.run([os.path.join(ROOT, "compat", "build", "dropin_fuse"), "--time"], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "FAILED" not in r.stdout and "MISMATCH" not in r.stdout
    for line in ("map-4 batched: state equal", "map-4 per target: state equal", "map-9 batched: state equal",
                 "one target: state equal", "no target: state equal", "crafted replace: state equal",
                 "TIMING fuse_forward_20 dropin_ms", "TIMING fuse_backward dropin_ms"):
        assert line in r.stdout
    # the crafted Replace in target 0 changes the candidate's descriptor before target 1: that pair is searched on the host
    m = re.search(r"crafted replace: .* host pairs (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 1
    # the random maps do fuse, and do replace points
    m = re.search(r"map-9 batched: state equal, (\d+) fused, (\d+) points replaced", r.stdout)
    assert m and int(m.group(1)) >= 50 and int(m.group(2)) >= 5
