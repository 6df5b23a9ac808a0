"""Tracking::SearchLocalPointsDirect with the per-point set-up on the device (the drop-in body
behind YGZFE_DIRECT_DEVICE_SETUP, tests/dropin/dropin_direct_setup.cpp): on a 130-keyframe local
map, mvKeys / mvpMapPoints / mvMatchedFrom, the cache set and the MapPoints' track fields are
bit-equal to a host loop in the stated arithmetic feeding ygzfe_search_local_points_direct; the
comparison runs inside the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_setup_body_matches_the_host_loop(gpu):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compat"), "dropin_direct_setup"])
    r = subprocess.run([os.path.join(ROOT, "compat", "build", "dropin_direct_setup"), "--time"], capture_output=True,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK")
    for line in ("device set-up [130 keyframes, mnCacheHitTh 150]", "device set-up [130 keyframes, mnCacheHitTh 1073741824]",
                 "mbTrackInView / mTrackProjX", "TIMING search_local_points_direct_130kf host_setup_ms"):
        assert line in r.stdout
    assert "FAILED" not in r.stdout
