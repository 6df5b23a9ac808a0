"""The local-map set-up of ygzfe_search_local_map_direct, host side: the float32 restatement
the GPU tests compare against (tests/_direct_map.py) against float64 geometry, and the ABI."""
import ctypes as C
import os

import numpy as np

import _direct_map as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0  # chosen so that at most 2 % of the scene lies within 1e-3 of a threshold (checked below)


def test_restatement_matches_float64_geometry():
    """The float32 restatement keeps the candidates the float64 formulas keep, and projects them to
    within 1e-3 px.  Candidates within 1e-3 of a threshold in float64 (px, m or cosine) may fall
    either way and are left out; they must stay a small part (<= 2 %) of the scene."""
    m = DM.map_scene(SEED, render=False)
    cam = m["scene"].cam
    r = DM.restate(m, cam)
    in64, u64, v64, margin = DM.restate64(m, cam)
    n = len(m["world"])
    clear = margin >= 1e-3
    assert (~clear).sum() <= 0.02 * n, ((~clear).sum(), n)
    assert clear.sum() > 1000
    in32 = ~r["culled"]
    assert np.array_equal(in32[clear], in64[clear])
    both = clear & in32
    assert both.sum() > 500
    assert np.abs(r["proj"][both, 0] - u64[both]).max() <= 1e-3
    assert np.abs(r["proj"][both, 1] - v64[both]).max() <= 1e-3
    # every rule of the cull is exercised by the scene, and the skip flag
    for rule in DM.CULL_RULES + (DM.SKIP,):
        assert (r["rule"] == rule).sum() >= 5, rule
    # the items are the n_sel largest kf_ids among the keyframes not excluded, in descending order
    for k in range(len(r["rows"])):
        a, b = r["item_ptr"][k], r["item_ptr"][k + 1]
        ids = m["kf_id"][r["ref_index"][a:b]]
        assert (np.diff(ids) < 0).all() and not m["kf_excluded"][r["ref_index"][a:b]].any()
        assert b - a == min(5, r["n_eligible"][r["rows"][k]])


def test_abi_exports():
    import ygzfe
    lib = C.CDLL(os.path.join(ROOT, "orb-ygz-slam_amd", "lib", "libygzfe.so"))
    for name in ("ygzfe_search_local_map_direct", "ygzfe_frame_set_keypoints", "ygzfe_frame_keypoint_count"):
        assert hasattr(lib, name), name
    assert callable(ygzfe.search_local_map_direct)
    assert callable(ygzfe.Frame.set_keypoints)
    assert ygzfe.DIRECT_CULLED == 4 and ygzfe.DIRECT_MAX_SEL == 8
