"""Preconditions of tests/test_gpu_direct_views.py, on the CPU: the oracle's GetWarpAffineMatrix /
GetBestSearchLevel / WarpAffine (oracle/align.c) against the independent restatement of
tests/_direct_views.py and against the plane's homography, on views where A is far from the
identity; that the scenes reach what they are for; that the oracle's FindDirectProjection works on
them end to end, and that the restatement's deliberate mistakes do not.
"""
import functools

import numpy as np
import pytest

import _direct_views as V
import _scenes as S

CASES = [(cfg, name, 0) for cfg in V.CONFIGS for name in V.view_names(cfg)] + \
        [(cfg, name, 1) for cfg in V.CONFIGS for name in ("zoom1.9", "roll30")]   # K1 items of the mixed calls


@functools.lru_cache(maxsize=None)
def data(cfg, name, k):
    """One view's items with the oracle's and the restatement's A and search level."""
    it = V.view_items(cfg, name, k)
    ov = V.oracle_view(cfg)
    nl = V.CONFIGS[cfg][3]
    scale, _, inv_s2 = V.pyramid_scales(cfg)
    uv = np.stack([it["kps"]["x"], it["kps"]["y"]], 1)
    A64 = V.warp_matrix(V.cam32(cfg), it["T_cr"]["q"][0], it["T_cr"]["t"][0], it["pt_ref"], uv,
                        scale[it["kps"]["octave"]])
    A32 = ov.warp_matrices(it)
    return {"it": it, "uv": uv, "A64": A64, "A32": A32, "sl64": V.best_search_level(A64, nl - 1, inv_s2[1]),
            "sl32": ov.search_levels(A32), "D": V.search_level_D(A64, nl - 1, inv_s2[1])}


@functools.lru_cache(maxsize=None)
def patches(cfg, name, k):
    """(oracle patch, restated patch, float64 samples, outside mask) per item, from the oracle's A."""
    d, ov = data(cfg, name, k), V.oracle_view(cfg)
    scale = V.pyramid_scales(cfg)[0]
    ref = ov.pyramid(k)
    out = []
    for i, kp in enumerate(d["it"]["kps"]):
        oc, sl = kp["octave"], d["sl32"][i]
        out.append((ov.warp(d["A32"][i], ref, kp, sl),) +
                   V.warp_patch(d["A32"][i], ref[oc], d["uv"][i], scale[oc], scale[sl]))
    return out


def test_scales_and_rendering():
    for cfg in V.CONFIGS:
        ov = V.oracle_view(cfg)
        for mine, theirs in zip(V.pyramid_scales(cfg), (ov.scale, ov.inv_scale, ov.inv_sigma2)):
            assert np.array_equal(mine, theirs)
        for name in V.view_names(cfg):
            assert V.view_in_texture(cfg, name), (cfg, name)


def test_items_well_defined():
    for cfg, name, k in CASES:
        d = data(cfg, name, k)
        it = d["it"]
        assert 150 <= len(it["kps"]) <= 300, (cfg, name, k, len(it["kps"]))
        c = V._qrot(it["T_cr"]["q"][0], it["pt_ref"].astype(np.float64)) + it["T_cr"]["t"][0]
        assert (c[:, 2] > 0).all() and (np.linalg.det(d["A64"]) > 0).all(), (cfg, name, k)
        assert all(np.isfinite(it[f]).all() for f in ("pt_ref", "px0", "px_true")), (cfg, name, k)


def test_oracle_A_against_float64():
    """ygzo_warp_affine_matrix (float32) against warp_matrix (float64) on every item.  The worst
    difference is the floor recorded as V.A_FLOOR; V.A_TOL = 4 x floor."""
    worst = {}
    for cfg, name, k in CASES:
        d = data(cfg, name, k)
        worst[cfg, name, k] = float(np.abs(d["A32"] - d["A64"]).max())
    top = max(worst, key=worst.get)
    print(f"worst |A_oracle - A_float64| = {worst[top]:.3e} at {top}; A_FLOOR {V.A_FLOOR:.1e}, A_TOL {V.A_TOL:.1e}")
    assert V.A_TOL == 4 * V.A_FLOOR
    assert worst[top] <= V.A_FLOOR, "the recorded floor is stale"
    # the views do leave the identity: off-diagonals and anisotropy of order one
    assert np.abs(data("sf20", "roll90", 0)["A64"][:, 0, 1]).min() > 0.9
    a = data("sf20", "oblique", 0)["A64"]
    assert np.median(a[:, 1, 1] / a[:, 0, 0]) > 1.15


def test_A_is_the_homography_difference():
    """K0 is fronto-parallel at depth PLANE_Z, so Pixel2Camera(px + 4 scale, depth) lies on the plane
    and A is the 4-px finite difference of the plane-induced homography K (R + t n^T / d) K^-1 (float64,
    n = e_z): a statement of A that rests on neither restatement."""
    for cfg, name, k in CASES:
        if k != 0:
            continue
        d = data(cfg, name, 0)
        it = d["it"]
        fx, fy, cx, cy = V.cam32(cfg)
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        q = it["T_cr"]["q"][0].astype(np.float64)
        q = q / np.linalg.norm(q)
        x, y, z, w = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        t = it["T_cr"]["t"][0].astype(np.float64)
        Hm = K @ (R + np.outer(t, [0, 0, 1.0]) / S.PLANE_Z) @ np.linalg.inv(K)

        def h(px):
            p = np.concatenate([px, np.ones((len(px), 1))], 1) @ Hm.T
            return p[:, :2] / p[:, 2:]

        ls = V.pyramid_scales(cfg)[0][it["kps"]["octave"]].astype(np.float64)
        uv = d["uv"].astype(np.float64)
        G = np.zeros_like(d["A64"])
        G[:, :, 0] = (h(uv + np.stack([4 * ls, 0 * ls], 1)) - h(uv)) / 4
        G[:, :, 1] = (h(uv + np.stack([0 * ls, 4 * ls], 1)) - h(uv)) / 4
        assert np.abs(d["A32"] - G).max() <= V.A_TOL, (cfg, name, np.abs(d["A32"] - G).max())
        assert np.abs(d["A64"] - G).max() <= V.A_TOL, (cfg, name)


def test_search_level():
    for cfg, name, k in CASES:
        d = data(cfg, name, k)
        # no determinant on the ladder is within relative 1e-5 of the threshold, on any item
        assert np.abs(d["D"].astype(np.float64) / 3.0 - 1.0).min() > 1e-5, (cfg, name, k)
        assert np.array_equal(d["sl32"], d["sl64"]), (cfg, name, k)


def test_coverage():
    for cfg in V.CONFIGS:
        nl = V.CONFIGS[cfg][3]
        hist = np.zeros(nl, np.int64)
        part = whole = 0
        for name in V.view_names(cfg):
            hist += np.bincount(data(cfg, name, 0)["sl32"], minlength=nl)
            outs = [p[3] for p in patches(cfg, name, 0)]
            part += sum(o.any() and not o.all() for o in outs)
            whole += sum(o.all() for o in outs)
        print(cfg, "levels", hist.tolist(), "partly zero", part, "wholly zero", whole)
        assert (hist >= 20).all(), hist
        assert (data(cfg, "cap", 0)["D"][:, -1] > 3.0).sum() >= 20
        assert part >= 20 and whole >= 3
        # outside the cap view the level is the one GetBestSearchLevel wants (zoom views)
        for s in V.ZOOMS[cfg]:
            assert (data(cfg, f"zoom{s:g}", 0)["D"][:, -1] <= 3.0).all()


def test_warped_patch_bytes():
    """ygzo_warp_affine against warp_patch byte for byte; a byte may differ only where the float64
    sample is within 1e-3 of an integer, and on at most 0.5 % of the bytes."""
    n = ndiff = 0
    for cfg, name, k in CASES:
        for pb, rb, val, outside in patches(cfg, name, k):
            diff = pb != rb
            n += diff.size
            if diff.any():
                ndiff += int(diff.sum())
                assert (np.abs(val[diff] - np.round(val[diff])) <= 1e-3).all(), (cfg, name, k)
    print(f"{ndiff} of {n} bytes differ")
    assert ndiff <= 0.005 * n


@functools.lru_cache(maxsize=None)
def oracle_end_to_end(cfg, name):
    d, ov = data(cfg, name, 0), V.oracle_view(cfg)
    px, lvl, ok = ov.find_direct(d["it"], [ov.pyramid(0)], ov.pyramid(name))
    assert np.array_equal(lvl, d["sl32"])
    inside = np.array([not p[3].any() for p in patches(cfg, name, 0)])
    return V.end_to_end(px, ok, inside, d["it"])


@pytest.mark.parametrize("cfg", list(V.CONFIGS))
def test_oracle_end_to_end(cfg):
    """ygzo_find_direct_projection per view (not `cap`): at least half of the items whose patch is fully
    inside converge, and the converged ones end nearer the true projection than px0 (medians, level-0 px)."""
    for name in V.view_names(cfg):
        if name == "cap":
            continue
        figs = oracle_end_to_end(cfg, name)
        print(cfg, name, "converged %.2f, median error %.3f px from %.3f px" % figs)
        assert V.end_to_end_passes(figs), (cfg, name, figs)


# the view on which each deliberate mistake of the restatement must fail the end-to-end check
MUTATION_VIEW = {"transpose_A": "roll90", "swap_R_offdiag": "roll90", "no_search_scale": "zoom4",
                 "level_from_octave": "zoom4"}


@pytest.mark.parametrize("mut", V.MUTATIONS)
@pytest.mark.parametrize("cfg", list(V.CONFIGS))
def test_mutations_fail_end_to_end(cfg, mut):
    """The restatement's warp with one mistake + the oracle's Align2D fails where the same pipeline
    without the mistake passes: the views tell these mistakes apart."""
    name = MUTATION_VIEW[mut]
    it = V.view_items(cfg, name)
    px, _, ok, inside = V.restated_find_direct(cfg, it, name)
    assert V.end_to_end_passes(V.end_to_end(px, ok, inside, it))
    px, _, ok, inside = V.restated_find_direct(cfg, it, name, (mut,))
    figs = V.end_to_end(px, ok, inside, it)
    print(cfg, name, mut, "converged %.2f, median error %.3f px from %.3f px" % figs)
    assert not V.end_to_end_passes(figs), (cfg, name, mut, figs)


def test_align2d_image_walk_cases():
    """The stored seeds give what test_gpu_align.py needs: trajectories that leave the first 48 x 48
    window inside the image, and one that leaves the image."""
    img = V.host_image()
    assert img.strides[0] > img.shape[1] and img.strides[1] == 1
    assert len(V.WALK_OUT_SEEDS) >= 5 and len(V.OUT_OF_IMAGE_SEEDS) >= 1
    for s in V.WALK_OUT_SEEDS:
        pwb, px = V.walk_case(s)
        assert V.walk_kind(img, px, V.align2d_trace(img, pwb, px)) == "walk_out", s
    for s in V.OUT_OF_IMAGE_SEEDS:
        pwb, px = V.walk_case(s, edge=True)
        assert V.walk_kind(img, px, V.align2d_trace(img, pwb, px)) == "out_of_image", s
