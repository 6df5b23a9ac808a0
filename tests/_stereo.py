"""numpy float32 restatement of Frame::ComputeStereoMatches (Frame.cc:509-682), written from that source, with an
outcome code per left keypoint, crafted one-rule cases, and a random sweep.

Kept as the reference has them: `float` stays float32 (every operation rounded once, nothing fused), the three
`round` calls are C round (half away from zero), `disparity = 0.01` / `bestuR = uL - 0.01` keep their double
literals, `1.5f * 1.4f * median` is a float product, the candidates of a row come in right-keypoint order.  The 11x11
windows hold integers (pixel minus the window's centre), so their L1 norms are exact integers below 2^24.

Where the reference would abort or read out of range, this file follows oracle/stereo.c: a left row outside
[0, nRows) and a window cut outside its level drop the keypoint (for vL in (-1, 0) the reference indexes row 0 and
then aborts on rowRange(-5, 6): dropped either way); with no match at all the median cut is a no-op.

The `deltaR < -1 || deltaR > 1` gate has no case, because it cannot fire: the best window is the first strict minimum
and lies strictly inside the slide, so with x = dist1 - dist2 >= 1 and y = dist3 - dist2 >= 0 (integers below
2^17) deltaR = (x - y) / (2 (x + y)) is in (-0.5, 0.5] and its denominator is positive.  +0.5 is reached when the
right neighbour equals the minimum (case `two_equal_minima`); -0.5 would need the left neighbour to equal it, and
then that neighbour is the first minimum itself: the same case seen from its second window, which only the
`sad_tie_last` mutation selects (it then gives exactly -0.5).

`mut` names a deliberate mistake, for the mutation tests of test_cpu_stereo.py.
"""
import numpy as np

F32 = np.float32
CODES = ("ROW_OUT", "U_NEG", "NO_CAND", "ORB_TH", "LEFT_WIN_OUT", "SLIDE_OUT", "SLIDE_END", "DISP_RANGE", "CUT", "KEPT",
         "KEPT_CLAMPED")
# cut_2p1 (threshold as 2.1f * median) is not here: 1.5f * 1.4f rounds to the float 2.1f, so it changes nothing
# (test_cpu_stereo.py::test_cut_constant_is_2p1f).
# clamp_f32 (bestuR = uL - 0.01f in float) is not here either: a left keypoint that reaches the clamp has its window
# inside its level, so uL >= 4.5, and from the binade [4, 8) upwards float(double(uL) - 0.01) == uL - 0.01f for every
# float uL: within a binade uL is a multiple of the ulp, so where uL - 0.01 falls between two floats depends on the
# binade alone, and in none of them does the 2.2e-10 between 0.01 and 0.01f straddle a rounding boundary
# (test_cpu_stereo.py::test_clamp_literals_agree).  `disparity = 0.01` rounds to 0.01f in either spelling.
MUTATIONS = ("band_swapped", "octave_pm2", "u_excl_lo", "u_excl_hi", "th_le_75", "hamming_tie_last", "sad_tie_last",
             "rint", "slide_endu_gt", "slide_end_kept", "no_clamp", "median_lo", "cut_le", "fma")
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
TH_HIGH, TH_LOW = 100, 50
W5 = 5   # w = L = 5 (Frame.cc:603, :612)


def c_round(x):
    """roundf: to the nearest integer, halfway cases away from zero."""
    x = F32(x)
    t = np.trunc(x)
    if abs(F32(x - t)) >= F32(0.5):      # x - t is exact
        t = F32(t + np.copysign(F32(1), x))
    return F32(t)


_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming_matrix(dl, dr):
    """DescriptorDistance of every (left, right) pair."""
    dl, dr = np.asarray(dl, np.uint8).reshape(-1, 32), np.asarray(dr, np.uint8).reshape(-1, 32)
    return _POP[dl[:, None, :] ^ dr[None, :, :]].sum(-1)


class Result:
    def __init__(self, n):
        self.u_right = np.full(n, -1, F32)
        self.depth = np.full(n, -1, F32)
        self.sad = np.full(n, -1, np.int32)
        self.code = ["?"] * n
        self.best_idx = np.full(n, -1, np.int64)     # the right keypoint that won the Hamming search
        self.best_inc = np.full(n, 99, np.int64)     # the best window's offset
        self.delta = np.full(n, np.nan, F32)         # deltaR
        self.median = None


def window_sads(IL, IR, r0, c0, cr0):
    """The 11 L1 norms of Frame.cc:622-636 as integers: left window at (r0, c0), right windows at (r0, cr0 + k)."""
    n = 2 * W5 + 1
    A = IL[r0:r0 + n, c0:c0 + n].astype(np.int64)
    A = A - A[W5, W5]
    out = []
    for k in range(n):
        B = IR[r0:r0 + n, cr0 + k:cr0 + k + n].astype(np.int64)
        out.append(int(np.abs(A - (B - B[W5, W5])).sum()))
    return out


def stereo_matches(left_levels, right_levels, scale, inv_scale, kl, dl, kr, dr, mb, mbf, mut=()):
    mut = set(mut)
    assert mut <= set(MUTATIONS), mut
    scale, inv_scale = np.asarray(scale, F32), np.asarray(inv_scale, F32)
    mb, mbf = F32(mb), F32(mbf)
    nl, nr = len(kl), len(kr)
    R = Result(nl)
    n_rows = left_levels[0].shape[0]
    rnd = (lambda v: F32(np.rint(F32(v)))) if "rint" in mut else c_round
    # the row band of every right keypoint (Frame.cc:526-536)
    y_r, o_r, x_r = kr["y"].astype(F32), kr["octave"].astype(np.int64), kr["x"].astype(F32)
    rad = (F32(2) * scale[o_r]).astype(F32) if nr else np.zeros(0, F32)
    lo, hi = (y_r - rad).astype(F32), (y_r + rad).astype(F32)
    if "band_swapped" in mut:
        band_lo, band_hi = np.ceil(lo).astype(np.int64), np.floor(hi).astype(np.int64)
    else:
        band_lo, band_hi = np.floor(lo).astype(np.int64), np.ceil(hi).astype(np.int64)
    dist = hamming_matrix(dl, dr)
    min_d = F32(0)
    max_d = F32(mbf / mb)
    span = 2 if "octave_pm2" in mut else 1
    pairs = []
    for il in range(nl):
        u_l, v_l, lvl = F32(kl["x"][il]), F32(kl["y"][il]), int(kl["octave"][il])
        if not (v_l >= 0) or int(v_l) >= n_rows:
            R.code[il] = "ROW_OUT"
            continue
        row = int(v_l)
        min_u, max_u = F32(u_l - max_d), F32(u_l - min_d)
        if max_u < 0:
            R.code[il] = "U_NEG"
            continue
        # the candidates of the row in right-keypoint order, `dist < bestDist` from TH_HIGH (Frame.cc:566-591)
        cand = (band_lo <= row) & (row <= band_hi) & (o_r >= lvl - span) & (o_r <= lvl + span)
        cand &= (x_r > min_u) if "u_excl_lo" in mut else (x_r >= min_u)
        cand &= (x_r < max_u) if "u_excl_hi" in mut else (x_r <= max_u)
        cand &= dist[il] < TH_HIGH
        best, best_r = TH_HIGH, 0
        if cand.any():
            idx = np.flatnonzero(cand)
            best = int(dist[il][idx].min())
            ties = idx[dist[il][idx] == best]
            best_r = int(ties[-1] if "hamming_tie_last" in mut else ties[0])
        if best >= TH_HIGH:
            R.code[il] = "NO_CAND"
            continue
        th = (TH_HIGH + TH_LOW) // 2
        if not (best <= th if "th_le_75" in mut else best < th):
            R.code[il] = "ORB_TH"
            continue
        R.best_idx[il] = best_r
        # sub-pixel match by correlation (Frame.cc:594-667)
        sf = inv_scale[lvl]
        su_l, sv_l = rnd(F32(u_l * sf)), rnd(F32(v_l * sf))
        su_r = rnd(F32(F32(kr["x"][best_r]) * sf))
        IL, IR = left_levels[lvl], right_levels[lvl]
        Hh, W = IL.shape
        n = 2 * W5 + 1
        r0, c0 = int(F32(sv_l - W5)), int(F32(su_l - W5))
        if r0 < 0 or r0 + n > Hh or c0 < 0 or c0 + n > W:
            R.code[il] = "LEFT_WIN_OUT"
            continue
        iniu = F32(F32(su_r + W5) - W5)
        endu = F32(F32(F32(su_r + W5) + W5) + 1)
        cr0 = int(F32(F32(su_r - W5) - W5))
        if iniu < 0 or (endu > W if "slide_endu_gt" in mut else endu >= W) or cr0 < 0 or int(endu) > W:
            R.code[il] = "SLIDE_OUT"
            continue
        sads = window_sads(IL, IR, r0, c0, cr0)
        best_sad, best_k = None, 0
        for k, s in enumerate(sads):
            if best_sad is None or s < best_sad or ("sad_tie_last" in mut and s == best_sad):
                best_sad, best_k = s, k
        inc = best_k - W5
        R.best_inc[il] = inc
        if inc in (-W5, W5):
            if "slide_end_kept" not in mut:
                R.code[il] = "SLIDE_END"
                continue
        # slide_end_kept: the neighbour that does not exist is taken as the end window itself
        d1, d2, d3 = (F32(sads[min(max(j, 0), 2 * W5)]) for j in (best_k - 1, best_k, best_k + 1))
        with np.errstate(all="ignore"):
            delta = F32(F32(d1 - d3) / F32(F32(2) * F32(F32(d1 + d3) - F32(F32(2) * d2))))
        R.delta[il] = delta
        if delta < -1 or delta > 1:     # unreachable without a mutation (see the module docstring)
            R.code[il] = "DELTA_OUT"
            continue
        t = F32(F32(su_r + F32(inc)) + delta)
        best_u = F32(scale[lvl] * t)
        disparity = F32(u_l - best_u)
        if "fma" in mut:                # uL - scale * t with the product unrounded
            disparity = F32(np.float64(u_l) - np.float64(scale[lvl]) * np.float64(t))
        if not (disparity >= min_d and disparity < max_d):
            R.code[il] = "DISP_RANGE"
            continue
        R.code[il] = "KEPT"
        if disparity <= 0:
            R.code[il] = "KEPT_CLAMPED"
            if "no_clamp" not in mut:
                disparity = F32(0.01)
                best_u = F32(np.float64(u_l) - 0.01)
        with np.errstate(all="ignore"):
            R.depth[il] = F32(mbf / disparity)
        R.u_right[il] = best_u
        R.sad[il] = best_sad
        pairs.append((best_sad, il))
    # the median outlier cut (Frame.cc:670-681)
    if pairs:
        pairs.sort()
        k = (len(pairs) - 1) // 2 if "median_lo" in mut else len(pairs) // 2
        median = F32(pairs[k][0])
        R.median = int(median)
        th_dist = F32(F32(F32(1.5) * F32(1.4)) * median)
        for s, il in pairs:
            if not (F32(s) <= th_dist if "cut_le" in mut else F32(s) < th_dist):
                R.u_right[il] = R.depth[il] = -1
                R.sad[il] = -1
                R.code[il] = "CUT"
    return R


# ---------------------------------------------------------------------------------------------- geometries
def orb_scales(scale_factor, nlevels):
    """mvScaleFactors / mvInvScaleFactors as ORBextractor.cc:412-427 forms them (float products, 1.0f / scale)."""
    s = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        s[i] = F32(s[i - 1] * F32(scale_factor))
    return s, (F32(1) / s).astype(F32)


class Geometry:
    """A pyramid shape: level l is cvRound(W * inv_scale[l]) x cvRound(H * inv_scale[l]) (ORBextractor.cc:1131-1132)."""

    def __init__(self, name, W, H, scale_factor, nlevels, mb, mbf):
        self.name, self.W, self.H, self.scale_factor, self.nlevels = name, W, H, scale_factor, nlevels
        self.scale, self.inv_scale = orb_scales(scale_factor, nlevels)
        self.sizes = [(int(np.rint(F32(F32(W) * i))), int(np.rint(F32(F32(H) * i)))) for i in self.inv_scale]
        self.mb, self.mbf = F32(mb), F32(mbf)
        self.max_d = F32(self.mbf / self.mb)
        self.extractor_args = (400, scale_factor, nlevels, 20, 7)


# x2: 88x64 -> 44x32 -> 22x16.  A slide needs scaleduR0 >= 10 and scaleduR0 + 11 < W, so the 22-wide top level
# has exactly one legal position (10).  x1.2: 160x122, because frame creation refuses 160x120 (its 45x33 top level would
# need 13 initial octree nodes; the extractor's plan allows 8) and 160x122 is the nearest height it takes.
GEOMETRIES = {"x2": Geometry("x2", 88, 64, 2.0, 3, 0.5, 16.0),          # maxD = 32
              "x1.2": Geometry("x1.2", 160, 122, 1.2, 8, 0.5, 40.0)}    # maxD = 80


def noise_levels(geom, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for (w, h) in geom.sizes]


def desc_base(tag):
    """A 32-byte descriptor per group tag: groups differ in about 128 bits, so they never see each other."""
    return np.random.default_rng(1000 + tag).integers(0, 256, 32, dtype=np.uint8)


def flip_bits(desc, k, first=0):
    """desc with bits [first, first + k) inverted: Hamming distance exactly k."""
    bits = np.unpackbits(desc)
    bits[first:first + k] ^= 1
    return np.packbits(bits)


# ---------------------------------------------------------------------------------------------- case builder
STEP = 130      # what a column outside the flat zone adds to each of its 10 non-centre rows
BASE_SAD = 7


class Builder:
    """Noise levels with planted strips.  A planted match has a left 11x11 patch whose rows are constant (row r
    holds a_r) centred at (uls, vls) of level o, and a right strip of 11 rows x 21 columns centred at the right
    keypoint's scaled column: the 11 columns of the `zone` around the wanted best window repeat the patch, every
    other column is a_r + step in its 10 non-centre rows.  Window k of the slide then differs from the patch by
    10 * step per column outside the zone, so with the best window at k0
        SAD(k) = sad + 10 * step_left * (k0 - k)  (k < k0),   sad + 10 * step_right * (k - k0)  (k > k0):
    one strict minimum, deltaR = 0 when both steps are equal, and every value known in closed form.  `sad` is added
    in the zone's centre column, which every window of the slide contains."""

    def __init__(self, geom, seed=1):
        self.g = geom
        self.L = noise_levels(geom, 2 * seed)
        self.R = noise_levels(geom, 2 * seed + 1)
        self.kl, self.dl, self.kr, self.dr = [], [], [], []
        self.codes, self.values = {}, {}
        self.rng = np.random.default_rng(seed)

    def left(self, x, y, o, desc):
        self.kl.append((F32(x), F32(y), o))
        self.dl.append(np.array(desc, np.uint8))
        return len(self.kl) - 1

    def right(self, x, y, o, desc):
        self.kr.append((F32(x), F32(y), o))
        self.dr.append(np.array(desc, np.uint8))
        return len(self.kr) - 1

    def filler(self, n):
        """n right keypoints no left keypoint can match (octave 0, row band [0, 3], descriptors of their own)."""
        for i in range(n):
            self.right(1.0, 1.0, 0, desc_base(5000 + len(self.kr)))

    def plant(self, o, uls, vls, su_r, inc, sad=BASE_SAD, step=(STEP, STEP), zone=11, a=None):
        """Left patch at (uls, vls), right strip around column su_r with the best window at su_r + inc; `step` =
        (left, right) column steps, zone = 11 or 12 columns (12: two equal minima, at inc and inc + 1).  sad: the
        best window's SAD, laid into the centre column first and then into its neighbours (at most 100 per pixel,
        so a window that loses a column still gains more from the column outside the zone it takes in)."""
        Lo, Ro = self.L[o], self.R[o]
        a = self.rng.integers(100, 121, 11).astype(np.int64) if a is None else a
        Lo[vls - 5:vls + 6, uls - 5:uls + 6] = a[:, None].astype(np.uint8)
        z0 = su_r + inc - 5
        for c in range(su_r - 10, su_r + 11):
            col = a.copy()
            if c < z0 or c >= z0 + zone:
                col += step[0] if c < z0 else step[1]
                col[5] = a[5]
            Ro[vls - 5:vls + 6, c] = col.astype(np.uint8)
        left_over = sad
        for dc in (0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5):
            for r in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):
                d = min(left_over, 100)
                Ro[vls - 5 + r, su_r + inc + dc] += d
                left_over -= d
        assert left_over == 0, "sad too large to plant"
        return a

    def pair(self, o, u_l, v_l, su_r, tag, inc=0, bits=0, o_r=None, dy=0.0, expect="KEPT", plant=True, **kw):
        """A left keypoint at level-0 (u_l, v_l) of octave o and its right keypoint at scaled column su_r (so at
        su_r * scale[o]), with the best window planted at su_r + inc.  Returns (iL, iR)."""
        g = self.g
        uls, vls = int(c_round(F32(F32(u_l) * g.inv_scale[o]))), int(c_round(F32(F32(v_l) * g.inv_scale[o])))
        if plant:
            self.plant(o, uls, vls, su_r, inc, **kw)
        base = desc_base(tag)
        il = self.left(u_l, v_l, o, base)
        ir = self.right(F32(F32(su_r) * g.scale[o]), F32(F32(v_l) + F32(dy)), o if o_r is None else o_r,
                        flip_bits(base, bits))
        self.codes[il] = expect
        if expect == "KEPT" and kw.get("step", (STEP, STEP))[0] == kw.get("step", (STEP, STEP))[1] \
                and kw.get("zone", 11) == 11:
            self.expect_kept(il, o, su_r + inc, kw.get("sad", BASE_SAD))
        return il, ir

    def expect_kept(self, il, o, best_col, sad):
        """Closed form of a planted match with equal steps: deltaR = 0, bestuR = scale * best_col."""
        u_l = self.kl[il][0]
        u_r = F32(self.g.scale[o] * F32(best_col))
        self.values[il] = (u_r, F32(self.g.mbf / F32(u_l - u_r)), sad)

    def case(self):
        kl = np.zeros(len(self.kl), KP_DTYPE)
        kr = np.zeros(len(self.kr), KP_DTYPE)
        for arr, rows in ((kl, self.kl), (kr, self.kr)):
            for i, (x, y, o) in enumerate(rows):
                arr["x"][i], arr["y"][i], arr["octave"][i] = x, y, o
                arr["size"][i] = 31.0
        dl = np.array(self.dl, np.uint8).reshape(-1, 32)
        dr = np.array(self.dr, np.uint8).reshape(-1, 32)
        codes = [self.codes[i] for i in range(len(kl))]
        return dict(geom=self.g, left=self.L, right=self.R, kl=kl, dl=dl, kr=kr, dr=dr, mb=self.g.mb, mbf=self.g.mbf,
                    codes=codes, values=dict(self.values))


def run(case, mut=()):
    g = case["geom"]
    return stereo_matches(case["left"], case["right"], g.scale, g.inv_scale, case["kl"], case["dl"], case["kr"],
                          case["dr"], case["mb"], case["mbf"], mut=mut)


def cell(c, r):
    """Scaled column of the right keypoint and row of cell (c, r) of a 22 x 12 grid: strips of different cells
    never overlap, and the left patches (at most 10 columns to the right of their strip's centre) neither."""
    return 22 * c + 11, 12 * r + 6


# The SADs of the median-cut cases.  th = 1.5f * 1.4f * median in float32; th(10) = 21 and th(4200) = 8820 exactly.
MEDIAN_SETS = {
    # 7 matches, median = element 3 = 10: 20 is kept, 21 (== th) and 22 are cut
    "median_odd": [3, 10, 10, 10, 20, 21, 22],
    # 8 matches, median = element 4 = 10 (element 3 = 9 would cut 19 and 20: th(9) = 18.9)
    "median_even": [3, 9, 9, 9, 10, 19, 20, 21],
    # repeated SADs on both sides of the median
    "median_repeats": [8, 8, 8, 8, 8, 8, 17, 17],
    # one high byte (0x01), low bytes apart: median 0x1a0 = 416, th = 873.6; were the select to take a neighbour
    # (0x19f -> 871.5, 0x1a1 -> 875.7) the rows at 872 / 875 would change sides
    "median_low_byte": [0x105, 0x110, 0x19F, 0x1A0, 0x1A1, 872, 875],
    # above 255 and above 4,095: median 4200, th = 8820 exactly
    "median_high": [300, 4096, 4200, 4200, 8819, 8820, 8821],
}


def _median_case(name):
    sads = MEDIAN_SETS[name]
    g = GEOMETRIES["x1.2"]
    B = Builder(g, seed=sum(map(ord, name)))
    srt = sorted(sads)
    th = F32(F32(F32(1.5) * F32(1.4)) * F32(srt[len(srt) // 2]))
    for i, s in enumerate(sads):
        su_r, vls = cell(i % 7, i // 7 + 2)
        il, _ = B.pair(0, su_r + 4, vls, su_r, tag=i, sad=s, expect="KEPT" if F32(s) < th else "CUT")
    return B.case()


def crafted_cases():
    """{name: case}; a case is a dict of geom, left / right levels, kl, dl, kr, dr, mb, mbf, codes (the outcome
    per left keypoint) and values {iL: (u_right, depth, sad)} where the planted closed form gives them."""
    A, Bg = GEOMETRIES["x2"], GEOMETRIES["x1.2"]
    cases = {}

    def one(name, geom, fn, seed=None):
        b = Builder(geom, seed=sum(map(ord, name)) if seed is None else seed)
        fn(b)
        cases[name] = b.case()

    # ---- row band ends with a fractional kpR.y: [floor(y - 2 s_o), ceil(y + 2 s_o)] (x1.2, octaves 0, 1, 7)
    for o, y_r in ((0, 40.3), (1, 40.3), (7, 60.3)):
        r = F32(F32(2) * Bg.scale[o])
        lo, hi = int(np.floor(F32(F32(y_r) - r))), int(np.ceil(F32(F32(y_r) + r)))
        for end, row_in, row_out in (("lo", lo, lo - 1), ("hi", hi, hi + 1)):
            def fn(b, o=o, y_r=y_r, row_in=row_in, row_out=row_out):
                su_r = 12
                u_l = F32(F32(su_r + 3) * Bg.scale[o])
                il, ir = b.pair(o, u_l, row_in + 0.5, su_r, tag=1)
                b.kr[ir] = (b.kr[ir][0], F32(y_r), o)
                j = b.left(u_l, row_out + 0.5, o, desc_base(1))
                b.codes[j] = "NO_CAND"
            one(f"band_{end}_o{o}", Bg, fn)

    # ---- the octave gate: left octave 3 against right octaves 1 .. 5
    for d in (-2, -1, 0, 1, 2):
        def fn(b, d=d):
            su_r = 14
            b.pair(3, F32(F32(su_r + 4) * Bg.scale[3]), 50.0, su_r, tag=2, o_r=3 + d,
                   expect="KEPT" if abs(d) <= 1 else "NO_CAND")
        one(f"octave_d{d:+d}", Bg, fn)

    # ---- the u range [uL - maxD, uL], both ends and one ulp outside each (x2, octave 0, maxD = 32)
    def u_range(b, lo):
        u_l = F32(60)
        for k, (row, outside) in enumerate(((12, False), (40, True))):
            if lo:      # right keypoint at minU = 28: best window 3 to its right, disparity 29
                x = F32(u_l - A.max_d)
                il, ir = b.pair(0, u_l, row, 28, tag=10 + k, inc=3, expect="NO_CAND" if outside else "KEPT")
                b.kr[ir] = (np.nextafter(x, F32(-1e9)) if outside else x,) + b.kr[ir][1:]
            else:       # right keypoint at maxU = uL: best window 3 to its left, disparity 3
                il, ir = b.pair(0, u_l, row, 60, tag=10 + k, inc=-3, expect="NO_CAND" if outside else "KEPT")
                b.kr[ir] = (np.nextafter(u_l, F32(1e9)) if outside else u_l,) + b.kr[ir][1:]
    one("u_at_min", A, lambda b: u_range(b, True))
    one("u_at_max", A, lambda b: u_range(b, False))

    def u_neg(b):
        i = b.left(-1e-3, 20.0, 0, desc_base(3))
        b.codes[i] = "U_NEG"
        j = b.left(0.0, 20.0, 0, desc_base(3))        # maxU = 0 passes; the window at column 0 leaves the level
        b.codes[j] = "LEFT_WIN_OUT"
        b.right(0.0, 20.0, 0, desc_base(3))
        k = b.left(30.0, -0.5, 0, desc_base(3))
        b.codes[k] = "ROW_OUT"
        m = b.left(30.0, 64.0, 0, desc_base(3))
        b.codes[m] = "ROW_OUT"
    one("u_negative_and_rows_out", A, u_neg)

    # ---- Hamming thresholds: 74 kept, 75 and 99 refused by (TH_HIGH + TH_LOW) / 2, 100 no candidate at all
    for k, want in ((74, "KEPT"), (75, "ORB_TH"), (99, "ORB_TH"), (100, "NO_CAND")):
        one(f"hamming_{k}", A, lambda b, k=k, want=want: b.pair(0, 50.0, 20.0, 44, tag=4, bits=k, expect=want))

    # ---- equal best distance: the lowest right index wins, whatever lane (index % 64) or stride it falls in
    def ties(b, idx, dist, winner):
        """Right keypoints at the indices `idx` (fillers between) with the distances `dist`, each with a strip of
        its own for the one left patch, so that mvuRight shows which of them won (x1.2, octave 0, maxD = 80)."""
        u_l, row, cols = F32(150), 30, (124, 80, 102)   # the first, lowest index is not the leftmost
        base = desc_base(6)
        il = b.left(u_l, row, 0, base)
        a = None
        for n, (i, d) in enumerate(zip(idx, dist)):
            b.filler(i - len(b.kr))
            a = b.plant(0, 150, row, cols[n], 0, a=a)
            b.right(F32(cols[n]), row, 0, flip_bits(base, d, first=8 * n))
        b.codes[il] = "KEPT"
        b.expect_kept(il, 0, cols[winner], BASE_SAD)
    one("tie_lanes_strides", Bg, lambda b: ties(b, (3, 67, 130), (20, 20, 20), 0))
    one("tie_lower_index_higher_lane", Bg, lambda b: ties(b, (10, 65), (20, 20), 0))
    one("smaller_distance_later", Bg, lambda b: ties(b, (3, 67, 130), (21, 21, 20), 2))

    # ---- the left window against the four borders of its level (x2, octave 1: 44 x 32)
    s1 = A.scale[1]
    # A window flush with the left border cannot be kept: the right keypoint is at most at uL, and a slide needs
    # scaleduR0 >= 10.  There the left window passes and the slide is refused; one column further the window is.
    for name, uls, vls, want in (("left", 5, 16, "SLIDE_OUT"), ("left_past", 4, 16, "LEFT_WIN_OUT"),
                                 ("right", 38, 16, "KEPT"), ("right_past", 39, 16, "LEFT_WIN_OUT"),
                                 ("top", 30, 5, "KEPT"), ("top_past", 30, 4, "LEFT_WIN_OUT"),
                                 ("bottom", 30, 26, "KEPT"), ("bottom_past", 30, 27, "LEFT_WIN_OUT")):
        def fn(b, uls=uls, vls=vls, want=want):
            su_r = uls if uls < 20 else 26
            b.pair(1, F32(uls * s1), F32(vls * s1), su_r, tag=7, expect=want, plant=want == "KEPT")
        one(f"left_window_{name}", A, fn)

    # ---- the slide against the left and right border of the level (x2, octave 1, W = 44: 10 .. 32 are legal)
    for name, su_r, want in (("left", 10, "KEPT"), ("left_past", 9, "SLIDE_OUT"), ("right", 32, "KEPT"),
                             ("right_past", 33, "SLIDE_OUT")):
        def fn(b, su_r=su_r, want=want):
            # planted even where the reference stops (the strip still fits), so that a kernel that went on would
            # report a match
            b.pair(1, F32((su_r + 4) * s1), F32(16 * s1), su_r, tag=8, expect=want, plant=su_r >= 10)
        one(f"slide_{name}", A, fn)
    # the top level (22 wide) has the one legal slide position 10
    for su_r, want in ((9, "SLIDE_OUT"), (10, "KEPT"), (11, "SLIDE_OUT")):
        one(f"top_level_slide_{su_r}", A, lambda b, su_r=su_r, want=want: b.pair(
            2, F32(14 * A.scale[2]), F32(8 * A.scale[2]), su_r, tag=9, expect=want, plant=su_r >= 10))

    # ---- the minimum at the ends of the slide and next to them
    for inc, want in ((-5, "SLIDE_END"), (-4, "KEPT"), (4, "KEPT"), (5, "SLIDE_END")):
        one(f"min_at_{inc:+d}", A, lambda b, inc=inc, want=want: b.pair(0, 60.0, 30.0, 40, tag=11, inc=inc,
                                                                           expect=want))

    # ---- two equal minima: the first wins, its right neighbour equals it, deltaR = +0.5 exactly
    def equal_minima(b):
        il, _ = b.pair(0, 60.0, 30.0, 40, tag=12, inc=-1, zone=12)
        u_r = F32(F32(F32(40) + F32(-1)) + F32(0.5))
        b.values[il] = (u_r, F32(A.mbf / F32(F32(60) - u_r)), BASE_SAD)
    one("two_equal_minima", A, equal_minima)

    def three_minima(b):
        # three equal minima: the first gives 39 + 0.5, the last would give 41 - 0.5
        il, _ = b.pair(0, 60.0, 30.0, 40, tag=12, inc=-1, zone=13)
        u_r = F32(F32(F32(40) + F32(-1)) + F32(0.5))
        b.values[il] = (u_r, F32(A.mbf / F32(F32(60) - u_r)), BASE_SAD)
    one("three_equal_minima", A, three_minima)

    # ---- a .5 tie in each round (x2, octave 1: x * 0.5f is exact): 36.5 -> 37, never 36
    def rounds(b, which):
        u_l, v_l = F32(74), F32(32)                     # scaled 37, 16
        if which == "uL":
            u_l = F32(73)                               # 36.5 -> 37
        if which == "vL":
            v_l = F32(33)                               # 16.5 -> 17
        if which == "uR0":                              # 26.5 -> 27, best window at +4 (from 26 it would be the end)
            il, ir = b.pair(1, u_l, v_l, 27, tag=13, inc=4)
            b.kr[ir] = (F32(53),) + b.kr[ir][1:]
        else:
            b.pair(1, u_l, v_l, 26, tag=13)
    for which in ("uL", "vL", "uR0"):
        one(f"round_half_{which}", A, lambda b, which=which: rounds(b, which))

    # ---- disparity: negative, equal to maxD, one ulp under it
    def negative(b):
        # the right keypoint at 39 passes the u gate; the best window is 3 to its right: bestuR = 42 > uL
        b.pair(0, 40.0, 30.0, 39, tag=14, inc=3, expect="DISP_RANGE")
    one("disparity_negative", A, negative)

    def at_max(b):
        # right keypoint at 30 (>= minU = 28), best window at 28: disparity 60 - 28 = maxD
        b.pair(0, 60.0, 12.0, 30, tag=15, inc=-2, expect="DISP_RANGE")
        il, _ = b.pair(0, np.nextafter(F32(60), F32(0)), 40.0, 30, tag=16, inc=-2)
    one("disparity_at_max_and_under", A, at_max)

    # ---- disparity exactly 0: clamped to 0.01 px, kept because the other matches make the median positive
    def clamp(b):
        for k, (u_l, row) in enumerate(((40.0, 8), (70.0, 20))):
            il, _ = b.pair(0, u_l, row, int(u_l) - 2, tag=20 + k, inc=2, expect="KEPT_CLAMPED")
            b.values[il] = (F32(np.float64(F32(u_l)) - 0.01), F32(A.mbf / F32(0.01)), BASE_SAD)
        b.pair(0, 60.0, 32.0, 50, tag=22)
        b.pair(0, 30.0, 44.0, 22, tag=23)
    one("disparity_zero_clamped", A, clamp)

    # ---- the median cut
    for name in MEDIAN_SETS:
        cases[name] = _median_case(name)

    def largest(b):
        """The largest best SAD built here: left patch 255 with centre 0, right strip 0 with the centre row's 11
        window centres 255.  SAD(k) = 110 * 510 + (10 - |k|) * 255 + |k| * 510 = 58,650 + 255 |k| (the bound for any
        window is 120 * 510 = 61,200; the centre row is shared by the 11 windows).  np == 1: median = 58,650."""
        b.L[0][25:36, 55:66] = 255
        b.L[0][30, 60] = 0
        b.R[0][25:36, 30:51] = 0
        b.R[0][30, 35:46] = 255
        il = b.left(60.0, 30.0, 0, desc_base(30))
        b.right(40.0, 30.0, 0, desc_base(30))
        b.codes[il] = "KEPT"
        b.values[il] = (F32(40), F32(A.mbf / F32(20)), 58650)
    one("median_single_largest_sad", A, largest)

    def none(b):
        b.pair(0, 60.0, 30.0, 40, tag=31, bits=80, expect="ORB_TH")
        b.pair(0, 60.0, 50.0, 40, tag=32, inc=5, expect="SLIDE_END")
    one("median_no_match", A, none)

    def fma(b):
        # x1.2 octaves, where scale * t is inexact: the depths of a fused disparity differ in the last place
        for k, (o, c, r) in enumerate(((1, 0, 1), (2, 1, 1), (3, 0, 0), (4, 1, 0), (5, 0, 1), (6, 0, 0), (7, 0, 0))):
            su_r, vls = cell(c, r)
            b.pair(o, F32(F32(su_r + 3) * Bg.scale[o]), F32(F32(vls) * Bg.scale[o]), su_r, tag=40 + k)
    one("inexact_scale_products", Bg, fma)
    return cases


# ---------------------------------------------------------------------------------------------- random sweep
def random_case(seed, geometry):
    """300 hand-placed left keypoints and a few more right ones on independent noise levels; each left window is
    copied (with +-2 of noise, clipped to the level, later copies overwriting earlier ones) to where its match
    should be found.  Every octave, many keypoints within 12 px of a level's border, disparities over
    [-3, maxD + 3], descriptor distances over 0 .. 120, some right keypoints doubled (ties), a few octave-0
    keypoints moved onto their bestuR (disparity exactly zero), the right keypoints in shuffled order."""
    g = GEOMETRIES[geometry]
    rng = np.random.default_rng(seed)
    L = noise_levels(g, 7000 + seed)
    R = [np.random.default_rng(9000 + seed + l).integers(0, 256, a.shape, dtype=np.uint8) for l, a in enumerate(L)]
    n = 300
    kl = np.zeros(n, KP_DTYPE)
    dl = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kr_rows, dr_rows = [], []
    for i in range(n):
        o = i % g.nlevels
        w, h = g.sizes[o]
        s = g.scale[o]
        if rng.random() < 0.4:      # near a border of the level
            xs = rng.choice([rng.uniform(0, 12), rng.uniform(w - 12, w)])
            ys = rng.choice([rng.uniform(0, 12), rng.uniform(h - 12, h)])
            if rng.random() < 0.5:
                xs = rng.uniform(0, w)
            else:
                ys = rng.uniform(0, h)
        else:
            xs, ys = rng.uniform(5, w - 5), rng.uniform(5, h - 5)
        if rng.random() < 0.3:
            xs, ys = np.floor(xs) + 0.5, np.floor(ys) + 0.5
        u_l, v_l = F32(F32(xs) * s), F32(F32(ys) * s)
        if rng.random() < 0.03:
            u_l = F32(-u_l * F32(0.01))
        if rng.random() < 0.03:
            v_l = F32(rng.choice([-1.0, g.H, g.H + 3.5]))
        kl["x"][i], kl["y"][i], kl["octave"][i] = u_l, v_l, o
        d = F32(rng.uniform(-3, float(g.max_d) + 3))
        if rng.random() < 0.5:
            d = F32(rng.uniform(0, min(float(g.max_d), 0.6 * w * float(s))))
        if rng.random() < 0.1:
            d = F32(0)
        if rng.random() < 0.08:
            d = F32(g.max_d)
        e = int(rng.integers(-6, 7))
        uls, vls = int(c_round(F32(u_l * g.inv_scale[o]))), int(c_round(F32(v_l * g.inv_scale[o])))
        urs = int(c_round(F32(F32(u_l - d) * g.inv_scale[o])))
        # the left window copied to where the match should be found, clipped to the level
        y0, y1 = max(vls - 5, 0), min(vls + 6, h)
        x0, x1 = max(-5, -uls, -urs), min(6, w - uls, w - urs)
        if y0 < y1 and x0 < x1:
            blk = L[o][y0:y1, uls + x0:uls + x1].astype(np.int64) + rng.integers(-2, 3, (y1 - y0, x1 - x0))
            R[o][y0:y1, urs + x0:urs + x1] = np.clip(blk, 0, 255).astype(np.uint8)
        o_r = int(np.clip(o + rng.choice([0, 0, 0, 1, -1, 2, -2]), 0, g.nlevels - 1))
        x_r = F32(F32(urs + e) * s)
        if rng.random() < 0.15:
            x_r = F32(u_l - d)
        y_r = F32(v_l + F32(rng.uniform(-1.5, 1.5) * float(s)))
        k = int(rng.choice([0, 5, 30, 60, 74, 75, 76, 99, 100, 120])) if rng.random() < 0.5 else int(rng.integers(0, 121))
        kr_rows.append((x_r, y_r, o_r))
        dr_rows.append(flip_bits(dl[i], k, first=int(rng.integers(0, 130))))
        if rng.random() < 0.1:      # a second right keypoint at the same distance, elsewhere
            kr_rows.append((F32(x_r - F32(3) * s), y_r, o_r))
            dr_rows.append(flip_bits(dl[i], k, first=130))
    order = rng.permutation(len(kr_rows))
    kr = np.zeros(len(kr_rows), KP_DTYPE)
    for j, src in enumerate(order):
        kr["x"][j], kr["y"][j], kr["octave"][j] = kr_rows[src]
    dr = np.array(dr_rows, np.uint8)[order]
    kl["size"], kr["size"] = 31.0, 31.0
    case = dict(geom=g, left=L, right=R, kl=kl, dl=dl, kr=kr, dr=dr, mb=g.mb, mbf=g.mbf)
    # matches with exactly zero disparity: octave-0 keypoints moved onto the bestuR the restatement finds for them
    oct0 = np.flatnonzero(kl["octave"] == 0)
    res = run(dict(case, kl=kl[oct0], dl=dl[oct0]))
    moved = 0
    for j, i in enumerate(oct0):
        if res.code[j] in ("KEPT", "CUT", "DISP_RANGE") and moved < 6 and np.isfinite(res.delta[j]):
            ir = res.best_idx[j]
            t = F32(F32(c_round(kr["x"][ir]) + F32(res.best_inc[j])) + res.delta[j])
            if c_round(t) == c_round(kl["x"][i]) and kr["x"][ir] <= t:
                kl["x"][i] = t
                moved += 1
    return case


RANDOM_SEEDS = tuple(range(20))    # test_cpu_stereo.py checks that every outcome code occurs over them, per geometry
_random = {}


def random_cases(geometry):
    """[(case, restatement result)] over RANDOM_SEEDS, computed once per process; callers must not modify them."""
    if geometry not in _random:
        _random[geometry] = [(c, run(c)) for c in (random_case(s, geometry) for s in RANDOM_SEEDS)]
    return _random[geometry]
