"""k_hamming_best2_pairs / hamming_block_mfma (csrc/hamming.hip) at their query-side and batch edges,
with synthetic descriptors, bit for bit against the oracle's hamming_best2.

Batch.bind(desc=, counts=) lets a test write descriptors and per-frame counts straight into device
buffers; ygzfe_batch_match reads exactly those bound buffers (csrc/api_hamming.cpp: b->ws.desc / b->ws.counts),
so no extraction is needed.  Covered here and nowhere else in the suite:

* frames with 0 rows as train and as query, counts either side of the 32-query group, the 64-lane
  wave, the 256-query workgroup (kHamQPB; the `blockIdx.x * kHamQPB >= nq` return and the
  inactive-wave path `active = qw < nq`) and the full kp_cap;
* arbitrary pair lists (the C ABI allows them): every count as query and as train against a small
  and a large frame, a frame against itself, reversed, repeated and non-adjacent pairs;
* rows >= counts[q] of all three outputs keep the sentinel they were filled with; a pair whose query
  frame is empty keeps its whole row; an empty train frame gives -1 / 257 / 257;
* descriptor rows past counts[f] are poisoned with exact copies of the queries (the first rows of
  every frame, so every pair's early queries have a copy right behind its train frame's last row,
  inside the partial tile): they must never be chosen.  The same poison through the single-call
  kernel: the Python binding (ORBmatcher.best2) copies exactly nt rows, so it cannot pass a longer
  train buffer; the C ABI's device entry ygzfe_hamming_best2_device can, and is used for that;
* the fused accumulator keys' full range at scale: 8,192 train rows (and 8,193, the unfused form),
  D = 0 and D = 256 with indices up to 8191 (2^23 + (512 << 13) + 8191);
* query counts 255 / 256 / 257 / 513 in the single call, ties planted at the first and last rows.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu
SENTINEL = -7
COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513]  # + kp_cap
PARAMS = (600, 2.0, 1, 20, 7, 0)  # one level of 600 features: kp_cap >= 612, the smallest that holds 513
W, H = 320, 240


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _same(got, want, what):
    for name, g, w in zip(("best index", "best distance", "second distance"), got, want):
        assert np.array_equal(g, w), f"{what}: {name} differs from the oracle at rows {np.flatnonzero(g != w)[:8]}"


def test_batch_check_before_any_extraction(gpu):
    """A batch that has not extracted (it may only match or align bound buffers) reports no octree
    overflow: the flag ygzfe_batch_check reads is cleared when the batch is created."""
    for _ in range(3):
        gpu.Batch(PARAMS, 0, W, H, 2).check()


@pytest.fixture(scope="module")
def poisoned_batch(gpu):
    """One batch of 14 frames with the counts above: random valid rows, the rows past each count
    copies of the other frames' (and its own) first rows, matched over an arbitrary pair list."""
    import torch
    F = len(COUNTS) + 1
    b = gpu.Batch(PARAMS, 0, W, H, F)
    cap = b.kp_cap
    assert cap > COUNTS[-1], cap
    counts = np.array(COUNTS + [cap], np.int32)
    rng = np.random.default_rng(2024)
    desc = np.zeros((F, cap, 32), np.uint8)
    for f in range(F):
        desc[f, :counts[f]] = rand_desc(rng, counts[f])
    valid = [desc[f, :counts[f]].copy() for f in range(F)]
    nonempty = [f for f in range(F) if counts[f] > 0]
    for f in range(F):  # poison: row counts[f] + j = row (j // 13) of non-empty frame j % 13
        for j in range(cap - counts[f]):
            g = nonempty[j % len(nonempty)]
            desc[f, counts[f] + j] = valid[g][(j // len(nonempty)) % counts[g]]
    small, large = COUNTS.index(33), F - 1
    pairs = []
    for f in range(F):
        pairs += [(f, small), (f, large), (small, f), (large, f), (f, f)]
    pairs += [(3, 9), (9, 3), (3, 9), (12, 1), (1, 12), (0, 0), (large, 0), (0, large)]  # reversed, repeated, empty
    qf = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device="cuda")
    tf = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device="cuda")
    d_desc = torch.from_numpy(desc).cuda()
    d_counts = torch.from_numpy(counts).cuda()
    b.bind(desc=d_desc.data_ptr(), counts=d_counts.data_ptr())
    out = [torch.full((len(pairs), cap), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    b.match(len(pairs), qf.data_ptr(), tf.data_ptr(), *(o.data_ptr() for o in out))
    torch.cuda.synchronize()
    b.check()
    got = [o.cpu().numpy() for o in out]
    del b  # before the bound tensors go
    return {"pairs": pairs, "counts": counts, "valid": valid, "got": got, "cap": cap}


def test_batch_pairs_every_count_vs_oracle(poisoned_batch):
    """Rows [0, counts[q]) of every pair equal the oracle's best2 of the VALID rows only: a poisoned
    row chosen (an exact copy of a query) would show as distance 0 at an index >= counts[t]."""
    pb = poisoned_batch
    seen_q, seen_t = set(), set()
    for p, (q, t) in enumerate(pb["pairs"]):
        nq, nt = pb["counts"][q], pb["counts"][t]
        want = O.hamming_best2(pb["valid"][q], pb["valid"][t])
        _same([g[p, :nq] for g in pb["got"]], want, f"pair {p} (query frame {q}: {nq} rows, train frame {t}: {nt} rows)")
        if nq and nt:
            assert pb["got"][0][p, :nq].max() < nt
        seen_q.add(int(nq))
        seen_t.add(int(nt))
    assert seen_q == seen_t == set(COUNTS + [pb["cap"]])


def test_batch_pairs_rows_past_the_query_count_untouched(poisoned_batch):
    pb = poisoned_batch
    for p, (q, t) in enumerate(pb["pairs"]):
        nq = pb["counts"][q]
        for g in pb["got"]:
            assert (g[p, nq:] == SENTINEL).all(), f"pair {p} ({q}, {t}): rows >= {nq} written"
    empty_q = [p for p, (q, t) in enumerate(pb["pairs"]) if pb["counts"][q] == 0]
    assert len(empty_q) >= 5  # against small, large, itself, and as listed
    for p in empty_q:
        assert all((g[p] == SENTINEL).all() for g in pb["got"])


def test_batch_pairs_empty_train_frame(poisoned_batch):
    pb = poisoned_batch
    hits = [(p, q) for p, (q, t) in enumerate(pb["pairs"]) if pb["counts"][t] == 0 and pb["counts"][q] > 0]
    assert {int(pb["counts"][q]) for _, q in hits} >= {33, pb["cap"]}
    for p, q in hits:
        nq = pb["counts"][q]
        bi, bd, sd = (g[p, :nq] for g in pb["got"])
        assert (bi == -1).all() and (bd == 257).all() and (sd == 257).all(), f"pair {p}"


def test_batch_pairs_repeated_pair_rows_equal(poisoned_batch):
    pb = poisoned_batch
    rows = [p for p, pr in enumerate(pb["pairs"]) if pr == (3, 9)]
    assert len(rows) == 2
    for g in pb["got"]:
        assert np.array_equal(g[rows[0]], g[rows[1]])


@pytest.mark.parametrize("nq,nt", [(70, 1), (70, 31), (70, 33), (257, 63), (257, 95), (513, 255), (40, 8191)])
def test_best2_device_poisoned_rows_past_nt(gpu, nq, nt):
    """The single-call kernel on a train buffer longer than nt whose rows past nt are exact copies
    of the queries (the buffer resource's nt * 32 bound and the partial tile's row mask)."""
    import torch
    rng = np.random.default_rng(nq * 31 + nt)
    q, t = rand_desc(rng, nq), rand_desc(rng, nt)
    q[1] = 0  # an all-zero query: a row past nt that reads as zero would be at distance 0
    buf = np.concatenate([t, q, q[:64]])
    d_q, d_t = torch.from_numpy(q).cuda(), torch.from_numpy(buf).cuda()
    out = [torch.full((nq + 5,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    rc = gpu.lib().ygzfe_hamming_best2_device(C.c_void_p(d_q.data_ptr()), nq, C.c_void_p(d_t.data_ptr()), nt,
                                              *(C.c_void_p(o.data_ptr()) for o in out), C.c_void_p(None))
    assert rc == 0
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in out]
    _same([g[:nq] for g in got], O.hamming_best2(q, t), f"nq {nq} nt {nt}")
    assert all((g[nq:] == SENTINEL).all() for g in got)


@pytest.mark.parametrize("nt", [8192, 8193])
@pytest.mark.parametrize("pattern", ["last_zero", "last_one", "all_one"])
def test_best2_key_range_at_scale(gpu, nt, pattern):
    """D = -256 .. +256 with train indices up to 8191 (tile 255) and, unfused, 8192: rows 0, 4100,
    8160 and the last all-one or all-zero among random rows; all-zero, all-one and random queries."""
    rng = np.random.default_rng(nt + len(pattern))
    t = rand_desc(rng, nt)
    special = [0, 4100, 8160, nt - 1]
    if pattern == "last_zero":      # all-zero query: D = 0 only at the last index; all-one: ties at 0 / 4100 / 8160
        t[special[:3]] = 255
        t[nt - 1] = 0
    elif pattern == "last_one":     # all-zero query against an all-one last row: the largest key there is
        t[special[:3]] = 0
        t[nt - 1] = 255
    else:                           # every key at D = +256 for the all-zero query
        t[:] = 255
    q = rand_desc(rng, 70)
    q[0], q[1], q[33], q[69] = 0, 255, 0, 255
    got = gpu.ORBmatcher().best2(q, t)
    _same(got, O.hamming_best2(q, t), f"nt {nt} {pattern}")
    bi, bd, sd = got
    if pattern == "last_zero":
        assert (bi[0], bd[0]) == (nt - 1, 0) and (bi[1], bd[1], sd[1]) == (0, 0, 0)
    elif pattern == "last_one":
        assert (bi[0], bd[0], sd[0]) == (0, 0, 0) and (bi[1], bd[1]) == (nt - 1, 0)
    else:
        assert (bi[0], bd[0], sd[0]) == (0, 256, 256) and (bi[69], bd[69], sd[69]) == (0, 0, 0)


@pytest.mark.parametrize("nq", [255, 256, 257, 513])
@pytest.mark.parametrize("nt", [97, 1000])
def test_best2_query_side_sizes(gpu, nq, nt):
    """Query counts either side of the 256-query workgroup (and two workgroups + 1) in the single
    call, with ties planted at the first and last train rows for the first and the last query."""
    rng = np.random.default_rng(nq * 7 + nt)
    q, t = rand_desc(rng, nq), rand_desc(rng, nt)
    t[0] = t[nt - 1] = q[0]
    t[1] = t[nt - 2] = q[nq - 1]
    got = gpu.ORBmatcher().best2(q, t)
    _same(got, O.hamming_best2(q, t), f"nq {nq} nt {nt}")
    bi, bd, sd = got
    assert (bi[0], bd[0], sd[0]) == (0, 0, 0) and (bi[nq - 1], bd[nq - 1], sd[nq - 1]) == (1, 0, 0)
