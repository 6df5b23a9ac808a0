"""The timed step's match results (C5Shard.bi / bd / sd) and its slot chi2 under every schedule,
at sequences of 11 and 12 frames.

tests/test_gpu_c5.py compares slots and counts over the 13,728-frame sequence; slots carry no match
results.  The chunked and `pipe` steps write chunk c's pairs at row offset s_c from per-chunk
batches, `pipe` on a second stream (ygzfe/sequence.py _match / _step_pipe / _step_chunked), so an
offset, an ordering or a missing stream edge there shows only in bi / bd / sd.  Here every pair row
p of every schedule is compared bit for bit with the oracle's hamming_best2 of the descriptors of
frames p + 1 (query) and p (train), the descriptors taken from the run's own slots (which
test_gpu_c5.py pins to the oracle's extraction), rows past the query count must keep the sentinel
the buffers were filled with, and all schedules of one sequence must agree.

Chunk shapes (s_c, L_c, hc, nc) = (first local frame, frames, own-frame offset, own frames) seen:
  n_seq 11, 4 chunks:          (0,3,0,3) (2,4,1,3) (5,4,1,3) (8,3,1,2)   unequal, Pc = 2,3,3,2
  n_seq 12, 4 chunks:          (0,3,0,3) (2,4,1,3) (5,4,1,3) (8,4,1,3)
  n_seq 11, pipe 2:            (0,6,0,6) (5,6,1,5);   n_seq 12, pipe 2: (0,6,0,6) (5,7,1,6)
  n_seq 11, world 2 rank 1 (frames 6..10 + halo 5), 2 chunks: (0,4,1,3) (3,3,1,2)
  n_seq 11, world 2 rank 1, 4 chunks: (0,3,1,2) (2,3,1,2) (4,2,1,1) (5,1,1,0)   Pc = 1 and an empty chunk
  n_seq 12, world 2 rank 1, 2 chunks: (0,4,1,3) (3,4,1,3);  4 chunks: (0,3,1,2) (2,3,1,2) (4,3,1,2) (6,1,1,0)
An empty chunk (nc == 0) is skipped by both steps.  No chunk with own frames but no pair (Pc == 0)
arises at these sizes: every non-empty chunk after the first carries the frame before it.
"""
import numpy as np
import pytest
import torch

import _align_cases as A
import _oracle as O
import _scenes as S
import ygzfe
from ygzfe import dist as D
from ygzfe.sequence import C5Shard

pytestmark = pytest.mark.gpu
SENTINEL = -7
SCHEDULES = [("serial", 1), ("tail", 1), ("split", 1), ("overlap", 1), ("serial", 4), ("pipe", 2), ("pipe", 4)]


def _step(sh):
    for t in (sh.bi, sh.bd, sh.sd):
        t.fill_(SENTINEL)
    torch.cuda.synchronize()
    sh.step()
    torch.cuda.synchronize()
    sh.check()


def _frames_desc(sh):
    """Descriptors of this rank's own frames, from its slots: {global frame: [n, 32] uint8}."""
    slots = sh.local_slots().cpu().numpy()
    out = {}
    for i in range(sh.n_own):
        u = D.unpack_slot(slots[i], sh.cap, ygzfe.KP_DTYPE)
        assert u["frame"] == sh.b0 + i
        out[sh.b0 + i] = u["desc"].copy()
    return out


class Ref:
    """The unsharded serial run of an n_seq-frame sequence: descriptors per frame, the oracle's
    best / second best per pair (computed once), and the run's own bi / bd / sd."""

    def __init__(self, n_seq):
        dev = torch.device("cuda", 0)
        self.sh = sh = C5Shard(n_seq, 0, 1, dev)
        _step(sh)
        self.desc = _frames_desc(sh)
        self.want = {g: O.hamming_best2(self.desc[g + 1], self.desc[g]) for g in range(n_seq - 1)}
        self.slots = sh.local_slots().clone()
        self.match = _check_match(sh, self.desc, self.want, "serial/1")


def _check_match(sh, desc, want, what):
    """Row p of bi / bd / sd = the oracle's best2 of global frames (hb + p + 1) against (hb + p)."""
    bi, bd, sd = (t.cpu().numpy() for t in (sh.bi, sh.bd, sh.sd))
    assert bi.shape == (sh.P, sh.cap)
    rows = {}
    for p in range(sh.P):
        g = sh.hb + p
        n = len(desc[g + 1])
        ri, rd, rs = want[g]
        for name, got, ref in (("bi", bi, ri), ("bd", bd, rd), ("sd", sd, rs)):
            assert np.array_equal(got[p, :n], ref), f"{what}: {name} of pair ({g}, {g + 1}) differs from the oracle"
            assert (got[p, n:] == SENTINEL).all(), f"{what}: {name} rows >= {n} of pair ({g}, {g + 1}) written"
        rows[g] = (bi[p, :n].copy(), bd[p, :n].copy(), sd[p, :n].copy())
    return rows


@pytest.fixture(scope="module")
def refs(gpu):
    cache = {}

    def get(n_seq):
        if n_seq not in cache:
            cache[n_seq] = Ref(n_seq)
        return cache[n_seq]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _shapes(sh):
    return [(s_c, L_c, hc, nc) for (s_c, L_c, hc, nc, bt, bufs, row0) in sh.chunks]


@pytest.mark.parametrize("n_seq", [11, 12])
@pytest.mark.parametrize("schedule,chunks", SCHEDULES)
def test_step_match_results_every_schedule(refs, n_seq, schedule, chunks):
    ref = refs(n_seq)
    dev = torch.device("cuda", 0)
    sh = C5Shard(n_seq, 0, 1, dev, chunks=chunks, schedule=schedule)
    what = f"n_seq {n_seq} {schedule}/{chunks}"
    print(what, "chunk shapes", _shapes(sh))
    for rep in range(2 if schedule == "pipe" else 1):  # pipe's second step reuses the chunk buffers
        _step(sh)
        got = _check_match(sh, ref.desc, ref.want, f"{what} step {rep}")
        assert torch.equal(sh.local_slots(), ref.slots), f"{what} step {rep}: slots differ from serial"
        for g in got:  # equal across the schedules (each equals the serial run's)
            assert all(np.array_equal(a, b) for a, b in zip(got[g], ref.match[g])), (what, g)
    if chunks == 4 and n_seq == 11:
        assert _shapes(sh) == [(0, 3, 0, 3), (2, 4, 1, 3), (5, 4, 1, 3), (8, 3, 1, 2)]  # unequal chunks
    if chunks == 2 and n_seq == 11:
        assert _shapes(sh) == [(0, 6, 0, 6), (5, 6, 1, 5)]


@pytest.mark.parametrize("n_seq", [11, 12])
@pytest.mark.parametrize("schedule,chunks", [("serial", 1), ("serial", 2), ("pipe", 2), ("pipe", 4)])
def test_step_match_results_virtual_shard(refs, n_seq, schedule, chunks):
    """Rank 1 of 2 on this GPU (gather off): pair row p is global frames (hb + p, hb + p + 1), the
    halo frame's descriptors from the unsharded run."""
    ref = refs(n_seq)
    dev = torch.device("cuda", 0)
    sh = C5Shard(n_seq, 1, 2, dev, chunks=chunks, schedule=schedule, gather=False)
    what = f"n_seq {n_seq} rank 1/2 {schedule}/{chunks}"
    print(what, "chunk shapes", _shapes(sh))
    assert sh.hb == sh.b0 - 1 and sh.P == sh.n_own
    for rep in range(2 if schedule == "pipe" else 1):
        _step(sh)
        own = _frames_desc(sh)
        for g, d in own.items():
            assert np.array_equal(d, ref.desc[g]), f"{what}: frame {g}'s descriptors differ from the unsharded run"
        got = _check_match(sh, ref.desc, ref.want, f"{what} step {rep}")
        assert torch.equal(sh.local_slots(), ref.slots[sh.b0:sh.e0]), f"{what} step {rep}: slots differ"
        for g in got:
            assert all(np.array_equal(a, b) for a, b in zip(got[g], ref.match[g])), (what, g)
    if chunks == 4:
        assert [s[3] for s in _shapes(sh)][-1] == 0      # an empty last chunk (nc == 0)
        if n_seq == 11:
            assert (4, 2, 1, 1) in _shapes(sh)           # a one-pair chunk


@pytest.mark.parametrize("schedule,chunks", [("serial", 1), ("pipe", 4)])
def test_step_slot_chi2_vs_oracle(refs, schedule, chunks):
    """Header word 9 of a few frames' slots (and the [P, 45] record's chi2 / H behind it) against the
    oracle's Gauss-Newton run of that pair, under the serial and the bench's default schedule."""
    n_seq = 11
    ref = refs(n_seq)
    if (schedule, chunks) == ("serial", 1):
        sh = ref.sh
    else:
        sh = C5Shard(n_seq, 0, 1, torch.device("cuda", 0), chunks=chunks, schedule=schedule)
        _step(sh)
    W, H, nf, sf, nl, ini, mn = S.CONFIGS["C2"]
    orc = O.OrbOracle(nf, sf, nl, ini, mn)
    slots = sh.local_slots().cpu().numpy()
    rec = sh.align_records()
    T0 = O.se3_from((0, 0, 0, 1), (0, 0, 0))
    for g in (1, 3, 6, 9, 10):  # first pair, both sides of the chunk edges, the last pair
        prev = D.unpack_slot(slots[g - 1], sh.cap, ygzfe.KP_DTYPE)
        cur = D.unpack_slot(slots[g], sh.cap, ygzfe.KP_DTYPE)
        n = prev["n"]
        o = O.sparse_align(orc.pyramid(ref.sh.batch.read_level(g - 1, 0)), orc.pyramid(ref.sh.batch.read_level(g, 0)),
                           orc.inv_scale, O.Cam(*sh.cam), prev["kps"], sh.xyz[g - 1, :n].cpu().numpy(),
                           np.ones(n, np.uint8), 3, 1, T0)
        assert cur["has_align"] and cur["n_visible"] == o.n_visible, g
        dc = A.chi2_dev(cur["chi2"], o.chi2)
        dh = A.h_dev(rec[g - 1, 9:45], o.H[:])
        print(f"{schedule}/{chunks} frame {g}: slot chi2 {cur['chi2']:.4f} vs {o.chi2:.4f} ({dc:.2e}), H dev {dh:.2e}")
        assert dc <= A.CHI2_TOL, f"frame {g}: slot chi2 {cur['chi2']} vs the oracle's {o.chi2}"
        assert np.float32(rec[g - 1, 8]) == np.float32(cur["chi2"]), g
        assert dh <= A.H_TOL, f"pair ({g - 1}, {g}): H differs by {dh:.2e}"
