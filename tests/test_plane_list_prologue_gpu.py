"""The plane scan's block prologue: a static first batch per thread block (vt_plan.h:
take_plan), the counter handing out only the batches beyond, template planes, TS and the
first batch asked for in one round trip, the second batch's ids off the critical path.

130 templates (blocks of 64, 64 and 2).  Index and score against the oracle and against the
keys of RS_VT_PRUNE=0, bit for bit; prune_stats() / prune_verified() against the NumPy rule
after every call.  Sizes 1, 3, 4, 5, 28, 29, 32, 33, 37 and 300 give list lengths around
every multiple of four, one group (G = 1) and eight, groups with no batch beside groups with
one, and lists served by fewer blocks than the grid holds.  Mixed batches put a chosen
number of queries (1, 5; 0, 3) on list 1 of blocks 0 and 1 through twins inside the block
and leave block 2's lists empty.  The sequences run every size on one handle, long and short
lists in turn, with dense launches between them: the counters are never reset, so one left
non-zero by any launch shows as a wrong key in the next."""
import functools

import numpy as np
import pytest

from oracle import view_templates as V
from test_plane_ondemand_gpu import T, THR, Case, base_library, forced, frozen, miss_case, noised
from test_prune_verify_rule import score_matrix

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 28, 29, 32, 33, 37, 300]
ALTERNATING = [300, 1, 37, 3, 33, 4, 32, 5, 29, 28]     # long and short lists in turn
TWINS = [(1, 0), (5, 0), (1, 3), (5, 3)]               # queries on list 1 of block 0, of block 1
NTW, NHIT = 8, 340


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


class Pool:
    """Per-query reference values (the rule's are per query), composed by index."""

    def __init__(self, c):
        self.lib, self.queries, self.scores = c.lib, c.queries, c.scores
        self.idx, self.best, self.ver, self.pairs, self.ntb = c.idx, c.best, c.ver, c.pairs, c.ntb

    def take(self, sel):
        c = Case.__new__(Case)
        sel = np.asarray(sel)
        c.lib, c.queries, c.scores = self.lib, frozen(self.queries[sel]), self.scores[sel]
        c.idx, c.best, c.ver, c.pairs, c.ntb = self.idx[sel], self.best[sel], self.ver[sel], self.pairs[sel], self.ntb
        return c


@functools.lru_cache(maxsize=None)
def twin_library():
    lib = base_library().copy()
    lib[40] = lib[12]      # twins inside block 0
    lib[100] = lib[90]     # twins inside block 1
    return frozen(lib)


@functools.lru_cache(maxsize=None)
def pool():
    """[0, NTW): noised template 12 (unsettled, candidate block 0); [NTW, 2 NTW): noised
    template 90 (unsettled, block 1); then plain hits: settled by the verification, on no
    list; then the all-miss queries."""
    lib = twin_library()
    hits, _ = V.synthetic_queries(lib, NHIT + 60, seed=271, hit_frac=1.0)
    q = np.concatenate([noised(lib[12], NTW, 272, True), noised(lib[90], NTW, 273, True), hits, miss_case().queries])
    p = Pool(Case(lib, q))
    assert not p.ver[:2 * NTW].any()
    assert (p.idx[:NTW] == 12).all() and (p.idx[NTW:2 * NTW] == 90).all()
    h0 = 2 * NTW
    plain = h0 + np.flatnonzero(p.ver[h0:h0 + NHIT + 60] & (p.pairs[h0:h0 + NHIT + 60] == 0))
    assert len(plain) >= 300
    p.plain, p.miss0 = plain, h0 + NHIT + 60
    assert not p.ver[p.miss0:].any()
    return p


def mixed(nq, k0, k1):
    """nq queries: k0 on list 1 of block 0, k1 on list 1 of block 1, the rest plain hits
    (the twins spread through the batch)."""
    p = pool()
    k0, k1 = min(k0, nq), min(k1, max(0, nq - k0))
    sel = list(p.plain[:nq])
    for j in range(k0):
        sel[(j * 7) % nq if nq >= 7 * k0 + 7 * k1 else j] = j
    for j in range(k1):
        sel[(j * 7 + 3) % nq if nq >= 7 * k0 + 7 * k1 else k0 + j] = NTW + j
    c = p.take(sel)
    assert int((~c.ver).sum()) == k0 + k1
    return c


def misses(nq):
    p = pool()
    return p.take(np.arange(p.miss0, p.miss0 + nq))


def check(h, c, dense=None):
    nq = len(c.queries)
    idx, score, new = h.match_templates(c.queries, mode=0)
    assert not new.any()
    assert np.array_equal(score, c.best) and np.array_equal(idx, c.idx)
    if dense is not None:    # the keys of the dense launch (RS_VT_PRUNE=0)
        di, ds, _ = dense.match_templates(c.queries, mode=0)
        assert np.array_equal(di, idx) and np.array_equal(ds, score)
    return c.stats(nq)


@pytest.fixture
def handles(vtmod, monkeypatch):
    lib = twin_library()
    monkeypatch.setenv('RS_VT_PRUNE', '0')
    dense = vtmod.ViewTemplates._from_shape((64, 32), THR)
    dense.add(lib)
    h = forced(vtmod, monkeypatch, lib)
    yield h, dense
    h.close()
    dense.close()


@pytest.mark.parametrize('nq', SIZES)
def test_all_miss_batches(handles, nq):
    h, dense = handles
    c = misses(nq)
    for _ in range(2):
        want = check(h, c, dense)
        assert (h.prune_stats(), h.prune_verified()) == want


@pytest.mark.parametrize('nq', SIZES)
def test_hits_with_chosen_list_lengths_and_empty_lists(handles, nq):
    h, dense = handles
    for k0, k1 in TWINS:
        c = mixed(nq, k0, k1)
        for _ in range(2):
            want = check(h, c, dense)
            assert (h.prune_stats(), h.prune_verified()) == want


def test_every_size_in_turn_on_one_handle_with_dense_launches_between(handles):
    h, dense = handles
    for rnd, (k0, k1) in enumerate([(0, 0)] + TWINS):
        for i, nq in enumerate(ALTERNATING):
            c = misses(nq) if rnd == 0 else mixed(nq, k0, k1)
            want = check(h, c, dense if rnd < 2 else None)
            assert (h.prune_stats(), h.prune_verified()) == want
            if i % 3 == 0:     # a dense (matrix) launch on the same counters
                k = min(nq, 5)
                got = h.scores(c.queries[:k], t0=66, nt=7)
                assert np.array_equal(got, c.scores[:k, 66:73].astype(np.uint64))
            if i % 4 == 1:
                one = mixed(1, 1, 0) if rnd else misses(1)
                assert check(h, one) == (h.prune_stats(), h.prune_verified())


def test_pruned_and_dense_calls_in_turn_at_the_default_threshold(vtmod, monkeypatch):
    """RS_VT_PRUNE=1: 512 and more queries prune, 37, 64 and one query take the dense launch
    (the folded key export) on the same counters."""
    p = pool()
    h = forced(vtmod, monkeypatch, p.lib, prune='1')
    big = [np.concatenate([np.arange(p.miss0, p.miss0 + 300), p.plain[:212]]),
           np.concatenate([p.plain[:300], np.arange(5), p.plain[:207]]),
           np.concatenate([np.arange(p.miss0, p.miss0 + 13), p.plain[:300], p.plain[:287], np.arange(NTW, NTW + 3)])]
    for sel in big:
        c = p.take(sel)
        want = check(h, c)
        assert (h.prune_stats(), h.prune_verified()) == want
        for small in (mixed(37, 5, 3), misses(64), mixed(1, 1, 0), misses(37), mixed(64, 1, 3)):
            check(h, small)
            assert (h.prune_stats(), h.prune_verified()) == want    # a dense call leaves them
    h.close()


@functools.lru_cache(maxsize=None)
def h32_case():
    lib = V.synthetic_library(T, 32, 32, seed=274)
    q, _ = V.synthetic_queries(lib, 70, seed=275, hit_frac=0.5)
    sc = score_matrix(lib, q)
    return frozen(lib), frozen(q), sc.argmin(axis=1), sc.min(axis=1).astype(np.uint64)


@pytest.mark.parametrize('nq', [1, 4, 5, 70])
def test_dense_prologue_at_height_32(vtmod, nq):
    lib, q, idx, best = h32_case()
    h = vtmod.ViewTemplates._from_shape((32, 32), THR)
    h.add(lib)
    for _ in range(2):
        gi, gs, _ = h.match_templates(q[:nq], mode=0)
        assert np.array_equal(gi, idx[:nq]) and np.array_equal(gs, best[:nq])
    h.close()


def test_match_stream_from_device_memory_equals_the_per_batch_calls(handles):
    from pyratslam_amd import _lib
    h, dense = handles
    cs = [mixed(37, 5, 3), misses(37), mixed(37, 1, 0)]
    q = np.ascontiguousarray(np.stack([c.queries for c in cs]))
    per = [h.match_templates(c.queries, mode=0)[:2] for c in cs]
    for hh in (h, dense):
        buf = _lib.DeviceBuffer(q.nbytes).upload(q)
        idx, score = hh.match_stream((3, 37, buf))[:2]
        buf.close()
        for b, c in enumerate(cs):
            assert np.array_equal(idx[b], per[b][0]) and np.array_equal(score[b], per[b][1])
            assert np.array_equal(idx[b], c.idx) and np.array_equal(score[b], c.best)
    ver = np.concatenate([c.ver for c in cs])
    pairs = np.concatenate([c.pairs for c in cs])
    assert (h.prune_stats(), h.prune_verified()) == ((111, int(pairs.sum()), 3 * 111, 2), int(ver.sum()))
