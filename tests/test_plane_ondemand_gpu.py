"""Query planes on demand in the pruned plane scan: ahead of a pruned scan only the compact
planes (the aligned start rows) are built, the prefilter and the verification shift every
other start row out of them, and the verification expands into the full layout exactly the
queries a scan pass stages (unsettled: list1; another block's bound <= U0: list2).  Every
other reader of the full planes expands all queries first.

Index and score against the oracle, bit for bit, with RS_VT_PRUNE=force on a 64 x 32
library of 130 templates (blocks of 64, 64 and 2) at 1, 4, 37 and 300 queries, and
prune_stats() / prune_verified() against the NumPy rule (test_prune_subunit_bound.
pruned_per_query): equal to the rule, unchanged when read twice, unchanged after a call
that does not prune, and counted from zero again by the next pruned call (the counters are
reset by the list kernels themselves; there is no closing launch)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import view_templates as V
from test_prune_subunit_bound import pruned_per_query
from test_prune_verify_rule import score_matrix

pytestmark = pytest.mark.gpu

T, NTB, THR = 130, 3, 45000
COUNTS = [1, 4, 37, 300]
NQ_MAX = max(COUNTS)


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


def frozen(a):
    a.setflags(write=False)
    return a


def noised(t, n, seed, shift=False):
    rng = np.random.default_rng(seed)
    out = np.clip(t.astype(np.int16)[None] - rng.integers(0, 4, size=(n, 64, 32)), 0, 255).astype(np.uint8)
    if shift:
        for i in range(n):
            out[i] = np.roll(out[i], (i % 15) - 7, axis=0)
    return out


class Case:
    """A library, NQ_MAX queries, their score matrix and what the rule predicts per query."""

    def __init__(self, lib, queries):
        self.lib, self.queries = frozen(lib), frozen(queries)
        self.scores = frozen(score_matrix(lib, queries))
        self.idx, self.best = self.scores.argmin(axis=1), self.scores.min(axis=1).astype(np.uint64)
        self.ver, self.pairs = pruned_per_query(lib, queries, scores=self.scores)
        self.ntb = (len(lib) + 63) // 64

    def stats(self, nq):
        return (nq, int(self.pairs[:nq].sum()), self.ntb * nq, 2), int(self.ver[:nq].sum())


@functools.lru_cache(maxsize=None)
def base_library():
    return frozen(V.synthetic_library(T, 64, 32, seed=171))


@functools.lru_cache(maxsize=None)
def miss_case():
    rng = np.random.default_rng(172)
    return Case(base_library(), rng.integers(0, 256, size=(NQ_MAX, 64, 32), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def mixed_case():
    """Hits, and in turn: a twin in another block (settled, and on list2), a twin in the
    same block (unsettled), a decoy in a lower block than the match (unsettled there, the
    match found by pass B2), a miss."""
    rng = np.random.default_rng(173)
    lib = base_library().copy()
    lib[70] = lib[5]                                   # twins in blocks 0 and 1
    lib[40] = lib[12]                                  # twins in block 0
    lib[3] = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    lib[3, 16:48] = lib[129, 16:48]                    # the decoy of template 129, in block 0
    kinds = [noised(lib[5], NQ_MAX, 174, True), noised(lib[12], NQ_MAX, 175, True), noised(lib[129], NQ_MAX, 176),
             V.synthetic_queries(lib, NQ_MAX, seed=177, hit_frac=1.0)[0],
             rng.integers(0, 256, size=(NQ_MAX, 64, 32), dtype=np.uint8)]
    pick = (np.arange(NQ_MAX) * 7) % 11
    sel = np.where(pick < 5, pick, 3)                  # more than half are plain hits
    q = np.stack([kinds[k][i] for i, k in enumerate(sel)])
    c = Case(lib, q)
    n = 37
    assert c.ver[:n][sel[:n] == 0].all() and (c.pairs[:n][sel[:n] == 0] >= 1).all()
    assert not c.ver[:n][sel[:n] == 1].any() and not c.ver[:n][sel[:n] == 2].any()
    assert (c.idx[sel == 2] == 129).all() and (c.pairs[:n][sel[:n] == 2] >= 1).all()
    plain = (sel == 3) & c.ver & (c.pairs == 0)        # settled, on no list: never expanded
    assert plain[:n].sum() >= n // 3 and not c.ver[sel == 4].any()
    return c


@functools.lru_cache(maxsize=None)
def offsets_case(settled):
    lib = base_library().copy()
    if not settled:
        lib[1:64:2] = lib[0:63:2]                      # pairs of twins within block 0: never settled
    src = (2 * np.arange(NQ_MAX)) % 64 if not settled else (37 * np.arange(NQ_MAX)) % T
    q = np.stack([np.roll(lib[s], (i % 15) - 7, axis=0) for i, s in enumerate(src)])
    c = Case(lib, q)
    assert (c.best == 0).all() and np.array_equal(c.idx, src)
    assert c.ver.all() if settled else not c.ver.any()
    return c


@functools.lru_cache(maxsize=None)
def zeros_case():
    return Case(np.full((T, 64, 32), 255, dtype=np.uint8), np.zeros((NQ_MAX, 64, 32), dtype=np.uint8))


def forced(vtmod, monkeypatch, lib, prune='force'):
    monkeypatch.setenv('RS_VT_PRUNE', prune)
    h = vtmod.ViewTemplates._from_shape((64, 32), THR)
    assert h.scan_form() == 'plane-pruned' and h.prune_stats() == (0, 0, 0, 0) and h.prune_verified() == 0
    h.add(lib)
    return h


def match(h, c, nq):
    idx, score, new = h.match_templates(c.queries[:nq], mode=0)
    assert not new.any()
    assert np.array_equal(score, c.best[:nq])
    assert np.array_equal(idx, c.idx[:nq])


def stats_contract(h, c, nq, rerun):
    """The rule's counts; read twice; after a scan that does not prune (a score matrix of a
    template range that starts in block 1, which reads every query's full planes); and
    from zero again on the next pruned call."""
    want = c.stats(nq)
    assert (h.prune_stats(), h.prune_verified()) == want
    assert (h.prune_stats(), h.prune_verified()) == want
    k = min(nq, 5)
    got = h.scores(c.queries[nq - k:nq], t0=66, nt=7)
    assert np.array_equal(got, c.scores[nq - k:nq, 66:73].astype(np.uint64))
    assert (h.prune_stats(), h.prune_verified()) == want
    rerun()
    assert (h.prune_stats(), h.prune_verified()) == want


@pytest.mark.parametrize('nq', COUNTS)
def test_stale_planes_cannot_hide_a_missing_expansion(vtmod, monkeypatch, nq):
    """All misses first (every query expanded), then other queries in the same slots: a
    query the verification must expand and does not would be scanned with the miss's planes."""
    miss, mixed = miss_case(), mixed_case()
    h = forced(vtmod, monkeypatch, mixed.lib)
    idx, score, _ = h.match_templates(miss.queries, mode=0)
    ref = score_matrix(mixed.lib, miss.queries[:8])
    assert np.array_equal(score[:8], ref.min(axis=1).astype(np.uint64)) and np.array_equal(idx[:8], ref.argmin(axis=1))
    assert h.prune_verified() == 0 and h.prune_stats()[0] == NQ_MAX
    match(h, mixed, nq)
    stats_contract(h, mixed, nq, lambda: match(h, mixed, nq))
    h.close()


@pytest.mark.parametrize('settled', [True, False], ids=['settled', 'unsettled'])
@pytest.mark.parametrize('nq', COUNTS)
def test_every_offset_as_the_unique_best(vtmod, monkeypatch, nq, settled):
    """Settled: every shift is taken in the verification.  Unsettled (a twin in the block):
    every shift is taken in the expansion, and the block scan reads its result."""
    c = offsets_case(settled)
    h = forced(vtmod, monkeypatch, c.lib)
    match(h, c, nq)
    stats_contract(h, c, nq, lambda: match(h, c, nq))
    h.close()


@pytest.mark.parametrize('nq', COUNTS)
def test_all_zero_queries_against_an_all_255_library(vtmod, monkeypatch, nq):
    c = zeros_case()
    assert (c.idx == 0).all()
    h = forced(vtmod, monkeypatch, c.lib)
    match(h, c, nq)
    stats_contract(h, c, nq, lambda: match(h, c, nq))
    h.close()


# --- keys equal to the dense launch's: streams and shards -------------------------
@pytest.mark.parametrize('where', ['device', 'host'])
@pytest.mark.parametrize('nq', COUNTS)
def test_match_stream_same_keys_as_the_dense_launch(vtmod, monkeypatch, where, nq):
    from pyratslam_amd import _lib
    c = mixed_case()
    nb = 3 if nq <= 37 else 1
    q = np.ascontiguousarray(np.stack([np.roll(c.queries, -b, axis=0)[:nq] for b in range(nb)]))
    # the stats are of the call's last launch: every batch (device-resident queries, or one
    # batch), or the last upload group, which for three host batches is the third alone
    bs = range(nb) if where == 'device' or nb == 1 else [nb - 1]
    last = Case.__new__(Case)
    last.ver = np.concatenate([np.roll(c.ver, -b)[:nq] for b in bs])
    last.pairs = np.concatenate([np.roll(c.pairs, -b)[:nq] for b in bs])
    last.ntb = c.ntb
    want = last.stats(len(bs) * nq)
    res = []
    for v in ('0', 'force'):
        monkeypatch.setenv('RS_VT_PRUNE', v)
        h = vtmod.ViewTemplates._from_shape((64, 32), THR)
        h.add(c.lib)

        def run():
            if where == 'device':
                buf = _lib.DeviceBuffer(q.nbytes).upload(q)
                out = h.match_stream((nb, nq, buf))
                buf.close()
                return out
            return h.match_stream(q)
        h.match_stream(np.ascontiguousarray(miss_case().queries[None]))   # stale planes of misses
        res.append(run())
        if v == 'force':
            assert (h.prune_stats(), h.prune_verified()) == want
            assert (h.prune_stats(), h.prune_verified()) == want
            run()
            assert (h.prune_stats(), h.prune_verified()) == want
        else:
            assert h.prune_stats()[3] == 0 and h.prune_verified() == 0
        h.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    for b in range(nb):
        assert np.array_equal(res[1][0][b], np.roll(c.idx, -b)[:nq])
        assert np.array_equal(res[1][1][b], np.roll(c.best, -b)[:nq])


def test_scan_local_on_three_shards_then_resolve_same_keys_as_the_dense_launch(vtmod, monkeypatch):
    from pyratslam_amd import _lib
    c = mixed_case()
    keys = []
    for v in ('0', 'force'):
        monkeypatch.setenv('RS_VT_PRUNE', v)
        shards = [vtmod.ShardedViewTemplates.from_shape((64, 32), THR, r, 3, reducer=lambda k: k) for r in range(3)]
        for s in shards:
            s.add(c.lib)
        per_call = []
        for nq in (300, 37, 4, 1):
            qs = np.ascontiguousarray(c.queries[:nq])
            local = []
            for r, s in enumerate(shards):
                k = np.empty(nq, dtype=np.uint64)
                _lib.check(s._lib.rs_vt_scan_local(s._h, nq, _lib.ptr(qs, ctypes.c_uint8), _lib.ptr(k, ctypes.c_uint64)))
                local.append(k)
                if v == 'force':                   # the shard's own templates: lib[r::3], one block
                    ver, pairs = shard_rule(r)
                    want = ((nq, int(pairs[:nq].sum()), nq, 2), int(ver[:nq].sum()))
                    assert (s.prune_stats(), s.prune_verified()) == want
                    assert (s.prune_stats(), s.prune_verified()) == want
            glob = np.minimum.reduce(local)
            for s in shards:                       # every rank resolves the global keys
                idx, score = np.empty(nq, dtype=np.int64), np.empty(nq, dtype=np.uint64)
                new = np.zeros(nq, dtype=np.uint8)
                _lib.check(s._lib.rs_vt_resolve(s._h, nq, _lib.ptr(glob, ctypes.c_uint64), 0,
                                                _lib.ptr(score, ctypes.c_uint64), _lib.ptr(idx, ctypes.c_int64),
                                                _lib.ptr(new, ctypes.c_uint8)))
                assert np.array_equal(idx, c.idx[:nq]) and np.array_equal(score, c.best[:nq]) and not new.any()
            per_call.append(local)
        keys.append(per_call)
        for s in shards:
            s.close()
    for a, b in zip(*keys):
        for ka, kb in zip(a, b):
            assert np.array_equal(ka, kb)


@functools.lru_cache(maxsize=None)
def shard_rule(rank):
    c = mixed_case()
    return pruned_per_query(c.lib[rank::3], c.queries, scores=c.scores[:, rank::3])


# --- SEQUENTIAL on a pruned handle: the candidates' matrix scan reads every query's planes --
@functools.lru_cache(maxsize=None)
def sequential_case():
    """Novel queries that become candidates, later queries that prefer one of them, hits."""
    rng = np.random.default_rng(178)
    lib = base_library()
    hits, _ = V.synthetic_queries(lib, NQ_MAX, seed=179, hit_frac=1.0)
    novel = rng.integers(0, 256, size=(NQ_MAX, 64, 32), dtype=np.uint8)
    q = np.empty((NQ_MAX, 64, 32), dtype=np.uint8)
    for i in range(NQ_MAX):
        if i % 3 == 0:
            q[i] = hits[i]
        elif i % 3 == 1 or i < 6:
            q[i] = novel[i]
        else:                                          # an earlier novel query again, shifted and noised
            q[i] = np.roll(noised(novel[i - 4], 1, 180 + i)[0], (i % 15) - 7, axis=0)
    out = {}
    for n in (37, 300):
        o = V.ViewTemplatesOracle.__new__(V.ViewTemplatesOracle)
        o.match_threshold, o.templates, o.locations = THR, list(lib), [(0, 0, 0)] * len(lib)
        out[n] = [o.match_template(q[i])[:2] for i in range(n)]
        assert sum(1 for _, new in out[n] if new) >= n // 4
        assert sum(1 for k, new in out[n] if not new and k >= T) >= n // 8
    return frozen(q), out


@pytest.mark.parametrize('nq', [37, 300])
def test_sequential_on_a_pruned_handle_learns_the_oracles_indices(vtmod, monkeypatch, nq):
    q, want = sequential_case()
    lib = base_library()
    h = forced(vtmod, monkeypatch, lib)
    idx, _, new = h.match_templates(q[:nq], mode=1)
    assert [(int(i), bool(n)) for i, n in zip(idx, new)] == want[nq]
    ver, pairs = pruned_per_query(lib, q[:nq])
    want_stats = ((nq, int(pairs.sum()), NTB * nq, 2), int(ver.sum()))
    assert (h.prune_stats(), h.prune_verified()) == want_stats
    assert (h.prune_stats(), h.prune_verified()) == want_stats
    assert h.count() == T + sum(1 for _, n in want[nq] if n)
    # the grown library, frozen: everything is found where the oracle put it
    idx2, score2, new2 = h.match_templates(q[:nq], mode=0)
    assert not new2.any() and np.array_equal(idx2, [k for k, _ in want[nq]])
    h.close()


# --- the default threshold: a pruned call, a small dense call, a pruned call ------------
def test_a_small_dense_call_between_two_pruned_calls(vtmod, monkeypatch):
    c, miss = mixed_case(), miss_case()
    q = np.concatenate([c.queries, miss.queries])[:512]
    sc = np.concatenate([c.scores, score_matrix(c.lib, miss.queries[:512 - NQ_MAX])])
    ver, pairs = pruned_per_query(c.lib, q, scores=sc)
    want = ((512, int(pairs.sum()), NTB * 512, 2), int(ver.sum()))
    h = forced(vtmod, monkeypatch, c.lib, prune='1')
    for _ in range(2):
        idx, score, _ = h.match_templates(q, mode=0)
        assert np.array_equal(idx, sc.argmin(axis=1)) and np.array_equal(score, sc.min(axis=1).astype(np.uint64))
        assert (h.prune_stats(), h.prune_verified()) == want
        assert (h.prune_stats(), h.prune_verified()) == want
        for nq in (37, 64):                            # below the threshold: the dense launch
            sub = q[100:100 + nq][::-1]
            idx, score, _ = h.match_templates(sub, mode=0)
            assert np.array_equal(idx, sc[100:100 + nq][::-1].argmin(axis=1))
            assert np.array_equal(score, sc[100:100 + nq][::-1].min(axis=1).astype(np.uint64))
            assert (h.prune_stats(), h.prune_verified()) == want
    h.close()
