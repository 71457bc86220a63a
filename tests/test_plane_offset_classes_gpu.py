"""The bit-plane scan's per-offset counts: every row offset -7..7 must reach the
minimum with its own count and its own TS(o), whatever order the kernel walks the
query start rows in and however it packs the counts.  Integer work: exact
equality with the oracle."""
import functools

import numpy as np
import pytest

from oracle import view_templates as V

pytestmark = pytest.mark.gpu

M = V.MAX_OFFSET


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


@functools.lru_cache(maxsize=None)
def _offset_case(h):
    """72 templates, 15 of which (indices 57..71, across the 64-template block
    boundary) equal the base query shifted by o = -7..7 rows except for 3 added to
    o+8 bytes of row 8+o: offset o is their strict best, scoring 3 (o + 8)."""
    rng = np.random.default_rng(100 + h)
    q = rng.integers(0, 256, (h, 32), dtype=np.uint8)
    lib = rng.integers(0, 256, (72, h, 32), dtype=np.uint8)
    for o in range(-M + 1, M):
        t = lib[57 + o + M - 1]
        t[M + o:h - M + o] = q[M:h - M]
        t[M + o, :o + M] += 3
    queries = np.concatenate([q[None], rng.integers(0, 256, (4, h, 32), dtype=np.uint8)])
    ref = np.stack([V.vt_scores_library(lib, x) for x in queries])
    ref.setflags(write=False)
    return lib, queries, ref


@pytest.mark.parametrize('nqc', ['1', '8'])
@pytest.mark.parametrize('h', [64, 32])
def test_every_offset_is_the_unique_best_somewhere(vtmod, monkeypatch, h, nqc):
    monkeypatch.setenv('RS_VT_NQC', nqc)
    lib_np, queries, ref = _offset_case(h)
    # the case is what it claims: template 57 + o + 7 scores 3 (o + 8) at offset o alone
    for o in range(-M + 1, M):
        t = lib_np[57 + o + M - 1]
        per = [int((t[M + p:h - M + p] - queries[0][M:h - M]).sum(dtype=np.uint64)) for p in range(-M + 1, M)]
        assert per[o + M - 1] == 3 * (o + M) == ref[0, 57 + o + M - 1]
        assert min(s for p, s in enumerate(per) if p != o + M - 1) > 50000
    lib = vtmod.ViewTemplates._from_shape((h, 32), 45000)
    lib.add(lib_np)
    assert np.array_equal(lib.scores(queries), ref)      # one full batch of 4 and a ragged one of 1
    idx, score, new = lib.match_templates(queries, mode=0)
    assert not new.any()
    assert np.array_equal(score, ref.min(axis=1))
    assert np.array_equal(idx, ref.argmin(axis=1))
    assert idx[0] == 57 and score[0] == 3


@pytest.mark.parametrize('h', [64, 32])
def test_saturated_counts_do_not_carry(vtmod, h):
    """All 0 against all 255: every byte pair of every unit borrows, the largest
    count each packed u16 half can reach; and the reverse pair, which never does."""
    rng = np.random.default_rng(200 + h)
    lib_np = rng.integers(0, 256, (7, h, 32), dtype=np.uint8)
    lib_np[2] = 0
    lib_np[4] = 255
    queries = rng.integers(0, 256, (6, h, 32), dtype=np.uint8)
    queries[1] = 255
    queries[3] = 0
    ref = np.stack([V.vt_scores_library(lib_np, x) for x in queries])
    n = (h - 2 * M) * 32
    assert ref[1, 2] == n == {64: 1536, 32: 512}[h]
    assert ref[3, 4] == 255 * n == {64: 391680, 32: 130560}[h]
    lib = vtmod.ViewTemplates._from_shape((h, 32), 45000)
    lib.add(lib_np)
    assert np.array_equal(lib.scores(queries), ref)
    idx, score, _ = lib.match_templates(queries, mode=0)
    assert np.array_equal(score, ref.min(axis=1))
    assert np.array_equal(idx, ref.argmin(axis=1))


@pytest.mark.parametrize('h', [64, 32])
def test_sequential_shifted_queries(vtmod, h):
    """The in-batch (matrix) scan: each query is the one before it rolled by +-7 or
    +-4 rows minus a little noise, so it meets the earlier ones at offsets
    +-7, +-4 and 0 or, beyond the offset range, becomes a template itself."""
    rng = np.random.default_rng(300 + h)
    thr = 20 * (h - 2 * M) * 32     # accumulated noise stays below it (<= 15 a byte), strangers far above
    qs = [rng.integers(0, 256, (h, 32), dtype=np.uint8)]
    for shift in (7, 4, -7, -4, 7):
        prev = np.roll(qs[-1], shift, axis=0).astype(np.int16)
        qs.append(np.clip(prev - rng.integers(0, 4, (h, 32)), 0, 255).astype(np.uint8))
    qs = np.stack(qs)
    ref = V.ViewTemplatesOracle((0, 128), (0, 64), 2, 2, 8, 8, thr)
    ref.shape = (h, 32)
    expect = [ref.match_template(x) for x in qs]
    assert 1 < sum(e[1] for e in expect) < len(qs)    # some become templates, some match
    lib = vtmod.ViewTemplates._from_shape((h, 32), thr)
    idx, score, new = lib.match_templates(qs)
    assert np.array_equal(idx, [e[0] for e in expect])
    assert np.array_equal(new, [e[1] for e in expect])
    assert np.array_equal(score, [np.iinfo(np.uint64).max if e[2] is None else e[2] for e in expect])
