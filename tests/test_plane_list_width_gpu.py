"""The list passes' entries per batch (vt_plan::list_width; PlaneList::nb, fill): a thread block
of vt_scan_plane_kernel<64, false, true> walks its list in batches of 4, 2 or 1 entries, chosen
on the device from the list's length, or forced by RS_VT_LIST_NB = 1, 2 or 4; and the fused
front's tail, which a wave without a query now skips.

RS_VT_PRUNE=force.  Index and score against the oracle and against the keys of RS_VT_PRUNE=0,
bit for bit; prune_stats() / prune_verified() against the NumPy rule after every call, so they
are the same at every width.

130 templates (blocks of 64, 64 and 2), at each forced width and by the rule: all-miss batches
of 1, 2, 3, 4, 5, 7, 8, 9, 37 and 300 queries (list lengths around every multiple of each width);
the same sizes with hits and 1, 2, 3 or 5 queries on list 1 of block 0 and 0 or 3 on list 1 of
block 1 (twins inside the block), block 2's lists empty; long and short lists in turn on one
handle with a matrix scan (a dense launch on the same counters) and a one-query call between;
match_stream from device memory.  The library, the queries and their references are those of
test_plane_list_prologue_gpu, computed once.

1,030 templates (17 blocks), by the rule: all-miss batches of 300 and 512 queries -- on a device
of 512 resident thread blocks the rule takes 2 and 4 for pass B2 there, and 1 for pass B1.  The
test asserts results and statistics, not the width, so it holds on any device.

The fused front (130 templates, by vt_plan::front_fused) with 1, 2, 3, 5, 6 and 7 queries: groups
whose last waves have no query, settled and unsettled queries side by side."""
import functools

import numpy as np
import pytest

from test_plane_list_prologue_gpu import check, misses, mixed, pool, twin_library
from test_plane_ondemand_gpu import THR, Case, forced, frozen
from oracle import view_templates as V

pytestmark = pytest.mark.gpu

WIDTHS = [pytest.param('1', id='nb1'), pytest.param('2', id='nb2'), pytest.param('4', id='nb4'),
          pytest.param(None, id='rule')]
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 37, 300]
ALTERNATING = [300, 1, 37, 2, 9, 3, 8, 4, 7, 5]          # long and short lists in turn
TWINS = [(k0, k1) for k1 in (0, 3) for k0 in (1, 2, 3, 5)]   # queries on list 1 of block 0, of block 1


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


def set_width(monkeypatch, width):
    if width is None:
        monkeypatch.delenv('RS_VT_LIST_NB', raising=False)
    else:
        monkeypatch.setenv('RS_VT_LIST_NB', width)
    monkeypatch.delenv('RS_VT_FRONT', raising=False)


@pytest.fixture
def dense(vtmod, monkeypatch):
    monkeypatch.setenv('RS_VT_PRUNE', '0')
    d = vtmod.ViewTemplates._from_shape((64, 32), THR)
    d.add(twin_library())
    yield d
    d.close()


@pytest.fixture(params=WIDTHS)
def handle(request, vtmod, monkeypatch, dense):
    set_width(monkeypatch, request.param)
    h = forced(vtmod, monkeypatch, twin_library())
    yield h
    h.close()


def checked_twice(h, c, dense=None):
    for _ in range(2):
        want = check(h, c, dense)
        assert (h.prune_stats(), h.prune_verified()) == want
        assert (h.prune_stats(), h.prune_verified()) == want


def test_the_override_takes_1_2_or_4_only(vtmod, monkeypatch):
    monkeypatch.setenv('RS_VT_PRUNE', 'force')
    for bad in ('3', '0', '8', '44', 'x'):
        monkeypatch.setenv('RS_VT_LIST_NB', bad)
        with pytest.raises(Exception):
            vtmod.ViewTemplates._from_shape((64, 32), THR)


@pytest.mark.parametrize('nq', SIZES)
def test_all_miss_batches(handle, dense, nq):
    checked_twice(handle, misses(nq), dense)


@pytest.mark.parametrize('nq', SIZES)
def test_hits_with_chosen_list_lengths_and_empty_lists(handle, dense, nq):
    for k0, k1 in TWINS:
        c = mixed(nq, k0, k1)
        assert (c.pairs == 0).all() and (c.idx[~c.ver] < 128).all()   # list 2 empty, list 1 of block 2 too
        checked_twice(handle, c, dense)


def test_long_and_short_lists_in_turn_on_one_handle(handle, dense):
    for rnd, (k0, k1) in enumerate([(0, 0), (5, 3), (2, 0)]):
        for i, nq in enumerate(ALTERNATING):
            c = misses(nq) if rnd == 0 else mixed(nq, k0, k1)
            want = check(handle, c, dense if rnd < 2 else None)
            assert (handle.prune_stats(), handle.prune_verified()) == want
            if i % 3 == 0:     # a dense (matrix) launch on the same counters
                k = min(nq, 5)
                got = handle.scores(c.queries[:k], t0=66, nt=7)
                assert np.array_equal(got, c.scores[:k, 66:73].astype(np.uint64))
            if i % 4 == 1:
                one = mixed(1, 1, 0) if rnd else misses(1)
                assert check(handle, one) == (handle.prune_stats(), handle.prune_verified())


def test_match_stream_from_device_memory_equals_the_per_batch_calls(handle):
    from pyratslam_amd import _lib
    cs = [mixed(37, 5, 3), misses(37), mixed(37, 1, 0)]
    q = np.ascontiguousarray(np.stack([c.queries for c in cs]))
    per = [handle.match_templates(c.queries, mode=0)[:2] for c in cs]
    buf = _lib.DeviceBuffer(q.nbytes).upload(q)
    idx, score = handle.match_stream((3, 37, buf))[:2]
    buf.close()
    for b, c in enumerate(cs):
        assert np.array_equal(idx[b], per[b][0]) and np.array_equal(score[b], per[b][1])
        assert np.array_equal(idx[b], c.idx) and np.array_equal(score[b], c.best)
    ver = np.concatenate([c.ver for c in cs])
    pairs = np.concatenate([c.pairs for c in cs])
    assert (handle.prune_stats(), handle.prune_verified()) == ((111, int(pairs.sum()), 3 * 111, 2), int(ver.sum()))


def test_every_width_gives_the_same_keys_and_statistics(vtmod, monkeypatch):
    p = pool()
    cases = [misses(37), mixed(37, 5, 3), mixed(300, 3, 3), misses(9)]
    got = []
    for width in ('1', '2', '4', None):
        set_width(monkeypatch, width)
        h = forced(vtmod, monkeypatch, p.lib)
        row = []
        for c in cases:
            idx, score, _ = h.match_templates(c.queries, mode=0)
            row.append((idx, score, np.array(h.prune_stats()), np.array(h.prune_verified())))
        got.append(row)
        h.close()
    for row in got[1:]:
        for a, b in zip(got[0], row):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


# --- 1,030 templates: the rule's own choice (on 512 resident thread blocks: 2 at 300 queries,
# 4 at 512 for pass B2; 1 for pass B1's lists of about 18 and 30)
NDISTINCT = 128


@functools.lru_cache(maxsize=None)
def wide_case():
    """17 template blocks and 128 distinct all-miss queries (a batch draws them again and again:
    the lists' lengths are those of as many distinct ones)."""
    lib = V.synthetic_library(1030, 64, 32, seed=371)
    q = np.random.default_rng(372).integers(0, 256, size=(NDISTINCT, 64, 32), dtype=np.uint8)
    c = Case(lib, q)
    assert not c.ver.any() and (c.pairs == c.ntb - 1).all() and c.ntb == 17
    return c


@pytest.mark.parametrize('nq', [300, 512])
def test_all_miss_batches_by_the_rule_at_17_template_blocks(vtmod, monkeypatch, nq):
    w = wide_case()
    sel = np.random.default_rng(nq).permutation(np.resize(np.arange(NDISTINCT), nq))
    set_width(monkeypatch, None)
    h = forced(vtmod, monkeypatch, w.lib)
    for _ in range(2):
        idx, score, new = h.match_templates(frozen(w.queries[sel]), mode=0)
        assert not new.any()
        assert np.array_equal(score, w.best[sel]) and np.array_equal(idx, w.idx[sel])
        for _ in range(2):
            assert h.prune_stats() == (nq, 16 * nq, 17 * nq, 2) and h.prune_verified() == 0
    h.close()


# --- the fused front: groups of four queries, a wave per query in the tail
@pytest.mark.parametrize('nq', [1, 2, 3, 5, 6, 7])
def test_front_groups_whose_last_waves_have_no_query(vtmod, monkeypatch, dense, nq):
    set_width(monkeypatch, None)
    h = forced(vtmod, monkeypatch, twin_library())
    for c in (mixed(nq, 0, 0), mixed(nq, 1, 1 if nq >= 3 else 0), misses(nq), mixed(nq, min(nq, 3), 0)):
        checked_twice(h, c, dense)
    h.close()
