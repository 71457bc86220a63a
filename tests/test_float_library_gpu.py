"""Device-resident float view-template library (rs_vtf): scores, first argmin,
growth and the ViewTemplates.match / match_batch traces, all bit for bit against
the reference's golden vectors and the oracle's vt_score on float arrays."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from oracle import view_templates as V

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ROS = ((32, 96), (32, 96), 2, 2, 256, 256)


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


def frame(mask, template):
    """A whole frame whose masked pixels carry ``template`` (in its dtype)."""
    im = np.zeros(mask.shape, dtype=template.dtype)
    im[mask] = template.ravel()
    return im


def ref_matrix(templates, queries):
    """(nq, nt) scores by the oracle's ViewTemplate.match, in the arrays' dtype."""
    out = np.empty((len(queries), len(templates)), dtype=templates.dtype)
    for i, q in enumerate(queries):
        for j, t in enumerate(templates):
            out[i, j] = V.vt_score(t, q)
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# -- reference-made pairs -------------------------------------------------------
@pytest.mark.parametrize('tag', ['f64', 'f32'])
@pytest.mark.parametrize('i', [0, 1, 2])
def test_reference_pairs(vtmod, tag, i):
    d = load_golden('vt_pairs_float')
    a, b, s = d[f'{tag}_{i}_a'], d[f'{tag}_{i}_b'], d[f'{tag}_{i}_score']
    lib = vtmod.ViewTemplates._from_shape(a.shape[1:], 45000)
    lib.add(a)
    assert lib.scan_form() == 'sad-resident' and lib.count() == len(lib.templates) == 16
    sc = lib.scores(b)                         # (query, template)
    assert sc.dtype == s.dtype
    assert same_bits(np.diagonal(sc).copy(), s)
    assert same_bits(sc, vtmod.sad_scores(a, b))
    assert same_bits(lib.scores(b[2:5], 3, 6), sc[2:5, 3:9])


# -- shapes: n = 3 (a leaf shorter than 8), 140 (leaves 64 + 76), 792 (96 / 104); and
# (24, 800), n = 6400, whose template does not fit the scan's LDS tile in either dtype
# (the general instance, reading global memory in place)
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', [(17, 3), (23, 20), (40, 33), (24, 800)])
def test_shapes_vs_oracle(vtmod, shape, dt):
    rng = np.random.default_rng(shape[0])
    a = (rng.random((5,) + shape) * 255).astype(dt)
    b = (rng.random((3,) + shape) * 255).astype(dt)
    b[1] = (np.roll(a[2], 3, axis=0) + rng.normal(0, 3, shape)).astype(dt)
    lib = vtmod.ViewTemplates._from_shape(shape, 45000)
    lib.add(a)
    assert same_bits(lib.scores(b), ref_matrix(a, b))


@pytest.mark.parametrize('dt', DTYPES)
def test_window_longer_than_numpys_reduction_buffer(vtmod, dt):
    """(18, 4200) at max_offset 8: a window of 2 x 4,200 = 8,400 elements, above the 8,192
    that np.sum hands its pairwise loop at a time, so numpy's sum is the first 8,192
    elements' pairwise sum plus the remaining 208's.  The template does not fit the scan's
    LDS tile: the general instance.  Both the pair-wise call and the resident library
    follow the one chunked plan.  Before rs_sad_scores took that plan its own unchunked
    pairwise order failed the first assertion (a CPU emulation of both orders on these
    inputs: a different minimum from np.sum's in 3 of 4 pairs, in float32 and in float64);
    the second assertion held then too.  The resident library is an rs_vtf handle through
    the ABI: a ViewTemplates also holds a uint8 handle, which takes no width above 4,096."""
    from pyratslam_amd import _lib
    rng = np.random.default_rng(0)
    a = (rng.random((2, 18, 4200)) * 255).astype(dt)
    b = (rng.random((2, 18, 4200)) * 255).astype(dt)
    ref = ref_matrix(a, b)
    assert same_bits(vtmod.sad_scores(a, b), ref)
    lib, h = _lib.require_device(), ctypes.c_void_p()
    code = _lib.RS_DT_F32 if dt is np.float32 else _lib.RS_DT_F64
    _lib.check(lib.rs_vtf_create(18, 4200, vtmod.MAX_OFFSET, code, 2, 0, ctypes.byref(h)))
    try:
        _lib.check(lib.rs_vtf_add(h, 2, ctypes.c_void_p(a.ctypes.data), None))
        sc = np.empty((2, 2), dtype=dt)
        _lib.check(lib.rs_vtf_scores(h, 2, ctypes.c_void_p(b.ctypes.data), 0, 2, ctypes.c_void_p(sc.ctypes.data)))
    finally:
        _lib.check(lib.rs_vtf_destroy(h))
    assert same_bits(sc, ref)


# -- library sizes x batch sizes ---------------------------------------------------
@pytest.fixture(scope='module', params=DTYPES, ids=['f32', 'f64'])
def scan_case(request):
    """130 templates and 70 queries of 24 x 20 with the full oracle score matrix:
    templates 3 and 7 equal, template 5 all inf, query 2 a copy of template 3,
    query 4 all NaN, query 0 a shifted noisy template 9."""
    dt = request.param
    rng = np.random.default_rng(21)
    t = rng.random((130, 24, 20)).astype(dt)
    q = rng.random((70, 24, 20)).astype(dt)
    t[7] = t[3]
    t[5] = np.inf
    q[0] = (np.roll(t[9], -2, axis=0) + rng.normal(0, 0.01, (24, 20))).astype(dt)
    q[2] = t[3]
    q[4] = np.nan
    for k in range(6, 70, 3):                  # near copies of templates all over the library
        q[k] = (t[(k * 37) % 130] + rng.normal(0, 0.02, (24, 20))).astype(dt)
    ref = ref_matrix(t, q)
    ref.setflags(write=False)
    return t, q, ref


@pytest.mark.parametrize('nt', [0, 1, 63, 64, 65, 130])
def test_frozen_scan_sizes(vtmod, scan_case, nt):
    from pyratslam_amd import _lib
    t, q, ref = scan_case
    lib = vtmod.ViewTemplates._from_shape(t.shape[1:], 45000, capacity=8)
    if nt:
        lib.add(t[:nt])
    for nq in (1, 5, 70):
        idx, score, new = lib.match_templates(q[:nq], mode=_lib.RS_VT_FROZEN)
        assert score.dtype == t.dtype and not new.any()
        if nt == 0:
            assert np.isposinf(score).all() and (idx == -1).all()
            continue
        r = ref[:nq, :nt]
        assert same_bits(score, r.min(axis=1))
        assert np.array_equal(idx, np.argmin(r, axis=1))
        assert not np.isnan(score).any()
        if nq >= 5:
            assert np.isposinf(score[4]) and idx[4] == 0          # the all-NaN query
            if nt >= 8:
                assert score[2] == 0 and idx[2] == 3              # duplicates at 3 and 7
    assert lib.count() == nt and len(lib.templates) == nt
    if nt >= 8:
        sc = lib.scores(q[:5])
        assert same_bits(sc, ref[:5, :nt]) and np.isposinf(sc[:, 5]).all()   # the all-inf template


# -- growth ----------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_growth_keeps_every_template(vtmod, dt):
    from pyratslam_amd import _lib
    data = np.random.default_rng(3).random((49, 32, 32)).astype(dt)
    lib = vtmod.ViewTemplates._from_shape((32, 32), 45000, capacity=4)
    assert lib.add(data[:9]) == 0
    assert lib.add(data[9:]) == 9
    assert lib.count() == 49
    out = np.empty((32, 32), dtype=dt)
    for i in range(49):
        _lib.check(lib._lib.rs_vtf_read(lib._vtf, i, ctypes.c_void_p(out.ctypes.data)))
        assert same_bits(out, data[i]), i
    idx, score, _ = lib.match_templates(data, mode=_lib.RS_VT_FROZEN)
    assert np.array_equal(idx, np.arange(49)) and (score == 0).all()
    with pytest.raises(ValueError):
        _lib.check(lib._lib.rs_vtf_read(lib._vtf, 49, ctypes.c_void_p(out.ctypes.data)))


# -- the reference's float trace ---------------------------------------------------
def _pc(k):
    return (k % 21, (3 * k) % 21, (5 * k) % 36)


def _run_trace(vts, frames, batch):
    """Indices of matching ``frames`` through match() (batch None) or match_batch()."""
    if batch is None:
        return [vts.match(f, *_pc(k)).get_index() for k, f in enumerate(frames)]
    idx = []
    for lo in range(0, len(frames), batch):
        ks = range(lo, min(lo + batch, len(frames)))
        idx += [t.get_index() for t in vts.match_batch([frames[k] for k in ks], [_pc(k) for k in ks])]
    return idx


@pytest.mark.parametrize('batch', [None, 60, 7], ids=['match', 'batch60', 'batch7'])
def test_reference_trace(vtmod, batch):
    d = load_golden('vt_pairs_float')
    vts = vtmod.ViewTemplates(*ROS, float(d['trace_threshold']))
    frames = [frame(vts.mask, q) for q in d['trace_queries']]
    idx = _run_trace(vts, frames, batch)
    assert np.array_equal(idx, d['trace_index'])
    assert same_bits(np.stack([t.template for t in vts.templates]), d['trace_templates'])
    assert vts.scan_form() == 'sad-resident'
    assert vts.count() == len(vts.templates)
    new = sorted(set(idx), key=idx.index)
    assert [vts.templates[g].location() for g in new] == [_pc(idx.index(g)) for g in new]
    # the device library holds the same bytes as the Python list
    assert (np.diagonal(vts.scores(d['trace_templates'])) == 0).all()


def _rule_loop(queries, thresholds):
    """The reference's rule (view_templates.py:63-75) as a plain loop over vt_score;
    thresholds[k] is match_threshold when query k arrives."""
    templates, idx = [], []
    for q, thr in zip(queries, thresholds):
        match_val = [V.vt_score(t, q) for t in templates]
        if len(match_val) == 0 or min(match_val) > thr:
            templates.append(q)
            idx.append(len(templates) - 1)
        else:
            idx.append(int(np.argmin(match_val)))
    return idx, templates


@pytest.fixture(scope='module')
def f32_trace():
    d = load_golden('vt_pairs_float')
    q = d['trace_queries'].astype(np.float32)
    thr = float(d['trace_threshold'])
    idx, templates = _rule_loop(q, [thr] * len(q))
    return q, thr, idx, np.stack(templates)


@pytest.mark.parametrize('batch', [None, 60, 7], ids=['match', 'batch60', 'batch7'])
def test_float32_sequential_trace(vtmod, f32_trace, batch):
    q, thr, want, templates = f32_trace
    vts = vtmod.ViewTemplates(*ROS, thr)
    idx = _run_trace(vts, [frame(vts.mask, x) for x in q], batch)
    assert idx == want
    assert same_bits(np.stack([t.template for t in vts.templates]), templates)
    assert vts.scan_form() == 'sad-resident' and vts.count() == len(templates)


@pytest.mark.parametrize('batch', [None, 7], ids=['match', 'batch7'])
def test_threshold_changed_mid_trace(vtmod, batch):
    """match_threshold is read at every call: a change is honoured from the next call on."""
    d = load_golden('vt_pairs_float')
    q, thr = d['trace_queries'], float(d['trace_threshold'])
    # calls [0, 21) at the fixture's threshold, [21, 42) never match (negative), then always
    thrs = [thr] * 21 + [-1.0] * 21 + [np.inf] * 18
    want, templates = _rule_loop(q, thrs)
    assert len(templates) > len(set(d['trace_index']))           # the change shows in the trace
    vts = vtmod.ViewTemplates(*ROS, thr)
    frames = [frame(vts.mask, x) for x in q]
    idx = []
    for lo in range(0, 60, 21):                                   # 21 is a multiple of the batch
        vts.match_threshold = thrs[lo]
        part = frames[lo:lo + 21]
        if batch is None:
            idx += [vts.match(f, *_pc(lo + k)).get_index() for k, f in enumerate(part)]
        else:
            for b in range(0, len(part), batch):
                idx += [t.get_index() for t in vts.match_batch(part[b:b + batch],
                                                               [_pc(0)] * len(part[b:b + batch]))]
    assert idx == want
    assert same_bits(np.stack([t.template for t in vts.templates]), np.stack(templates))
    assert vts.scan_form() == 'sad-resident' and vts.count() == len(templates)


# -- what falls back, what refuses ---------------------------------------------------
def test_uint8_arguments_refused_after_a_float_frame(vtmod):
    d = load_golden('vt_pairs_float')
    vts = vtmod.ViewTemplates(*ROS, float(d['trace_threshold']))
    vts.match(frame(vts.mask, d['trace_queries'][0]), 0, 0, 0)
    assert vts.scan_form() == 'sad-resident'
    u8 = np.zeros((1,) + vts.shape, dtype=np.uint8)
    f32 = np.zeros((1,) + vts.shape, dtype=np.float32)
    for call in (lambda: vts.add(u8), lambda: vts.scores(u8), lambda: vts.match_templates(u8),
                 lambda: vts.match_stream(u8[None]),
                 lambda: vts.match_frames(np.zeros((1, 256, 256), np.uint8), None),
                 lambda: vts.add(f32), lambda: vts.scores(f32), lambda: vts.match_templates(f32)):
        with pytest.raises(TypeError, match='float frames'):
            call()
    assert vts.count() == len(vts.templates) == 1


def _mixed_state(vtmod, thr):
    """A ViewTemplates held in the mixed state from the start: every match goes through
    the pair-wise path over the Python template list, as before float libraries."""
    vts = vtmod.ViewTemplates(*ROS, thr)
    vts._float = True
    return vts


def test_float_frame_at_a_uint8_library_falls_back(vtmod):
    d = load_golden('vt_pairs_float')
    q, thr = d['trace_queries'], 45000.0
    seq = [np.floor(x * 255).astype(np.uint8) for x in q[:12]] + [x * 255 for x in q[12:40]]
    a, b = vtmod.ViewTemplates(*ROS, thr), _mixed_state(vtmod, thr)
    ia = [a.match(frame(a.mask, x), 0, 0, 0).get_index() for x in seq]
    ib = [b.match(frame(b.mask, x), 0, 0, 0).get_index() for x in seq]
    assert ia == ib and len(set(ia)) > 1
    assert a.scan_form() != 'sad-resident' and a._float


def test_other_float_dtype_falls_back(vtmod):
    d = load_golden('vt_pairs_float')
    q, thr = d['trace_queries'], float(d['trace_threshold'])
    seq = list(q[:25]) + [q[3].astype(np.float32)] + list(q[25:45]) + [q[30].astype(np.float32)]
    a, b = vtmod.ViewTemplates(*ROS, thr), _mixed_state(vtmod, thr)
    ia = [a.match(frame(a.mask, x), 0, 0, 0).get_index() for x in seq[:25]]
    assert a.scan_form() == 'sad-resident'
    ia += [a.match(frame(a.mask, x), 0, 0, 0).get_index() for x in seq[25:]]
    ib = [b.match(frame(b.mask, x), 0, 0, 0).get_index() for x in seq]
    assert ia == ib
    assert a.scan_form() != 'sad-resident' and a._float
    assert [t.template.dtype for t in a.templates] == [t.template.dtype for t in b.templates]
    # and the reverse: a float64 frame arriving at a float32 library
    a, b = vtmod.ViewTemplates(*ROS, thr), _mixed_state(vtmod, thr)
    seq = [x.astype(np.float32) for x in q[:10]] + list(q[10:20])
    ia = [a.match(frame(a.mask, x), 0, 0, 0).get_index() for x in seq]
    ib = [b.match(frame(b.mask, x), 0, 0, 0).get_index() for x in seq]
    assert ia == ib and a._float
