"""The true-SAD metric of the uint8 view-template library on the GPU (csrc/vt_sad.h:
vt_qform_sad_kernel, vt_scan_sad_kernel, vt_scan_sad_generic_kernel; metric='sad').
Integer work with no tolerance: scores, first-argmin indices, is_new and the stored
templates equal the NumPy restatement (numpy_sad_u8_scores; tests/test_vt_sad.py pins it
to the reference's formula on float casts).  The shapes and call paths mirror
tests/test_byte_scans_gpu.py, with two-sided noise throughout."""
import concurrent.futures
import ctypes
import functools

import numpy as np
import pytest

from oracle import view_templates as V

pytestmark = pytest.mark.gpu

U64_MAX = np.iinfo(np.uint64).max


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


def form_of(shape):
    return 'sad' if shape[0] in (32, 64) else 'sad-generic'


def new_handle(vtmod, shape, thr):
    lib = vtmod.ViewTemplates._from_shape(shape, thr, metric='sad')
    assert lib.metric == 'sad' and lib.scan_form() == form_of(shape)
    return lib


def pixel_threshold(shape):
    """The shipped 45000 of a 48 x 32 window (64 x 32 templates), kept per pixel."""
    return 29 * (shape[0] - 16) * shape[1]


def sad_matrix(library, queries):
    """(nq, nt) restatement scores; the queries go over a few threads (NumPy releases the GIL)."""
    from pyratslam_amd.view_templates import numpy_sad_u8_scores
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        return np.stack(list(pool.map(lambda q: numpy_sad_u8_scores(library, q), queries)))


class SadOracle:
    """ViewTemplates.match (view_templates.py:63-75) on the restatement: linear scan, strict
    threshold, first argmin, append on a miss.  Returns (index, is_new, best or None)."""

    def __init__(self, thr, templates=(), mask=None, shape=None):
        self.match_threshold, self.mask, self.shape = thr, mask, shape
        self.templates = [np.array(t) for t in templates]
        self.locations = [(0, 0, 0)] * len(self.templates)

    def match_template(self, template, pc=(0, 0, 0)):
        from pyratslam_amd.view_templates import numpy_sad_u8_scores
        best = None
        if self.templates:
            scores = numpy_sad_u8_scores(np.stack(self.templates), template)
            best = int(scores.min())
            if not best > self.match_threshold:
                return int(np.argmin(scores)), False, best
        self.templates.append(np.array(template))
        self.locations.append(tuple(pc))
        return len(self.templates) - 1, True, best

    def match(self, image, *pc):
        return self.match_template(np.asarray(image)[self.mask].reshape(self.shape), pc)


def two_sided_queries(library, q, seed, noise=3):
    """Nine in ten a stored template rolled by -7..7 rows plus noise in -noise..noise, clipped
    to a byte (both signs: such a pixel wraps to about 255 under the wrapped metric); the
    rest fresh images."""
    rng = np.random.default_rng(seed)
    t, h, w = library.shape
    out = np.empty((q, h, w), np.uint8)
    for i in range(q):
        if t and rng.random() < 0.9:
            b = np.roll(library[int(rng.integers(0, t))], int(rng.integers(-7, 8)), axis=0)
            out[i] = np.clip(b.astype(np.int64) + rng.integers(-noise, noise + 1, (h, w)), 0, 255)
        else:
            out[i] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return out


# --- a. frozen scan and full score matrix ------------------------------------
# fast form: ntb = ceil(t / 64) template blocks, min(WD, 8) waves per block, WD = ceil(W / 4)
# dword columns dealt over them, query groups of 4 (the tail clamped)
FROZEN_CASES = [
    (140, 37, 64, 32),    # three blocks, the last of 12 slots; odd q: a group of one query
    (70, 9, 32, 32),      # the ROS shape
    (140, 37, 64, 48),    # WD = 12 > 8 waves: waves 0-3 take a second column per group
    (200, 33, 32, 30),    # W % 4 = 2: padding bytes in the last dword of every row
    (70, 9, 64, 3),       # WD = 1: one wave per block, W < 4
    (90, 21, 40, 32),     # generic, although W = 32
    (65, 6, 18, 8),       # generic, two-row window; one template in the second block
    (64, 5, 16, 32),      # generic, H = 2 * max_offset: the window is empty, every score 0
    (1000, 256, 64, 32),  # 16 template blocks x 64 query groups: several rounds of blocks
]


@pytest.mark.parametrize('t,q,h,w', FROZEN_CASES)
def test_frozen_scan_and_score_matrix(vtmod, t, q, h, w):
    rng = np.random.default_rng(1000 * h + w)
    lib_np = V.synthetic_library(t, h, w, seed=t)
    lib_np[5] = 0
    lib_np[6] = 255
    lib_np[7] = np.where(rng.random((h, w)) < 0.5, 0, 255)
    queries = two_sided_queries(lib_np, q, seed=q)
    queries[0] = 255
    queries[1] = 0
    ref = sad_matrix(lib_np, queries)
    assert ref[0, 5] == ref[1, 6] == (h - 16) * w * 255 and ref[0, 6] == ref[1, 5] == 0
    lib = new_handle(vtmod, (h, w), 45000)
    lib.add(lib_np)
    idx, score, new = lib.match_templates(queries, mode=0)
    assert not new.any()
    assert np.array_equal(score, ref.min(axis=1))
    assert np.array_equal(idx, ref.argmin(axis=1))
    assert np.array_equal(lib.scores(queries), ref)
    if t >= 73:     # a template range inside the second block: the scan starts at block 1
        assert np.array_equal(lib.scores(queries[:5], t0=70, nt=3), ref[:5, 70:73])
    if h == 2 * V.MAX_OFFSET:
        assert not ref.any() and not idx.any()
    assert lib.count() == t
    lib.close()


@pytest.mark.parametrize('shape', [(64, 32), (32, 30), (40, 32)])
def test_ties_pick_first_index(vtmod, shape):
    """70 templates stored twice: every query's minimum is tied between slot g of the first
    block and slot g + 70 of the second or third; the packed keys' atomic minimum keeps the
    lower index."""
    t = V.synthetic_library(70, *shape, seed=2)
    lib = new_handle(vtmod, shape, 10 ** 9)
    lib.add(np.concatenate([t, t]))
    idx, score, _ = lib.match_templates(t[::3], mode=0)
    assert np.array_equal(idx, np.arange(0, 70, 3)) and (score == 0).all()
    lib.close()


# --- b. sequential in-batch semantics ----------------------------------------
@functools.lru_cache(maxsize=None)
def sequence_case(shape, nbase=40, n=300):
    """Base templates and a query sequence that appends, hits base templates, and hits
    templates appended earlier: 50% a base template rolled by -7..7 plus noise in -2..2,
    15% the same with noise in -59..59 (mean |noise| 29.7 a pixel, next to the threshold
    of 29), 17% a fresh image, 18% a copy of one of the previous 40 queries with noise in
    -2..2 again: two-sided noise on a noisy copy, which the wrapped metric cannot match."""
    h, w = shape
    base = V.synthetic_library(nbase, h, w, seed=8)
    rng = np.random.default_rng(9)
    qs = np.empty((n, h, w), np.uint8)
    for i in range(n):
        u = rng.random() if i else 0.0
        if u < 0.65:
            b = np.roll(base[int(rng.integers(0, nbase))], int(rng.integers(-7, 8)), axis=0)
            k = 2 if u < 0.5 else 59
            qs[i] = np.clip(b.astype(np.int64) + rng.integers(-k, k + 1, (h, w)), 0, 255)
        elif u < 0.82:
            qs[i] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        else:
            b = qs[int(rng.integers(max(0, i - 40), i))]
            qs[i] = np.clip(b.astype(np.int64) + rng.integers(-2, 3, (h, w)), 0, 255)
    qs.setflags(write=False)
    base.setflags(write=False)
    return base, qs


def trace_counts(trace, nbase, batch):
    """(new, hits on base templates, hits on a template appended earlier in the same
    batch, hits on one appended in an earlier batch) of an oracle trace."""
    born = {}
    new = on_base = same = earlier = 0
    for i, (idx, is_new, _) in enumerate(trace):
        if is_new:
            born[idx] = i
            new += 1
        elif idx < nbase:
            on_base += 1
        elif born[idx] // batch == i // batch:
            same += 1
        else:
            earlier += 1
    return new, on_base, same, earlier


@functools.lru_cache(maxsize=None)
def sequence_trace(shape):
    base, qs = sequence_case(shape)
    ref = SadOracle(pixel_threshold(shape), base)
    trace = [ref.match_template(q) for q in qs]
    return trace, np.stack(ref.templates)


@pytest.mark.parametrize('shape', [(64, 32), (32, 30), (40, 32)])
def test_sequential_batches_equal_oracle_sequence(vtmod, shape):
    """ViewTemplates.match semantics inside and across batches of 64: the candidate buffer
    and its score matrix (MATRIX instances), appends through the padded store, later
    queries preferring a template of their own batch."""
    base, qs = sequence_case(shape)
    trace, stored = sequence_trace(shape)
    counts = trace_counts(trace, len(base), 64)
    print('new / base hits / same-batch hits / earlier-batch hits:', counts)
    assert min(counts) >= 1, counts
    lib = new_handle(vtmod, shape, pixel_threshold(shape))
    lib.add(base)
    got = [lib.match_templates(qs[i:i + 64]) for i in range(0, len(qs), 64)]
    idx, score, new = (np.concatenate([g[k] for g in got]) for k in range(3))
    assert np.array_equal(idx, [t[0] for t in trace])
    assert np.array_equal(new, [t[1] for t in trace])
    assert all(t[2] is not None for t in trace)      # the base templates are always there
    assert np.array_equal(score, np.array([t[2] for t in trace], dtype=np.uint64))
    assert np.array_equal(np.stack([t.template for t in lib.templates]), stored)
    assert lib.count() == len(stored)
    lib.close()


# --- c. simulated shards -------------------------------------------------------
def test_sharded_ranks_simulated_on_one_gpu(vtmod):
    """Three handles on one GPU, each owning templates g % 3 == rank, at (32, 30); the
    elementwise min over their local keys plays the RCCL allreduce(min)."""
    from pyratslam_amd import _lib
    shape, nranks = (32, 30), 3
    thr = pixel_threshold(shape)
    base, queries = sequence_case(shape)
    queries = queries[:200]
    shards = [vtmod.ShardedViewTemplates.from_shape(shape, thr, r, nranks, reducer=lambda k: k, metric='sad')
              for r in range(nranks)]
    single = new_handle(vtmod, shape, thr)
    for s in shards:
        assert s.scan_form() == 'sad' and s.metric == 'sad'
        s.add(base)
    single.add(base)
    ref = SadOracle(thr, base)
    trace = []
    for lo in range(0, 200, 50):
        batch = queries[lo:lo + 50]
        local = []
        for s in shards:     # scan on every rank first (collective order), then resolve everywhere
            keys = np.empty(len(batch), dtype=np.uint64)
            _lib.check(s._lib.rs_vt_scan_local(s._h, len(batch), _lib.ptr(batch, ctypes.c_uint8),
                                               _lib.ptr(keys, ctypes.c_uint64)))
            local.append(keys)
        glob = np.minimum.reduce(local)
        trace += [ref.match_template(x) for x in batch]
        expect = np.array([t[0] for t in trace[lo:]])
        for s in shards:
            idx = np.empty(len(batch), dtype=np.int64)
            new = np.empty(len(batch), dtype=np.uint8)
            _lib.check(s._lib.rs_vt_resolve(s._h, len(batch), _lib.ptr(glob, ctypes.c_uint64), 1,
                                            None, _lib.ptr(idx, ctypes.c_int64),
                                            _lib.ptr(new, ctypes.c_uint8)))
            assert np.array_equal(idx, expect)
        assert np.array_equal(single.match_templates(batch)[0], expect)
    assert min(trace_counts(trace, len(base), 50)) >= 1     # appends and every kind of hit
    total = len(ref.templates)
    assert single.count() == total
    assert all(s.count() == total for s in shards)
    for s in shards + [single]:
        s.close()


# --- d. match_stream ------------------------------------------------------------
@pytest.mark.parametrize('t,nb,q', [(70, 3, 33), (0, 2, 5)])
@pytest.mark.parametrize('shape', [(64, 32), (32, 30), (40, 32)])
def test_match_stream(vtmod, shape, t, nb, q):
    """rs_vt_match_stream on a SAD handle (a form build and a scan per batch), from host
    memory and from batches resident in HBM: equal to each other, to nb frozen
    match_templates calls and to the restatement on every query; an empty library gives
    (-1, UINT64_MAX)."""
    from pyratslam_amd import _lib
    full = V.synthetic_library(max(t, 8), *shape, seed=t + 5)
    lib_np = full[:t]
    batches = np.stack([two_sided_queries(full, q, seed=100 + b) for b in range(nb)])
    lib = new_handle(vtmod, shape, 45000)
    if t:
        lib.add(lib_np)
    idx_h, score_h = lib.match_stream(batches)
    buf = _lib.DeviceBuffer(batches.nbytes).upload(batches)
    idx_d, score_d = lib.match_stream((nb, q, buf))
    buf.close()
    assert np.array_equal(idx_h, idx_d) and np.array_equal(score_h, score_d)
    for b in range(nb):
        idx, score, new = lib.match_templates(batches[b], mode=0)
        assert not new.any()
        assert np.array_equal(idx_h[b], idx) and np.array_equal(score_h[b], score)
    if t == 0:
        assert (idx_h == -1).all() and (score_h == U64_MAX).all()
    else:
        ref = np.stack([sad_matrix(lib_np, batch) for batch in batches])
        assert np.array_equal(score_h, ref.min(axis=2))
        assert np.array_equal(idx_h, ref.argmin(axis=2))
    assert lib.count() == t
    lib.close()


# --- e. match_frames through the public constructor ---------------------------
@pytest.mark.parametrize('geom,shape,first', [(((0, 128), (0, 64), 2, 2, 128, 128), (64, 32), 0),
                                              (((0, 64), (0, 60), 2, 2, 64, 64), (32, 30), 60)])
def test_match_frames_public_constructor(vtmod, geom, shape, first):
    """ViewTemplates(x_range, y_range, ..., metric='sad'): whole frames gathered on the device
    (vt_gather_kernel -> vt_qform_sad_kernel) in three calls, from host memory and from HBM,
    against the restatement's sequence on the same frames and against match() frame by frame.
    The 60 queries of the sequence from `first` on: a stretch with every kind of hit."""
    from pyratslam_amd import _lib
    thr = pixel_threshold(shape)
    mask, mshape = V.py2_mask(*geom)
    assert mshape == shape
    base, qs = sequence_case(shape)
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (60,) + mask.shape, dtype=np.uint8)   # noise off the mask
    for f, x in zip(frames, qs[first:first + 60]):
        f[mask] = x.ravel()
    pcs = [(k % 21, (3 * k) % 21, (5 * k) % 36) for k in range(60)]
    ref = SadOracle(thr, base, mask, shape)
    trace = [ref.match(f, *pc) for f, pc in zip(frames, pcs)]
    expect = np.array([t[0] for t in trace])
    counts = trace_counts(trace, len(base), 20)
    print('new / base hits / same-call hits / earlier-call hits:', counts)
    assert counts[0] >= 1 and counts[1] >= 1 and counts[2] + counts[3] >= 1, counts
    host, dev, single = (vtmod.ViewTemplates(*geom, thr, metric='sad') for _ in range(3))
    for vts in (host, dev, single):
        assert vts.shape == shape and vts.scan_form() == 'sad'
        vts.add(base)
    buf = _lib.DeviceBuffer(frames.nbytes).upload(frames)
    got_h, got_d = [], []
    for lo in (0, 20, 40):
        got_h.append(host.match_frames(frames[lo:lo + 20], pcs[lo:lo + 20])[0])
        got_d.append(dev.match_frames((20, buf.offset(lo * mask.size)), pcs[lo:lo + 20])[0])
    buf.close()
    got_s = [single.match(f, *pc).get_index() for f, pc in zip(frames, pcs)]
    assert np.array_equal(np.concatenate(got_h), expect)
    assert np.array_equal(np.concatenate(got_d), expect)
    assert np.array_equal(got_s, expect)
    for vts in (host, dev, single):
        assert np.array_equal(np.stack([t.template for t in vts.templates]), np.stack(ref.templates))
        assert [t.location() for t in vts.templates] == ref.locations
        vts.close()


# --- f. ViewTemplate.match, the default metric beside it, the ABI ---------------
def test_view_template_match_scores_by_the_owners_metric(vtmod):
    """ViewTemplate.match on a template a SAD library owns (through the library's scores()),
    on one a sharded SAD library owns (through its _solo helper, which inherits the metric),
    and the mixed-dtype fidelity path's uint8 pairs."""
    from pyratslam_amd.view_templates import numpy_sad_u8_scores
    shape = (64, 32)
    lib_np = V.synthetic_library(6, *shape, seed=4)
    q = two_sided_queries(lib_np[2:3], 1, seed=1)[0]
    want = numpy_sad_u8_scores(lib_np, q)
    assert want[2] != V.vt_scores_library(lib_np, q)[2]      # the metrics differ on this pair
    lib = new_handle(vtmod, shape, np.inf)
    lib.add(lib_np)
    for g in range(6):
        s = lib.templates[g].match(q)
        assert s == want[g] and s.dtype == np.uint64
    shard = vtmod.ShardedViewTemplates.from_shape(shape, np.inf, 0, 2, reducer=lambda k: k, metric='sad')
    shard.add(lib_np)
    assert shard.templates[2].match(q) == want[2]
    assert shard.templates[2]._solo.metric == 'sad'
    # a float frame at a library of uint8 templates: the host's list, pair by pair; a uint8
    # frame then scores its uint8 pairs by the library's metric
    mixed = vtmod.ViewTemplates._from_shape(shape, 5000, metric='sad')
    mixed.mask = np.ones(shape, dtype=bool)
    mixed.add(lib_np)
    assert mixed.match(np.full(shape, 300.0, np.float32), 0, 0, 0).get_index() == 6
    assert mixed.match(q, 0, 0, 0).get_index() == 2          # SAD of a few hundred; wrapped would miss
    assert want[2] < 5000 < V.vt_scores_library(lib_np, q)[2]
    for h in (lib, shard, mixed):
        h.close()


def test_default_handle_keeps_the_wrapped_plane_scan(vtmod):
    """The default metric on the inputs of the first frozen case: still the plane scan, still
    the wrapped scores; rs_vt_metric tells the two handles apart."""
    from pyratslam_amd import _lib
    t, q, h, w = FROZEN_CASES[0]
    lib_np = V.synthetic_library(t, h, w, seed=t)
    queries = two_sided_queries(lib_np, q, seed=q)
    lib = vtmod.ViewTemplates._from_shape((h, w), 45000)
    sad = new_handle(vtmod, (h, w), 45000)
    assert lib.metric == 'wrapped' and lib.scan_form().startswith('plane')
    for vts, code in ((lib, _lib.RS_VT_METRIC_WRAPPED), (sad, _lib.RS_VT_METRIC_SAD)):
        m = ctypes.c_int(-1)
        _lib.check(vts._lib.rs_vt_metric(vts._h, ctypes.byref(m)))
        assert m.value == code
    lib.add(lib_np)
    ref = np.stack([V.vt_scores_library(lib_np, x) for x in queries])
    idx, score, _ = lib.match_templates(queries, mode=0)
    assert np.array_equal(score, ref.min(axis=1)) and np.array_equal(idx, ref.argmin(axis=1))
    assert np.array_equal(lib.scores(queries), ref)
    assert not np.array_equal(ref, sad_matrix(lib_np, queries))
    lib.close()
    sad.close()


def test_abi_refusals_leave_the_handle_null(vtmod):
    from pyratslam_amd import _lib
    lib = _lib.require_device()
    for args in ((64, 32, 8, 0, 64, 0, 2), (64, 32, 8, 0, 64, 0, -1),     # unknown metric
                 (0, 32, 8, 0, 64, 0, 1), (64, 32, 0, 0, 64, 0, 1),        # bad shape / max_offset
                 (64, 32, 8, 0, -1, 0, 1), (64, 32, 8, 0, 64, 10 ** 6, 1)):    # capacity / device
        h = ctypes.c_void_p(0xDEAD)
        assert lib.rs_vt_create_metric(*args, ctypes.byref(h)) == _lib.RS_ERR_ARG, args
        assert not h.value
        assert (b'metric' in lib.rs_last_error()) == (args[6] not in (0, 1))
    assert lib.rs_vt_create_metric(64, 32, 8, 0, 64, 0, 1, None) == _lib.RS_ERR_ARG
    m = ctypes.c_int(7)
    assert lib.rs_vt_metric(None, ctypes.byref(m)) == _lib.RS_ERR_ARG and m.value == 7


# --- g. replay -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ros_case(n=120, thr=2048):
    from pyratslam_amd import replay, synthetic
    events = synthetic.ros_stream(n)
    frames = np.stack([ev[2] for ev in events if ev[0] == 'image'])
    mask, shape = V.py2_mask(replay.X_RANGE, replay.Y_RANGE, replay.X_STEP, replay.Y_STEP, *replay.IM_SIZE)
    ref = SadOracle(thr, (), mask, shape)
    index = np.array([ref.match(f)[0] for f in frames])
    return events, frames, index


@pytest.mark.parametrize('how', ['per-frame', 'window', 'window-feedback', 'frames'])
def test_replay_under_sad(vtmod, how):
    """ros_stream(120) with vt_metric='sad', match_threshold=2048: the template index of
    every frame is the restatement's sequence, frame by frame, in windows of 8 with and
    without feedback, and through replay_frames(batch=7)."""
    from pyratslam_amd import replay
    events, frames, index = ros_case()
    assert 1 < index.max() + 1 < len(index)          # places are created and revisited
    kw = dict(vt_metric='sad', match_threshold=2048)
    if how == 'frames':
        r = replay.RatslamReplay(use_visual_odometry=True, **kw).replay_frames(frames, batch=7)
    else:
        r = replay.RatslamReplay(window=8 if how.startswith('window') else 1,
                                 feedback_energy=0.02 if how.endswith('feedback') else None, **kw)
        assert r._windowed() == how.startswith('window')
        r.replay_events(events)
    assert r.vts.metric == 'sad' and r.vts.scan_form() == 'sad'
    res = r.results()
    assert np.array_equal(res['template_index'], index)
    assert res['templates'] == index.max() + 1
