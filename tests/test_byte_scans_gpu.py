"""The byte-SWAR scans of the uint8 view-template matcher (vt_scan_carry_kernel,
vt_scan_carry_col_kernel, vt_scan_generic_kernel) at the shapes that reach them
without an environment switch: H in {32, 64} with W != 32 (carry forms) and any
other H (generic form).  Integer work: scores, first-argmin indices, is_new and
the stored templates equal the oracle exactly.  tests/test_carry_identity.py
pins the formulation itself on the CPU."""
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
    return 'carry' if shape[0] in (32, 64) else 'generic'


def new_handle(vtmod, shape, thr):
    """A handle on the byte scans: a later change of the dispatch cannot move the
    case onto the plane scan unnoticed."""
    lib = vtmod.ViewTemplates._from_shape(shape, thr)
    assert lib.scan_form() == form_of(shape)
    return lib


def pixel_threshold(shape):
    """The shipped 45000 of a 48 x 32 window (64 x 32 templates), kept per pixel."""
    return 29 * (shape[0] - 16) * shape[1]


def make_oracle(shape, thr, templates=()):
    ref = V.ViewTemplatesOracle((0, 2), (0, 2), 1, 1, 2, 2, thr)
    ref.shape = tuple(shape)
    ref.templates = [np.array(t) for t in templates]
    return ref


# --- a. frozen scan and full score matrix ------------------------------------
# ntb = ceil(t / 64), WD = ceil(W / 4); match_templates launches the keys
# instance (MATRIX = false), scores() the matrix instance.
FROZEN_CASES = [
    # carry<64,2,false> / carry<64,2,true>: WD = 12 > 8 rules the column form out; the
    # last block holds 12 slots; odd q, so the NQ = 2 tail clamp runs
    (140, 37, 64, 48),
    # carry_col<32,1> (ntb*nq = 132, WD = 5: three idle column lanes) / carry<32,2,true>
    (200, 33, 32, 20),
    # carry<32,2,false> (ntb*nq = 2061 >= 2048; 9 template blocks, the last of 8 slots;
    # 115 query groups padded to 120: blocks return early) / carry<32,2,true>
    (520, 229, 32, 20),
    # carry_col<32,1> (WD = 8) / carry<32,2,true>, W % 4 = 2: padding bytes in the last
    # dword of every row
    (200, 33, 32, 30),
    # carry_col<64,1> / carry<64,2,true>, WD = 1, W < 4
    (70, 9, 64, 3),
    # generic<false> / generic<true>, although W = 32
    (90, 21, 40, 32),
    # generic, two-row window; one template in the second block
    (65, 6, 18, 8),
    # generic, H = 2 * max_offset: the window is empty, every score 0 and every index 0,
    # as the reference's empty slices give
    (64, 5, 16, 32),
]


@pytest.mark.parametrize('t,q,h,w', FROZEN_CASES)
def test_frozen_scan_and_score_matrix(vtmod, t, q, h, w):
    rng = np.random.default_rng(1000 * h + w)
    lib_np = V.synthetic_library(t, h, w, seed=t)
    lib_np[5] = 0
    lib_np[6] = 255
    lib_np[7] = np.where(rng.random((h, w)) < 0.5, 0, 255)
    queries, _ = V.synthetic_queries(lib_np, q, seed=q)
    queries[0] = 255
    queries[1] = 0
    ref = np.stack([V.vt_scores_library(lib_np, x) for x in queries])
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


@pytest.mark.parametrize('shape', [(64, 48), (32, 20), (40, 32)])
def test_ties_pick_first_index(vtmod, shape):
    """70 templates stored twice: every query's minimum is tied between slot g of the
    first block and slot g + 70 of the second or third; the packed keys' atomic
    minimum keeps the lower index (carry, carry_col and generic key emits)."""
    t = V.synthetic_library(70, *shape, seed=2)
    lib = new_handle(vtmod, shape, 10 ** 9)
    lib.add(np.concatenate([t, t]))
    idx, score, _ = lib.match_templates(t[::3], mode=0)
    assert np.array_equal(idx, np.arange(0, 70, 3)) and (score == 0).all()


# --- b. sequential in-batch semantics ----------------------------------------
@functools.lru_cache(maxsize=None)
def sequence_case(shape, nbase=40, n=300):
    """Base templates and a query sequence that appends, hits base templates, and
    hits templates appended earlier (generator of the module's sequential tests):
    50% a base template rolled by -7..7 minus noise in 0..2, 15% the same with
    noise in 0..59 (near the threshold), 17% a fresh image, 18% an exact copy of
    one of the previous 40 queries.  Noise stays one-sided against a clean
    template (a noisy copy against another noisy copy wraps mod 256)."""
    h, w = shape
    base = V.synthetic_library(nbase, h, w, seed=8)
    rng = np.random.default_rng(9)
    qs = np.empty((n, h, w), np.uint8)
    for i in range(n):
        u = rng.random() if i else 0.0
        if u < 0.65:
            b = np.roll(base[int(rng.integers(0, nbase))], int(rng.integers(-7, 8)), axis=0)
            noise = rng.integers(0, 3 if u < 0.5 else 60, (h, w))
            qs[i] = np.clip(b.astype(np.int64) - noise, 0, 255)
        elif u < 0.82:
            qs[i] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        else:
            qs[i] = qs[int(rng.integers(max(0, i - 40), i))]
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
    ref = make_oracle(shape, pixel_threshold(shape), base)
    trace = [ref.match_template(q) for q in qs]
    return trace, np.stack(ref.templates)


@pytest.mark.parametrize('shape', [(64, 48), (32, 20), (32, 30), (40, 32)])
def test_sequential_batches_equal_oracle_sequence(vtmod, shape):
    """ViewTemplates.match semantics inside and across batches of 64 on the byte
    scans: the candidate buffer and its score matrix (MATRIX instances), appends
    through the padded store, later queries preferring a template of their own batch."""
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


# --- c. simulated shards, read round trip ------------------------------------
def read_template(lib, g):
    from pyratslam_amd import _lib
    out = np.full(lib.shape, 0xEE, dtype=np.uint8)
    _lib.check(lib._lib.rs_vt_read(lib._h, g, _lib.ptr(out, ctypes.c_uint8)))
    return out


def test_sharded_ranks_simulated_on_one_gpu(vtmod):
    """Three handles on one GPU, each owning templates g % 3 == rank, at (32, 20);
    the elementwise min over their local keys plays the RCCL allreduce(min)."""
    from pyratslam_amd import _lib
    shape, nranks = (32, 20), 3
    thr = pixel_threshold(shape)
    base, queries = sequence_case(shape)
    queries = queries[:200]
    shards = [vtmod.ShardedViewTemplates.from_shape(shape, thr, r, nranks, reducer=lambda k: k)
              for r in range(nranks)]
    single = new_handle(vtmod, shape, thr)
    for s in shards:
        assert s.scan_form() == 'carry'
        s.add(base)
    single.add(base)
    ref = make_oracle(shape, thr, base)
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
    for g in range(total):        # every template readable on its owner: the padded layout at W = 20
        assert np.array_equal(read_template(shards[g % nranks], g), ref.templates[g]), g
        assert np.array_equal(read_template(single, g), ref.templates[g]), g


def test_read_round_trip_with_padding_bytes(vtmod):
    """rs_vt_read of every stored template at W % 4 = 2, two template blocks."""
    lib_np = V.synthetic_library(70, 32, 30, seed=33)
    lib_np[3] = 255
    lib = new_handle(vtmod, (32, 30), 45000)
    lib.add(lib_np)
    for g in range(70):
        assert np.array_equal(read_template(lib, g), lib_np[g]), g


# --- d. match_stream on non-planar handles -----------------------------------
@pytest.mark.parametrize('t,nb,q', [(70, 3, 33), (0, 2, 5)])
@pytest.mark.parametrize('shape', [(32, 30), (40, 32)])
def test_match_stream_per_batch_loop(vtmod, shape, t, nb, q):
    """rs_vt_match_stream on a handle without planes runs one form build and one scan
    per batch, reusing the raw and form buffers batch after batch, from host memory
    and from batches resident in HBM: equal to each other, to nb frozen
    match_templates calls and to the oracle on every query."""
    from pyratslam_amd import _lib
    full = V.synthetic_library(max(t, 8), *shape, seed=t + 5)
    lib_np = full[:t]
    batches = np.stack([V.synthetic_queries(full, q, seed=100 + b)[0] for b in range(nb)])
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
        ref = np.stack([[V.vt_scores_library(lib_np, x) for x in batch] for batch in batches])
        assert np.array_equal(score_h, ref.min(axis=2))
        assert np.array_equal(idx_h, ref.argmin(axis=2))
    assert lib.count() == t


def test_match_stream_per_batch_collective_one_rank(vtmod):
    """A handle without planes and a 1-rank RCCL communicator: rs_vt_match_stream's per-batch
    path with each batch's row min-reduced on the collective stream (evScan, evComm) while
    the next batch is built and scanned, the main stream joined before the export.  Twice,
    so the collective stream and its events are reused: equal to a plain handle's
    match_stream and to the oracle's minimum and first argmin on every query."""
    shape, t, nb, q = (32, 30), 70, 3, 33
    lib_np = V.synthetic_library(t, *shape, seed=t + 5)
    batches = np.stack([V.synthetic_queries(lib_np, q, seed=100 + b)[0] for b in range(nb)])
    uid = vtmod.ShardedViewTemplates.unique_id()
    s = vtmod.ShardedViewTemplates.from_shape(shape, 45000, 0, 1, reducer='rccl', unique_id=uid)
    plain = new_handle(vtmod, shape, 45000)
    assert s.scan_form() == 'carry' and plain.scan_form() == 'carry'
    s.add(lib_np)
    plain.add(lib_np)
    ref = np.stack([[V.vt_scores_library(lib_np, x) for x in batch] for batch in batches])
    ref_idx, ref_score = plain.match_stream(batches)
    for _ in range(2):
        idx, score = s.match_stream(batches)
        assert np.array_equal(idx, ref_idx) and np.array_equal(score, ref_score)
        assert np.array_equal(score, ref.min(axis=2))
        assert np.array_equal(idx, ref.argmin(axis=2))
    assert s.count() == t
    s.close()
    plain.close()


# --- e. match_frames through the public constructor ---------------------------
@pytest.mark.parametrize('geom,shape', [(((0, 128), (0, 96), 2, 2, 128, 128), (64, 48)),
                                        (((0, 64), (0, 40), 2, 2, 64, 64), (32, 20))])
def test_match_frames_public_constructor(vtmod, geom, shape):
    """ViewTemplates(x_range, y_range, ...) with a crop other than the shipped ones:
    whole frames gathered on the device (vt_gather_kernel -> vt_qform_kernel) in three
    calls, from host memory and from HBM, against ViewTemplatesOracle.match on the
    same frames and against match() frame by frame."""
    from pyratslam_amd import _lib
    thr = pixel_threshold(shape)
    mask, mshape = V.py2_mask(*geom)
    assert mshape == shape
    base, qs = sequence_case(shape)
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (60,) + mask.shape, dtype=np.uint8)   # noise off the mask
    for f, x in zip(frames, qs):
        f[mask] = x.ravel()
    pcs = [(k % 21, (3 * k) % 21, (5 * k) % 36) for k in range(60)]
    ref = V.ViewTemplatesOracle(*geom, thr)
    ref.templates = [np.array(b) for b in base]      # the clean templates the queries come from
    ref.locations = [(0, 0, 0)] * len(base)
    trace = [ref.match(f, *pc) for f, pc in zip(frames, pcs)]
    expect = np.array([t[0] for t in trace])
    counts = trace_counts(trace, len(base), 20)
    print('new / base hits / same-call hits / earlier-call hits:', counts)
    assert counts[0] >= 1 and counts[1] >= 1 and counts[2] + counts[3] >= 1, counts
    host, dev, single = (vtmod.ViewTemplates(*geom, thr) for _ in range(3))
    for vts in (host, dev, single):
        assert vts.shape == shape and vts.scan_form() == 'carry'
        assert np.array_equal(vts.mask, mask)
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
