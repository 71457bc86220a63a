"""The row offset of a view-template match on the GPU (csrc/vt_offset.h: vt_offset_profile_kernel;
rs_vt_offset_profile, ViewTemplates.offset_profile / offsets=True / shift_axis='cols',
RatslamReplay(view_shift=True)).  Integer work with no tolerance: offsets and whole profiles equal
the NumPy restatement (numpy_offset_profile, which tests/test_vt_offset.py pins to the explicit
loop), for both metrics, every scan form and every way the queries arrive."""
import ctypes

import numpy as np
import pytest

from oracle import view_templates as V

pytestmark = pytest.mark.gpu

U32_MAX = 0xFFFFFFFF


@pytest.fixture(scope='module')
def vtmod():
    from pyratslam_amd import _build
    _build.build()
    import pyratslam_amd.view_templates as m
    return m


@pytest.fixture(scope='module')
def L():
    from pyratslam_amd import _lib
    return _lib


def noisy_rolls(library, q, seed, noise=3):
    """Queries off a library: template i % T rolled by -7..7 rows plus two-sided noise."""
    rng = np.random.default_rng(seed)
    t, h, w = library.shape
    out = np.empty((q, h, w), np.uint8)
    for i in range(q):
        b = np.roll(library[i % t], int(rng.integers(-7, 8)), axis=0)
        out[i] = np.clip(b.astype(np.int64) + rng.integers(-noise, noise + 1, (h, w)), 0, 255)
    return out


def restated(vtmod, library, queries, index, metric, m=8):
    off = np.zeros(len(index), np.int32)
    prof = np.full((len(index), 2 * m - 1), U32_MAX, np.uint32)
    for i, g in enumerate(index):
        if g >= 0:
            off[i], prof[i] = vtmod.numpy_offset_profile(library[g], queries[i], m, metric)
    return off, prof


def first_argmin(profiles):
    return np.argmin(profiles, axis=1).astype(np.int32) - (profiles.shape[1] - 1) // 2


# (scan form, shape, metric, RS_VT_SCAN)
FORMS = [('plane-pruned', (64, 32), 'wrapped', None), ('plane', (32, 32), 'wrapped', None),
         ('carry', (64, 32), 'wrapped', 'carry'), ('carry', (32, 32), 'wrapped', 'carry'),
         ('sad', (64, 32), 'sad', None), ('sad', (32, 32), 'sad', None),
         ('generic', (24, 10), 'wrapped', None), ('generic', (16, 5), 'wrapped', None),
         ('sad-generic', (24, 10), 'sad', None), ('sad-generic', (16, 5), 'sad', None)]
# library size -> queries: 1, 2, 65 and 257 queries over libraries of 1, 64, 65 and 130 templates
SIZES = [(1, 2), (64, 1), (65, 65), (130, 257)]


@pytest.mark.parametrize('form,shape,metric,scan', FORMS)
def test_device_equals_the_restatement(vtmod, L, monkeypatch, form, shape, metric, scan):
    if scan:
        monkeypatch.setenv('RS_VT_SCAN', scan)
    h, w = shape
    for t, nq in SIZES:
        lib_np = V.synthetic_library(t, h, w, seed=t + h)
        if t > 5:
            lib_np[3], lib_np[4] = 0, 255
        vts = vtmod.ViewTemplates._from_shape(shape, 45000, capacity=64, metric=metric)
        assert vts.scan_form() == form
        vts.add(lib_np)
        qs = noisy_rolls(lib_np, nq, seed=nq)
        qs[0] = 0 if nq > 1 else qs[0]
        # slots 0, 63, 64 and the last, and -1 (no template), cycled over the queries
        slots = [s for s in (0, 63, 64, t - 1) if s < t] + [-1]
        index = np.array([slots[i % len(slots)] for i in range(nq)], np.int64)
        if nq == 1:
            index[:] = t - 1
        want_o, want_p = restated(vtmod, lib_np, qs, index, metric)
        # host queries
        off, prof = vts.offset_profile(index, qs)
        assert off.dtype == np.int32 and prof.dtype == np.uint32 and prof.shape == (nq, 15)
        assert np.array_equal(prof, want_p) and np.array_equal(off, want_o)
        if h == 16:      # an empty window: zeros and the first offset
            assert not prof[index >= 0].any() and (off[index >= 0] == -7).all()
        assert (prof[index < 0] == U32_MAX).all() and (off[index < 0] == 0).all()
        # device-resident queries, read in place
        buf = L.DeviceBuffer(qs.nbytes).upload(qs)
        off, prof = vts.offset_profile(index, (nq, buf))
        buf.close()
        assert np.array_equal(prof, want_p) and np.array_equal(off, want_o)
        # the batch a match staged: any indices may be profiled against it
        idx, score, _ = vts.match_templates(qs, mode=L.RS_VT_FROZEN)
        off, prof = vts.offset_profile(index)
        assert np.array_equal(prof, want_p) and np.array_equal(off, want_o)
        # ... and the match's own: the minimum is the score, the offset its first argmin
        off, prof = vts.offset_profile(idx)
        assert np.array_equal(prof.min(axis=1), score) and np.array_equal(off, first_argmin(prof))
        vts.close()


@pytest.mark.parametrize('metric', ['wrapped', 'sad'])
def test_abi_with_another_max_offset(vtmod, L, metric):
    """(10, 7) with max_offset 3 through the ABI: the generic instance, 5 offsets, W mod 4 = 3."""
    lib = L.require_device()
    h, w, m, t, nq = 10, 7, 3, 70, 9
    hd = ctypes.c_void_p()
    L.check(lib.rs_vt_create_metric(h, w, m, 0, 64, 0, vtmod.METRICS[metric], ctypes.byref(hd)))
    try:
        lib_np = V.synthetic_library(t, h, w, seed=7)
        L.check(lib.rs_vt_add(hd, t, L.ptr(lib_np, ctypes.c_uint8), None))
        rng = np.random.default_rng(3)
        qs = np.stack([np.roll(lib_np[i], int(rng.integers(-2, 3)), axis=0) for i in range(nq)])
        qs[1] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        index = np.array([0, 1, 63, 64, 69, -1, 5, 6, 64], np.int64)
        qs[3] = np.roll(lib_np[64], 1, axis=0)
        prof = np.zeros((nq, 2 * m - 1), np.uint32)
        off = np.zeros(nq, np.int32)
        L.check(lib.rs_vt_offset_profile(hd, nq, ctypes.c_void_p(qs.ctypes.data), L.ptr(index, ctypes.c_int64),
                                         L.ptr(prof, ctypes.c_uint32), L.ptr(off, ctypes.c_int32)))
        want_o, want_p = restated(vtmod, lib_np, qs, index, metric, m)
        assert np.array_equal(prof, want_p) and np.array_equal(off, want_o)
        assert off[0] in range(-2, 3) and prof[0].min() == 0 and off[3] == -1
        # profile may be NULL
        off2 = np.full(nq, 9, np.int32)
        L.check(lib.rs_vt_offset_profile(hd, nq, ctypes.c_void_p(qs.ctypes.data), L.ptr(index, ctypes.c_int64),
                                         None, L.ptr(off2, ctypes.c_int32)))
        assert np.array_equal(off2, want_o)
    finally:
        L.check(lib.rs_vt_destroy(hd))


def check_tie(vtmod, vts, stored, queries, idx, score, new, metric):
    """last_offsets / last_profiles of the call that returned (idx, score, new): the profile's
    minimum is the score and the offset its first argmin; a query that became a template meets
    itself.  ``stored``: the library's templates after the call."""
    off, prof = vts.last_offsets, vts.last_profiles
    assert off.shape == idx.shape and prof.shape == (len(idx), 15)
    old = ~new & (idx >= 0)
    assert np.array_equal(prof[old].min(axis=1), score[old])
    assert np.array_equal(off[old], first_argmin(prof[old]))
    assert (prof[new][:, 7] == 0).all() and (off[new] == 0).all()
    want_o, want_p = restated(vtmod, stored, queries, idx, metric)
    assert np.array_equal(prof, want_p)
    assert np.array_equal(off[old], want_o[old])


@pytest.mark.parametrize('shape,metric', [((64, 32), 'wrapped'), ((32, 32), 'sad'), ((24, 10), 'wrapped')])
def test_offsets_follow_match_templates(vtmod, L, shape, metric):
    from pyratslam_amd import synthetic
    h, w = shape
    thr = 29 * (h - 16) * w
    lib_np = V.synthetic_library(130, h, w, seed=11)
    vts = vtmod.ViewTemplates._from_shape(shape, thr, capacity=64, metric=metric, offsets=True)
    assert vts.last_offsets is None
    vts.add(lib_np)
    qs, _ = synthetic.queries_fast(lib_np, 150, seed=5)      # rolled by -7..7 with noise, one in ten fresh
    idx, score, new = vts.match_templates(qs, mode=L.RS_VT_FROZEN)
    assert not new.any()
    check_tie(vtmod, vts, lib_np, qs, idx, score, new, metric)
    idx, score, new = vts.match_templates(qs)                # sequential: the fresh ones are appended
    assert 3 < new.sum() < 40
    stored = np.stack([np.asarray(t.template) for t in vts.templates])
    check_tie(vtmod, vts, stored, qs, idx, score, new, metric)
    vts.close()
    # an empty library: the second query is the first rolled by 3 rows and matches the template
    # the first one just created, in the same batch
    vts = vtmod.ViewTemplates._from_shape(shape, thr, capacity=64, metric=metric, offsets=True)
    q0 = lib_np[9]
    batch = np.stack([q0, np.roll(q0, 3, axis=0), lib_np[10]])
    idx, score, new = vts.match_templates(batch)
    assert idx.tolist() == [0, 0, 1] and new.tolist() == [True, False, True] and score[1] == 0
    want = vtmod.numpy_offset_profile(q0, batch[1], 8, metric)
    assert want[0] == -3
    assert vts.last_offsets.tolist() == [0, -3, 0] and np.array_equal(vts.last_profiles[1], want[1])
    # frozen against an empty-handed index: -1 gives offset 0 and a row of UINT32_MAX
    empty = vtmod.ViewTemplates._from_shape(shape, thr, metric=metric, offsets=True)
    idx, score, new = empty.match_templates(batch, mode=L.RS_VT_FROZEN)
    assert (idx == -1).all() and (empty.last_offsets == 0).all() and (empty.last_profiles == U32_MAX).all()
    empty.close()
    vts.close()


@pytest.mark.parametrize('metric', ['wrapped', 'sad'])
def test_index_64_of_a_library_grown_by_one_append(vtmod, L, metric):
    shape = (64, 32)
    lib_np = V.synthetic_library(66, *shape, seed=2)
    vts = vtmod.ViewTemplates._from_shape(shape, 45000, capacity=64, metric=metric, offsets=True)
    vts.add(lib_np[:64])
    idx, score, new = vts.match_templates(lib_np[64:65])       # a fresh image: appended as index 64
    assert idx.tolist() == [64] and new.all() and len(vts) == 65
    assert vts.last_offsets.tolist() == [0] and vts.last_profiles[0, 7] == 0
    q = np.roll(lib_np[64], -5, axis=0)[None]
    off, prof = vts.offset_profile([64], q)
    want = vtmod.numpy_offset_profile(lib_np[64], q[0], 8, metric)
    assert off[0] == want[0] == 5 and np.array_equal(prof[0], want[1])
    idx, score, new = vts.match_templates(q)
    assert idx.tolist() == [64] and not new.any() and vts.last_offsets.tolist() == [5]
    vts.close()


def ros_templates(vtmod, thr, **kw):
    from pyratslam_amd import replay
    return vtmod.ViewTemplates(replay.X_RANGE, replay.Y_RANGE, replay.X_STEP, replay.Y_STEP, *replay.IM_SIZE, thr, **kw)


@pytest.mark.parametrize('metric', ['wrapped', 'sad'])
def test_offsets_follow_match_frames(vtmod, L, metric):
    """Whole frames gathered on the GPU, from the host and from HBM: a stored frame rolled by
    2k image rows is its template rolled by k rows (the mask keeps every second row)."""
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (6, 256, 256), dtype=np.uint8)
    # random 32 x 32 templates score about 62,000 (wrapped) or 40,000 (sad) against each other,
    # a rolled one with noise below 3 at most 2 * 512
    vts = ros_templates(vtmod, 8000, metric=metric, offsets=True)
    idx, score, new = vts.match_frames(base, None)
    assert new.all() and (vts.last_offsets == 0).all() and (vts.last_profiles[:, 7] == 0).all()
    stored = np.stack([vts.subsample(f) for f in base])
    ks = [-7, -3, 0, 2, 7, 5]
    frames = np.stack([np.roll(base[i], 2 * k, axis=0) for i, k in enumerate(ks)])
    frames[3] = np.clip(frames[3].astype(np.int64) - rng.integers(0, 3, (256, 256)), 0, 255)   # one-sided noise
    fresh = rng.integers(0, 256, (1, 256, 256), dtype=np.uint8)
    for mode in (L.RS_VT_FROZEN, L.RS_VT_SEQUENTIAL):
        batch = np.concatenate([frames, fresh]) if mode == L.RS_VT_SEQUENTIAL else frames
        qs = np.stack([vts.subsample(f) for f in batch])
        for device in (False, True):
            if mode == L.RS_VT_SEQUENTIAL and device:
                batch = batch[:6]      # (the fresh frame is a template by now)
                qs = qs[:6]
            buf = L.DeviceBuffer(batch.nbytes).upload(batch) if device else None
            idx, score, new = vts.match_frames((len(batch), buf) if device else batch, None, mode=mode)
            if buf is not None:
                buf.close()
            assert idx[:6].tolist() == list(range(6)) and not new[:6].any()
            assert vts.last_offsets[:6].tolist() == [-k for k in ks]
            lib_now = np.stack([np.asarray(t.template) for t in vts.templates])
            assert np.array_equal(lib_now[:6], stored)
            check_tie(vtmod, vts, lib_now, qs, idx, score, new, metric)
            if len(batch) == 7:
                assert new[6] and idx[6] == 6
    vts.close()


def test_explicit_queries_leave_the_staged_batch(vtmod, L):
    lib = L.require_device()
    shape = (64, 32)
    lib_np = V.synthetic_library(100, *shape, seed=4)
    vts = vtmod.ViewTemplates._from_shape(shape, 45000, capacity=128)
    vts.add(lib_np)
    qs = noisy_rolls(lib_np, 40, seed=6)
    idx, score, _ = vts.match_templates(qs, mode=L.RS_VT_FROZEN)
    other = noisy_rolls(lib_np[50:], 13, seed=7)
    off, prof = vts.offset_profile(np.arange(50, 63), other)
    want_o, want_p = restated(vtmod, lib_np, other, np.arange(50, 63), 'wrapped')
    assert np.array_equal(off, want_o) and np.array_equal(prof, want_p)
    # queries == NULL: the batch of 40 is still staged, and gives the keys it gave
    idx2 = np.empty(40, np.int64)
    score2 = np.empty(40, np.uint64)
    L.check(lib.rs_vt_match_batch(vts._h, 40, None, L.RS_VT_FROZEN, L.ptr(score2, ctypes.c_uint64),
                                  L.ptr(idx2, ctypes.c_int64), None))
    assert np.array_equal(idx2, idx) and np.array_equal(score2, score)
    off, prof = vts.offset_profile(idx)
    assert np.array_equal(prof.min(axis=1), score)
    vts.close()


def test_refusals_leave_the_handle_usable(vtmod, L):
    lib = L.require_device()
    shape = (32, 32)
    lib_np = V.synthetic_library(10, *shape, seed=1)
    vts = vtmod.ViewTemplates._from_shape(shape, 45000)
    vts.add(lib_np)
    qs = noisy_rolls(lib_np, 4, seed=2, noise=0)

    def works():
        idx, score, _ = vts.match_templates(qs, mode=L.RS_VT_FROZEN)
        assert idx.tolist() == [0, 1, 2, 3]
        off, prof = vts.offset_profile(idx)
        assert np.array_equal(prof.min(axis=1), score)

    works()
    for bad in ([0, 1, 2, 10], [0, -2, 1, 2], [0, 1, 2, 1 << 40]):
        with pytest.raises(ValueError, match='outside'):          # RS_ERR_ARG
            vts.offset_profile(bad, qs)
        with pytest.raises(ValueError, match='outside'):
            vts.offset_profile(bad)
        works()
    index = np.zeros(3, np.int64)
    off = np.zeros(3, np.int32)
    st = lib.rs_vt_offset_profile(vts._h, 3, None, L.ptr(index, ctypes.c_int64), None, L.ptr(off, ctypes.c_int32))
    assert st == L.RS_ERR_STATE and b'staged' in lib.rs_last_error()      # 4 staged, 3 asked for
    with pytest.raises(L.HipLibraryError, match='staged'):
        vts.offset_profile([0, 1, 2])
    works()
    with pytest.raises(ValueError):
        vts.offset_profile([0, 1], qs)         # 4 queries for 2 indices
    vts.add(lib_np[:1])                        # the staging buffer now holds templates
    with pytest.raises(L.HipLibraryError, match='staged'):
        vts.offset_profile([0, 1, 2, 3])
    works()
    vts.close()
    # a sharded handle: RS_ERR_STATE from the ABI, TypeError from the class
    hd = ctypes.c_void_p()
    L.check(lib.rs_vt_create(32, 32, 8, 0, 64, 0, ctypes.byref(hd)))
    L.check(lib.rs_vt_set_shard(hd, 0, 2))
    L.check(lib.rs_vt_add(hd, 4, L.ptr(lib_np, ctypes.c_uint8), None))
    index = np.zeros(1, np.int64)
    st = lib.rs_vt_offset_profile(hd, 1, ctypes.c_void_p(qs.ctypes.data), L.ptr(index, ctypes.c_int64), None,
                                  L.ptr(off, ctypes.c_int32))
    assert st == L.RS_ERR_STATE and b'unsharded' in lib.rs_last_error()
    L.check(lib.rs_vt_destroy(hd))
    sh = vtmod.ShardedViewTemplates.from_shape(shape, 45000, 0, 2, reducer=lambda k: k)
    with pytest.raises(TypeError, match='sharded'):
        sh.offset_profile([0], qs[:1])
    sh.close()
    with pytest.raises(TypeError, match='sharded'):
        vtmod.ShardedViewTemplates.from_shape(shape, 45000, 0, 2, reducer=lambda k: k, offsets=True)
    # a float library
    fl = vtmod.ViewTemplates._from_shape(shape, 45000)
    fl.add(lib_np.astype(np.float32))
    assert fl.scan_form() == 'sad-resident'
    with pytest.raises(TypeError, match='float'):
        fl.offset_profile([0], qs[:1])
    assert fl.match_templates(qs.astype(np.float32), mode=L.RS_VT_FROZEN)[0].tolist() == [0, 1, 2, 3]
    fl.close()
    on = vtmod.ViewTemplates._from_shape(shape, 45000, offsets=True)
    with pytest.raises(TypeError, match='uint8'):
        on.match_templates(qs.astype(np.float32))
    with pytest.raises(TypeError, match='uint8'):
        on.add(lib_np.astype(np.float64))
    idx, _, new = on.match_templates(qs)       # still a uint8 device library
    assert new.all() and on.scan_form() == 'plane' and (on.last_offsets == 0).all()
    on.close()


def pano_frame(pano, col, rng=None, noise=0):
    f = pano[:, (col + np.arange(256)) % pano.shape[1]]
    if noise:
        f = np.clip(f.astype(np.int64) + rng.integers(-noise, noise + 1, f.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(f)


@pytest.mark.parametrize('noise', [0, 3])
def test_column_major_templates_measure_the_heading(vtmod, L, noise):
    """shift_axis='cols' on the synthetic panorama: a frame cut 2k columns further than the
    stored one matches it with offset k, through match_frames and through match()."""
    from pyratslam_amd import synthetic
    pano = synthetic.panorama(256, 1024, 0)
    rng = np.random.default_rng(noise)
    for c0 in (0, 517, 1000):
        vts = ros_templates(vtmod, 2048, metric='sad', shift_axis='cols', offsets=True)
        assert vts.shape == (32, 32)
        idx, _, new = vts.match_frames(pano_frame(pano, c0)[None], None)
        assert new.all()
        assert np.array_equal(vts.templates[0].template, vts.subsample(pano_frame(pano, c0)))
        frames = np.stack([pano_frame(pano, c0 + 2 * k, rng, noise) for k in range(-7, 8)])
        idx, score, new = vts.match_frames(frames, None)
        assert (idx == 0).all() and not new.any() and vts.last_offsets.tolist() == list(range(-7, 8))
        want_o, want_p = restated(vtmod, np.stack([vts.templates[0].template]),
                                  np.stack([vts.subsample(f) for f in frames]), idx, 'sad')
        assert np.array_equal(vts.last_profiles, want_p) and np.array_equal(vts.last_offsets, want_o)
        if noise == 0:
            assert (score == 0).all()
        for k in (-7, -1, 0, 4, 7):
            t = vts.match(frames[k + 7], 1, 2, 3)
            assert t.get_index() == 0 and vts.last_offsets.tolist() == [k]
            assert np.array_equal(vts.last_profiles[0], want_p[k + 7])
        assert len(vts) == 1
        vts.close()


# --- the replay ------------------------------------------------------------------------
THR = 2048          # 4 per window pixel under 'sad' (replay's help text); distinct views score > 5,000
# the heading in panorama columns after each twist (20 columns = 0.1227 rad a step), and the
# frames: a place is first seen at columns 0, 40 and 80; column 40 again; then the first
# heading plus 6 image columns (3 template rows), twice; then the second and the third place
# plus 6, the third twice: 9 frames, so that windows and batches of 7 split them
PATH = [0, 20, 40, 60, 80, 60, 40, 20, 6, 6, 26, 46, 66, 86, 86]
FRAME_AFTER = {0: 0, 2: 40, 4: 80, 6: 40, 8: 6, 9: 6, 11: 46, 13: 86, 14: 86}


def replay_events():
    from pyratslam_amd import synthetic
    pano = synthetic.panorama(256, 1024, 0)
    events, t, col = [('image', 99.9, pano_frame(pano, 0))], 100.0, 0
    for s in range(1, len(PATH)):
        dcol = PATH[s] - col
        col = PATH[s]
        # (1.3 m/s: 0.13 m a step, off the +0.5 edge of the pose cells' filter table that 0.1 m sits on)
        events.append(('odom', t, (1.3, 0.0, 0.0), (0.0, 0.0, dcol * 2 * np.pi / 1024 * 10)))
        if s in FRAME_AFTER:
            assert FRAME_AFTER[s] == col
            events.append(('image', t + 0.05, pano_frame(pano, col)))
        t += 0.1
    return events


def restated_replay(vtmod, frames):
    """ViewTemplates.match on the restatement, column-major: (index, offset) per frame."""
    from pyratslam_amd import replay
    geo = vtmod.ViewTemplates.__new__(vtmod.ViewTemplates)._set_geometry(
        replay.X_RANGE, replay.Y_RANGE, replay.X_STEP, replay.Y_STEP, *replay.IM_SIZE, 'cols')
    stored, index, offset = [], [], []
    for f in frames:
        q = geo.subsample(f)
        s = vtmod.numpy_sad_u8_scores(np.stack(stored), q) if stored else np.zeros(0)
        if len(s) == 0 or s.min() > THR:
            stored.append(q)
            index.append(len(stored) - 1)
            offset.append(0)
        else:
            index.append(int(np.argmin(s)))
            offset.append(vtmod.numpy_offset_profile(stored[index[-1]], q, 8, 'sad')[0])
    return index, offset


def ends(links):
    return links['a'].tolist(), links['b'].tolist()


def test_replay_hands_the_offset_to_the_linked_map(vtmod):
    from pyratslam_amd import LinkedExperienceMap, NumpyLinkedExperienceMap, replay
    events = replay_events()
    frames = np.stack([ev[2] for ev in events if ev[0] == 'image'])
    want_index, want_offset = restated_replay(vtmod, frames)
    assert want_index == [0, 1, 2, 1, 0, 0, 1, 2, 2] and want_offset == [0, 0, 0, 0, 3, 3, 3, 3, 3]
    rad = replay.X_STEP * (np.pi / 2) / 256

    def run(**kw):
        r = replay.RatslamReplay(view_shift=True, view_fov=np.pi / 2, vt_metric='sad', match_threshold=THR,
                                 em=LinkedExperienceMap(), **kw)
        assert r.vts.shift_axis == 'cols' and r.vts.offsets and r.rad_per_row == rad
        return r

    # odometry mode: frame by frame, and windows of 7 frames
    ref = NumpyLinkedExperienceMap()
    frame = 0
    for ev in events:
        if ev[0] == 'odom':
            ref.update(ev[2][0] / 10, ev[3][2] / 10)
        else:
            ref.on_template(want_index[frame], want_offset[frame] * rad)
            frame += 1
    assert len(ref.links()) == 4      # 0 -> 1 -> 2 -> 1 -> 0: the closures 2 -> 1 and 1 -> 0; 0 -> 1 and 1 -> 2 exist
    for window in (1, 7):
        r = run(window=window).replay_events(events)
        res = r.results()
        assert res['view_offset'].tolist() == want_offset and res['template_index'].tolist() == want_index
        assert ends(r.em.links()) == ends(ref.links())
        assert np.abs(r.em.poses() - ref.poses()).max() < 1e-12
        assert np.abs(r.em.links()['f'] - ref.links()['f']).max() < 1e-12
        r.em.close()
        r.vts.close()
    # the closure 1 -> 0 is faced by the stored heading: without the offset its facing would
    # carry the 6 columns the robot is turned by
    links = ref.links()
    back = links[(links['a'] == 1) & (links['b'] == 0)][0]
    plain = NumpyLinkedExperienceMap()
    frame = 0
    for ev in events:
        if ev[0] == 'odom':
            plain.update(ev[2][0] / 10, ev[3][2] / 10)
        else:
            plain.on_template(want_index[frame])
            frame += 1
    pl = plain.links()
    assert abs((pl[(pl['a'] == 1) & (pl['b'] == 0)][0]['f'] - back['f']) - 3 * rad) < 1e-12
    # camera only: the batched pipeline in batches of 64 and of 7, and the same offsets
    for batch in (64, 7):
        r = run(use_visual_odometry=True).replay_frames(frames, batch=batch)
        res = r.results()
        assert res['view_offset'].tolist() == want_offset and res['template_index'].tolist() == want_index
        cam = NumpyLinkedExperienceMap()
        for j, o, (vt, vr) in zip(want_index, want_offset, r.deltas):
            cam.on_template(j, o * rad)
            cam.update(vt, vr)
        assert ends(r.em.links()) == ends(cam.links())
        assert np.abs(r.em.poses() - cam.poses()).max() < 1e-12
        r.em.close()
        r.vts.close()
    # a library passed in without the offsets is refused
    plain_vts = ros_templates(vtmod, THR, metric='sad')
    with pytest.raises(ValueError, match='shift_axis'):
        replay.RatslamReplay(view_shift=True, view_fov=np.pi / 2, vt_metric='sad', vts=plain_vts)
    plain_vts.close()
