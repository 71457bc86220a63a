"""Patch-normalised uint8 view templates on the GPU (csrc/vt_norm.h: vt_normalise_kernel;
rs_vt_set_normalise, ViewTemplates(normalise=...), RatslamReplay(vt_normalise=...)).  Integer work
with no tolerance: the bytes a normalising handle keeps equal ``normalise_u8`` (which
tests/test_vt_norm.py pins to an explicit loop and to the host rule), and every way into such a
handle returns what a plain handle returns on images normalised on the host."""
import ctypes

import numpy as np
import pytest

import _vt_norm_cases as C
from oracle import view_templates as V

pytestmark = pytest.mark.gpu

NORM = (3, 32)


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


def library(t, shape, seed):
    """t images: random ones, with the 0/255 patterns, a constant and a low-contrast image among
    the first."""
    lib = np.random.default_rng(seed).integers(0, 256, (t,) + shape, dtype=np.uint8)
    for i, im in enumerate(C.images(shape, seed)[1:]):
        if 1 + i < t:
            lib[1 + i] = im
    return lib


def noisy(lib, nq, seed, noise=3):
    """Queries off a library: image i % T rolled by -3..3 rows, its grey levels moved by a
    constant, plus two-sided noise; every fifth one fresh."""
    rng = np.random.default_rng(seed)
    out = np.empty((nq,) + lib.shape[1:], np.uint8)
    for i in range(nq):
        b = np.roll(lib[i % len(lib)], int(rng.integers(-3, 4)), axis=0).astype(np.int64) + int(rng.integers(-20, 21))
        out[i] = np.clip(b + rng.integers(-noise, noise + 1, b.shape), 0, 255)
        if i % 5 == 4:
            out[i] = rng.integers(0, 256, b.shape)
    return out


def read(L, handle, index, shape):
    out = np.full(shape, 0x5A, dtype=np.uint8)
    L.check(L.require_device().rs_vt_read(handle, int(index), L.ptr(out, ctypes.c_uint8)))
    return out


def download(L, buf, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    L.check(L.require_device().rs_dev_copy(ctypes.c_void_p(out.ctypes.data), buf.ptr, nbytes))
    return out


def np_scores(vtmod, metric, lib, q, m=8):
    return V.vt_scores_library(lib, q, m) if metric == 'wrapped' else vtmod.numpy_sad_u8_scores(lib, q, m)


# --- the bytes a normalising handle keeps ----------------------------------------------------
# (70, 130) crosses the 32 x 32 tiles in both directions; the others around it are the tile side
# minus and plus one in either direction, and two tiles plus and minus one
BYTE_SHAPES = [((64, 32), None), ((64, 32), 'force'), ((32, 32), None), ((64, 48), None), ((24, 10), None),
               ((16, 5), None), ((70, 130), None), ((31, 33), None), ((33, 31), None), ((65, 63), None)]


@pytest.mark.parametrize('shape,prune', BYTE_SHAPES)
def test_stored_bytes_equal_the_restatement(vtmod, L, monkeypatch, shape, prune):
    if prune:
        monkeypatch.setenv('RS_VT_PRUNE', prune)
    for t in (1, 64, 65, 130):
        lib_np = library(t, shape, seed=t + shape[1])
        for radius in (1, 3, 7):
            vts = vtmod.ViewTemplates._from_shape(shape, 45000, capacity=64, normalise=(radius, 32))
            if shape == (64, 32):
                assert vts.scan_form() == 'plane-pruned'
            assert vts.normalise == (radius, 32)
            # in two calls: the second append starts inside a 64-slot block
            if t > 1:
                vts.add(lib_np[:t // 2])
            vts.add(lib_np[t // 2:])
            want = vtmod.normalise_u8(lib_np, radius, 32)
            # (a read is a copy per 16-byte chunk: the special images, the halves' seam, the block's)
            for g in sorted({0, 1, 2, 3, 4, 5, 6, 7, t // 2, 62, 63, 64, t - 1} & set(range(t))):
                assert np.array_equal(read(L, vts._h, g, shape), want[g]), (t, radius, g)
            assert np.array_equal(stored(vts), want)
            vts.close()


@pytest.mark.parametrize('metric', ['wrapped', 'sad'])
def test_abi_with_another_max_offset(vtmod, L, metric):
    """(10, 7) with max_offset 3 through the ABI: an image smaller than the window at R = 7,
    W mod 4 = 3, the getter, and a frozen match on the normalised bytes."""
    lib = L.require_device()
    h, w, m = 10, 7, 3
    for t in (1, 64, 65, 130):
        lib_np = library(t, (h, w), seed=t)
        qs = noisy(lib_np, 5, seed=t + 1)
        for radius, gain in ((1, 127), (3, 32), (7, 1)):
            hd = ctypes.c_void_p()
            L.check(lib.rs_vt_create_metric(h, w, m, 0, 64, 0, vtmod.METRICS[metric], ctypes.byref(hd)))
            try:
                r, g = ctypes.c_int(-1), ctypes.c_int(-1)
                L.check(lib.rs_vt_normalise(hd, ctypes.byref(r), ctypes.byref(g)))
                assert (r.value, g.value) == (0, 0)
                L.check(lib.rs_vt_set_normalise(hd, radius, gain))
                L.check(lib.rs_vt_normalise(hd, ctypes.byref(r), ctypes.byref(g)))
                assert (r.value, g.value) == (radius, gain)
                L.check(lib.rs_vt_add(hd, t, L.ptr(lib_np, ctypes.c_uint8), None))
                want = vtmod.normalise_u8(lib_np, radius, gain)
                for i in range(t):
                    assert np.array_equal(read(L, hd, i, (h, w)), want[i])
                idx = np.empty(5, np.int64)
                score = np.empty(5, np.uint64)
                L.check(lib.rs_vt_match_batch(hd, 5, L.ptr(qs, ctypes.c_uint8), L.RS_VT_FROZEN,
                                              L.ptr(score, ctypes.c_uint64), L.ptr(idx, ctypes.c_int64), None))
                qn = vtmod.normalise_u8(qs, radius, gain)
                for i in range(5):
                    s = np_scores(vtmod, metric, want, qn[i], m)
                    assert idx[i] == int(np.argmin(s)) and score[i] == s.min()
            finally:
                L.check(lib.rs_vt_destroy(hd))


# --- scores ---------------------------------------------------------------------------------
# (scan form, shape, metric, RS_VT_SCAN, RS_VT_PRUNE)
FORMS = [('plane-pruned', (64, 32), 'wrapped', None, 'force'), ('plane', (64, 32), 'wrapped', None, '0'),
         ('plane', (32, 32), 'wrapped', None, None), ('carry', (64, 32), 'wrapped', 'carry', None),
         ('carry', (32, 32), 'wrapped', 'carry', None), ('generic', (24, 10), 'wrapped', None, None),
         ('generic', (70, 130), 'wrapped', None, None), ('sad', (64, 32), 'sad', None, None),
         ('sad', (32, 32), 'sad', None, None), ('sad-generic', (24, 10), 'sad', None, None)]


@pytest.mark.parametrize('form,shape,metric,scan,prune', FORMS)
def test_keys_and_score_matrix_equal_the_restatement(vtmod, L, monkeypatch, form, shape, metric, scan, prune):
    if scan:
        monkeypatch.setenv('RS_VT_SCAN', scan)
    if prune:
        monkeypatch.setenv('RS_VT_PRUNE', prune)
    t, nq = (130, 7) if shape != (70, 130) else (66, 3)        # an odd query count
    lib_np = library(t, shape, seed=shape[0])
    qs = noisy(lib_np, nq, seed=shape[1])
    vts = vtmod.ViewTemplates._from_shape(shape, 45000, capacity=64, metric=metric, normalise=NORM)
    assert vts.scan_form() == form
    vts.add(lib_np)
    ln, qn = vtmod.normalise_u8(lib_np, *NORM), vtmod.normalise_u8(qs, *NORM)
    want = np.stack([np_scores(vtmod, metric, ln, q) for q in qn])
    idx, score, new = vts.match_templates(qs, mode=L.RS_VT_FROZEN)
    assert np.array_equal(idx, want.argmin(axis=1)) and np.array_equal(score, want.min(axis=1)) and not new.any()
    got = vts.scores(qs)
    assert got.shape == (nq, t) and np.array_equal(got, want)
    assert np.array_equal(vts.scores(qs[1:2], 63, 3), want[1:2, 63:66])
    vts.close()


# --- every entry against a plain handle on host-normalised images ----------------------------
def pair(vtmod, shape, thr, metric, lib_np, **kw):
    """A normalising handle filled with raw templates, a plain one with the same templates
    normalised on the host."""
    vn = vtmod.ViewTemplates._from_shape(shape, thr, capacity=64, metric=metric, normalise=NORM, **kw)
    vp = vtmod.ViewTemplates._from_shape(shape, thr, capacity=64, metric=metric, **kw)
    assert vp.normalise is None
    if len(lib_np):
        vn.add(lib_np)
        vp.add(vtmod.normalise_u8(lib_np, *NORM))
    return vn, vp


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def stored(vts):
    return np.stack([np.asarray(t.template) for t in vts.templates])


@pytest.mark.parametrize('shape,metric', [((64, 32), 'wrapped'), ((32, 32), 'sad'), ((24, 10), 'wrapped')])
def test_match_templates_in_both_modes(vtmod, L, shape, metric):
    lib_np = library(70, shape, seed=4)
    qs = noisy(lib_np, 33, seed=5)
    qn = vtmod.normalise_u8(qs, *NORM)
    # the threshold: the median of the restatement's scores, so that some queries become templates
    s = np.stack([np_scores(vtmod, metric, vtmod.normalise_u8(lib_np, *NORM), q) for q in qn]).min(axis=1)
    thr = int(np.sort(s)[16])
    vn, vp = pair(vtmod, shape, thr, metric, lib_np)
    got, want = vn.match_templates(qs, mode=L.RS_VT_FROZEN), vp.match_templates(qn, mode=L.RS_VT_FROZEN)
    assert same(got, want) and np.array_equal(got[1], s)
    # queries == NULL: the staged batch holds normalised bytes, and gives the keys it gave
    idx2, score2 = np.empty(33, np.int64), np.empty(33, np.uint64)
    L.check(L.require_device().rs_vt_match_batch(vn._h, 33, None, L.RS_VT_FROZEN, L.ptr(score2, ctypes.c_uint64),
                                                 L.ptr(idx2, ctypes.c_int64), None))
    assert np.array_equal(idx2, got[0]) and np.array_equal(score2, got[1])
    got, want = vn.match_templates(qs), vp.match_templates(qn)
    assert same(got, want) and 0 < got[2].sum() < 33 and len(vn) == len(vp) == 70 + got[2].sum()
    assert np.array_equal(stored(vn), stored(vp))
    for g in (0, 69, 70, len(vn) - 1):      # the appended ones were stored normalised, once
        assert np.array_equal(read(L, vn._h, g, shape), read(L, vp._h, g, shape))
    vn.close()
    vp.close()


@pytest.mark.parametrize('metric', ['wrapped', 'sad'])
def test_sequential_batches_from_an_empty_library(vtmod, L, metric):
    shape = (32, 32)
    base = library(12, shape, seed=9)
    qs = noisy(base, 150, seed=10)
    qn = vtmod.normalise_u8(qs, *NORM)
    thr = 5000 if metric == 'sad' else 60000     # (61 and 37 templates by the restatement)
    want_idx, want_score, lib = C.sequence_oracle(qn, thr, lambda lb, q: np_scores(vtmod, metric, lb, q))
    assert 20 < len(lib) < 80
    vn = vtmod.ViewTemplates._from_shape(shape, thr, capacity=64, metric=metric, normalise=NORM)
    idx, score = [], []
    for lo in range(0, 150, 64):
        i, s, _ = vn.match_templates(qs[lo:lo + 64])
        idx += i.tolist()
        score += s.tolist()
    assert idx == want_idx
    assert [None if w is None else g for g, w in zip(score, want_score)] == want_score
    assert np.array_equal(stored(vn), np.stack(lib))
    vn.close()


def ros_pair(vtmod, thr, metric, **kw):
    vn = vtmod.ViewTemplates(**C.ROS, match_threshold=thr, metric=metric, normalise=NORM, **kw)
    vp = vtmod.ViewTemplates(**C.ROS, match_threshold=thr, metric=metric, **kw)
    return vn, vp


def test_match_frames_from_the_host_and_from_hbm(vtmod, L):
    frames = C.place_frames()
    rev = C.revisit_frames(frames, 1.3, -30)
    vn, vp = ros_pair(vtmod, 3139, 'sad')
    tn = vtmod.normalise_u8(C.ros_templates(frames), *NORM)
    got, want = vn.match_frames(frames[:8], None), vp.match_templates(tn[:8])
    assert same(got, want)
    buf = L.DeviceBuffer(frames[8:].nbytes).upload(frames[8:])
    got, want = vn.match_frames((8, buf), None), vp.match_templates(tn[8:])
    assert same(got, want)
    assert np.array_equal(download(L, buf, frames[8:].nbytes), frames[8:].reshape(-1))      # gathered, never written
    buf.close()
    assert len(vn) == len(vp) and np.array_equal(stored(vn), stored(vp))       # from the host rule and from rs_vt_read
    qn = vtmod.normalise_u8(C.ros_templates(rev), *NORM)
    buf = L.DeviceBuffer(rev.nbytes).upload(rev)
    for mode in (L.RS_VT_FROZEN, L.RS_VT_SEQUENTIAL):
        want = vp.match_templates(qn, mode=mode)
        assert same(vn.match_frames(rev, None, mode=mode), want)
        assert same(vn.match_frames((16, buf), None, mode=mode), want)
    assert np.array_equal(download(L, buf, rev.nbytes), rev.reshape(-1))
    buf.close()
    vn.close()
    vp.close()


@pytest.mark.parametrize('shape,metric,scan', [((64, 32), 'wrapped', None), ((64, 32), 'sad', None),
                                                ((32, 32), 'wrapped', 'carry'), ((24, 10), 'wrapped', None)])
def test_match_stream_from_the_host_and_from_hbm(vtmod, L, monkeypatch, shape, metric, scan):
    """Planar handles take the fused path (HBM, several batches), the per-batch one (HBM, one
    batch) and the upload groups (host); the others go batch by batch."""
    if scan:
        monkeypatch.setenv('RS_VT_SCAN', scan)
    lib_np = library(130, shape, seed=6)
    vn, vp = pair(vtmod, shape, 45000, metric, lib_np)
    for nb, nq in ((5, 7), (1, 9), (2, 64)):
        qs = noisy(lib_np, nb * nq, seed=nb).reshape((nb, nq) + shape)
        want = vp.match_stream(vtmod.normalise_u8(qs.reshape((-1,) + shape), *NORM).reshape(qs.shape))
        assert same(vn.match_stream(qs), want)
        buf = L.DeviceBuffer(qs.nbytes).upload(qs)
        assert same(vn.match_stream((nb, nq, buf)), want)
        assert same(vn.match_stream((nb, nq, buf)), want)      # the caller's batches were left raw
        assert np.array_equal(download(L, buf, qs.nbytes), qs.reshape(-1))
        buf.close()
        assert same(vn.match_templates(qs[0], mode=L.RS_VT_FROZEN)[:2], (want[0][0], want[1][0]))
    vn.close()
    vp.close()


@pytest.mark.parametrize('shape,metric', [((64, 32), 'wrapped'), ((32, 32), 'sad'), ((24, 10), 'sad')])
def test_offset_profile_of_host_device_and_staged_queries(vtmod, L, shape, metric):
    lib_np = library(70, shape, seed=12)
    qs = noisy(lib_np, 9, seed=13)
    qn = vtmod.normalise_u8(qs, *NORM)
    vn, vp = pair(vtmod, shape, 45000, metric, lib_np)
    index = np.array([0, 1, 63, 64, 69, -1, 5, 6, 64], np.int64)
    want = vp.offset_profile(index, qn)
    ln = vtmod.normalise_u8(lib_np, *NORM)
    for i, g in enumerate(index):
        if g >= 0:
            o, p = vtmod.numpy_offset_profile(ln[g], qn[i], 8, metric)
            assert want[0][i] == o and np.array_equal(want[1][i], p)
    staged = noisy(lib_np, 9, seed=14)
    keys = vn.match_templates(staged, mode=L.RS_VT_FROZEN)
    assert same(vn.offset_profile(index, qs), want)                      # host queries
    buf = L.DeviceBuffer(qs.nbytes).upload(qs)
    assert same(vn.offset_profile(index, (9, buf)), want)                # device queries, left as they are
    assert np.array_equal(download(L, buf, qs.nbytes), qs.reshape(-1))
    buf.close()
    # the staged batch is untouched by both, and holds normalised bytes
    vp.match_templates(vtmod.normalise_u8(staged, *NORM), mode=L.RS_VT_FROZEN)
    assert same(vn.offset_profile(index), vp.offset_profile(index))
    off, prof = vn.offset_profile(keys[0])
    assert np.array_equal(prof.min(axis=1), keys[1])
    vn.close()
    vp.close()


def test_offsets_recorded_with_every_match(vtmod, L):
    shape = (64, 32)
    lib_np = library(66, shape, seed=15)
    qs = noisy(lib_np, 21, seed=16)
    vn, vp = pair(vtmod, shape, 20000, 'sad', lib_np, offsets=True)
    for mode in (L.RS_VT_FROZEN, L.RS_VT_SEQUENTIAL):
        got, want = vn.match_templates(qs, mode=mode), vp.match_templates(vtmod.normalise_u8(qs, *NORM), mode=mode)
        assert same(got, want)
        assert np.array_equal(vn.last_offsets, vp.last_offsets) and np.array_equal(vn.last_profiles, vp.last_profiles)
    assert len(vn) == len(vp) > 66
    vn.close()
    vp.close()


def test_view_template_match_normalises_once(vtmod, L):
    shape = (32, 32)
    lib_np = library(5, shape, seed=17)
    qs = noisy(lib_np, 3, seed=18)
    for metric in ('wrapped', 'sad'):
        vn, vp = pair(vtmod, shape, 45000, metric, lib_np)
        ln, qn = vtmod.normalise_u8(lib_np, *NORM), vtmod.normalise_u8(qs, *NORM)
        for g in (0, 4):
            assert np.array_equal(vn.templates[g].template, ln[g])
            for q, qh in zip(qs, qn):
                want = np_scores(vtmod, metric, ln[g:g + 1], qh)[0]
                assert vn.templates[g].match(q) == want == vp.templates[g].match(qh)
        with pytest.raises(TypeError, match='normalise'):
            vn.templates[0].match(qs[0].astype(np.float32))
        vn.close()
        vp.close()


def test_three_simulated_shards_with_a_callable_reducer(vtmod, L):
    """Three handles on one GPU, template g on rank g % 3; the reducer hands each rank the
    minimum over all three ranks' local keys, taken before any of them resolves."""
    shape = (64, 32)
    lib_np = library(31, shape, seed=19)
    box = {}
    shards = [vtmod.ShardedViewTemplates.from_shape(shape, 20000, r, 3, reducer=lambda k: box['keys'],
                                                    metric='sad', normalise=NORM) for r in range(3)]
    single = vtmod.ViewTemplates._from_shape(shape, 20000, metric='sad')
    for s in shards:
        assert s.normalise == NORM
        s.add(lib_np)
    single.add(vtmod.normalise_u8(lib_np, *NORM))
    qs = noisy(lib_np, 90, seed=20)
    for lo in range(0, 90, 30):
        batch = np.ascontiguousarray(qs[lo:lo + 30])
        local = []
        for s in shards:
            k = np.empty(30, np.uint64)
            L.check(s._lib.rs_vt_scan_local(s._h, 30, L.ptr(batch, ctypes.c_uint8), L.ptr(k, ctypes.c_uint64)))
            local.append(k)
        box['keys'] = np.minimum.reduce(local)
        want = single.match_templates(vtmod.normalise_u8(batch, *NORM))
        for s in shards:
            assert same(s.match_templates(batch), want)
    assert len(single) > 31 and all(len(s) == len(single) for s in shards)
    for g in range(len(single)):
        owner = shards[g % 3]
        assert np.array_equal(read(L, owner._h, g, shape), read(L, single._h, g, shape))
        assert np.array_equal(owner.templates[g].template, single.templates[g].template)
    # a template of a sharded owner is scored through a plain helper library: q normalised once
    q = qs[7]
    assert shards[31 % 3].templates[31].match(q) == single.templates[31].match(vtmod.normalise_u8(q, *NORM))
    for s in shards:
        s.close()
    single.close()


# --- refusals and default handles -----------------------------------------------------------
def test_setting_is_refused_once_bytes_are_in(vtmod, L):
    lib = L.require_device()
    shape = (32, 32)
    lib_np = library(6, shape, seed=21)
    qs = noisy(lib_np, 4, seed=22)

    def create():
        hd = ctypes.c_void_p()
        L.check(lib.rs_vt_create(32, 32, 8, 0, 64, 0, ctypes.byref(hd)))
        return hd

    def frozen(hd, q):
        idx, score = np.empty(len(q), np.int64), np.empty(len(q), np.uint64)
        L.check(lib.rs_vt_match_batch(hd, len(q), L.ptr(q, ctypes.c_uint8), L.RS_VT_FROZEN,
                                      L.ptr(score, ctypes.c_uint64), L.ptr(idx, ctypes.c_int64), None))
        return idx, score

    hd = create()
    for radius, gain in ((-1, 32), (8, 32), (3, 0), (3, 128), (1, -5)):
        assert lib.rs_vt_set_normalise(hd, radius, gain) == L.RS_ERR_ARG
    L.check(lib.rs_vt_set_normalise(hd, 0, 999))        # off: the gain is ignored
    L.check(lib.rs_vt_set_normalise(hd, 3, 32))
    L.check(lib.rs_vt_set_normalise(hd, 0, 0))          # and off again, while the handle is empty
    L.check(lib.rs_vt_set_normalise(hd, 3, 32))
    # after an add
    L.check(lib.rs_vt_add(hd, 6, L.ptr(lib_np, ctypes.c_uint8), None))
    assert lib.rs_vt_set_normalise(hd, 0, 0) == L.RS_ERR_STATE and b'before' in lib.rs_last_error()
    assert lib.rs_vt_set_normalise(hd, 5, 32) == L.RS_ERR_STATE
    ln, qn = vtmod.normalise_u8(lib_np, *NORM), vtmod.normalise_u8(qs, *NORM)
    want = np.stack([V.vt_scores_library(ln, q) for q in qn])
    idx, score = frozen(hd, qs)
    assert np.array_equal(idx, want.argmin(axis=1)) and np.array_equal(score, want.min(axis=1))
    L.check(lib.rs_vt_destroy(hd))
    # after a staged batch on an empty library
    hd = create()
    idx, score = frozen(hd, qs)
    assert (idx == -1).all()
    assert lib.rs_vt_set_normalise(hd, 3, 32) == L.RS_ERR_STATE
    r, g = ctypes.c_int(-1), ctypes.c_int(-1)
    L.check(lib.rs_vt_normalise(hd, ctypes.byref(r), ctypes.byref(g)))
    assert (r.value, g.value) == (0, 0)
    L.check(lib.rs_vt_add(hd, 6, L.ptr(lib_np, ctypes.c_uint8), None))
    want = np.stack([V.vt_scores_library(lib_np, q) for q in qs])      # still a plain handle
    idx, score = frozen(hd, qs)
    assert np.array_equal(idx, want.argmin(axis=1)) and np.array_equal(score, want.min(axis=1))
    L.check(lib.rs_vt_destroy(hd))
    assert lib.rs_vt_set_normalise(None, 3, 32) == L.RS_ERR_STATE


@pytest.mark.parametrize('shape,metric', [((64, 32), 'wrapped'), ((32, 32), 'sad'), ((24, 10), 'wrapped')])
def test_default_handles_are_plain(vtmod, L, shape, metric):
    lib_np = library(70, shape, seed=23)
    qs = noisy(lib_np, 9, seed=24)
    vts = vtmod.ViewTemplates._from_shape(shape, 45000, metric=metric)
    r, g = ctypes.c_int(-1), ctypes.c_int(-1)
    L.check(vts._lib.rs_vt_normalise(vts._h, ctypes.byref(r), ctypes.byref(g)))
    assert (r.value, g.value) == (0, 0) and vts.normalise is None
    vts.add(lib_np)
    want = np.stack([np_scores(vtmod, metric, lib_np, q) for q in qs])
    idx, score, _ = vts.match_templates(qs, mode=L.RS_VT_FROZEN)
    assert np.array_equal(idx, want.argmin(axis=1)) and np.array_equal(score, want.min(axis=1))
    assert np.array_equal(vts.scores(qs), want)
    assert np.array_equal(read(L, vts._h, 69, shape), lib_np[69])
    vts.close()


# --- the exposure sequence --------------------------------------------------------------------
def test_revisits_under_another_exposure_close_the_loop(vtmod, L):
    """The 16 places of the panorama, stored, then revisited with every grey level moved by 40
    and two-sided noise, frame by frame through match() under 'sad'."""
    frames = C.place_frames()
    rev = C.revisit_frames(frames, 1.0, 40)
    tpl, q = C.ros_templates(frames), C.ros_templates(rev)
    s = C.score_matrix(vtmod.normalise_u8(tpl, *NORM), vtmod.normalise_u8(q, *NORM))
    own, foreign = int(np.diag(s).max()), int(s[~np.eye(16, dtype=bool)].min())
    assert own < foreign
    thr = (own + foreign) // 2

    def run(normalise):
        vts = vtmod.ViewTemplates(**C.ROS, match_threshold=thr, metric='sad', normalise=normalise)
        vts.add(tpl)
        got = [vts.match(f, 1, 2, 3).get_index() for f in rev]
        n = len(vts)
        vts.close()
        return got, n

    def oracle(normalise):
        f = (lambda x: vtmod.normalise_u8(x, *normalise)) if normalise else (lambda x: x)
        idx, _, lib = C.sequence_oracle(f(q), thr, vtmod.numpy_sad_u8_scores, lib=f(tpl))
        return idx, len(lib)

    got, n = run(NORM)
    assert got == list(range(16)) and n == 16
    assert (got, n) == oracle(NORM)
    got, n = run(None)
    assert got != list(range(16)) and n > 16
    assert (got, n) == oracle(None)


# --- the replay ---------------------------------------------------------------------------------
def test_replay_frame_by_frame_and_in_windows(vtmod):
    from pyratslam_amd import replay, synthetic
    events = synthetic.ros_stream(40)
    frames = np.stack([ev[2] for ev in events if ev[0] == 'image'])
    want, _, lib = C.sequence_oracle(vtmod.normalise_u8(C.ros_templates(frames), *NORM), 3000,
                                     vtmod.numpy_sad_u8_scores)
    assert 3 < len(lib) < 30
    res = []
    for window in (1, 8):
        r = replay.RatslamReplay(vt_normalise=NORM, vt_metric='sad', match_threshold=3000, window=window)
        assert r.vts.normalise == NORM and r.vt_normalise == NORM
        r.replay_events(events)
        res.append(r.results())
        r.vts.close()
    assert res[0]['template_index'].tolist() == want == res[1]['template_index'].tolist()
    assert res[0]['templates'] == res[1]['templates'] == len(lib)
    assert np.array_equal(res[0]['pc_max'], res[1]['pc_max'])
    assert np.array_equal(res[0]['em_points'], res[1]['em_points'])
    plain = vtmod.ViewTemplates(**C.ROS, match_threshold=3000, metric='sad')
    with pytest.raises(ValueError, match='vt_normalise'):
        replay.RatslamReplay(vt_normalise=NORM, vt_metric='sad', vts=plain)
    plain.close()
