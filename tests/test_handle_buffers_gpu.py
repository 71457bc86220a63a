"""The handles' device and pinned buffers (rs::DevBuf / rs::PinnedBuf members) through their
growth sites, on a 64 x 32 library of 130 templates (three blocks, the last partial), dense
and with RS_VT_PRUNE=force: one handle's query buffers grown twice by match_batch, its
stream buffers by host and device-resident match_stream, its candidate, matrix and index
buffers by a sequential batch that appends; every index and score against the C oracle for
the library as it stood at that call, and the batch matched before the streams matched
again after them bit for bit (the streams read their own view of the query forms and leave
the batch's alone).  Then every handle kind created and destroyed 20 times (the view
templates' upload stream and its events with it), the timing events of the kinds no other
test times, and a library too large for the device refused with MemoryError, after which a
fresh handle matches."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import view_templates as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, THR = 130, 45000

# RS_VT_PRUNE is the child's environment, as in test_wait_paths_gpu.py
CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from pyratslam_amd import _lib
from pyratslam_amd.view_templates import ViewTemplates
d = np.load(%(inp)r)
h = ViewTemplates._from_shape((64, 32), %(thr)d)
assert h.scan_form() == %(form)r, h.scan_form()
h.add(d['lib'])
out = {}
def keep(name, idx, score):
    out[name + '_idx'], out[name + '_score'] = idx, score
i, s, _ = h.match_templates(d['q300'][:70], mode=0); keep('s1', i, s)
keep('s2', *h.match_stream(d['qs']))
buf = _lib.DeviceBuffer(d['qd'].nbytes).upload(d['qd'])
keep('s3', *h.match_stream((3, 40, buf)))
buf.close()
i, s, _ = h.match_templates(d['q300'][:70], mode=0); keep('s4', i, s)
i, s, _ = h.match_templates(d['q300'], mode=0); keep('s5', i, s)
i, s, n = h.match_templates(d['q20'], mode=1); keep('s6', i, s)
out['s6_new'] = n
out['count'] = np.int64(h.count())
h.close()
np.savez(%(out)r, **out)
'''


@pytest.fixture(scope='module')
def built():
    from pyratslam_amd import _build
    _build.build()


def data():
    lib = V.synthetic_library(T, 64, 32, seed=301)
    q300, _ = V.synthetic_queries(lib, 300, seed=302, hit_frac=0.8)
    qs, _ = V.synthetic_queries(lib, 120, seed=303, hit_frac=0.8)
    qd, _ = V.synthetic_queries(lib, 120, seed=304, hit_frac=0.8)
    q20, _ = V.synthetic_queries(lib, 20, seed=305, hit_frac=0.5)
    return dict(lib=lib, q300=q300, qs=qs.reshape(3, 40, 64, 32), qd=qd.reshape(3, 40, 64, 32), q20=q20)


def oracle_sequential(lib, queries):
    """ViewTemplates.match query by query through the C oracle: (index, score, is_new)."""
    from oracle import c_oracle as C
    lib = list(lib)
    idx, score, new = [], [], []
    for q in queries:
        s, i = C.vt_best(np.stack(lib), q[None])
        miss = float(s[0]) > THR
        idx.append(len(lib) if miss else int(i[0]))
        score.append(int(s[0]))
        new.append(miss)
        if miss:
            lib.append(q)
    return np.array(idx), np.array(score, dtype=np.uint64), np.array(new)


@pytest.mark.parametrize('prune', [None, 'force'], ids=['dense', 'pruned'])
def test_growth_across_capacities_and_the_stream_view(built, tmp_path, prune):
    from oracle import c_oracle as C
    d = data()
    inp, outp = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(inp, **d)
    env = {k: v for k, v in os.environ.items() if k != 'RS_VT_PRUNE'}
    if prune:
        env['RS_VT_PRUNE'] = prune
    # (unset: the pruned form, which prunes only large calls -- these all take the dense launch)
    script = CHILD % {'root': ROOT, 'inp': inp, 'out': outp, 'thr': THR, 'form': 'plane-pruned'}
    subprocess.run([sys.executable, '-c', script], env=env, check=True, timeout=120)
    r = np.load(outp)

    def check(name, queries):
        score, idx = C.vt_best(d['lib'], queries.reshape(-1, 64, 32))
        got_i, got_s = r[name + '_idx'].reshape(-1), r[name + '_score'].reshape(-1)
        print(name, 'mismatches: index', int((got_i != idx).sum()), 'score', int((got_s != score).sum()))
        assert np.array_equal(got_i, idx), name
        assert np.array_equal(got_s, score), name

    check('s1', d['q300'][:70])
    check('s2', d['qs'])
    check('s3', d['qd'])
    check('s4', d['q300'][:70])
    assert np.array_equal(r['s4_idx'], r['s1_idx']) and np.array_equal(r['s4_score'], r['s1_score'])
    check('s5', d['q300'])
    idx, score, new = oracle_sequential(d['lib'], d['q20'])
    assert 0 < new.sum() < len(new)
    assert np.array_equal(r['s6_idx'], idx)
    assert np.array_equal(r['s6_score'], score)
    assert np.array_equal(r['s6_new'], new)
    assert int(r['count']) == T + int(new.sum())


def test_create_and_destroy_every_handle_kind_20_times(built):
    """close() raises unless rs_*_destroy returned RS_OK."""
    import pyratslam_amd.view_templates as vt
    from pyratslam_amd.linked_experience_map import LinkedExperienceMap
    from pyratslam_amd.pose_ensemble import PoseCellEnsemble
    from pyratslam_amd.posecell_network import PoseCellNetwork
    from pyratslam_amd.visual_odometer import SimpleVisualOdometer
    lib = V.synthetic_library(T, 64, 32, seed=301)
    q, _ = V.synthetic_queries(lib, 4, seed=306, hit_frac=1.0)
    # five host batches: upload groups (1, 2, 2), so both upload buffers and every event of the group
    qs, _ = V.synthetic_queries(lib, 20, seed=309, hit_frac=0.8)
    frames = np.random.default_rng(307).integers(0, 256, size=(3, 48, 64), dtype=np.uint8)
    def use_vt(h):                                               # rs_vt
        h.add(lib)
        idx, _, new = h.match_templates(q, mode=0)
        assert not new.any() and idx.shape == (4,)
        want_i, want_s, _ = h.match_templates(qs, mode=0)
        got_i, got_s = h.match_stream(qs.reshape(5, 4, 64, 32))  # ... its upload stream and four events
        assert np.array_equal(got_i.reshape(-1), want_i) and np.array_equal(got_s.reshape(-1), want_s)

    def use_vtf(f):                                              # rs_vtf, made by the first float batch
        fq = q.astype(np.float32)
        fi, _, fn = f.match_templates(fq)
        assert f._vtf is not None and fn[0] and f.count() == int(fn.sum())

    def use_vo(vo):                                              # rs_vo
        assert vo.run(frames).shape == (3, 2)

    def use_pc(pc):                                              # rs_pc
        pc.inject(1.0, (5, 6, 7))
        assert len(pc.update((0.2, 0.01))) == 3

    def use_em(em):                                              # rs_em
        for _ in range(3):
            em.add_experience()
        em.add_link(0, 1, 1.0, 0.5, -0.5)
        em.iterate(1)
        assert em.poses().shape == (3, 3)

    def use_pce(pce):                                            # rs_pce
        pce.inject(1.0, (3, 4, 5))
        assert pce.run([(0.2, 0.01), (0.2, 0.01)]).shape == (2, 2, 3)

    for k in range(20):
        kinds = [(lambda: vt.ViewTemplates._from_shape((64, 32), THR), use_vt),
                 (lambda: vt.ViewTemplates._from_shape((64, 32), 1e9), use_vtf),
                 (SimpleVisualOdometer, use_vo),
                 (lambda: PoseCellNetwork((32, 32, 18), precision='float32' if k % 2 == 0 else 'float64'), use_pc),
                 (lambda: LinkedExperienceMap(capacity=2), use_em),
                 (lambda: PoseCellEnsemble(2, (8, 8, 8)), use_pce)]
        for make, use in kinds:
            if k == 0:      # the first round: a with block closes, and a second close() is no call
                with make() as h:
                    use(h)
                assert h._h is None
                h.close()
            else:
                h = make()
                use(h)
                h.close()


def test_timing_events_of_the_float_library_the_pose_cells_and_the_ensemble(built):
    """With timing on, one call, then a time that is finite and not negative.  (The other three
    kinds: test_view_templates_gpu.py::test_untimed_scans, test_visual_odometer_gpu.py::
    test_timing_is_off_by_default_and_per_call, test_linked_experience_map_gpu.py::
    test_interleaved_calls_keep_their_order.)"""
    import pyratslam_amd.view_templates as vt
    from pyratslam_amd.pose_ensemble import PoseCellEnsemble
    from pyratslam_amd.posecell_network import PoseCellNetwork

    def is_time(ms):
        return np.isfinite(ms) and ms >= 0

    lib = V.synthetic_library(8, 64, 32, seed=310)
    f = vt.ViewTemplates._from_shape((64, 32), 1e9)              # rs_vtf
    f.set_timing(True)
    f.match_templates(lib[:4].astype(np.float32))
    assert f._vtf is not None
    f.match_templates(lib[4:].astype(np.float32))                # (a scan of a library that is not empty)
    print('rs_vtf device_ms', f.device_ms())
    assert is_time(f.device_ms())
    f.close()
    pc = PoseCellNetwork((32, 32, 18))                           # rs_pc: the call's events and the pool's
    pc.inject(1.0, (5, 6, 7))
    pc.set_profiling(True, per_kernel=True)
    assert pc.run([(0.2, 0.01)] * 3).shape == (3, 3)
    print('rs_pc device_ms', pc.device_ms(), 'kernel_ms', pc.kernel_ms())
    assert is_time(pc.device_ms()) and all(is_time(ms) for ms in pc.kernel_ms())
    pc.close()
    pce = PoseCellEnsemble(2, (8, 8, 8))                         # rs_pce
    pce.inject(1.0, (3, 4, 5))
    pce.set_timing(True)
    pce.run([(0.2, 0.01), (0.2, 0.01)])
    print('rs_pce device_ms', pce.device_ms())
    assert is_time(pce.device_ms())
    pce.close()


def test_a_refused_allocation_is_a_memory_error(built):
    """2^40 slots of 2 KiB: refused by the runtime, before any kernel."""
    from oracle import c_oracle as C
    import pyratslam_amd.view_templates as vt
    with pytest.raises(MemoryError):
        vt.ViewTemplates._from_shape((64, 32), THR, capacity=1 << 40)
    lib = V.synthetic_library(T, 64, 32, seed=301)
    q, _ = V.synthetic_queries(lib, 4, seed=308, hit_frac=1.0)
    h = vt.ViewTemplates._from_shape((64, 32), THR)
    h.add(lib)
    idx, score, new = h.match_templates(q, mode=0)
    want_s, want_i = C.vt_best(lib, q)
    assert np.array_equal(idx, want_i) and np.array_equal(score, want_s) and not new.any()
    h.close()
