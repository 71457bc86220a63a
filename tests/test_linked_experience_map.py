"""The linked experience map without a GPU: the library's host rule (rs_em_relax_host, the
kernels' per-experience function and the library's incidence-list builder) against the NumPy
restatement, the summation order, the relaxation's behaviour and on_template's bookkeeping.

Bound: 1e-12 absolute on x, y, th, the project's float64 bound.  The two
sides differ only in cos / sin (libm against NumPy's); moving every cos / sin result by up
to 2 ulp moves the poses of a map 3 units wide by about 1e-15."""
import os
import subprocess

import numpy as np
import pytest

import _em_graphs as G
from conftest import ROOT
from pyratslam_amd import _build, _lib
from pyratslam_amd import linked_experience_map as M

TOL = 1e-12


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def gather_sweep(poses, links, c):
    """The sweep written as a per-experience gather, in plain Python floats."""
    out = poses.copy()
    for i in range(poses.shape[0]):
        frm = [l for l in range(len(links)) if links['a'][l] == i]
        to = [l for l in range(len(links)) if links['b'][l] == i]
        if not frm and not to:
            continue
        s = [0.0, 0.0, 0.0]
        for sign, ids in ((1.0, frm), (-1.0, to)):
            for l in ids:
                a, b = int(links['a'][l]), int(links['b'][l])
                d, h, f = (np.float64(links[k][l]) for k in 'dhf')
                ex = poses[b, 0] - (poses[a, 0] + d * np.cos(poses[a, 2] + h))
                ey = poses[b, 1] - (poses[a, 1] + d * np.sin(poses[a, 2] + h))
                df = M.wrap(poses[b, 2] - (poses[a, 2] + f))
                for k, e in enumerate((ex, ey, df)):
                    s[k] = s[k] + sign * e
        w = np.float64(c) / np.float64(len(frm) + len(to))
        out[i, 0] = poses[i, 0] + w * s[0]
        out[i, 1] = poses[i, 1] + w * s[1]
        out[i, 2] = M.wrap(poses[i, 2] + w * s[2])
    return out


@pytest.mark.parametrize('name', sorted(G.GRAPHS))
@pytest.mark.parametrize('loops', [0, 1, 2, 100])
def test_host_rule_matches_the_restatement(lib, name, loops):
    poses, links = G.GRAPHS[name]()
    want = M.relax(poses, links, loops)
    got = M.relax_host(poses, links, loops)
    err = np.abs(got - want).max()
    print('%s loops=%d max|d| = %.3g' % (name, loops, err))
    assert got.shape == want.shape and err <= TOL
    if loops == 0:
        assert np.array_equal(got, poses)


def test_host_rule_on_random_graphs(lib):
    for n, seed in ((1, 3), (65, 4), (1025, 5)):
        poses, links = G.random_graph(n, seed)
        assert np.abs(M.relax_host(poses, links, 20) - M.relax(poses, links, 20)).max() <= TOL


def test_wrap():
    a = np.array([-6.29, 6.29, np.pi + 1e-9, -np.pi - 1e-9, 0.5, -2 * np.pi, 7 * np.pi + 0.25])
    w = M.wrap(a)
    assert np.all(np.abs(w) <= np.pi + 1e-15)
    assert np.allclose(np.exp(1j * w), np.exp(1j * a), atol=1e-14)
    assert abs(M.wrap(-6.29) - (-6.29 + 2 * np.pi)) < 1e-15   # (clip_rad_180 gives +6.27)
    assert M.wrap(0.5) == 0.5


@pytest.mark.parametrize('name', ['ring', 'hub', 'isolated', 'wrap', 'pair', 'single'])
def test_gather_order_equals_add_at_bit_for_bit(name):
    poses, links = G.GRAPHS[name]() if name != 'ring' else G.ring(40)
    p, q = poses.copy(), poses.copy()
    for _ in range(3):
        p, q = M.sweep(p, links, 0.5), gather_sweep(q, links, 0.5)
        assert np.array_equal(p, q)


def test_isolated_experiences_keep_their_bits(lib):
    poses, links = G.isolated()
    poses[1::2, 2] += 4 * np.pi   # unwrapped headings stay unwrapped
    for r in (M.relax(poses, links, 5), M.relax_host(poses, links, 5)):
        assert np.array_equal(r[1::2], poses[1::2])
        assert not np.array_equal(r[0::2], poses[0::2])


@pytest.fixture(scope='module')
def circle():
    """The circle driven three times without relaxing: (map, residual history of 100 sweeps)."""
    em = G.drive_circle(M.NumpyLinkedExperienceMap(exp_loops=0))
    hist = [em.rms_residual()]
    for _ in range(100):
        em.iterate(1)
        hist.append(em.rms_residual())
    return em, np.array(hist)


def test_circle_closure_is_one_link(circle):
    em, _ = circle
    links = em.links()
    assert em.count == 200 and len(links) == 200
    assert (links['a'][-1], links['b'][-1]) == (199, 0)
    assert np.array_equal(links['a'][:-1], np.arange(199)) and np.array_equal(links['b'][:-1], np.arange(1, 200))


def test_relaxation_reduces_the_residuals(circle):
    _, hist = circle
    print('position rms %.4f -> %.4f, heading rms %.4f -> %.4f' % (hist[0, 0], hist[-1, 0], hist[0, 1], hist[-1, 1]))
    assert hist[-1, 0] * 2 < hist[0, 0]
    assert hist[-1, 1] * 2 < hist[0, 1]
    assert np.all(np.diff(hist[:, 1]) <= 0)   # the heading residual never rises


def test_chain_without_closure_does_not_move():
    em = G.drive_circle(M.NumpyLinkedExperienceMap(exp_loops=0), laps=1, places=200)
    assert len(em.links()) == 199
    before = em.poses()
    em.iterate(100)
    assert np.abs(em.poses() - before).max() < 1e-12


def test_new_experience_has_zero_residual_on_its_link():
    em = M.NumpyLinkedExperienceMap()
    rng = np.random.default_rng(7)
    for k in range(30):
        em.on_template(k % 20 if k < 25 else int(rng.integers(0, 20)))
        em.update(rng.uniform(0, 0.3), rng.uniform(-0.2, 0.2))
    em2 = M.NumpyLinkedExperienceMap(exp_loops=0)
    em2.on_template(0)
    em2.update(0.3, 0.1)
    em2.update(0.2, -0.3)
    em2.on_template(1)
    ex, ey, df = M.residuals(em2.poses(), em2.links())
    assert max(abs(ex[0]), abs(ey[0]), abs(df[0])) < 1e-15
    assert em.count == 20


# -- on_template bookkeeping -------------------------------------------------------
def test_on_template_cases():
    em = M.NumpyLinkedExperienceMap(exp_loops=0)
    em.update(0.5, 0.2)                       # motion before the first frame
    assert em.get_current_point() == (float(em.accum_delta_x), float(em.accum_delta_y))
    assert em.on_template(7) == 0             # unseen, empty map: the origin, heading ath
    assert np.array_equal(em.poses(), [[0.0, 0.0, 0.2]])
    assert em.current_exp == 0 and em.accum_delta_x == 0 and em.accum_delta_y == 0
    assert em.theta_current == em.accum_delta_th == np.float64(0.2)
    assert len(em.links()) == 0

    em.update(1.0, 0.3)
    assert em.on_template(7) == 0             # e == cur: nothing, the accumulators keep running
    assert em.count == 1 and len(em.links()) == 0 and em.accum_delta_x != 0
    em.update(1.0, 0.0)
    ax, ay, ath = em.accum_delta_x, em.accum_delta_y, em.accum_delta_th
    d, h, f = em.measurement()
    assert d == float(np.sqrt(ax * ax + ay * ay))
    assert h == float(M.wrap(np.arctan2(ay, ax) - np.float64(0.2))) and f == float(M.wrap(ath - np.float64(0.2)))

    assert em.on_template(3) == 1             # unseen: a new experience and the link cur -> new
    assert em.links().tolist() == [(0, 1, d, h, f)]
    assert np.array_equal(em.poses()[1], M.place([0.0, 0.0, 0.2], d, h, f))
    assert em.current_exp == 1 and em.accum_delta_x == 0 and em.accum_delta_y == 0
    assert em.theta_current == ath and em.accum_delta_th == ath   # ath is never reset

    em.update(0.4, -0.1)
    assert em.on_template(7) == 0             # seen, e != cur: the link cur -> e
    assert [(l[0], l[1]) for l in em.links().tolist()] == [(0, 1), (1, 0)]
    assert em.current_exp == 0 and em.accum_delta_x == 0
    em.update(0.4, 0.1)
    assert em.on_template(3) == 1             # the link 0 -> 1 exists: refused, cur still moves
    assert len(em.links()) == 2 and em.current_exp == 1 and em.accum_delta_x == 0
    assert em.exp_vt == [7, 3] and em.vt_exp == {7: 0, 3: 1}
    assert em.get_points() == [tuple(p[:2]) for p in em.poses().tolist()]


def test_current_point_turns_into_the_relaxed_heading():
    em = M.NumpyLinkedExperienceMap(exp_loops=0)
    em.on_template(0)
    em.update(1.0, 0.0)
    assert em.get_current_point() == (1.0, 0.0)
    em.set_poses([[2.0, 3.0, np.pi / 2]])     # the experience was relaxed a quarter turn
    x, y = em.get_current_point()
    assert abs(x - 2.0) < 1e-15 and abs(y - 4.0) < 1e-15


def test_refusals(lib):
    em = M.NumpyLinkedExperienceMap()
    em.load(np.zeros((3, 3)), [(0, 1, 1.0, 0.0, 0.0)])
    for a, b in ((0, 3), (-1, 1), (1, 1), (0, 1)):
        with pytest.raises(ValueError):
            em.add_link(a, b, 1.0, 0.0, 0.0)
    assert len(em.links()) == 1
    em.add_link(1, 0, 1.0, 0.0, 0.0)          # the reverse link is another link
    with pytest.raises(ValueError):
        em.on_template(-1)
    with pytest.raises(ValueError):
        em.add_experience(3)
    with pytest.raises(ValueError):
        em.set_poses(np.zeros((2, 3)), first=2)
    for kw in ({'exp_loops': -1}, {'exp_correction': 0.0}, {'exp_correction': 1.5}):
        with pytest.raises(ValueError):
            M.NumpyLinkedExperienceMap(**kw)
    p = np.zeros((2, 3))
    for bad in ([(0, 2, 1.0, 0.0, 0.0)], [(-1, 0, 1.0, 0.0, 0.0)], [(1, 1, 1.0, 0.0, 0.0)]):
        with pytest.raises(ValueError):
            M.relax_host(p, bad, 1)
    with pytest.raises(ValueError):
        M.relax_host(p, [], -1)


def test_no_cpu_fallback_without_device(lib):
    if lib.rs_device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(_lib.HipLibraryError):
        M.LinkedExperienceMap()


def test_replay_calls_on_template_only_where_the_map_has_it():
    from pyratslam_amd.experience_map import ExperienceMap
    from pyratslam_amd.replay import RatslamReplay

    class Match:
        def __init__(self, i):
            self.i = i

        def get_index(self):
            return self.i

    class Vts:
        templates = []

        def __init__(self, seq):
            self.seq = list(seq)

        def match(self, **kw):
            return Match(self.seq.pop(0))

    class Pcn:
        def inject(self, *a):
            pass

        def get_pc_max(self):
            return (1, 2, 3)

        def update(self, v):
            pass

    seq = [0, 1, 1, 0, 2]
    maps = [M.NumpyLinkedExperienceMap(), ExperienceMap()]
    for em in maps:
        r = RatslamReplay(pcn=Pcn(), vts=Vts(seq), em=em, batch=False)
        for k in seq:
            r.vis_callback(None)
            r.update_posecells(0.2, 0.1)
        assert r.template_index == seq and len(r.em_points) == len(seq)
    assert maps[0].exp_vt == [0, 1, 2]
    assert [(l[0], l[1]) for l in maps[0].links().tolist()] == [(0, 1), (1, 0), (0, 2)]
    assert len(maps[1].experiences) == len(seq)


# -- the host rule and the incidence builder under sanitizers ------------------------
@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason='hipcc absent')
def test_host_rule_and_incidence_builder_under_sanitizers(tmp_path):
    """tests/em_host_main.cpp with experience_map.hip and rs_common.cpp, the host side built
    with -fsanitize=address,undefined, run as a child process on the CPU (it makes no device
    call).  The sanitizer is linked into the program; nothing is preloaded."""
    exe = str(tmp_path / 'em_host')
    csrc = os.path.join(ROOT, 'pyratslam_amd', 'csrc')
    san = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined']
    subprocess.check_call([_build.HIPCC, '--offload-arch=' + _build.ARCH, '-O1', '-g', '-std=c++17',
                           '-ffp-contract=off', *san, '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
                           '-x', 'hip', os.path.join(csrc, 'experience_map.hip'),
                           os.path.join(csrc, 'rs_common.cpp'),
                           os.path.join(ROOT, 'tests', 'em_host_main.cpp'),
                           '-fsanitize=address,undefined', '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
