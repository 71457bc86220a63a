"""The linked experience map on the GPU (rs_em_*): both kernel forms against the NumPy
restatement within 1e-12 (the project's float64 bound; the sides differ in
cos / sin alone), against each other with no tolerance, the poses made on the device, growth
and ordering of the queued calls, and the replay with the GPU map against the NumPy map."""
import ctypes

import numpy as np
import pytest

import _em_graphs as G
from pyratslam_amd import _lib
from pyratslam_amd import linked_experience_map as M

pytestmark = pytest.mark.gpu

TOL = 1e-12
FORMS = ('lds', 'sweep')


def gpu_map(monkeypatch, form=None, **kw):
    """A LinkedExperienceMap with RS_EM_FORM (read at create) set to `form` or unset."""
    if form is None:
        monkeypatch.delenv('RS_EM_FORM', raising=False)
    else:
        monkeypatch.setenv('RS_EM_FORM', form)
    return M.LinkedExperienceMap(**kw)


@pytest.fixture(scope='module')
def references():
    """NumPy results, computed once: {(graph, loops): poses}."""
    out = {}
    for name, make in G.GRAPHS.items():
        poses, links = make()
        p = poses.copy()
        for loops in range(101):
            if loops in (0, 1, 2, 100):
                out[name, loops] = p
            p = M.sweep(p, links)
    return out


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', sorted(G.GRAPHS))
def test_gpu_matches_the_restatement(monkeypatch, references, name, form):
    poses, links = G.GRAPHS[name]()
    for loops in (0, 1, 2, 100):
        em = gpu_map(monkeypatch, form, capacity=8).load(poses, links)
        assert em.form() == form
        em.iterate(loops)
        got = em.poses()
        em.close()
        err = np.abs(got - references[name, loops]).max()
        print('%s %s loops=%d max|d| = %.3g' % (name, form, loops, err))
        assert got.shape == poses.shape and err <= TOL
        if loops == 0:
            assert np.array_equal(got, poses)


@pytest.mark.parametrize('n', [1, 65, 1025, 3072])
def test_lds_equals_sweep(monkeypatch, n):
    poses, links = G.random_graph(n, seed=n)
    deg = np.bincount(links['a'], minlength=n) + np.bincount(links['b'], minlength=n) if n > 1 else np.zeros(1)
    assert n < 65 or (deg.min() == 0 and deg.max() >= 8)
    got = {}
    for form in FORMS:
        em = gpu_map(monkeypatch, form).load(poses, links)
        for loops in (1, 2, 25):      # odd and even counts: the result is what poses() reads
            em.iterate(loops)
        got[form] = em.poses()
        em.close()
    assert np.array_equal(got['lds'], got['sweep'])
    assert np.abs(got['lds'] - M.relax(poses, links, 28)).max() <= TOL


def test_above_the_lds_cap(monkeypatch):
    n = 3073
    poses, links = G.random_graph(n, seed=n)
    em = gpu_map(monkeypatch).load(poses[:768])
    assert em.form() == 'lds'               # the default follows the size: lds up to 768 ...
    em.load(poses[768:769])
    assert em.form() == 'sweep'             # ... sweep above
    em.load(poses[769:], links)
    assert em.form() == 'sweep'
    em.iterate(7)
    got = em.poses()
    em.close()
    assert np.abs(got - M.relax(poses, links, 7)).max() <= TOL
    em = gpu_map(monkeypatch, 'sweep').load(poses, links)
    em.iterate(7)
    assert np.array_equal(em.poses(), got)
    em.close()
    em = gpu_map(monkeypatch, 'lds').load(poses, links)
    with pytest.raises(ValueError):         # a forced lds above its cap is refused
        em.iterate(1)
    assert np.array_equal(em.poses(), poses)
    em.close()
    monkeypatch.setenv('RS_EM_FORM', 'tiles')
    with pytest.raises(ValueError):
        M.LinkedExperienceMap()


@pytest.mark.parametrize('form', FORMS)
def test_device_made_poses_and_growth(monkeypatch, form):
    """Driven from capacity 4: every new pose is made on the device from the relaxed pose
    of `cur` (zero residual on its creating link, checked before any later sweep), and the
    whole history equals the NumPy map's."""
    em = gpu_map(monkeypatch, form, capacity=4, exp_loops=0)
    ref = M.NumpyLinkedExperienceMap(exp_loops=0)
    rng = np.random.default_rng(5)
    for k in range(40):
        t = k if k < 20 else int(rng.integers(0, 20))
        before = em.count
        assert em.on_template(t) == ref.on_template(t)
        if em.count > before and before > 0:    # a pose made on the device just now
            links = em.links()
            assert (links['a'][-1], links['b'][-1]) == (ref.links()['a'][-1], em.count - 1)
            ex, ey, df = M.residuals(em.poses(), links[-1:])
            assert max(abs(ex[0]), abs(ey[0]), abs(df[0])) <= TOL
        em.iterate(10)
        ref.iterate(10)
        v = rng.uniform(0, 0.3), rng.uniform(-0.2, 0.2)
        em.update(*v)
        ref.update(*v)
        assert np.abs(np.subtract(em.get_current_point(), ref.get_current_point())).max() <= TOL
    assert em.count == 20 and np.array_equal(em.links(), ref.links())
    assert np.abs(em.poses() - ref.poses()).max() <= TOL
    em.close()


def test_interleaved_calls_keep_their_order(monkeypatch):
    em = gpu_map(monkeypatch, capacity=4)
    ref = M.NumpyLinkedExperienceMap()
    poses, links = G.ring(40, seed=3)
    for m in (em, ref):
        m.load(poses[:10], links[:9])
        m.iterate(3)
        m.load(poses[10:], links[9:].tolist())   # add behind a relax, across two growths
        first = m.poses()                        # read ...
        m.iterate(5)                             # ... and a relax queued behind the read
        m.set_poses(first[5:8] + 0.25, first=5)  # write behind the relax
        m.iterate(4)
        m.add_link(0, 20, 1.0, 0.5, -0.5)
        m.iterate(1)
        m.iterate(0)
    assert np.abs(em.poses() - ref.poses()).max() <= TOL
    assert np.array_equal(em.links(), ref.links())
    em.set_timing(True)
    em.iterate(2)
    assert em.device_ms() > 0
    em.set_timing(False)
    em.iterate(2)
    assert em.device_ms() == -1.0
    ref.iterate(4)
    assert np.abs(em.poses() - ref.poses()).max() <= TOL
    em.close()
    em.close()


def test_refusals(monkeypatch):
    em = gpu_map(monkeypatch).load(np.zeros((3, 3)), [(0, 1, 1.0, 0.0, 0.0)])
    lib, h = em._lib, em._h
    for a, b in ((0, 3), (-1, 1), (2, 2), (3, 0)):
        assert lib.rs_em_add_link(h, a, b, 1.0, 0.0, 0.0, None) == _lib.RS_ERR_ARG
    assert lib.rs_em_add_experience(h, 3, 1.0, 0.0, 0.0, None) == _lib.RS_ERR_ARG
    assert lib.rs_em_relax(h, -1) == _lib.RS_ERR_ARG
    out = np.zeros((4, 3))
    assert lib.rs_em_read(h, 0, 4, _lib.ptr(out, ctypes.c_double)) == _lib.RS_ERR_ARG
    assert lib.rs_em_read(h, 3, 1, _lib.ptr(out, ctypes.c_double)) == _lib.RS_ERR_ARG
    with pytest.raises(ValueError):
        em.set_poses(np.zeros((2, 3)), first=2)
    with pytest.raises(ValueError):
        M.LinkedExperienceMap(capacity=0)
    assert len(em.links()) == 1 and em.count == 3
    em.close()


# -- replay -------------------------------------------------------------------------
N_REPLAY = 96


@pytest.fixture(scope='module')
def stream():
    from pyratslam_amd import synthetic
    return synthetic.ros_stream(N_REPLAY, seed=4)


@pytest.fixture(scope='module')
def replay_reference(stream):
    """(plain ExperienceMap replay, NumPy linked-map replay), per frame."""
    from pyratslam_amd.replay import RatslamReplay
    plain = RatslamReplay().replay_events(stream)
    ref = RatslamReplay(em=M.NumpyLinkedExperienceMap(exp_loops=20)).replay_events(stream)
    return plain, ref


def same_map(a, b):
    assert a.exp_vt == b.exp_vt and a.current_exp == b.current_exp
    assert np.array_equal(a.links(), b.links())
    assert np.abs(a.poses() - b.poses()).max() <= TOL


def test_replay_with_the_gpu_map(monkeypatch, stream, replay_reference):
    from pyratslam_amd.replay import RatslamReplay
    plain, ref = replay_reference
    r = RatslamReplay(em=gpu_map(monkeypatch, exp_loops=20)).replay_events(stream)
    for other in (plain, ref):      # peaks and template indices do not depend on the map
        assert r.pc_max == other.pc_max and r.template_index == other.template_index
    assert ref.em.count > 1 and len(ref.em.links()) > ref.em.count   # (the stream closes loops)
    same_map(r.em, ref.em)
    assert np.abs(np.array(r.em_points) - np.array(ref.em_points)).max() <= TOL
    r.em.close()


def test_replay_cli_loop_closure(monkeypatch, capsys):
    import json
    from pyratslam_amd import replay
    monkeypatch.delenv('RS_EM_FORM', raising=False)
    assert replay.main(['--synthetic', '24', '--loop-closure', '--exp-loops', '5']) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(out['experiences']) == out['templates'] == len(set(out['template_index']))
    assert len(out['links']) >= out['templates'] - 1 and all(len(l) == 5 for l in out['links'])
    assert len(out['em_points']) == out['updates']
    with pytest.raises(SystemExit):
        replay.main(['--synthetic', '4', '--exp-loops', '5'])


@pytest.mark.parametrize('batch', [64, 7])
def test_camera_only_replay_batched(monkeypatch, stream, batch):
    """replay_frames in batches applies on_template(idx_i), then the step's update, in frame
    order: the same map as the per-frame replay, for the GPU map and the NumPy map."""
    from pyratslam_amd.replay import RatslamReplay
    frames = np.stack([ev[2] for ev in stream if ev[0] == 'image'])[:48]
    runs = {}
    for key, em, b in (('frame', M.NumpyLinkedExperienceMap(exp_loops=10), 1),
                       ('plain', None, batch),
                       ('numpy', M.NumpyLinkedExperienceMap(exp_loops=10), batch),
                       ('gpu', gpu_map(monkeypatch, exp_loops=10), batch)):
        runs[key] = RatslamReplay(use_visual_odometry=True, em=em).replay_frames(frames, batch=b)
    for key in ('plain', 'numpy', 'gpu'):
        assert runs[key].pc_max == runs['frame'].pc_max
        assert runs[key].template_index == runs['frame'].template_index
    same_map(runs['numpy'].em, runs['frame'].em)
    same_map(runs['gpu'].em, runs['frame'].em)
    assert np.abs(np.array(runs['gpu'].em_points) - np.array(runs['frame'].em_points)).max() <= TOL
    runs['gpu'].em.close()
