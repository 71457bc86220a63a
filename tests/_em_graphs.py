"""Graphs shared by test_linked_experience_map.py and test_linked_experience_map_gpu.py:
each builder returns ``(poses (n, 3) float64, links LINK_DTYPE array)``."""
import numpy as np

from pyratslam_amd import linked_experience_map as M


def measure(pa, pb):
    """The exact measurement (d, h, f) of pose ``pb`` from pose ``pa``."""
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return (float(np.hypot(dx, dy)), float(M.wrap(np.arctan2(dy, dx) - pa[2])), float(M.wrap(pb[2] - pa[2])))


def ring(n=200, seed=0, radius=3.0):
    """A chain of n experiences on a circle closed by the one link n-1 -> 0: exact
    measurements, poses off by N(0, 0.02)."""
    rng = np.random.default_rng(seed)
    ang = np.arange(n) * 2 * np.pi / n
    truth = np.stack([radius * np.cos(ang), radius * np.sin(ang), M.wrap(ang + np.pi / 2)], axis=1)
    links = [(i, (i + 1) % n) + measure(truth[i], truth[(i + 1) % n]) for i in range(n)]
    return truth + rng.normal(0, 0.02, truth.shape), M.as_links(links)


def single():
    return np.array([[0.25, -1.5, 0.75]]), M.as_links([])


def pair():
    return np.array([[0.0, 0.0, 0.1], [1.1, 0.2, -0.4]]), M.as_links([(0, 1, 1.0, 0.05, -0.3)])


def hub(degree=300, seed=1):
    """Experience 0 linked with `degree` others, every other link pointing at the hub."""
    rng = np.random.default_rng(seed)
    n = degree + 1
    poses = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], axis=1)
    links = []
    for i in range(1, n):
        a, b = (0, i) if i % 2 else (i, 0)
        d, h, f = measure(poses[a], poses[b])
        links.append((a, b, d * 1.01, h + 0.01, f - 0.01))
    return poses, M.as_links(links)


def isolated(n=50, seed=2):
    """Links among the even experiences only; the odd ones have none."""
    rng = np.random.default_rng(seed)
    poses = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], axis=1)
    links = []
    for i in range(0, n - 2, 2):
        links.append((i, i + 2) + tuple(rng.uniform(-1, 1, 3)))
    links.append((n - 2 if n % 2 == 0 else n - 1, 0) + tuple(rng.uniform(-1, 1, 3)))
    return poses, M.as_links(links)


def wrap_case(eps=1e-9):
    """Pairs whose heading difference th_b - (th_a + f) lies just beyond and just short of
    +-2pi and +-pi (the poses are not wrapped), chained so every sweep mixes them."""
    diffs = [s * t + e for t in (2 * np.pi, np.pi) for s in (1, -1) for e in (eps, -eps)]
    poses, links = [], []
    for k, df in enumerate(diffs):
        tha, f = 0.3 * k - 1.0, 0.2
        poses += [[float(k), 0.0, tha], [float(k) + 0.5, 0.25, tha + f + df]]
        links.append((2 * k, 2 * k + 1, 0.5, 0.1, f))
        if k:
            links.append((2 * k - 1, 2 * k, 0.6, -0.2, 0.05))
    return np.array(poses), M.as_links(links)


def random_graph(n, seed, max_degree=8):
    """n experiences with random links of degree 0 .. max_degree (up to max_degree / 2 drawn
    from each experience, none to one that is full), no self-links, no duplicate (a, b)."""
    rng = np.random.default_rng(seed)
    poses = np.concatenate([rng.uniform(-5, 5, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], axis=1)
    links, seen, deg = [], set(), [0] * n
    if n > 1:
        for a in range(n):
            for _ in range(int(rng.integers(0, max_degree // 2 + 1))):
                b = int(rng.integers(0, n))
                if b == a or (a, b) in seen or max(deg[a], deg[b]) >= max_degree:
                    continue
                seen.add((a, b))
                deg[a] += 1
                deg[b] += 1
                links.append((a, b, float(rng.uniform(0, 2)), float(rng.uniform(-np.pi, np.pi)),
                              float(rng.uniform(-np.pi, np.pi))))
    return poses, M.as_links(links)


GRAPHS = {'ring': ring, 'single': single, 'pair': pair, 'hub': hub, 'isolated': isolated,
          'wrap': wrap_case}


def drive_circle(em, laps=3, places=200, step=0.1, dist_drift=0.002, head_drift=0.01):
    """Drive `laps` times round a circle of `places` view templates with drifting
    odometry (distance and heading scaled up by the drifts): on_template, then the step."""
    turn = 2 * np.pi / places
    for k in range(laps * places):
        em.on_template(k % places)
        em.update(step * (1 + dist_drift), turn * (1 + head_drift))
    return em
