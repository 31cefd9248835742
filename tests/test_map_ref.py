"""The map oracle (tests/map_ref.py) against what the maps must satisfy analytically: a column map integrates to the
mass, a slice through a particle's centre reads m K / h^3 there."""
import numpy as np

import map_ref as mr

UNIT = [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]


def test_one_particle_column_integrates_to_its_mass():
    K = mr.kernel_constant()
    r = mr.render(np.array([[0.5, 0.5, 0.5]]), [0.05], [3.0], UNIT, [0, 0, 0], mr.COLUMN, 2, [0.5, 0.5, 0.5], [0.4, 0.4],
                  [200, 200], K=K)
    total = r["sum0"].sum() * (0.4 / 200) ** 2
    assert abs(total - 3.0) < 1e-6 * 3.0, total
    assert r["count"].max() == 1 and r["count"].sum() > 0


def test_line_of_sight_kernel_is_normalised():
    """K int Y 2 pi q dq = 1, and Y(0) is the value the issue states"""
    K = mr.kernel_constant()
    xq, wq = np.polynomial.legendre.leggauss(400)
    q = 1.0 + xq
    assert abs(K * np.sum(wq * mr.kernel_y(q * q) * 2.0 * np.pi * q) - 1.0) < 1e-10
    assert abs(mr.kernel_y(np.array([0.0]))[0] - 1.09986220787) < 1e-10
    assert mr.kernel_y(np.array([4.0, 5.0])).tolist() == [0.0, 0.0]


def test_slice_through_a_particle_centre():
    K = mr.kernel_constant()
    h, m = 0.07, 2.5
    # an odd number of pixels: the middle pixel's centre is the particle
    # axis 0: u = y, v = z; the window is centred on (y, z) = (0.6, 0.45), the plane is x = center[0]
    r = mr.render(np.array([[0.3, 0.6, 0.45]]), [h], [m], UNIT, [0, 0, 0], mr.SLICE, 0, [0.3, 0.6, 0.45], [0.2, 0.2],
                  [21, 21], K=K)
    assert abs(r["sum0"][10, 10] - m * K / h ** 3) < 1e-12 * m * K / h ** 3
    assert r["sum0"].max() == r["sum0"][10, 10]


def test_periodic_column_map_conserves_mass():
    """2000 uniform random particles in the periodic unit box, h in [0.06, 0.078], 32 x 32 full-box column map:
    sum S0 du dv = sum m within 1e-5 (measured: 2e-8 at this shape, 5e-7 at h ~ 0.03 / 48^2, 3e-7 at 300 particles /
    h ~ 0.1 / 16^2).  A condition on resolved particles only: where h is clamped to half a pixel the pixel sum is a
    coarse quadrature of the particle's disc (h = 0.01 at 32^2 gives 1.8e-3), so it is not asserted there."""
    rng = np.random.default_rng(7)
    n = 2000
    pos = rng.random((n, 3))
    h = rng.uniform(0.06, 0.078, n)
    m = rng.uniform(0.5, 1.5, n) / n
    r = mr.render(pos, h, m, UNIT, [1, 1, 1], mr.COLUMN, 2, [0.5, 0.5, 0.5], [1.0, 1.0], [32, 32])
    total = r["sum0"].sum() / 32 ** 2
    print("mass defect", abs(total - m.sum()) / m.sum())
    assert abs(total - m.sum()) <= 1e-5 * m.sum()
