"""Pins the spectra's oracle (tests/spectrum_ref.py) against independent statements: a plane of the mesh is the maps'
slice through that plane, Parseval, the mode count, and a field whose spectrum is known.  No GPU, no library."""
import numpy as np
import pytest

import map_ref as mr
import spectrum_ref as sr

UNIT = [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]
K = mr.kernel_constant()


@pytest.fixture(scope="module")
def cloud():
    pos, h, m = sr.lattice(16)
    return pos, h, m, sr.shear_velocity(pos)


@pytest.fixture(scope="module")
def meshes(cloud):
    pos, h, m, v = cloud
    return {n: sr.mesh(pos, h, m, UNIT, n, K=K, a=v) for n in (16, 32)}


@pytest.mark.parametrize("n", [16, 32])
def test_mesh_plane_is_the_maps_slice(cloud, meshes, n):
    pos, h, m, v = cloud
    assert float(h.min()) >= 0.5 / n  # no clamp: the slice does not clamp its h
    worst = 0.0
    for iz in (0, n // 3, n - 1):
        zc = (iz + 0.5) / n
        ref = mr.render(pos, h, m, UNIT, [1, 1, 1], mr.SLICE, 2, [0.5, 0.5, zc], [1.0, 1.0], [n, n], K=K, a=v[:, 0])
        for got, want in ((meshes[n]["sum0"][iz], ref["sum0"]), (meshes[n]["sum1"][0][iz], ref["sum1"])):
            scale = ref["sum0"] if want is ref["sum0"] else ref["abs1"]
            assert (scale > 0).all()
            worst = max(worst, float((np.abs(got - want) / scale).max()))
        assert np.array_equal(meshes[n]["count"][iz], ref["count"])
    print("n = %d: max relative difference to the slice %.2e" % (n, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("weight", [0, 1, 2])
def test_parseval(meshes, n, weight):
    W = sr.field(meshes[n]["sum0"], meshes[n]["sum1"], weight)
    power, modes = sr.spectrum(W, n, prefactor=0.5)
    want = 0.5 * float((W ** 2).sum()) / n ** 3
    print("n = %d, weight %d: Parseval to %.2e" % (n, weight, abs(power.sum() - want) / want))
    assert abs(power.sum() - want) <= 1e-12 * want
    # W_x + i W_y as one complex field gives the same shell sums
    packed, _ = sr.spectrum([W[0] + 1j * W[1], W[2]], n, prefactor=0.5)
    assert np.abs(packed - power).max() <= 1e-12 * power.max()


@pytest.mark.parametrize("n", [16, 32, 64, 128, 256])
def test_modes_add_up(n):
    s, modes = sr.shells(n)
    assert int(modes.sum()) == n ** 3 and modes.size == sr.num_shells(n) == int(s.max()) + 1
    assert modes[0] == 1 and modes[1] == 6 + 12 and (modes > 0).all()  # shell 1: |n|^2 = 1 and 2


@pytest.mark.parametrize("n", [16, 32])
def test_known_field(meshes, n):
    """0.7 sin(2 pi 3 y) x^ + 0.35 cos(2 pi 2 x) z^: shells 3 and 2 hold nearly all of the power"""
    W = sr.field(meshes[n]["sum0"], meshes[n]["sum1"], 0)
    power, _ = sr.spectrum(W, n, prefactor=0.5)
    order = np.argsort(power)[::-1]
    print("n = %d: shells 2 and 3 hold %.4f of the power" % (n, (power[2] + power[3]) / power.sum()))
    assert sorted(order[:2].tolist()) == [2, 3]
