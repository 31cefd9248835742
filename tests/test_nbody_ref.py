"""The CPU composition of the NbodyProp step (tests/nbody_ref.py), its fixture and the Plummer initial condition.

* the composition through oracle/_ref (the reference's own functions) and through the restatement
  (libsphexa_oracle.so) give the same 20 steps from po.evrard_state(14), bit for bit (skipped without _ref);
* tests/golden/nbody_evrard14.npz (tests/gen_nbody_golden.py, written from the _ref run) equals a fresh composition
  through the restatement, which needs no _ref;
* egrav is the one exception to "bit for bit": both libraries sum it in an OpenMP reduction whose order depends on the
  thread schedule, so two runs of the SAME library differ in its last bits (measured: up to 3.3e-16 absolute on
  -0.59; with one thread the two libraries agree bit for bit).  It, and the total energy formed from it, are held to
  rel 1e-12, the bound tests/test_oracle_gravity.py already uses for this sum; no field and no other scalar depends
  on egrav;
* ic.plummer: zero centre of mass and momentum to rounding, virial ratio within the sampling spread.
"""
import numpy as np
import pytest

import gen_nbody_golden as gg
import pyoracle as po
from sphexa_amd import ic


def same(a, b):
    """equality of two compositions: bit for bit, but egrav and the total energy (see above)"""
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "series_egrav":
            assert np.allclose(a[k], b[k], rtol=1e-12, atol=0), k
        elif k == "final_scalars":  # minDt, minDt_m1, ttot, egrav, ekin, etot
            assert np.array_equal(a[k][[0, 1, 2, 4]], b[k][[0, 1, 2, 4]]), k
            assert np.allclose(a[k][[3, 5]], b[k][[3, 5]], rtol=1e-12, atol=0), k
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def fresh():
    return gg.compose(po.load_oracle())


@pytest.mark.ref
@pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref not built")
def test_composition_ref_equals_oracle(fresh):
    same(gg.compose(po.load_ref()), fresh)


def test_fixture_equals_fresh_composition(fresh):
    with np.load(gg.PATH) as d:
        same({k: d[k] for k in d.files}, fresh)
    assert fresh["series_dt"].size == gg.STEPS


def _virial(f):
    """2T / |W| with the unsoftened pair potential, numpy doubles"""
    X = np.stack([f[k] for k in "xyz"], 1)
    V = np.stack([f["v" + k].astype(np.float64) for k in "xyz"], 1)
    m = f["m"].astype(np.float64)
    T = 0.5 * np.sum(m * np.sum(V * V, 1))
    iu = np.triu_indices(m.size, 1)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))[iu]
    W = -np.sum((m[:, None] * m[None, :])[iu] / d)
    return 2.0 * T / abs(W)


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_plummer(seed):
    n = 512
    f, lim, bnd, dt0 = ic.plummer(n, seed)
    assert sorted(f) == sorted(["x", "y", "z", "h", "m", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "id"])
    assert all(f[k].size == n for k in f) and bnd == [0, 0, 0]
    assert np.all(f["m"] == np.float32(1.0 / n)) and np.all(f["h"] == f["h"][0]) and f["h"][0] > 0
    m = f["m"].astype(np.float64)
    for k in "xyz":
        # the centre of mass is removed in double: what is left is the rounding of n additions of values below rmax
        assert abs(np.sum(m * f[k])) <= n * 2.0 ** -52 * np.max(np.abs(f[k]))
        # the velocities are stored as floats: each carries at most half an ulp of the largest, 2^-24 max|v|
        v = f["v" + k].astype(np.float64)
        assert abs(np.sum(m * v)) <= 2.0 ** -24 * np.max(np.abs(v))
        assert np.array_equal(f[k + "_m1"], (v * dt0).astype(np.float32))
        assert np.all(np.abs(f[k]) < lim[1])
    # 2T/|W| at n = 512 over the seeds 0..19: mean 0.984, standard deviation 0.040 (min 0.887, max 1.047; the
    # truncation at 8 scale radii removes the most weakly bound tail).  Three standard deviations around that mean.
    q = _virial(f)
    assert abs(q - 0.984) < 3 * 0.040, q
