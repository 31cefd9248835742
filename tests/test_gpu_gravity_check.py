"""The force-error check inside sx_sim (sx_sim_set_gravity_check / sx_sim_gravity_check): the armed step walks a sample
of its own target blocks once more and sums them directly (sx_gravity_direct); the figures are
|a_walk - a_direct| / |a_direct| over the sample.

Bounds: with a theta at which the walk opens every node the two sides are the same sum, each within the fast variant's
1e-5 of it (tests/test_gpu_direct.py; the walk's fast P2P is the same arithmetic), so 2e-5; at theta = 0.5 the median
is below the 1e-2 that tests/test_oracle_gravity.py asks of the oracle's walk.
"""
import numpy as np
import pytest

import sphexa_amd as sx
from sphexa_amd import ic

pytestmark = pytest.mark.gpu

FIELDS = ["id", "x", "y", "z", "h", "m", "temp", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "du_m1", "alpha", "ax", "ay",
          "az", "du", "nc"]


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def evrard_sim(ctx, theta, **kw):
    f, lim, bnd, dt0 = ic.evrard(14)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), params=sx.default_params(g=1.0, theta=theta, **kw))
    sim.set_state(f, dt0, dt0)
    return sim


def periodic_sim(ctx, theta):
    """a 12^3 lattice in the periodic unit cube, the masses modulated along x"""
    f, lim, bnd, dt0 = ic.turbulence(12)
    assert bnd == [1, 1, 1] and lim[1] - lim[0] == 1.0
    f["m"] = (f["m"] * (1.0 + 0.3 * np.sin(2.0 * np.pi * f["x"]))).astype(np.float32)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), params=sx.default_params(g=1.0, theta=theta))
    sim.set_state(f, dt0, dt0)
    return sim


def checked_step(sim, targets):
    sim.set_gravity_check(targets)
    sim.step()
    return sim.gravity_check()


def test_tiny_theta_reproduces_the_direct_sum_open_box(ctx):
    sim = evrard_sim(ctx, 0.01)
    try:
        n = sim.size()
        c = checked_step(sim, n)  # every block
        print("open box, theta 0.01:", c)
        assert c["targets"] == n
        assert c["max"] <= 2e-5
        assert c["mean"] <= c["max"] and c["median"] <= c["p99"] <= c["max"]
    finally:
        sim.close()


def test_tiny_theta_reproduces_the_direct_sum_periodic_box(ctx):
    sim = periodic_sim(ctx, 0.01)
    try:
        c = checked_step(sim, sim.size())
        print("periodic box, theta 0.01:", c)
        assert c["targets"] == sim.size()
        assert c["rms"] <= 2e-5
    finally:
        sim.close()


def test_error_rises_with_theta(ctx):
    med = []
    for theta in (0.3, 0.5, 0.9):
        sim = evrard_sim(ctx, theta)
        try:
            c = checked_step(sim, 512)
            print("theta", theta, c)
            assert 256 <= c["targets"] <= 768  # about 512, in whole 64-particle blocks
            med.append(c["median"])
        finally:
            sim.close()
    assert med[0] < med[1] < med[2]
    assert med[1] < 1e-2


@pytest.mark.parametrize("std", [False, True], ids=["ve", "std"])
def test_the_check_does_not_change_the_step(ctx, std):
    out = []
    for armed in (False, True):
        sim = evrard_sim(ctx, 0.5, std=std)
        try:
            for k in range(3):
                if armed and k == 1:
                    sim.set_gravity_check(256)
                sim.step()
            if armed:
                assert sim.gravity_check()["targets"] > 0
            out.append((sim.get(FIELDS), sim.scalars()))
        finally:
            sim.close()
    for k in FIELDS:
        assert out[0][0][k].tobytes() == out[1][0][k].tobytes(), k
    assert out[0][1] == out[1][1]


def test_reading_and_refusals(ctx):
    sim = evrard_sim(ctx, 0.5)
    try:
        with pytest.raises(sx.SxError, match="no armed step"):
            sim.gravity_check()
        sim.set_gravity_check(128)
        sim.set_gravity_check(0)  # disarmed again
        sim.step()
        with pytest.raises(sx.SxError, match="no armed step"):
            sim.gravity_check()
        # a communicator: refused before it is used (a NULL one suffices)
        sim.set_gravity_check(128)
        assert sim.L.sx_sim_set_comm(sim.h, None) == sx.SX_ERR_ARG
        assert b"one rank" in sim.L.sx_last_error(ctx.h)
        sim.step()
        assert sim.gravity_check()["targets"] > 0
    finally:
        sim.close()
    bdt = evrard_sim(ctx, 0.5, bdt=True)
    try:
        with pytest.raises(sx.SxError, match="ve-bdt"):
            bdt.set_gravity_check(128)
    finally:
        bdt.close()
    f, lim, bnd, dt0 = ic.evrard(14)
    nograv = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd))
    try:
        with pytest.raises(sx.SxError, match="no self-gravity"):
            nograv.set_gravity_check(128)
    finally:
        nograv.close()
