"""sx_cool and sx_cooling_time on the device against the float64 oracle (cooling_ref.py), on its shared inputs: the wave
and block tails, more than one block of partials, temperatures on every node, below the floor and above T_N, six decades
of rho, and per input one call that cools by nothing, one by 1e-15 .. 1e-7 of T, a moderate one and one that sends the
dense particles to the floor.

Tolerance: the kernels run the oracle's operations in the oracle's order (-ffp-contract=off); what differs is the
device's log, exp, log1p and expm1, a few ulp where glibc's are under one.  The integration amplifies such a rounding
exactly as it amplifies the oracle's own, whose sum is eps_ref = max |T64 - T_mp| / T_old, measured here against mpmath
on the same inputs (floored at 4 * 2^-52): |T_gpu - T64| <= 16 eps_ref T_old.
"""
import math

import numpy as np
import pytest

import cooling_ref as cr
import sphexa_amd as sx
from sphexa_amd import cooling

pytestmark = pytest.mark.gpu

MARGIN = 16.0


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table():
    c = cooling.Cooling(cr.GPU_T, cr.GPU_L)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference():
    ref = cr.gpu_reference(0)
    eps = max(ref["eps_ref"], cr.eps_floor())
    print("eps_ref = %.3e, tolerance %.3e T_old" % (ref["eps_ref"], MARGIN * eps))
    return ref, eps


def run_cool(ctx, table, c, cv, dt):
    rho, m, temp = ctx.upload(c["rho"]), ctx.upload(c["m"]), ctx.upload(c["temp"])
    try:
        stats = cooling.cool(ctx, table, rho, m, temp, cv, dt)
        return temp.get(), stats
    finally:
        for d in (rho, m, temp):
            ctx.free(d)


@pytest.mark.parametrize("n", cr.GPU_SIZES)
def test_cool(ctx, table, reference, n):
    ref, eps = reference
    cases = cr.gpu_cases(0)
    c, cv, T1 = cases[n], cases["cv"], cr.GPU_T[0]
    T_old = c["temp"]
    above = T_old >= T1
    worst = 0.0
    for dt in cases["dts"]:
        T64, terms, _ = ref[(n, dt)]
        T, stats = run_cool(ctx, table, c, cv, dt)
        # the exact properties
        assert np.all(T <= T_old), dt
        assert np.all(T[above] >= T1), dt
        assert np.array_equal(T[~above], T_old[~above]), dt
        if dt == 0.0:
            assert np.array_equal(T, T_old)
            assert stats["radiated"] == 0.0
        # against the oracle
        ratio = np.max(np.abs(T - T64) / (eps * T_old))
        worst = max(worst, ratio)
        print("n = %d dt = %g: max |T_gpu - T64| / (eps_ref T_old) = %.3f" % (n, dt, ratio))
        assert ratio <= MARGIN, (n, dt, ratio)
        assert stats["cooled"] == int(above.sum())
        assert stats["on_floor"] == int(np.sum(above & (T == T1)))
        # the energy: one rounding per term, then a double sum in a fixed order
        mine = (c["m"].astype(np.float64) * cv) * (T_old - T)
        mine = np.where(above, mine, 0.0)
        exact = math.fsum(mine)
        bound = (n + 1) * 2.0 ** -53 * math.fsum(np.abs(mine))
        assert abs(stats["radiated"] - exact) <= bound, (n, dt, stats["radiated"], exact, bound)
        # the same bits on a second run
        T2, stats2 = run_cool(ctx, table, c, cv, dt)
        assert np.array_equal(T2, T)
        assert np.float64(stats2["radiated"]).tobytes() == np.float64(stats["radiated"]).tobytes()
    if n == 4099:
        assert any(ref[(n, dt)][0][above].min() == T1 for dt in cases["dts"])  # some reach the floor
        rel = (T_old - ref[(n, 1e-10)][0])[above] / T_old[above]
        assert np.any((rel > 0) & (rel < 1e-11))  # and some cool by next to nothing: the cancellation case
    print("n = %d: worst ratio %.3f of %.0f" % (n, worst, MARGIN))


@pytest.mark.parametrize("n", cr.GPU_SIZES)
def test_cooling_time(ctx, table, reference, n):
    _, eps = reference
    cases = cr.gpu_cases(0)
    c, cv = cases[n], cases["cv"]
    rho, temp = ctx.upload(c["rho"]), ctx.upload(c["temp"])
    try:
        got = cooling.cooling_time(ctx, table, rho, temp, cv)
    finally:
        ctx.free(rho), ctx.free(temp)
    want = cr.cooling_time64(cases["table"], c["temp"], c["rho"], cv).min()
    print("n = %d: min t_cool %.17g, oracle %.17g, ratio %.3f" % (n, got, want, abs(got - want) / (eps * want)))
    assert math.isfinite(want) and abs(got - want) <= MARGIN * eps * want


def test_cooling_time_below_the_floor(ctx, table):
    n = 300
    rho = ctx.upload(np.full(n, 2.0, np.float32))
    temp = ctx.upload(np.linspace(0.01, 0.999, n))
    try:
        assert cooling.cooling_time(ctx, table, rho, temp, 1.25) == math.inf
        # and one particle on the floor itself cools: L(T_1) = L_1
        t = np.linspace(0.01, 0.999, n)
        t[137] = 1.0
        temp.set(t)
        assert cooling.cooling_time(ctx, table, rho, temp, 1.25) == pytest.approx(1.25 * 1.0 / (2.0 * 0.5), rel=1e-15)
    finally:
        ctx.free(rho), ctx.free(temp)


def test_kernel_times_and_a_changed_table(ctx, table):
    """the events of sx_set_cooling_timing; and a second table between two calls is uploaded, the first again after it"""
    c, cv = cr.gpu_cases(0)[4099], cr.GPU_CV
    other = cooling.Cooling(cr.GPU_T, [2.0 * v for v in cr.GPU_L])
    try:
        assert cooling.kernel_times(ctx) == dict(cool=0.0, coolingTime=0.0)
        cooling.set_timing(ctx, True)
        first, _ = run_cool(ctx, table, c, cv, 0.01)
        assert cooling.kernel_times(ctx)["cool"] > 0.0
        twice, _ = run_cool(ctx, other, c, cv, 0.005)  # twice the rate for half the time: the same curve
        again, _ = run_cool(ctx, table, c, cv, 0.01)
        assert np.array_equal(again, first)
        assert not np.array_equal(run_cool(ctx, other, c, cv, 0.01)[0], first)
        assert np.all(np.abs(twice - first) <= 2 * MARGIN * max(cr.gpu_reference(0)["eps_ref"], cr.eps_floor()) * c["temp"])
    finally:
        cooling.set_timing(ctx, False)
        other.close()


def test_refuses_bad_arguments(ctx, table):
    rho, temp = ctx.upload(np.ones(4, np.float32)), ctx.upload(np.ones(4))
    try:
        with pytest.raises(sx.SxError, match="sx_cool: bad arguments"):
            cooling.cool(ctx, table, rho, rho, temp, 1.25, -1.0)
        with pytest.raises(sx.SxError, match="sx_cooling_time: bad arguments"):
            cooling.cooling_time(ctx, table, rho, temp, 0.0)
    finally:
        ctx.free(rho), ctx.free(temp)
