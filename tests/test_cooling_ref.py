"""The oracle of the radiative cooling (cooling_ref.py) held to things it did not produce: closed forms of a single
power law, a fine Runge-Kutta integration of the ODE across a table with kinks, the semigroup property, Y at the nodes,
and the floor.  It also measures eps_ref, the distance of the float64 mode from the mpmath mode over the GPU tests'
inputs, which those tests turn into their tolerance; no figure for it is fixed here.
"""
import mpmath as mp
import numpy as np
import pytest

import cooling_ref as cr

ULP = 2.0 ** -52


def single_law(alpha, T0=1.0, T1=128.0):
    """a two-node table whose one segment has exactly the exponent log(L1/L0)/log(T1/T0) the oracle derives"""
    tab = cr.Table([T0, T1], [2.0, 2.0 * (T1 / T0) ** alpha])
    return tab


def closed_form(tab, T_start, s):
    """the closed form at 50 digits with the table's own exponent: t / t_cool = s L(T_start) / T_start"""
    mp.mp.dps = cr.MP_DIGITS
    a = mp.mpf(float(tab.alpha[0]))
    Ts = mp.mpf(float(T_start))
    L = mp.mpf(float(tab.L[0])) * (Ts / mp.mpf(float(tab.T[0]))) ** a
    return cr.closed_form_mp(a, T_start, mp.mpf(float(s)) * L / Ts)


def closed_form_tol(tab, T_start):
    """Twelve rounded operations lie between T_old and T_new on one segment (quotient, log, product, expm1, quotient,
    the step in z, product, log1p, quotient, exp, product, and the exponent itself), rounded up to 16.  With
    x = T_old / T_k, a rounding of ln x enters ln T_new as it is, one of the exponent with ln x, and one of z or of
    1 + (1 - alpha) z with z / (1 + (1 - alpha) z) = z x^(alpha - 1): of order 1 for alpha < 1, but x^(alpha - 1) /
    (alpha - 1) for alpha > 1, where z runs into its limit 1 / (alpha - 1) and 1 + (1 - alpha) z cancels.  That is the
    price of a wide segment with a steep law (a table sampled finely pays nothing), and the bound follows it"""
    a = tab.alpha[0]
    x = np.asarray(T_start) / tab.T[0]
    z = np.log(x) if a == 1.0 else np.expm1((1.0 - a) * np.log(x)) / (1.0 - a)
    return 16 * ULP * (1.0 + np.log(x) + z * x ** (a - 1.0))


CLOSED_FORM_TOL = 64 * ULP  # where x <= 4 and alpha = 1: the condition numbers above stay below 4


@pytest.mark.parametrize("alpha", [-0.7, 0.5, 2.0])
def test_closed_form_power_law(alpha):
    tab = single_law(alpha)
    T_start = np.array([2.0, 7.5, 40.0, 128.0, 300.0])  # the last one above T_N: the law continues
    for frac in (1e-9, 1e-3, 0.3):
        # a fraction of the time to the floor (alpha < 1) or of t_cool (any alpha), so that T stays above T_1
        s = frac * T_start / cr.rate64(tab, T_start) * (0.5 if alpha >= 1.0 else min(1.0, 1.0 / (1.0 - alpha)))
        T64 = cr.integrate64(tab, T_start, s)
        assert np.all(T64 > tab.T[0]) and np.all(T64 < T_start)
        for t0, x, t, tol in zip(T_start, s, T64, closed_form_tol(tab, T_start)):
            exact = closed_form(tab, t0, x)
            assert abs(mp.mpf(float(t)) - exact) <= tol * exact, (alpha, frac, t0)


def test_closed_form_exponential():
    tab = cr.Table([1.0, 2.0, 4.0], [3.0, 6.0, 12.0])  # L = 3 T: alpha = 1 exactly on both segments
    assert np.all(tab.alpha == 1.0)
    T_start = np.array([1.5, 2.0, 3.9, 9.0])
    for s in (1e-12, 1e-3, 0.05):  # stays on its segment
        T64 = cr.integrate64(tab, T_start, np.full(4, s))
        for t0, t in zip(T_start, T64):
            exact = mp.mpf(float(t0)) * mp.exp(-mp.mpf(3) * mp.mpf(float(s)))
            assert abs(mp.mpf(float(t)) - exact) <= CLOSED_FORM_TOL * exact
    # across the node at 2: Y is searched; still the one exponential (Y / c_0 = 1.4: no cancellation to speak of)
    T64 = cr.integrate64(tab, np.array([3.5]), np.array([0.2]))
    exact = mp.mpf(3.5) * mp.exp(-mp.mpf(3) * mp.mpf(0.2))
    assert 1.0 < T64[0] < 2.0 and abs(mp.mpf(float(T64[0])) - exact) <= CLOSED_FORM_TOL * exact


def rk4(tab, T0, s_total, steps):
    """dT/ds = -L(T), classical Runge-Kutta with a fixed step"""
    T = np.array(T0, dtype=np.float64)
    h = s_total / steps
    f = lambda t: -cr.rate64(tab, t)  # noqa: E731
    for _ in range(steps):
        k1 = f(T)
        k2 = f(T + 0.5 * h * k1)
        k3 = f(T + 0.5 * h * k2)
        k4 = f(T + h * k3)
        T = T + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
    return T


def test_rk4_across_the_kinks():
    """the five-segment table of the GPU tests: from 3000 and 300 down through the nodes to between 1 and 3.  L is
    continuous with kinks at the nodes, so a step across a node has a local error of second order: the error falls by
    about four per halving, not sixteen"""
    tab = cr.Table(cr.GPU_T, cr.GPU_L)
    T0 = np.array([3000.0, 300.0, 3000.0])
    # the s that takes T0 to the target, from Y (which the oracle's integrate is not asked for here)
    target = np.array([2.0, 1.5, 30.0])
    s_total = (cr.Y64(tab, target) - cr.Y64(tab, T0)) / tab.norm
    oracle = np.array([cr.integrate64(tab, T0[i:i + 1], s_total[i:i + 1])[0] for i in range(3)])
    # the three trajectories side by side.  Where in a step a node falls decides how much of the second-order error
    # that step commits, so from one halving to the next the error wanders (and changes sign); over two halvings the
    # sixteen-fold fall of a second-order scheme shows: at least three-fold is asked
    runs = [rk4(tab, T0, s_total, steps) for steps in (1000, 4000, 16000)]
    errs = [np.max(np.abs(T - oracle) / oracle) for T in runs]
    print("rk4 errors", errs)
    assert errs[1] < errs[0] / 3.0 and errs[2] < errs[1] / 3.0, errs
    # what the finest run resolves: its last steps, at T = 1.5 .. 2 with L near 1, are 0.03 wide
    assert errs[2] < 1e-5, errs


def rk4_in_T(tab, T_from, T_to, steps):
    """the same ODE read as ds/dT = -1 / L(T), T the independent variable: the steps can end on the nodes, so no step
    straddles a kink and the scheme keeps its fourth order (for a right-hand side without s it is Simpson's rule)"""
    h = (T_to - T_from) / steps
    T = T_from + h * np.arange(steps)
    f = lambda t: -1.0 / cr.rate64(tab, t)  # noqa: E731
    return float(np.sum((h / 6.0) * (f(T) + 4.0 * f(T + 0.5 * h) + f(T + h))))


def test_rk4_from_node_to_node():
    tab = cr.Table(cr.GPU_T, cr.GPU_L)
    for T0, target in ((3000.0, 2.0), (300.0, 1.5), (9000.0, 30.0), (5.0, 3.5)):
        s = float((cr.Y64(tab, np.array([target])) - cr.Y64(tab, np.array([T0])))[0] / tab.norm)
        T_new = cr.integrate64(tab, np.array([T0]), np.array([s]))[0]
        stops = [T0] + [t for t in tab.T[::-1] if T_new < t < T0] + [T_new]
        errs = []
        for steps in (100, 200, 400):
            took = sum(rk4_in_T(tab, a, b, steps) for a, b in zip(stops[:-1], stops[1:]))
            errs.append(abs(took - s) / s)
        print("T %g -> %.15g: relative error of s" % (T0, T_new), errs)
        # fourth order: sixteen-fold per halving until rounding takes over (1e-13: the sums of a few hundred terms)
        assert errs[1] < max(errs[0] / 10.0, 1e-13) and errs[2] < max(errs[1] / 10.0, 1e-13), errs
        assert errs[2] < 1e-9, errs


def test_semigroup():
    """dt_1 then dt_2 equals dt_1 + dt_2.  Each of the three evaluations lies within eps_ref of the solution; an error
    made at the intermediate temperature is carried to the end by dT_new / dT_mid = L(T_new) / L(T_mid) <= R, the
    ratio of the largest to the smallest value on the table"""
    cases = cr.gpu_cases(0)
    tab, cv = cases["table"], cases["cv"]
    eps = max(cr.gpu_reference(0)["eps_ref"], cr.eps_floor())
    R = tab.L.max() / tab.L.min()
    c = cases[4099]
    for dt1, dt2 in ((1e-10, 2e-10), (0.004, 0.006), (1e-10, 0.01), (20.0, 10.0)):
        s1 = (c["rho"].astype(np.float64) * dt1) / cv
        s2 = (c["rho"].astype(np.float64) * dt2) / cv
        two = cr.integrate64(tab, cr.integrate64(tab, c["temp"], s1), s2)
        one = cr.integrate64(tab, c["temp"], s1 + s2)
        assert np.all(np.abs(two - one) <= (2.0 + R) * eps * c["temp"]), (dt1, dt2)


def test_Y_at_the_nodes():
    tab = cr.Table(cr.GPU_T, cr.GPU_L)
    tmp = cr.TableMp(tab.T, tab.L)
    assert tab.Y[-1] == 0.0 and np.all(np.diff(tab.Y) < 0.0)
    # the nodes' values against 50 digits: a sum of five terms of at most Y_0, each a few roundings
    for k in range(tab.n):
        assert abs(mp.mpf(float(tab.Y[k])) - tmp.Y[k]) <= 16 * ULP * tmp.Y[0]
    # continuity: the segment below a node, evaluated at the node, gives the node's value
    for k in range(1, tab.n - 1):
        from_below = cr.Y64(tab, tab.T[k:k + 1], k=np.array([k - 1]))[0]
        assert abs(from_below - tab.Y[k]) <= 8 * ULP * tab.Y[0], k
    # monotone over a fine grid through every node, from below T_2 to above T_N
    T = np.geomspace(1.0, 15000.0, 20001)
    assert np.all(np.diff(cr.Y64(tab, T)) < 0.0)
    # and the exponent that is 1 exactly is 1 exactly
    assert tab.alpha[1] == 1.0 and tab.alpha[0] > 1.0 and tab.alpha[4] > 1.0


def test_floor():
    tab = cr.Table(cr.GPU_T, cr.GPU_L)
    T0 = np.array([0.2, 0.999, 1.0, 1.0 + 1e-15, 2.0, 80.0, 9000.0])
    big = np.full(T0.size, 1e6)
    T = cr.integrate64(tab, T0, big)
    assert np.array_equal(T[:2], T0[:2])  # below the floor: untouched
    assert np.all(T[2:] == tab.T[0])  # arrival
    assert np.array_equal(cr.integrate64(tab, T, big), T)  # and staying there
    assert np.array_equal(cr.integrate64(tab, T, np.full(T0.size, 1e-30)), T)
    assert np.all(cr.rate64(tab, T0[:2]) == 0.0) and cr.rate64(tab, T0[2:3])[0] == tab.L[0]
    assert np.all(np.isinf(cr.cooling_time64(tab, T0[:2], np.float32([1.0, 1.0]), 1.25)))
    # dt = 0 leaves every bit
    assert np.array_equal(cr.integrate64(tab, T0, np.zeros(T0.size)), T0)
    # never above T_old, never below the floor from above it, whatever rounding does
    c = cr.gpu_cases(0)[4099]
    for dt in (1e-14, 1e-10, 1e-4, 1.0, 1e3):
        Tn = cr.integrate64(tab, c["temp"], (c["rho"].astype(np.float64) * dt) / 1.25)
        assert np.all(Tn <= c["temp"])
        assert np.all(Tn[c["temp"] >= 1.0] >= 1.0)
        assert np.array_equal(Tn[c["temp"] < 1.0], c["temp"][c["temp"] < 1.0])


def test_eps_ref_is_measured_against_the_right_thing():
    """eps_ref = max |T64 - T_mp| / T_old over gpu_cases is what the GPU tests scale their tolerance by.  Here it is
    printed, and the reference it is measured against is itself checked: where a closed form exists the mpmath mode
    reproduces it to 40 digits, so the float64 mode's distance to the mpmath mode is its distance to the solution"""
    ref = cr.gpu_reference(0)
    print("eps_ref = %.3e (%.1f ulp); per call:" % (ref["eps_ref"], ref["eps_ref"] / ULP))
    for key in sorted(k for k in ref if k != "eps_ref"):
        print("  n = %4d dt = %-6g eps = %.3e" % (key[0], key[1], ref[key][2]))
    for alpha in (-0.7, 0.5, 2.0):
        tab = single_law(alpha)
        tmp = cr.TableMp(tab.T, tab.L)
        T_start = np.array([2.0, 7.5, 40.0, 128.0, 300.0])
        s = 0.3 * T_start / cr.rate64(tab, T_start) * (0.5 if alpha >= 1.0 else min(1.0, 1.0 / (1.0 - alpha)))
        T64 = cr.integrate64(tab, T_start, s)
        Tmp = cr.integrate_mp(tmp, T_start, s)
        for t0, x, t64, tm, tol in zip(T_start, s, T64, Tmp, closed_form_tol(tab, T_start)):
            # the closed form with the exponent at 50 digits, as the mpmath mode holds it
            Ts = mp.mpf(float(t0))
            L = tmp.L[0] * (Ts / tmp.T[0]) ** tmp.alpha[0]
            exact = cr.closed_form_mp(tmp.alpha[0], t0, mp.mpf(float(x)) * L / Ts)
            residue = abs(tm - exact)
            assert residue <= mp.mpf(10) ** -40 * exact
            # so of the two modes the float64 one is the one to be judged, and it is as near as one segment allows
            assert abs(mp.mpf(float(t64)) - exact) <= tol * exact
