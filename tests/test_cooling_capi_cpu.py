"""Host side of the radiative cooling (no GPU): what sx_cooling_create refuses, the header's declarations and their
bindings, the table and the host evaluators against the float64 oracle (cooling_ref.py: the same operations in the same
order, so a difference can come only from the two libraries' log, exp, log1p and expm1), and to_code_units against a
case worked by hand."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import cooling_ref as cr
import sphexa_amd as sx
from sphexa_amd import cooling

NEW_SYMBOLS = ["sx_cooling_create", "sx_cooling_destroy", "sx_cooling_num_nodes", "sx_cooling_get_table",
               "sx_cooling_rate_host", "sx_cooling_integrate_host", "sx_cooling_time", "sx_cool", "sx_set_cooling_timing", "sx_cooling_times", "sx_sim_set_cooling",
               "sx_sim_cooling_stats", "sx_sim_set_cooling_radiated", "sx_sim_cooling_times"]


def create(T, lam, n=None):
    T = np.ascontiguousarray(T, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    h = C.c_void_p()
    rc = sx.lib().sx_cooling_create(C.byref(h), T.ctypes.data, lam.ctypes.data, T.size if n is None else n)
    if rc == sx.SX_OK:
        sx.lib().sx_cooling_destroy(h)
    return rc


@pytest.mark.parametrize("T, lam", [
    ([1.0], [1.0]),                                   # n < 2
    (np.arange(1.0, 258.0), np.ones(257)),            # n > 256
    ([1.0, 1.0], [1.0, 2.0]),                         # T not strictly increasing
    ([1.0, 3.0, 2.0], [1.0, 2.0, 3.0]),
    ([1.0, math.nan], [1.0, 2.0]),                    # not finite
    ([1.0, math.inf], [1.0, 2.0]),
    ([1.0, 2.0], [1.0, math.nan]),
    ([1.0, 2.0], [math.inf, 1.0]),
    ([0.0, 2.0], [1.0, 1.0]),                         # not positive
    ([-1.0, 2.0], [1.0, 1.0]),
    ([1.0, 2.0], [0.0, 1.0]),
    ([1.0, 2.0], [1.0, -3.0]),
])
def test_create_refuses(T, lam):
    assert create(T, lam) == sx.SX_ERR_ARG
    with pytest.raises((sx.SxError, ValueError)):
        cooling.Cooling(T, lam)


def test_create_refuses_null_and_accepts_the_limits():
    L = sx.lib()
    h = C.c_void_p()
    two = np.array([1.0, 2.0])
    assert L.sx_cooling_create(None, two.ctypes.data, two.ctypes.data, 2) == sx.SX_ERR_ARG
    assert L.sx_cooling_create(C.byref(h), None, two.ctypes.data, 2) == sx.SX_ERR_ARG
    assert L.sx_cooling_create(C.byref(h), two.ctypes.data, None, 2) == sx.SX_ERR_ARG
    assert create(two, two) == sx.SX_OK
    T = np.geomspace(1.0, 1e8, 256)
    assert create(T, 1.0 + np.sin(np.arange(256.0)) ** 2) == sx.SX_OK
    assert L.sx_cooling_num_nodes(None) == 0


def test_header_and_bindings():
    txt = open(sx.HEADER).read()
    assert re.search(r"#define\s+SX_COOLING_MAX_NODES\s+256\b", txt)
    assert re.search(r"typedef\s+struct\s+sx_cooling\s+sx_cooling\s*;", txt)
    declared = sx.header_symbols()
    L = sx.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert getattr(L, name).argtypes is not None, name
    assert L.sx_cooling_rate_host.restype is C.c_double and L.sx_cooling_integrate_host.restype is C.c_double
    # the struct of the device scalars gained its word at the end: sx_sim_scalars keeps its six
    src = open(sx.HEADER.replace("include/sphexa_hip.h", "sph-exa_amd/csrc/sx_sim.hpp")).read()
    body = re.search(r"struct Scalars\s*\{(.*?)\};", src, re.S).group(1)
    members = re.findall(r"(\w+)\s*;", re.sub(r"//[^\n]*", "", body))
    assert members[-1] == "minDtCool" and members[-2] == "gravErr"
    assert re.search(r"int\s+sx_sim_scalars\(sx_sim\* sim, double out\[6\]\)", txt)


@pytest.fixture(scope="module")
def gpu_table():
    c = cooling.Cooling(cr.GPU_T, cr.GPU_L)
    yield c, cr.Table(cr.GPU_T, cr.GPU_L)
    c.close()


def test_table_against_the_oracle(gpu_table):
    c, tab = gpu_table
    assert c.num_nodes == 6
    t = c.table()
    assert np.array_equal(t["T"], tab.T) and np.array_equal(t["lam"], tab.L)
    # alpha: one quotient of two logarithms; Y: at most five terms of a few roundings each, none above Y_0
    assert np.all(np.abs(t["alpha"] - tab.alpha) <= 4 * 2.0 ** -52 * np.abs(tab.alpha))
    assert t["alpha"][1] == 1.0 and t["alpha"][5] == t["alpha"][4]
    assert np.all(np.abs(t["Y"] - tab.Y) <= 16 * 2.0 ** -52 * tab.Y[0])
    assert t["Y"][5] == 0.0 and np.all(np.diff(t["Y"]) < 0.0)
    # every pointer may be NULL
    L = sx.lib()
    only_Y = np.empty(6)
    assert L.sx_cooling_get_table(c.h, None, None, None, only_Y.ctypes.data) == sx.SX_OK
    assert np.array_equal(only_Y, t["Y"])
    assert L.sx_cooling_get_table(c.h, None, None, None, None) == sx.SX_OK
    assert L.sx_cooling_get_table(None, None, None, None, None) == sx.SX_ERR_ARG


def test_rate_host_against_the_oracle(gpu_table):
    c, tab = gpu_table
    T = cr.gpu_cases(0)[4099]["temp"]
    r = c.rate(T)
    ref = cr.rate64(tab, T)
    assert np.all(r[T < 1.0] == 0.0) and np.all(r[T >= 1.0] > 0.0)
    # product, log, product, exp, product: the exponent's argument |alpha ln x| stays below 4
    assert np.all(np.abs(r - ref) <= 16 * 2.0 ** -52 * ref)
    assert c.rate(1.0) == 0.5 and c.rate(5000.0) == 40.0 and c.rate(math.nan) == 0.0


def test_integrate_host_against_the_oracle(gpu_table):
    """the library's host evaluator and the numpy oracle run the same operations; their libraries' log, exp, log1p
    and expm1 may differ in the last place, which the integration amplifies exactly as it amplifies the oracle's own
    roundings: the bound is the GPU tests', 16 eps_ref T_old"""
    c, tab = gpu_table
    cases, ref = cr.gpu_cases(0), cr.gpu_reference(0)
    eps = max(ref["eps_ref"], cr.eps_floor())
    for n in cr.GPU_SIZES:
        cs = cases[n]
        for dt in cases["dts"]:
            s = (cs["rho"].astype(np.float64) * dt) / cases["cv"]
            Th = c.integrate(cs["temp"], s)
            T64 = ref[(n, dt)][0]
            assert np.all(np.abs(Th - T64) <= 16 * eps * cs["temp"]), (n, dt)
            assert np.all(Th <= cs["temp"])
            above = cs["temp"] >= 1.0
            assert np.all(Th[above] >= 1.0) and np.array_equal(Th[~above], cs["temp"][~above])
            if dt == 0.0:
                assert np.array_equal(Th, cs["temp"])
    assert math.isnan(c.integrate(math.nan, 1.0))


def test_power_law_and_from_samples():
    c = cooling.power_law(L0=2.0, alpha=-0.5, T0=10.0, Tmin=1.0, Tmax=100.0)
    t = c.table()
    assert np.array_equal(t["T"], [1.0, 100.0])
    assert abs(t["alpha"][0] + 0.5) < 1e-15 and abs(c.rate(10.0) - 2.0) < 1e-14
    assert c.rate(0.5) == 0.0 and abs(c.rate(400.0) - 2.0 * 40.0 ** -0.5) < 1e-14  # the law continues above Tmax
    c.close()
    c = cooling.from_samples([50.0, 1.0, 6.0, 3.0, 400.0, 5000.0], [1.0, 0.5, 4.0, 2.0, 3.0, 40.0])
    assert np.array_equal(c.table()["T"], cr.GPU_T) and np.array_equal(c.table()["lam"], cr.GPU_L)
    c.close()


def test_to_code_units_by_hand():
    """unit_mass = 2e33 g, unit_length = 3e21 cm, unit_time = 1e15 s, X = 0.5:
    unit_density = 2e33 / 2.7e64 = 7.407407...e-32 g/cm^3, unit_specific_energy = (3e6)^2 = 9e12 erg/g;
    (X / m_H)^2 = (0.5 / 1.67262192369e-24)^2 = 8.936025e46 g^-2 (0.5 / 1.67262192369 = 0.29893185, squared 0.08936025);
    Lambda = 1e-22 erg cm^3/s -> Lhat_cgs = 8.936025e24; times 7.407407e-32 * 1e15 / 9e12 = 8.230453e-30 -> 7.354754e-5.
    T = 9e6 K -> 9e6 / 9e12 = 1e-6."""
    T, lam = cooling.to_code_units([9e6, 1.8e7], [1e-22, 2e-22], unit_mass=2e33, unit_length=3e21, unit_time=1e15, X=0.5)
    assert T == pytest.approx([1e-6, 2e-6], rel=1e-15)
    assert lam[0] == pytest.approx(7.354754e-5, rel=2e-6)
    assert lam[1] == pytest.approx(2.0 * lam[0], rel=1e-15)
    # the formulas themselves, once more from their parts
    expect = (0.5 / cooling.M_H) ** 2 * 1e-22 * (2e33 / 3e21 ** 3) * 1e15 / (3e21 / 1e15) ** 2
    assert lam[0] == pytest.approx(expect, rel=1e-14)
    # X defaults to 0.76
    _, lam76 = cooling.to_code_units([9e6, 1.8e7], [1e-22, 2e-22], 2e33, 3e21, 1e15)
    assert lam76[0] == pytest.approx(lam[0] * (0.76 / 0.5) ** 2, rel=1e-14)
