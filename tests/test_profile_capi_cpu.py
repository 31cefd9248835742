"""Host side of the profiles (no GPU): what sx_profile_check refuses, and the number format of the exact sums --
sx_profile_window, sx_profile_to_fixed, sx_profile_add_fixed, sx_profile_from_fixed -- against the Python-integer oracle
(tests/profile_ref.py), bit for bit."""
import math

import numpy as np
import pytest

import profile_ref as pr
import sphexa_amd as sx

BOX = ([-0.5, 0.5] * 3, [1, 1, 1])
EDGES = np.linspace(0.0, 0.5, 11)
TABLE = ("table", [0.0, 0.5, 1.0], [1.0, 2.0, 3.0])


def spec(**kw):
    return sx.SxProfile(**dict(dict(edges=EDGES, quantities=("vel", "h")), **kw))


def raw(change):
    s = spec()
    change(s)
    return s


def set_sol(s, slot, **kw):
    for k, v in kw.items():
        setattr(s.sol[slot], k, v)


@pytest.mark.parametrize("make, message", [
    (lambda: raw(lambda s: setattr(s, "coord", 5)), "unknown coord"),
    (lambda: raw(lambda s: setattr(s, "coord", -1)), "unknown coord"),
    (lambda: raw(lambda s: (setattr(s, "coord", 4), setattr(s, "coordQ", 11))), "unknown quantity for the coordinate"),
    (lambda: raw(lambda s: s.q.__setitem__(1, 11)), "unknown quantity"),
    (lambda: raw(lambda s: s.q.__setitem__(0, -1)), "unknown quantity"),
    (lambda: raw(lambda s: setattr(s, "weight", 2)), "unknown weight"),
    (lambda: raw(lambda s: set_sol(s, 0, kind=3)), "unknown solution kind"),
    (lambda: spec(edges=[0.0]), r"nbins must be in 1 \.\. 4096"),
    (lambda: spec(edges=np.arange(4098.0)), r"nbins must be in 1 \.\. 4096"),
    (lambda: spec(edges=[0.0, np.inf]), "edges must be finite"),
    (lambda: spec(edges=[0.0, np.nan, 1.0]), "edges must be finite"),
    (lambda: spec(edges=[0.0, 0.2, 0.2, 0.3]), "strictly ascending"),
    (lambda: spec(edges=[0.0, 0.3, 0.2]), "strictly ascending"),
    (lambda: spec(quantities=("vel", "h", "c", "alpha", "divv")), "at most 4 quantities"),
    (lambda: spec(solutions={"vel": ("table", [0.0], [1.0])}), r"a table needs 2 \.\. 2\^20 entries"),
    (lambda: raw(lambda s: (s.set_solution(0, TABLE), set_sol(s, 0, nt=(1 << 20) + 1))), r"a table needs 2 \.\. 2\^20 entries"),
    (lambda: raw(lambda s: (s.set_solution(0, TABLE), set_sol(s, 0, y=None))), "a table needs r and y"),
    (lambda: spec(solutions={"vel": ("table", [0.0, 1.0, 0.5], [1.0, 2.0, 3.0])}), "finite and ascending"),
    (lambda: spec(solutions={"vel": ("table", [0.0, np.nan, 0.5], [1.0, 2.0, 3.0])}), "finite and ascending"),
    (lambda: spec(solutions={"h": ("noh", dict(time=0.1, xgeom=0))}), "xgeom must be 1, 2 or 3"),
    (lambda: spec(solutions={"h": ("noh", dict(time=0.1, xgeom=4))}), "xgeom must be 1, 2 or 3"),
    (lambda: raw(lambda s: s.set_solution(2, TABLE)), "a slot that holds no quantity"),
])
def test_profile_check_refuses(make, message):
    s = make()
    with pytest.raises(sx.SxError, match=message):
        sx.profile_check(s, sx.make_box(*BOX))
    assert sx.lib().sx_profile_check(sx.C.byref(s), sx.C.byref(sx.make_box(*BOX))) == sx.SX_ERR_ARG


def test_profile_check_refuses_null():
    L = sx.lib()
    assert L.sx_profile_check(None, sx.C.byref(sx.make_box(*BOX))) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()
    assert L.sx_profile_check(sx.C.byref(spec()), None) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()
    s = spec()
    s.edges = None
    with pytest.raises(sx.SxError, match="null edges"):
        sx.profile_check(s, sx.make_box(*BOX))


def test_profile_check_accepts():
    box = sx.make_box(*BOX)
    for coord in ("radius", "x", "y", "z", "rho", "alpha"):
        for weight in ("number", "mass"):
            sx.profile_check(spec(coord=coord, weight=weight), box)
    sx.profile_check(spec(edges=np.arange(4097.0), quantities=()), box)
    sx.profile_check(spec(edges=[-1.0, 1.0], quantities=("rho", "p", "u", "temp"),
                          solutions={"rho": ("noh", dict(time=0.3)), "p": ("table", [0.0, 0.0, 1.0], [1.0, 2.0, 3.0], 0.5)}), box)


def test_lds_bins():
    """64 KB less 128 bytes per workgroup, 24 + 64 nq bytes per bin, two of the bins are underflow and overflow"""
    for nq in range(5):
        assert sx.profile_lds_bins(nq) == min(4096, (65536 - 128) // (24 + 64 * nq) - 2)
    assert sx.profile_lds_bins(5) == 0 and sx.profile_lds_bins(-1) == 0


def device_sum(terms):
    """the library's window, fixed-point images, 128-bit sum and final rounding; checked against the oracle's on the way"""
    t = np.asarray(terms, np.float64)
    E = sx.profile_window(t)
    assert E == pr.window(t)
    fx = sx.profile_to_fixed(t, E)
    ints = [pr.to_fixed(v, E) for v in t]
    assert [(int(a), int(b)) for a, b in fx] == [pr.words(v) for v in ints]
    acc = sx.profile_add_fixed(fx)
    assert acc == pr.words(sum(ints))
    half = t.size // 2  # any grouping gives the same integer
    assert sx.profile_add_fixed(fx[half:], sx.profile_add_fixed(fx[:half])) == acc
    out = sx.profile_from_fixed(acc, E)
    ref = pr.from_fixed(sum(ints), E)
    assert np.float64(out).view(np.uint64) == np.float64(ref).view(np.uint64), (out, ref)
    return out, E


M = 3.7e11
CASES = {
    "zeros": [0.0, -0.0, 0.0],
    "plus M": [M],
    "minus M": [-M],
    "plus and minus M": [M, -M, M],
    "small next to M": [M, M * 2.0 ** -100, -M * 2.0 ** -100, M * 2.0 ** -96, M * 2.0 ** -95],
    "subnormals": [5e-324, -1.5e-323, 2.2250738585072014e-308 / 4, 3e-310],
    "one subnormal": [5e-324],
    "subnormal sum that becomes normal": [2.2250738585072009e-308] * 3,
    "largest doubles": [1.7976931348623157e308, -1.7976931348623157e308, 1e308],
    "ties": [1.0, 2.0 ** -53, 1.0 + 2.0 ** -52, 2.0 ** -53],
    "carries": [M] * 5000,
    "borrows": [-M] * 5000,
    "carries then borrows": [M] * 5000 + [-M] * 5000 + [1.0],
    "pairs": [v for a in np.logspace(-20, 20, 41) for v in (a, -a)],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixed_point_against_the_oracle(name):
    out, E = device_sum(CASES[name])
    if name == "zeros":
        assert E == pr.ZERO_WINDOW and out == 0.0
    if name == "pairs":
        assert out == 0.0
    if name == "small next to M":  # 2^-100 M is dropped, 2^-96 M and 2^-95 M are kept (M is not a power of two)
        E = pr.window([M])
        assert pr.to_fixed(M * 2.0 ** -100, E) == 0 and pr.to_fixed(M * 2.0 ** -95, E) > 0


@pytest.mark.parametrize("k", [-1074, -1073, -1022, -1, 0, 1, 52, 53, 1023])
def test_power_of_two_window(k):
    """M = 2^k gives E = k + 1, and the double below it E = k"""
    m = math.ldexp(1.0, k)
    assert sx.profile_window([m]) == k + 1 == pr.window([m])
    if k > -1074:
        below = np.nextafter(m, 0.0)
        assert sx.profile_window([below, -below]) == k == pr.window([below])
    device_sum([m, -m / 2, m / 4])


def test_random_terms_equal_fsum():
    """20000 mixed-sign terms over 24 decades: the window keeps every bit that matters to the rounded sum"""
    rng = np.random.default_rng(7)
    for _ in range(3):
        t = rng.standard_normal(20000) * 10.0 ** rng.uniform(-12, 12, 20000)
        out, _ = device_sum(t)
        assert out == math.fsum(t)


def test_refusals_of_the_helpers():
    with pytest.raises(sx.SxError, match="not finite"):
        sx.profile_window([1.0, np.nan])
    with pytest.raises(sx.SxError, match="not below"):
        sx.profile_to_fixed([4.0], 2)
    assert sx.profile_to_fixed([3.999], 2).tolist() == [list(pr.words(pr.to_fixed(3.999, 2)))]
