"""Host side of the two-point statistics (no GPU): what sx_twopoint_check refuses, with its figures; the cell grid of
sx_twopoint_grid against a restatement in Python; the layout of the two structs; the shift-64 number format of the host
helpers against the Python-integer oracle (tests/twopoint_ref.py)."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import sphexa_amd as sx
import twopoint_ref as tr

CUBIC = ([0.0, 1.0] * 3, [1, 1, 1])
OPEN = ([0.0, 1.0] * 3, [0, 0, 0])
MIXED = ([-0.5, 0.5, 0.0, 2.0, -1.0, 0.5], [1, 0, 2])
E3 = [0.0, 0.1, 0.2, 0.3]


@pytest.mark.parametrize("edges, kw, box, message", [
    ([0.1], {}, CUBIC, r"nbins must be 1 \.\. 256 \(got 0\)"),
    (np.linspace(0.0, 0.3, 258), {}, CUBIC, r"nbins must be 1 \.\. 256 \(got 257\)"),
    ([0.0, math.nan, 0.2], {}, CUBIC, r"edge 1 is not finite \(-?nan\)"),
    ([0.0, 0.1, math.inf], {}, OPEN, r"edge 2 is not finite \(inf\)"),
    ([-0.1, 0.1, 0.2], {}, CUBIC, r"the first edge is negative \(-0\.1\)"),
    ([0.0, 0.2, 0.2], {}, CUBIC, r"do not ascend strictly at 1 \(0\.2, then 0\.2\)"),
    ([0.0, 0.2, 0.1], {}, CUBIC, r"do not ascend strictly at 1 \(0\.2, then 0\.1\)"),
    (E3, {"stride": 0}, CUBIC, r"stride is 0"),
    (E3, {"stride": 3, "phase": 3}, CUBIC, r"phase 3 is not below stride 3"),
    (E3, {"series": 64 | 1}, CUBIC, r"unknown series flags 0x40 \(known: 0x3f\)"),
    ([0.0, 0.34], {}, CUBIC, r"r_max 0\.34 exceeds a third of the periodic x extent 1 \(0\.333333\)"),
    ([0.0, 0.5], {}, ([0.0, 4.0, 0.0, 1.2, 0.0, 4.0], [1, 1, 1]), r"r_max 0\.5 exceeds a third of the periodic y extent 1\.2 \(0\.4\)"),
    ([0.0, 0.5], {}, ([0.0, 4.0, 0.0, 4.0, -1.0, 0.0], [0, 2, 1]), r"r_max 0\.5 exceeds a third of the periodic z extent 1 \(0\.333333\)"),
])
def test_twopoint_check_refuses(edges, kw, box, message):
    spec, b = sx.SxTwoPoint(edges, **kw), sx.make_box(*box)
    with pytest.raises(sx.SxError, match=message):
        sx.twopoint_check(spec, b)
    assert sx.lib().sx_twopoint_check(C.byref(spec), C.byref(b)) == sx.SX_ERR_ARG
    with pytest.raises(sx.SxError, match=message):
        sx.twopoint_grid(spec, b, 1000)


def test_twopoint_check_refuses_null_and_accepts():
    L = sx.lib()
    assert L.sx_twopoint_check(None, C.byref(sx.make_box(*CUBIC))) == sx.SX_ERR_ARG
    assert "null specification or box" in L.sx_last_error(None).decode()
    assert L.sx_twopoint_check(C.byref(sx.SxTwoPoint(E3)), None) == sx.SX_ERR_ARG
    assert "null specification or box" in L.sx_last_error(None).decode()
    assert L.sx_twopoint_check(C.byref(sx.SxTwoPoint()), C.byref(sx.make_box(*CUBIC))) == sx.SX_ERR_ARG
    assert "null edges" in L.sx_last_error(None).decode()
    assert L.sx_twopoint_grid(C.byref(sx.SxTwoPoint(E3)), C.byref(sx.make_box(*CUBIC)), 10, None) == sx.SX_ERR_ARG
    assert "null dims" in L.sx_last_error(None).decode()
    sx.twopoint_check(sx.SxTwoPoint([0.0, 1.0 / 3.0]), sx.make_box(*CUBIC))  # a third itself is accepted
    sx.twopoint_check(sx.SxTwoPoint([0.5, 5.0]), sx.make_box(*OPEN))  # no limit without a periodic axis
    sx.twopoint_check(sx.SxTwoPoint(np.linspace(0, 0.3, 257), series=("count", "vel", "mass"), stride=8, phase=7),
                      sx.make_box(*CUBIC))
    assert sx.SxTwoPoint(E3, series=("count",)).series == 0 and sx.SxTwoPoint(E3).series == 31
    assert sx.SxTwoPoint(E3, mass=True).series == 63 and sx.SxTwoPoint(E3, series=("U2", "WW")).series == 34


def grid_restated(length, lim, bnd, n):
    """the rule of sx_fof_grid in Python, the same double operations, with r_max for the linking length"""
    dims, lowest = [], []
    for a in range(3):
        L = lim[2 * a + 1] - lim[2 * a]
        q = math.floor(L / length * (1.0 - 2.0 ** -20))
        lo = 3 if bnd[a] == 1 else 1
        dims.append(1024 if q >= 1024 else q if q >= lo else lo)
        lowest.append(lo)
    limit = max(27, 2 * n)
    while dims[0] * dims[1] * dims[2] > limit:
        a = max(range(3), key=lambda k: (dims[k], -k))
        dims[a] = max(lowest[a], (dims[a] + 1) // 2)
    return tuple(dims)


@pytest.mark.parametrize("box", [CUBIC, OPEN, MIXED], ids=["cubic", "open", "mixed"])
@pytest.mark.parametrize("n", [0, 1, 64, 4000, 10 ** 6, 2 ** 31 - 1])
@pytest.mark.parametrize("rmax", [1.0 / 3.0, 0.25, 0.0123, 1e-3, 1e-300])
def test_twopoint_grid(box, n, rmax):
    lim, bnd = box
    spec = sx.SxTwoPoint([0.25 * rmax, 0.5 * rmax, rmax])
    dims = sx.twopoint_grid(spec, sx.make_box(lim, bnd), n)
    assert dims == grid_restated(rmax, lim, bnd, n)
    assert dims == sx.fof_grid(sx.SxFof(rmax), sx.make_box(lim, bnd), n), "the group finder's grid at linking = r_max"
    for a in range(3):
        assert (lim[2 * a + 1] - lim[2 * a]) / dims[a] >= rmax, "a cell is at least r_max wide"
        assert dims[a] >= (3 if bnd[a] == 1 else 1)


def header_members(name):
    """the member names of `typedef struct name { ... } name;` in the header, in order"""
    txt = open(sx.HEADER).read()
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", item).group(1) for decl in body.split(";") if decl.strip()
            for item in decl.split(",")]


def test_struct_layouts_match_the_header():
    assert {"sx_twopoint_check", "sx_twopoint_grid", "sx_twopoint_compute", "sx_twopoint_stats", "sx_set_twopoint_timing",
            "sx_twopoint_times", "sx_twopoint_window", "sx_twopoint_to_fixed", "sx_twopoint_add_fixed",
            "sx_twopoint_from_fixed", "sx_sim_twopoint", "sx_sim_twopoint_stats"} <= set(sx.header_symbols())
    assert header_members("sx_twopoint") == [k for k, _ in sx.SxTwoPoint._fields_]
    assert C.sizeof(sx.SxTwoPoint) == 24
    assert [getattr(sx.SxTwoPoint, k).offset for k, _ in sx.SxTwoPoint._fields_] == [0, 8, 12, 16, 20]
    assert header_members("sx_twopoint_result") == [k for k, _ in sx.SxTwoPointResult._fields_]
    assert C.sizeof(sx.SxTwoPointResult) == 8 * C.sizeof(C.c_void_p)
    txt = open(sx.HEADER).read()
    for k, name in enumerate(sx.TP_SERIES):
        assert "#define SX_TP_%s %du" % (name, 1 << k) in txt and sx.TP_FLAGS[name] == tr.FLAGS[name] == 1 << k


# ---- the number format -------------------------------------------------------------------------------------------
def lib_window(t):
    t = np.ascontiguousarray(t, np.float64)
    E = C.c_int32()
    assert sx.lib().sx_twopoint_window(t.ctypes.data, t.size, C.byref(E)) == sx.SX_OK
    return E.value


def lib_sum(t, E):
    """(the 128-bit sum as a Python integer modulo 2^128, its rounding) of the terms t in window E through the helpers"""
    t = np.ascontiguousarray(t, np.float64)
    lohi = np.zeros(2 * t.size, np.uint64)
    assert sx.lib().sx_twopoint_to_fixed(t.ctypes.data, t.size, E, lohi.ctypes.data) == sx.SX_OK, \
        sx.lib().sx_last_error(None).decode()
    for v, lo, hi in zip(t, lohi[0::2], lohi[1::2]):
        assert (int(lo), int(hi)) == tr.words(tr.to_fixed(v, E)), (v, E)
    acc = np.zeros(2, np.uint64)
    assert sx.lib().sx_twopoint_add_fixed(acc.ctypes.data, lohi.ctypes.data, t.size) == sx.SX_OK
    out = C.c_double()
    assert sx.lib().sx_twopoint_from_fixed(acc.ctypes.data, E, C.byref(out)) == sx.SX_OK
    return (int(acc[0]), int(acc[1])), out.value


def check_sum(t, E):
    want = sum(tr.to_fixed(v, E) for v in t)
    got, value = lib_sum(t, E)
    assert got == tr.words(want)
    ref = tr.from_fixed(want, E)
    assert value == ref
    return value


def test_format_zeros_bound_and_windows():
    assert lib_window([]) == lib_window([0.0, -0.0]) == tr.ZERO_WINDOW
    for t in ([1.0], [0.999], [5e-324], [1.7e308], [3.0, -4.0], [2.0 ** -1022]):
        assert lib_window(t) == tr.window(t)
    assert check_sum([0.0, -0.0], tr.ZERO_WINDOW) == 0.0
    assert check_sum([0.0], 5) == 0.0
    # the velocity windows of vmax = 0: every term is a zero, every window far below the subnormals
    for E in tr.windows(0.0, 0.0).values():
        assert check_sum([0.0, -0.0, 0.0], E) == 0.0
    # +-bound: u = +-0.87 2^Eu, and the window's own top 2^E, which an underflowing product may round up to
    for E in (-1071, -40, 0, 3, 900):
        top = math.ldexp(1.0, E)
        lo, hi = tr.words(tr.to_fixed(top, E))
        assert (lo, hi) == (0, 1), "2^E is 2^64 in the fixed point"
        check_sum([top, -top, 0.87 * top, -0.87 * top, math.nextafter(top, 0.0)], E)
        assert check_sum([math.nextafter(top, 0.0)] * 3, E) == 3 * math.nextafter(top, 0.0)
    t = np.array([2.0])
    lohi = np.zeros(2, np.uint64)
    assert sx.lib().sx_twopoint_to_fixed(t.ctypes.data, 1, 0, lohi.ctypes.data) == sx.SX_ERR_ARG
    assert "above 2^E" in sx.lib().sx_last_error(None).decode()
    t[0] = math.inf
    assert sx.lib().sx_twopoint_to_fixed(t.ctypes.data, 1, 0, lohi.ctypes.data) == sx.SX_ERR_ARG


def test_format_subnormal_windows():
    """vmax = 5e-324: ev = -1073, Eu = -1071; u is a small multiple of 2^-1074, its powers underflow to zero"""
    E = tr.windows(5e-324, 5e-324)
    assert E["U1"] == -1071 and E["U2"] == E["T2"] == -2142 and E["U3"] == E["A3"] == -3213 and E["WW"] == -2146
    tiny = 5e-324
    assert check_sum([tiny, tiny, -tiny, 3 * tiny, -2 * tiny, 6 * tiny], E["U1"]) == 8 * tiny
    assert check_sum([tiny * tiny, 0.0], E["U2"]) == 0.0 and check_sum([0.0], E["U3"]) == 0.0
    # a sum that leaves the subnormals
    t = [math.ldexp(1.0, -1023)] * 5 + [tiny]
    assert check_sum(t, -1020) == math.fsum(t)


def test_format_carries_borrows_and_cancellation():
    rng = np.random.default_rng(8)
    E = 3
    # 5000 terms near +-the bound: the low word wraps on nearly every add, upwards and downwards
    t = (0.5 + 0.37 * rng.random(5000)) * 8.0 * rng.choice([-1.0, 1.0], 5000)
    value = check_sum(t, E)
    assert abs(value - math.fsum(t)) <= 5000 * 2.0 ** (E - 64), "within count 2^(E - 64) of the real sum"
    check_sum(np.abs(t), E)
    check_sum(-np.abs(t), E)
    # terms below one unit of the fixed point are floored away, magnitude-wise
    assert check_sum([2.0 ** -62, -(2.0 ** -62), 2.0 ** -61, -(2.0 ** -61)], E) == 0.0
    assert tr.to_fixed(2.0 ** -62, E) == 0 and tr.to_fixed(-(2.0 ** -61), E) == -1
    # exact cancellation: a set and its negation, shuffled
    both = np.concatenate([t, -t])
    rng.shuffle(both)
    got, value = lib_sum(both, E)
    assert got == (0, 0) and value == 0.0 and math.copysign(1.0, value) == 1.0
    # a rounding tie: 2^53 + 1 units of 2^(E - 64) rounds to even
    assert check_sum([math.ldexp(1.0, E - 11), math.ldexp(1.0, E - 64)], E) == math.ldexp(1.0, E - 11)
    assert check_sum([math.ldexp(1.0, E - 11), math.ldexp(3.0, E - 64)], E) == math.ldexp(1.0, E - 11) + math.ldexp(4.0, E - 64)
