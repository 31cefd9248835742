"""Host side of the friends-of-friends groups (no GPU): what sx_fof_check refuses, with its figures; the cell grid of
sx_fof_grid against a restatement in Python; the layout of the two structs against the header."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import sphexa_amd as sx

CUBIC = ([0.0, 1.0] * 3, [1, 1, 1])
OPEN = ([0.0, 1.0] * 3, [0, 0, 0])
MIXED = ([-0.5, 0.5, 0.0, 2.0, -1.0, 0.5], [1, 0, 2])


@pytest.mark.parametrize("linking, box, message", [
    (0.0, CUBIC, r"finite and positive \(got 0\)"),
    (-0.1, CUBIC, r"finite and positive \(got -0\.1\)"),
    (math.nan, CUBIC, r"finite and positive \(got -?nan\)"),
    (math.inf, OPEN, r"finite and positive \(got inf\)"),
    (0.34, CUBIC, r"linking length 0\.34 exceeds a third of the periodic x extent 1 \(0\.333333\)"),
    (0.4, MIXED, r"linking length 0\.4 exceeds a third of the periodic x extent 1 \(0\.333333\)"),
    (0.5, ([0.0, 4.0, 0.0, 1.2, 0.0, 4.0], [1, 1, 1]), r"linking length 0\.5 exceeds a third of the periodic y extent 1\.2 \(0\.4\)"),
    (0.5, ([0.0, 4.0, 0.0, 4.0, -1.0, 0.0], [0, 2, 1]), r"linking length 0\.5 exceeds a third of the periodic z extent 1 \(0\.333333\)"),
])
def test_fof_check_refuses(linking, box, message):
    spec, b = sx.SxFof(linking), sx.make_box(*box)
    with pytest.raises(sx.SxError, match=message):
        sx.fof_check(spec, b)
    assert sx.lib().sx_fof_check(C.byref(spec), C.byref(b)) == sx.SX_ERR_ARG
    with pytest.raises(sx.SxError, match=message):
        sx.fof_grid(spec, b, 1000)


def test_fof_check_refuses_null_and_accepts():
    L = sx.lib()
    assert L.sx_fof_check(None, C.byref(sx.make_box(*CUBIC))) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()
    assert L.sx_fof_check(C.byref(sx.SxFof(0.1)), None) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()
    assert L.sx_fof_grid(C.byref(sx.SxFof(0.1)), C.byref(sx.make_box(*CUBIC)), 10, None) == sx.SX_ERR_ARG
    sx.fof_check(sx.SxFof(1.0 / 3.0), sx.make_box(*CUBIC))  # a third itself is accepted
    sx.fof_check(sx.SxFof(5.0), sx.make_box(*OPEN))  # no limit without a periodic axis
    wide_open = ([0.0, 3.0, 0.0, 0.5, 0.0, 0.5], [1, 0, 2])
    sx.fof_check(sx.SxFof(0.9), sx.make_box(*wide_open))  # y open, z fixed: only the periodic x extent counts


def grid_restated(linking, lim, bnd, n):
    """sx_fof_grid in Python, the same double operations"""
    dims, lowest = [], []
    for a in range(3):
        L = lim[2 * a + 1] - lim[2 * a]
        q = math.floor(L / linking * (1.0 - 2.0 ** -20))
        lo = 3 if bnd[a] == 1 else 1
        dims.append(1024 if q >= 1024 else q if q >= lo else lo)
        lowest.append(lo)
    limit = max(27, 2 * n)
    while dims[0] * dims[1] * dims[2] > limit:
        a = max(range(3), key=lambda k: (dims[k], -k))
        dims[a] = max(lowest[a], (dims[a] + 1) // 2)
    return tuple(dims)


@pytest.mark.parametrize("box", [CUBIC, OPEN, MIXED], ids=["cubic", "open", "mixed"])
@pytest.mark.parametrize("n", [0, 1, 7, 64, 1000, 20000, 10 ** 6, 2 ** 31 - 1])
@pytest.mark.parametrize("linking", [1.0 / 3.0, 0.25, 0.1, 0.0123, 0.2 * 20000 ** (-1 / 3), 1e-3, 1e-7, 1e-300])
def test_fof_grid(box, n, linking):
    lim, bnd = box
    dims = sx.fof_grid(sx.SxFof(linking), sx.make_box(lim, bnd), n)
    assert dims == grid_restated(linking, lim, bnd, n)
    for a in range(3):
        L = lim[2 * a + 1] - lim[2 * a]
        assert L / dims[a] >= linking, "a cell is at least a linking length wide"
        assert 1 <= dims[a] <= 1024
        if bnd[a] == 1:
            assert dims[a] >= 3, "three distinct cells on a periodic axis"
    assert dims[0] * dims[1] * dims[2] <= max(27, 2 * n), "the cell-start array stays within twice the particles"


def test_fof_grid_wide_linking_and_grid_grows_with_n():
    # an open box and a linking length beyond it: one cell
    assert sx.fof_grid(sx.SxFof(5.0), sx.make_box(*OPEN), 1000) == (1, 1, 1)
    # the tiny-l grid is bounded by the particles, not by l
    small = sx.fof_grid(sx.SxFof(1e-6), sx.make_box(*CUBIC), 1000)
    large = sx.fof_grid(sx.SxFof(1e-6), sx.make_box(*CUBIC), 10 ** 6)
    assert np.prod(small) <= 2000 < np.prod(large) <= 2 * 10 ** 6
    # when l allows it the cells are as small as l allows: floor(L / l) per axis, less the safety margin
    assert sx.fof_grid(sx.SxFof(0.1001), sx.make_box(*CUBIC), 10 ** 6) == (9, 9, 9)
    assert sx.fof_grid(sx.SxFof(0.1001), sx.make_box(*MIXED), 10 ** 6) == (9, 19, 14)


def header_struct(name):
    """the members of `typedef struct name { ... } name;` in the header: [(type, member)]"""
    txt = open(sx.HEADER).read()
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(\w+)\s*(.*)", decl)
        for item in m.group(2).split(","):
            item = item.strip()
            out.append((m.group(1) + ("*" if item.startswith("*") or m.group(2).lstrip().startswith("*") else ""),
                        item.lstrip("* ")))
    return out


def test_struct_layouts_match_the_header():
    assert {"sx_fof_check", "sx_fof_grid", "sx_fof_compute", "sx_fof_stats", "sx_set_fof_timing", "sx_fof_times",
            "sx_sim_fof", "sx_sim_fof_stats"} <= set(sx.header_symbols())
    sizes = {"double": (C.c_double, 8), "uint32_t": (C.c_uint32, 4)}
    members = header_struct("sx_fof")
    assert [m for _, m in members] == [k for k, _ in sx.SxFof._fields_]
    for (ctype, member), (_, py) in zip(members, sx.SxFof._fields_):
        assert sizes[ctype][0] is py, member
    assert C.sizeof(sx.SxFof) == 16 and sx.SxFof.minMembers.offset == 8 and sx.SxFof.maxGroups.offset == 12
    members = header_struct("sx_fof_result")
    assert [m for _, m in members] == [k for k, _ in sx.SxFofResult._fields_]
    assert all(t.endswith("*") for t, _ in members)
    assert C.sizeof(sx.SxFofResult) == 7 * C.sizeof(C.c_void_p)
    s = sx.SxFof(0.25, min_members=7, max_groups=99)
    assert (s.linking, s.minMembers, s.maxGroups) == (0.25, 7, 99)
