"""Host side of the group properties (no GPU): what sx_halo_check refuses, with its message; the layout of sx_halo and
sx_halo_result against the header and the ctypes mirrors; sx_fof and sx_fof_result as they were."""
import ctypes as C
import math
import re

import pytest

import sphexa_amd as sx

CUBIC = ([0.0, 1.0] * 3, [1, 1, 1])
OPEN = ([0.0, 1.0] * 3, [0, 0, 0])


@pytest.mark.parametrize("kw, box, message", [
    (dict(linking=0.0), CUBIC, r"sx_fof_check: the linking length must be finite and positive \(got 0\)"),
    (dict(linking=math.nan), OPEN, r"finite and positive \(got -?nan\)"),
    (dict(linking=0.34), CUBIC, r"linking length 0\.34 exceeds a third of the periodic x extent 1 \(0\.333333\)"),
    (dict(linking=0.1, rho_min=math.nan), CUBIC, r"sx_halo_check: rhoMin must be finite \(got -?nan\)"),
    (dict(linking=0.1, rho_min=math.inf), CUBIC, r"sx_halo_check: rhoMin must be finite \(got inf\)"),
    (dict(linking=0.1, G=math.inf), CUBIC, r"sx_halo_check: G must be finite \(got inf\)"),
    (dict(linking=0.1, G=math.nan), CUBIC, r"sx_halo_check: G must be finite \(got -?nan\)"),
    (dict(linking=0.1, flags=8), CUBIC, r"sx_halo_check: unknown flags 0x8 \(known: 0x7\)"),
    (dict(linking=0.1, flags=0x13), CUBIC, r"sx_halo_check: unknown flags 0x10 \(known: 0x7\)"),
    (dict(linking=0.1, flags=("thermal",), gamma=1.0), CUBIC, r"thermal energy needs a finite gamma > 1 \(got 1\)"),
    (dict(linking=0.1, flags=("thermal",), gamma=math.nan), CUBIC, r"thermal energy needs a finite gamma > 1"),
    (dict(linking=0.1, flags=("thermal",), mui_const=0.0), CUBIC, r"thermal energy needs a finite muiConst > 0 \(got 0\)"),
    (dict(linking=0.1, flags=("moments", "thermal"), mui_const=-2.0), OPEN, r"finite muiConst > 0 \(got -2\)"),
])
def test_halo_check_refuses(kw, box, message):
    spec, b = sx.SxHalo(**kw), sx.make_box(*box)
    with pytest.raises(sx.SxError, match=message):
        sx.halo_check(spec, b)
    assert sx.lib().sx_halo_check(C.byref(spec), C.byref(b)) == sx.SX_ERR_ARG


def test_halo_check_refuses_null_and_accepts():
    L = sx.lib()
    assert L.sx_halo_check(None, C.byref(sx.make_box(*CUBIC))) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()
    assert L.sx_halo_check(C.byref(sx.SxHalo(0.1)), None) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()
    sx.halo_check(sx.SxHalo(0.1), sx.make_box(*CUBIC))
    sx.halo_check(sx.SxHalo(1.0 / 3.0, rho_min=-1.0, G=0.0, flags=()), sx.make_box(*CUBIC))
    # gamma and muiConst are read for the thermal energy only
    sx.halo_check(sx.SxHalo(0.1, flags=("moments", "potential"), gamma=0.5, mui_const=0.0), sx.make_box(*OPEN))
    sx.halo_check(sx.SxHalo(0.1, flags=("moments", "thermal", "potential"), max_pair_members=256), sx.make_box(*OPEN))
    with pytest.raises(ValueError, match="unknown group property"):
        sx.SxHalo(0.1, flags=("spin",))


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


CTYPES = {"double": C.c_double, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float}


def test_struct_layouts_match_the_header():
    assert {"sx_halo_check", "sx_halo_compute", "sx_halo_stats", "sx_set_halo_timing", "sx_halo_times", "sx_sim_halos",
            "sx_sim_halos_stats"} <= set(sx.header_symbols())
    members = header_struct("sx_halo")
    assert [m for _, m in members] == [k for k, _ in sx.SxHalo._fields_]
    offset = 0
    for (ctype, member), (_, py) in zip(members, sx.SxHalo._fields_):
        assert CTYPES[ctype] is py, member
        size = C.sizeof(py)
        offset = (offset + size - 1) // size * size  # the C layout: every member at its natural alignment
        assert getattr(sx.SxHalo, member).offset == offset, member
        offset += size
    assert C.sizeof(sx.SxHalo) == (offset + 7) // 8 * 8 == 56
    assert [getattr(sx.SxHalo, k).offset for k, _ in sx.SxHalo._fields_] == [0, 8, 12, 16, 24, 28, 32, 36, 40, 48]
    members = header_struct("sx_halo_result")
    assert [m for _, m in members] == [k for k, _ in sx.SxHaloResult._fields_]
    assert all(t.endswith("*") for t, _ in members)
    assert C.sizeof(sx.SxHaloResult) == 13 * C.sizeof(C.c_void_p)
    # the seven of sx_fof_result lead, in its order
    assert [k for k, _ in sx.SxHaloResult._fields_][:7] == [k for k, _ in sx.SxFofResult._fields_]
    s = sx.SxHalo(0.25, 7, 99, rho_min=3.5, std=True, G=2.0, flags=("thermal", "potential"), mui_const=0.5, gamma=1.4,
                  max_pair_members=300)
    assert (s.linking, s.minMembers, s.maxGroups, s.rhoMin, s.std, s.G, s.flags, s.muiConst, s.gamma,
            s.maxPairMembers) == (0.25, 7, 99, 3.5, 1, 2.0, 6, 0.5, 1.4, 300)
    assert (sx.HALO_FLAGS["moments"], sx.HALO_FLAGS["thermal"], sx.HALO_FLAGS["potential"]) == (1, 2, 4)
    txt = open(sx.HEADER).read()
    for name, bit in (("MOMENTS", 1), ("THERMAL", 2), ("POTENTIAL", 4)):
        assert re.search(r"#define SX_HALO_%s %du\b" % (name, bit), txt)


def test_fof_structs_are_unchanged():
    assert C.sizeof(sx.SxFof) == 16 and sx.SxFof.minMembers.offset == 8 and sx.SxFof.maxGroups.offset == 12
    assert C.sizeof(sx.SxFofResult) == 7 * C.sizeof(C.c_void_p)
    assert [m for _, m in header_struct("sx_fof")] == ["linking", "minMembers", "maxGroups"]
    assert [m for _, m in header_struct("sx_fof_result")] == ["label", "groupLabel", "groupCount", "groupMass", "groupCom",
                                                              "groupVel", "numGroups"]
