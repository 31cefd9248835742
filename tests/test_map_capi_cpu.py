"""Host side of the maps (no GPU): the register-resident line-of-sight kernel against a quadrature, and what
sx_map_check refuses."""
import numpy as np
import pytest

import map_ref as mr
import sphexa_amd as sx

# max |mapKernelY - Y| / Y(0) and max |mapKernelY / Y - 1| (for 1 - t / 4 > 1e-3) in float, the figures in the header of
# sx_kernel_poly.hpp
FIT_ERROR = 5.5e-7
FIT_RELATIVE = 8.8e-7


def test_map_kernel_matches_the_quadrature():
    t = np.linspace(0.0, 4.0, 4001).astype(np.float32)
    y = sx.map_kernel(t)
    ref = mr.kernel_y(t.astype(np.float64))
    y0 = mr.kernel_y(np.array([0.0]))[0]
    err = np.abs(y - ref).max() / y0
    print("max |mapKernelY - Y| / Y(0) = %.3e" % err)
    assert err <= 4 * FIT_ERROR
    assert (y >= 0).all()
    inner = t < 4.0 * (1.0 - 1e-3)
    rel = np.abs(y[inner] / ref[inner] - 1.0).max()
    print("max |mapKernelY / Y - 1| = %.3e" % rel)
    assert rel <= 4 * FIT_RELATIVE
    beyond = np.array([4.0, np.nextafter(np.float32(4.0), np.float32(5.0)), 4.5, 100.0, 1e30], np.float32)
    assert np.array_equal(sx.map_kernel(beyond), np.zeros(5, np.float32))


PERIODIC = ([0.0, 1.0, -1.0, 1.0, 0.0, 4.0], [1, 1, 0])  # Lx = 1 and Ly = 2 periodic, z open


def spec(**kw):
    d = dict(kind="column", axis=2, center=(0.5, 0.0, 2.0), width=(1.0, 2.0), depth=0.0, npix=(64, 32))
    d.update(kw)
    return sx.SxMap(**d)


@pytest.mark.parametrize("kw, message", [
    (dict(kind=2), "unknown kind"),
    (dict(kind=-1), "unknown kind"),
    (dict(axis=3), "unknown axis"),
    (dict(npix=(0, 32)), "npix must be 1..4096"),
    (dict(npix=(64, 4097)), "npix must be 1..4096"),
    (dict(width=(0.0, 1.0)), "width must be positive"),
    (dict(width=(1.0, -2.0)), "width must be positive"),
    (dict(width=(1.0001, 2.0)), "width exceeds the box length on a periodic axis"),
    (dict(width=(1.0, 2.5)), "width exceeds the box length on a periodic axis"),
    (dict(depth=-0.1), "depth must not be negative"),
])
def test_map_check_refuses(kw, message):
    box = sx.make_box(*PERIODIC)
    with pytest.raises(sx.SxError, match=message):
        sx.map_check(spec(**kw), box)
    assert sx.lib().sx_map_check(sx.C.byref(spec(**kw)), sx.C.byref(box)) == sx.SX_ERR_ARG


def test_map_check_accepts():
    box = sx.make_box(*PERIODIC)
    sx.map_check(spec(), box)
    # a window that straddles the periodic edges in u and v
    sx.map_check(spec(center=(0.95, 0.9, 2.0), width=(0.5, 1.0)), box)
    # the open axis takes any width; so does a slice, whose depth is ignored
    sx.map_check(spec(axis=1, width=(10.0, 1.0)), box)  # axis 1: u = z (open), v = x (periodic)
    sx.map_check(spec(kind="slice", depth=0.0, npix=(4096, 1)), box)
    with pytest.raises(sx.SxError, match="periodic axis"):
        sx.map_check(spec(axis=1, width=(10.0, 1.5)), box)


def test_gray16_and_pgm_round_trip(tmp_path):
    from sphexa_amd import maps

    img = np.array([[0.0, 1.0, 10.0], [100.0, np.nan, 1000.0]])
    g = maps.to_gray16(img)  # log10: 1 .. 1000 over 0 .. 65535
    assert g.dtype == np.uint16 and g.tolist() == [[0, 0, 21845], [43690, 0, 65535]]
    lin = maps.to_gray16(img, log=False, vmin=0.0, vmax=2000.0)
    assert lin.tolist() == [[0, 33, 328], [3277, 0, 32768]]
    assert not maps.to_gray16(np.zeros((2, 2))).any()
    path = tmp_path / "a.pgm"
    maps.write_pgm(path, g)
    raw = open(path, "rb").read()
    assert raw.startswith(b"P5\n3 2\n65535\n") and len(raw) == 13 + 12
    assert raw[13 + 10:] == bytes([0xFF, 0xFF])  # big-endian samples, the last pixel is 65535
    assert np.array_equal(maps.read_pgm(path), g)
    with pytest.raises(ValueError):
        maps.write_pgm(path, img)
