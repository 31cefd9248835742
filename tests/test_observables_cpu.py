"""The host side of the observables, without a GPU: sx_obs_finalize against closed forms, sx_obs_default_settings,
sx_obs_num_sums, sx_grav_wave_htt against the float64 restatement, and the constants.txt line of
format_constants_row (fileutils::writeColumns, main/src/io/file_utils.hpp:14-18)."""
import ctypes as C
import math

import numpy as np
import pytest

import obs_ref
import sphexa_amd as sx


def test_default_settings():
    s = sx.SxObsSettings()
    assert [getattr(s, k) for k, _ in s._fields_] == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    assert C.sizeof(s) == 6 * 8
    assert sx.lib().sx_obs_default_settings(None) == sx.SX_ERR_ARG
    with pytest.raises(TypeError):
        sx.SxObsSettings(rhoInt=1.0)


def test_num_sums_and_names():
    L = sx.lib()
    for name, k in sx.OBS_KINDS.items():
        assert L.sx_obs_num_sums(k) == len(sx.OBS_SUMS[name]) == len(obs_ref.EXTRA[name])
    assert L.sx_obs_num_sums(-1) == -1 and L.sx_obs_num_sums(5) == -1
    assert sx.CONSERVED_SUMS == obs_ref.CONSERVED
    assert [len(sx.OBS_COLUMNS[k]) for k in obs_ref.KINDS] == [9, 10, 10, 11, 15]


def sums_with(extra):
    return np.concatenate([np.arange(1.0, 10.0), np.asarray(extra, dtype=np.float64)])


def test_finalize_closed_forms():
    assert sx.obs_finalize("time_energy", sums_with([]), 10) == []
    # Mach: sqrt(sum / N), N the global count
    assert sx.obs_finalize("mach_rms", sums_with([36.0]), 9) == [2.0]
    assert sx.obs_finalize("mach_rms", sums_with([0.0]), 4096) == [0.0]
    assert sx.obs_finalize("mach_rms", sums_with([2.0]), 3) == [math.sqrt(2.0 / 3)]
    # KH: 2 sqrt(s^2 + c^2) / d
    assert sx.obs_finalize("kh_growth", sums_with([3.0, -4.0, 0.5]), 7) == [20.0]
    assert sx.obs_finalize("kh_growth", sums_with([1e-3, 2e-3, 7.0]), 7) == \
        [2.0 * math.sqrt(1e-3 * 1e-3 + 2e-3 * 2e-3) / 7.0]
    # wind bubble: count * particleMass / initialMass
    st = sx.SxObsSettings(particleMass=0.25, initialMass=8.0)
    assert sx.obs_finalize("wind_bubble", sums_with([64.0]), 100, st) == [2.0]
    assert sx.obs_finalize("wind_bubble", sums_with([0.0]), 100, st) == [0.0]
    # gravitational waves: seen along the z axis (theta = phi = 0), h+ = (xx - yy) gwunits and hx = 2 xy gwunits
    st = sx.SxObsSettings(gravWaveTheta=0.0, gravWavePhi=0.0)
    hp, hx = sx.obs_finalize("grav_waves", sums_with([5.0, 2.0, 11.0, 0.75, 13.0, 17.0]), 1, st)
    assert hp == pytest.approx(3.0 * obs_ref.GWUNITS, rel=1e-15) and hx == pytest.approx(1.5 * obs_ref.GWUNITS, rel=1e-15)
    # a dict of named sums is accepted as Context.observables returns it
    d = dict(zip(sx.CONSERVED_SUMS + sx.OBS_SUMS["mach_rms"], sums_with([36.0])))
    assert sx.obs_finalize("mach_rms", d, 9) == [2.0]
    with pytest.raises(ValueError):
        sx.obs_finalize("mach_rms", sums_with([]), 9)
    with pytest.raises(ValueError):
        sx.obs_finalize("vorticity", sums_with([]), 9)


def test_finalize_refuses_bad_arguments():
    L = sx.lib()
    s = sums_with([1.0]).ctypes.data_as(C.POINTER(C.c_double))
    out = (C.c_double * 2)()
    assert L.sx_obs_finalize(7, None, s, 1, out) == sx.SX_ERR_ARG
    assert L.sx_obs_finalize(1, None, None, 1, out) == sx.SX_ERR_ARG
    assert L.sx_obs_finalize(3, None, s, 1, out) == sx.SX_ERR_ARG  # the wind bubble needs its settings
    assert L.sx_obs_finalize(1, None, s, 1, out) == sx.SX_OK and out[0] == 1.0


def test_htt_against_the_restatement():
    rng = np.random.default_rng(11)
    for _ in range(20):
        q = rng.normal(0.0, 1.0, 6)
        theta, phi = rng.uniform(0, np.pi), rng.uniform(-np.pi, np.pi)
        got = sx.grav_wave_htt(q, theta, phi)
        want = obs_ref.htt(q, theta, phi)
        scale = np.sum(np.abs(q)) * 4 * obs_ref.GWUNITS
        assert abs(got[0] - want[0]) <= 1e-14 * scale and abs(got[1] - want[1]) <= 1e-14 * scale
    # the trace-free part alone radiates: a multiple of the identity gives nothing along any direction
    hp, hx = sx.grav_wave_htt([2.0, 2.0, 2.0, 0.0, 0.0, 0.0], 0.7, 1.9)
    assert abs(hp) <= 1e-15 * 8 * obs_ref.GWUNITS and abs(hx) <= 1e-15 * 8 * obs_ref.GWUNITS


HEAD = [7, 0.001953125, 1e-06, -0.5, 1.25, 2.5e-07, -1.75]


@pytest.mark.parametrize("kind,tail,line", [
    ("time_energy", [3e-18, 123456789.0],
     " 7 0.00195312 1e-06 -0.5 1.25 2.5e-07 -1.75 3e-18 1.23457e+08\n"),
    ("mach_rms", [0.0, 1.0, 0.333333333333],
     " 7 0.00195312 1e-06 -0.5 1.25 2.5e-07 -1.75 0 1 0.333333\n"),
    ("kh_growth", [0.0, 1.0, 1e-5],
     " 7 0.00195312 1e-06 -0.5 1.25 2.5e-07 -1.75 0 1 1e-05\n"),
    ("wind_bubble", [0.0, 1.0, 0.98765432, 0.0208444],
     " 7 0.00195312 1e-06 -0.5 1.25 2.5e-07 -1.75 0 1 0.987654 0.0208444\n"),
    ("grav_waves", [1.5e-50, -2.25e-51, 1.0, -2.0, 3.0, 100000.0, 1000000.0, -0.0001],
     " 7 0.00195312 1e-06 -0.5 1.25 2.5e-07 -1.75 1.5e-50 -2.25e-51 1 -2 3 100000 1e+06 -0.0001\n"),
])
def test_format_constants_row(kind, tail, line):
    """operator<< on a default stream: an integer iteration, doubles as %g (six significant digits, no trailing zeros),
    one separator in FRONT of every column, a newline"""
    row = HEAD + tail
    got = sx.format_constants_row(row, kind)
    assert got == line
    assert got.startswith(" 7 ") and got.endswith("\n") and "7.0" not in got
    assert sx.format_constants_row(dict(zip(sx.OBS_COLUMNS[kind], row)), kind) == line
    assert sx.format_constants_row(row, sx.OBS_KINDS[kind]) == line
    with pytest.raises(ValueError):
        sx.format_constants_row(row[:-1], kind)
