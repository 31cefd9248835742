"""The gravitational-wave restatement (tests/obs_ref.py), sx_grav_wave_htt and the committed fixture against the
reference's own main/src/observables/grav_waves_calculations.hpp, through tests/gravwaves_ref_harness.cpp compiled here
with g++ (no OpenMP: the header's sums run sequentially).  That header compiles alone; turbulence_mach_rms.hpp,
time_energy_growth.hpp and wind_bubble_fraction.hpp pull in particles_data.hpp, which does not compile here, so their
restatement in obs_ref.py is by reading, with file:line cited there.

Runs where /root/reference and g++ exist; skipped elsewhere.

    python tests/test_observables_ref.py --write      regenerates tests/golden/gravwaves_ref.npz
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import obs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_HDR = os.path.join(REF, "main", "src", "observables", "grav_waves_calculations.hpp")
SRC = os.path.join(ROOT, "tests", "gravwaves_ref_harness.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gravwaves_ref.npz")
N, FIRST, LAST = 2053, 5, 2053 - 3
THETA, PHI = 0.3, 0.4
NAMES = ["x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az", "m"]

pytestmark = [pytest.mark.ref,
              pytest.mark.skipif(not os.path.exists(REF_HDR) or shutil.which("g++") is None,
                                 reason="reference sources / g++ not present")]

DP, FP = C.POINTER(C.c_double), C.POINTER(C.c_float)


def inputs(seed=20241016):
    rng = np.random.default_rng(seed)
    f = {k: rng.uniform(0.0, 1.0, N) for k in "xyz"}
    for k in ("vx", "vy", "vz", "ax", "ay", "az"):
        f[k] = rng.normal(0.0, 1.0, N).astype(np.float32)
    f["m"] = rng.uniform(0.5, 1.5, N).astype(np.float32)
    return f


def build_harness(outdir):
    so = os.path.join(str(outdir), "libgravwaves_ref.so")
    r = subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-w", f"-I{REF}/main/src", SRC, "-o", so],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    lib.ref_d2q.restype, lib.ref_d2q.argtypes = None, [C.c_size_t, C.c_size_t] + [DP] * 3 + [FP] * 7 + [DP]
    lib.ref_htt.restype, lib.ref_htt.argtypes = None, [DP, C.c_double, C.c_double, DP]
    return lib


def ref_d2q(lib, f, first, last):
    out = np.zeros(6)
    args = [np.ascontiguousarray(f[k]) for k in NAMES]
    lib.ref_d2q(first, last, *[a.ctypes.data_as(DP if a.dtype == np.float64 else FP) for a in args],
                out.ctypes.data_as(DP))
    return out


def ref_htt(lib, q, theta, phi):
    q, out = np.ascontiguousarray(q, dtype=np.float64), np.zeros(2)
    lib.ref_htt(q.ctypes.data_as(DP), theta, phi, out.ctypes.data_as(DP))
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("gravwaves_ref"))


def test_restatement_sums_match_the_reference(harness):
    """the six sums of obs_ref within 1e-15 sum|term| of the reference's sequential loop (only numpy's pairwise
    summation differs; measured <= 6e-17)"""
    f = inputs()
    want = ref_d2q(harness, f, FIRST, LAST)
    s, a = obs_ref.sums("grav_waves", f, first=FIRST, last=LAST, conserved=False)
    for k, name in enumerate(obs_ref.EXTRA["grav_waves"]):
        err = abs(s[name] - want[k])
        print(name, "error / sum|term| =", err / a[name])
        assert err <= 1e-15 * a[name], (name, err / a[name])


def test_terms_match_the_reference_bit_for_bit(harness):
    """one particle at a time the reference's loop adds one term to 0: every term of the restatement is that term"""
    f = inputs()
    t = obs_ref.grav_terms({k: f[k] for k in NAMES})
    for i in (0, 1, 7, 1000, N - 1):
        want = ref_d2q(harness, f, i, i + 1)
        got = np.array([t[name][i] for name in obs_ref.EXTRA["grav_waves"]])
        got[:3] = got[:3] * 2.0 / 3.0
        assert np.array_equal(got, want), (i, got, want)


def test_htt_equals_the_reference_bit_for_bit(harness):
    import sphexa_amd as sx

    rng = np.random.default_rng(3)
    qs = [ref_d2q(harness, inputs(), FIRST, LAST), np.zeros(6), np.eye(6)[3]] + list(rng.normal(0, 1e40, (8, 6)))
    for q in qs:
        for theta, phi in ((THETA, PHI), (0.0, 0.0), (1.2, -2.5), (np.pi / 2, np.pi)):
            got = np.array(sx.grav_wave_htt(q, theta, phi))
            want = ref_htt(harness, q, theta, phi)
            assert np.array_equal(got, want), (q, theta, phi, got, want)


def fixture_content(lib):
    f = inputs()
    d2q = ref_d2q(lib, f, FIRST, LAST)
    out = dict(f)
    out.update(first=np.int64(FIRST), last=np.int64(LAST), theta=np.float64(THETA), phi=np.float64(PHI), d2q=d2q,
               htt=ref_htt(lib, d2q, THETA, PHI))
    return out


def test_fixture_is_the_reference_output(harness):
    want = fixture_content(harness)
    with np.load(FIXTURE) as got:
        assert sorted(got.files) == sorted(want)
        for k, v in want.items():
            a, b = np.asarray(got[k]), np.asarray(v)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            np.savez(FIXTURE, **fixture_content(build_harness(tmp)))
        print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
