"""The direct-sum restatement (tests/direct_ref.py) and the committed fixture tests/golden/direct_ref.npz against the
reference's own ryoanji::directSum (nbody/traversal_cpu.hpp:234-270), through tests/direct_ref_harness.cpp compiled
here with g++ (no OpenMP, no FMA contraction: the loops run sequentially and every operation rounds on its own).

Runs where /root/reference and g++ exist; skipped elsewhere.

    python tests/test_direct_ref.py --write      regenerates tests/golden/direct_ref.npz
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import direct_ref as dr

ROOT = dr.ROOT
REF = "/root/reference"
REF_HDR = os.path.join(REF, "ryoanji", "src", "ryoanji", "nbody", "traversal_cpu.hpp")
SRC = os.path.join(ROOT, "tests", "direct_ref_harness.cpp")

pytestmark = [pytest.mark.ref,
              pytest.mark.skipif(not os.path.exists(REF_HDR) or shutil.which("g++") is None,
                                 reason="reference sources / g++ not present")]

DP, FP = C.POINTER(C.c_double), C.POINTER(C.c_float)


def build_harness(outdir):
    so = os.path.join(str(outdir), "libdirect_ref.so")
    r = subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w",
                        f"-I{REF}/ryoanji/src", f"-I{REF}/domain/include", SRC, "-o", so],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    lib.ref_direct_sum.restype = None
    lib.ref_direct_sum.argtypes = [C.c_size_t] + [DP] * 4 + [FP, C.c_float] + [C.c_double] * 3 + [C.c_int] + [DP] * 4
    return lib


def ref_out4(lib, f, shells):
    """{G m phi, G ax, G ay, G az} per particle from the reference (outputs zeroed: un-accumulated)"""
    n = f["x"].size
    x, y, z = (np.ascontiguousarray(f[k], np.float64) for k in "xyz")
    h = np.ascontiguousarray(f["h"].astype(np.float64))  # Th == Tc: every fixture h is exact in float and double
    m = np.ascontiguousarray(f["m"], np.float32)
    ax, ay, az, u = (np.zeros(n) for _ in range(4))
    lib.ref_direct_sum(n, *[a.ctypes.data_as(DP) for a in (x, y, z, h)], m.ctypes.data_as(FP), float(dr.G), dr.L, dr.L,
                       dr.L, shells, *[a.ctypes.data_as(DP) for a in (ax, ay, az, u)])
    return np.column_stack([u, ax, ay, az])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("direct_ref"))


def fixture_content(lib):
    out = {}
    for case, (key, n, seed, shells) in dr.CASES.items():
        f = dr.inputs(n, seed)
        for k, v in f.items():
            out[f"{key}_{k}"] = v
        out[f"{case}_out4"] = ref_out4(lib, f, shells)
    return out


def test_fixture_is_the_reference_output(harness):
    want = fixture_content(harness)
    assert os.path.getsize(dr.FIXTURE) < 200 * 1024
    with np.load(dr.FIXTURE) as got:
        assert sorted(got.files) == sorted(want)
        for k, v in want.items():
            a, b = np.asarray(got[k]), np.asarray(v)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def test_fixture_inputs_meet_both_softening_branches():
    """h_i + h_j is exact in float and about 0.2 % of the pairs are softened (a target's own image always is)"""
    for case in dr.CASES:
        f, shells = dr.case_inputs(case)
        h = f["h"]
        hij = h[:, None] + h[None, :]
        assert np.array_equal(hij.astype(np.float64), h.astype(np.float64)[:, None] + h.astype(np.float64)[None, :])
        d2 = sum((f[k][:, None] - f[k][None, :]) ** 2 for k in "xyz")
        soft = d2 < (hij.astype(np.float64)) ** 2
        np.fill_diagonal(soft, False)
        frac = soft.mean()
        print(case, "softened pairs:", frac, "targets with none:", int((soft.sum(axis=1) == 0).sum()))
        assert 5e-4 < frac < 1e-2


@pytest.mark.parametrize("case", list(dr.CASES))
def test_restatement_within_the_reorder_bound(harness, case):
    """numpy's pairwise sums against the reference's sequential loop: within the bound for a re-ordered sum
    (measured: at most 1.5e-2 of it, on the potential column of the open case; 4e-3 with images)"""
    f, shells = dr.case_inputs(case)
    want = ref_out4(harness, f, shells)
    got, scale = dr.direct(f, shells)
    bound = dr.reorder_bound(f["x"].size, shells, scale)
    ratio = np.max(np.abs(got - want) / bound)
    print(case, "restatement error / reorder bound:", ratio)
    assert np.all(np.abs(got - want) <= bound), ratio
    assert np.max(np.abs(want[:, 1:])) > 1.0  # O(1) accelerations: the bound is ~1e-10 of them


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            np.savez(dr.FIXTURE, **fixture_content(build_harness(tmp)))
        print("wrote", dr.FIXTURE, os.path.getsize(dr.FIXTURE), "bytes")
