"""The drop-in sph-exa_amd/host/observables/gpu_reductions.h (gpuGrowthRate, machSquareSumGpu, survivorsGpu in namespace
sphexa) against the reference's cstone headers, on the CPU, in the manner of test_turb_mirror_compile.py:
tests/obs_mirror_compile.cpp instantiates the three templates with the SphTypes combinations and calls them as the
reference's observables do; it is compiled with g++ and linked against libsphexa_hip.so, and the object's undefined
sx_* symbols are functions of include/sphexa_hip.h.

Runs where /root/reference exists; skipped on the GPU box.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_BOX = os.path.join(REF, "domain", "include", "cstone", "sfc", "box.hpp")
LIBDIR = os.path.join(ROOT, "sph-exa_amd", "lib")
SRC = os.path.join(ROOT, "tests", "obs_mirror_compile.cpp")

needs_ref = pytest.mark.skipif(not os.path.exists(REF_BOX) or shutil.which("g++") is None,
                               reason="reference sources / g++ not present")


def compile_cmd(out, extra):
    return ["g++", "-std=c++20", "-O0", "-w", f"-I{REF}/domain/include", f"-I{ROOT}/include",
            f"-I{ROOT}/sph-exa_amd/host", SRC, "-o", str(out)] + extra


@needs_ref
def test_mirror_defines_the_three_reductions(tmp_path):
    import sphexa_amd as sx

    obj = tmp_path / "obs_mirror.o"
    r = subprocess.run(compile_cmd(obj, ["-c"]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    nm = subprocess.run(["nm", "-C", str(obj)], capture_output=True, text=True, check=True).stdout
    lines = nm.splitlines()
    undefined = {ln.split(maxsplit=1)[-1] for ln in lines if ln.lstrip().startswith("U ")}
    for name, types in (("gpuGrowthRate", "<double, float, float>"), ("machSquareSumGpu", "<float, float>"),
                        ("survivorsGpu", "<float, double, float>")):
        assert not any(name in u for u in undefined), undefined
        assert any(f"sphexa::{name}{types}" in ln and " W " in ln for ln in lines), (name, nm[-3000:])
    undefined_sx = {u for u in undefined if u.startswith("sx_")}
    assert "sx_observables" in undefined_sx
    assert undefined_sx <= set(sx.header_symbols()), undefined_sx - set(sx.header_symbols())


@needs_ref
@pytest.mark.skipif(not os.path.exists(os.path.join(LIBDIR, "libsphexa_hip.so")), reason="library not built")
def test_mirror_links(tmp_path):
    exe = tmp_path / "obs_mirror"
    r = subprocess.run(compile_cmd(exe, [f"-L{LIBDIR}", "-lsphexa_hip", f"-Wl,-rpath,{LIBDIR}"]), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
