"""sph::computeStirringGpu of the C++ mirror (sph-exa_amd/host/sphexa_amd/sph_gpu.hpp) against the reference's own
declaration (sph/include/sph/hydro_turb/stirring.hpp:123-126), on the CPU, in the manner of test_mirror_compile.py:
tests/turb_mirror_compile.cpp calls it as driveTurbulence does, is compiled with g++ against the reference's headers
and linked against libsphexa_hip.so; the object's undefined sx_* symbols are functions of include/sphexa_hip.h.

Runs where /root/reference exists; skipped on the GPU box.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_STIR = os.path.join(REF, "sph", "include", "sph", "hydro_turb", "stirring.hpp")
LIBDIR = os.path.join(ROOT, "sph-exa_amd", "lib")
SRC = os.path.join(ROOT, "tests", "turb_mirror_compile.cpp")

needs_ref = pytest.mark.skipif(not os.path.exists(REF_STIR) or shutil.which("g++") is None,
                               reason="reference sources / g++ not present")


def compile_cmd(out, extra):
    return ["g++", "-std=c++20", "-O0", "-w", f"-I{REF}/domain/include", f"-I{REF}/sph/include", f"-I{ROOT}/include",
            f"-I{ROOT}/sph-exa_amd/host", SRC, "-o", str(out)] + extra


@needs_ref
def test_stirring_mirror_defines_the_reference_template(tmp_path):
    import sphexa_amd as sx

    obj = tmp_path / "turb_mirror.o"
    r = subprocess.run(compile_cmd(obj, ["-c"]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    nm = subprocess.run(["nm", "-C", str(obj)], capture_output=True, text=True, check=True).stdout
    undefined = {ln.split(maxsplit=1)[-1] for ln in nm.splitlines() if ln.lstrip().startswith("U ")}
    # the reference's template is defined here (a weak instantiation), not left for a stirring_gpu.cu to provide
    assert not any("computeStirringGpu" in u for u in undefined), undefined
    assert any("computeStirringGpu" in ln and " W " in ln for ln in nm.splitlines()), nm[-2000:]
    undefined_sx = {u for u in undefined if u.startswith("sx_")}
    assert "sx_stir_device" in undefined_sx
    assert undefined_sx <= set(sx.header_symbols()), undefined_sx - set(sx.header_symbols())


@needs_ref
@pytest.mark.skipif(not os.path.exists(os.path.join(LIBDIR, "libsphexa_hip.so")), reason="library not built")
def test_stirring_mirror_links(tmp_path):
    exe = tmp_path / "turb_mirror"
    r = subprocess.run(compile_cmd(exe, [f"-L{LIBDIR}", "-lsphexa_hip", f"-Wl,-rpath,{LIBDIR}"]), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
