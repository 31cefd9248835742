"""Host side of the spectra (no GPU): what sx_spectrum_check refuses, and the shell tables against the oracle's."""
import numpy as np
import pytest

import spectrum_ref as sr
import sphexa_amd as sx

CUBE = ([-0.5, 0.5, 0.0, 1.0, 2.0, 3.0], [1, 1, 1])


def check(spec, lim=CUBE[0], bnd=CUBE[1]):
    sx.spectrum_check(spec, sx.make_box(lim, bnd))


@pytest.mark.parametrize("kw, box, message", [
    (dict(kind=2), CUBE, "unknown kind"),
    (dict(kind=-1), CUBE, "unknown kind"),
    (dict(weight=3), CUBE, "unknown weight"),
    (dict(weight=-1), CUBE, "unknown weight"),
    (dict(kind="scalar", weight=1), CUBE, "SX_SPEC_SCALAR takes weight 0 only"),
    (dict(n=0), CUBE, "n must be 16, 32, 64, 128 or 256"),
    (dict(n=24), CUBE, "n must be 16, 32, 64, 128 or 256"),
    (dict(n=512), CUBE, "n must be 16, 32, 64, 128 or 256"),
    (dict(), (CUBE[0], [1, 1, 0]), "periodic on all three axes"),
    (dict(), (CUBE[0], [2, 1, 1]), "periodic on all three axes"),
    (dict(), ([0.0, 1.0, 0.0, 1.0, 0.0, 1.5], [1, 1, 1]), "must be cubic"),
    (dict(), ([0.0, 1.0, 0.0, 0.999, 0.0, 1.0], [1, 1, 1]), "must be cubic"),
])
def test_spectrum_check_refuses(kw, box, message):
    with pytest.raises(sx.SxError, match=message):
        check(sx.SxSpectrum(**kw), *box)
    b = sx.make_box(*box)
    assert sx.lib().sx_spectrum_check(sx.C.byref(sx.SxSpectrum(**kw)), sx.C.byref(b)) == sx.SX_ERR_ARG


def test_spectrum_check_refuses_null():
    L = sx.lib()
    b = sx.make_box(*CUBE)
    assert L.sx_spectrum_check(None, sx.C.byref(b)) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()
    assert L.sx_spectrum_check(sx.C.byref(sx.SxSpectrum()), None) == sx.SX_ERR_ARG
    assert "null" in L.sx_last_error(None).decode()


def test_spectrum_check_accepts():
    for n in sx.SPEC_SIZES:
        for kind, weights in (("velocity", (0, 1, 2, "mean", "energy", "third")), ("scalar", (0,))):
            for w in weights:
                check(sx.SxSpectrum(kind, w, n))


@pytest.mark.parametrize("n", [16, 32, 64, 128, 256])
def test_shell_tables(n):
    _, modes = sr.shells(n)
    assert sx.spectrum_num_shells(n) == sr.num_shells(n) == modes.size
    got = sx.spectrum_modes(n)
    assert got.dtype == np.uint64 and np.array_equal(got, modes)


def test_shell_tables_refuse_other_sizes():
    assert sx.spectrum_num_shells(48) == 0 and sx.spectrum_num_shells(512) == 0
    with pytest.raises(sx.SxError, match="16, 32, 64, 128 or 256"):
        sx.spectrum_modes(48)
    assert sx.spectrum_chunk_records() == 256
