"""Images of the maps of Sim.render / Context.render_map as files, without an imaging package: 16-bit grey PGM.

    sum0, _ = sim.render("column", axis=2, npix=512)
    maps.write_pgm("sedov.pgm", maps.to_gray16(sum0))
"""
import numpy as np


def to_gray16(img, log=True, vmin=None, vmax=None):
    """img scaled to 0..65535 (uint16), linearly or in log10.  vmin, vmax default to the range of the finite (log:
    positive) pixels; pixels outside it are clipped, non-finite ones (log: non-positive too) become 0."""
    a = np.asarray(img, np.float64)
    ok = np.isfinite(a) & ((a > 0) if log else True)
    out = np.zeros(a.shape, np.uint16)
    if not ok.any():
        return out
    v = np.log10(a[ok]) if log else a[ok]
    lo = float(v.min()) if vmin is None else (np.log10(vmin) if log else float(vmin))
    hi = float(v.max()) if vmax is None else (np.log10(vmax) if log else float(vmax))
    scale = 65535.0 / (hi - lo) if hi > lo else 0.0
    out[ok] = np.rint(np.clip((v - lo) * scale, 0.0, 65535.0)).astype(np.uint16)
    return out


def write_pgm(path, img16):
    """binary PGM (P5, maxval 65535, big-endian samples) of a 2-D uint16 array; row 0 is the top line of the image, so
    pass img16[::-1] to have v grow upwards"""
    a = np.asarray(img16)
    if a.ndim != 2 or a.dtype != np.uint16:
        raise ValueError("write_pgm: a 2-D uint16 array is required (to_gray16)")
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (a.shape[1], a.shape[0]))
        f.write(a.astype(">u2").tobytes())


def read_pgm(path):
    """the array write_pgm wrote"""
    with open(path, "rb") as f:
        magic, dims, maxval = f.readline(), f.readline(), f.readline()
        if magic.strip() != b"P5" or int(maxval) != 65535:
            raise ValueError("read_pgm: not a 16-bit binary PGM")
        w, h = (int(v) for v in dims.split())
        return np.frombuffer(f.read(2 * w * h), dtype=">u2").reshape(h, w).astype(np.uint16)
