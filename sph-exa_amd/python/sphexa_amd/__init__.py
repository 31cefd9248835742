"""ctypes binding of libsphexa_hip.so (include/sphexa_hip.h) -- the host-side mirror used by tests and bench.

The product is the C-ABI library; this module only marshals plain pointers.  It never falls back to a CPU
path: if the library is missing, importing `lib()` raises.
"""
import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.dirname(HERE))          # .../sph-exa_amd
ROOT = os.path.dirname(PKG)
# SPHEXA_AMD_LIB selects another in-tree build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("SPHEXA_AMD_LIB") or os.path.join(PKG, "lib", "libsphexa_hip.so")
HEADER = os.path.join(ROOT, "include", "sphexa_hip.h")

SX_OK, SX_ERR_TRAVERSAL, SX_ERR_NOT_CONVERGED, SX_ERR_HIP, SX_ERR_ARG, SX_ERR_NOMEM = range(6)
KTABLE = 20000
GROUP = 64


class SxBox(C.Structure):
    _fields_ = [("lim", C.c_double * 6), ("bnd", C.c_int32 * 3)]


class SxParams(C.Structure):
    _fields_ = [("K", C.c_double), ("ng0", C.c_uint32), ("ngmax", C.c_uint32), ("Kcour", C.c_double),
                ("Krho", C.c_double), ("gamma", C.c_double), ("muiConst", C.c_float), ("alphamin", C.c_float),
                ("alphamax", C.c_float), ("decay_constant", C.c_float), ("Atmin", C.c_float),
                ("Atmax", C.c_float), ("ramp", C.c_float), ("maxDtIncrease", C.c_double), ("avClean", C.c_int32),
                ("theta", C.c_float), ("g", C.c_double), ("eps", C.c_double), ("etaAcc", C.c_double),
                ("propagator", C.c_int32)]


_P = C.c_void_p
FIELD_ORDER = [  # sx_fields, ParticlesData order
    ("x", _P), ("y", _P), ("z", _P), ("x_m1", _P), ("y_m1", _P), ("z_m1", _P), ("vx", _P), ("vy", _P), ("vz", _P),
    ("rho", _P), ("u", _P), ("p", _P), ("prho", _P), ("tdpdTrho", _P), ("h", _P), ("m", _P), ("c", _P),
    ("ax", _P), ("ay", _P), ("az", _P), ("du", _P), ("du_m1", _P), ("c11", _P), ("c12", _P), ("c13", _P),
    ("c22", _P), ("c23", _P), ("c33", _P), ("mue", _P), ("mui", _P), ("temp", _P), ("cv", _P), ("xm", _P),
    ("kx", _P), ("divv", _P), ("curlv", _P), ("alpha", _P), ("gradh", _P), ("keys", _P), ("nc", _P),
    ("dV11", _P), ("dV12", _P), ("dV13", _P), ("dV22", _P), ("dV23", _P), ("dV33", _P), ("markRamp", _P),
    ("rung", _P)]


class SxFields(C.Structure):
    _fields_ = [("n", C.c_size_t)] + FIELD_ORDER


class SxTree(C.Structure):
    _fields_ = [("numLeafNodes", C.c_int32), ("numNodes", C.c_int32), ("prefixes", _P), ("childOffsets", _P),
                ("internalToLeaf", _P), ("levelRange", _P), ("leaves", _P), ("layout", _P), ("centers", _P),
                ("sizes", _P), ("searchExtFactor", C.c_float)]


class SxEwaldSettings(C.Structure):
    """sx_ewald_settings (ryoanji::EwaldSettings, nbody/ewald.h:15-22); the reference's defaults"""
    _fields_ = [("numReplicaShells", C.c_int), ("lCut", C.c_double), ("hCut", C.c_double), ("alphaScale", C.c_double),
                ("smallRScaleFactor", C.c_double)]

    def __init__(self, numReplicaShells=1, lCut=2.6, hCut=2.8, alphaScale=2.0, smallRScaleFactor=3.0e-3):
        super().__init__(numReplicaShells, lCut, hCut, alphaScale, smallRScaleFactor)


class SxGroups(C.Structure):
    _fields_ = [("firstBody", C.c_uint32), ("lastBody", C.c_uint32), ("numGroups", C.c_uint32),
                ("groupStart", _P), ("groupEnd", _P)]


class SxTimestep(C.Structure):
    """sph::Timestep (sph/timestep.h:38-48)"""
    _fields_ = [("nextDt", C.c_float), ("elapsedDt", C.c_float), ("totDt", C.c_float), ("numRungs", C.c_int),
                ("substep", C.c_int), ("rungRanges", C.c_uint32 * 5), ("dt_m1", C.c_float * 4),
                ("dt_drift", C.c_float * 4)]


class SxTurbSettings(C.Structure):
    """sx_turb_settings: the entries of TurbulenceConstants() (main/src/init/turbulence_init.hpp:48-71) that
    TurbulenceData::initModes reads; the defaults are the reference's"""
    _fields_ = [("solWeight", C.c_double), ("stMaxModes", C.c_uint64), ("Lbox", C.c_double),
                ("stEnergyPrefac", C.c_double), ("stMachVelocity", C.c_double), ("epsilon", C.c_double),
                ("rngSeed", C.c_uint64), ("stSpectForm", C.c_uint32), ("powerLawExp", C.c_double),
                ("anglesExp", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().sx_turb_default_settings(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown turbulence setting {k!r}")
            setattr(self, k, v)


class SxObsSettings(C.Structure):
    """sx_obs_settings: what the observables read besides the fields (factory.hpp:48-66)"""
    _fields_ = [("rhoBubble", C.c_double), ("tempWind", C.c_double), ("initialMass", C.c_double),
                ("particleMass", C.c_double), ("gravWaveTheta", C.c_double), ("gravWavePhi", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().sx_obs_default_settings(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"unknown observable setting {k!r}")
            setattr(self, k, float(v))


# the observables of observablesFactory (factory.hpp:46-69): SX_OBS_* by name, the sums sx_observables appends to the
# nine conserved ones, and the columns of the constants.txt row
OBS_KINDS = {"time_energy": 0, "mach_rms": 1, "kh_growth": 2, "wind_bubble": 3, "grav_waves": 4}
CONSERVED_SUMS = ["ecin", "eint", "px", "py", "pz", "Lx", "Ly", "Lz", "totalNeighbors"]
OBS_SUMS = {"time_energy": [], "mach_rms": ["machSquareSum"], "kh_growth": ["sumsi", "sumci", "sumdi"],
            "wind_bubble": ["survivors"], "grav_waves": ["d2xx", "d2yy", "d2zz", "d2xy", "d2xz", "d2yz"]}
_ROW_HEAD = ["iteration", "ttot", "minDt", "etot", "ecin", "eint", "egrav"]
OBS_COLUMNS = {
    "time_energy": _ROW_HEAD + ["linmom", "angmom"],
    "mach_rms": _ROW_HEAD + ["linmom", "angmom", "machRms"],
    "kh_growth": _ROW_HEAD + ["linmom", "angmom", "khgr"],
    "wind_bubble": _ROW_HEAD + ["linmom", "angmom", "bubbleFraction", "normalizedTime"],
    "grav_waves": _ROW_HEAD + ["httplus", "httcross"] + OBS_SUMS["grav_waves"],
}


def obs_kind(kind):
    """(SX_OBS_* value, name) of a kind given by name or value"""
    names = {v: k for k, v in OBS_KINDS.items()}
    if kind in OBS_KINDS:
        return OBS_KINDS[kind], kind
    if kind in names:
        return kind, names[kind]
    raise ValueError(f"unknown observable {kind!r}: one of {sorted(OBS_KINDS)}")


def grav_wave_htt(q, theta, phi):
    """(h+, hx) of the quadrupole's second derivative q = (xx, yy, zz, xy, xz, yz) (sx_grav_wave_htt: computeHtt,
    grav_waves_calculations.hpp:50-84).  Needs no GPU."""
    qq = (C.c_double * 6)(*[float(v) for v in q])
    out = (C.c_double * 2)()
    if lib().sx_grav_wave_htt(qq, float(theta), float(phi), out) != SX_OK:
        raise SxError("sx_grav_wave_htt failed")
    return out[0], out[1]


def obs_finalize(kind, sums, num_particles_global, settings=None):
    """the observable's values from the global sums of Context.observables (sx_obs_finalize): [] for time_energy,
    [machRms], [khgr], [bubbleFraction] or [h+, hx].  Needs no GPU."""
    k, name = obs_kind(kind)
    settings = settings if settings is not None else SxObsSettings()
    s = np.ascontiguousarray([sums[n] for n in CONSERVED_SUMS + OBS_SUMS[name]] if isinstance(sums, dict) else sums,
                             dtype=np.float64)
    if s.size != 9 + len(OBS_SUMS[name]):
        raise ValueError(f"{name}: {9 + len(OBS_SUMS[name])} sums expected, got {s.size}")
    out = (C.c_double * 2)()
    rc = lib().sx_obs_finalize(k, C.byref(settings), s.ctypes.data_as(C.POINTER(C.c_double)),
                               int(num_particles_global), out)
    if rc != SX_OK:
        raise SxError(f"sx_obs_finalize: code {rc}")
    return list(out)[:{"time_energy": 0, "grav_waves": 2}.get(name, 1)]


def format_constants_row(row, kind):
    """the line fileutils::writeColumns(out, ' ', ...) writes for a row of Sim.observe (main/src/io/file_utils.hpp:14-18):
    every column preceded by one separator, the iteration an integer, doubles in the stream's default format (%g)"""
    _, name = obs_kind(kind)
    cols = OBS_COLUMNS[name]
    vals = [row[c] for c in cols] if isinstance(row, dict) else list(row)
    if len(vals) != len(cols):
        raise ValueError(f"{name}: {len(cols)} columns expected, got {len(vals)}")
    return "".join([" %d" % int(vals[0])] + [" %g" % float(v) for v in vals[1:]]) + "\n"


class SxMap(C.Structure):
    """sx_map: an image plane with normal `axis` (0 x, 1 y, 2 z; in-plane axes u, v = its cyclic successors), the window
    centre (its normal component: the slice plane / slab centre), the extent along u and v, the slab thickness of a
    column map (0: unbounded) and the pixels along u and v"""
    _fields_ = [("kind", C.c_int32), ("axis", C.c_int32), ("center", C.c_double * 3), ("width", C.c_double * 2),
                ("depth", C.c_double), ("npix", C.c_uint32 * 2)]

    def __init__(self, kind="column", axis=2, center=(0.0, 0.0, 0.0), width=(1.0, 1.0), depth=0.0, npix=(512, 512)):
        npix = (npix, npix) if np.isscalar(npix) else npix
        width = (width, width) if np.isscalar(width) else width
        super().__init__(MAP_KINDS.get(kind, kind), int(axis), (C.c_double * 3)(*[float(v) for v in center]),
                         (C.c_double * 2)(*[float(v) for v in width]), float(depth),
                         (C.c_uint32 * 2)(*[int(v) for v in npix]))

    @property
    def shape(self):
        """the image as a numpy shape: npix[1] rows of npix[0]"""
        return int(self.npix[1]), int(self.npix[0])


MAP_KINDS = {"column": 0, "slice": 1}
# the column a of Sim.render (SX_MAP_FIELD_*)
MAP_FIELDS = {None: 0, "none": 0, "temp": 1, "p": 2, "c": 3, "vx": 4, "vy": 5, "vz": 6, "divv": 7, "curlv": 8,
              "alpha": 9, "h": 10}


def map_check(spec, box):
    """sx_map_check: raises SxError with the reason for a specification a render would refuse.  Needs no GPU."""
    if lib().sx_map_check(C.byref(spec), C.byref(box)) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())


def map_kernel(t):
    """the column maps' line-of-sight kernel Y(t), t = q^2, as the device evaluates it (sx_map_kernel).  Needs no GPU."""
    t = np.ascontiguousarray(t, dtype=np.float32)
    y = np.empty_like(t)
    lib().sx_map_kernel(t.ctypes.data, t.size, y.ctypes.data)
    return y


def pair_bands(row_counts, cap=0):
    """the bands [(r0, r1), ...] the maps and the mesh deposit make of rows with these pair counts under a pair cap
    (0: the default): sx_pair_bands_internal, the planner on its own.  Raises SxError with the code and the refusal.
    Needs no GPU."""
    counts = np.ascontiguousarray(row_counts, dtype=np.uint64)
    r0r1 = np.zeros(2 * max(counts.size, 1), np.int32)
    nb = C.c_int()
    rc = lib().sx_pair_bands_internal(counts.ctypes.data, counts.size, int(cap), r0r1.ctypes.data, C.byref(nb))
    if rc != SX_OK:
        raise SxError(f"sx_pair_bands_internal: code {rc}: {lib().sx_last_error(None).decode()}")
    return [(int(r0r1[2 * k]), int(r0r1[2 * k + 1])) for k in range(nb.value)]


def map_chunk_records():
    """records per LDS chunk of the render kernel (sx_map_chunk_records)"""
    return int(lib().sx_map_chunk_records())


class SxSpectrum(C.Structure):
    """sx_spectrum: kind ("velocity" or "scalar"), weight (the p of W = S0^p S1 / S0: 0, 1 for 1/2, 2 for 1/3; "mean",
    "energy", "third") and the cells per axis n"""
    _fields_ = [("kind", C.c_int32), ("weight", C.c_int32), ("n", C.c_uint32)]

    def __init__(self, kind="velocity", weight=0, n=128):
        super().__init__(SPEC_KINDS.get(kind, kind), SPEC_WEIGHTS.get(weight, weight), int(n))

    @property
    def prefactor(self):
        return 0.5 if self.kind == 0 else 1.0


SPEC_KINDS = {"velocity": 0, "scalar": 1}
SPEC_WEIGHTS = {None: 0, "mean": 0, "energy": 1, "third": 2}
SPEC_SIZES = (16, 32, 64, 128, 256)


def spectrum_check(spec, box):
    """sx_spectrum_check: raises SxError with the reason for a specification a call would refuse.  Needs no GPU."""
    if lib().sx_spectrum_check(C.byref(spec), C.byref(box)) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())


def spectrum_num_shells(n):
    """floor(sqrt(3) n / 2 + 1/2) + 1 (sx_spectrum_num_shells; 0 for an n that is not a mesh size).  Needs no GPU."""
    return int(lib().sx_spectrum_num_shells(int(n)))


def spectrum_modes(n):
    """wave vectors per shell (sx_spectrum_modes), uint64.  Needs no GPU."""
    out = np.zeros(max(1, spectrum_num_shells(n)), np.uint64)
    if lib().sx_spectrum_modes(int(n), out.ctypes.data) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())
    return out


def spectrum_chunk_records():
    """records per LDS chunk of the mesh gather (sx_spectrum_chunk_records)"""
    return int(lib().sx_spectrum_chunk_records())


PROF_COORDS = {"radius": 0, "x": 1, "y": 2, "z": 3, "quantity": 4}
PROF_QUANTITIES = {"rho": 0, "p": 1, "u": 2, "temp": 3, "vel": 4, "vrad": 5, "c": 6, "h": 7, "divv": 8, "curlv": 9,
                   "alpha": 10}
PROF_WEIGHTS = {"number": 0, "mass": 1}
PROF_SOLUTIONS = {"none": 0, "table": 1, "noh": 2}
PROF_MAX_Q = 4


class SxProfileSolution(C.Structure):
    """sx_profile_solution: "table" (r, y ascending in r, evaluated as numpy.interp at c * rscale) or "noh" (the closed
    form of the Noh density with gamma, rho0, vel0, time, xgeom)"""
    _fields_ = [("kind", C.c_int32), ("nt", C.c_uint32), ("r", C.c_void_p), ("y", C.c_void_p), ("rscale", C.c_double),
                ("gamma", C.c_double), ("rho0", C.c_double), ("vel0", C.c_double), ("time", C.c_double),
                ("xgeom", C.c_int32)]


class SxProfile(C.Structure):
    """sx_profile: the bin coordinate ("radius", "x", "y", "z", or a quantity name: then coord is "quantity"), the
    weight ("number" or "mass"), the centre, the edges (nbins + 1, ascending), up to four quantities (names of
    PROF_QUANTITIES) and per quantity a solution: None, ("table", r, y[, rscale]) or ("noh", dict(time=, gamma=5/3,
    rho0=1, vel0=-1, xgeom=3, rscale=1)).  The arrays are kept alive by the object."""
    _fields_ = [("coord", C.c_int32), ("coordQ", C.c_int32), ("weight", C.c_int32), ("center", C.c_double * 3),
                ("nbins", C.c_uint32), ("edges", C.c_void_p), ("nq", C.c_uint32), ("q", C.c_int32 * PROF_MAX_Q),
                ("sol", SxProfileSolution * PROF_MAX_Q)]

    def __init__(self, edges=(0.0, 1.0), quantities=("rho",), coord="radius", center=(0.0, 0.0, 0.0), weight="number",
                 solutions=None):
        super().__init__()
        if coord in PROF_QUANTITIES:
            self.coord, self.coordQ = PROF_COORDS["quantity"], PROF_QUANTITIES[coord]
        else:
            self.coord = PROF_COORDS.get(coord, coord)
        self.weight = PROF_WEIGHTS.get(weight, weight)
        for k in range(3):
            self.center[k] = float(center[k])
        self._keep = [np.ascontiguousarray(edges, dtype=np.float64)]
        self.nbins = max(0, self._keep[0].size - 1)
        self.edges = self._keep[0].ctypes.data
        self.names = [q if isinstance(q, str) else PROF_QUANTITIES_BY_CODE.get(q, str(q)) for q in quantities]
        self.nq = len(quantities)
        for k, q in enumerate(list(quantities)[:PROF_MAX_Q]):
            self.q[k] = PROF_QUANTITIES.get(q, q)
        for name, sol in (solutions or {}).items():
            self.set_solution(self.names.index(name) if isinstance(name, str) else int(name), sol)

    def set_solution(self, slot, sol):
        s = self.sol[slot]
        if sol is None:
            s.kind = 0
        elif sol[0] == "table":
            r, y = (np.ascontiguousarray(v, dtype=np.float64) for v in sol[1:3])
            if r.size != y.size:
                raise ValueError("a table's r and y differ in length")
            self._keep += [r, y]
            s.kind, s.nt, s.r, s.y = 1, r.size, r.ctypes.data, y.ctypes.data
            s.rscale = float(sol[3]) if len(sol) > 3 else 1.0
        elif sol[0] == "noh":
            kw = dict(gamma=5.0 / 3.0, rho0=1.0, vel0=-1.0, xgeom=3, rscale=1.0)
            kw.update(sol[1])
            s.kind, s.rscale, s.gamma, s.rho0, s.vel0 = 2, kw["rscale"], kw["gamma"], kw["rho0"], kw["vel0"]
            s.time, s.xgeom = kw["time"], kw["xgeom"]
        else:
            raise ValueError(f"unknown solution {sol[0]!r}: 'table' or 'noh'")


PROF_QUANTITIES_BY_CODE = {v: k for k, v in PROF_QUANTITIES.items()}


class SxProfileResult(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("count", "nonfinite", "W", "S1", "S2", "D", "min", "max")]


def profile_check(spec, box):
    """sx_profile_check: raises SxError with the reason for a specification a call would refuse.  Needs no GPU."""
    if lib().sx_profile_check(C.byref(spec) if spec is not None else None, C.byref(box) if box is not None else None) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())


def profile_lds_bins(nq):
    """the largest nbins whose bins of nq quantities are accumulated in LDS (sx_profile_lds_bins)"""
    return int(lib().sx_profile_lds_bins(int(nq)))


def profile_window(t):
    """the window E of the terms t: the smallest E with max |t| < 2^E, -1074 for zeros (sx_profile_window)"""
    t = np.ascontiguousarray(t, dtype=np.float64)
    E = C.c_int32()
    if lib().sx_profile_window(t.ctypes.data, t.size, C.byref(E)) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())
    return E.value


def profile_to_fixed(t, E):
    """fixed(t) of window E as (n, 2) uint64: low and high word of the 128-bit integer (sx_profile_to_fixed)"""
    t = np.ascontiguousarray(t, dtype=np.float64)
    out = np.zeros((t.size, 2), np.uint64)
    if lib().sx_profile_to_fixed(t.ctypes.data, t.size, int(E), out.ctypes.data) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())
    return out


def profile_add_fixed(lohi, acc=(0, 0)):
    """acc + the integers of lohi modulo 2^128, as (low, high) Python ints (sx_profile_add_fixed)"""
    lohi = np.ascontiguousarray(lohi, dtype=np.uint64)
    a = (C.c_uint64 * 2)(int(acc[0]), int(acc[1]))
    if lib().sx_profile_add_fixed(a, lohi.ctypes.data, lohi.size // 2) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())
    return int(a[0]), int(a[1])


def profile_from_fixed(acc, E):
    """the double nearest to acc 2^(E - 96), acc = (low, high) (sx_profile_from_fixed)"""
    a = (C.c_uint64 * 2)(int(acc[0]), int(acc[1]))
    out = C.c_double()
    if lib().sx_profile_from_fixed(a, int(E), C.byref(out)) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())
    return out.value


def profile_dict(spec, res):
    """the packed arrays of a profile call as the dict Sim.profile returns"""
    nb, nq = int(spec.nbins), int(spec.nq)
    out = {"edges": spec._keep[0].copy(), "count": res["count"][:nb], "under": int(res["count"][nb]),
           "over": int(res["count"][nb + 1]), "nonfinite": int(res["nonfinite"][0]), "W": res["W"][:nb],
           "raw": res}
    wsum = 0.0
    for w in res["W"]:
        wsum += float(w)
    for key in ("mean", "sum", "sum2", "min", "max", "dev", "l1"):
        out[key] = {}
    for k, name in enumerate(spec.names):
        s1 = res["S1"][k]
        out["sum"][name], out["sum2"][name] = s1[:nb], res["S2"][k][:nb]
        out["min"][name], out["max"][name] = res["min"][k][:nb], res["max"][k][:nb]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["mean"][name] = s1[:nb] / res["W"][:nb]
        if spec.sol[k].kind:
            out["dev"][name] = res["D"][k][:nb]
            d = 0.0
            for v in res["D"][k]:
                d += float(v)
            out["l1"][name] = d / wsum if wsum else float("nan")
    return out


class SxFof(C.Structure):
    """sx_fof: the absolute linking length, the smallest group the catalogue lists, the catalogue's capacity"""
    _fields_ = [("linking", C.c_double), ("minMembers", C.c_uint32), ("maxGroups", C.c_uint32)]

    def __init__(self, linking=0.0, min_members=20, max_groups=4096):
        super().__init__(float(linking), int(min_members), int(max_groups))


class SxFofResult(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("label", "groupLabel", "groupCount", "groupMass", "groupCom", "groupVel",
                                          "numGroups")]


def fof_check(spec, box):
    """sx_fof_check: raises SxError with the reason for a specification a call would refuse.  Needs no GPU."""
    if lib().sx_fof_check(C.byref(spec) if spec is not None else None, C.byref(box) if box is not None else None) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())


def fof_grid(spec, box, n):
    """the cells per axis a call on n particles uses (sx_fof_grid).  Needs no GPU."""
    dims = (C.c_uint32 * 3)()
    if lib().sx_fof_grid(C.byref(spec) if spec is not None else None, C.byref(box) if box is not None else None,
                         int(n), dims) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())
    return tuple(int(d) for d in dims)


def _fof_arrays(n, cap, labels):
    """host arrays of a group-finder call: name -> (array, sx_fof_result member)"""
    out = {"group_label": (np.zeros(max(1, cap), np.uint64), "groupLabel"),
           "count": (np.zeros(max(1, cap), np.uint32), "groupCount"),
           "mass": (np.zeros(max(1, cap), np.float64), "groupMass"),
           "com": (np.zeros((max(1, cap), 3), np.float64), "groupCom"),
           "vel": (np.zeros((max(1, cap), 3), np.float64), "groupVel"),
           "num": (np.zeros(2, np.uint64), "numGroups")}
    if labels:
        out["label"] = (np.zeros(max(1, n), np.uint64), "label")
    return out


def _fof_dict(arr, n, cap):
    """the dict Context.fof and Sim.fof return from the filled arrays of _fof_arrays"""
    num = arr["num"][0]
    k = min(int(num[0]), int(cap))
    out = {"num_groups": int(num[0]), "num_all": int(num[1]), "label": arr["label"][0][:n] if "label" in arr else None}
    for key in ("group_label", "count", "mass", "com", "vel"):
        out[key] = arr[key][0][:k]
    return out


HALO_FLAGS = {"moments": 1, "thermal": 2, "potential": 4}


def halo_flags(names):
    """the SX_HALO_* bits of an iterable of names ("moments", "thermal", "potential") or of an int"""
    if isinstance(names, int):
        return names
    bits = 0
    for k in names:
        if k not in HALO_FLAGS:
            raise ValueError(f"unknown group property {k!r}: one of {sorted(HALO_FLAGS)}")
        bits |= HALO_FLAGS[k]
    return bits


class SxHalo(C.Structure):
    """sx_halo: sx_fof's three, the density cut (rho_min <= 0: none; std: the rho column instead of kx m / xm), G, the
    flags, muiConst and gamma of the thermal energy, and the largest group that still gets a potential (0: 2^20)"""
    _fields_ = [("linking", C.c_double), ("minMembers", C.c_uint32), ("maxGroups", C.c_uint32), ("rhoMin", C.c_double),
                ("std", C.c_int32), ("G", C.c_float), ("flags", C.c_uint32), ("muiConst", C.c_float),
                ("gamma", C.c_double), ("maxPairMembers", C.c_uint32)]

    def __init__(self, linking=0.0, min_members=20, max_groups=4096, rho_min=0.0, std=False, G=1.0,
                 flags=("moments", "potential"), mui_const=10.0, gamma=5.0 / 3.0, max_pair_members=0):
        super().__init__(float(linking), int(min_members), int(max_groups), float(rho_min), int(bool(std)), float(G),
                         halo_flags(flags), float(mui_const), float(gamma), int(max_pair_members))


class SxHaloResult(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("label", "groupLabel", "groupCount", "groupMass", "groupCom", "groupVel",
                                          "numGroups", "groupSigma", "groupShape", "groupAngmom", "groupRmax",
                                          "groupEint", "groupEpot")]


def halo_check(spec, box):
    """sx_halo_check: raises SxError with the reason for a specification a call would refuse.  Needs no GPU."""
    if lib().sx_halo_check(C.byref(spec) if spec is not None else None, C.byref(box) if box is not None else None) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())


#: key of the dict -> (sx_halo_result member, trailing shape, flag)
_HALO_EXTRA = {"sigma": ("groupSigma", (6,), 1), "shape": ("groupShape", (6,), 1), "angmom": ("groupAngmom", (3,), 1),
               "rmax": ("groupRmax", (), 1), "eint": ("groupEint", (), 2), "epot": ("groupEpot", (), 4)}


def _halo_arrays(n, cap, labels, flags):
    """host arrays of a group-property call: those of _fof_arrays and, for the flags that are set, the properties
    (filled with NaN: an entry the call does not write stays NaN)"""
    out = _fof_arrays(n, cap, labels)
    for key, (member, tail, bit) in _HALO_EXTRA.items():
        if flags & bit:
            out[key] = (np.full((max(1, cap),) + tail, np.nan), member)
    return out


def _halo_dict(arr, n, cap, flags):
    """the dict Context.halos and Sim.halos return: _fof_dict's and the properties, then what follows from them: ekin =
    0.5 M (sigma_xx + sigma_yy + sigma_zz), alpha_vir = 2 ekin / |epot|, bound = ekin + eint + epot < 0 (eint 0 without
    the thermal flag), axes = the eigenvalues of shape, ascending"""
    out = _fof_dict(arr, n, cap)
    k = len(out["count"])
    for key in _HALO_EXTRA:
        out[key] = arr[key][0][:k] if key in arr else None
    if flags & 1:
        sg, sh = out["sigma"], out["shape"]
        out["ekin"] = 0.5 * out["mass"] * (sg[:, 0] + sg[:, 3] + sg[:, 5])
        full = sh[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(k, 3, 3)
        out["axes"] = np.linalg.eigvalsh(full) if k else np.zeros((0, 3))
    else:
        out["ekin"] = out["axes"] = None
    if flags & 1 and flags & 4:
        with np.errstate(divide="ignore", invalid="ignore"):
            out["alpha_vir"] = 2.0 * out["ekin"] / np.abs(out["epot"])
        out["bound"] = out["ekin"] + (out["eint"] if flags & 2 else 0.0) + out["epot"] < 0.0
    else:
        out["alpha_vir"] = out["bound"] = None
    return out


class SxTwoPoint(C.Structure):
    """sx_twopoint: the bin edges (kept alive here), the series flags, and the target rule key % stride == phase"""
    _fields_ = [("edges", C.c_void_p), ("nbins", C.c_uint32), ("series", C.c_uint32), ("stride", C.c_uint32),
                ("phase", C.c_uint32)]

    def __init__(self, edges=None, series=("count", "vel"), stride=1, phase=0, mass=False):
        e = np.ascontiguousarray(edges if edges is not None else [], dtype=np.float64)
        self._keep = e
        super().__init__(e.ctypes.data if e.size else None, max(0, e.size - 1),
                         twopoint_flags(series) | (TP_FLAGS["WW"] if mass else 0), int(stride), int(phase))


class SxTwoPointResult(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("count", "U1", "U2", "U3", "A3", "T2", "WW", "totals")]


TP_SERIES = ("U1", "U2", "U3", "A3", "T2", "WW")
TP_FLAGS = {k: 1 << i for i, k in enumerate(TP_SERIES)}
TP_VEL = 31


def twopoint_flags(series):
    """the flag word of a list of series names: "count" (always on), "vel" (the five velocity series), "mass" or one of
    U1 U2 U3 A3 T2 WW; an integer is passed through"""
    if isinstance(series, int):
        return series
    flags = 0
    for name in series:
        if name == "count":
            continue
        if name == "vel":
            flags |= TP_VEL
        elif name == "mass":
            flags |= TP_FLAGS["WW"]
        elif name in TP_FLAGS:
            flags |= TP_FLAGS[name]
        else:
            raise ValueError(f"twopoint: unknown series {name!r}")
    return flags


def twopoint_check(spec, box):
    """sx_twopoint_check: raises SxError with the reason for a specification a call would refuse.  Needs no GPU."""
    if lib().sx_twopoint_check(C.byref(spec) if spec is not None else None,
                               C.byref(box) if box is not None else None) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())


def twopoint_grid(spec, box, n):
    """the cells per axis a call on n particles uses (sx_twopoint_grid).  Needs no GPU."""
    dims = (C.c_uint32 * 3)()
    if lib().sx_twopoint_grid(C.byref(spec) if spec is not None else None, C.byref(box) if box is not None else None,
                              int(n), dims) != SX_OK:
        raise SxError(lib().sx_last_error(None).decode())
    return tuple(int(d) for d in dims)


def _twopoint_arrays(spec):
    """host arrays of a two-point call: sx_twopoint_result member -> array; the series that are off keep their NaNs"""
    nb = max(1, int(spec.nbins))
    out = {"count": np.zeros(nb, np.uint64), "totals": np.zeros(3, np.uint64)}
    for k in TP_SERIES:
        out[k] = np.full(nb, np.nan, np.float64)
    return out


def twopoint_dict(spec, arr, box, n):
    """the dict Context.twopoint and Sim.twopoint return from the filled arrays of _twopoint_arrays over n particles"""
    nb = int(spec.nbins)
    edges = spec._keep.copy()
    count = arr["count"][:nb]
    targets, nonfinite, coincident = (int(v) for v in arr["totals"])
    out = {"edges": edges, "count": count, "targets": targets, "nonfinite": nonfinite, "coincident": coincident,
           "raw": arr}
    for k in TP_SERIES:
        out[k] = arr[k][:nb] if spec.series & TP_FLAGS[k] else None
    with np.errstate(divide="ignore", invalid="ignore"):
        cnt = count.astype(np.float64)
        for name, k in (("s1", "U1"), ("s2", "U2"), ("s3", "U3"), ("s3abs", "A3"), ("dv2", "T2")):
            out[name] = out[k] / cnt if out[k] is not None else None
    out["ww"] = out["WW"]
    nf = int(n) - nonfinite
    out["pairs_expected"] = targets * (nf - 1) - targets * (targets - 1) // 2
    out["xi"] = None
    if all(int(b) == 1 for b in box.bnd):
        lim = box.lim
        vol = (lim[1] - lim[0]) * (lim[3] - lim[2]) * (lim[5] - lim[4])
        shell = (4.0 * np.pi / 3.0) * (edges[1:] ** 3 - edges[:-1] ** 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["xi"] = cnt / (out["pairs_expected"] * shell / vol) - 1.0
    return out


class SxOctree(C.Structure):
    _fields_ = [("prefixes", _P), ("childOffsets", _P), ("parents", _P), ("levelRange", _P),
                ("internalToLeaf", _P), ("leafToInternal", _P)]


class SxNbStats(C.Structure):
    _fields_ = [("sumNeighbors", C.c_uint64), ("maxNeighbors", C.c_uint32), ("numFailed", C.c_uint32),
                ("sumCandidates", C.c_uint64), ("sumUnion", C.c_uint64), ("build", C.c_uint32),
                ("maxUnion", C.c_uint32)]


# field dtypes (sph::SphTypes, sph/types.hpp:39-46)
DTYPES = {k: np.float32 for k, _ in FIELD_ORDER}
DTYPES.update(x=np.float64, y=np.float64, z=np.float64, u=np.float64, du=np.float64, temp=np.float64,
              keys=np.uint64, nc=np.uint32, rung=np.uint8)

_lib = None

# host-staged transport callbacks (sx_alltoallv_cb / sx_allreduce_cb)
ALLTOALLV_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p,
                           C.POINTER(C.c_uint64))
ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int)


def header_symbols():
    """every sx_* function declared in include/sphexa_hip.h"""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sx_[a-z0-9_]+)\s*\(", txt)))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not built (run __graft_entry__.build() or make -C sph-exa_amd)")
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t
    sig = {
        "sx_create": (C.c_int, [C.POINTER(vp), C.c_int]),
        "sx_destroy": (None, [vp]),
        "sx_set_stream": (C.c_int, [vp, vp]),
        "sx_get_stream": (vp, [vp]),
        "sx_last_error": (C.c_char_p, [vp]),
        "sx_set_exact": (C.c_int, [vp, C.c_int]),
        "sx_kernel_constant": (C.c_double, []),
        "sx_copy_tables": (C.c_int, [vp, vp, vp]),
        "sx_kernel_poly": (C.c_int, [vp, C.c_size_t, vp, vp]),
        "sx_set_pack12_max": (C.c_int, [vp, u32]),
        "sx_pack12_row_words": (u32, [u32]),
        "sx_pack12_pack": (C.c_int, [vp, u32, vp]),
        "sx_pack12_unpack": (C.c_int, [vp, u32, vp]),
        "sx_synchronize": (C.c_int, [vp]),
        "sx_device_alloc": (vp, [vp, sz]),
        "sx_device_free": (C.c_int, [vp, vp]),
        "sx_memcpy": (C.c_int, [vp, vp, vp, sz, C.c_int]),
        "sx_memset": (C.c_int, [vp, vp, C.c_int, sz]),
        "sx_sfc_keys": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(SxBox)]),
        "sx_sort_keys": (C.c_int, [vp, vp, vp, sz]),
        "sx_gather": (C.c_int, [vp, vp, sz, vp, vp, C.c_int]),
        "sx_compute_octree": (C.c_int, [vp, vp, sz, u32, vp, vp, i32, C.POINTER(i32)]),
        "sx_build_octree": (C.c_int, [vp, vp, i32, C.POINTER(SxOctree)]),
        "sx_node_centers": (C.c_int, [vp, vp, i32, C.POINTER(SxBox), vp, vp]),
        "sx_leaf_layout": (C.c_int, [vp, vp, i32, vp]),
        "sx_compute_groups": (C.c_int, [vp, u32, u32, C.POINTER(SxGroups)]),
        "sx_set_search_mode": (C.c_int, [vp, C.c_int]),
        "sx_mark_ramp": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                   C.POINTER(SxBox), vp]),
        "sx_positions_rungs": (C.c_int, [vp, C.POINTER(SxGroups), C.c_float, vp, vp, C.POINTER(SxFields), C.c_double,
                                         C.c_double, C.POINTER(SxBox)]),
        "sx_drift_positions": (C.c_int, [vp, C.POINTER(SxGroups), C.c_float, C.c_float, vp, vp, C.POINTER(SxFields),
                                         C.c_double, C.c_double]),
        "sx_group_divv_timestep": (C.c_int, [vp, C.c_float, C.POINTER(SxGroups), vp, vp]),
        "sx_group_acc_timestep": (C.c_int, [vp, C.c_float, C.POINTER(SxGroups), vp, vp, vp, vp]),
        "sx_store_rung": (C.c_int, [vp, C.POINTER(SxGroups), C.c_uint8, vp]),
        "sx_rung_timestep": (C.c_int, [vp, vp, vp, u32, C.c_float, vp, C.POINTER(SxTimestep)]),
        "sx_minimum_group_dt": (C.c_int, [vp, C.POINTER(SxTimestep), vp, vp, u32, vp, C.POINTER(C.c_float), vp]),
        "sx_extract_groups": (C.c_int, [vp, C.POINTER(SxGroups), vp, u32, u32, vp, vp]),
        "sx_spatial_groups": (C.c_int, [vp, u32, u32, vp, vp, vp, C.POINTER(SxTree), C.POINTER(SxBox), C.c_float,
                                        vp, u32, C.POINTER(SxGroups)]),
        "sx_find_neighbors": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxTree), C.POINTER(SxBox),
                                        C.POINTER(SxParams), u32, u32, C.c_int, C.POINTER(SxNbStats)]),
        "sx_export_neighbors": (C.c_int, [vp, vp, u32, u32, u32, vp]),
        "sx_import_neighbors": (C.c_int, [vp, u32, u32, u32, vp]),
        "sx_xmass": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams), C.POINTER(SxBox),
                               C.POINTER(SxTree)]),
        "sx_xmass_only": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                    C.POINTER(SxBox)]),
        "sx_ve_def_gradh": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                      C.POINTER(SxBox)]),
        "sx_eos": (C.c_int, [vp, u32, u32, C.c_float, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sx_iad_divv_curlv": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                        C.POINTER(SxBox)]),
        "sx_av_switches": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                     C.POINTER(SxBox), C.c_double]),
        "sx_momentum_energy": (C.c_int, [vp, C.POINTER(SxGroups), vp, C.POINTER(SxFields), C.POINTER(SxParams),
                                         C.POINTER(SxBox), C.POINTER(C.c_float)]),
        "sx_momentum_energy_avclean": (C.c_int, [vp, C.POINTER(SxGroups), vp, C.POINTER(SxFields),
                                                 C.POINTER(SxParams), C.POINTER(SxBox), C.POINTER(C.c_float)]),
        "sx_density": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                 C.POINTER(SxBox), C.POINTER(SxTree)]),
        "sx_density_only": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                      C.POINTER(SxBox)]),
        "sx_eos_std": (C.c_int, [vp, u32, u32, C.c_float, C.c_double, vp, vp, vp, vp, vp]),
        "sx_iad": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams), C.POINTER(SxBox)]),
        "sx_momentum_energy_std": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxParams),
                                             C.POINTER(SxBox), C.POINTER(C.c_float)]),
        "sx_positions": (C.c_int, [vp, u32, u32, C.c_double, C.c_double, C.POINTER(SxFields), C.c_double,
                                   C.c_float, C.POINTER(SxBox)]),
        "sx_nbody_positions": (C.c_int, [vp, u32, u32, C.c_double, C.c_double, C.POINTER(SxFields), C.POINTER(SxBox),
                                         vp]),
        "sx_update_h": (C.c_int, [vp, u32, u32, u32, vp, vp]),
        "sx_update_h_groups": (C.c_int, [vp, vp, u32, vp, vp]),
        "sx_max_divv": (C.c_int, [vp, u32, u32, vp, C.POINTER(C.c_float)]),
        "sx_sim_create": (C.c_int, [C.POINTER(vp), vp, sz, C.POINTER(SxParams), C.POINTER(SxBox), u32]),
        "sx_sim_destroy": (None, [vp]),
        "sx_sim_init_sedov": (C.c_int, [vp, u32]),
        "sx_sim_set_state": (C.c_int, [vp, sz] + [vp] * 15 + [C.c_double, C.c_double]),
        "sx_sim_fields": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(vp)]),
        "sx_sim_size": (sz, [vp]),
        "sx_sim_step": (C.c_int, [vp]),
        "sx_sim_scalars": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_char_p)]),
        "sx_sim_last_stats": (C.c_int, [vp, C.POINTER(SxNbStats)]),
        "sx_sim_kernel_times": (C.c_int, [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_char_p)]),
        "sx_sim_set_comm": (C.c_int, [vp, vp]),
        "sx_sim_gravity_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_sim_gravity_interactions": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_sim_set_gravity_counting": (C.c_int, [vp, C.c_int]),
        "sx_sim_set_gravity_check": (C.c_int, [vp, u32]),
        "sx_sim_gravity_check": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_conserved": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_conserved_quantities": (C.c_int, [vp, C.POINTER(SxFields), u32, u32, C.c_float, C.c_double,
                                              C.POINTER(C.c_double)]),
        "sx_sim_init_sedov_rank": (C.c_int, [vp, u32, C.c_int, C.c_int]),
        "sx_sim_layout": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_sim_memory": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_sim_set_overlap": (C.c_int, [vp, C.c_int]),
        "sx_sim_overlap_stats": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "sx_sim_timestep": (C.c_int, [vp, C.POINTER(SxTimestep)]),
        "sx_sim_set_timestep": (C.c_int, [vp, C.POINTER(SxTimestep), vp]),
        "sx_sim_set_time": (C.c_int, [vp, C.c_double]),
        "sx_sim_set_skin": (C.c_int, [vp, C.c_float, C.c_int]),
        "sx_sim_rebuild_lists": (C.c_int, [vp]),
        "sx_sim_skin_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_sim_export_neighbors": (C.c_int, [vp, vp]),
        "sx_comm_unique_id": (C.c_int, [vp]),
        "sx_comm_create_rccl": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, vp]),
        "sx_comm_create_host": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, ALLTOALLV_CB, ALLREDUCE_CB, vp]),
        "sx_comm_destroy": (None, [vp]),
        "sx_comm_alltoallv": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "sx_comm_allreduce": (C.c_int, [vp, vp, C.c_uint64, C.c_int, vp]),
        "sx_domain_splitters": (C.c_int, [vp, u32, C.c_int, vp]),
        "sx_gravity_upsweep": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxTree), C.c_float, vp, vp]),
        "sx_gravity_traverse": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxTree),
                                          C.POINTER(SxBox), vp, vp, C.c_float, C.POINTER(C.c_double)]),
        "sx_gravity_traverse_pbc": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxTree),
                                              C.POINTER(SxBox), vp, vp, C.c_float, C.c_int, C.POINTER(C.c_double)]),
        "sx_gravity_ewald": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxBox), vp, vp,
                                       C.c_float, C.POINTER(SxEwaldSettings), C.POINTER(C.c_double)]),
        "sx_gravity_direct": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.POINTER(SxBox), C.c_int,
                                        C.c_float, vp, C.POINTER(C.c_double)]),
        "sx_set_direct_splits": (C.c_int, [vp, u32]),
        "sx_ctx_direct_targets_per_lane_internal": (C.c_int, [vp, u32]),
        "sx_sim_set_skin_frozen_stage_internal": (C.c_int, [vp, u32]),
        "sx_domain_halo_layout": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint64, vp, vp]),
        "sx_turb_default_settings": (C.c_int, [C.POINTER(SxTurbSettings)]),
        "sx_turb_create": (C.c_int, [C.POINTER(vp), C.POINTER(SxTurbSettings)]),
        "sx_turb_destroy": (None, [vp]),
        "sx_turb_num_modes": (C.c_uint64, [vp]),
        "sx_turb_get_scalars": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_turb_get_arrays": (C.c_int, [vp, vp, vp, vp]),
        "sx_turb_get_rng": (C.c_int64, [vp, C.c_char_p, sz]),
        "sx_turb_set_state": (C.c_int, [vp, C.POINTER(C.c_double), C.c_uint64, vp, vp, vp, C.c_char_p]),
        "sx_turb_max_index": (C.c_int, [vp]),
        "sx_turb_fast_limit": (C.c_int, []),
        "sx_turb_update_noise": (C.c_int, [vp, C.c_double]),
        "sx_turb_compute_phases": (C.c_int, [vp, vp, vp]),
        "sx_stir": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), vp]),
        "sx_stir_device": (C.c_int, [vp, C.POINTER(SxGroups), C.POINTER(SxFields), C.c_uint64, vp, vp, vp, vp,
                                     C.c_double]),
        "sx_sim_set_turbulence": (C.c_int, [vp, C.POINTER(SxTurbSettings)]),
        "sx_sim_turbulence": (C.c_int, [vp, C.POINTER(vp)]),
        "sx_sim_set_turbulence_state": (C.c_int, [vp, C.POINTER(C.c_double), C.c_uint64, vp, vp, vp, C.c_char_p]),
        "sx_sim_turbulence_times": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "sx_obs_default_settings": (C.c_int, [C.POINTER(SxObsSettings)]),
        "sx_obs_num_sums": (C.c_int, [C.c_int]),
        "sx_observables": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, C.c_int,
                                     C.POINTER(SxObsSettings), C.c_float, C.c_double, C.POINTER(C.c_double), C.c_int]),
        "sx_grav_wave_htt": (C.c_int, [C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_double)]),
        "sx_obs_finalize": (C.c_int, [C.c_int, C.POINTER(SxObsSettings), C.POINTER(C.c_double), C.c_uint64,
                                      C.POINTER(C.c_double)]),
        "sx_sim_set_observable": (C.c_int, [vp, C.c_int, C.POINTER(SxObsSettings)]),
        "sx_sim_observe": (C.c_int, [vp, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
        "sx_sim_set_iteration": (C.c_int, [vp, C.c_uint64]),
        "sx_map_check": (C.c_int, [C.POINTER(SxMap), C.POINTER(SxBox)]),
        "sx_map_kernel": (C.c_int, [vp, sz, vp]),
        "sx_map_chunk_records": (u32, []),
        "sx_pair_bands_internal": (C.c_int, [vp, C.c_int, C.c_uint64, vp, C.POINTER(C.c_int)]),
        "sx_set_map_pair_cap": (C.c_int, [vp, C.c_uint64]),
        "sx_map_render": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, C.c_double, C.POINTER(SxMap),
                                    vp, C.c_int, vp, vp]),
        "sx_map_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_set_map_timing": (C.c_int, [vp, C.c_int]),
        "sx_map_times": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_render": (C.c_int, [vp, C.POINTER(SxMap), C.c_int, vp, vp]),
        "sx_sim_map_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_sim_set_map_pair_cap": (C.c_int, [vp, C.c_uint64]),
        "sx_spectrum_check": (C.c_int, [C.POINTER(SxSpectrum), C.POINTER(SxBox)]),
        "sx_spectrum_num_shells": (u32, [u32]),
        "sx_spectrum_modes": (C.c_int, [u32, vp]),
        "sx_spectrum_chunk_records": (u32, []),
        "sx_set_spectrum_pair_cap": (C.c_int, [vp, C.c_uint64]),
        "sx_mesh_deposit": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, C.c_double, u32,
                                      C.POINTER(vp), C.c_int, C.c_int, vp, vp]),
        "sx_fft3d": (C.c_int, [vp, vp, u32]),
        "sx_shell_sums": (C.c_int, [vp, vp, u32, C.c_double, C.c_int, vp, vp]),
        "sx_spectrum_compute": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, C.c_double,
                                          C.POINTER(SxSpectrum), C.POINTER(vp), C.c_int, vp, vp]),
        "sx_spectrum_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_set_spectrum_timing": (C.c_int, [vp, C.c_int]),
        "sx_spectrum_times": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_spectrum": (C.c_int, [vp, C.POINTER(SxSpectrum), C.c_int, vp, vp]),
        "sx_sim_spectrum_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_sim_set_spectrum_pair_cap": (C.c_int, [vp, C.c_uint64]),
        "sx_profile_check": (C.c_int, [C.POINTER(SxProfile), C.POINTER(SxBox)]),
        "sx_profile_window": (C.c_int, [vp, sz, C.POINTER(i32)]),
        "sx_profile_to_fixed": (C.c_int, [vp, sz, i32, vp]),
        "sx_profile_add_fixed": (C.c_int, [C.POINTER(C.c_uint64), vp, sz]),
        "sx_profile_from_fixed": (C.c_int, [C.POINTER(C.c_uint64), i32, C.POINTER(C.c_double)]),
        "sx_profile_lds_bins": (u32, [C.c_int]),
        "sx_set_profile_lds": (C.c_int, [vp, C.c_int]),
        "sx_profile_compute": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, C.POINTER(SxParams),
                                         C.c_int, C.POINTER(SxProfile), C.POINTER(SxProfileResult)]),
        "sx_profile_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_set_profile_timing": (C.c_int, [vp, C.c_int]),
        "sx_profile_times": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_profile": (C.c_int, [vp, C.POINTER(SxProfile), C.POINTER(SxProfileResult)]),
        "sx_sim_profile_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_fof_check": (C.c_int, [C.POINTER(SxFof), C.POINTER(SxBox)]),
        "sx_fof_grid": (C.c_int, [C.POINTER(SxFof), C.POINTER(SxBox), C.c_uint64, C.POINTER(u32)]),
        "sx_fof_compute": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, vp, C.POINTER(SxFof),
                                     C.POINTER(SxFofResult)]),
        "sx_fof_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_set_fof_timing": (C.c_int, [vp, C.c_int]),
        "sx_fof_times": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_fof": (C.c_int, [vp, C.POINTER(SxFof), C.POINTER(SxFofResult)]),
        "sx_sim_fof_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_halo_check": (C.c_int, [C.POINTER(SxHalo), C.POINTER(SxBox)]),
        "sx_halo_compute": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, vp, C.POINTER(SxHalo),
                                      C.POINTER(SxHaloResult)]),
        "sx_halo_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_set_halo_timing": (C.c_int, [vp, C.c_int]),
        "sx_halo_times": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_halos": (C.c_int, [vp, C.POINTER(SxHalo), C.POINTER(SxHaloResult)]),
        "sx_sim_halos_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_twopoint_check": (C.c_int, [C.POINTER(SxTwoPoint), C.POINTER(SxBox)]),
        "sx_twopoint_grid": (C.c_int, [C.POINTER(SxTwoPoint), C.POINTER(SxBox), C.c_uint64, C.POINTER(u32)]),
        "sx_twopoint_compute": (C.c_int, [vp, C.POINTER(SxFields), C.POINTER(SxBox), u32, u32, vp,
                                          C.POINTER(SxTwoPoint), C.POINTER(SxTwoPointResult)]),
        "sx_twopoint_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_set_twopoint_timing": (C.c_int, [vp, C.c_int]),
        "sx_twopoint_times": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_twopoint_window": (C.c_int, [vp, sz, C.POINTER(i32)]),
        "sx_twopoint_to_fixed": (C.c_int, [vp, sz, i32, vp]),
        "sx_twopoint_add_fixed": (C.c_int, [vp, vp, sz]),
        "sx_twopoint_from_fixed": (C.c_int, [vp, i32, C.POINTER(C.c_double)]),
        "sx_sim_twopoint": (C.c_int, [vp, C.POINTER(SxTwoPoint), C.POINTER(SxTwoPointResult)]),
        "sx_sim_twopoint_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "sx_cooling_create": (C.c_int, [C.POINTER(vp), vp, vp, u32]),
        "sx_cooling_destroy": (None, [vp]),
        "sx_cooling_num_nodes": (u32, [vp]),
        "sx_cooling_get_table": (C.c_int, [vp, vp, vp, vp, vp]),
        "sx_cooling_rate_host": (C.c_double, [vp, C.c_double]),
        "sx_cooling_integrate_host": (C.c_double, [vp, C.c_double, C.c_double]),
        "sx_cooling_time": (C.c_int, [vp, vp, u32, vp, vp, C.c_double, C.POINTER(C.c_double)]),
        "sx_cool": (C.c_int, [vp, vp, u32, vp, vp, vp, C.c_double, C.c_double, C.POINTER(C.c_double)]),
        "sx_set_cooling_timing": (C.c_int, [vp, C.c_int]),
        "sx_cooling_times": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_set_cooling": (C.c_int, [vp, vp, C.c_double]),
        "sx_sim_cooling_stats": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "sx_sim_set_cooling_radiated": (C.c_int, [vp, C.c_double]),
        "sx_sim_cooling_times": (C.c_int, [vp, C.POINTER(C.c_float)]),
    }
    for name, (res, args) in sig.items():
        # a measurement build named by SPHEXA_AMD_LIB (an A/B against an older library) may predate an entry
        if os.environ.get("SPHEXA_AMD_LIB") and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def domain_splitters(hist, hist_bits, nranks):
    """equal-count SFC splitters (nranks+1 keys) from an all-reduced key histogram (sx_domain_splitters)"""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.size != 1 << hist_bits:
        raise ValueError("histogram size must be 2^hist_bits")
    out = np.zeros(nranks + 1, np.uint64)
    rc = lib().sx_domain_splitters(h.ctypes.data, hist_bits, nranks, out.ctypes.data)
    if rc != SX_OK:
        raise SxError(f"sx_domain_splitters failed: {rc}")
    return out


def halo_layout(recv_counts, rank, num_local):
    """halo receive offsets [lower ranks | locals | higher ranks] and (first, last, total) (sx_domain_halo_layout)"""
    rc_ = np.ascontiguousarray(recv_counts, dtype=np.uint64)
    off = np.zeros(rc_.size, np.uint64)
    out = np.zeros(3, np.uint64)
    rc = lib().sx_domain_halo_layout(rc_.ctypes.data, rc_.size, rank, num_local, off.ctypes.data, out.ctypes.data)
    if rc != SX_OK:
        raise SxError(f"sx_domain_halo_layout failed: {rc}")
    return off, tuple(int(v) for v in out)


def default_params(K=None, ngmax=150, ng0=100, av_clean=False, g=0.0, theta=0.5, std=False, bdt=False, nbody=False):
    """ParticlesData defaults (particles_data.hpp:86-138); av_clean selects HydroVeProp<true> (with bdt:
    HydroVeBdtProp<true>), std the std propagator (HydroProp), bdt the block time-step VE propagator
    (HydroVeBdtProp, one substep per step) and nbody the gravity-only propagator (NbodyProp, needs g != 0) in sx_sim."""
    if std + bdt + nbody > 1:
        raise ValueError("std, bdt and nbody are different propagators")
    if K is None:
        K = lib().sx_kernel_constant()
    return SxParams(K=K, ng0=ng0, ngmax=ngmax, Kcour=0.2, Krho=0.06, gamma=5.0 / 3.0, muiConst=10.0, alphamin=0.05,
                    alphamax=1.0, decay_constant=0.2, Atmin=0.1, Atmax=0.2,
                    ramp=float(np.float32(1.0) / (np.float32(0.2) - np.float32(0.1))), maxDtIncrease=1.1,
                    avClean=1 if av_clean else 0, theta=theta, g=g, eps=0.005, etaAcc=0.2,
                    propagator=1 if std else (2 if bdt else (3 if nbody else 0)))


def make_box(lim, bnd):
    b = SxBox()
    for k in range(6):
        b.lim[k] = float(lim[k])
    for k in range(3):
        b.bnd[k] = int(bnd[k])
    return b


# the step attributes of a restart file, in the order ParticlesData::loadOrStoreAttributes writes them
# (particles_data.hpp:170-190) followed by Box::loadOrStore (box.hpp:170-171)
ATTRIBUTE_NAMES = ["iteration", "numParticlesGlobal", "ng0", "ngmax", "time", "minDt", "minDt_m1", "Kcour", "Krho",
                   "gravConstant", "gamma", "eps", "etaAcc", "muiConst", "alphamin", "alphamax", "decay_constant",
                   "sincIndex", "kernelChoice", "box", "boundaryType"]


def reference_attributes(params, box, scalars, iteration, num_particles_global):
    """the reference's restart attributes with the reference's types (size_t/uint64 counters, double scalars, float
    muiConst/alpha parameters, int kernel choice, 6 box limits, 3 boundary-type chars)"""
    p = params
    return {
        "iteration": np.uint64(iteration), "numParticlesGlobal": np.uint64(num_particles_global),
        "ng0": np.uint32(p.ng0), "ngmax": np.uint32(p.ngmax), "time": np.float64(scalars["ttot"]),
        "minDt": np.float64(scalars["minDt"]), "minDt_m1": np.float64(scalars["minDt_m1"]),
        "Kcour": np.float64(p.Kcour), "Krho": np.float64(p.Krho), "gravConstant": np.float64(p.g),
        "gamma": np.float64(p.gamma), "eps": np.float64(p.eps), "etaAcc": np.float64(p.etaAcc),
        "muiConst": np.float32(p.muiConst), "alphamin": np.float32(p.alphamin), "alphamax": np.float32(p.alphamax),
        "decay_constant": np.float32(p.decay_constant), "sincIndex": np.float64(6.0),  # sinc_6, the kernel tabulated
        "kernelChoice": np.int32(0),  # SphKernelType::sinc_n
        "box": np.array([box.lim[k] for k in range(6)], dtype=np.float64),
        "boundaryType": np.array([box.bnd[k] for k in range(3)], dtype=np.int8),
    }


class SxError(RuntimeError):
    pass


# the step attributes TurbulenceData::loadOrStore writes (turbulence_data.hpp:92-115), in its order
TURBULENCE_ATTRIBUTES = ["turbulence::variance", "turbulence::decayTime", "turbulence::solWeight",
                         "turbulence::solWeightNorm", "turbulence::numModes", "turbulence::modes",
                         "turbulence::amplitudes", "turbulence::phases", "rngEngineState"]


#: what a checkpoint of a cooling Sim adds: the table's nodes and values, the limiter, this rank's energy radiated
COOLING_ATTRIBUTES = ["cooling::T", "cooling::lambda", "cooling::ct_crit", "cooling::erad"]


class Turbulence:
    """the host state of the turbulence stirring (sx_turb_*): sph::TurbulenceData (turbulence_data.hpp:46-184) with
    createStirringModes, updateNoise (driver.hpp:80-92) and computePhases (phases.hpp:47-72).  Needs no GPU.
    Turbulence(solWeight=..., rngSeed=..., ...) takes the fields of SxTurbSettings; a Sim hands out a borrowed one."""

    def __init__(self, settings=None, _borrowed=None, **kw):
        self.L = lib()
        self.owned = _borrowed is None
        if _borrowed is not None:
            self.h = C.c_void_p(_borrowed)
            return
        self.settings = settings if settings is not None else SxTurbSettings(**kw)
        self.h = C.c_void_p()
        rc = self.L.sx_turb_create(C.byref(self.h), C.byref(self.settings))
        if rc != SX_OK:
            raise SxError(f"sx_turb_create: code {rc}: invalid settings")

    def close(self):
        if self.h and self.owned:
            self.L.sx_turb_destroy(self.h)
        self.h = None

    @property
    def num_modes(self):
        return int(self.L.sx_turb_num_modes(self.h))

    def scalars(self):
        out = (C.c_double * 4)()
        self.L.sx_turb_get_scalars(self.h, out)
        return dict(zip(["variance", "decayTime", "solWeight", "solWeightNorm"], list(out)))

    def arrays(self):
        m = self.num_modes
        modes, amp, ph = np.empty(3 * m), np.empty(m), np.empty(6 * m)
        self.L.sx_turb_get_arrays(self.h, modes.ctypes.data, amp.ctypes.data, ph.ctypes.data)
        return dict(modes=modes, amplitudes=amp, phases=ph)

    def rng_state(self):
        """the generator as operator<< on std::mt19937 writes it (the reference's rngEngineState)"""
        n = self.L.sx_turb_get_rng(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        self.L.sx_turb_get_rng(self.h, buf, n + 1)
        return buf.value.decode()

    def state(self):
        """everything TurbulenceData::loadOrStore saves, under its attribute names"""
        sc, ar = self.scalars(), self.arrays()
        d = {"turbulence::" + k: np.float64(v) for k, v in sc.items()}
        d["turbulence::numModes"] = np.uint64(self.num_modes)
        d.update({"turbulence::" + k: v for k, v in ar.items()})
        d["rngEngineState"] = np.frombuffer(self.rng_state().encode(), dtype=np.uint8).copy()
        return {k: d[k] for k in TURBULENCE_ATTRIBUTES}

    @staticmethod
    def _state_args(state):
        sc = (C.c_double * 4)(*[float(np.asarray(state["turbulence::" + k]).ravel()[0])
                                for k in ("variance", "decayTime", "solWeight", "solWeightNorm")])
        m = int(np.asarray(state["turbulence::numModes"]).ravel()[0])
        arr = [np.ascontiguousarray(np.atleast_1d(state["turbulence::" + k]), dtype=np.float64)
               for k in ("modes", "amplitudes", "phases")]
        if [a.size for a in arr] != [3 * m, m, 6 * m]:
            raise ValueError("turbulence state: array sizes do not match numModes")
        rng = state.get("rngEngineState")
        if rng is not None and not isinstance(rng, (bytes, str)):
            rng = np.atleast_1d(rng).astype(np.uint8).tobytes()
        if isinstance(rng, str):
            rng = rng.encode()
        if rng is not None:
            rng = rng.split(b"\0")[0]
        return sc, m, arr, rng

    def _own(self, what):
        if not self.owned:
            raise SxError(f"Turbulence.{what}: this is a Sim's state, a host copy of what the device holds; "
                          "change it with Sim.set_turbulence_state")

    def set_state(self, state):
        self._own("set_state")
        sc, m, arr, rng = self._state_args(state)
        rc = self.L.sx_turb_set_state(self.h, sc, m, *[a.ctypes.data for a in arr], rng)
        if rc != SX_OK:
            raise SxError(f"sx_turb_set_state: code {rc}")

    def max_index(self):
        return int(self.L.sx_turb_max_index(self.h))

    def update_noise(self, dt):
        self._own("update_noise")
        self.L.sx_turb_update_noise(self.h, float(dt))

    def compute_phases(self):
        m = self.num_modes
        re, im = np.empty(3 * m), np.empty(3 * m)
        self.L.sx_turb_compute_phases(self.h, re.ctypes.data, im.ctypes.data)
        return re, im


def stir(ctx, groups, fields, turb):
    """sx_stir: the stirring accelerations of turb's current phases onto fields.ax, ay, az over the group view"""
    ctx.check(ctx.L.sx_stir(ctx.h, C.byref(groups), C.byref(fields), turb.h), "sx_stir")


class Context:
    def __init__(self, device=0, exact=False):
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.sx_create(C.byref(self.h), device)
        self.check(rc, "sx_create")
        self.L.sx_set_exact(self.h, 1 if exact else 0)
        self.allocs = []

    def check(self, rc, what=""):
        if rc != SX_OK:
            msg = self.L.sx_last_error(self.h) if self.h else b"?"
            raise SxError(f"{what}: code {rc}: {msg.decode() if msg else ''}")

    def set_exact(self, exact):
        self.L.sx_set_exact(self.h, 1 if exact else 0)

    def set_pack12_max(self, max_union=None):
        """cluster lists of unions up to max_union entries are packed12, larger ones u16 (None: the default, 4095, or
        0 for an exact context; tests set it).  Takes effect with the next search; a Sim reads it when it is created."""
        v = 0xffffffff if max_union is None else int(max_union)
        self.check(self.L.sx_set_pack12_max(self.h, v), "sx_set_pack12_max")

    def set_direct_splits(self, k=0):
        """source splits of gravity_direct (sx_set_direct_splits): 0 is the automatic rule, a k beyond the number of
        256-source tiles is clamped"""
        self.check(self.L.sx_set_direct_splits(self.h, int(k)), "sx_set_direct_splits")

    def gravity_direct(self, fields, groups, box=None, num_shells=0, G=1.0, out4=False):
        """the direct sum over all sources of fields for the targets of groups (sx_gravity_direct: ryoanji::directSum).
        Adds G acc to fields.ax, ay, az when the three are set; out4=True also returns {G m phi, G ax, G ay, G az} per
        particle, (n, 4) doubles, zero outside the view.  Returns (egrav, out4 or None)."""
        n = int(fields.n)
        d = None
        if out4:
            d = self.alloc(4 * n, np.float64)
            self.check(self.L.sx_memset(self.h, d.ptr, 0, 32 * n), "sx_memset")
        e = C.c_double(0.0)
        try:
            self.check(self.L.sx_gravity_direct(self.h, C.byref(groups), C.byref(fields),
                                                C.byref(box) if box is not None else None, int(num_shells), float(G),
                                                d.ptr if d is not None else None, C.byref(e)), "sx_gravity_direct")
            return e.value, (d.get().reshape(n, 4) if d is not None else None)
        finally:
            if d is not None:
                self.free(d)

    # ---- device arrays --------------------------------------------------------------------------------------
    def alloc(self, n, dtype):
        nbytes = int(n) * np.dtype(dtype).itemsize
        p = self.L.sx_device_alloc(self.h, nbytes)
        if not p:
            raise SxError("device alloc failed")
        self.allocs.append(p)
        return DeviceArray(self, p, int(n), dtype)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.alloc(arr.size, arr.dtype)
        self.check(self.L.sx_memcpy(self.h, d.ptr, arr.ctypes.data, arr.nbytes, 1), "upload")
        return d

    def free(self, arr):
        """release one DeviceArray of alloc/upload"""
        if arr.ptr in self.allocs:
            self.allocs.remove(arr.ptr)
            self.L.sx_device_free(self.h, arr.ptr)

    def free_all(self):
        for p in self.allocs:
            self.L.sx_device_free(self.h, p)
        self.allocs = []

    def close(self):
        self.free_all()
        if self.h:
            self.L.sx_destroy(self.h)
            self.h = None

    def sync(self):
        self.check(self.L.sx_synchronize(self.h), "sync")

    def set_map_pair_cap(self, pairs=0):
        """(tile, particle) pairs render_map produces and sorts at a time (sx_set_map_pair_cap); 0: the default"""
        self.check(self.L.sx_set_map_pair_cap(self.h, int(pairs)), "sx_set_map_pair_cap")

    def render_map(self, fields, box, spec, a=None, first=0, last=None, K=None, sum0=None, sum1=None):
        """the map `spec` (an SxMap) of the particles [first, last) of an SxFields (sx_map_render): (sum0, sum1) as
        arrays of shape spec.shape, sum1 None without a.  a: a DeviceArray of float32 or float64, one value per particle
        of fields.  sum0, sum1: DeviceArrays to render into (the caller reads them); by default temporaries."""
        ny, nx = spec.shape
        last = fields.n if last is None else last
        if sum0 is not None and a is not None and sum1 is None:
            raise ValueError("render_map: a column rendered into the caller's sum0 needs the caller's sum1 too")
        d0 = sum0 if sum0 is not None else self.alloc(nx * ny, np.float64)
        d1 = sum1 if (sum1 is not None or a is None) else self.alloc(nx * ny, np.float64)  # None: no a, sum1 untouched
        try:
            if a is not None and a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise TypeError("render_map: a must be float32 or float64")
            self.check(self.L.sx_map_render(self.h, C.byref(fields), C.byref(box), int(first), int(last),
                                            float(self.L.sx_kernel_constant() if K is None else K), C.byref(spec),
                                            a.ptr if a is not None else None,
                                            int(a is not None and a.dtype == np.dtype(np.float64)), d0.ptr,
                                            d1.ptr if d1 is not None else None),
                       "sx_map_render")
            if sum0 is not None:
                return None, None
            return d0.get().reshape(ny, nx), (d1.get().reshape(ny, nx) if a is not None else None)
        finally:
            if sum0 is None:
                self.free(d0)
            if sum1 is None and d1 is not None:
                self.free(d1)

    def map_stats(self):
        """the last render_map: {pairs, bands, longest (tile list), footprints (particles with one in the window)}"""
        out = (C.c_uint64 * 4)()
        self.check(self.L.sx_map_stats(self.h, out), "sx_map_stats")
        return dict(zip(["pairs", "bands", "longest", "footprints"], [int(v) for v in out]))

    def set_map_timing(self, on=True):
        self.check(self.L.sx_set_map_timing(self.h, 1 if on else 0), "sx_set_map_timing")

    def map_times(self):
        """{binning, sort, render} in ms and the scratch bytes of the last render_map (after set_map_timing)"""
        out = (C.c_double * 4)()
        self.check(self.L.sx_map_times(self.h, out), "sx_map_times")
        return {"binning_ms": out[0], "sort_ms": out[1], "render_ms": out[2], "scratch_bytes": int(out[3])}

    # ---- power spectra ----------------------------------------------------------------------------------------
    def set_spectrum_pair_cap(self, pairs=0):
        """(block, particle) pairs mesh_deposit produces and sorts at a time (sx_set_spectrum_pair_cap); 0: the default"""
        self.check(self.L.sx_set_spectrum_pair_cap(self.h, int(pairs)), "sx_set_spectrum_pair_cap")

    @staticmethod
    def _columns(a):
        """(pointer array, count, is double) of up to three DeviceArrays of one dtype"""
        a = [] if a is None else list(a)
        if len(a) > 3:
            raise ValueError("at most three columns")
        kinds = {c.dtype for c in a}
        if len(kinds) > 1 or (kinds and kinds.pop() not in (np.dtype(np.float32), np.dtype(np.float64))):
            raise TypeError("columns must be all float32 or all float64")
        ptrs = (C.c_void_p * 3)(*([c.ptr for c in a] + [None] * (3 - len(a))))
        return ptrs, len(a), int(bool(a) and a[0].dtype == np.dtype(np.float64))

    def mesh_deposit(self, fields, box, n, a=None, first=0, last=None, K=None):
        """the particles [first, last) of an SxFields deposited onto the n^3 mesh (sx_mesh_deposit): (S0, S1), arrays of
        shape (n, n, n) [iz][iy][ix] and (len(a), n, n, n); a: up to three DeviceArrays of one dtype"""
        ptrs, num, dbl = self._columns(a)
        n3 = int(n) ** 3
        last = fields.n if last is None else last
        d0 = self.alloc(n3, np.float64)
        d1 = self.alloc(max(1, num) * n3, np.float64)
        try:
            self.check(self.L.sx_mesh_deposit(self.h, C.byref(fields), C.byref(box), int(first), int(last),
                                              float(self.L.sx_kernel_constant() if K is None else K), int(n), ptrs, num,
                                              dbl, d0.ptr, d1.ptr), "sx_mesh_deposit")
            return d0.get().reshape(n, n, n), d1.get()[: num * n3].reshape(num, n, n, n)
        finally:
            self.free(d0)
            self.free(d1)

    def fft3d(self, mesh):
        """the forward transform of a complex (n, n, n) array scaled by n^-3 (sx_fft3d), or of a DeviceArray of 2 n^3
        doubles in place (then n is taken from its size and nothing is returned)"""
        if isinstance(mesh, DeviceArray):
            n = round((mesh.n // 2) ** (1.0 / 3.0))
            self.check(self.L.sx_fft3d(self.h, mesh.ptr, n), "sx_fft3d")
            return None
        mesh = np.ascontiguousarray(mesh, dtype=np.complex128)
        n = mesh.shape[0]
        d = self.upload(mesh.view(np.float64).ravel())
        try:
            self.check(self.L.sx_fft3d(self.h, d.ptr, n), "sx_fft3d")
            return d.get().view(np.complex128).reshape(mesh.shape)
        finally:
            self.free(d)

    def shell_sums(self, mesh, prefactor=1.0, power=None):
        """(power, modes) of a transformed complex (n, n, n) array or DeviceArray of 2 n^3 doubles (sx_shell_sums);
        power: an array of earlier sums to add to (accumulate = 1)"""
        if isinstance(mesh, DeviceArray):
            d, n, own = mesh, round((mesh.n // 2) ** (1.0 / 3.0)), False
        else:
            mesh = np.ascontiguousarray(mesh, dtype=np.complex128)
            d, n, own = self.upload(mesh.view(np.float64).ravel()), mesh.shape[0], True
        ns = spectrum_num_shells(n)
        dp = self.upload(np.asarray(power, np.float64)) if power is not None else self.alloc(max(1, ns), np.float64)
        dm = self.alloc(max(1, ns), np.uint64)
        try:
            self.check(self.L.sx_shell_sums(self.h, d.ptr, n, float(prefactor), int(power is not None), dp.ptr, dm.ptr),
                       "sx_shell_sums")
            return dp.get()[:ns], dm.get()[:ns]
        finally:
            self.free(dp)
            self.free(dm)
            if own:
                self.free(d)

    def spectrum(self, fields, box, spec, a=None, first=0, last=None, K=None):
        """(power, modes) of the particles [first, last) of an SxFields (sx_spectrum_compute); a: the three velocity
        columns (None: fields.vx, vy, vz) or [the scalar column] (None: the mesh density), DeviceArrays of one dtype"""
        ptrs, num, dbl = self._columns(a)
        ns = max(1, spectrum_num_shells(spec.n))
        last = fields.n if last is None else last
        dp, dm = self.alloc(ns, np.float64), self.alloc(ns, np.uint64)
        try:
            self.check(self.L.sx_spectrum_compute(self.h, C.byref(fields), C.byref(box), int(first), int(last),
                                                  float(self.L.sx_kernel_constant() if K is None else K), C.byref(spec),
                                                  ptrs if num else None, dbl, dp.ptr, dm.ptr), "sx_spectrum_compute")
            return dp.get(), dm.get()
        finally:
            self.free(dp)
            self.free(dm)

    def spectrum_stats(self):
        """the last deposit: {pairs, bands, longest (block list), clamped (particles with h below half a cell)}"""
        out = (C.c_uint64 * 4)()
        self.check(self.L.sx_spectrum_stats(self.h, out), "sx_spectrum_stats")
        return dict(zip(["pairs", "bands", "longest", "clamped"], [int(v) for v in out]))

    def set_spectrum_timing(self, on=True):
        self.check(self.L.sx_set_spectrum_timing(self.h, 1 if on else 0), "sx_set_spectrum_timing")

    def spectrum_times(self):
        """{binning, sort, gather, fft, shells} in ms since the last deposit began (after set_spectrum_timing)"""
        out = (C.c_double * 5)()
        self.check(self.L.sx_spectrum_times(self.h, out), "sx_spectrum_times")
        return dict(zip(["binning_ms", "sort_ms", "gather_ms", "fft_ms", "shells_ms"], list(out)))

    # ---- binned profiles with exact sums ---------------------------------------------------------------------
    def profile(self, fields, box, spec, first=0, last=None, params=None, std=False):
        """the profile `spec` (an SxProfile) of the particles [first, last) of an SxFields (sx_profile_compute): a dict
        of arrays with nbins + 2 entries per row (the last two: underflow, overflow): count (uint64), nonfinite, W, and
        S1, S2, D, min, max of shape (nq, nbins + 2).  params: gamma and muiConst (default_params())."""
        # a spec beyond the limits is refused by the call before it writes: the arrays need not hold it
        nb2, nq = min(int(spec.nbins), 4096) + 2, min(int(spec.nq), PROF_MAX_Q)
        last = fields.n if last is None else last
        params = params if params is not None else default_params()
        shapes = {"count": (nb2,), "nonfinite": (1,), "W": (nb2,)}
        shapes.update({k: (nq, nb2) for k in ("S1", "S2", "D", "min", "max")})
        dev = {k: self.alloc(max(1, int(np.prod(s))), np.uint64 if k in ("count", "nonfinite") else np.float64)
               for k, s in shapes.items()}
        res = SxProfileResult(**{k: d.ptr for k, d in dev.items()})
        try:
            self.check(self.L.sx_profile_compute(self.h, C.byref(fields), C.byref(box), int(first), int(last),
                                                 C.byref(params), int(bool(std)), C.byref(spec), C.byref(res)),
                       "sx_profile_compute")
            return {k: dev[k].get()[: int(np.prod(s))].reshape(s) for k, s in shapes.items()}
        finally:
            for d in dev.values():
                self.free(d)

    def set_profile_lds(self, on=True):
        """False: the following profiles accumulate in the global array whatever nbins (sx_set_profile_lds)"""
        self.check(self.L.sx_set_profile_lds(self.h, 1 if on else 0), "sx_set_profile_lds")

    def profile_stats(self):
        """the last profile: {particles, lds (1: the bins were in LDS), passes, nonfinite}"""
        out = (C.c_uint64 * 4)()
        self.check(self.L.sx_profile_stats(self.h, out), "sx_profile_stats")
        return dict(zip(["particles", "lds", "passes", "nonfinite"], [int(v) for v in out]))

    def set_profile_timing(self, on=True):
        self.check(self.L.sx_set_profile_timing(self.h, 1 if on else 0), "sx_set_profile_timing")

    def profile_times(self):
        """{pass 1, pass 2, conversion} in ms of the last profile (after set_profile_timing) and the bytes a pass reads"""
        out = (C.c_double * 4)()
        self.check(self.L.sx_profile_times(self.h, out), "sx_profile_times")
        return {"pass1_ms": out[0], "pass2_ms": out[1], "final_ms": out[2], "pass_bytes": out[3]}

    # ---- friends-of-friends groups ----------------------------------------------------------------------------
    def fof(self, fields, box, spec, id=None, first=0, last=None, labels=True):
        """the friends-of-friends groups `spec` (an SxFof) of the particles [first, last) of an SxFields
        (sx_fof_compute).  id: a DeviceArray of uint64, one per particle of fields, or None (labels are indices then).
        A dict: label (uint64 per particle of the range, None without labels), num_groups (groups of min_members or
        more), num_all (all groups, singles included), and the catalogue cut to min(num_groups, maxGroups) entries,
        ordered by count descending then label ascending: group_label, count, mass, com (k, 3), vel (k, 3)."""
        last = fields.n if last is None else last
        n, cap = max(0, int(last) - int(first)), int(spec.maxGroups)
        if id is not None and id.dtype != np.dtype(np.uint64):
            raise TypeError("fof: id must be uint64")
        host = _fof_arrays(n, cap, labels)
        dev = {k: self.alloc(a.size, a.dtype) for k, (a, _) in host.items()}
        res = SxFofResult(**{host[k][1]: d.ptr for k, d in dev.items()})
        try:
            self.check(self.L.sx_fof_compute(self.h, C.byref(fields), C.byref(box), int(first), int(last),
                                             id.ptr if id is not None else None, C.byref(spec), C.byref(res)),
                       "sx_fof_compute")
            got = {k: (dev[k].get().reshape(a.shape), m) for k, (a, m) in host.items()}
            return _fof_dict(got, n, cap)
        finally:
            for d in dev.values():
                self.free(d)

    def fof_stats(self):
        """the last fof(): {pair tests, union retries, all groups, groups of min_members or more}"""
        out = (C.c_uint64 * 4)()
        self.check(self.L.sx_fof_stats(self.h, out), "sx_fof_stats")
        return dict(zip(["pair_tests", "union_retries", "num_all", "num_groups"], [int(v) for v in out]))

    def set_fof_timing(self, on=True):
        self.check(self.L.sx_set_fof_timing(self.h, 1 if on else 0), "sx_set_fof_timing")

    def fof_times(self):
        """{grid, link, compress, catalogue} in ms of the last fof() of the context or of a Sim on it (after
        set_fof_timing); the catalogue's interval includes the host's read of the group count"""
        out = (C.c_double * 4)()
        self.check(self.L.sx_fof_times(self.h, out), "sx_fof_times")
        return {"grid_ms": out[0], "link_ms": out[1], "compress_ms": out[2], "catalogue_ms": out[3]}

    # ---- group properties ----------------------------------------------------------------------------------------
    def halos(self, fields, box, spec, id=None, first=0, last=None, labels=True):
        """the friends-of-friends groups `spec` (an SxHalo) of the particles [first, last) of an SxFields behind the
        density cut, and their properties (sx_halo_compute).  The dict of fof() -- an unselected particle's label is
        2^64 - 1 -- and per catalogue entry sigma (k, 6), shape (k, 6) (xx xy xz yy yz zz), angmom (k, 3), rmax, eint,
        epot (None where the flag is clear; epot NaN for a group over max_pair_members), and derived from them ekin,
        alpha_vir, bound and axes (see _halo_dict)."""
        last = fields.n if last is None else last
        n, cap, flags = max(0, int(last) - int(first)), int(spec.maxGroups), int(spec.flags)
        if id is not None and id.dtype != np.dtype(np.uint64):
            raise TypeError("halos: id must be uint64")
        host = _halo_arrays(n, cap, labels, flags)
        dev = {k: self.upload(a.reshape(-1)) for k, (a, _) in host.items()}
        res = SxHaloResult(**{host[k][1]: d.ptr for k, d in dev.items()})
        try:
            self.check(self.L.sx_halo_compute(self.h, C.byref(fields), C.byref(box), int(first), int(last),
                                              id.ptr if id is not None else None, C.byref(spec), C.byref(res)),
                       "sx_halo_compute")
            got = {k: (dev[k].get().reshape(a.shape), m) for k, (a, m) in host.items()}
            return _halo_dict(got, n, cap, flags)
        finally:
            for d in dev.values():
                self.free(d)

    def halo_stats(self):
        """the last halos(): {pair terms evaluated, pair work items, groups with an epot, groups over the cap}"""
        out = (C.c_uint64 * 4)()
        self.check(self.L.sx_halo_stats(self.h, out), "sx_halo_stats")
        return dict(zip(["pair_terms", "pair_items", "with_epot", "over_cap"], [int(v) for v in out]))

    def set_halo_timing(self, on=True):
        self.check(self.L.sx_set_halo_timing(self.h, 1 if on else 0), "sx_set_halo_timing")

    def halo_times(self):
        """{group search, moments, pair kernel, combination and copies} in ms of the last halos() of the context or of
        a Sim on it (after set_halo_timing)"""
        out = (C.c_double * 4)()
        self.check(self.L.sx_halo_times(self.h, out), "sx_halo_times")
        return {"search_ms": out[0], "moments_ms": out[1], "pairs_ms": out[2], "combine_ms": out[3]}

    # ---- two-point statistics -----------------------------------------------------------------------------------
    def twopoint(self, fields, box, spec, id=None, first=0, last=None):
        """the pair counts and velocity structure functions `spec` (an SxTwoPoint) of the particles [first, last) of an
        SxFields (sx_twopoint_compute).  id: a DeviceArray of uint64, one per particle of fields, or None (targets go
        by index then).  A dict: edges, count (uint64 per bin), the exact sums U1 U2 U3 A3 T2 WW (None where the series
        is off), the means s1 s2 s3 s3abs dv2 = sum / count (NaN in an empty bin), ww, targets, nonfinite, coincident,
        pairs_expected = targets (n_f - 1) - targets (targets - 1) / 2, and in a box periodic on all three axes
        xi = count / (pairs_expected (4 pi / 3)(e_{b+1}^3 - e_b^3) / V) - 1."""
        last = fields.n if last is None else last
        if id is not None and id.dtype != np.dtype(np.uint64):
            raise TypeError("twopoint: id must be uint64")
        host = _twopoint_arrays(spec)
        dev = {k: self.upload(a) for k, a in host.items()}
        res = SxTwoPointResult(**{k: d.ptr for k, d in dev.items()})
        try:
            self.check(self.L.sx_twopoint_compute(self.h, C.byref(fields), C.byref(box), int(first), int(last),
                                                  id.ptr if id is not None else None, C.byref(spec), C.byref(res)),
                       "sx_twopoint_compute")
            got = {k: dev[k].get() for k in host}
            return twopoint_dict(spec, got, box, max(0, int(last) - int(first)))
        finally:
            for d in dev.values():
                self.free(d)

    def twopoint_stats(self):
        """the last twopoint(): {pairs tested, pairs binned, targets, nonfinite, coincident}"""
        out = (C.c_uint64 * 5)()
        self.check(self.L.sx_twopoint_stats(self.h, out), "sx_twopoint_stats")
        return dict(zip(["pairs_tested", "pairs_binned", "targets", "nonfinite", "coincident"], [int(v) for v in out]))

    def set_twopoint_timing(self, on=True):
        self.check(self.L.sx_set_twopoint_timing(self.h, 1 if on else 0), "sx_set_twopoint_timing")

    def twopoint_times(self):
        """{grid, windows + gather, pairs, conversion} in ms of the last twopoint() of the context or of a Sim on it
        (after set_twopoint_timing)"""
        out = (C.c_double * 4)()
        self.check(self.L.sx_twopoint_times(self.h, out), "sx_twopoint_times")
        return {"grid_ms": out[0], "window_ms": out[1], "pairs_ms": out[2], "final_ms": out[3]}

    def observables(self, fields, kind, first=0, last=None, box=None, settings=None, mui=10.0, gamma=5.0 / 3.0,
                    cap=None):
        """this rank's sums of one fused pass over [first, last) of an SxFields (sx_observables): a dict with the
        nine conserved sums (CONSERVED_SUMS) followed by the kind's (OBS_SUMS); kind by name or SX_OBS_* value"""
        k, name = obs_kind(kind)
        names = CONSERVED_SUMS + OBS_SUMS[name]
        cap = len(names) if cap is None else int(cap)
        out = (C.c_double * max(1, cap))()
        last = fields.n if last is None else last
        self.check(self.L.sx_observables(self.h, C.byref(fields), C.byref(box) if box is not None else None,
                                         int(first), int(last), k, C.byref(settings) if settings is not None else None,
                                         float(mui), float(gamma), out, cap), "sx_observables")
        return dict(zip(names, list(out)))


class DeviceArray:
    def __init__(self, ctx, ptr, n, dtype):
        self.ctx, self.ptr, self.n, self.dtype = ctx, ptr, n, np.dtype(dtype)

    def get(self):
        out = np.empty(self.n, self.dtype)
        self.ctx.check(self.ctx.L.sx_memcpy(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes, 2), "download")
        return out

    def set(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.size == self.n
        self.ctx.check(self.ctx.L.sx_memcpy(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes, 1), "upload")


class DeviceState:
    """A full ParticlesData-like device field set built from a host dict of numpy arrays."""

    def __init__(self, ctx, host, grad_v=False, std=False):
        """grad_v: also allocate the velocity gradient dV11..dV33 (GradVFields of the avClean propagator);
        std: also allocate rho and p (DependentFields of the std propagator, std_hydro.hpp:78-79)"""
        self.ctx = ctx
        n = len(host["x"])
        self.n = n
        self.dev = {}
        self.fields = SxFields()
        self.fields.n = n
        grad = ("dV11", "dV12", "dV13", "dV22", "dV23", "dV33")
        for name, _ in FIELD_ORDER:
            if name in ("tdpdTrho", "u", "mue", "mui", "cv", "markRamp", "rung") or \
                    (name in grad and not grad_v) or (name in ("rho", "p") and not std):
                continue
            dt = DTYPES[name]
            if name in host:
                d = ctx.upload(np.asarray(host[name], dtype=dt))
            else:
                d = ctx.alloc(n, dt)
                ctx.L.sx_memset(ctx.h, d.ptr, 0, n * np.dtype(dt).itemsize)
            self.dev[name] = d
            setattr(self.fields, name, d.ptr)

    def get(self, name):
        return self.dev[name].get()

    def set(self, name, arr):
        self.dev[name].set(arr)


class Comm:
    """Inter-GPU transport. backend 'rccl' (RCCL over xGMI, production) or 'host' (staged through host memory and
    torch.distributed -- used to run several ranks on one GPU in tests). torch.distributed must be initialised
    (gloo) by the caller; it is only the control plane (unique-id broadcast) for 'rccl'."""

    def __init__(self, backend="rccl"):
        import torch
        import torch.distributed as dist

        self.L = lib()
        self.rank, self.size = dist.get_rank(), dist.get_world_size()
        self.h = C.c_void_p()
        if backend == "rccl":
            uid = (C.c_uint8 * 128)()
            if self.rank == 0:
                rc = self.L.sx_comm_unique_id(uid)
                if rc != SX_OK:
                    raise SxError("ncclGetUniqueId failed")
            t = torch.tensor(list(uid), dtype=torch.uint8)
            dist.broadcast(t, 0)
            for k in range(128):
                uid[k] = int(t[k])
            rc = self.L.sx_comm_create_rccl(C.byref(self.h), self.rank, self.size, uid)
        else:
            def a2a(user, send, sendBytes, recv, recvBytes):
                try:
                    sb = [int(sendBytes[q]) for q in range(self.size)]
                    rb = [int(recvBytes[q]) for q in range(self.size)]
                    src = np.ctypeslib.as_array((C.c_uint8 * max(1, sum(sb))).from_address(send)) if sum(sb) else \
                        np.zeros(1, np.uint8)
                    out = torch.empty(sum(rb), dtype=torch.uint8)
                    dist.all_to_all_single(out, torch.from_numpy(src[:sum(sb)].copy()), rb, sb)
                    if sum(rb):
                        C.memmove(recv, out.numpy().ctypes.data, sum(rb))
                    return 0
                except Exception as e:  # noqa: BLE001 -- report through the return code
                    print("alltoallv callback failed:", e)
                    return 1

            def allreduce(user, buf, count, op):
                try:
                    if op in (0, 3, 4):  # u32 sum, min, max
                        a = np.ctypeslib.as_array((C.c_uint32 * count).from_address(buf))
                        t = torch.from_numpy(a.astype(np.int64))
                        dist.all_reduce(t, op={0: dist.ReduceOp.SUM, 3: dist.ReduceOp.MIN, 4: dist.ReduceOp.MAX}[op])
                        a[:] = t.numpy().astype(np.uint32)
                    else:
                        a = np.ctypeslib.as_array((C.c_double * count).from_address(buf))
                        t = torch.from_numpy(a.copy())
                        dist.all_reduce(t, op=dist.ReduceOp.MIN if op == 1 else dist.ReduceOp.SUM)
                        a[:] = t.numpy()
                    return 0
                except Exception as e:  # noqa: BLE001
                    print("allreduce callback failed:", e)
                    return 1

            self._cbs = (ALLTOALLV_CB(a2a), ALLREDUCE_CB(allreduce))
            rc = self.L.sx_comm_create_host(C.byref(self.h), self.rank, self.size, self._cbs[0], self._cbs[1], None)
        if rc != SX_OK:
            raise SxError(f"communicator creation failed ({backend}): {rc}")

    def alltoallv(self, send, send_bytes, send_off, recv, recv_bytes, recv_off, stream=None):
        """sx_comm_alltoallv on device pointers (byte counts / offsets per rank); enqueued on `stream`"""
        arr = [np.ascontiguousarray(a, dtype=np.uint64) for a in (send_bytes, send_off, recv_bytes, recv_off)]
        if any(a.size != self.size for a in arr):
            raise ValueError("alltoallv: one count and one offset per rank")
        rc = self.L.sx_comm_alltoallv(self.h, send, arr[0].ctypes.data, arr[1].ctypes.data, recv, arr[2].ctypes.data,
                                      arr[3].ctypes.data, stream)
        if rc != SX_OK:
            raise SxError(f"sx_comm_alltoallv failed: {rc}")

    ALLREDUCE_OPS = {"sum_u32": 0, "min_f64": 1, "sum_f64": 2, "min_u32": 3, "max_u32": 4}

    def allreduce(self, dev, count, op, stream=None):
        """sx_comm_allreduce in place on a device buffer: op 'sum_u32', 'min_f64' or 'sum_f64'"""
        rc = self.L.sx_comm_allreduce(self.h, dev, int(count), self.ALLREDUCE_OPS[op], stream)
        if rc != SX_OK:
            raise SxError(f"sx_comm_allreduce failed: {rc}")

    def close(self):
        if self.h:
            self.L.sx_comm_destroy(self.h)
            self.h = None


class Sim:
    """device-resident propagator on one GPU (sx_sim_*): VE by default; params.propagator (or the propagator keyword,
    which overrides it) selects 0 = ve, 1 = std, 2 = ve-bdt, 3 = nbody (gravity only: params.g must not be 0)"""

    def __init__(self, ctx, capacity, box, params=None, bucket=64, propagator=None):
        self.ctx = ctx
        self.L = ctx.L
        self.params = params or default_params()
        if propagator is not None:
            self.params = SxParams.from_buffer_copy(self.params)  # the caller's params stay as they are
            self.params.propagator = int(propagator)
        self.box = box
        self.iteration = 0  # completed steps (the reference's "iteration" attribute)
        self.stirred = False  # set_turbulence was called: checkpoints carry the turbulence state
        self.last_sum1 = None  # sum1 of the last render() with a field (the numerator of its mean); None without one
        self.cooling = None  # the table of set_cooling (checkpoints carry it, ct_crit and the energy radiated)
        self.ct_crit = 0.0
        self.h = C.c_void_p()
        ctx.check(self.L.sx_sim_create(C.byref(self.h), ctx.h, int(capacity), C.byref(self.params), C.byref(box),
                                       bucket), "sx_sim_create")

    def init_sedov(self, side, rank=0, size=1):
        self.ctx.check(self.L.sx_sim_init_sedov_rank(self.h, side, rank, size), "init_sedov")

    def set_comm(self, comm):
        self.comm = comm
        self.ctx.check(self.L.sx_sim_set_comm(self.h, comm.h), "set_comm")

    def set_turbulence(self, settings=None, **kw):
        """stir every following step (sx_sim_set_turbulence: TurbVeProp, VE propagator on one rank); settings: an
        SxTurbSettings, or its fields as keywords"""
        self.turb_settings = settings if settings is not None else SxTurbSettings(**kw)
        self.ctx.check(self.L.sx_sim_set_turbulence(self.h, C.byref(self.turb_settings)), "set_turbulence")
        self.stirred = True

    def turbulence(self):
        """the sim's turbulence state as a borrowed Turbulence (sx_sim_turbulence: synchronises, brings the device
        phases back); valid until the sim is closed"""
        p = C.c_void_p()
        self.ctx.check(self.L.sx_sim_turbulence(self.h, C.byref(p)), "turbulence")
        return Turbulence(_borrowed=p.value)

    def turbulence_state(self):
        """what TurbulenceData::loadOrStore saves (Turbulence.state) of the running sim"""
        return self.turbulence().state()

    def set_turbulence_state(self, state):
        """restart: restore Turbulence.state and upload it (sx_sim_set_turbulence_state)"""
        sc, m, arr, rng = Turbulence._state_args(state)
        self.ctx.check(self.L.sx_sim_set_turbulence_state(self.h, sc, m, *[a.ctypes.data for a in arr], rng),
                       "set_turbulence_state")

    def turbulence_times(self):
        """device ms of the last step's noise advance and stirring kernel (sx_sim_turbulence_times)"""
        out = (C.c_float * 2)()
        self.ctx.check(self.L.sx_sim_turbulence_times(self.h, out), "turbulence_times")
        return dict(noise=out[0], stirring=out[1])

    def set_cooling(self, cooling, ct_crit=0.1):
        """every following step cools (sx_sim_set_cooling; VE and std propagators, any number of ranks): an exact,
        operator-split update of temp after the position update, and ct_crit times the shortest cooling time among the
        time-step candidates (ct_crit <= 0: no limiter).  cooling: a cooling.Cooling, whose table is copied; None: off
        again"""
        self.ctx.check(self.L.sx_sim_set_cooling(self.h, cooling.h if cooling is not None else None, float(ct_crit)),
                       "set_cooling")
        self.cooling = cooling.table() if cooling is not None else None
        self.ct_crit = float(ct_crit)

    def cooling_stats(self):
        """this rank's figures of the cooling (sx_sim_cooling_stats): minDtCool (ct_crit min t_cool of the last step,
        inf without the limiter), radiated (energy, last step), radiated_total (since set_state or load_checkpoint),
        on_floor (particles at the floor temperature after the last step); sum over the ranks yourself"""
        out = (C.c_double * 4)()
        self.ctx.check(self.L.sx_sim_cooling_stats(self.h, out), "cooling_stats")
        return dict(minDtCool=out[0], radiated=out[1], radiated_total=out[2], on_floor=int(out[3]))

    def cooling_times(self):
        """device ms of the last step's cooling-time kernel and cooling kernel (sx_sim_cooling_times)"""
        out = (C.c_float * 2)()
        self.ctx.check(self.L.sx_sim_cooling_times(self.h, out), "cooling_times")
        return dict(coolingTime=out[0], cool=out[1])

    def set_overlap(self, on):
        self.ctx.check(self.L.sx_sim_set_overlap(self.h, int(bool(on))), "set_overlap")

    def overlap_stats(self):
        out = (C.c_uint32 * 2)()
        self.L.sx_sim_overlap_stats(self.h, out)
        return dict(interior=out[0], boundary=out[1])

    def layout(self):
        out = (C.c_uint64 * 4)()
        self.L.sx_sim_layout(self.h, out)
        return dict(first=out[0], last=out[1], n=out[2], haloRetries=out[3])

    def set_state(self, st, minDt=1e-6, minDt_m1=1e-6):
        """upload the conserved fields (sx_sim_set_state); the gravity-only propagator keeps no temp, du_m1 and alpha:
        they may be missing from st and are ignored if given"""
        skip = self.NBODY_ABSENT if self.params.propagator == 3 else ()
        arrs = [None if k in skip else np.ascontiguousarray(st[k], dtype=t) for k, t in [
            ("x", np.float64), ("y", np.float64), ("z", np.float64), ("h", np.float32), ("m", np.float32),
            ("temp", np.float64), ("vx", np.float32), ("vy", np.float32), ("vz", np.float32), ("x_m1", np.float32),
            ("y_m1", np.float32), ("z_m1", np.float32), ("du_m1", np.float32), ("alpha", np.float32),
            ("id", np.uint64)]]
        self._keep = arrs
        self.ctx.check(self.L.sx_sim_set_state(self.h, arrs[0].size,
                                               *[None if a is None else a.ctypes.data for a in arrs],
                                               float(minDt), float(minDt_m1)), "set_state")

    CONSERVED = ["x", "y", "z", "h", "m", "temp", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "du_m1", "alpha", "id"]
    NBODY_ABSENT = ("temp", "du_m1", "alpha")  # conserved fields of VE that NbodyProp does not keep (nbody.hpp:74)

    def conserved_fields(self):
        """the fields a restart file of this propagator holds (Propagator::conservedFields)"""
        if self.params.propagator == 3:
            return [k for k in self.CONSERVED if k not in self.NBODY_ABSENT]
        return list(self.CONSERVED)

    def memory(self):
        """bytes the sim holds (sx_sim_memory): device and pinned host memory"""
        out = (C.c_uint64 * 2)()
        self.ctx.check(self.L.sx_sim_memory(self.h, out), "memory")
        return dict(device=int(out[0]), pinned=int(out[1]))

    def save_checkpoint(self, path, num_particles_global=None):
        """restart file of this rank: the conserved fields under the reference's field names
        (ParticlesData::fieldNames, particles_data.hpp:247-251; the set HydroVeProp restarts from,
        ve_hydro.hpp:74 + x,y,z,h,m) and the step attributes under the reference's names
        (reference_attributes: ParticlesData::loadOrStoreAttributes, particles_data.hpp:142-193, and
        Box::loadOrStore, box.hpp:168-175).  A path ending in ".h5" appends a step to an H5Part-layout file (the
        reference's format, sphexa_amd.h5part over the image's serial HDF5); any other path writes an .npz."""
        bdt = self.params.propagator == 2
        if bdt:
            ts = self.timestep()
            if not self._hierarchy_boundary(ts):
                # the reference writes files only when isSynced() (sphexa.cpp:165): inside a block time-step hierarchy
                # the state is not restartable (drifted inactive rungs, halo lists of the hierarchy's sync)
                raise ValueError(f"ve-bdt checkpoint inside a time-step hierarchy (substep {ts['substep']} of "
                                 f"{1 << (ts['numRungs'] - 1)}): save after the hierarchy's last substep")
        st = self.get(self.conserved_fields() + (["rung"] if bdt else []))
        # a run restarted from this file begins with a full sync + neighbor build; so does this one's next step, so
        # the two take identical steps (skin lists, sx_sim_rebuild_lists); the gravity-only propagator syncs every step
        if self.params.propagator != 3:
            self.rebuild_lists()
        if num_particles_global is None:
            num_particles_global = self.size()
            comm = getattr(self, "comm", None)
            if comm is not None and comm.size > 1:  # numParticlesGlobal is the sum over the ranks
                import torch
                import torch.distributed as dist

                t = torch.tensor([num_particles_global], dtype=torch.int64)
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                num_particles_global = int(t.item())
        attrs = reference_attributes(self.params, self.box, self.scalars(), self.iteration, num_particles_global)
        if bdt:  # Timestep::loadOrStore(writer, "ts::") (sph/timestep.h:29-33, HydroVeBdtProp::save)
            attrs["ts::numRungs"] = np.int32(ts["numRungs"])
            attrs["ts::dt_m1"] = np.array(ts["dt_m1"], dtype=np.float32)
        if self.stirred:  # TurbVeProp::save (turb_ve.hpp:121): TurbulenceData::loadOrStore
            attrs.update(self.turbulence_state())
        if self.cooling is not None:  # the table, the limiter and this rank's account of the energy radiated
            attrs["cooling::T"] = self.cooling["T"]
            attrs["cooling::lambda"] = self.cooling["lam"]
            attrs["cooling::ct_crit"] = np.float64(self.ct_crit)
            attrs["cooling::erad"] = np.float64(self.cooling_stats()["radiated_total"])
        if str(path).endswith(".h5"):
            from . import h5part

            h5part.write_step(path, st, attrs, mode="a")
        else:
            np.savez(path, **st, **attrs)

    @staticmethod
    def _hierarchy_boundary(ts):
        """HydroVeBdtProp::isSynced (ve_hydro_bdt.hpp:108-112, :220) for the NEXT substep"""
        return ts["substep"] == 0 or ts["substep"] >= (1 << (ts["numRungs"] - 1))

    # attributes ParticlesData::loadOrStoreAttributes restores (particles_data.hpp:170-190) that are parameters of
    # this Sim (fixed at sx_sim_create): a restart must run with the stored values
    PARAM_ATTRIBUTES = ["ng0", "ngmax", "Kcour", "Krho", "gravConstant", "gamma", "eps", "etaAcc", "muiConst",
                        "alphamin", "alphamax", "decay_constant"]

    def _read_checkpoint(self, path, step):
        """{name: array or scalar} of a restart file: the conserved fields (+ rung), and the attributes present"""
        mine = reference_attributes(self.params, self.box, {"ttot": 0.0, "minDt": 0.0, "minDt_m1": 0.0}, 0, 0)
        if str(path).endswith(".h5"):
            from . import h5part

            names = self.conserved_fields() + (["rung"] if self.params.propagator == 2 else [])
            with h5part.H5PartFile(path, "r") as f:
                f.set_step(step)
                present = set(f.attrib_names())
                fields = {k: f.read_field(k, DTYPES.get(k, np.uint64)) for k in names if f.field_info(k) is not None}
            types = {k: np.asarray(v).dtype for k, v in mine.items()}
            types.update({"ts::numRungs": np.int32, "ts::dt_m1": np.float32, "ttot": np.float64})
            types.update({k: np.float64 for k in TURBULENCE_ATTRIBUTES})
            types.update({"turbulence::numModes": np.uint64, "rngEngineState": np.uint8})
            types.update({k: np.float64 for k in COOLING_ATTRIBUTES})
            _, attrs = h5part.read_step(path, {}, {k: t for k, t in types.items() if k in present}, step)
            return {**fields, **attrs}
        with np.load(path, allow_pickle=False) as d:
            return {k: d[k] for k in d.files}

    def load_checkpoint(self, path, step=-1):
        """continue from save_checkpoint's file (.h5: its step `step`, negative = the last, as the reference's
        --init file.h5:step; .npz: the one state): set_state with the saved fields and time-steps; returns the time.
        The stored parameters must equal this Sim's (ValueError otherwise: the reference would load them, a Sim's
        parameters are fixed at creation).  Files of the earlier format (time under 'ttot', no 'iteration') load
        with iteration 0."""
        d = self._read_checkpoint(path, step)
        mine = reference_attributes(self.params, self.box, {"ttot": 0.0, "minDt": 0.0, "minDt_m1": 0.0}, 0, 0)
        bad = [k for k in self.PARAM_ATTRIBUTES if k in d and d[k] != mine[k]]
        if bad:
            raise ValueError("restart file parameters differ from this Sim's: " +
                             ", ".join(f"{k}={d[k]!r} (Sim: {mine[k]!r})" for k in bad))
        st = {k: d[k] for k in self.conserved_fields()}
        self.set_state(st, float(d["minDt"]), float(d["minDt_m1"]))
        if self.params.propagator == 2 and "ts::numRungs" in d:
            # HydroVeBdtProp::load (ve_hydro_bdt.hpp:155-168): Timestep numRungs + dt_m1, substep 0, and the rungs
            if "rung" not in d:
                raise ValueError("restart file has ts::numRungs but no 'rung' field")
            rung = np.ascontiguousarray(d["rung"], dtype=np.uint8)
            if rung.shape != (len(st["x"]),):
                raise ValueError(f"restart file's 'rung' has {rung.size} entries for {len(st['x'])} particles")
            ts = SxTimestep()
            ts.numRungs = int(d["ts::numRungs"])
            for k, v in enumerate(np.asarray(d["ts::dt_m1"], np.float32)):
                ts.dt_m1[k] = float(v)
            self._keep_rung = rung
            self.ctx.check(self.L.sx_sim_set_timestep(self.h, C.byref(ts), rung.ctypes.data), "set_timestep")
        if "turbulence::numModes" in d:
            if not self.stirred:
                raise ValueError("restart file carries a turbulence state (turbulence::*) but this Sim is not stirred: "
                                 "call set_turbulence before load_checkpoint")
            # TurbVeProp::load (turb_ve.hpp:123-135); a file without the attributes keeps the state of set_turbulence,
            # as the reference's optional attributes do
            self.set_turbulence_state(d)
        if "cooling::T" in d:
            if self.cooling is None:
                raise ValueError("restart file carries a cooling table (cooling::*) but this Sim does not cool: call "
                                 "set_cooling before load_checkpoint")
            # the table and ct_crit are parameters of this Sim (set_cooling), as PARAM_ATTRIBUTES are: the energy radiated
            # under one curve does not continue under another
            same = (np.array_equal(np.atleast_1d(d["cooling::T"]), self.cooling["T"]) and
                    np.array_equal(np.atleast_1d(d["cooling::lambda"]), self.cooling["lam"]) and
                    float(np.asarray(d["cooling::ct_crit"]).ravel()[0]) == self.ct_crit)
            if not same:
                raise ValueError("restart file's cooling table or ct_crit (cooling::T, cooling::lambda, "
                                 "cooling::ct_crit) differ from those of this Sim's set_cooling")
            # the running total of the energy radiated continues
            self.ctx.check(self.L.sx_sim_set_cooling_radiated(self.h, float(np.asarray(d["cooling::erad"]).ravel()[0])),
                           "set_cooling_radiated")
        self.iteration = int(d["iteration"]) if "iteration" in d else 0
        t = float(d["time"] if "time" in d else d["ttot"])
        self.ctx.check(self.L.sx_sim_set_time(self.h, t), "set_time")
        return t

    def set_skin(self, factor=0.05, max_reuse=24):
        """neighbor lists behind a skin of relative width `factor` (sx_sim_set_skin; 0: sync + search every step)"""
        self.ctx.check(self.L.sx_sim_set_skin(self.h, float(factor), int(max_reuse)), "set_skin")

    def rebuild_lists(self):
        """the next step does a full sync + build of every skin (sx_sim_rebuild_lists)"""
        self.ctx.check(self.L.sx_sim_rebuild_lists(self.h), "rebuild_lists")

    def skin_stats(self):
        out = (C.c_uint64 * 14)()
        self.ctx.check(self.L.sx_sim_skin_stats(self.h, out), "skin_stats")
        d = dict(zip(["builds", "reuse_steps", "stale_clusters", "exact_clusters", "last_stale", "last_exact",
                      "capacity", "plain_steps"], list(out)[:8]))
        d["factor"], d["next_factor"] = out[8] * 1e-6, out[9] * 1e-6
        d["resyncs"] = out[10]
        d["kept_clusters"] = out[11]
        d["frozen_clusters"] = out[12]
        d["early_exact"] = out[13]
        return d

    def neighbor_sets(self):
        """the last step's neighbor lists as {particle id: sorted array of neighbor ids} (sx_sim_export_neighbors)"""
        n = self.size()
        ngmax = int(self.params.ngmax)
        buf = self.ctx.alloc(max(1, n * ngmax), np.uint32)
        try:
            self.ctx.check(self.L.sx_sim_export_neighbors(self.h, buf.ptr), "export_neighbors")
            rows = buf.get()[: n * ngmax].reshape(n, ngmax)
        finally:
            self.ctx.free(buf)
        g = self.get(["id", "nc"])
        ids, nc = g["id"], g["nc"].astype(np.int64)
        return {int(ids[i]): np.sort(ids[rows[i, : min(nc[i] - 1, ngmax)]]) for i in range(n)}

    def step(self):
        rc = self.L.sx_sim_step(self.h)
        if rc != SX_OK:
            raise SxError(f"sx_sim_step failed with code {rc}")
        self.iteration += 1

    def size(self):
        return self.L.sx_sim_size(self.h)

    def scalars(self):
        out = (C.c_double * 6)()
        self.ctx.check(self.L.sx_sim_scalars(self.h, out), "scalars")
        return dict(zip(["minDt", "minDt_m1", "ttot", "minDtCourant", "minDtRho", "egrav"], list(out)))

    def fields(self):
        """(SxFields, id pointer) of the locals (sx_sim_fields); a field the propagator does not keep is None"""
        f = SxFields()
        idp = C.c_void_p()
        self.L.sx_sim_fields(self.h, C.byref(f), C.byref(idp))
        return f, idp.value

    def allocated_fields(self):
        """names of the fields this propagator keeps (the non-NULL members of sx_sim_fields, and id)"""
        f, _ = self.fields()
        return [name for name, _ in FIELD_ORDER if getattr(f, name)] + ["id"]

    def get(self, names):
        f, idp = self.fields()
        n = self.size()
        out = {}
        for name in names:
            ptr = idp if name == "id" else getattr(f, name)
            if not ptr:
                raise KeyError(f"field {name!r} is not allocated under propagator {self.params.propagator}")
            dt = np.uint64 if name == "id" else DTYPES[name]
            out[name] = DeviceArray(self.ctx, ptr, n, dt).get()
        return out

    def stage_times(self):
        ms = (C.c_float * 16)()
        names = (C.c_char_p * 16)()
        k = self.L.sx_sim_stage_times(self.h, ms, 16, names)
        return {names[i].decode(): ms[i] for i in range(k)}

    def kernel_times(self):
        ms = (C.c_float * 16)()
        names = (C.c_char_p * 16)()
        k = self.L.sx_sim_kernel_times(self.h, ms, 16, names)
        return {names[i].decode(): ms[i] for i in range(k)}

    def stats(self):
        s = SxNbStats()
        self.ctx.check(self.L.sx_sim_last_stats(self.h, C.byref(s)), "last_stats")
        return dict(sumNeighbors=s.sumNeighbors, maxNeighbors=s.maxNeighbors, numFailed=s.numFailed,
                    sumCandidates=s.sumCandidates, sumUnion=s.sumUnion, build=s.build, maxUnion=s.maxUnion)

    def conserved(self):
        """computeConservedQuantities over all ranks (sx_sim_conserved)"""
        out = (C.c_double * 13)()
        self.ctx.check(self.L.sx_sim_conserved(self.h, out), "conserved")
        names = ["ecin", "eint", "egrav", "etot", "linmom", "angmom", "totalNeighbors", "px", "py", "pz", "Lx", "Ly",
                 "Lz"]
        return dict(zip(names, list(out)))

    def set_observable(self, kind, **settings):
        """select the observable of observe() (sx_sim_set_observable; observablesFactory, factory.hpp:46-69): "time_energy"
        (the default), "mach_rms", "kh_growth", "wind_bubble" (rhoInt, uExt, rSphere as the reference's settings;
        particleMass, default: the first particle's mass) or "grav_waves" (gravWaveTheta, gravWavePhi)"""
        k, name = obs_kind(kind)
        allowed = {"wind_bubble": {"rhoInt": "rhoBubble", "uExt": "tempWind", "rSphere": "initialMass",
                                   "particleMass": "particleMass"},
                   "grav_waves": {"gravWaveTheta": "gravWaveTheta", "gravWavePhi": "gravWavePhi"}}.get(name, {})
        bad = [s for s in settings if s not in allowed]
        if bad:
            raise TypeError(f"observable {name!r} takes the settings {sorted(allowed)}, not {bad}")
        if name == "wind_bubble":
            missing = [s for s in ("rhoInt", "uExt", "rSphere") if s not in settings]
            if missing:
                raise TypeError(f"observable 'wind_bubble' needs {missing}")
            settings.setdefault("particleMass", 0.0)
        st = SxObsSettings(**{allowed[s]: v for s, v in settings.items()})
        self.ctx.check(self.L.sx_sim_set_observable(self.h, k, C.byref(st)), "set_observable")
        self.observable = name

    def observe(self):
        """the constants.txt row of the current state (sx_sim_observe), a dict under the reference's names in the
        reference's column order (OBS_COLUMNS); nothing is computed on steps after which this is not called"""
        row = (C.c_double * 16)()
        n = C.c_int()
        self.ctx.check(self.L.sx_sim_set_iteration(self.h, int(self.iteration)), "set_iteration")
        self.ctx.check(self.L.sx_sim_observe(self.h, row, 16, C.byref(n)), "observe")
        cols = OBS_COLUMNS[getattr(self, "observable", "time_energy")]
        assert n.value == len(cols)
        d = dict(zip(cols, list(row)))
        d["iteration"] = int(d["iteration"])
        return d

    def map_spec(self, kind="column", axis=2, center=None, width=None, npix=512, depth=0.0):
        """the SxMap of render(): center and width default to the whole box"""
        lim = list(self.box.lim)
        u, v = (axis + 1) % 3, (axis + 2) % 3
        if center is None:
            center = [0.5 * (lim[2 * k] + lim[2 * k + 1]) for k in range(3)]
        if width is None:
            width = (lim[2 * u + 1] - lim[2 * u], lim[2 * v + 1] - lim[2 * v])
        return SxMap(kind, axis, center, width, depth, npix)

    def render(self, kind="column", axis=2, center=None, width=None, npix=512, depth=0.0, field=None, spec=None):
        """a column-density ("column") or slice map of the current state over all ranks (sx_sim_render): (sum0, mean),
        arrays of npix[1] rows of npix[0].  sum0 is the column density or the density on the plane; mean = sum1 / sum0 is
        the mass-weighted mean of `field` (one of MAP_FIELDS) where sum0 > 0 and NaN elsewhere, None without a field.
        center and width default to the whole box; spec: a ready SxMap instead of the keywords."""
        spec = spec if spec is not None else self.map_spec(kind, axis, center, width, npix, depth)
        if field not in MAP_FIELDS:
            raise ValueError(f"unknown map field {field!r}: one of {sorted(k for k in MAP_FIELDS if k)}")
        s0 = np.empty(spec.shape, np.float64)
        s1 = np.empty(spec.shape, np.float64) if MAP_FIELDS[field] else None
        self.ctx.check(self.L.sx_sim_render(self.h, C.byref(spec), MAP_FIELDS[field], s0.ctypes.data,
                                            s1.ctypes.data if s1 is not None else None), "sx_sim_render")
        self.last_sum1 = s1  # the numerator of the mean, None after a render without a field
        if s1 is None:
            return s0, None
        mean = np.full(spec.shape, np.nan)
        np.divide(s1, s0, out=mean, where=s0 > 0)
        return s0, mean

    def map_stats(self):
        """this rank's figures of the last render(): {pairs, bands, longest, footprints}"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.L.sx_sim_map_stats(self.h, out), "sx_sim_map_stats")
        return dict(zip(["pairs", "bands", "longest", "footprints"], [int(v) for v in out]))

    def set_map_pair_cap(self, pairs=0):
        self.ctx.check(self.L.sx_sim_set_map_pair_cap(self.h, int(pairs)), "sx_sim_set_map_pair_cap")

    def spectrum(self, n=128, kind="velocity", weight=None, field=None):
        """the power spectrum of the current state over all ranks (sx_sim_spectrum): (k, power, modes) per shell s with
        k = 2 pi s / L.  kind "velocity": weight None / "mean" (p = 0), "energy" (p = 1/2: the kinetic-energy spectrum)
        or "third" (p = 1/3).  kind "scalar": the mass-weighted mean of `field` (one of MAP_FIELDS) on the mesh, or
        the mesh density without one."""
        if field not in MAP_FIELDS:
            raise ValueError(f"unknown spectrum field {field!r}: one of {sorted(k for k in MAP_FIELDS if k)}")
        if kind not in SPEC_KINDS or weight not in SPEC_WEIGHTS:
            raise ValueError(f"spectrum: kind one of {sorted(SPEC_KINDS)}, weight one of "
                             f"{sorted(k for k in SPEC_WEIGHTS if k)} or None")
        spec = SxSpectrum(kind, weight, n)
        ns = max(1, spectrum_num_shells(n))
        power, modes = np.zeros(ns), np.zeros(ns, np.uint64)
        self.ctx.check(self.L.sx_sim_spectrum(self.h, C.byref(spec), MAP_FIELDS[field], power.ctypes.data,
                                              modes.ctypes.data), "sx_sim_spectrum")
        L = self.box.lim[1] - self.box.lim[0]
        return 2.0 * np.pi * np.arange(ns) / L, power, modes

    def spectrum_stats(self):
        """this rank's figures of the last spectrum(): {pairs, bands, longest, clamped}"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.L.sx_sim_spectrum_stats(self.h, out), "sx_sim_spectrum_stats")
        return dict(zip(["pairs", "bands", "longest", "clamped"], [int(v) for v in out]))

    def set_spectrum_pair_cap(self, pairs=0):
        self.ctx.check(self.L.sx_sim_set_spectrum_pair_cap(self.h, int(pairs)), "sx_sim_set_spectrum_pair_cap")

    def profile_spec(self, edges, quantities=("rho", "p", "vel", "u"), coord="radius", center=None, weight="number",
                     solutions=None):
        """the SxProfile of profile(): center defaults to the box centre"""
        if center is None:
            center = [0.5 * (self.box.lim[2 * k] + self.box.lim[2 * k + 1]) for k in range(3)]
        return SxProfile(edges, quantities, coord, center, weight, solutions)

    def profile(self, edges, quantities=("rho", "p", "vel", "u"), coord="radius", center=None, weight="number",
                solutions=None, spec=None):
        """binned moments of the current state over all ranks with exact, order-independent sums (sx_sim_profile).
        coord: "radius", "x", "y", "z" or a quantity name (a PDF of it); quantities: up to four names of
        PROF_QUANTITIES; weight "number" or "mass"; center: the box centre by default; solutions: {quantity: ("table",
        r, y[, rscale]) or ("noh", dict(time=..., rho0=..., ...))}.  Returns a dict: edges, count, under, over,
        nonfinite, W, and per quantity name mean, sum, sum2, min, max, plus dev and l1 (the mean |q - solution| over all
        particles) where a solution was given; raw holds the arrays with the underflow and overflow entries."""
        spec = spec if spec is not None else self.profile_spec(edges, quantities, coord, center, weight, solutions)
        nb2, nq = int(spec.nbins) + 2, int(spec.nq)
        res = {"count": np.zeros(nb2, np.uint64), "nonfinite": np.zeros(1, np.uint64), "W": np.zeros(nb2)}
        res.update({k: np.zeros((min(nq, PROF_MAX_Q), nb2)) for k in ("S1", "S2", "D", "min", "max")})
        out = SxProfileResult(**{k: v.ctypes.data for k, v in res.items()})
        self.ctx.check(self.L.sx_sim_profile(self.h, C.byref(spec), C.byref(out)), "sx_sim_profile")
        return profile_dict(spec, res)

    def profile_stats(self):
        """this rank's figures of the last profile(): {particles, lds, passes, nonfinite}"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.L.sx_sim_profile_stats(self.h, out), "sx_sim_profile_stats")
        return dict(zip(["particles", "lds", "passes", "nonfinite"], [int(v) for v in out]))

    def fof_spec(self, linking=0.2, length=None, min_members=20, max_groups=4096):
        """the SxFof of fof(): linking in units of the mean interparticle spacing (V_box / N)^(1/3) of the locals,
        or length, an absolute linking length that overrides it"""
        if length is None:
            lim = self.box.lim
            vol = (lim[1] - lim[0]) * (lim[3] - lim[2]) * (lim[5] - lim[4])
            length = float(linking) * (vol / max(1, self.size())) ** (1.0 / 3.0)
        return SxFof(length, min_members, max_groups)

    def fof(self, linking=0.2, length=None, min_members=20, max_groups=4096, labels=False, spec=None):
        """the friends-of-friends groups of the current state (sx_sim_fof; one rank): the dict of Context.fof.  With
        labels=True, label[k] belongs to the particle get(["id"])["id"][k]; labels are the smallest id of a group.  The
        centre of mass is exact for groups narrower than half the box on a periodic axis.  Changes no state."""
        spec = spec if spec is not None else self.fof_spec(linking, length, min_members, max_groups)
        n, cap = self.size(), int(spec.maxGroups)
        arr = _fof_arrays(n, cap, labels)
        res = SxFofResult(**{m: a.ctypes.data for a, m in arr.values()})
        self.ctx.check(self.L.sx_sim_fof(self.h, C.byref(spec), C.byref(res)), "sx_sim_fof")
        return _fof_dict(arr, n, cap)

    def fof_stats(self):
        """the last fof(): {pair tests, union retries, all groups, groups of min_members or more}"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.L.sx_sim_fof_stats(self.h, out), "sx_sim_fof_stats")
        return dict(zip(["pair_tests", "union_retries", "num_all", "num_groups"], [int(v) for v in out]))

    def halos_spec(self, linking=0.2, length=None, min_members=20, max_groups=4096, rho_min=0.0,
                   flags=("moments", "potential"), max_pair_members=0):
        """the SxHalo of halos(): the linking length as in fof_spec; G, muiConst, gamma and the density rule are the
        sim's (sx_sim_halos reads them from its parameters)"""
        length = self.fof_spec(linking, length).linking
        p = self.params
        return SxHalo(length, min_members, max_groups, rho_min, p.propagator == 1, p.g, flags, p.muiConst, p.gamma,
                      max_pair_members)

    def halos(self, linking=0.2, length=None, min_members=20, max_groups=4096, rho_min=0.0,
              flags=("moments", "potential"), max_pair_members=0, labels=False, spec=None):
        """the friends-of-friends groups of the current state among the particles with a density of rho_min or more
        (rho_min <= 0: all), and their properties (sx_sim_halos; one rank): the dict of Context.halos.  flags: any of
        "moments", "thermal", "potential".  The gravity-only propagator serves without a cut and without "thermal".
        Changes no state."""
        spec = spec if spec is not None else self.halos_spec(linking, length, min_members, max_groups, rho_min, flags,
                                                             max_pair_members)
        n, cap, bits = self.size(), int(spec.maxGroups), int(spec.flags)
        arr = _halo_arrays(n, cap, labels, bits)
        res = SxHaloResult(**{m: a.ctypes.data for a, m in arr.values()})
        self.ctx.check(self.L.sx_sim_halos(self.h, C.byref(spec), C.byref(res)), "sx_sim_halos")
        return _halo_dict(arr, n, cap, bits)

    def halos_stats(self):
        """the last halos(): {pair terms evaluated, pair work items, groups with an epot, groups over the cap}"""
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.L.sx_sim_halos_stats(self.h, out), "sx_sim_halos_stats")
        return dict(zip(["pair_terms", "pair_items", "with_epot", "over_cap"], [int(v) for v in out]))

    def twopoint_spec(self, edges, series=("count", "vel"), stride=1, phase=0, mass=False):
        """the SxTwoPoint of twopoint(): absolute bin edges, the series ("count", "vel", "mass" or single names), and
        the targets key % stride == phase on the id column"""
        return SxTwoPoint(edges, series, stride, phase, mass)

    def twopoint(self, edges=None, series=("count", "vel"), stride=1, phase=0, mass=False, spec=None):
        """the pair counts and longitudinal velocity structure functions of the current state binned by separation
        (sx_sim_twopoint; one rank): the dict of Context.twopoint.  stride > 1 takes every stride-th id as a target and
        counts the pairs with at least one target member.  Changes no state."""
        spec = spec if spec is not None else self.twopoint_spec(edges, series, stride, phase, mass)
        arr = _twopoint_arrays(spec)
        res = SxTwoPointResult(**{k: a.ctypes.data for k, a in arr.items()})
        self.ctx.check(self.L.sx_sim_twopoint(self.h, C.byref(spec), C.byref(res)), "sx_sim_twopoint")
        return twopoint_dict(spec, arr, self.box, self.size())

    def twopoint_stats(self):
        """the last twopoint(): {pairs tested, pairs binned, targets, nonfinite, coincident}"""
        out = (C.c_uint64 * 5)()
        self.ctx.check(self.L.sx_sim_twopoint_stats(self.h, out), "sx_sim_twopoint_stats")
        return dict(zip(["pairs_tested", "pairs_binned", "targets", "nonfinite", "coincident"], [int(v) for v in out]))

    def write_constants(self, fileobj):
        """append the row of observe() to a constants.txt (format_constants_row); returns the row"""
        row = self.observe()
        fileobj.write(format_constants_row(row, getattr(self, "observable", "time_energy")))
        return row

    def timestep(self):
        """ve-bdt: the Timestep after the last substep (sx_sim_timestep)"""
        ts = SxTimestep()
        self.ctx.check(self.L.sx_sim_timestep(self.h, C.byref(ts)), "timestep")
        return dict(nextDt=ts.nextDt, elapsedDt=ts.elapsedDt, totDt=ts.totDt, numRungs=ts.numRungs,
                    substep=ts.substep, rungRanges=list(ts.rungRanges), dt_m1=list(ts.dt_m1),
                    dt_drift=list(ts.dt_drift))

    def gravity_stats(self):
        out = (C.c_uint64 * 3)()
        self.L.sx_sim_gravity_stats(self.h, out)
        return dict(halos=out[0], far_cells=out[1], remote_cells=out[2])

    def set_gravity_counting(self, enable=True):
        """count the gravity interactions of the following steps (sx_sim_set_gravity_counting; off by default)"""
        self.ctx.check(self.L.sx_sim_set_gravity_counting(self.h, 1 if enable else 0), "set_gravity_counting")

    def set_gravity_check(self, num_targets=4096):
        """arm the next step's force-error check of the walk against the direct sum on about num_targets sampled
        targets (sx_sim_set_gravity_check; 0 disarms)"""
        self.ctx.check(self.L.sx_sim_set_gravity_check(self.h, int(num_targets)), "set_gravity_check")

    def gravity_check(self):
        """the last armed step's |a_walk - a_direct| / |a_direct| over the sample (sx_sim_gravity_check)"""
        out = (C.c_double * 6)()
        self.ctx.check(self.L.sx_sim_gravity_check(self.h, out), "gravity_check")
        d = dict(zip(["targets", "mean", "median", "p99", "max", "rms"], list(out)))
        d["targets"] = int(d["targets"])
        return d

    def gravity_interactions(self):
        """P2P and M2P interactions of the last step (sx_sim_gravity_interactions; the reference's BhStats)"""
        out = (C.c_uint64 * 2)()
        self.ctx.check(self.L.sx_sim_gravity_interactions(self.h, out), "gravity_interactions")
        return dict(p2p=out[0], m2p=out[1])

    def close(self):
        if self.h:
            self.L.sx_sim_destroy(self.h)
            self.h = None
