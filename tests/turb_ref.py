"""numpy / Python restatement of the turbulence stirring, written from the formulas (no reference file is read):

* libstdc++'s std::mt19937 + generate_canonical<double, 53> + std::normal_distribution<double> (Marsaglia polar method
  with its saved second value) + std::uniform_real_distribution<double>;
* the derived constants and the mode table of spectral forms 0 (band) and 1 (parabola): every lattice point
  k = 2 pi (i, j, k) / L, i, j, k >= 0, with stirMin <= |k| <= stirMax, in i-major order, as the four sign variants
  (+j +k), (-j +k), (+j -k), (-j -k);
* the Ornstein-Uhlenbeck step x <- x f + sigma sqrt(1 - f^2) z, f = exp(-dt / ts), and the Helmholtz projection of
  the six phases of a mode into three real and three imaginary coefficients;
* the stirring acceleration solWeightNorm sum_m amplitude_m (Re_m cos(k_m x) - Im_m sin(k_m x)) in double.

Scalar libm calls go through `math` (the platform libm), elementwise arithmetic through numpy float64 (IEEE).
"""
import math

import numpy as np

DEFAULTS = dict(solWeight=0.5, stMaxModes=100000, Lbox=1.0, stEnergyPrefac=5.0e-3, stMachVelocity=0.3, epsilon=1e-15,
                rngSeed=251299, stSpectForm=1, powerLawExp=5.0 / 3, anglesExp=2.0)


class StdRng:
    """std::mt19937 seeded with `seed` and the libstdc++ distributions on top of it"""

    def __init__(self, seed):
        self.bg = np.random.RandomState(int(seed) & 0xFFFFFFFF)._bit_generator  # init_genrand(seed), as mt19937(seed)

    def raw(self):
        return int(self.bg.random_raw())

    def canonical(self):
        """generate_canonical<double, 53>: two 32-bit words, low word first"""
        lo, hi = self.raw(), self.raw()
        r = (float(lo) + float(hi) * 4294967296.0) / 18446744073709551616.0
        return math.nextafter(1.0, 0.0) if r >= 1.0 else r

    def uniform(self):
        return self.canonical() * 1.0 + 0.0

    def normals(self, n, mean=0.0, stddev=1.0):
        """n draws from ONE std::normal_distribution<double>(mean, stddev) object"""
        out, saved = [], None
        for _ in range(n):
            if saved is not None:
                ret, saved = saved, None
            else:
                while True:
                    x = 2.0 * self.canonical() - 1.0
                    y = 2.0 * self.canonical() - 1.0
                    r2 = x * x + y * y
                    if not (r2 > 1.0 or r2 == 0.0):
                        break
                mult = math.sqrt(-2 * math.log(r2) / r2)
                saved = x * mult
                ret = y * mult
            out.append(ret * stddev + mean)
        return np.array(out)


def constants(s):
    twopi = 2.0 * math.pi
    L, v = s["Lbox"], s["stMachVelocity"]
    energy = s["stEnergyPrefac"] * math.pow(v, 3) / L
    decay = L / (2.0 * v)
    sw = s["solWeight"]
    return dict(stirMin=(1.0 - s["epsilon"]) * twopi / L, stirMax=(3.0 + s["epsilon"]) * twopi / L, decayTime=decay,
                variance=math.sqrt(energy / decay),
                solWeightNorm=math.sqrt(3.0) * math.sqrt(3.0 / 3.0) / math.sqrt(1.0 - 2.0 * sw + 3.0 * sw * sw))


def mode_table(s):
    """forms 0 and 1: (modes [M, 3], amplitudes [M])"""
    assert s["stSpectForm"] in (0, 1)
    c = constants(s)
    twopi, L = 2.0 * math.pi, s["Lbox"]
    lo, hi = c["stirMin"], c["stirMax"]
    kc = 0.5 * (lo + hi) if s["stSpectForm"] == 1 else lo
    pre = -4.0 / ((hi - lo) * (hi - lo))
    top = int(math.floor(hi * L / twopi)) + 1
    modes, amps = [], []
    for i in range(top + 1):
        kx = twopi * i / L
        for j in range(top + 1):
            ky = twopi * j / L
            for k in range(top + 1):
                kz = twopi * k / L
                kn = math.sqrt(kx * kx + ky * ky + kz * kz)
                if not (lo <= kn <= hi):
                    continue
                if len(amps) + 4 > s["stMaxModes"]:
                    continue
                a = 1.0
                if s["stSpectForm"] == 1:
                    a = abs(pre * (kn - kc) * (kn - kc) + 1.0)
                a = 2.0 * math.sqrt(a) * math.pow(kc / kn, 1.0)
                for sy, sz in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                    modes.append((kx, sy * ky, sz * kz))
                    amps.append(a)
    return np.array(modes).reshape(-1, 3), np.array(amps)


def ou_step(phases, variance, dt, decay, normals):
    a = math.exp(-dt / decay)
    b = math.sqrt(1.0 - a * a)
    return phases * a + variance * b * normals


def project(phases, modes, sol_weight):
    """(phasesReal [M, 3], phasesImag [M, 3]) from the OU phases [6 M] (per mode: re x, im x, re y, im y, re z, im z)"""
    ph = phases.reshape(-1, 3, 2)
    kk = np.zeros(len(modes))
    ka = np.zeros(len(modes))
    kb = np.zeros(len(modes))
    for j in range(3):
        kk = kk + modes[:, j] * modes[:, j]
        ka = ka + modes[:, j] * ph[:, j, 1]
        kb = kb + modes[:, j] * ph[:, j, 0]
    re, im = np.empty((len(modes), 3)), np.empty((len(modes), 3))
    for j in range(3):
        diva = modes[:, j] * ka / kk
        divb = modes[:, j] * kb / kk
        curla = ph[:, j, 0] - divb
        curlb = ph[:, j, 1] - diva
        re[:, j] = sol_weight * curla + (1.0 - sol_weight) * divb
        im[:, j] = sol_weight * curlb + (1.0 - sol_weight) * diva
    return re, im


def stir(x, y, z, modes, re, im, amplitudes, sol_weight_norm):
    """the stirring acceleration [n, 3] in double"""
    acc = np.zeros((len(x), 3))
    for m in range(len(modes)):
        ang = modes[m, 0] * x + modes[m, 1] * y + modes[m, 2] * z
        c, s = np.cos(ang), np.sin(ang)
        for e in range(3):
            acc[:, e] += amplitudes[m] * (re[m, e] * c - im[m, e] * s)
    return sol_weight_norm * acc


def stir_scale(re, im, amplitudes, sol_weight_norm):
    """S = solWeightNorm sum_m amplitude_m (|Re_m| + |Im_m|) per component: the magnitude of the terms of the sum"""
    return sol_weight_norm * np.sum(amplitudes[:, None] * (np.abs(re) + np.abs(im)), axis=0)


def stir_bound(num_modes, scale, a_before):
    """the reference accumulates numModes terms in float and adds the result to a float acceleration: at most half an
    ulp of a partial sum <= S per term, and the rounding of the stored sum"""
    return num_modes * 2.0 ** -24 * scale[None, :] + 2.0 ** -23 * np.abs(a_before)


def ulp_diff(a, b):
    """distance in units in the last place of b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))
