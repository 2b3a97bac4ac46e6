"""tests/golden/rys_boys_moments.npz: the arguments X = rho |PQ|^2 at which the root / weight lookups of the integral kernels are
probed (dqc_probe_rys, tests/test_gpu_rys_range.py; the table itself in tests/test_oracle_cpu.py) and the Boys functions
F_0 ... F_17 at each of them, evaluated with mpmath at 50 digits and rounded to double.

    x_n<N>, f_n<N>   N = 1 ... 9: arguments of the N-root lookups (Chebyshev intervals of width 2.5 up to XMAX = 35 + 5 N, the
                     Hermite asymptote from there on) and F (len, 18).  Per interval k: 2.5 k and its two neighbouring doubles,
                     the midpoint, three seeded random interior points; 0, 1e-12; XMAX and its two neighbours; 1.5 XMAX, 200,
                     1e3, 1e5
    x_boys, f_boys   arguments of the F_0 / F_1 Taylor table (nodes i/8 up to 40): every node, every half-way point
                     i/8 + 1/16 (the largest Taylor step) with its two neighbouring doubles, 40 with its neighbours, 60, 1e3, 1e5

The file is written without time stamps: running this script again reproduces it byte for byte.
    python tools/make_rys_golden.py [--check]      (--check: compare with the committed file instead of writing)"""
import io
import os
import sys
import zipfile

import numpy as np
from mpmath import mp, mpf, gammainc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rys_boys_moments.npz")
KMAX = 17
WIDTH = 2.5
SEED = 20161


def boys_row(X):
    """F_0 ... F_KMAX at the double X: F_k = gamma(k + 1/2, X) / (2 X^(k + 1/2)), 1 / (2k + 1) at zero"""
    if X == 0.0:
        return [1.0 / (2 * k + 1) for k in range(KMAX + 1)]
    x = mpf(X)
    return [float(gammainc(mpf(k) + mpf(1) / 2, 0, x) / (2 * x ** (mpf(k) + mpf(1) / 2))) for k in range(KMAX + 1)]


def rys_points(n):
    rng = np.random.default_rng(SEED + n)
    xmax = 35.0 + 5.0 * n
    xs = [0.0, 1e-12]
    for k in range(14 + 2 * n):
        lo = WIDTH * k
        xs += [lo, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), lo + 0.5 * WIDTH]
        xs += list(lo + WIDTH * rng.uniform(0.0, 1.0, 3))
    xs += [xmax, np.nextafter(xmax, 0.0), np.nextafter(xmax, np.inf), 1.5 * xmax, 200.0, 1e3, 1e5]
    return np.unique(np.array([x for x in xs if x >= 0.0]))


def boys_points():
    xs = [i / 8.0 for i in range(321)]
    for i in range(320):
        h = i / 8.0 + 1.0 / 16.0
        xs += [h, np.nextafter(h, 0.0), np.nextafter(h, np.inf)]
    xs += [np.nextafter(40.0, 0.0), np.nextafter(40.0, np.inf), 60.0, 1e3, 1e5]
    return np.unique(np.array(xs))


def make():
    mp.dps = 50
    arrays = {}
    for n in range(1, 10):
        x = rys_points(n)
        arrays["x_n%d" % n] = x
        arrays["f_n%d" % n] = np.array([boys_row(float(v)) for v in x])
    x = boys_points()
    arrays["x_boys"] = x
    arrays["f_boys"] = np.array([boys_row(float(v)) for v in x])
    return arrays


def to_bytes(arrays):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name], dtype=np.float64), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    return buf.getvalue()


if __name__ == "__main__":
    data = to_bytes(make())
    if "--check" in sys.argv:
        same = open(OUT, "rb").read() == data
        print("%s: %s" % (OUT, "identical" if same else "DIFFERENT"))
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print("%s: %d bytes" % (OUT, len(data)))
