"""Pointwise fixtures for the functional kernels of dqc_amd/csrc/xc.hip, first AND second order, from the 50-digit reference of
oracle/xc_exact.py: tests/golden/xc_exact_unpol.npz and tests/golden/xc_exact_pol.npz.

Per functional and point each file holds the truth and the SCALE (sum of the absolute values of the same derivative of the
additive parts of the functional, see oracle/xc_exact.py) of

    unpolarised   row 0: e;  1, 2: de/drho, de/dsigma;  3, 4: the Hessian in (rho, sigma) times (d rho, d sigma);
                  5, 6, 7: the rows (rho_u, sigma_uu, sigma_ud) of the POLARISED Hessian at rho_u = rho_d = rho / 2 times the spin-flip
                  response d rho_u = -d rho_d = d rho / 2 (the triplet kernel);  8, 9: de/dsigma_uu, de/dsigma_ud of the polarised form
    polarised     row 0: e;  1 .. 5: the gradient by (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd);  6 .. 10: the Hessian times the response

as `<name>_val[0]` (truth) and `<name>_val[1]` (scale), with d sigma = 2 grad rho . grad d rho and its polarised analogues.  The tests
compose v_grad = 2 v_sigma grad rho and the d v_grad of tools/make_fxc_golden.py's docstring from these rows, and the scales of those
outputs from the same formulas with absolute values.  `<name>_double_err` = the largest |torch-double - truth| / scale of the
composed outputs over the points, for (e, first order, second order): the tolerance of the GPU tests is derived from it.  `old_<name>` holds the truth at the
points of tests/golden/oracle_fxc_pointwise.npz (the finite-difference fixture of the Hessian tests): rows v_sigma, H d (unpolarised),
the three v_sigma and the five H d (polarised).

Points (all seeded; `cls` labels them):
    unpolarised  0  bulk: 256 points, rho log-uniform in [1e-14, 1e4], s log-uniform in [1e-6, 1e2], every eighth with grad rho = 0
                    exactly; responses up to 30 % of the ground state
                 1  rho = 3 / (4 pi) (1 + d), the branch point r_s = 1 of PZ81 / P86      } d = +-1e-3, +-1e-6, +-1e-12
                 2  x_s = 1e-4 (1 + d), the series switch of x asinh x in gga_x_b88       }
                 3  b s = 1e-4 (1 + d), b = 1 / X2S, the same switch in gga_x_pw91        }
                 4  rho = 1.1e-15 (just above the density cutoff)     5  rho = 0.9e-15 (below it: every output exactly zero)
    polarised    0  128 points, rho in [1e-6, 1e3], 1 - |zeta| log-uniform in [1e-8, 1] (every eighth: zeta = 0 exactly), per-spin
                    s in [1e-3, 30], grad rho_u and grad rho_d in turn parallel, antiparallel, orthogonal, and grad rho_d = 0
                 1  fully polarised: rho_d = 0 and grad rho_d = 0 exactly        2  below the density cutoff

Excluded from the comparison (printed, and asserted <= 2 % of the (functional, point, output) triples by tests/test_xc_exact_cpu.py):
the d v_grad of gga_x_g96 of a spin whose gradient is exactly zero (its v_sigma ~ sigma^(-1/4) does not exist there), and the
outputs of the empty spin at fully polarised points.

Imports oracle.xc_exact only, never dqc_amd or oracle.xc.      usage: python tools/make_xc_exact_golden.py [processes]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oracle import xc_exact as xe  # noqa: E402

NAMES = xe.NAMES
GOLDEN = os.path.join(ROOT, "tests", "golden")
NBULK, NPOL, NFULL = 256, 128, 4
SEAM_D = (1e-3, -1e-3, 1e-6, -1e-6, 1e-12, -1e-12)
KS = 2.0 * (3.0 * np.pi ** 2) ** (1.0 / 3)      # |grad rho| = s KS rho^(4/3)
X2S = 1.0 / (2.0 * (6.0 * np.pi ** 2) ** (1.0 / 3))
UNPOL_OUTPUTS, POL_OUTPUTS = xe.UNPOL_OUTPUTS, xe.POL_OUTPUTS


def _unit(rng, n):
    u = rng.normal(size=(3, n))
    return u / np.linalg.norm(u, axis=0)


def _response(rng, rho, grho):
    n = rho.shape[0]
    gnorm = np.linalg.norm(grho, axis=0)
    return rho * rng.uniform(-0.3, 0.3, n), np.maximum(gnorm, 1e-3 * rho) * rng.uniform(-0.3, 0.3, (3, n))


def unpol_points():
    rng = np.random.default_rng(20261001)
    rho = 10.0 ** rng.uniform(-14, 4, NBULK)
    s = 10.0 ** rng.uniform(-6, 2, NBULK)
    s[7::8] = 0.0
    cls = [0] * NBULK
    for d in SEAM_D:  # r_s = 1
        rho, s, cls = np.append(rho, 3.0 / (4.0 * np.pi) * (1.0 + d)), np.append(s, 0.7), cls + [1]
    for c, r0 in ((2, 0.3), (3, 7.0)):  # x_s = |grad rho / 2| / (rho / 2)^(4/3) = s / X2S
        for d in SEAM_D:
            rho, s, cls = np.append(rho, r0), np.append(s, 1e-4 * (1.0 + d) * X2S), cls + [c]
    rho, s, cls = np.append(rho, [1.1e-15, 0.9e-15]), np.append(s, [0.4, 0.4]), cls + [4, 5]
    grho = s * KS * rho ** (4.0 / 3) * _unit(rng, rho.shape[0])
    drho, dgrho = _response(rng, rho, grho)
    return {"rho": rho, "grho": grho, "drho": drho, "dgrho": dgrho, "cls": np.array(cls)}


def pol_points():
    rng = np.random.default_rng(20261002)
    n = NPOL + NFULL + 2
    rho = 10.0 ** rng.uniform(-6, 3, n)
    omz = 10.0 ** rng.uniform(-8, 0, n)
    zeta = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0) * (1.0 - omz)
    zeta[::8] = 0.0
    ru, rd = 0.5 * rho * (1.0 + zeta), 0.5 * rho * (1.0 - zeta)
    cls = np.zeros(n, dtype=int)
    cls[NPOL:NPOL + NFULL] = 1
    ru[cls == 1], rd[cls == 1] = 10.0 ** rng.uniform(-3, 2, NFULL), 0.0
    cls[-2:] = 2
    ru[-2:], rd[-2:] = [0.6e-15, 0.2e-15], [0.3e-15, 0.2e-15]
    su, sd = 10.0 ** rng.uniform(-3, np.log10(30.0), n), 10.0 ** rng.uniform(-3, np.log10(30.0), n)
    a = _unit(rng, n)
    b = _unit(rng, n)
    b = b - (a * b).sum(0) * a
    b /= np.linalg.norm(b, axis=0)
    geo = np.arange(n) % 4  # parallel, antiparallel, orthogonal, grad rho_d = 0
    dird = np.where(geo == 0, a, np.where(geo == 1, -a, b))
    # per spin: x_s = |grad rho_s| / rho_s^(4/3) = s / X2S
    gu = su / X2S * ru ** (4.0 / 3) * a
    gd = np.where(geo == 3, 0.0, sd / X2S * rd ** (4.0 / 3)) * dird
    gd[:, cls == 1] = 0.0
    dru, dgu = _response(rng, ru, gu)
    drd, dgd = _response(rng, rd, gd)
    dgd[:, cls == 1] = 0.0
    return {"rho_u": ru, "rho_d": rd, "grho_u": gu, "grho_d": gd, "drho_u": dru, "drho_d": drd, "dgrho_u": dgu, "dgrho_d": dgd, "cls": cls}


# ------------------------------------------------------------------------------------------------ the rows of one point
def _sig(a, b):
    return float((a * b).sum())


def unpol_row(name, p, i):
    """(2, 10) truth and scale at point i of an unpolarised point set (zeros below the density cutoff)"""
    out = np.zeros((2, 10))
    g, dg = p["grho"][:, i], p["dgrho"][:, i]
    pt = xe.effective_point_unpol(p["rho"][i], _sig(g, g))
    if pt is None:
        return out
    x, dz, dps, zero = pt
    r = xe.mp_eval(name, x, dz, delta=[p["drho"][i], 2.0 * _sig(g, dg)], dps=dps, zero=zero)
    out[:, 0] = r["e"]
    for k in range(2):
        out[:, 1 + k], out[:, 3 + k] = r["d1"][k], r["d2"][k]
    # the spin-flip response: d rho_u = -d rho_d = d rho / 2, d sigma_uu = -d sigma_dd = g . dg / 2, d sigma_ud = 0
    xp = list(xe.unpolarised(*x))
    t = xe.mp_eval(name, xp, dz, delta=[0.5 * p["drho"][i], -0.5 * p["drho"][i], 0.5 * _sig(g, dg), 0.0, -0.5 * _sig(g, dg)],
                   variables=(0, 2, 3), dps=dps, zero=(2, 3, 4) if zero else ())
    for j, k in enumerate((0, 2, 3)):
        out[:, 5 + j] = t["d2"][k]
    out[:, 8], out[:, 9] = t["d1"][2], t["d1"][3]
    return out


def pol_inputs(p, i):
    gu, gd, dgu, dgd = p["grho_u"][:, i], p["grho_d"][:, i], p["dgrho_u"][:, i], p["dgrho_d"][:, i]
    x = (p["rho_u"][i], p["rho_d"][i], _sig(gu, gu), _sig(gu, gd), _sig(gd, gd))
    delta = [p["drho_u"][i], p["drho_d"][i], 2.0 * _sig(gu, dgu), _sig(gu, dgd) + _sig(dgu, gd), 2.0 * _sig(gd, dgd)]
    return x, delta


def pol_row(name, p, i):
    """(2, 11) truth and scale at point i of a polarised point set"""
    out = np.zeros((2, 11))
    x, delta = pol_inputs(p, i)
    pt = xe.effective_point(*x)
    if pt is None:
        return out
    r = xe.mp_eval(name, list(pt[0]), pt[1], delta=delta, dps=pt[2], zero=pt[3])
    out[:, 0] = r["e"]
    for k in range(5):
        out[:, 1 + k], out[:, 6 + k] = r["d1"][k], r["d2"][k]
    return out


def old_points():
    fx = np.load(os.path.join(GOLDEN, "oracle_fxc_pointwise.npz"))
    r = {k: fx["r_" + k] for k in ("rho", "grho", "drho", "dgrho")}
    q = {"%s_%s" % (k, s): fx["p_%s_%s" % (k, s)] for k in ("rho", "grho", "drho", "dgrho") for s in "ud"}
    return r, q


def _job(job):
    kind, name, i = job
    p = _POINTS[kind]
    return kind, name, i, (unpol_row if kind in ("unpol", "old_unpol") else pol_row)(name, p, i)


_POINTS = {}


def load_points():
    if not _POINTS:
        _POINTS["unpol"], _POINTS["pol"] = unpol_points(), pol_points()
        _POINTS["old_unpol"], _POINTS["old_pol"] = old_points()
    return _POINTS


# ------------------------------------------------------------------------------------------------ exclusions and the yardstick
def excluded_share(kind, p):
    tot = exc = 0
    for name in NAMES:
        m = (xe.unpol_excluded if kind == "unpol" else xe.pol_excluded)(name, p)
        for o, mask in m.items():
            if "grad" in o and not xe.IS_GGA[name]:
                continue  # an LDA functional has no gradient outputs
            tot += mask.size
            exc += int(mask.sum())
    return exc / tot


def double_rows(kind, name, p, idx=None):
    """the torch-double backend at the points idx of a point set, in the rows of `<name>_val` (zeros below the cutoff)"""
    n = (p["rho"] if kind == "unpol" else p["rho_u"]).shape[0]
    idx = range(n) if idx is None else idx
    nrow = 10 if kind == "unpol" else 11
    out = np.zeros((nrow, n))
    xs, dzs, dls, tds, live = [], [], [], [], []
    for i in idx:
        if kind == "unpol":
            g, dg = p["grho"][:, i], p["dgrho"][:, i]
            pt = xe.effective_point_unpol(p["rho"][i], _sig(g, g))
            delta = [p["drho"][i], 2.0 * _sig(g, dg)]
        else:
            x, delta = pol_inputs(p, i)
            pt = xe.effective_point(*x)
        if pt is None:
            continue
        live.append(i)
        if kind == "unpol":
            tds.append([0.5 * delta[0], -0.5 * delta[0], 0.25 * delta[1], 0.0, -0.25 * delta[1]])
        xs.append([float(v) for v in pt[0]])
        dzs.append(float(pt[1]))
        dls.append(delta)
    if not live:
        return out
    x, dz, dl = np.array(xs).T, np.array(dzs), np.array(dls).T
    e, d1, d2 = xe.td_eval(name, x, dz, dl)
    out[0, live] = e
    nv = x.shape[0]
    out[1:1 + nv, live], out[1 + nv:1 + 2 * nv, live] = d1, d2
    if kind == "unpol":
        _, t1, t2 = xe.td_eval(name, np.array(xe.unpolarised(x[0], x[1])), dz, np.array(tds).T)
        out[5:8, live], out[8:10, live] = t2[[0, 2, 3]], t1[[2, 3]]
    return out


def compose(kind, rows, p, absolute=False):
    if kind == "unpol":
        return xe.compose_unpol(rows, p["grho"], p["dgrho"], absolute)
    return xe.compose_pol(rows, p["grho_u"], p["grho_d"], p["dgrho_u"], p["dgrho_d"], absolute)


def double_err(kind, name, p, val, idx=None):
    """the largest scaled error of the OUTPUTS composed from the torch-double backend against those composed from the truth
    `val` (2, rows, n), over the points idx (default: all): (e, first order, second order)"""
    got = compose(kind, double_rows(kind, name, p, idx), p)
    truth, scale = compose(kind, val[0], p), compose(kind, val[1], p, absolute=True)
    exc = (xe.unpol_excluded if kind == "unpol" else xe.pol_excluded)(name, p)
    n = val.shape[2]
    sel = np.ones(n, dtype=bool)
    if idx is not None:
        sel[:] = False
        sel[list(idx)] = True
    err = [0.0, 0.0, 0.0]
    for o in got:
        c = xe.output_class(o)
        err[c] = max(err[c], xe.scaled_error(got[o], truth[o], scale[o], exc[o] | ~sel))
    return np.array(err)


# ------------------------------------------------------------------------------------------------ the meta-GGA fixtures
MGGA_DOC = """Pointwise fixtures for the four meta-GGA functionals of dqc_amd/csrc/xc.hip (mgga_x_scan, mgga_c_scan, mgga_x_tpss, mgga_c_tpss),
value and first order, from the 50-digit reference of oracle/xc_exact.py: tests/golden/xc_exact_mgga_unpol.npz, xc_exact_mgga_pol.npz
(tools/make_xc_exact_golden.py, whose docstring describes the LDA / GGA fixtures).

    unpolarised   `<name>_val[0 / 1]` (truth / scale), rows: e; de/drho, de/dsigma, de/dtau
    polarised     rows: e; the gradient by (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd, tau_u, tau_d)
    `<name>_double_err` (point class, output class): the largest |torch-double - truth| / scale of the composed outputs over the points
    of a class, for (e, first order) -- per class, so that an ill-conditioned class (alpha = (tau - tau_W) / tau_unif where tau -> tau_W)
    does not loosen the bar of the others.  `classes`: the names of the point classes, `p_cls` the class of each point.
    `extra`: LDA / GGA functionals whose first-order truth at the same points is held in the same rows (rows of tau: zero), for term
    lists that mix them with the meta-GGAs.

Every gradient lies along a coordinate axis with a 26-bit mantissa: sigma = |grad rho|^2 is then the same double in any order of the
operations, and tau_W = sigma / (8 rho) near tau is conditioned by the functional alone.

Points (seeded):
    unpolarised  0  bulk: 256 points, rho log-uniform in [1e-14, 1e4] (both sides of r_s = 1), s log-uniform in [1e-6, 1e2], every eighth
                    with grad rho = 0 exactly; alpha from {1e-9, 0.5, 2, 50, 1e4}, and alpha = 0 (tau = 0) where grad rho = 0 (with a
                    gradient alpha = 0 is z = 1, where the potential of TPSS jumps: not sampled)
                 1  seam: 1 - alpha = +-{1e-14, 1e-13, 1e-11, 1e-9, 1e-6, 1e-3, 1e-2, 0.1} at (rho, s) = (0.3, 0.7), (1e-3, 3), (50, 0)
                 2  iso-orbital: tau = tau_W (1 + {1e-12, 1e-9, 1e-6}) and tau = 0.9 tau_W at (rho, s) = (0.3, 0.7), (1e-3, 3), (20, 100), (1e-8, 1)
                 3  tau floor: rho = 1e-13, 1e-14, 3e-13 with alpha = 1, s = 0.5 (tau < 1e-20), and tau = 0 exactly
                 4  zero gradient: grad rho = 0 exactly, alpha = 0.5, 1, 2 at rho = 1e-5, 0.3, 100
                 5  density cutoff: rho = 1.1e-15 (live) and 0.9e-15 (every output exactly zero)
    polarised    0  120 points, rho in [1e-3, 1e2], 1 - |zeta| in turn 1e-1, 1e-4, 1e-8, 1e-10 and zeta = 0; per-spin s in [1e-3, 30]; grad rho_u
                    and grad rho_d in turn parallel, antiparallel, orthogonal, and grad rho_d = 0 (sigma_ud < 0 when antiparallel); tau in
                    turn per spin (alpha_s from {0.05, 0.5, 2, 50}), the same total split evenly, and split 95 / 5 (a spin may get tau_s < tau_W,s)
                 1  fully polarised: rho_d = 0, grad rho_d = 0, tau_d = 0 exactly
                 2  one electron: fully polarised with tau_u = tau_W (1 + 1e-12)
                 3  seam: 1 - alpha = +-{1e-13, 1e-6, 1e-2} of the up spin (exchange), then of the total density (SCAN correlation), zeta = 0.3
                 4  zero gradient per spin, alpha_s = 0.5, 1, 2        5  below the density cutoff

Excluded (asserted <= 2 % of the triples by tests/test_xc_exact_cpu.py): v_rho, v_grad (and for exchange v_tau) of the empty spin at
fully polarised points -- nothing else."""
MGGA_NAMES = list(getattr(xe, "MGGA_NAMES", ()))  # (the LDA / GGA half of this tool runs on a reference without the meta-GGAs)
MGGA_CLASSES = {"mgga_unpol": ("bulk", "seam", "iso-orbital", "tau-floor", "zero-gradient", "stationary", "cutoff"),
                "mgga_pol": ("polarised", "nearly full", "fully polarised", "one-electron", "seam", "zero-gradient", "stationary", "cutoff")}
TAU_UNIF = 0.3 * (3.0 * np.pi ** 2) ** (2.0 / 3)   # tau_unif = TAU_UNIF rho^(5/3)
SEAM_MGGA = (1e-14, 1e-13, 1e-11, 1e-9, 1e-6, 1e-3, 1e-2, 0.1)


def _short(x):
    """x rounded to a 26-bit mantissa: its square, and its product with another such number, are exact in double"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** 26) / 2.0 ** 26, e)


def _axis(k, n):
    a = np.zeros((3, n))
    a[np.asarray(k) % 3, np.arange(n)] = 1.0
    return a


def mgga_unpol_points():
    rng = np.random.default_rng(20261101)
    rho = 10.0 ** rng.uniform(-14, 4, NBULK)
    s = 10.0 ** rng.uniform(-6, 2, NBULK)
    s[7::8] = 0.0
    alpha = rng.choice([1e-9, 0.5, 2.0, 50.0, 1e4], NBULK)
    alpha[7::8] = np.resize([0.0, 1e-9, 0.5, 2.0, 50.0, 1e4], NBULK // 8)
    close = (alpha == 1e-9) & (s > 1.0)  # 1 - z = alpha tau_unif / tau: kept at the closest approach of the iso-orbital class
    s[close] = 10.0 ** rng.uniform(-6, 0, int(close.sum()))
    cls = [0] * NBULK
    tw_factor = []  # where not None: tau = factor * tau_W instead of tau_W + alpha tau_unif

    def add(r, s_, a, c, f=None):
        nonlocal rho, s, alpha, cls
        rho, s, alpha, cls = np.append(rho, r), np.append(s, s_), np.append(alpha, a), cls + [c]
        tw_factor.append((rho.shape[0] - 1, f))
    for r0, s0 in ((0.3, 0.7), (1e-3, 3.0), (50.0, 0.05)):
        for d in SEAM_MGGA:
            add(r0, s0, 1.0 - d, 1)
            add(r0, s0, 1.0 + d, 1)
    for r0, s0 in ((0.3, 0.7), (1e-3, 3.0), (20.0, 100.0), (1e-8, 1.0)):
        for f in (1.0 + 1e-12, 1.0 + 1e-9, 1.0 + 1e-6, 0.9):
            add(r0, s0, 0.0, 2, f)
    for r0 in (1e-13, 1e-14, 3e-13):
        add(r0, 0.5, 1.0, 3)
    for r0, s0 in ((1e-13, 0.0), (1e-3, 0.0), (10.0, 0.0), (0.3, 0.7)):
        add(r0, s0, 0.0, 3, 0.0)
    for r0 in (1e-5, 0.3, 100.0):
        for a in (0.5, 1.0, 2.0):
            add(r0, 0.0, a, 5 if a == 1.0 else 4)
    add(1.1e-15, 0.4, 0.5, 6)
    add(0.9e-15, 0.4, 0.5, 6)
    n = rho.shape[0]
    g = _short(s * KS * rho ** (4.0 / 3)) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    grho = g * _axis(np.arange(n), n)
    tau_w = g * g / (8.0 * rho)
    tau = tau_w + alpha * TAU_UNIF * rho ** (5.0 / 3)
    for i, f in tw_factor:
        if f is not None:
            tau[i] = f * tau_w[i]
    return {"rho": rho, "grho": grho, "tau": tau, "cls": np.array(cls)}


NPOL_MGGA = 120


def mgga_pol_points():
    rng = np.random.default_rng(20261102)
    n0 = NPOL_MGGA
    i0 = np.arange(n0)
    rho = 10.0 ** rng.uniform(-3, 2, n0)
    omz = np.resize([1e-1, 1e-4, 1e-8, 1e-10, 1.0], n0)
    minor = 0.5 * rho * omz
    up = rng.uniform(size=n0) < 0.5  # the majority spin
    ru, rd = np.where(up, rho - minor, minor), np.where(up, minor, rho - minor)
    su, sd = 10.0 ** rng.uniform(-3, np.log10(30.0), n0), 10.0 ** rng.uniform(-3, np.log10(30.0), n0)
    geo = i0 % 4  # parallel, antiparallel, orthogonal, grad rho_d = 0
    au, ad = rng.choice([0.05, 0.5, 2.0, 50.0], n0), rng.choice([0.05, 0.5, 2.0, 50.0], n0)
    split = np.where(omz >= 1e-1, (i0 // 4) % 3, 0)  # tau per spin, the total split evenly, split 95 / 5
    cls = [1 if o <= 1e-8 else 0 for o in omz]

    def add(u, d, su_, sd_, g_, au_, ad_, c):
        nonlocal ru, rd, su, sd, geo, au, ad, split, cls
        ru, rd, su, sd, geo = np.append(ru, u), np.append(rd, d), np.append(su, su_), np.append(sd, sd_), np.append(geo, g_)
        au, ad, split, cls = np.append(au, au_), np.append(ad, ad_), np.append(split, 0), cls + [c]
    for u, s_, a in zip(10.0 ** rng.uniform(-3, 2, 4), (0.2, 1.0, 4.0, 20.0), (0.5, 2.0, 1e-9, 50.0)):
        add(u, 0.0, s_, 0.0, 3, a, 0.0, 2)
    one = []
    for u, s_ in ((1e-2, 0.3), (30.0, 5.0)):
        add(u, 0.0, s_, 0.0, 3, 0.0, 0.0, 3)
        one.append(ru.shape[0] - 1)
    seam_c = []
    for k in range(2):
        for d in (1e-13, 1e-6, 1e-2):
            for sg in (1.0, -1.0):
                add(0.325, 0.175, 0.8, 0.6, 0, 1.0 - sg * d, 0.5, 4)
                if k:
                    seam_c.append((ru.shape[0] - 1, 1.0 - sg * d))
    for a in (0.5, 1.0, 2.0):
        add(0.26, 0.14, 0.0, 0.0, 0, a, a, 6 if a == 1.0 else 5)
    add(0.6e-15, 0.3e-15, 0.4, 0.4, 0, 0.5, 0.5, 7)
    add(0.2e-15, 0.2e-15, 0.4, 0.4, 2, 0.5, 0.5, 7)
    n = ru.shape[0]
    # per spin: x_s = |grad rho_s| / rho_s^(4/3) = s / X2S
    gu = _short(su / X2S * ru ** (4.0 / 3))
    gd = _short(np.where(geo == 3, 0.0, sd / X2S * rd ** (4.0 / 3)))
    grho_u = gu * _axis(np.zeros(n, dtype=int), n)
    grho_d = np.where(geo == 1, -1.0, 1.0) * gd * _axis(np.where(geo == 2, 1, 0), n)
    tw_u, tw_d = gu * gu / (8.0 * np.maximum(ru, 1e-300)), gd * gd / (8.0 * np.maximum(rd, 1e-300))
    tau_u = tw_u + au * 0.5 * TAU_UNIF * (2.0 * ru) ** (5.0 / 3)
    tau_d = tw_d + ad * 0.5 * TAU_UNIF * (2.0 * rd) ** (5.0 / 3)
    tot = tau_u + tau_d
    tau_u = np.where(split == 1, 0.5 * tot, np.where(split == 2, 0.95 * tot, tau_u))
    tau_d = np.where(split == 1, 0.5 * tot, np.where(split == 2, 0.05 * tot, tau_d))
    for i in one:
        tau_u[i] = tw_u[i] * (1.0 + 1e-12)
    for i, a in seam_c:  # the alpha of the total density: (tau - tau_W) / (tau_unif ds(zeta))
        r, z = ru[i] + rd[i], (ru[i] - rd[i]) / (ru[i] + rd[i])
        ds = 0.5 * ((1.0 + z) ** (5.0 / 3) + (1.0 - z) ** (5.0 / 3))
        t = ((grho_u[:, i] + grho_d[:, i]) ** 2).sum() / (8.0 * r) + a * TAU_UNIF * r ** (5.0 / 3) * ds
        tau_u[i] = tau_d[i] = 0.5 * t
    tau_d[rd == 0.0] = 0.0
    return {"rho_u": ru, "rho_d": rd, "grho_u": grho_u, "grho_d": grho_d, "tau_u": tau_u, "tau_d": tau_d, "cls": np.array(cls)}


def mgga_unpol_point(p, i):
    g = p["grho"][:, i]
    return xe.effective_point_unpol(p["rho"][i], _sig(g, g), p["tau"][i])


def mgga_pol_point(p, i):
    gu, gd = p["grho_u"][:, i], p["grho_d"][:, i]
    return xe.effective_point(p["rho_u"][i], p["rho_d"][i], _sig(gu, gu), _sig(gu, gd), _sig(gd, gd), p["tau_u"][i], p["tau_d"][i])


# LDA / GGA functionals whose first-order truth at the same points the fixtures hold as well (rows of tau: zero): the term lists of
# the tests mix them with the meta-GGAs
MGGA_EXTRA = {"mgga_unpol": ["gga_x_b88", "gga_x_pw91", "lda_c_pz"], "mgga_pol": ["gga_c_pbe"]}


def _lda_gga_point(kind, p, i):
    if kind == "mgga_unpol":
        g = p["grho"][:, i]
        return xe.effective_point_unpol(p["rho"][i], _sig(g, g))
    gu, gd = p["grho_u"][:, i], p["grho_d"][:, i]
    return xe.effective_point(p["rho_u"][i], p["rho_d"][i], _sig(gu, gu), _sig(gu, gd), _sig(gd, gd))


def mgga_row(kind, name, p, i):
    """(2, 4) [(2, 8)] truth and scale at point i of an unpolarised [polarised] meta-GGA point set (zeros below the density cutoff)"""
    nv = 3 if kind == "mgga_unpol" else 7
    out = np.zeros((2, 1 + nv))
    if name in xe.FUNCS:
        pt, nv = _lda_gga_point(kind, p, i), nv - (1 if kind == "mgga_unpol" else 2)
    else:
        pt = (mgga_unpol_point if kind == "mgga_unpol" else mgga_pol_point)(p, i)
    if pt is None:
        return out
    r = xe.mp_eval(name, list(pt[0]), pt[1], dps=pt[2], zero=pt[3])
    out[:, 0] = r["e"]
    for k in range(nv):
        out[:, 1 + k] = r["d1"][k]
    return out


def mgga_double_rows(kind, name, p):
    """the torch-double backend at every point, in the rows of `<name>_val`"""
    n = p["cls"].shape[0]
    nv = 3 if kind == "mgga_unpol" else 7
    out = np.zeros((1 + nv, n))
    if name in xe.FUNCS:
        pts = [_lda_gga_point(kind, p, i) for i in range(n)]
    else:
        pts = [(mgga_unpol_point if kind == "mgga_unpol" else mgga_pol_point)(p, i) for i in range(n)]
    live = [i for i in range(n) if pts[i] is not None]
    x = np.array([[float(v) for v in pts[i][0]] for i in live]).T
    off = np.array([[float(v) for v in np.atleast_1d(pts[i][1])] for i in live]).T
    e, d1, _ = xe.td_eval(name, x, off if name in xe.MGGA_FUNCS else off[0])
    out[0, live], out[1:1 + d1.shape[0], live] = e, d1
    return out


def mgga_compose(kind, rows, p, absolute=False):
    if kind == "mgga_unpol":
        return xe.compose_unpol(rows, p["grho"], None, absolute)
    return xe.compose_pol(rows, p["grho_u"], p["grho_d"], None, None, absolute)


def mgga_excluded(kind, name, p):
    if name in xe.FUNCS:  # first order of an LDA / GGA functional: the empty spin only
        m = mgga_excluded(kind, "mgga_c_scan", p)
        return dict(m, vtau_d=m["vrho_d"]) if kind == "mgga_pol" else m
    return (xe.unpol_excluded if kind == "mgga_unpol" else xe.pol_excluded)(name, p)


def mgga_double_err(kind, name, p, val):
    """(point class, output class) the largest scaled error of the outputs composed from the torch-double backend"""
    got = mgga_compose(kind, mgga_double_rows(kind, name, p), p)
    truth, scale = mgga_compose(kind, val[0], p), mgga_compose(kind, val[1], p, absolute=True)
    exc = mgga_excluded(kind, name, p)
    err = np.zeros((len(MGGA_CLASSES[kind]), 2))
    for c in range(err.shape[0]):
        for o in got:
            k = xe.output_class(o)
            err[c, k] = max(err[c, k], xe.scaled_error(got[o], truth[o], scale[o], exc[o] | (p["cls"] != c)))
    return err


def mgga_excluded_share(kind, p):
    masks = [m for name in MGGA_NAMES for m in mgga_excluded(kind, name, p).values()]
    return sum(int(m.sum()) for m in masks) / sum(m.size for m in masks)


def load_mgga_points():
    if "mgga_unpol" not in _POINTS:
        _POINTS["mgga_unpol"], _POINTS["mgga_pol"] = mgga_unpol_points(), mgga_pol_points()
    return _POINTS


def _mgga_job(job):
    kind, name, i = job
    return kind, name, i, mgga_row(kind, name, _POINTS[kind], i)


def make_mgga(nproc):
    import multiprocessing as mproc
    pts = load_mgga_points()
    names = {k: MGGA_NAMES + MGGA_EXTRA[k] for k in MGGA_CLASSES}
    jobs = [(k, n, i) for k in MGGA_CLASSES for n in names[k] for i in range(pts[k]["cls"].shape[0])]
    val = {(k, n): np.zeros((2, 4 if k == "mgga_unpol" else 8, pts[k]["cls"].shape[0])) for k in MGGA_CLASSES for n in names[k]}
    with mproc.Pool(nproc) as pool:
        for k, n, i, row in pool.imap_unordered(_mgga_job, jobs, chunksize=4):
            val[(k, n)][:, :, i] = row
    for kind in MGGA_CLASSES:
        p = pts[kind]
        out = {"_how": np.array(MGGA_DOC), "names": np.array(MGGA_NAMES), "extra": np.array(MGGA_EXTRA[kind]), "classes": np.array(MGGA_CLASSES[kind]),
               "h_rel": np.array(xe.H_REL), "dps": np.array(xe.DPS)}
        out.update({"p_" + k: v for k, v in p.items()})
        share = mgga_excluded_share(kind, p)
        out["excluded_share"] = np.array(share)
        print("%s: %d points, excluded share %.2f %%" % (kind, p["cls"].shape[0], 100.0 * share))
        print("%-12s %-15s %9s %9s" % ("functional", "class", "e", "first"))
        for n in names[kind]:
            out[n + "_val"] = val[(kind, n)]
            out[n + "_double_err"] = err = mgga_double_err(kind, n, p, val[(kind, n)])
            for c, cn in enumerate(MGGA_CLASSES[kind]):
                print("%-12s %-15s %9.1e %9.1e" % (n, cn, err[c, 0], err[c, 1]), flush=True)
        path = os.path.join(GOLDEN, "xc_exact_%s.npz" % kind)
        np.savez_compressed(path, **out)
        print("%s: %d bytes" % (path, os.path.getsize(path)))
        assert os.path.getsize(path) <= 532000 and share <= 0.02


# ------------------------------------------------------------------------------------------------
if __name__ == "__main__":
    import multiprocessing as mproc
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    what = sys.argv[2] if len(sys.argv) > 2 else "all"  # "lda_gga", "mgga" or "all"
    if what in ("mgga", "all"):
        make_mgga(nproc)
    if what == "mgga":
        sys.exit(0)
    pts = load_points()
    size = {"unpol": pts["unpol"]["rho"].shape[0], "pol": pts["pol"]["rho_u"].shape[0],
            "old_unpol": pts["old_unpol"]["rho"].shape[0], "old_pol": pts["old_pol"]["rho_u"].shape[0]}
    rows = {"unpol": 10, "pol": 11, "old_unpol": 10, "old_pol": 11}
    val = {(k, n): np.zeros((2, rows[k], size[k])) for k in size for n in NAMES}
    jobs = [(k, n, i) for k in size for n in NAMES for i in range(size[k])]
    with mproc.Pool(nproc) as pool:
        for done, (k, n, i, row) in enumerate(pool.imap_unordered(_job, jobs, chunksize=16)):
            val[(k, n)][:, :, i] = row
            if done % 5000 == 0:
                print("%d / %d" % (done, len(jobs)), flush=True)
    for kind in ("unpol", "pol"):
        p = pts[kind]
        out = {"_how": np.array(__doc__), "names": np.array(NAMES), "h_rel": np.array(xe.H_REL), "dps": np.array(xe.DPS)}
        out.update({"p_" + k: v for k, v in p.items()})
        share = excluded_share(kind, p)
        out["excluded_share"] = np.array(share)
        print("%s: %d points, excluded share %.2f %%" % (kind, size[kind], 100.0 * share))
        for n in NAMES:
            out[n + "_val"] = val[(kind, n)]
            out[n + "_double_err"] = double_err(kind, n, p, val[(kind, n)])
            o = val[("old_" + kind, n)][0]
            out["old_" + n] = o[[2, 3, 4]] if kind == "unpol" else o[[3, 4, 5, 6, 7, 8, 9, 10]]
            print("%-14s double_err  e %.1e  first %.1e  second %.1e" % ((n,) + tuple(out[n + "_double_err"])), flush=True)
        path = os.path.join(GOLDEN, "xc_exact_%s.npz" % kind)
        np.savez_compressed(path, **out)
        print("%s: %d bytes" % (path, os.path.getsize(path)))
        assert os.path.getsize(path) <= 1011830 and share <= 0.02
