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


# ------------------------------------------------------------------------------------------------
if __name__ == "__main__":
    import multiprocessing as mproc
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
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
