"""Pointwise fixture for the THIRD-order functional kernel of dqc_amd/csrc/xc.hip (dqc_xc_eval_kxc, restricted closed shell), from the
reference of oracle/xc_exact.py: tests/golden/xc_kxc_exact_unpol.npz.

Points: the unpolarised point set of tools/make_xc_exact_golden.py (`unpol_points`: rho 1e-14 .. 1e4, s 1e-6 .. 100, grad rho = 0, both
sides of the PZ81 branch, of the x asinh x switch and of the density cutoff; `cls` labels them) with its response as the FIRST
direction (d rho_1, grad d rho_1) and a second, independent one from the same recipe (`_response`, its own seed).

With a = (d rho_1, d sigma_1), b = (d rho_2, d sigma_2), d sigma_k = 2 grad rho . grad d rho_k (formed in double, as the kernel forms
them, and taken as given), per functional and point the file holds the truth and the SCALE (sum of the absolute values of the same
derivative of the additive parts, oracle/xc_exact.py) of the rows

    0, 1   T_rho, T_sigma = d/d(rho, sigma) of the second directional derivative (a . grad)(b . grad) e
    2, 3   (H a)_sigma, (H b)_sigma = e_rs d rho_k + e_ss d sigma_k
    4, 5   e_rs, e_ss

as `<name>_val[0]` and `<name>_val[1]`.  The outputs of the kernel are composed from them (`compose_kxc`), with d2 sigma = 2 grad d rho_1 .
grad d rho_2:

    d2vrho  = T_rho + e_rs d2 sigma
    d2vgrad = 2 (T_sigma + e_ss d2 sigma) grad rho + 2 (H a)_sigma grad d rho_2 + 2 (H b)_sigma grad d rho_1

and their scales from the same formulas with absolute values.  Truth: mpmath central differences of every additive part of
ALL_FUNCS[name] -- a third mixed difference over x +- h e_k +- t a +- t b for rows 0, 1 (relative step H_REL = 1e-20: it loses 60 digits,
so at least 120 are carried, more where the variables differ by orders of magnitude: `third_dps`), xc_exact.mp_eval for the others.
`step_agreement` (per functional): the largest |truth(1e-20) - truth(1e-15)| / scale over the points CHECK_IDX -- the adequacy of the
step.  `<name>_double_err` (2, 6): the largest scaled error of (d2vrho, d2vgrad) composed from torch float64 TRIPLE autograd on the same
formula, per point class; points where that backend is not finite are left out of it and counted in `<name>_double_nonfinite`.  The
tolerance of tests/test_gpu_xc_kxc.py is max(1e-11, 10 x double_err).

Excluded from the comparison: gga_x_g96 where grad rho is exactly zero (its v_sigma does not exist there; both outputs: d2vrho holds
(d v_sigma / d rho) d2 sigma, and d2 sigma does not vanish with grad rho); nothing else.

Imports oracle.xc_exact and tools/make_xc_exact_golden.py only, never dqc_amd.      usage: python tools/make_xc_kxc_golden.py [processes]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402
import make_xc_exact_golden as g1  # noqa: E402
from oracle import xc_exact as xe  # noqa: E402

NAMES = xe.NAMES
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUTPUTS = ("d2vrho", "d2vgrad")
NROW, NCLS = 6, 6
H_REL, H_CHECK = 1e-20, 1e-15
FLOOR = 1e-11


def kxc_points():
    """the closed-shell points of the first- and second-order fixture with a second response direction"""
    p = dict(g1.unpol_points())
    rng = np.random.default_rng(20261031)
    p["drho2"], p["dgrho2"] = g1._response(rng, p["rho"], p["grho"])
    return p


CHECK_IDX = tuple(range(0, g1.NBULK, 4)) + tuple(range(g1.NBULK, g1.NBULK + 20))  # every fourth bulk point, every special point


def directions(p, i):
    """a, b in (rho, sigma) and d2 sigma at point i, in double"""
    g, a, b = p["grho"][:, i], p["dgrho"][:, i], p["dgrho2"][:, i]
    return [p["drho"][i], 2.0 * g1._sig(g, a)], [p["drho2"][i], 2.0 * g1._sig(g, b)], 2.0 * g1._sig(a, b)


def third_dps(dps2):
    """digits for the third difference: xc_exact._work_dps sizes a SECOND difference (50 + 30 + twice the decimal exponents of the
    ratios of the variables); a third one with steps of 1e-20 loses 60 digits and resolves the ratios to the third power"""
    return xe.DPS + 70 + (3 * (dps2 - xe.DPS - 30) + 1) // 2


def third_rows(name, x, dz, a, b, dps, zero=(), h_rel=H_REL):
    """[(truth, scale) of d/dx_k (a . grad)(b . grad) e for k = rho, sigma]: the mixed central difference of every part, as mpf"""
    ns = xe.MP(dps)
    f = xe.ALL_FUNCS[name]

    def parts(y):
        return [xe._re(v) for v in f(ns, *xe.unpolarised(*y), dz)]

    st = [abs(v) for v in x]
    a, b = [mp.mpf(float(v)) for v in a], [mp.mpf(float(v)) for v in b]
    e_scale = mp.fsum(abs(v) for v in parts(x))
    t = mp.mpf(h_rel)
    out = []
    for k in range(2):
        h = t * st[k]
        acc = None
        for sk in (1, -1):
            for sa in (1, -1):
                for sb in (1, -1):
                    y = [x[j] + sa * t * a[j] + sb * t * b[j] for j in range(2)]
                    y[k] = y[k] + sk * h
                    vals = parts(y)
                    acc = [sk * sa * sb * v for v in vals] if acc is None else [u + sk * sa * sb * v for u, v in zip(acc, vals)]
        vals = [v / (8 * h * t * t) for v in acc]
        # the scale floors of xc_exact.mp_eval, one more direction
        lo = mp.mpf(xe.TINY_S ** 3 if k in zero else xe.SCALE_FLOOR) * e_scale / st[k]
        lo = lo * max(abs(u) / c for u, c in zip(a, st)) * max(abs(u) / c for u, c in zip(b, st))
        out.append((mp.fsum(vals), max(mp.fsum(abs(v) for v in vals), lo)))
    return out


def kxc_row(name, p, i, h_rel=H_REL):
    """(2, NROW) truth and scale at point i (zeros below the density cutoff)"""
    out = np.zeros((2, NROW))
    g = p["grho"][:, i]
    pt = xe.effective_point_unpol(p["rho"][i], g1._sig(g, g))
    if pt is None:
        return out
    x, dz, dps, zero = pt
    a, b, _ = directions(p, i)
    # the differences step by h_rel TIMES the direction: a direction is first scaled (by a power of two: exactly) so that no variable
    # moves by more than h_rel of itself -- grad d rho may be orders of magnitude above grad rho at small s
    xf = [float(v) for v in x]
    sa, sb = (2.0 ** np.ceil(np.log2(max(1.0, abs(d[0]) / xf[0], abs(d[1]) / xf[1]))) for d in (a, b))
    a, b = [v / sa for v in a], [v / sb for v in b]
    t3 = third_rows(name, x, dz, a, b, third_dps(dps), zero, h_rel)
    for k in range(2):
        out[:, k] = [float(v * sa * sb) for v in t3[k]]
    for col, d, s in ((2, a, sa), (3, b, sb), (4, [xf[0], 0.0], 1.0 / xf[0]), (5, [0.0, xf[1]], 1.0 / xf[1])):
        r = xe.mp_eval(name, x, dz, delta=d, h_rel=h_rel, variables=(1,), dps=dps, zero=zero, number=mp.mpf)["d2"][1]
        out[:, col] = [float(v * s) for v in r]
    return out


def compose_kxc(rows, p, absolute=False):
    """the outputs of dqc_xc_eval_kxc from the rows (NROW, n) of the fixture; absolute=True: the scales of the outputs from the scales"""
    g, a, b = p["grho"], p["dgrho"], p["dgrho2"]
    dds = 2.0 * (a * b).sum(0)
    if absolute:
        g, a, b, dds = np.abs(g), np.abs(a), np.abs(b), np.abs(dds)
    return {"d2vrho": rows[0] + rows[4] * dds, "d2vgrad": 2.0 * (rows[1] + rows[5] * dds) * g + 2.0 * rows[2] * b + 2.0 * rows[3] * a}


def excluded(name, p):
    """{output: mask} of what a comparison leaves out: gga_x_g96 where grad rho is exactly zero, BOTH outputs -- v_sigma ~ sigma^(-1/4)
    does not exist there, and at this order it enters d2vrho as well, through e_rs d2 sigma = (d v_sigma / d rho) 2 grad d rho_1 . grad d rho_2,
    which does not vanish with grad rho"""
    m = {o: np.zeros(p["rho"].shape[0], dtype=bool) for o in OUTPUTS}
    if name == "gga_x_g96":
        m["d2vgrad"] = (np.abs(p["grho"]).sum(0) == 0.0) & (p["rho"] > xe.DENS_THRESHOLD)
        m["d2vrho"] = m["d2vgrad"].copy()
    return m


def double_rows(name, p):
    """the rows from torch float64 triple autograd on the same formula (zeros below the cutoff)"""
    import torch
    n = p["rho"].shape[0]
    out = np.zeros((NROW, n))
    live, xs, dzs, as_, bs = [], [], [], [], []
    for i in range(n):
        g = p["grho"][:, i]
        pt = xe.effective_point_unpol(p["rho"][i], g1._sig(g, g))
        if pt is None:
            continue
        a, b, _ = directions(p, i)
        live.append(i)
        xs.append([float(v) for v in pt[0]])
        dzs.append(float(pt[1]))
        as_.append(a)
        bs.append(b)
    x = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in np.array(xs).T]
    a, b = torch.tensor(np.array(as_).T), torch.tensor(np.array(bs).T)
    parts = xe.ALL_FUNCS[name](xe.TD(), *xe.unpolarised(*x), torch.tensor(dzs))
    e = sum(parts[1:], parts[0])

    def grad(y):
        if not y.requires_grad:
            return [torch.zeros_like(x[0]), torch.zeros_like(x[0])]
        r = torch.autograd.grad(y.sum(), x, create_graph=True, allow_unused=True)
        return [torch.zeros_like(x[0]) if v is None else v for v in r]

    g = grad(e)
    ha, hb = grad(g[0] * a[0] + g[1] * a[1]), grad(g[0] * b[0] + g[1] * b[1])
    t3 = grad(ha[0] * b[0] + ha[1] * b[1])
    hs = grad(g[1])  # e_sr, e_ss
    for r, v in enumerate((t3[0], t3[1], ha[1], hb[1], hs[0], hs[1])):
        out[r, live] = v.detach().numpy()
    return out


def class_errors(name, p, val, got_rows):
    """(2, NCLS) the largest scaled error of the outputs composed from `got_rows` per output and point class, and the number of
    points left out because got_rows is not finite there"""
    got = compose_kxc(got_rows, p)
    truth, scale, exc = compose_kxc(val[0], p), compose_kxc(val[1], p, absolute=True), excluded(name, p)
    err, bad = np.zeros((2, NCLS)), 0
    for j, o in enumerate(OUTPUTS):
        finite = np.isfinite(got[o]).reshape(-1, got[o].shape[-1]).all(0)
        bad += int((~finite & ~exc[o]).sum())
        for c in range(NCLS):
            mask = exc[o] | ~finite | (p["cls"] != c)
            err[j, c] = xe.scaled_error(np.where(finite, got[o], 0.0), truth[o], scale[o], mask)
    return err, bad


def step_agreement(p, val, chk, idx):
    """the largest |output(step 1) - output(step 2)| / scale of the composed outputs over the points idx (a row that is exactly zero,
    like the e_ss of gga_c_lyp, holds the round-off of the difference over a scale at its floor: the OUTPUTS are what is compared)"""
    sub = {k: v[..., idx] for k, v in p.items()}
    a, b, s = compose_kxc(val[0][:, idx], sub), compose_kxc(chk[0][:, idx], sub), compose_kxc(val[1][:, idx], sub, absolute=True)
    return max(xe.scaled_error(b[o], a[o], s[o]) for o in OUTPUTS)


_P = {}


def _job(job):
    name, i, h_rel = job
    if not _P:
        _P.update(kxc_points())
    return name, i, h_rel, kxc_row(name, _P, i, h_rel)


if __name__ == "__main__":
    import multiprocessing as mproc
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    p = kxc_points()
    n = p["rho"].shape[0]
    assert n == g1.NBULK + 20
    val = {nm: np.zeros((2, NROW, n)) for nm in NAMES}
    chk = {nm: np.zeros((2, NROW, n)) for nm in NAMES}
    jobs = [(nm, i, H_REL) for nm in NAMES for i in range(n)] + [(nm, i, H_CHECK) for nm in NAMES for i in CHECK_IDX]
    with mproc.Pool(nproc) as pool:
        for done, (nm, i, h_rel, row) in enumerate(pool.imap_unordered(_job, jobs, chunksize=8)):
            (val if h_rel == H_REL else chk)[nm][:, :, i] = row
            if done % 1000 == 0:
                print("%d / %d" % (done, len(jobs)), flush=True)
    out = {"_how": np.array(__doc__), "names": np.array(NAMES), "h_rel": np.array(H_REL), "h_check": np.array(H_CHECK),
           "check_idx": np.array(CHECK_IDX)}
    out.update({"p_" + k: v for k, v in p.items()})
    nexc = 0
    for nm in NAMES:
        out[nm + "_val"] = val[nm]
        agree = step_agreement(p, val[nm], chk[nm], list(CHECK_IDX))
        out[nm + "_step_agreement"] = np.array(agree)
        err, bad = class_errors(nm, p, val[nm], double_rows(nm, p))
        out[nm + "_double_err"], out[nm + "_double_nonfinite"] = err, np.array(bad)
        nexc += int(sum(m.sum() for m in excluded(nm, p).values()))
        print("%-14s step agreement %.1e   torch-double: d2vrho %.1e  d2vgrad %.1e  (worst class; %d points not finite)"
              % (nm, agree, err[0].max(), err[1].max(), bad), flush=True)
    out["n_excluded"] = np.array(nexc)
    path = os.path.join(GOLDEN, "xc_kxc_exact_unpol.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, %d (functional, point, output) triples excluded" % (path, os.path.getsize(path), nexc))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, "xc_exact_unpol.npz"))
