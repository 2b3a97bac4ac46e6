"""Pointwise fixture for the second-order functional kernels (dqc_xc_eval_fxc, dqc_xc_eval_fxc_pol): for every LDA / GGA functional
of the kernel set, restricted and spin-polarised, the response of the oracle's FIRST-order potentials to a change of the density,

    d v_rho = d/dt v_rho[rho + t d rho, grad rho + t grad d rho],     d v_grad = d/dt v_grad[...]   at t = 0,

at seeded points (rho, grad rho, d rho, grad d rho).  v_grad is what the Hamiltonian integrates: 2 v_sigma grad rho, and
2 v_uu grad rho_u + v_ud grad rho_d per spin (oracle/xc.py: XC.get_vxc, compute_pol).

The oracle's closed forms are numpy (hand-derived first derivatives and numpy dual arrays), not torch: they cannot be
differentiated by autograd, so the derivative in t is a central difference with two steps (h, h / 2) and Richardson extrapolation,
(4 D(h/2) - D(h)) / 3.  Per functional the file records `fd_error` = max |Richardson - D(h/2)| relative to the largest value of
that output: the test's tolerance is derived from it.  The last NLOW points lie below the density cutoff (1e-15): every output is
exactly zero there.

Imports `oracle` only, never dqc_amd.  Writes tests/golden/oracle_fxc_pointwise.npz.      usage: python tools/make_fxc_golden.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oracle import xc as ox  # noqa: E402

NAMES = ["lda_x", "lda_c_pw", "lda_c_pw_mod", "lda_c_vwn", "lda_c_pz", "gga_x_pbe", "gga_x_pbe_r", "gga_x_pbe_sol", "gga_x_rpbe",
         "gga_c_pbe", "gga_c_pbe_sol", "gga_x_b88", "gga_c_lyp", "gga_c_p86", "gga_x_pw91", "gga_x_b86", "gga_x_g96", "gga_x_pw86",
         "gga_x_optx", "gga_x_wc"]
NPT, NLOW, H = 200, 8, 2e-3


def points(seed, rho=None):
    """rho (n,), grad rho (3, n), d rho (n,), grad d rho (3, n): densities log-uniform in [1e-4, 10], reduced gradients s in
    [0, 2.5], responses up to 30 % of the ground state; the last NLOW points below the cutoff"""
    rng = np.random.default_rng(seed)
    rho = 10.0 ** rng.uniform(-4, 1, NPT) if rho is None else rho.copy()
    s = rng.uniform(0.0, 2.5, NPT)
    gnorm = s * 2.0 * (3.0 * np.pi ** 2) ** (1.0 / 3) * rho ** (4.0 / 3)
    u = rng.normal(size=(3, NPT))
    grho = gnorm * u / np.linalg.norm(u, axis=0)
    drho = rho * rng.uniform(-0.3, 0.3, NPT)
    dgrho = gnorm.clip(min=1e-3 * rho) * rng.uniform(-0.3, 0.3, (3, NPT))
    rho[-NLOW:] = 10.0 ** rng.uniform(-19, -15.5, NLOW)
    drho[-NLOW:] = 0.1 * rho[-NLOW:]
    return rho, grho, drho, dgrho


def richardson(f, h):
    d1 = [(a - b) / (2 * h) for a, b in zip(f(h), f(-h))]
    d2 = [(a - b) / h for a, b in zip(f(h / 2), f(-h / 2))]
    return [(4 * b - a) / 3 for a, b in zip(d1, d2)], d2


def restricted(name, rho, grho, drho, dgrho):
    fam, fn = ox._FUNCS[name]

    def pot(t):
        r, g = rho + t * drho, grho + t * dgrho
        _, vr, vs = fn(r, (g * g).sum(0))
        return [vr, 2.0 * vs[None] * g if fam == 2 else np.zeros_like(g)]
    return richardson(pot, H)


def polarised(name, ru, rd, gu, gd, dru, drd, dgu, dgd):
    fam = ox._FUNCS[name][0]
    xc = ox.XC([(1.0, name)])

    def pot(t):
        a, b, ga, gb = ru + t * dru, rd + t * drd, gu + t * dgu, gd + t * dgd
        _, (vu, vd), (vgu, vgd), _ = ox.compute_pol(xc, a, b, ga if fam == 2 else None, gb if fam == 2 else None)
        z = np.zeros_like(ga)
        return [vu, vd, vgu if fam == 2 else z, vgd if fam == 2 else z]
    return richardson(pot, H)


def err(rich, half):
    return max(float(np.abs(r - h2).max() / max(np.abs(r).max(), 1e-300)) for r, h2 in zip(rich, half))


if __name__ == "__main__":
    out = {"_how": np.array(__doc__), "names": np.array(NAMES), "nlow": np.array(NLOW), "h": np.array(H)}
    rho, grho, drho, dgrho = points(20260901)
    out.update(r_rho=rho, r_grho=grho, r_drho=drho, r_dgrho=dgrho)
    zeta = np.random.default_rng(20260904).uniform(-0.8, 0.8, NPT)
    rho0 = points(20260905)[0]
    pu, pd = points(20260902, 0.5 * (1 + zeta) * rho0), points(20260903, 0.5 * (1 - zeta) * rho0)
    for k, a in zip(("rho", "grho", "drho", "dgrho"), pu):
        out["p_" + k + "_u"] = a
    for k, a in zip(("rho", "grho", "drho", "dgrho"), pd):
        out["p_" + k + "_d"] = a
    for name in NAMES:
        rich, half = restricted(name, rho, grho, drho, dgrho)
        out[name + "_dvrho"], out[name + "_dvgrad"] = rich
        out[name + "_fd_error"] = np.array(err(rich, half))
        assert all(np.all(r[..., -NLOW:] == 0.0) for r in rich), name
        richp, halfp = polarised(name, pu[0], pd[0], pu[1], pd[1], pu[2], pd[2], pu[3], pd[3])
        for k, a in zip(("dvrho_u", "dvrho_d", "dvgrad_u", "dvgrad_d"), richp):
            out[name + "_pol_" + k] = a
        out[name + "_pol_fd_error"] = np.array(err(richp, halfp))
        assert all(np.all(r[..., -NLOW:] == 0.0) for r in richp), name
        print("%-14s fd_error %.2e   polarised %.2e" % (name, out[name + "_fd_error"], out[name + "_pol_fd_error"]), flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "oracle_fxc_pointwise.npz"), **out)
