"""The 50-digit functional reference (oracle/xc_exact.py) and its fixtures (tools/make_xc_exact_golden.py): published values, the
fixtures are the tool's output, the torch-double yardstick recorded in them, oracle/xc.py pointwise against the truth, and the tie
to the finite-difference fixture the Hessian tests have trusted (tests/golden/oracle_fxc_pointwise.npz).  The second half does the
same for the four meta-GGAs (value and first order; fixtures xc_exact_mgga_unpol.npz, xc_exact_mgga_pol.npz), with limits that do not
come from this code base's codings in place of the Hessian fixture."""
import importlib.util
import json
import os

import mpmath as mp
import numpy as np
import pytest

from oracle import xc_exact as xe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = (1e-13, 1e-13, 1e-12)  # of tests/test_gpu_xc_exact.py


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("make_xc_exact_golden", os.path.join(ROOT, "tools", "make_xc_exact_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.load_points()
    return m


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return {k: np.load(os.path.join(golden_dir, "xc_exact_%s.npz" % k)) for k in ("unpol", "pol")}


def test_reference_stands_alone():
    src = open(os.path.join(ROOT, "oracle", "xc_exact.py")).read()
    imports = [ln.strip() for ln in src.splitlines() if ln.strip().startswith(("import ", "from "))]
    assert imports and not [ln for ln in imports if "dqc_amd" in ln or "oracle" in ln], imports
    assert sorted(xe.FUNCS) == sorted(xe.NAMES) and len(xe.NAMES) == 20


def _e_mp(name, ru, rd, suu, sud, sdd):
    pt = xe.effective_point(ru, rd, suu, sud, sdd)
    if pt is None:  # below the density cutoff
        return mp.mpf(0)
    x, dz, dps, _ = pt
    ns = xe.MP(dps)
    return mp.fsum(xe.FUNCS[name](ns, *x, dz))


def test_truth_reproduces_the_published_values(golden_dir):
    """tests/golden/functional_points.json within each entry's own tolerance: hydrogen-atom energies by radial Gauss-Legendre
    quadrature of the exact density n_up = exp(-2r) / pi, n_down = 0, and Ceperley-Alder correlation energies of the uniform gas"""
    pts = json.load(open(os.path.join(golden_dir, "functional_points.json")))
    x, w = np.polynomial.legendre.leggauss(160)
    r, w = 0.5 * (x + 1.0) * 30.0, 0.5 * 30.0 * w
    seen = 0
    for row in pts["h_atom"]:
        if row["xc"] not in xe.FUNCS:
            continue  # the meta-GGAs have tests of their own
        seen += 1
        e = 0.0
        for ri, wi in zip(r, w):
            ra = float(np.exp(-2.0 * ri) / np.pi)
            e += 4.0 * np.pi * ri * ri * wi * float(_e_mp(row["xc"], ra, 0.0, 4.0 * ra * ra, 0.0, 0.0))
        assert abs(e - row["value"]) < row["tol"], (row["xc"], e, row["value"])
    assert seen == 10
    for row in pts["uniform_gas"]:
        for name in row["xcs"]:
            if name not in xe.FUNCS:
                continue
            n = 3.0 / (4.0 * np.pi * row["rs"] ** 3)
            ru, rd = 0.5 * n * (1 + row["zeta"]), max(0.5 * n * (1 - row["zeta"]), n * 1e-14)
            eps = float(_e_mp(name, ru, rd, 0.0, 0.0, 0.0)) / n
            assert abs(eps - row["value"]) < row["rtol"] * abs(row["value"]), (name, row["rs"], row["zeta"], eps, row["value"])


def test_halving_the_step_changes_nothing_at_1e_20(tool):
    """the central differences of the truth: relative step 1e-13 against 0.5e-13, in units of the scale, on bulk, zero-gradient,
    seam and nearly fully polarised points"""
    pu, pp = tool._POINTS["unpol"], tool._POINTS["pol"]
    worst = 0.0
    for name in ("gga_c_pbe", "gga_x_b88", "gga_c_lyp", "gga_c_p86", "gga_x_rpbe", "lda_c_vwn"):
        for i in (0, 7, 100, 257, 263, 274):
            g, dg = pu["grho"][:, i], pu["dgrho"][:, i]
            x, dz, dps, zero = xe.effective_point_unpol(pu["rho"][i], tool._sig(g, g))
            d = [pu["drho"][i], 2.0 * tool._sig(g, dg)]
            a = xe.mp_eval(name, x, dz, d, dps=dps, number=mp.mpf, zero=zero)
            b = xe.mp_eval(name, x, dz, d, dps=dps, number=mp.mpf, zero=zero, h_rel=0.5 * xe.H_REL)
            worst = max([worst] + [float(abs(a[k][j][0] - b[k][j][0]) / a[k][j][1]) for k in ("d1", "d2") for j in a[k]])
        for i in (1, 60, 75, 129):
            x, d = tool.pol_inputs(pp, i)
            x, dz, dps, zero = xe.effective_point(*x)
            a = xe.mp_eval(name, list(x), dz, d, dps=dps, number=mp.mpf, zero=zero)
            b = xe.mp_eval(name, list(x), dz, d, dps=dps, number=mp.mpf, zero=zero, h_rel=0.5 * xe.H_REL)
            worst = max([worst] + [float(abs(a[k][j][0] - b[k][j][0]) / a[k][j][1]) for k in ("d1", "d2") for j in a[k]])
    print("largest change on halving the step: %.1e of the scale" % worst)
    assert worst < 1e-20


def test_fixtures_are_the_tools_output(tool, fixtures):
    """every 16th point of both fixtures (and of the rows at the old fixture's points), regenerated: the stored numbers to 1e-15"""
    def same(a, b):
        return np.all(np.abs(a - b) <= 1e-15 * np.abs(b))
    for kind, row, old_rows in (("unpol", tool.unpol_row, [2, 3, 4]), ("pol", tool.pol_row, [3, 4, 5, 6, 7, 8, 9, 10])):
        fx, p = fixtures[kind], tool._POINTS[kind]
        for k, v in p.items():
            assert np.array_equal(fx["p_" + k], v), k
        n = p["cls"].shape[0]
        assert list(fx["names"]) == xe.NAMES
        for name in xe.NAMES:
            for i in range(0, n, 16):
                assert same(row(name, p, i), fx[name + "_val"][:, :, i]), (kind, name, i)
            q = tool._POINTS["old_" + kind]
            for i in range(0, 200, 16):
                assert same(row(name, q, i)[0][old_rows], fx["old_" + name][:, i]), (kind, name, i)
    assert int((tool._POINTS["unpol"]["cls"] == 0).sum()) >= 256 and int((tool._POINTS["pol"]["cls"] == 0).sum()) >= 128


def test_excluded_share(tool, fixtures):
    for kind in ("unpol", "pol"):
        share = tool.excluded_share(kind, tool._POINTS[kind])
        print("%s: %.2f %% of the (functional, point, output) triples are left out" % (kind, 100.0 * share))
        assert share == float(fixtures[kind]["excluded_share"]) and share <= 0.02


def test_double_yardstick_is_the_recorded_one(tool, fixtures):
    """the torch-double backend against the truth: the largest scaled error per functional and output class, recomputed, agrees with
    the fixture's `double_err` within a factor of 2 (figures below a tenth of the floor do not enter a tolerance: compared there)"""
    for kind in ("unpol", "pol"):
        for name in xe.NAMES:
            got = tool.double_err(kind, name, tool._POINTS[kind], fixtures[kind][name + "_val"])
            rec = fixtures[kind][name + "_double_err"]
            print("%-6s %-14s recorded %s  recomputed %s" % (kind, name, " ".join("%.1e" % v for v in rec), " ".join("%.1e" % v for v in got)))
            for c in range(3):
                a, b = max(got[c], 0.1 * FLOOR[c]), max(rec[c], 0.1 * FLOOR[c])
                assert 0.5 <= a / b <= 2.0, (kind, name, c, got[c], rec[c])


def test_oracle_first_order_against_the_truth(tool, fixtures):
    """oracle/xc.py (numpy double, hand-derived and dual-array derivatives) pointwise, polarised and closed shell, within the
    tolerance of the GPU tests: max(1e-13, 10 x double_err)"""
    from oracle import xc as ox
    bad = []
    pu, pp = tool._POINTS["unpol"], tool._POINTS["pol"]
    for name in xe.NAMES:
        fam, fn = ox._FUNCS[name]
        e, vr, vs = fn(pu["rho"], (pu["grho"] ** 2).sum(0))
        got = {"e": e, "vrho": vr, "vgrad": 2.0 * vs[None] * pu["grho"] if fam == 2 else None}
        xc = ox.XC([(1.0, name)])
        gg = fam == 2
        ep, (vu, vd), (gu, gd), _ = ox.compute_pol(xc, pp["rho_u"], pp["rho_d"], pp["grho_u"] if gg else None, pp["grho_d"] if gg else None)
        gotp = {"e": ep, "vrho_u": vu, "vrho_d": vd, "vgrad_u": gu, "vgrad_d": gd}
        for kind, g, p, exc in (("unpol", got, pu, xe.unpol_excluded(name, pu)), ("pol", gotp, pp, xe.pol_excluded(name, pp))):
            v = fixtures[kind][name + "_val"]
            truth, scale = tool.compose(kind, v[0], p), tool.compose(kind, v[1], p, absolute=True)
            for o, a in g.items():
                if a is None:
                    continue
                c = xe.output_class(o)
                tol = max(FLOOR[c], 10.0 * float(fixtures[kind][name + "_double_err"][c]))
                err = xe.scaled_error(a, truth[o], scale[o], exc[o])
                print("%-6s %-14s %-8s %.1e (tolerance %.1e)" % (kind, name, o, err, tol))
                if not err < tol:
                    bad.append((kind, name, o, err, tol))
    assert not bad, bad


def test_truth_agrees_with_the_finite_difference_fixture(tool, fixtures, golden_dir):
    """the truth at the points of oracle_fxc_pointwise.npz against its Richardson-extrapolated differences of the oracle's
    potentials, in that fixture's own measure (largest deviation over the largest value) within 10 x its own `fd_error`"""
    old = np.load(os.path.join(golden_dir, "oracle_fxc_pointwise.npz"))
    r, q = tool._POINTS["old_unpol"], tool._POINTS["old_pol"]

    def rel(a, b):
        return float(np.abs(a - b).max() / np.abs(b).max())
    for name in xe.NAMES:
        gga = xe.IS_GGA[name]
        vs, hr, hs = fixtures["unpol"]["old_" + name]
        tol = 10.0 * float(old[name + "_fd_error"])
        assert rel(hr, old[name + "_dvrho"]) < tol, name
        if gga:
            assert rel(2.0 * hs * r["grho"] + 2.0 * vs * r["dgrho"], old[name + "_dvgrad"]) < tol, name
        v = np.zeros((11, 200))
        v[3:] = fixtures["pol"]["old_" + name]
        out = xe.compose_pol(v, q["grho_u"], q["grho_d"], q["dgrho_u"], q["dgrho_d"])
        tol = 10.0 * float(old[name + "_pol_fd_error"])
        for o in ("dvrho_u", "dvrho_d") + (("dvgrad_u", "dvgrad_d") if gga else ()):
            assert rel(out[o], old[name + "_pol_" + o]) < tol, (name, o)


# ------------------------------------------------------------------------------------------------ the meta-GGA functionals
MGGA_KINDS = ("mgga_unpol", "mgga_pol")


@pytest.fixture(scope="module")
def mtool(tool):
    tool.load_mgga_points()
    return tool


@pytest.fixture(scope="module")
def mfixtures(golden_dir):
    return {k: np.load(os.path.join(golden_dir, "xc_exact_%s.npz" % k)) for k in MGGA_KINDS}


def test_mgga_reference_is_registered_beside_the_first_twenty():
    assert xe.MGGA_NAMES == ["mgga_x_scan", "mgga_c_scan", "mgga_x_tpss", "mgga_c_tpss"] and sorted(xe.MGGA_FUNCS) == sorted(xe.MGGA_NAMES)
    assert not set(xe.MGGA_NAMES) & set(xe.NAMES) and sorted(xe.ALL_FUNCS) == sorted(xe.NAMES + xe.MGGA_NAMES)


def _mp_parts(name, rho, zeta, s, alpha=None, z=None, dps=60):
    """the parts of a meta-GGA at a point given by (rho, zeta, s, alpha or z = tau_W / tau) of the TOTAL density with parallel spin
    gradients in proportion to the densities and tau_s in proportion to rho_s^(5/3) ... / the densities; in mpmath, no thresholds"""
    ns = xe.MP(dps)
    rho, zeta, s = mp.mpf(rho), mp.mpf(zeta), mp.mpf(s)
    ru, rd = rho * (1 + zeta) / 2, rho * (1 - zeta) / 2
    kf2 = mp.power(3 * mp.pi ** 2 * rho, mp.mpf(2) / 3)
    sig = 4 * s * s * kf2 * rho * rho
    fu, fd = ru / rho, rd / rho
    tw = sig / (8 * rho)
    ds = (mp.power(1 + zeta, mp.mpf(5) / 3) + mp.power(1 - zeta, mp.mpf(5) / 3)) / 2
    tau = tw / mp.mpf(z) if z is not None else tw + mp.mpf(alpha) * mp.mpf(0.3) * kf2 * rho * ds
    return ns, xe.ALL_FUNCS[name](ns, ru, rd, sig * fu * fu, sig * fu * fd, sig * fd * fd, tau * fu, tau * fd), rho


def test_mgga_truth_against_limits_from_outside_this_code_base():
    """the exact constraints the papers build the functionals on, at 60 digits and without thresholds (the reference's constants
    are the doubles the kernels hold: 0.3, 1.174, 4.9479 here as well)"""
    tiny = mp.mpf(10) ** -30
    for rho in ("0.003", "0.7", "40"):
        ns, lda, _ = _mp_parts("mgga_x_scan", rho, 0, tiny, alpha=1 + tiny)
        r = mp.mpf(rho)
        ex = -mp.mpf(3) / 4 * mp.cbrt(3 / mp.pi) * r * mp.cbrt(r)   # the uniform gas: F_x = 1
        for name in ("mgga_x_scan", "mgga_x_tpss"):
            e = mp.fsum(_mp_parts(name, rho, 0, tiny, alpha=1 + tiny)[1])
            assert abs(e / ex - 1) < mp.mpf(10) ** -25, (name, rho)
        # SCAN exchange at alpha = 0: F_x = h0 g(s) at every s, -> h0 = 1.174 as s -> 0
        for s in ("1e-8", "1e-3", "0.5"):
            e = mp.fsum(_mp_parts("mgga_x_scan", rho, 0, s, alpha=0)[1])
            g = 1 - mp.exp(-mp.mpf(4.9479) / mp.sqrt(mp.mpf(s)))
            assert abs(e / (ex * mp.mpf(1.174) * g) - 1) < mp.mpf(10) ** -40, (rho, s)
        assert abs(mp.fsum(_mp_parts("mgga_x_scan", rho, 0, "1e-8", alpha=0)[1]) / ex - mp.mpf(1.174)) < mp.mpf(10) ** -40
        for zeta in (0, "0.4", "-0.9"):
            ru, rd = r * (1 + mp.mpf(zeta)) / 2, r * (1 - mp.mpf(zeta)) / 2
            # SCAN correlation at sigma = 0, alpha = 1: the LSDA it is built on
            ns, parts, _ = _mp_parts("mgga_c_scan", rho, zeta, tiny, alpha=1 + tiny)
            ref = mp.fsum(xe.lda_c_pw_mod(ns, ru, rd, 0, 0, 0))
            assert abs(mp.fsum(parts) / ref - 1) < mp.mpf(10) ** -25, (rho, zeta)
            # TPSS correlation as tau -> infinity (z -> 0): PBE
            for s in ("0.01", "0.8", "6"):
                ns, parts, _ = _mp_parts("mgga_c_tpss", rho, zeta, s, z=mp.mpf(10) ** -40)
                kf2 = mp.power(3 * mp.pi ** 2 * r, mp.mpf(2) / 3)
                sig = 4 * mp.mpf(s) ** 2 * kf2 * r * r
                fu, fd = ru / r, rd / r
                ref = mp.fsum(xe.gga_c_pbe(ns, ru, rd, sig * fu * fu, sig * fu * fd, sig * fd * fd))
                assert abs(mp.fsum(parts) / ref - 1) < mp.mpf(10) ** -40, (rho, zeta, s)
        # no correlation for a one-electron density: fully polarised (rho_d -> 0), tau = tau_W
        for name in ("mgga_c_scan", "mgga_c_tpss"):
            for s in ("0.2", "1.5"):
                _, parts, _ = _mp_parts(name, rho, 1 - mp.mpf(10) ** -40, s, z=1)
                assert abs(mp.fsum(parts)) < mp.mpf(10) ** -20 * mp.fsum(abs(v) for v in parts), (name, rho, s)


def test_mgga_exchange_truth_is_spin_scaled():
    """E_x[rho_u, rho_d] = (E_x[2 rho_u] + E_x[2 rho_d]) / 2 with the closed-shell form on the right, part by part"""
    ns = xe.MP(60)
    ru, rd, suu, sdd, tu, td = (mp.mpf(v) for v in ("0.31", "0.07", "0.4", "0.002", "0.9", "0.05"))
    for name in ("mgga_x_scan", "mgga_x_tpss"):
        f = xe.ALL_FUNCS[name]
        pol = f(ns, ru, rd, suu, mp.mpf("-0.01"), sdd, tu, td)
        one = [f(ns, *xe.unpolarised(2 * r, 4 * s, 2 * t)) for r, s, t in ((ru, suu, tu), (rd, sdd, td))]
        k = len(pol) // 2
        for j in range(k):
            assert abs(pol[j] - (one[0][j] + one[0][k + j]) / 2) < mp.mpf(10) ** -50 * abs(pol[j])
            assert abs(pol[k + j] - (one[1][j] + one[1][k + j]) / 2) < mp.mpf(10) ** -50 * abs(pol[k + j])


def _e_mp_mgga(name, ru, rd, suu, sud, sdd, tu, td):
    pt = xe.effective_point(ru, rd, suu, sud, sdd, tu, td)
    if pt is None:
        return mp.mpf(0)
    x, off, dps, _ = pt
    return mp.fsum(xe.ALL_FUNCS[name](xe.MP(dps), *x, off))


def test_mgga_truth_reproduces_the_published_values(golden_dir):
    """the meta-GGA rows of tests/golden/functional_points.json (the values tests/test_gpu_parity.py holds the kernels to): the
    hydrogen atom (tau = tau_W of one orbital) and the uniform gas (sigma = 0, tau = tau_unif), at libxc's thresholds"""
    pts = json.load(open(os.path.join(golden_dir, "functional_points.json")))
    x, w = np.polynomial.legendre.leggauss(160)
    r, w = 0.5 * (x + 1.0) * 30.0, 0.5 * 30.0 * w
    seen = 0
    for row in pts["h_atom"]:
        if row["xc"] not in xe.MGGA_FUNCS:
            continue
        seen += 1
        e = 0.0
        for ri, wi in zip(r, w):
            ra = float(np.exp(-2.0 * ri) / np.pi)
            sg = 4.0 * ra * ra
            e += 4.0 * np.pi * ri * ri * wi * float(_e_mp_mgga(row["xc"], ra, 0.0, sg, 0.0, 0.0, sg / (8.0 * ra), 0.0))
        assert abs(e - row["value"]) < row["tol"], (row["xc"], e, row["value"])
    assert seen == 4
    for row in pts["uniform_gas"]:
        for name in row["xcs"]:
            if name not in xe.MGGA_FUNCS:
                continue
            seen += 1
            n = 3.0 / (4.0 * np.pi * row["rs"] ** 3)
            tau = 0.3 * (3.0 * np.pi ** 2) ** (2.0 / 3) * n ** (5.0 / 3)
            eps = float(_e_mp_mgga(name, 0.5 * n, 0.5 * n, 0.0, 0.0, 0.0, 0.5 * tau, 0.5 * tau)) / n
            assert abs(eps - row["value"]) < row["rtol"] * abs(row["value"]), (name, eps, row["value"])
    assert seen == 6


def test_halving_the_step_changes_nothing_at_1e_20_mgga(mtool):
    """the central differences of the meta-GGA truth on bulk, zero-gradient, iso-orbital, tau-floor and polarised points, and on
    both sides of the alpha = 1 seam down to |1 - alpha| = 1e-14: both branches of the switch are flat to all orders there, so a
    step that straddled the seam would change nothing either"""
    pu, pp = mtool._POINTS["mgga_unpol"], mtool._POINTS["mgga_pol"]
    seam = [int(i) for i in np.nonzero(pu["cls"] == 1)[0][:8]] + [int(i) for i in np.nonzero(pu["cls"] == 1)[0][32:36]]
    pseam = [int(i) for i in np.nonzero(pp["cls"] == 4)[0]]
    worst = 0.0
    for name in xe.MGGA_NAMES:
        for kind, p, idx, point in (("mgga_unpol", pu, [0, 7, 100, 305, 312, 320, 328] + seam, mtool.mgga_unpol_point),
                                    ("mgga_pol", pp, [1, 3, 60, 121, 125] + pseam, mtool.mgga_pol_point)):
            for i in idx:
                x, off, dps, zero = point(p, i)
                a = xe.mp_eval(name, list(x), off, dps=dps, number=mp.mpf, zero=zero)
                b = xe.mp_eval(name, list(x), off, dps=dps, number=mp.mpf, zero=zero, h_rel=0.5 * xe.H_REL)
                worst = max([worst] + [float(abs(a["d1"][j][0] - b["d1"][j][0]) / a["d1"][j][1]) for j in a["d1"]])
    print("largest change on halving the step: %.1e of the scale" % worst)
    assert worst < 1e-20


def test_mgga_fixtures_are_the_tools_output(mtool, mfixtures):
    """every 8th point of both meta-GGA fixtures and every point outside the bulk block, regenerated: the stored numbers to 1e-15"""
    for kind in MGGA_KINDS:
        fx, p = mfixtures[kind], mtool._POINTS[kind]
        for k, v in p.items():
            assert np.array_equal(fx["p_" + k], v), k
        assert list(fx["names"]) == xe.MGGA_NAMES and list(fx["classes"]) == list(mtool.MGGA_CLASSES[kind])
        assert sorted(set(p["cls"].tolist())) == list(range(len(mtool.MGGA_CLASSES[kind])))
        n = p["cls"].shape[0]
        for name in xe.MGGA_NAMES:
            for i in [i for i in range(n) if i % 8 == 0 or p["cls"][i] != 0]:
                a, b = mtool.mgga_row(kind, name, p, i), fx[name + "_val"][:, :, i]
                assert np.all(np.abs(a - b) <= 1e-15 * np.abs(b)), (kind, name, i)
    assert np.all(mtool._POINTS["mgga_unpol"]["cls"][:256] == 0)  # one contiguous bulk block comes first


def test_mgga_excluded_share(mtool, mfixtures):
    for kind in MGGA_KINDS:
        share = mtool.mgga_excluded_share(kind, mtool._POINTS[kind])
        print("%s: %.2f %% of the (functional, point, output) triples are left out" % (kind, 100.0 * share))
        assert share == float(mfixtures[kind]["excluded_share"]) and share <= 0.02
    assert mtool.mgga_excluded_share("mgga_unpol", mtool._POINTS["mgga_unpol"]) == 0.0


def test_mgga_double_yardstick_is_the_recorded_one(mtool, mfixtures):
    """per point class and output class, recomputed: within a factor of 2 of the fixture's `double_err` (above a tenth of the floor)"""
    for kind in MGGA_KINDS:
        for name in xe.MGGA_NAMES:
            got = mtool.mgga_double_err(kind, name, mtool._POINTS[kind], mfixtures[kind][name + "_val"])
            rec = mfixtures[kind][name + "_double_err"]
            assert got.shape == rec.shape == (len(mtool.MGGA_CLASSES[kind]), 2)
            for c in range(rec.shape[0]):
                for k in range(2):
                    a, b = max(got[c, k], 0.1 * FLOOR[k]), max(rec[c, k], 0.1 * FLOOR[k])
                    assert 0.5 <= a / b <= 2.0, (kind, name, c, k, got[c, k], rec[c, k])


def mgga_class_errors(fx, p, name, got, compose, exc):
    """[(class, output, worst scaled error, tolerance = max(1e-13, 10 x double_err[class, output class]))] of the outputs `got`"""
    v = fx[name + "_val"]
    truth, scale = compose(v[0]), compose(v[1], True)
    rows = []
    for c, cn in enumerate(fx["classes"]):
        for o, a in got.items():
            k = xe.output_class(o)
            tol = max(FLOOR[k], 10.0 * float(fx[name + "_double_err"][c, k]))
            rows.append((str(cn), o, xe.scaled_error(a, truth[o], scale[o], exc[o] | (p["cls"] != c)), tol))
    return rows


def _oracle_mgga_outputs(name, pu, pp):
    """oracle/xc.py's closed-shell outputs, and its polarised ones (exchange by the spin-scaling relation, as dqc_amd/xc.py does)"""
    from oracle import xc as ox
    fn = ox._FUNCS_MGGA[name]
    e, vr, vs, vt = fn(pu["rho"], (pu["grho"] ** 2).sum(0), pu["tau"])
    unpol = {"e": e, "vrho": vr, "vgrad": 2.0 * vs[None] * pu["grho"], "vtau": vt}
    gu, gd = pp["grho_u"], pp["grho_d"]
    if name.startswith("mgga_x_"):
        ch = [fn(2.0 * pp["rho_" + s], 4.0 * (pp["grho_" + s] ** 2).sum(0), 2.0 * pp["tau_" + s]) for s in "ud"]
        pol = {"e": 0.5 * (ch[0][0] + ch[1][0]), "vrho_u": ch[0][1], "vrho_d": ch[1][1], "vgrad_u": 4.0 * ch[0][2][None] * gu,
               "vgrad_d": 4.0 * ch[1][2][None] * gd, "vtau_u": ch[0][3], "vtau_d": ch[1][3]}
        live = pp["rho_u"] + pp["rho_d"] > xe.DENS_THRESHOLD  # the cutoff is on the total density
        pol = {o: np.where(live, a, 0.0) for o, a in pol.items()}
    elif name == "mgga_c_scan":
        e, (vu, vd), vs, vt = ox.mgga_c_scan_pol(pp["rho_u"], pp["rho_d"], ((gu + gd) ** 2).sum(0), pp["tau_u"] + pp["tau_d"])
        pol = {"e": e, "vrho_u": vu, "vrho_d": vd, "vgrad_u": 2.0 * vs[None] * (gu + gd), "vgrad_d": 2.0 * vs[None] * (gu + gd), "vtau_u": vt, "vtau_d": vt}
    else:
        e, (vu, vd), (a, b, c), vt = ox.mgga_c_tpss_pol(pp["rho_u"], pp["rho_d"], (gu * gu).sum(0), (gu * gd).sum(0), (gd * gd).sum(0),
                                                       pp["tau_u"] + pp["tau_d"])
        pol = {"e": e, "vrho_u": vu, "vrho_d": vd, "vgrad_u": 2.0 * a[None] * gu + b[None] * gd, "vgrad_d": 2.0 * c[None] * gd + b[None] * gu,
               "vtau_u": vt, "vtau_d": vt}
    return unpol, pol


def test_oracle_mgga_first_order_against_the_truth(mtool, mfixtures):
    """oracle/xc.py's four meta-GGAs (numpy double, dual arrays) pointwise in the scaled measure, closed shell and polarised, per
    point class within max(1e-13, 10 x double_err)"""
    pu, pp = mtool._POINTS["mgga_unpol"], mtool._POINTS["mgga_pol"]
    bad = []
    for name in xe.MGGA_NAMES:
        unpol, pol = _oracle_mgga_outputs(name, pu, pp)
        for kind, got, p in (("mgga_unpol", unpol, pu), ("mgga_pol", pol, pp)):
            rows = mgga_class_errors(mfixtures[kind], p, name, got, lambda r, a=False: mtool.mgga_compose(kind, r, p, a),
                                     mtool.mgga_excluded(kind, name, p))
            for cn, o, err, tol in rows:
                print("%-10s %-12s %-15s %-8s %.1e (tolerance %.1e)" % (kind, name, cn, o, err, tol))
                if not err < tol:
                    bad.append((kind, name, cn, o, err, tol))
    assert not bad, bad
