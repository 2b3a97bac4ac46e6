"""The 50-digit functional reference (oracle/xc_exact.py) and its fixtures (tools/make_xc_exact_golden.py): published values, the
fixtures are the tool's output, the torch-double yardstick recorded in them, oracle/xc.py pointwise against the truth, and the tie
to the finite-difference fixture the Hessian tests have trusted (tests/golden/oracle_fxc_pointwise.npz)."""
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
