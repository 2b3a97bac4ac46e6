"""Orbital-Hessian products on the GPU: the second-order functional kernels (dqc_xc_eval_fxc, dqc_xc_eval_fxc_pol), the
Hessian-vector product of dqc_amd/response.py, SCF stability (lowest_eival_orb_hessian, is_orb_min) and the analytic polarizability.

Yardsticks: tests/golden/oracle_fxc_pointwise.npz (tools/make_fxc_golden.py: two-step central differences of the oracle's
first-order potentials, with their own error estimate) and tests/golden/oracle_orb_hessian.npz (tools/make_orb_hessian_golden.py:
dense Hessians from central differences of the oracle's Fock matrix, finite-field polarizabilities, each with its error estimate).
Tolerances: max(floor, 10 x the fixture's recorded error estimate) -- the factor 10 covers the estimate being an estimate; the
floors are 1e-10 (pointwise, relative to the largest value of the output) and 1e-9 (the standing Fock-matrix bar of the parity suite)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TIGHT = {"f_tol": 1e-11, "maxiter": 300}
NAMES = ["lda_x", "lda_c_pw", "lda_c_pw_mod", "lda_c_vwn", "lda_c_pz", "gga_x_pbe", "gga_x_pbe_r", "gga_x_pbe_sol", "gga_x_rpbe",
         "gga_c_pbe", "gga_c_pbe_sol", "gga_x_b88", "gga_c_lyp", "gga_c_p86", "gga_x_pw91", "gga_x_b86", "gga_x_g96", "gga_x_pw86",
         "gga_x_optx", "gga_x_wc"]
CASES = ["h2o_rhf", "h2o_lda", "h2o_pbe", "h2o_blyp", "h2o_pbe0", "ch3_uhf", "ch3_upbe", "h2_14_uhf", "h2_14_ulda", "h2_40_uhf", "h2_40_ulda"]
STABLE = [c for c in CASES if not c.startswith("h2_40")]
DAVIDSON_TOL = 1e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "oracle_fxc_pointwise.npz"))


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_orb_hessian.npz"))
    return g, json.loads(str(g["meta"]))


def _cu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _check_output(what, got, ref, tol, nlow):
    got = got.cpu().numpy()
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max() / scale
    print("%-28s max|d| / max|ref| %.2e  (tolerance %.2e, max|ref| %.2e)" % (what, err, tol, scale))
    assert got.shape == ref.shape
    assert np.all(got[..., -nlow:] == 0.0), what + ": points below the density cutoff must be exactly zero"
    assert err < tol, what


# ------------------------------------------------------------------------------------------------ 1. pointwise kernels
def test_fixture_lists_every_lda_and_gga_functional_of_the_kernel_set(fx):
    from dqc_amd.xc import _FAMILY
    assert sorted(NAMES) == sorted(n for n, f in _FAMILY.items() if f in (1, 2))
    assert sorted(str(n) for n in fx["names"]) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_fxc_kernel_matches_the_differenced_oracle(dev, fx, name):
    from dqc_amd import lib
    gga, nlow = name.startswith("gga_"), int(fx["nlow"])
    tol = max(1e-10, 10.0 * float(fx[name + "_fd_error"]))
    rho, grho, drho, dgrho = (_cu(fx["r_" + k]) for k in ("rho", "grho", "drho", "dgrho"))
    dv, dvg = lib.xc_eval_fxc([(1.0, name)], rho, grho if gga else None, drho[None], dgrho[None] if gga else None)
    _check_output(name + " dvrho", dv[0], fx[name + "_dvrho"], tol, nlow)
    if gga:
        _check_output(name + " dvgrad", dvg[0], fx[name + "_dvgrad"], tol, nlow)
    else:
        assert dvg is None and not np.any(fx[name + "_dvgrad"])
    # a block of trial vectors: the response is linear, every vector of the block is handled like a single one
    blk = torch.stack([drho, -2.0 * drho, 0.5 * drho])
    gblk = torch.stack([dgrho, -2.0 * dgrho, 0.5 * dgrho]) if gga else None
    bv, bg = lib.xc_eval_fxc([(1.0, name)], rho, grho if gga else None, blk, gblk)
    assert torch.equal(bv[0], dv[0])
    assert float((bv[1] + 2.0 * dv[0]).abs().max()) <= 1e-13 * float(dv[0].abs().max())
    if gga:
        assert torch.equal(bg[0], dvg[0])
        assert float((bg[2] - 0.5 * dvg[0]).abs().max()) <= 1e-13 * float(dvg[0].abs().max())


@pytest.mark.parametrize("name", NAMES)
def test_fxc_pol_kernel_matches_the_differenced_oracle(dev, fx, name):
    from dqc_amd import lib
    gga, nlow = name.startswith("gga_"), int(fx["nlow"])
    tol = max(1e-10, 10.0 * float(fx[name + "_pol_fd_error"]))
    a = {k + s: _cu(fx["p_%s_%s" % (k, s)]) for k in ("rho", "grho", "drho", "dgrho") for s in "ud"}
    g = (lambda t: t) if gga else (lambda t: None)
    (dvu, dvd), (dgu, dgd) = lib.xc_eval_fxc_pol([(1.0, name)], a["rhou"], a["rhod"], g(a["grhou"]), g(a["grhod"]), a["drhou"][None],
                                                 a["drhod"][None], g(a["dgrhou"][None]), g(a["dgrhod"][None]))
    _check_output(name + " pol dvrho_u", dvu[0], fx[name + "_pol_dvrho_u"], tol, nlow)
    _check_output(name + " pol dvrho_d", dvd[0], fx[name + "_pol_dvrho_d"], tol, nlow)
    if gga:
        _check_output(name + " pol dvgrad_u", dgu[0], fx[name + "_pol_dvgrad_u"], tol, nlow)
        _check_output(name + " pol dvgrad_d", dgd[0], fx[name + "_pol_dvgrad_d"], tol, nlow)
    else:
        assert dgu is None and dgd is None


def test_fxc_term_list_is_the_weighted_sum_and_closed_shell_limit(dev, fx):
    """(coef, id) lists: the weighted sum of the single terms; and the polarised kernel at rho_u = rho_d = rho / 2 with the response
    split evenly gives both spins the restricted kernel's response"""
    from dqc_amd import lib
    rho, grho, drho, dgrho = (_cu(fx["r_" + k]) for k in ("rho", "grho", "drho", "dgrho"))
    terms = [(0.08, "lda_x"), (0.72, "gga_x_b88"), (0.19, "lda_c_vwn"), (0.81, "gga_c_lyp")]
    dv, dvg = lib.xc_eval_fxc(terms, rho, grho, drho[None], dgrho[None])
    sv, sg = 0.0, 0.0
    for c, n in terms:
        v1, g1 = lib.xc_eval_fxc([(1.0, n)], rho, grho, drho[None], dgrho[None])
        sv = sv + c * v1
        sg = sg + c * g1
    assert float((dv - sv).abs().max()) <= 1e-12 * float(sv.abs().max())
    assert float((dvg - sg).abs().max()) <= 1e-12 * float(sg.abs().max())
    h = 0.5
    (pu, pd), (gu, gd) = lib.xc_eval_fxc_pol(terms, h * rho, h * rho, h * grho, h * grho, h * drho[None], h * drho[None], h * dgrho[None],
                                             h * dgrho[None])
    for got, ref in ((pu, dv), (pd, dv), (gu, dvg), (gd, dvg)):
        assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())


def test_fxc_refuses_meta_gga_by_name(dev, fx):
    from dqc_amd import lib
    rho, grho, drho, dgrho = (_cu(fx["r_" + k]) for k in ("rho", "grho", "drho", "dgrho"))
    with pytest.raises(NotImplementedError, match="mgga_x_scan"):
        lib.xc_eval_fxc([(1.0, "mgga_x_scan")], rho, grho, drho[None], dgrho[None])
    with pytest.raises(NotImplementedError, match="mgga_c_scan"):
        lib.xc_eval_fxc_pol([(1.0, "mgga_c_scan")], rho, rho, grho, grho, drho[None], drho[None], dgrho[None], dgrho[None])


# ------------------------------------------------------------------------------------------------ 2. - 4. the Hessian
_QC = {}


def _calc(case, gold):
    """the GPU calculation of a golden case, converged from the oracle's density (kept for the module)"""
    if case in _QC:
        return _QC[case]
    import dqc_amd
    from dqc_amd.utils.datastruct import SpinParam
    g, meta = gold
    m = meta[case]
    spin = m["spin"]
    mol = dqc_amd.Mol((m["atomzs"], m["atompos"]), basis=m["basis"], grid=m["grid"], **({"spin": spin} if spin else {}))
    kw = {} if spin is None else {"restricted": False}
    qc = dqc_amd.HF(mol, **kw) if m["xc"] is None else dqc_amd.KS(mol, xc=m["xc"], **kw)
    h = qc._engine.hamilton
    sx = h._ovlp_ao @ h._orthozer
    dms = [(sx.T @ _cu(g["%s_dm_ao_%d" % (case, s)]) @ sx).contiguous() for s in range(1 if spin is None else 2)]
    qc.run(dm0=dms[0] if spin is None else SpinParam(u=dms[0], d=dms[1]), fwd_options=TIGHT)
    assert qc.accepted
    _QC[case] = qc
    return qc


def _oracle_hessian(case, gold):
    from dqc_amd.response import OrbitalHessian
    g, meta = gold
    qc = _calc(case, gold)
    orbs = [(g["%s_c_ao_%d" % (case, s)], g["%s_eps_%d" % (case, s)]) for s in range(1 if meta[case]["spin"] is None else 2)]
    return OrbitalHessian(qc, orbitals=orbs if len(orbs) == 2 else orbs[0])


@pytest.mark.parametrize("case", CASES)
def test_hessian_vector_product_matches_golden(dev, gold, case):
    g, meta = gold
    H = _oracle_hessian(case, gold)
    assert H.n == meta[case]["n"]
    tol = max(1e-9, 10.0 * float(g[case + "_fd_error"]))
    got = H.mm(_cu(g[case + "_kappa"])[None])[0].cpu().numpy()
    err = np.abs(got - g[case + "_hkappa"]).max()
    print("%-12s max|H kappa - golden| %.2e  (tolerance %.2e, max|H kappa| %.2e)" % (case, err, tol, np.abs(got).max()))
    assert err < tol
    rng = np.random.default_rng(5)
    blk = rng.normal(size=(4, H.n))
    blk = _cu(blk / np.linalg.norm(blk, axis=1, keepdims=True))  # unit vectors: the bounds below are absolute
    hb = H.mm(blk)
    singles = torch.cat([H.mm(blk[i:i + 1]) for i in range(4)])
    assert float((hb - singles).abs().max()) < 1e-12
    x, y = blk[0], blk[1]
    assert abs(float(x @ hb[1]) - float(y @ hb[0])) < 1e-10


@pytest.mark.parametrize("case", CASES)
def test_lowest_eigenvalue_and_stability(dev, gold, case):
    import dqc_amd
    g, meta = gold
    qc = _calc(case, gold)
    tol = max(1e-9, 10.0 * float(g[case + "_fd_error"])) + DAVIDSON_TOL
    ev = dqc_amd.lowest_eival_orb_hessian(qc, tol=DAVIDSON_TOL)
    assert ev.shape == (1,)
    err = abs(float(ev[0]) - float(g[case + "_eig3"][0]))
    print("%-12s lowest eigenvalue %.10f  golden %.10f  |d| %.2e  (tolerance %.2e)" % (case, float(ev[0]), float(g[case + "_eig3"][0]), err, tol))
    assert err < tol
    assert dqc_amd.lowest_eival_orb_hessian(qc, tol=DAVIDSON_TOL) is ev  # memoised on the calculation
    assert dqc_amd.is_orb_min(qc) == meta[case]["stable"]


@pytest.mark.parametrize("case", STABLE)
def test_polarizability_matches_oracle_finite_field(dev, gold, case):
    import dqc_amd
    g, meta = gold
    qc = _calc(case, gold)
    alpha = dqc_amd.polarizability(qc).cpu().numpy()
    tol = 10.0 * float(g[case + "_alpha_error"])
    err = np.abs(alpha - g[case + "_alpha"]).max()
    print("%-12s max|alpha - finite field| %.2e  (tolerance %.2e)\n%s" % (case, err, tol, alpha))
    assert alpha.shape == (3, 3) and err < tol
    assert np.abs(alpha - alpha.T).max() < 1e-7


@pytest.mark.parametrize("case", ["h2o_rhf", "h2o_pbe", "ch3_upbe"])
def test_polarizability_matches_the_finite_field_routine(dev, gold, case):
    """against properties._polarizability (central differences of the dipole in a field, left as it was).  Its error at the step s is
    c s^2 + O(s^4): the values at s = 2e-3 and s / 2 differ by 3/4 c s^2, three times the error c s^2 / 4 of the one at s / 2 that
    is compared -- the bound, with nothing added."""
    import dqc_amd
    from dqc_amd.properties import _polarizability
    qc = _calc(case, gold)
    alpha = dqc_amd.polarizability(qc).cpu().numpy()
    a1, a2 = _polarizability(qc, 2e-3).numpy(), _polarizability(qc, 1e-3).numpy()
    bound = np.abs(a1 - a2).max()
    err = np.abs(alpha - a2).max()
    print("%-12s max|alpha - finite field(1e-3)| %.2e  (bound %.2e)" % (case, err, bound))
    assert err < bound


def test_results_follow_the_state_when_the_calculation_is_run_again(dev, gold):
    """the stability workflow: the symmetric H2 solution at 4 Bohr is a saddle point; run() of the SAME object from a density with the
    two electrons on different atoms finds the broken-symmetry minimum, and every memoised result is that state's, not the first's"""
    import dqc_amd
    from dqc_amd.response import orbital_hessian
    from dqc_amd.utils.datastruct import SpinParam
    g, meta = gold
    m = meta["h2_40_uhf"]
    qc = dqc_amd.HF(dqc_amd.Mol((m["atomzs"], m["atompos"]), basis=m["basis"]), restricted=False)
    h = qc._engine.hamilton
    sx = h._ovlp_ao @ h._orthozer
    sym = [(sx.T @ _cu(g["h2_40_uhf_dm_ao_%d" % s]) @ sx).contiguous() for s in range(2)]
    qc.run(dm0=SpinParam(u=sym[0], d=sym[1]), fwd_options=TIGHT)
    e_sym, ev_sym, op_sym = float(qc.energy()), dqc_amd.lowest_eival_orb_hessian(qc), orbital_hessian(qc)
    assert not dqc_amd.is_orb_min(qc) and abs(float(ev_sym[0]) - float(g["h2_40_uhf_eig3"][0])) < 1e-5
    left, right = np.zeros((4, 4)), np.zeros((4, 4))
    left[:2, :2], right[2:, 2:] = g["h2_40_uhf_dm_ao_0"][:2, :2], g["h2_40_uhf_dm_ao_0"][2:, 2:]  # (the AOs of atom 0, of atom 1)
    qc.run(dm0=SpinParam(u=(sx.T @ _cu(2.0 * left) @ sx).contiguous(), d=(sx.T @ _cu(2.0 * right) @ sx).contiguous()), fwd_options=TIGHT)
    assert qc.accepted
    e_min, ev_min = float(qc.energy()), dqc_amd.lowest_eival_orb_hessian(qc)
    print("symmetric: E %.8f lowest %.6f   broken symmetry: E %.8f lowest %.6f" % (e_sym, float(ev_sym[0]), e_min, float(ev_min[0])))
    assert e_min < e_sym - 1e-3  # the run did leave the saddle point
    assert ev_min is not ev_sym and float(ev_min[0]) > 0.0 and dqc_amd.is_orb_min(qc)
    assert orbital_hessian(qc) is not op_sym
    op = orbital_hessian(qc)
    x = torch.ones((1, op.n), dtype=torch.float64, device="cuda")
    assert float((op.mm(x) - op_sym.mm(x)).abs().max()) > 1e-3  # the operator is built on the new orbitals
    alpha = dqc_amd.polarizability(qc)
    assert dqc_amd.polarizability(qc) is alpha and float(alpha[2, 2]) > 0.0


# ------------------------------------------------------------------------------------------------ 5. what is refused
def test_unsupported_configurations_raise(dev):
    import dqc_amd
    from dqc_amd.response import OrbitalHessian
    from dqc_amd.utils.datastruct import SpinParam
    from tests import molecules as M
    qc = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid="sg2").densityfit(auxbasis="etb"), xc="lda_x").run()
    with pytest.raises(NotImplementedError, match="density fitting"):
        OrbitalHessian(qc)
    qc = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid="sg2"), xc="mgga_x_scan").run()
    with pytest.raises(NotImplementedError, match="mgga_x_scan"):
        dqc_amd.is_orb_min(qc)
    w = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.7, 0.3], dtype=torch.float64)
    qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G", orb_weights=SpinParam(u=w, d=w.clone()))).run()
    with pytest.raises(NotImplementedError, match="occupations"):
        dqc_amd.lowest_eival_orb_hessian(qc)
