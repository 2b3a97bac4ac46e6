"""TDDFT / TDA excited-state gradients end to end on the GPU: dqc_amd.tddft_gradient (dqc_amd/excited.py) on the third-order
exchange-correlation kernel dqc_xc_eval_kxc and the grid passes of dqc_amd/gradient.py.

The yardstick that fixes every factor: the Richardson-extrapolated central difference of KS(Mol(R +- h)).energy() +
excitations(...).energies[state], geometry, constants and step of tests/test_gpu_excited_gradient.py (H2O distorted, TIGHT SCF, tol = 1e-8,
ztol = 1e-9, six roots, h = 4e-3 Bohr: its docstring gives the reasoning), 3-21G on grid "sg2"; components (O, z), (H1, y), (H2, x).

Bound: |analytic - Richardson| <= 10 |FD(h) - FD(2h)| + eps, eps = max(1e-9, 10 n / (2 h)) with n = the difference of E + w between two
FRESH runs at the reference geometry, measured here per functional (the 1e-9 of the Hartree-Fock test comes from the noise of a
Hartree-Fock energy; a Kohn-Sham energy adds the grid sums).  Per case the gradient without the Z-vector and the gradient without the
third-order kernel each miss the bound (LDA: the miss without the kernel is printed, and asserted only if it is above the bound).
The relaxed dipole against the finite field has no grid motion: it isolates the Z-vector and V2 from the weight terms."""
import pytest
import torch

from tests import molecules as M
from tests.test_gpu_excited_gradient import COMPONENTS, DIRECTIONS, H, NST, POS, TIGHT, TOL, ZS, ZTOL

pytestmark = pytest.mark.gpu

GRID = "sg2"
CASES = {"lda-tda": ("lda_x+lda_c_pw", True), "pbe-full": ("gga_x_pbe+gga_c_pbe", False), "pbe0-tda": ("pbe0", True),
         "pbe0-full": ("pbe0", False), "b3lyp5-full": ("hyb_gga_xc_b3lyp5", False)}
HYBRID = {"pbe0", "hyb_gga_xc_b3lyp5"}
_RUNS, _NOISE = {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


def _make(xc, basis, atom=None, d=None, m=0, field=None):
    import dqc_amd
    if field is not None:
        kw = {}
        if field[1]:
            kw["efield"] = torch.tensor([field[1] * 1e-3 * x for x in DIRECTIONS[field[0]]], dtype=torch.float64)
        geom = M.H2O
    else:
        pos = [list(p) for p in POS]
        if m:
            pos[atom][d] += m * H
        geom, kw = (ZS, pos), {}
    if xc is None:
        qc = dqc_amd.HF(dqc_amd.Mol(geom, basis=basis, **kw))
    else:
        qc = dqc_amd.KS(dqc_amd.Mol(geom, basis=basis, grid=GRID, **kw), xc=xc)
    qc.run(fwd_options=TIGHT)
    assert qc.accepted
    return qc


def _run(xc, basis, atom=None, d=None, m=0, field=None):
    """the converged calculation of H2O at POS with coordinate (atom, d) moved by m * H Bohr, or of M.H2O in a field; cached per functional"""
    key = (xc, basis, atom, d, m, field)
    if key not in _RUNS:
        _RUNS[key] = _make(xc, basis, atom, d, m, field)
    return _RUNS[key]


def _roots(qc, tda, spin="singlet"):
    import dqc_amd
    return dqc_amd.excitations(qc, nstates=NST, spin=spin, tda=tda, tol=TOL)


def _pick_state(qc, tda, spin="singlet"):
    w = _roots(qc, tda, spin).energies.cpu().tolist()
    for k in range(NST - 1):
        if (k == 0 or w[k] - w[k - 1] > 1e-2) and w[k + 1] - w[k] > 1e-2:
            return k, w
    raise AssertionError("no root of %s is more than 1e-2 Ha from its neighbours" % (w,))


def _noise(xc, basis, tda, state):
    """n: |E + w| of two fresh runs at the reference geometry apart (measured once per functional, basis and problem)"""
    key = (xc, basis, tda, state)
    if key not in _NOISE:
        e = []
        for _ in range(2):
            q = _make(xc, basis)
            e.append(float(q.energy()) + float(_roots(q, tda).energies[state]))
        _NOISE[key] = abs(e[0] - e[1])
    return _NOISE[key]


def _fd(xc, basis, atom, d, energy):
    e = {m: energy(_run(xc, basis, atom, d, m)) for m in (1, -1, 2, -2)}
    f1, f2 = (e[1] - e[-1]) / (2 * H), (e[2] - e[-2]) / (4 * H)
    return f1, f2, (4.0 * f1 - f2) / 3.0


def _tsum(g):
    return float(g.sum(0).abs().max())


@pytest.mark.parametrize("case", sorted(CASES))
def test_tddft_gradient_against_finite_differences(dev, case):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.excited import _gradient
    xc, tda = CASES[case]
    qc = _run(xc, "3-21G")
    state, w = _pick_state(qc, tda)
    print("%s: roots %s, state %d" % (case, " ".join("%.6f" % x for x in w), state))
    kw = dict(state=state, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL)
    with lib.call_trace() as tr:
        g = dqc_amd.tddft_gradient(qc, **kw)
    names = [row[0] for row in tr.rows]
    assert names.count("dqc_eri_grad2") == (3 if xc in HYBRID else 2) and names.count("dqc_xc_eval_kxc") == 2
    assert dqc_amd.tddft_gradient(qc, **kw) is g
    assert isinstance(g, dqc_amd.ExcitedGradient) and tuple(g.gradient.shape) == (3, 3) and not g.gradient.requires_grad
    assert g.z_residual <= ZTOL and g.state == state and g.spin == "singlet" and g.tda == tda
    scf_now = qc.nuclear_gradient()
    assert float((g.scf - scf_now).abs().max()) <= 1e-12
    assert float(g.omega) == w[state] and abs(float(g.e_tot) - float(qc.energy()) - w[state]) <= 1e-12
    p = g.density.dm_mo
    assert float((p - p.t()).abs().max()) <= 1e-14 and abs(float(p.diagonal().sum())) <= 1e-12
    assert float(p[5:, :5].abs().max()) > 1e-3
    with torch.no_grad():
        noz = _gradient(qc, state, "singlet", tda, NST, TOL, ZTOL, with_z=False, who="tddft_gradient").gradient.cpu()
        nok = _gradient(qc, state, "singlet", tda, NST, TOL, ZTOL, with_kxc=False, who="tddft_gradient").gradient.cpu()
    n = _noise(xc, "3-21G", tda, state)
    eps = max(1e-9, 10.0 * n / (2.0 * H))
    print("%s: noise of E + w between two fresh runs %.2e Ha, eps %.2e" % (case, n, eps))
    grad, scf = g.gradient.cpu(), g.scf.cpu()
    energy = lambda q: float(q.energy()) + float(_roots(q, tda).energies[state])  # noqa: E731
    miss_k = 0
    for atom, k in COMPONENTS:
        f1, f2, fr = _fd(xc, "3-21G", atom, k, energy)
        bound = 10.0 * abs(f1 - f2) + eps
        diff = abs(fr - float(grad[atom, k]))
        print("(%d, %d)  %s: analytic % .10f  scf % .10f  without z % .10f  without kxc % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  "
              "|analytic - FD| %.2e  bound %.2e  |without z - FD| %.2e  |without kxc - FD| %.2e"
              % (atom, k, case, float(grad[atom, k]), float(scf[atom, k]), float(noz[atom, k]), float(nok[atom, k]), f1, f2, fr, diff, bound,
                 abs(float(noz[atom, k]) - fr), abs(float(nok[atom, k]) - fr)))
        assert diff <= bound
        assert abs(float(noz[atom, k]) - fr) > bound                        # the relaxation is not silently skipped
        miss_k += abs(float(nok[atom, k]) - fr) > bound
    print("%s: components that miss the bound without the third-order kernel: %d of %d" % (case, miss_k, len(COMPONENTS)))
    if not case.startswith("lda"):
        assert miss_k == len(COMPONENTS)                                    # the third-order kernel is not silently skipped
    t, t0 = _tsum(grad), _tsum(scf_now.cpu())
    print("%s translational invariance: |sum_A g_A| = %.2e (SCF gradient alone: %.2e)" % (case, t, t0))
    assert t <= 10.0 * t0 + 1e-10


H_FINE = 2.5e-4


@pytest.mark.parametrize("case", ["lda-tda", "pbe0-full"])
def test_tddft_gradient_against_a_finer_difference(dev, case):
    """A second, sharper look, on top of the comparison above.  A Kohn-Sham energy on the grid is rougher in R than a Hartree-Fock one: at
    h = 4e-3 Bohr |FD(h) - FD(2h)| is 1e-5 ... 2e-5 (Hartree-Fock: 2e-7 ... 5e-7) and the Richardson value is 3e-5 ... 9e-5 off the
    analytic gradient for the SCF part alone as for the whole (docs/LOG_r31.md, section 4), so the bound above is two orders wider than
    for Hartree-Fock.  At h = 2.5e-4 the same difference quotient of the same discretised functional agrees with the analytic gradient
    to 1e-8: component (O, z), bound 10 |FD(h) - FD(2h)| + max(1e-9, 10 n / (2 h)) with the measured noise n, as above"""
    import dqc_amd
    from dqc_amd.excited import _gradient
    xc, tda = CASES[case]
    qc = _run(xc, "3-21G")
    state, _ = _pick_state(qc, tda)
    g = dqc_amd.tddft_gradient(qc, state=state, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL).gradient
    with torch.no_grad():
        nok = _gradient(qc, state, "singlet", tda, NST, TOL, ZTOL, with_kxc=False, who="tddft_gradient").gradient

    def e_at(m):
        pos = [list(p) for p in POS]
        pos[0][2] += m * H_FINE
        q = dqc_amd.KS(dqc_amd.Mol((ZS, pos), basis="3-21G", grid=GRID), xc=xc)
        q.run(fwd_options=TIGHT)
        assert q.accepted
        return float(q.energy()) + float(_roots(q, tda).energies[state])

    e = {m: e_at(m) for m in (1, -1, 2, -2)}
    f1, f2 = (e[1] - e[-1]) / (2 * H_FINE), (e[2] - e[-2]) / (4 * H_FINE)
    fr = (4.0 * f1 - f2) / 3.0
    n = _noise(xc, "3-21G", tda, state)
    bound = 10.0 * abs(f1 - f2) + max(1e-9, 10.0 * n / (2.0 * H_FINE))
    print("(0, 2)  %s, h = %.1e: analytic % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  |analytic - FD| %.2e  bound %.2e  noise %.2e  "
          "|without kxc - FD| %.2e" % (case, H_FINE, float(g[0, 2]), f1, f2, fr, abs(fr - float(g[0, 2])), bound, n, abs(fr - float(nok[0, 2]))))
    assert abs(fr - float(g[0, 2])) <= bound
    assert abs(fr - float(nok[0, 2])) > bound


def test_tddft_gradient_d_shells(dev):
    """cc-pVDZ, pbe0 TDA, the component (H2, x): d shells in the grid passes and in the bilinear ERI pass"""
    import dqc_amd
    xc, tda = "pbe0", True
    qc = _run(xc, "cc-pvdz")
    state, w = _pick_state(qc, tda)
    g = dqc_amd.tddft_gradient(qc, state=state, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL)
    f1, f2, fr = _fd(xc, "cc-pvdz", 2, 0, lambda q: float(q.energy()) + float(_roots(q, tda).energies[state]))
    n = _noise(xc, "cc-pvdz", tda, state)
    bound = 10.0 * abs(f1 - f2) + max(1e-9, 10.0 * n / (2.0 * H))
    print("(2, 0)  pbe0 TDA / cc-pVDZ state %d: analytic % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  |analytic - FD| %.2e  "
          "bound %.2e  noise %.2e" % (state, float(g.gradient[2, 0]), f1, f2, fr, abs(fr - float(g.gradient[2, 0])), bound, n))
    assert abs(fr - float(g.gradient[2, 0])) <= bound


def _fd_dipole(xc, direction, energy):
    zs, pos = M.H2O
    ion = sum(z * sum(x * y for x, y in zip(p, DIRECTIONS[direction])) for z, p in zip(zs, pos))
    e = {m: energy(_run(xc, "3-21G", field=(direction, m))) for m in (1, -1, 2, -2)}
    f1, f2 = -(e[1] - e[-1]) / 2e-3 + ion, -(e[2] - e[-2]) / 4e-3 + ion
    return f1, f2, (4.0 * f1 - f2) / 3.0


@pytest.mark.parametrize("xc,tda", [("gga_x_pbe+gga_c_pbe", True), ("pbe0", False)], ids=["pbe-tda", "pbe0-full"])
def test_tddft_relaxed_dipole_against_finite_field(dev, xc, tda):
    """construction and bound of tests/test_gpu_excited_gradient.py::test_relaxed_dipole_against_finite_field"""
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.response import orbital_hessian
    qc = _run(xc, "3-21G", field=(None, 0))
    state, w = _pick_state(qc, tda)
    g = dqc_amd.tddft_gradient(qc, state=state, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL)
    mu = g.density.dipole(unit=None).cpu()
    h = qc._engine.hamilton
    sp = orbital_hessian(qc).spins[0]
    c = torch.cat([sp.co, sp.cv], dim=1)
    zbar = c @ (g.density.dm_mo - g.density.unrelaxed_mo) @ c.t()
    mu_u = (mu.to(h.device) + torch.einsum("dab,ba->d", lib.int1e("r0", h._tab, h.device), zbar)).cpu()
    along = lambda v, d: float(sum(x * y for x, y in zip(v.tolist(), DIRECTIONS[d])))  # noqa: E731
    for d in ("z", "yz"):
        f1, f2, fr = _fd_dipole(xc, d, lambda q: float(q.energy()) + float(_roots(q, tda).energies[state]))
        bound = 10.0 * abs(f1 - f2) + ZTOL
        print("%-2s  %s %s state %d: relaxed %.10f  unrelaxed %.10f  FD(h) %.10f  FD(2h) %.10f  Richardson %.10f  |relaxed - FD| %.2e  bound %.2e"
              % (d, xc, "TDA" if tda else "full", state, along(mu, d), along(mu_u, d), f1, f2, fr, abs(fr - along(mu, d)), bound))
        assert abs(fr - along(mu, d)) <= bound
        assert abs(along(mu_u, d) - fr) > bound


@pytest.mark.parametrize("xc,restricted", [pytest.param("lda_x+lda_c_pw", True, id="lda_x+lda_c_pw"),
                                           pytest.param("gga_x_pbe+gga_c_pbe", True, id="gga_x_pbe+gga_c_pbe"),
                                           pytest.param("mgga_x_scan", True, id="mgga_x_scan"),
                                           pytest.param("gga_x_pbe+gga_c_pbe", False, id="gga_x_pbe+gga_c_pbe-unrestricted")])
def test_xc_potential_gradient_reproduces_the_ground_state_terms(dev, xc, restricted):
    """Restricted LDA and PBE: _xc_potential_gradient with M = D and the ground-state potentials, plus _xc_weight_gradient on the energy
    density, is the XC part of nuclear_gradient (gradient._xc_gradient) to 1e-12: on the path it chooses (GGA: the fused kernel) and on
    the torch passes.  Both names now run the one gradient._xc_grid_terms, so this comparison is partly true by construction; what
    holds that function independently is (a) the two further cases here -- restricted SCAN (the tau terms) and unrestricted PBE on the
    triplet of the same geometry (two spins): _xc_gradient on the fused kernel dqc_grid_xc_gradient_terms against _xc_gradient(fused=
    False) on the torch passes, 1e-12, same molecule, basis and grid and so the same scale -- and (b) the finite-difference tests of
    _xc_gradient through nuclear_gradient in tests/test_gpu_parity.py: test_nuclear_gradient_vs_oracle_finite_differences (LDA, PBE,
    UKS PBE) and test_nuclear_gradient_water_ccpvdz_vs_gpu_finite_differences (SCAN, unrestricted SCAN)."""
    import dqc_amd
    from dqc_amd import gradient as G, lib
    from dqc_amd.utils.datastruct import ValGrad
    if xc == "mgga_x_scan" or not restricted:   # the two cases of (a)
        if restricted:
            qc = _run(xc, "3-21G")
        else:  # a genuine open shell: the triplet
            qc = dqc_amd.KS(dqc_amd.Mol((ZS, POS), basis="3-21G", grid=GRID, spin=2), xc=xc, restricted=False).run(fwd_options=TIGHT)
        eng = qc._engine
        d_aos, _, _ = G._pulay_densities(qc)
        assert len(d_aos) == (1 if restricted else 2)
        if not restricted:
            assert float((d_aos[0] - d_aos[1]).abs().max()) > 1e-2
        got = []
        for fused in (None, False):
            with lib.call_trace() as tr:
                got.append(G._xc_gradient(eng, d_aos, fused=fused))
            calls = [r[0] for r in tr.rows].count("dqc_grid_xc_gradient_terms")
            assert calls == (len(d_aos) if fused is None else 0)
        err = float((got[0] - got[1]).abs().max())
        print("xc gradient %s %s: max |fused - torch passes| %.2e (max |g| %.3e)"
              % (xc, "restricted" if restricted else "unrestricted", err, float(got[1].abs().max())))
        assert err <= 1e-12
        return
    qc = _run(xc, "3-21G")
    eng = qc._engine
    h = eng.hamilton
    gga = h.xcfamily >= 2
    d_aos, d_tot, _ = G._pulay_densities(qc)
    ref = G._xc_gradient(eng, d_aos)
    ao = lib.eval_gto(h._tab, h.rgrid, 3 if gga else 1)
    rho, grho = lib.grid_density(ao[:4], h._nao_ao, lib.pad_matrix(d_tot, h._ld), gga)
    dens = ValGrad(value=rho, grad=grho if gga else None)
    pot = h.xc.get_vxc(dens)
    wts = G._xc_weight_gradient(eng, h.xc.get_edensityxc(dens))
    for fused in (None, False):
        with lib.call_trace() as tr:
            got = G._xc_potential_gradient(eng, ao, d_tot, pot.value, pot.grad if gga else None, fused=fused) + wts
        took = "dqc_grid_xc_gradient_terms" in [r[0] for r in tr.rows]
        assert took == (gga and fused is None)
        err = float((got - ref).abs().max())
        print("xc potential gradient %s fused=%s: max |helper - _xc_gradient| %.2e (max |ref| %.3e)" % (xc, took, err, float(ref.abs().max())))
        assert err <= 1e-12


def test_tddft_gradient_on_hartree_fock_is_excited_gradient(dev):
    import dqc_amd
    qc = _run(None, "3-21G")
    for spin in ("singlet", "triplet"):
        state, _ = _pick_state(qc, True, spin)
        kw = dict(state=state, spin=spin, tda=True, nstates=NST, tol=TOL, ztol=ZTOL)
        a, b = dqc_amd.tddft_gradient(qc, **kw), dqc_amd.excited_gradient(qc, **kw)
        assert a is not b and float((a.gradient - b.gradient).abs().max()) <= 1e-12 and float(a.omega) == float(b.omega)
        assert float((a.density.dm_mo - b.density.dm_mo).abs().max()) <= 1e-12


def test_tddft_gradient_refusals(dev):
    import dqc_amd
    from dqc_amd import lib
    mol = lambda **kw: dqc_amd.Mol((ZS, POS), basis="3-21G", **kw)  # noqa: E731
    pbe = _run("gga_x_pbe+gga_c_pbe", "3-21G")
    refused = [(pbe, dict(spin="triplet"), "tddft_gradient: triplet states of a Kohn-Sham reference"),
               (dqc_amd.KS(mol(grid=GRID), xc="mgga_x_scan").run(), {}, "tddft_gradient: meta-GGA functionals are not supported"),
               (dqc_amd.KS(mol(grid=GRID), xc="lda_x", restricted=False).run(), {}, "tddft_gradient: unrestricted calculations"),
               (dqc_amd.KS(mol(grid=GRID).densityfit(auxbasis="etb"), xc="lda_x").run(), {}, "OrbitalHessian: density fitting is not supported"),
               (dqc_amd.KS(mol(grid=GRID, efield=torch.tensor([0.0, 0.0, 1e-3], dtype=torch.float64)), xc="lda_x").run(), {},
                "nuclear gradients in a non-zero electric field")]
    for qc, kw, msg in refused:
        with lib.call_trace() as tr:
            with pytest.raises(NotImplementedError, match=msg):
                dqc_amd.tddft_gradient(qc, **kw)
        assert not tr.rows, msg                       # nothing reached the library
    with pytest.raises(NotImplementedError, match="excited_gradient: a Kohn-Sham reference .* third-order exchange-correlation kernel"):
        dqc_amd.excited_gradient(pbe)
    with pytest.raises(ValueError, match="tddft_gradient: spin is"):
        dqc_amd.tddft_gradient(pbe, spin="quintet")
    with pytest.raises(ValueError, match="tddft_gradient: state must be >= 0"):
        dqc_amd.tddft_gradient(pbe, state=-1)
    with pytest.raises(ValueError, match="tddft_gradient: state 3 is outside the 2 roots found"):
        dqc_amd.tddft_gradient(pbe, state=3, nstates=2)
