"""CIS / TDHF excited-state gradients on the GPU: the bilinear derivative pass dqc_eri_grad2 (the ERI_OUT_GRAD2 kernels) and
dqc_amd.excited_gradient end to end.

Yardsticks:
  * the kernel, class by class: the oracle's analytic derivative integrals (natives.int2e_ip_quartets, Cartesian) contracted densely
    with two DIFFERENT random matrices (tests/test_excited_gradient_cpu.py: eri_grad2_reference, which uses no symmetry of them), on the
    stratum basis of tests/test_gpu_gradient_terms.py; the bar of that file, 1e-10 of the largest reference component + 1e-13;
  * the kernel against the quadratic pass: eri_grad2(D, D) = eri_grad(D), and 2 eri_grad2(D, P) = Q(D + P) - Q(D) - Q(P), the same
    integrals in other sums, 1e-12 of the largest component (P of the magnitude of D, so that the three-call side does not cancel);
  * end to end -- the test that fixes the factors: excited_gradient against the Richardson-extrapolated central difference of
    HF(Mol(R +- h)).energy() + excitations(...).energies[state], bound 10 |FD(h) - FD(2h)| + 1e-9; the relaxed dipole against the
    finite-field derivative in the same way (construction and bound of tests/test_gpu_mp2_density.py).

The step of the nuclear displacements is H = 4e-3 Bohr (and 2 H), not the 1e-3 of tests/test_gpu_mp2_gradient.py, for this reason.  An SCF
energy of this molecule carries evaluation noise eps of 3e-11 ... 1e-10 Ha (the Fock build's atomic sums: docs/LOG_r29.md section 3, where
the SCF rows miss their own finite difference by up to 8e-8 Ha / Bohr at h = 1e-3; the same rows here, printed by the tests).  A central
difference turns it into sqrt(2) eps / (2 h) = 2e-8 ... 7e-8 at h = 1e-3, while the term of the bound that is meant to carry it,
10 |FD(h) - FD(2h)|, is 10 h^2 |E'''| / 2 of the TRUE energy plus the same noise: for the component (H2, x) the true part of
FD(h) - FD(2h) is 1e-8 ... 3e-8 at h = 1e-3 (tests/test_excited_gradient_cpu.py prints it free of noise for STO-3G: 8e-9 ... 3.5e-8), so
there the bound of that component is made of noise and the test a coin toss.  At H = 4e-3 the noise of a difference is 4 times smaller
(5e-9 ... 2e-8) and the true part of FD(h) - FD(2h) 16 times larger (2e-7 ... 5e-7), so the bound stands an order above the noise of
the extrapolated value; the truncation error of that value, h^4 E^(5) / 30 = 1e-11 E^(5), stays far below it.
Measured on the MI355X: docs/LOG_r30.md."""
import warnings

import numpy as np
import pytest
import torch

from tests import molecules as M
from tests.test_excited_gradient_cpu import dense_eri_ip, eri_grad2_reference

pytestmark = pytest.mark.gpu

TIGHT = {"maxiter": 300, "f_tol": 1e-11}   # (the SCF tolerances of tests/test_gpu_mp2_gradient.py)
TOL, ZTOL = 1e-8, 1e-9
NST = 6                                    # roots asked for everywhere: the state is chosen among the first five
H = 4e-3                                   # nuclear displacement of the finite differences, Bohr (module docstring)
ZS = [8, 1, 1]
POS = [[0.0, 0.0, 0.2217], [0.0, 1.4309, -0.8867], [0.1, -1.4309, -0.8867]]   # H2O, distorted: no symmetry left
DIRECTIONS = {"z": (0.0, 0.0, 1.0), "yz": (0.0, 0.5 ** 0.5, 0.5 ** 0.5)}      # (tests/test_gpu_mp2_density.py)
CASES = {"cis-singlet": ("singlet", True), "tdhf-singlet": ("singlet", False), "cis-triplet": ("triplet", True)}
_WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    for k in sorted(_WORST):
        print("WORST %-34s %.3e" % (k, _WORST[k]))


def _check(what, g, ref, tol=1e-10, floor=1e-13):
    g, ref = np.asarray(g), np.asarray(ref)
    scale = np.abs(ref).max()
    err = np.abs(g - ref).max()
    _WORST[what] = max(_WORST.get(what, 0.0), err / max(scale, 1e-300))
    assert err <= tol * scale + floor, (what, err, scale)


def _dev(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev).contiguous()


def _ncart(l):
    return (l + 1) * (l + 2) // 2


def _k_grad2(dev, tab, a, b, js, ks):
    from dqc_amd import lib
    g = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    lib.eri_grad2(g, _dev(a, dev), _dev(b, dev), js, ks, tab)
    return g.cpu().numpy()


def _k_eri(dev, tab, d, js, ks):
    from dqc_amd import lib
    g = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    lib.eri_grad(g, _dev(d, dev), ks, tab, jscale=js)
    return g.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the kernel
# one contracted (tight + diffuse) shell of every l = 0 ... 4 per atom: the stratum basis of tests/test_gpu_gradient_terms.py
_SPEC = [[(l, [2.9 + 0.3 * a, 0.42 + 0.05 * l], [0.55, 0.6]) for l in range(5)] for a in range(3)]
_TRIPLES = [(a, b, c) for a in range(5) for b in range(a, 5) for c in range(b, 5)]


def _strat_cart(full_t, pick, block):
    """a Cartesian matrix of the full stratum basis that is `block` on the picked shells (atom, l) and zero elsewhere"""
    offs = np.concatenate([[0], np.cumsum([_ncart(int(l)) for l in full_t.bas[:, 1]])])
    idx = np.concatenate([np.arange(offs[a * 5 + l], offs[a * 5 + l + 1]) for (a, l) in pick])
    out = np.zeros((offs[-1], offs[-1]))
    out[np.ix_(idx, idx)] = block
    return out


@pytest.fixture(scope="module")
def strat(dev):
    from oracle import basis as ob
    from dqc_amd import lib
    t = ob.make_tables(M.GRAD3, _SPEC)
    return t, lib.Tables(t.atm, t.bas, t.env)


@pytest.mark.parametrize("la,lb,lc", _TRIPLES)
def test_eri_grad2_class_strata(dev, strat, la, lb, lc):
    """every shell triple (la <= lb <= lc) on three different atoms (the construction of test_eri_grad_class_strata; one triple per case:
    a call walks every quartet of the stratum basis, 1.3 s per triple), A != B random on those shells only: every compile-time class and
    the runtime kernel, g shells in each of the four positions.  Symmetric pairs with (j, k) = (1, 1), (1, 0), (0, 1); an antisymmetric
    pair with (0, 1)"""
    from oracle import basis as ob
    ft, ftab = strat
    rng = np.random.default_rng(600 + 25 * la + 5 * lb + lc)
    sub = ob.make_tables(M.GRAD3, [[_SPEC[0][la]], [_SPEC[1][lb]], [_SPEC[2][lc]]])
    ip = dense_eri_ip(sub, cart=True)
    n = _ncart(la) + _ncart(lb) + _ncart(lc)
    pick = [(0, la), (1, lb), (2, lc)]
    ra, rb = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    a, b = ra + ra.T, rb + rb.T
    af, bf = _strat_cart(ft, pick, a), _strat_cart(ft, pick, b)
    for js, ks in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0)):
        _check("grad2 strata symmetric", _k_grad2(dev, ftab, af, bf, js, ks), eri_grad2_reference(sub, a, b, js, ks, cart=True, ip=ip))
    a, b = ra - ra.T, rb - rb.T
    _check("grad2 strata antisymmetric", _k_grad2(dev, ftab, _strat_cart(ft, pick, a), _strat_cart(ft, pick, b), 0.0, 1.0),
           eri_grad2_reference(sub, a, b, 0.0, 1.0, cart=True, ip=ip))


def test_eri_grad2_diagonal_and_polarisation(dev):
    """CH4 / cc-pVDZ, seeded densities D and P (another seed: the same magnitude, so that Q(D + P) - Q(D) - Q(P) keeps its digits):
    eri_grad2(D, D, j, k) against eri_grad(D, k, jscale=j), and 2 eri_grad2(D, P) against the three calls of the quadratic pass;
    1e-12 of the largest component.  Accumulation into a pre-filled gradient"""
    from oracle import basis as ob
    from dqc_amd import lib
    t = ob.make_tables(M.CH4, "cc-pvdz")
    tab = lib.Tables(t.atm, t.bas, t.env)
    s = lib.int1e("ovlp", tab, dev).cpu().numpy()
    T = lib.cart2sph_matrix(tab, dev).cpu().numpy()
    d, p = (T.T @ M.seeded_dm_ao(t.nao, 10, s, seed) @ T for seed in (3, 4))
    d, p = 0.5 * (d + d.T), 0.5 * (p + p.T)
    assert 0.2 < np.abs(p).max() / np.abs(d).max() < 5.0
    for js, ks in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.6, 0.8)):
        _check("grad2 diagonal = quadratic pass", _k_grad2(dev, tab, d, d, js, ks), _k_eri(dev, tab, d, js, ks), tol=1e-12, floor=0.0)
        three = _k_eri(dev, tab, d + p, js, ks) - _k_eri(dev, tab, d, js, ks) - _k_eri(dev, tab, p, js, ks)
        _check("grad2 polarisation identity", 2.0 * _k_grad2(dev, tab, d, p, js, ks), three, tol=1e-12, floor=0.0)
        _check("grad2 symmetric in (A, B)", _k_grad2(dev, tab, p, d, js, ks), _k_grad2(dev, tab, d, p, js, ks), tol=1e-12, floor=0.0)
    pre = 0.01 * np.random.default_rng(2).standard_normal((tab.natm, 3))
    out = _dev(pre, dev)
    lib.eri_grad2(out, _dev(d, dev), _dev(p, dev), 1.0, 1.0, tab)
    _check("grad2 accumulates", out.cpu().numpy() - pre, _k_grad2(dev, tab, d, p, 1.0, 1.0), tol=1e-12, floor=0.0)


def test_eri_grad2_argument_checks_raise_before_any_launch(dev):
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    t = ob.make_tables((ZS, POS), "3-21G")
    tab = lib.Tables(t.atm, t.bas, t.env)
    n = nat.ao_count(t, True)
    rng = np.random.default_rng(8)
    r = rng.standard_normal((n, n))
    sym, asym = _dev(r + r.T, dev), _dev(r - r.T, dev)
    grad = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    wide = torch.zeros((n, 2 * n), dtype=torch.float64, device=dev)[:, ::2]
    assert tuple(wide.shape) == (n, n) and not wide.is_contiguous()
    with lib.call_trace() as tr:
        for a, b, g, js, what in ((sym[:-1, :-1].contiguous(), sym, grad, 1.0, "eri_grad2: A must be"),      # wrong shape
                                  (sym, sym[:-1].contiguous(), grad, 1.0, "eri_grad2: B must be"),
                                  (sym.to(torch.float32), sym, grad, 1.0, "eri_grad2: A must be"),          # wrong dtype
                                  (sym, sym.cpu(), grad, 1.0, "eri_grad2: B must be"),                      # wrong device
                                  (wide, sym, grad, 1.0, "contiguous"),                                     # a strided view
                                  (sym, sym, grad[:-1].contiguous(), 1.0, "eri_grad2: grad must be"),
                                  (sym, sym, torch.zeros((3, tab.natm), dtype=torch.float64, device=dev).t(), 1.0, "eri_grad2: grad must be"),
                                  (_dev(r, dev), sym, grad, 1.0, "A is neither exactly symmetric nor exactly antisymmetric"),
                                  (sym, _dev(r, dev), grad, 1.0, "B is neither exactly symmetric nor exactly antisymmetric"),
                                  (sym, asym, grad, 0.0, "one matrix is symmetric and the other antisymmetric"),   # mixed parity
                                  (asym, sym, grad, 0.0, "one matrix is symmetric and the other antisymmetric"),
                                  (asym, asym, grad, 1.0, "an antisymmetric pair has no Coulomb part")):    # (after refused calls, too)
            with pytest.raises(lib.DqcAmdError, match=what):
                lib.eri_grad2(g, a, b, js, 1.0, tab)
    assert not tr.rows                               # nothing reached the library
    assert float(grad.abs().max()) == 0.0
    # the C entry point's own gates, with real operands: an error string, nothing launched, the gradient untouched
    L = lib.load()
    with torch.cuda.device(dev):
        for pa, pb, js, msg in ((1, -1, 0.0, "one matrix is symmetric"), (-1, -1, 1.0, "no Coulomb part")):
            rc = L.dqc_eri_grad2(lib._ptr(grad), lib._ptr(sym), lib._ptr(sym), n, pa, pb, js, 1.0, *tab.args(), None)
            assert rc != 0 and msg in L.dqc_last_error().decode()
        rc = L.dqc_eri_grad2(lib._ptr(grad), lib._ptr(sym), lib._ptr(sym), n - 1, 1, 1, 1.0, 1.0, *tab.args(), None)
        assert rc != 0 and "Cartesian functions" in L.dqc_last_error().decode()
    assert float(grad.abs().max()) == 0.0
    # a good call after the refused ones runs, and is the dense reference
    with lib.call_trace() as tr:
        lib.eri_grad2(grad, asym, asym, 0.0, 1.0, tab)
    assert [row[0] for row in tr.rows] == ["dqc_eri_grad2"]
    a = (r - r.T)
    _check("grad2 after refusals", grad.cpu().numpy(), eri_grad2_reference(t, a, a, 0.0, 1.0, cart=True))


# ------------------------------------------------------------------------------------------------ 2. end to end
_RUNS = {}


def _run(basis, atom=None, d=None, m=0, field=None):
    """the converged HF calculation of H2O at POS with coordinate (atom, d) moved by m * H Bohr -- or, field = (direction, m), of M.H2O
    in the field m * 1e-3 a.u. along DIRECTIONS[direction] (field = (None, 0): no field) -- cached"""
    import dqc_amd
    key = (basis, atom, d, m, field)
    if key not in _RUNS:
        if field is not None:
            kw = {}
            if field[1]:
                kw["efield"] = torch.tensor([field[1] * 1e-3 * x for x in DIRECTIONS[field[0]]], dtype=torch.float64)
            mol = dqc_amd.Mol(M.H2O, basis=basis, **kw)
        else:
            pos = [list(p) for p in POS]
            if m:
                pos[atom][d] += m * H
            mol = dqc_amd.Mol((ZS, pos), basis=basis)
        qc = dqc_amd.HF(mol)
        qc.run(fwd_options=TIGHT)
        assert qc.accepted
        _RUNS[key] = qc
    return _RUNS[key]


def _roots(qc, spin, tda):
    import dqc_amd
    return dqc_amd.excitations(qc, nstates=NST, spin=spin, tda=tda, tol=TOL)


def _pick_state(qc, spin, tda):
    """the lowest of the first NST - 1 roots more than 1e-2 Ha away from both neighbours (asserted: there is one)"""
    w = _roots(qc, spin, tda).energies.cpu().tolist()
    for k in range(NST - 1):
        if (k == 0 or w[k] - w[k - 1] > 1e-2) and w[k + 1] - w[k] > 1e-2:
            return k, w
    raise AssertionError("no root of %s is more than 1e-2 Ha from its neighbours" % (w,))


def _fd(basis, atom, d, energy):
    """(FD(h), FD(2h), Richardson) of dE / dR for coordinate (atom, d), h = H"""
    e = {m: energy(_run(basis, atom, d, m)) for m in (1, -1, 2, -2)}
    f1, f2 = (e[1] - e[-1]) / (2 * H), (e[2] - e[-2]) / (4 * H)
    return f1, f2, (4.0 * f1 - f2) / 3.0


COMPONENTS = [(0, 2), (1, 1), (2, 0)]     # (O, z), (H1, y), (H2, x)


@pytest.mark.parametrize("case", sorted(CASES))
def test_excited_gradient_against_finite_differences(dev, case):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.excited import _gradient
    spin, tda = CASES[case]
    qc = _run("3-21G")
    state, w = _pick_state(qc, spin, tda)
    print("%s: roots %s, state %d" % (case, " ".join("%.6f" % x for x in w), state))
    with lib.call_trace() as tr:
        g = dqc_amd.excited_gradient(qc, state=state, spin=spin, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL)
    assert [row[0] for row in tr.rows].count("dqc_eri_grad2") == 3
    assert dqc_amd.excited_gradient(qc, state=state, spin=spin, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL) is g
    assert isinstance(g, dqc_amd.ExcitedGradient) and tuple(g.gradient.shape) == (3, 3) and not g.gradient.requires_grad
    assert g.z_residual <= ZTOL and g.state == state and g.spin == spin and g.tda == tda
    assert float((g.scf - qc.nuclear_gradient()).abs().max()) <= 1e-12       # (two runs of the same atomic sums)
    assert float((g.excitation - (g.gradient - g.scf)).abs().max()) == 0.0
    assert float(g.omega) == w[state] and abs(float(g.e_tot) - float(qc.energy()) - w[state]) <= 1e-12
    ex = _roots(qc, spin, tda)
    assert torch.equal(g.xpy, ex.xpy[state]) and torch.equal(g.xmy, ex.xpy[state] if tda else ex.xmy[state])
    no = 5
    p, tu = g.density.dm_mo, g.density.unrelaxed_mo
    assert float((p - p.t()).abs().max()) <= 1e-14 and abs(float(p.diagonal().sum())) <= 1e-12     # a difference density: traceless
    assert float((p[:no, :no] - tu[:no, :no]).abs().max()) == 0.0 and float(tu[no:, :no].abs().max()) == 0.0
    assert float(p[no:, :no].abs().max()) > 1e-3                                                  # the Z-vector blocks
    with torch.no_grad():
        noz = _gradient(qc, state, spin, tda, NST, TOL, ZTOL, with_z=False).gradient.cpu()
    grad, scf = g.gradient.cpu(), g.scf.cpu()
    energy = lambda q: float(q.energy()) + float(_roots(q, spin, tda).energies[state])  # noqa: E731
    for atom, k in COMPONENTS:
        f1, f2, fr = _fd("3-21G", atom, k, energy)
        bound = 10.0 * abs(f1 - f2) + 1e-9
        diff = abs(fr - float(grad[atom, k]))
        _WORST["gradient - FD, %s" % case] = max(_WORST.get("gradient - FD, %s" % case, 0.0), diff)
        print("(%d, %d)  %s: analytic % .10f  scf % .10f  without z % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  "
              "|analytic - FD| %.2e  bound %.2e" % (atom, k, case, float(grad[atom, k]), float(scf[atom, k]), float(noz[atom, k]), f1, f2, fr,
                                                    diff, bound))
        assert diff <= bound
        assert abs(float(noz[atom, k]) - fr) > bound                        # the relaxation is not silently skipped
    tsum = float(grad.sum(0).abs().max())
    print("%s translational invariance: |sum_A g_A| = %.2e" % (case, tsum))
    assert tsum < 1e-10


def test_excited_gradient_d_shells(dev):
    """cc-pVDZ: d shells in the orbital basis -- the (l + 1, l | d d) classes with both matrices"""
    import dqc_amd
    spin, tda = CASES["cis-singlet"]
    qc = _run("cc-pvdz")
    state, w = _pick_state(qc, spin, tda)
    g = dqc_amd.excited_gradient(qc, state=state, spin=spin, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL)
    f1, f2, fr = _fd("cc-pvdz", 2, 0, lambda q: float(q.energy()) + float(_roots(q, spin, tda).energies[state]))
    bound = 10.0 * abs(f1 - f2) + 1e-9
    print("(2, 0)  CIS / cc-pVDZ state %d: analytic % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  |analytic - FD| %.2e  "
          "bound %.2e" % (state, float(g.gradient[2, 0]), f1, f2, fr, abs(fr - float(g.gradient[2, 0])), bound))
    assert abs(fr - float(g.gradient[2, 0])) <= bound
    assert float(g.gradient.sum(0).abs().max()) < 1e-10


def _fd_dipole(direction, energy):
    """(FD(h), FD(2h), Richardson) of mu . e = -dE/dF + sum Z R . e for the field F e, e = DIRECTIONS[direction]; atomic units, h = 1e-3"""
    zs, pos = M.H2O
    ion = sum(z * sum(x * y for x, y in zip(p, DIRECTIONS[direction])) for z, p in zip(zs, pos))
    e = {m: energy(_run("3-21G", field=(direction, m))) for m in (1, -1, 2, -2)}
    f1, f2 = -(e[1] - e[-1]) / 2e-3 + ion, -(e[2] - e[-2]) / 4e-3 + ion
    return f1, f2, (4.0 * f1 - f2) / 3.0


@pytest.mark.parametrize("case", ["cis-singlet", "tdhf-singlet"])
def test_relaxed_dipole_against_finite_field(dev, case):
    import dqc_amd
    spin, tda = CASES[case]
    qc = _run("3-21G", field=(None, 0))
    state, w = _pick_state(qc, spin, tda)
    g = dqc_amd.excited_gradient(qc, state=state, spin=spin, tda=tda, nstates=NST, tol=TOL, ztol=ZTOL)
    mu = g.density.dipole(unit=None).cpu()
    assert torch.allclose(g.density.dipole(), mu.to(g.gradient.device) * 2.541746473, rtol=1e-12, atol=0)   # Debye by default, as edipole
    from dqc_amd import lib
    from dqc_amd.response import orbital_hessian
    h = qc._engine.hamilton
    sp = orbital_hessian(qc).spins[0]
    c = torch.cat([sp.co, sp.cv], dim=1)
    zbar = c @ (g.density.dm_mo - g.density.unrelaxed_mo) @ c.t()                         # the Z-vector blocks alone
    mu_u = (mu.to(h.device) + torch.einsum("dab,ba->d", lib.int1e("r0", h._tab, h.device), zbar)).cpu()   # the dipole without them
    scf = dqc_amd.edipole(qc, unit=None).cpu()
    along = lambda v, d: float(sum(x * y for x, y in zip(v.tolist(), DIRECTIONS[d])))  # noqa: E731
    for d in ("z", "yz"):
        f1, f2, fr = _fd_dipole(d, lambda q: float(q.energy()) + float(_roots(q, spin, tda).energies[state]))
        bound = 10.0 * abs(f1 - f2) + ZTOL
        print("%-2s  %s state %d: relaxed %.10f  unrelaxed %.10f  scf %.10f  FD(h) %.10f  FD(2h) %.10f  Richardson %.10f  |relaxed - FD| %.2e  "
              "bound %.2e" % (d, case, state, along(mu, d), along(mu_u, d), along(scf, d), f1, f2, fr, abs(fr - along(mu, d)), bound))
        assert abs(fr - along(mu, d)) <= bound
        assert abs(along(mu_u, d) - fr) > bound               # the Z-vector is not silently skipped


def test_excited_gradient_refusals(dev):
    import dqc_amd
    mol = lambda **kw: dqc_amd.Mol((ZS, POS), basis="3-21G", **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match="excited_gradient: a Kohn-Sham reference .* third-order exchange-correlation kernel"):
        dqc_amd.excited_gradient(dqc_amd.KS(mol(grid="sg2"), xc="pbe0").run())
    with pytest.raises(NotImplementedError, match="excited_gradient: a Kohn-Sham reference"):
        dqc_amd.excited_gradient(dqc_amd.KS(mol(grid="sg2"), xc="lda_x").run())
    with pytest.raises(NotImplementedError, match="excited_gradient: unrestricted calculations are not supported"):
        dqc_amd.excited_gradient(dqc_amd.HF(mol(), restricted=False).run())
    with pytest.raises(NotImplementedError, match="OrbitalHessian: density fitting is not supported"):
        dqc_amd.excited_gradient(dqc_amd.HF(mol().densityfit(auxbasis="etb", exchange=True)).run())
    with pytest.raises(NotImplementedError, match="nuclear gradients in a non-zero electric field"):
        dqc_amd.excited_gradient(dqc_amd.HF(mol(efield=torch.tensor([0.0, 0.0, 1e-3], dtype=torch.float64))).run())
    qc = _run("3-21G")
    with pytest.raises(ValueError, match="excited_gradient: spin is"):
        dqc_amd.excited_gradient(qc, spin="quintet")
    with pytest.raises(ValueError, match="excited_gradient: state must be >= 0"):
        dqc_amd.excited_gradient(qc, state=-1)
    with pytest.raises(ValueError, match="excited_gradient: state 3 is outside the 2 roots found"):
        dqc_amd.excited_gradient(qc, state=3, nstates=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # (OrbitalHessian.excite warns about the same residual)
        with pytest.raises(RuntimeError, match="excited_gradient: the excitation vectors are not converged"):
            dqc_amd.excited_gradient(qc, tda=True, tol=1e-300)
