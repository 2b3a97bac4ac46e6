"""GPU tests (-m gpu) of the converged SCF energy as a torch.autograd node (dqc_amd/autograd.py) and of its new kernel,
dqc_int1e_potential (csrc/grad.hip): the electronic electrostatic potential at points, used for dE/dZ.

The derivatives are checked against the existing analytic nuclear gradient, the oracle's finite-difference gradients
(tests/golden/oracle_fd_gradients.json), torch.autograd.gradcheck in the reference's own test patterns (dqc/test/test_hf.py
:82-111, test_ks.py:161-240) and central differences of the energy."""
import json
import os

import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

FD_TOL = {"maxiter": 300, "f_tol": 1e-11}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


# ------------------------------------------------------------------------------------------------
# dqc_int1e_potential against the oracle's nuclear-attraction integrals (unit charge on one centre at a time)
# ------------------------------------------------------------------------------------------------
_BASES = [("h2o-sto3g", M.H2O, "sto-3g"), ("ch4-ccpvdz", M.CH4, "cc-pvdz"), ("ch4-ccpvtz", M.CH4, "cc-pvtz"),
          ("hno-ccpvtz", M.HNO, "cc-pvtz"), ("co-6311ppgss", ([6, 8], [[-1.0, 0.1, 0], [1.1, 0, 0.05]]), "6-311++G**"),
          ("grad3-spdg", M.GRAD3, M.GRAD3_BAS)]


def _shells(zs, basis):
    from oracle import basis as ob
    if isinstance(basis, str):
        return [ob.loadbasis(int(z), basis) for z in zs]
    return [[(l, np.asarray(a, float), ob.wfnormalize(l, a, c)) for (l, a, c) in ab] for ab in basis]


@pytest.mark.parametrize("name,mol,basis", _BASES, ids=[b[0] for b in _BASES])
def test_int1e_potential_vs_oracle(dev, name, mol, basis):
    """V_C = sum D_ab <a|1/|r - P_C||b> at the nuclei and at off-nucleus points (ghost atoms of the oracle table), D = T^T D T
    of a random symmetric D; two calls (and deterministic mode on / off) bitwise equal"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    zs, pos = mol
    rng = np.random.default_rng(3)
    ghosts = rng.uniform(-2.5, 2.5, (3, 3)).tolist() + [[0.35, -0.2, 0.1]]
    t = ob.Tables(list(zs) + [0] * len(ghosts), [list(map(float, p)) for p in pos] + ghosts,
                  _shells(zs, basis) + [[] for _ in ghosts])
    tab = lib.Tables(t.atm, t.bas, t.env)
    n = t.nao
    D = rng.standard_normal((n, n))
    D = (D + D.T) / n
    ref = []
    for c in range(t.natm):
        one = np.zeros(t.natm)
        one[c] = 1.0
        ref.append(-np.sum(D * nat.int1e("nuc", t, zs=one)))  # V = -Z <1/r>
    ref = np.array(ref)
    T = lib.cart2sph_matrix(tab, "cpu").numpy()
    dc = torch.as_tensor(T.T @ D @ T, device=dev).contiguous()
    pts = torch.as_tensor(t.atompos, dtype=torch.float64, device=dev)
    v = lib.int1e_potential(dc, pts, tab)
    err = np.abs(v.cpu().numpy() - ref).max()
    assert err <= 1e-10 * np.abs(ref).max(), (err, np.abs(ref).max())
    v2 = lib.int1e_potential(dc, pts, tab)
    assert torch.equal(v, v2)
    prev = lib.set_deterministic(True)
    try:
        v3 = lib.int1e_potential(dc, pts, tab)
        lib.set_deterministic(False)
        v4 = lib.int1e_potential(dc, pts, tab)
    finally:
        lib.set_deterministic(prev)
    assert torch.equal(v, v3) and torch.equal(v, v4)


# ------------------------------------------------------------------------------------------------
# forces
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h2-321g-rhf", "h2o-sto3g-rhf", "lih-321g-lda", "lih-321g-pbe", "lih-321g-pbe-df",
                                  "ch3-321g-uhf", "ch3-321g-upbe"])
def test_autograd_forces_equal_nuclear_gradient_and_oracle_fd(dev, golden_dir, name):
    """torch.autograd.grad(qc.energy(), pos) == qc.nuclear_gradient() (RHF, RKS LDA / PBE, DF-PBE, UHF, UKS PBE) and the
    oracle's central differences (Becke cut off for KS, as test_nuclear_gradient_vs_oracle_finite_differences runs them)"""
    import dqc_amd
    import dqc_amd.grid as G
    c = json.load(open(os.path.join(golden_dir, "oracle_fd_gradients.json")))[name]
    G._BECKE_CUT = 2.0
    try:
        pos = torch.tensor(c["atompos"], dtype=torch.float64, requires_grad=True)
        m = dqc_amd.Mol((c["atomzs"], pos), basis=c["basis"], grid=c["grid"], spin=c["spin"])
        if c["auxbasis"]:
            m.densityfit(auxbasis=c["auxbasis"])
        qc = (dqc_amd.KS(m, xc=c["xc"]) if c["xc"] else dqc_amd.HF(m)).run(fwd_options=FD_TOL)
        assert qc.accepted
        e = qc.energy()
        assert e.requires_grad
        g, = torch.autograd.grad(e, pos)
        ref = qc.nuclear_gradient().cpu()
    finally:
        G._BECKE_CUT = 0.74
    assert g.shape == pos.shape and g.device == pos.device
    assert float((g - ref).abs().max()) < 1e-12
    assert np.abs(g.numpy() - np.array(c["gradient"])).max() < 2e-6


@pytest.mark.parametrize("atomzs,dist", [([1, 1], 1.0), ([7, 7], 2.0)], ids=["h2", "n2"])
def test_rhf_grad_pos_gradcheck(dev, atomzs, dist):
    """the reference's test_rhf_grad_pos (test_hf.py:82-111), first derivative, non-variational"""
    import dqc_amd

    def get_energy(dist_tensor):
        pos = torch.tensor([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]], dtype=torch.float64) * dist_tensor
        mol = dqc_amd.Mol((atomzs, pos), basis="3-21G")
        return dqc_amd.HF(mol, restricted=True).run(fwd_options=FD_TOL).energy()

    d = torch.tensor(dist, dtype=torch.float64, requires_grad=True)
    # (nondet_tol: the gradient kernels sum with fp64 atomics, two backward passes may differ in the last bits)
    assert torch.autograd.gradcheck(get_energy, (d,), nondet_tol=1e-10)


# ------------------------------------------------------------------------------------------------
# electric field and field gradient
# ------------------------------------------------------------------------------------------------
def _h2o_field(f0, g0=None, **kw):
    import dqc_amd
    ef = (f0,) if g0 is None else (f0, g0)
    m = dqc_amd.Mol(M.H2O, basis="3-21G", efield=ef, **kw)
    return dqc_amd.HF(m).run(fwd_options=FD_TOL)


_F = [2e-3, -1e-3, 3e-3]
_G = [[1e-3, 2e-4, 0.0], [2e-4, -5e-4, 1e-4], [0.0, 1e-4, -5e-4]]


def test_field_derivative_is_the_dipole_and_the_central_difference(dev):
    import dqc_amd
    F = torch.tensor(_F, dtype=torch.float64, requires_grad=True)
    qc = _h2o_field(F)
    gF, = torch.autograd.grad(qc.energy(), F)
    assert gF.shape == (3,)
    mol = qc.get_system()
    ion = (mol.atompos * mol.atomzs.to(torch.float64).unsqueeze(-1)).sum(0)
    mu = dqc_amd.edipole(qc, unit=None).cpu()
    assert float((-gF + ion - mu).abs().max()) < 1e-10
    h = 2e-4
    for d in range(3):
        e = []
        for s in (1, -1):
            f = torch.tensor(_F, dtype=torch.float64)
            f[d] += s * h
            e.append(float(_h2o_field(f).energy()))
        assert abs((e[0] - e[1]) / (2 * h) - float(gF[d])) < 1e-6, d


def test_field_gradient_leaf_vs_central_difference(dev):
    F = torch.tensor(_F, dtype=torch.float64, requires_grad=True)
    G = torch.tensor(_G, dtype=torch.float64, requires_grad=True)
    qc = _h2o_field(F, G)
    gF, gG = torch.autograd.grad(qc.energy(), (F, G))
    assert gF.shape == (3,) and gG.shape == (3, 3)
    h = 2e-4
    for (i, j) in ((0, 0), (1, 2), (2, 1), (2, 2)):
        e = []
        for s in (1, -1):
            g = torch.tensor(_G, dtype=torch.float64)
            g[i, j] += s * h
            e.append(float(_h2o_field(torch.tensor(_F, dtype=torch.float64), g).energy()))
        assert abs((e[0] - e[1]) / (2 * h) - float(gG[i, j])) < 1e-6, (i, j)


# ------------------------------------------------------------------------------------------------
# external potential
# ------------------------------------------------------------------------------------------------
_H2 = ([1, 1], [[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]])


def test_rks_grad_vext_gradcheck(dev):
    """the reference's test_rks_grad_vext (test_ks.py:161-179): vext = |r|^2 p, LDA, 3-21G, grid 3"""
    import dqc_amd
    mol = dqc_amd.Mol(_H2, basis="3-21G", grid=3)
    mol.setup_grid()
    rn = torch.norm(mol.get_grid().get_rgrid(), dim=-1)

    def get_energy(p):
        m = dqc_amd.Mol(_H2, basis="3-21G", grid=3, vext=rn * rn * p)
        return dqc_amd.KS(m, xc="lda_x", restricted=True).run(fwd_options=FD_TOL).energy()

    p = torch.tensor(0.1, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(get_energy, (p,), nondet_tol=1e-10)


def test_vext_derivative_is_weighted_density_on_the_callers_grid(dev):
    import dqc_amd
    mol0 = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3)
    mol0.setup_grid()
    grid = mol0.get_grid()
    rg = grid.get_rgrid()
    vext = (1e-3 * rg[:, 0] + 1e-4 * (rg * rg).sum(-1)).detach().clone().requires_grad_(True)
    m = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3, vext=vext)
    qc = dqc_amd.KS(m, xc="lda_x").run(fwd_options=FD_TOL)
    gv, = torch.autograd.grad(qc.energy(), vext)
    assert gv.shape == vext.shape and gv.device == vext.device
    h = m.get_hamiltonian()
    w = grid.get_dvolume().to(dev)
    rho = h.aodm2dens(qc.aodm(), rg.to(dev))  # the density at every point of the caller's grid
    ref = w * rho
    gv = gv.to(dev)
    assert bool((gv[w == 0] == 0).all())  # (points of weight zero are not resident: exact zeros)
    assert float((gv - ref).abs().max()) < 1e-12 * float(ref.abs().max()) + 1e-15


# ------------------------------------------------------------------------------------------------
# parameters of a user functional
# ------------------------------------------------------------------------------------------------
class _PseudoPBE(torch.nn.Module):
    """PBE-like exchange with parameters (kappa, mu) (the reference's PseudoPBE, test_ks.py:208-225); the potential is
    written out (no autograd inside the SCF's captured steps)"""

    def __init__(self, kappa, mu):
        super().__init__()
        self.kappa, self.mu = kappa, mu

    family = 2

    @staticmethod
    def _terms(rho, grad, kappa, mu):
        ck = (3 * np.pi * np.pi) ** (1.0 / 3)
        a = -3.0 / (4 * np.pi) * ck
        r = rho.abs().clamp_min(1e-20)
        sig = (grad * grad).sum(-2)
        s2 = sig / (4 * ck * ck * r ** (8.0 / 3))
        den = 1 + mu * s2 / kappa
        fx = 1 + kappa - kappa / den
        return a, r, s2, den, fx

    def get_edensityxc(self, densinfo):
        from dqc_amd.utils.datastruct import ValGrad
        if not isinstance(densinfo, ValGrad):
            return 0.5 * (self.get_edensityxc(densinfo.u * 2) + self.get_edensityxc(densinfo.d * 2))
        a, r, s2, den, fx = self._terms(densinfo.value, densinfo.grad, self.kappa, self.mu)
        return a * r ** (4.0 / 3) * fx

    def get_vxc(self, densinfo):
        from dqc_amd.utils.datastruct import ValGrad
        kappa, mu = self.kappa.detach(), self.mu.detach()
        a, r, s2, den, fx = self._terms(densinfo.value, densinfo.grad, kappa, mu)
        dfx = mu / (den * den)                                      # dF / ds2
        ck = (3 * np.pi * np.pi) ** (1.0 / 3)
        vrho = a * (4.0 / 3) * r ** (1.0 / 3) * fx + a * r ** (4.0 / 3) * dfx * (-8.0 / 3) * s2 / r
        dsig = a * r ** (4.0 / 3) * dfx / (4 * ck * ck * r ** (8.0 / 3))
        return ValGrad(value=vrho, grad=2.0 * dsig.unsqueeze(-2) * densinfo.grad)


def test_rks_grad_xc_parameters_gradcheck(dev):
    """the reference's test_rks_grad_vxc (test_ks.py:227-240) with its PBE-like functional"""
    import dqc_amd
    mol = dqc_amd.Mol(_H2, basis="3-21G", grid=3)

    def get_energy(*params):
        return dqc_amd.KS(mol, xc=_PseudoPBE(*params), restricted=True).run(fwd_options=FD_TOL).energy()

    params = tuple(torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in (0.804, 0.21951))
    assert torch.autograd.gradcheck(get_energy, params, nondet_tol=1e-10)


# ------------------------------------------------------------------------------------------------
# nuclear charges and occupations
# ------------------------------------------------------------------------------------------------
_N2 = [[1.2, 0.0, 0.0], [-1.2, 0.0, 0.0]]


def _n2_energy(zs, **kw):
    import dqc_amd
    m = dqc_amd.Mol((zs, torch.tensor(_N2, dtype=torch.float64)), basis="3-21G", **kw)
    return dqc_amd.HF(m).run(fwd_options=FD_TOL).energy()


def test_alchemical_direction_at_integer_charges(dev):
    """examples/03-alchemy-gradient.py: N2 with Z = (7 + d, 7 - d) at d = 0 (electron count fixed)"""
    d = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    e = _n2_energy(torch.cat((7.0 + d, 7.0 - d)), spin=0)
    g, = torch.autograd.grad(e, d)
    h = 1e-4
    fd = (float(_n2_energy(torch.tensor([7.0 + h, 7.0 - h]), spin=0)) -
          float(_n2_energy(torch.tensor([7.0 - h, 7.0 + h]), spin=0))) / (2 * h)
    assert abs(float(g) - fd) < 1e-6, (float(g), fd)


def test_per_atom_charge_derivative_at_fractional_electron_count(dev):
    """N2 with Z = (7.3, 6.9): 14.2 electrons at charge 0, so dE/dZ_C carries the electron-count term (the fractional
    orbital's eigenvalue)"""
    z0 = [7.3, 6.9]
    zs = torch.tensor(z0, dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(_n2_energy(zs, spin=0), zs)
    assert g.shape == (2,)
    h = 1e-4
    for c in range(2):
        e = []
        for s in (1, -1):
            z = torch.tensor(z0, dtype=torch.float64)
            z[c] += s * h
            e.append(float(_n2_energy(z, spin=0)))
        assert abs((e[0] - e[1]) / (2 * h) - float(g[c])) < 1e-6, c


def test_user_orb_weights_derivative_is_the_orbital_energy(dev):
    import dqc_amd
    from dqc_amd.utils.datastruct import SpinParam
    u0, d0 = [1.0, 1.0, 1.0, 1.0, 0.7], [1.0, 1.0, 1.0, 1.0, 0.9]

    def energy(u, d):
        m = dqc_amd.Mol(M.H2O, basis="sto-3g", orb_weights=SpinParam(u=u, d=d))
        return dqc_amd.HF(m).run(fwd_options=FD_TOL).energy()

    u = torch.tensor(u0, dtype=torch.float64, requires_grad=True)
    d = torch.tensor(d0, dtype=torch.float64, requires_grad=True)
    gu, gd = torch.autograd.grad(energy(u, d), (u, d))
    assert gu.shape == (5,) and gd.shape == (5,)
    h = 1e-4
    for ch, i in ((0, 4), (0, 2), (1, 4), (1, 0)):
        e = []
        for s in (1, -1):
            w = [torch.tensor(u0, dtype=torch.float64), torch.tensor(d0, dtype=torch.float64)]
            w[ch][i] += s * h
            e.append(float(energy(*w)))
        assert abs((e[0] - e[1]) / (2 * h) - float((gu, gd)[ch][i])) < 1e-6, (ch, i)


# ------------------------------------------------------------------------------------------------
# unchanged and refused
# ------------------------------------------------------------------------------------------------
def test_energy_without_grad_leaves_is_todays_tensor(dev):
    import dqc_amd
    pos = torch.tensor(M.H2O[1], dtype=torch.float64)
    def todays(qc):
        """energy() must hand back the very tensor it returned before: the driver's stored energy, else dm2energy(dm)"""
        seen = []
        f = qc._engine.dm2energy
        qc._engine.dm2energy = lambda dm: seen.append(f(dm)) or seen[-1]
        stored = getattr(qc, "_energy", None)
        return lambda: stored if stored is not None else seen[0]

    qc = dqc_amd.HF(dqc_amd.Mol((M.H2O[0], pos), basis="sto-3g")).run()
    ref = todays(qc)
    e = qc.energy()
    assert not e.requires_grad and e is ref()
    assert float((e - qc._engine.dm2energy(qc._dm)).abs()) < 1e-12  # (a second evaluation: fp64-atomic sums, last bits)
    pg = pos.clone().requires_grad_(True)
    qg = dqc_amd.HF(dqc_amd.Mol((M.H2O[0], pg), basis="sto-3g")).run()
    ref = todays(qg)
    with torch.no_grad():
        e2 = qg.energy()
    assert not e2.requires_grad and e2 is ref()
    assert abs(float(e2) - float(e)) < 1e-10


def test_second_derivatives_and_unsupported_position_derivatives_raise(dev):
    import dqc_amd
    pos = torch.tensor(M.H2O[1], dtype=torch.float64, requires_grad=True)
    e = dqc_amd.HF(dqc_amd.Mol((M.H2O[0], pos), basis="sto-3g")).run().energy()
    with pytest.raises(NotImplementedError, match="hessian_pos"):
        torch.autograd.grad(e, pos, create_graph=True)
    F = torch.tensor(_F, dtype=torch.float64)
    qf = dqc_amd.HF(dqc_amd.Mol((M.H2O[0], pos), basis="sto-3g", efield=(F,))).run()
    with pytest.raises(NotImplementedError, match="electric field"):
        torch.autograd.grad(qf.energy(), pos)
    Fg = F.clone().requires_grad_(True)
    qf2 = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="sto-3g", efield=(Fg,))).run()
    gF, = torch.autograd.grad(qf2.energy(), Fg)
    assert bool(torch.isfinite(gF).all())
    m0 = dqc_amd.Mol(M.H2O, basis="sto-3g", grid=3)
    m0.setup_grid()
    vext = 1e-3 * m0.get_grid().get_rgrid()[:, 0]
    qv = dqc_amd.HF(dqc_amd.Mol((M.H2O[0], pos), basis="sto-3g", grid=3, vext=vext)).run()
    with pytest.raises(NotImplementedError, match="external potential"):
        torch.autograd.grad(qv.energy(), pos)
