"""DF-CCSD on the GPU end to end: dqc_amd.ccsd with the ladder on dqc_cc_ladder, SCF converged to TIGHT.

Yardsticks, all on the host in fp64 from the calculation's own B tensor and the eigenpairs of its converged Fock matrix:
  * two electrons (H2): the lowest eigenvalue of the n^2 x n^2 alpha-beta Hamiltonian, for which CCSD is exact;
  * `ccsd_reference` (dqc_amd/ccsd.py): the spin-orbital equations of Stanton et al. on dense antisymmetrised integrals -- its residual
    function applied to the amplitudes `ccsd` returns (bar 10 tol) and its own converged energy;
  * size-extensivity: two H2 molecules 100 Bohr apart against the two fragments, each exact.
The bar on an energy is computed from the tensors, as in tests/test_ccsd_cpu.py: sum |2 (ia|jb) - (ib|ja)| 10 tol / min(eps_a - eps_i)."""
import pytest
import torch

from tests import molecules as M
from tests.test_gpu_gw import _host_spins
from tests.test_gpu_mp2 import TIGHT, _run

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


_QC = {}


def _hf(name):
    """converged Hartree-Fock calculations, built once and shared"""
    if name not in _QC:
        import dqc_amd
        fit = dict(auxbasis="etb", exchange=True)
        if name == "h2":
            mol = dqc_amd.Mol(([1, 1], [[0, 0, 0], [0, 0, 1.4]]), basis="cc-pvdz").densityfit(**fit)
        elif name == "h2-long":
            mol = dqc_amd.Mol(([1, 1], [[0, 0, 100.0], [0, 0, 101.6]]), basis="cc-pvdz").densityfit(**fit)
        elif name == "h2-h2":
            mol = dqc_amd.Mol(([1, 1, 1, 1], [[0, 0, 0], [0, 0, 1.4], [0, 0, 100.0], [0, 0, 101.6]]), basis="cc-pvdz").densityfit(**fit)
        elif name == "h2o-ccpvdz":
            mol = dqc_amd.Mol(M.H2O, basis="cc-pvdz").densityfit(**fit)
        qc = dqc_amd.HF(mol).run(fwd_options=TIGHT)
        assert qc.accepted
        _QC[name] = qc
    return _QC[name]


def _bound(bmo, eps, no, tol):
    ovov = torch.einsum("ipa,jpb->iajb", bmo[:no, :, no:], bmo[:no, :, no:])
    return float((2.0 * ovov - ovov.transpose(1, 3)).abs().sum()) * 10.0 * tol / float((eps[no:, None] - eps[None, :no]).min())


def _two_electron_exact(bmo, eps):
    """(E_exact - E_ref) of two electrons in the orbitals of bmo (n, naux, n), orbital 0 doubly occupied in the reference"""
    n = int(eps.numel())
    eri = torch.einsum("pkr,qks->prqs", bmo, bmo)
    h = torch.diag(eps) - (2.0 * eri[:, :, 0, 0] - eri[:, 0, 0, :])
    eye = torch.eye(n, dtype=torch.float64)
    ham = (torch.einsum("pr,qs->pqrs", h, eye) + torch.einsum("pr,qs->pqrs", eye, h) + eri.permute(0, 2, 1, 3)).reshape(n * n, n * n)
    return float(torch.linalg.eigvalsh(0.5 * (ham + ham.t()))[0]) - (2.0 * float(h[0, 0]) + float(eri[0, 0, 0, 0]))


def _against_the_reference(qc, b, r, frozen, what):
    """energy and residuals of the result `r` against `ccsd_reference` on the tensor b (naux, nao, nao) of the calculation"""
    from dqc_amd.ccsd import ccsd_reference, spin_orbital_amplitudes
    bmo, _, eps = _host_spins(qc, b)[0]
    nocc = int((qc._engine.orb_weight != 0).sum())
    bmo, eps, no = bmo[frozen:, :, frozen:].contiguous(), eps[frozen:], nocc - frozen
    e_ref, residual_fn = ccsd_reference(bmo, eps, no, tol=1e-11)
    r1, r2 = residual_fn(*spin_orbital_amplitudes(r.t1.cpu(), r.t2.cpu()))
    worst, diff, bar = max(float(r1.abs().max()), float(r2.abs().max())), abs(float(r.e_corr) - float(e_ref)), _bound(bmo, eps, no, TOL)
    print("CCSD %s: e_corr %.10f  reference %.10f  |diff| %.2e (bar %.2e)  spin-orbital residual of the amplitudes %.2e (bar %.0e)  "
          "e_mp2 %.10f  T1 diagnostic %.4f  %d iterations, residual %.1e, naux %d"
          % (what, float(r.e_corr), float(e_ref), diff, bar, worst, 10 * TOL, float(r.e_mp2), r.t1_diagnostic, r.niter, r.residual, r.naux))
    assert r.converged and r.residual < TOL and r.frozen == frozen
    assert tuple(r.t1.shape) == (no, int(eps.numel()) - no) and tuple(r.t2.shape) == (no, no) + 2 * (int(eps.numel()) - no,)
    assert float((r.t2 - r.t2.permute(1, 0, 3, 2)).abs().max()) <= 1e-14 and not r.t2.requires_grad
    assert worst <= 10 * TOL
    assert diff <= bar
    assert abs(float(r.e_tot) - (float(qc.energy()) + float(r.e_corr))) < 1e-12


def test_h2_is_solved_exactly(dev):
    import dqc_amd
    qc = _hf("h2")
    r = dqc_amd.ccsd(qc, tol=TOL)
    bmo, _, eps = _host_spins(qc, qc._engine.hamilton.df._b)[0]
    exact, bar = _two_electron_exact(bmo, eps), _bound(bmo, eps, 1, TOL)
    print("CCSD H2 / cc-pVDZ (%d orbitals, naux %d): e_corr %.10f  exact %.10f  |diff| %.2e (bar %.2e)  e_mp2 %.10f  %d iterations"
          % (eps.numel(), r.naux, float(r.e_corr), exact, abs(float(r.e_corr) - exact), bar, float(r.e_mp2), r.niter))
    assert r.converged and r.df is qc._engine.hamilton.df
    assert abs(float(r.e_corr) - exact) <= bar


@pytest.mark.parametrize("frozen", [0, 1])
def test_h2o_on_the_exact_tile_store(dev, frozen):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.postscf import b_tensor
    qc = _run("h2o-rhf-exact")
    assert qc._engine.hamilton.df is None
    with lib.call_trace() as tr:
        r = dqc_amd.ccsd(qc, frozen=frozen, auxbasis="etb", tol=TOL)
    names = [row[0] for row in tr.rows]
    if names:                                           # (not the memoised object of an earlier test of this session)
        assert names.count("dqc_cc_ladder") == r.niter and "dqc_bse_exchange" not in names
    _against_the_reference(qc, b_tensor(qc, "etb")._b, r, frozen, "H2O / 3-21G exact integrals, etb, frozen=%d" % frozen)
    m = dqc_amd.mp2(qc, frozen=frozen, auxbasis="etb")
    print("   e_mp2 - mp2().e_corr %.2e (bar 1e-11)" % (float(r.e_mp2) - float(m.e_corr)))
    assert abs(float(r.e_mp2) - float(m.e_corr)) <= 1e-11 and r.df is m.df
    with lib.call_trace() as tr:
        again = dqc_amd.ccsd(qc, frozen=frozen, auxbasis="etb", tol=TOL)
    assert again is r and not tr.rows                   # memoised on the converged state


def test_the_first_call_runs_one_ladder_per_iteration(dev):
    import dqc_amd
    from dqc_amd import lib
    qc = _run("h2o-rhf-exact")
    with lib.call_trace() as tr:
        r = dqc_amd.ccsd(qc, auxbasis="etb", tol=1e-7, maxiter=40)       # (an argument set no other test asks for)
    names = [row[0] for row in tr.rows]
    assert r.converged and names.count("dqc_cc_ladder") == r.niter and "dqc_bse_exchange" not in names


def test_h2o_cc_pvdz(dev):
    """nvir = 19: a second virtual tile with a ragged edge in a real calculation"""
    import dqc_amd
    qc = _hf("h2o-ccpvdz")
    r = dqc_amd.ccsd(qc, tol=TOL)
    assert tuple(r.t2.shape) == (5, 5, 19, 19)
    _against_the_reference(qc, qc._engine.hamilton.df._b, r, 0, "H2O / cc-pVDZ fitted")


def test_two_distant_h2_molecules_are_the_sum_of_the_fragments(dev):
    import dqc_amd
    ab, a, b = _hf("h2-h2"), _hf("h2"), _hf("h2-long")
    e = [float(dqc_amd.ccsd(qc, tol=TOL).e_corr) for qc in (ab, a, b)]
    m = [float(dqc_amd.mp2(qc).e_corr) for qc in (ab, a, b)]
    d_cc, d_mp2 = abs(e[0] - e[1] - e[2]), abs(m[0] - m[1] - m[2])
    bar = 10.0 * max(1e-10, d_mp2)
    print("CCSD H2 ... H2 (100 Bohr): e_corr %.10f = %.10f + %.10f + %.2e  (bar %.2e: 10 x the MP2 defect %.2e)"
          % (e[0], e[1], e[2], e[0] - e[1] - e[2], bar, d_mp2))
    for qc, ec in ((a, e[1]), (b, e[2])):               # each fragment is exact
        bmo, _, eps = _host_spins(qc, qc._engine.hamilton.df._b)[0]
        assert abs(ec - _two_electron_exact(bmo, eps)) <= _bound(bmo, eps, 1, TOL)
    assert d_cc <= bar


def test_refusals_on_real_calculations(dev):
    import dqc_amd
    with pytest.raises(NotImplementedError, match="ccsd: an unrestricted"):
        dqc_amd.ccsd(_run("h2o-uhf-df"))
    h2 = ([1, 1], [[0, 0, 0], [0, 0, 1.4]])
    pbe = dqc_amd.KS(dqc_amd.Mol(h2, basis="3-21G", grid="sg2").densityfit(auxbasis="etb", exchange=True), xc="gga_x_pbe+gga_c_pbe")
    with pytest.raises(NotImplementedError, match="ccsd: a Kohn-Sham reference"):
        dqc_amd.ccsd(pbe.run(fwd_options=TIGHT))
    # (Hartree-Fock cannot run on a fit without exchange: the refusal is raised from the Hamiltonian, before the state is asked for)
    jonly = dqc_amd.HF(dqc_amd.Mol(h2, basis="3-21G").densityfit(auxbasis="etb"))
    with pytest.raises(NotImplementedError, match="ccsd: .*Coulomb term only"):
        dqc_amd.ccsd(jonly)
    with pytest.raises(ValueError, match="ccsd: frozen"):
        dqc_amd.ccsd(_run("h2o-rhf-exact"), frozen=-1, auxbasis="etb")
    with pytest.raises(NotImplementedError, match="ccsd: no occupied orbital is left after freezing 5 of 5"):
        dqc_amd.ccsd(_run("h2o-rhf-exact"), frozen=5, auxbasis="etb")
