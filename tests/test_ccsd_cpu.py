"""DF-CCSD on the host: the algebra of dqc_amd/ccsd.py driven with an einsum ladder (W stored) on model tensors.

The models are physical in form: a random tensor B[p, P, q] = B[q, P, p] (naux 12 ... 20) over 6 ... 8 orbitals, orbital energies with a
gap of at least 1.5, the one-electron operator h = diag(eps) - G[B] that makes diag(eps) the Fock matrix, scaled so that the iteration
converges while t1 stays visible (largest |t1| about 1e-2).

Yardsticks:
  * two electrons: the lowest eigenvalue of the n^2 x n^2 alpha-beta Hamiltonian, for which CCSD is exact;
  * `ccsd_reference`: the spin-orbital equations of Stanton et al. on dense antisymmetrised integrals from the same B -- the residual
    function applied to the production amplitudes expanded to spin orbitals, and its own converged energy.
The bar on an energy is computed from the tensors: sum |2 (ia|jb) - (ib|ja)| 10 tol / min(eps_a - eps_i) -- the energy is linear in t2
with these weights, and amplitudes whose residual is below tol are within about tol / min D of the solution (10: the off-diagonal
part of the Jacobian and the quadratic t1 term).  Both sides are converged (1e-11, 1e-12) or diagonalised in fp64."""
import sys
import warnings
from types import SimpleNamespace

import pytest
import torch

import dqc_amd
from dqc_amd.ccsd import CCSD, ccsd_reference, einsum_ladder, residuals, solve, spin_orbital_amplitudes
from tests.test_mp2_cpu import _fake_qc


def _model(no, nv, naux, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    nmo = no + nv
    b = torch.randn((nmo, naux, nmo), dtype=torch.float64, generator=g)
    b = (scale * 0.5 / naux ** 0.5) * (b + b.permute(2, 1, 0))
    eps = torch.cat([-1.0 - 0.3 * torch.arange(no - 1, -1, -1, dtype=torch.float64), 0.5 + 0.4 * torch.arange(nv, dtype=torch.float64)])
    return b.contiguous(), eps


def _bound(b, eps, no, tol):
    ovov = torch.einsum("ipa,jpb->iajb", b[:no, :, no:], b[:no, :, no:])
    gap = float((eps[no:, None] - eps[None, :no]).min())
    return float((2.0 * ovov - ovov.transpose(1, 3)).abs().sum()) * 10.0 * tol / gap


_SOLVED = {}


def _solved(no, nv, naux, seed, tol):
    """the converged production amplitudes of a model, computed once and shared (read only)"""
    key = (no, nv, naux, seed, tol)
    if key not in _SOLVED:
        b, eps = _model(no, nv, naux, seed)
        _SOLVED[key] = (b, eps, solve(b, eps, no, einsum_ladder, tol=tol, maxiter=80))
    return _SOLVED[key]


@pytest.mark.parametrize("nv,naux", [(1, 12), (3, 16), (5, 20), (7, 13)])
def test_two_electrons_are_solved_exactly(nv, naux):
    tol = 1e-10
    b, eps = _model(1, nv, naux, 100 + nv)
    n = 1 + nv
    s = solve(b, eps, 1, einsum_ladder, tol=tol, maxiter=80)
    assert s["converged"]
    eri = torch.einsum("pkr,qks->prqs", b, b)                                  # (pr|qs)
    h = torch.diag(eps) - (2.0 * eri[:, :, 0, 0] - eri[:, 0, 0, :])
    eye = torch.eye(n, dtype=torch.float64)
    ham = (torch.einsum("pr,qs->pqrs", h, eye) + torch.einsum("pr,qs->pqrs", eye, h) + eri.permute(0, 2, 1, 3)).reshape(n * n, n * n)
    e0 = float(torch.linalg.eigvalsh(0.5 * (ham + ham.t()))[0])
    e_ref = 2.0 * float(h[0, 0]) + float(eri[0, 0, 0, 0])
    diff, bar = abs(float(s["e_corr"]) + e_ref - e0), _bound(b, eps, 1, tol)
    print("two electrons in %d orbitals: E_ref %.10f  e_corr %.10f  exact - E_ref %.10f  |diff| %.2e  (bar %.2e; %d iterations, "
          "largest |t1| %.1e)" % (n, e_ref, float(s["e_corr"]), e0 - e_ref, diff, bar, s["niter"], float(s["t1"].abs().max())))
    assert float(s["e_corr"]) < 0.0 and diff <= bar


@pytest.mark.parametrize("nv", [4, 5])
def test_production_amplitudes_solve_the_reference_equations(nv):
    tol = 1e-11
    b, eps, s = _solved(3, nv, 14 + nv, 30 + nv, tol)
    assert s["converged"] and s["residual"] < tol
    e_ref, residual_fn = ccsd_reference(b, eps, 3, tol=1e-12)
    r1, r2 = residual_fn(*spin_orbital_amplitudes(s["t1"], s["t2"]))
    worst = max(float(r1.abs().max()), float(r2.abs().max()))
    diff, bar = abs(float(s["e_corr"]) - float(e_ref)), _bound(b, eps, 3, tol)
    ovov = torch.einsum("ipa,jpb->iajb", b[:3, :, 3:], b[:3, :, 3:])
    d = eps[:3, None, None, None] + eps[None, None, :3, None] - eps[None, 3:, None, None] - eps[None, None, None, 3:]
    e_mp2 = float((ovov * (2.0 * ovov - ovov.transpose(1, 3)) / d).sum())
    print("CCSD model (nocc 3, nvir %d): e_corr %.12f  reference %.12f  |diff| %.2e (bar %.2e)  spin-orbital residual %.2e (bar %.0e)  "
          "e_mp2 %.12f (written out: diff %.1e)  %d iterations, largest |t1| %.1e"
          % (nv, float(s["e_corr"]), float(e_ref), diff, bar, worst, 10 * tol, float(s["e_mp2"]), float(s["e_mp2"]) - e_mp2, s["niter"],
             float(s["t1"].abs().max())))
    assert float(s["t1"].abs().max()) > 1e-3            # (the singles terms are exercised)
    assert worst <= 10 * tol
    assert diff <= bar
    assert abs(float(s["e_mp2"]) - e_mp2) <= 1e-14


def test_pair_symmetry():
    _, _, s = _solved(3, 5, 19, 35, 1e-11)
    t2 = s["t2"]
    assert float((t2 - t2.permute(1, 0, 3, 2)).abs().max()) <= 1e-15
    assert float((t2 - t2.transpose(2, 3)).abs().max()) > 1e-4      # (no more symmetry than that)


def test_frozen_core_is_the_calculation_without_that_orbital():
    b, eps = _model(3, 4, 15, 77)
    frozen = solve(b, eps, 3, einsum_ladder, frozen=1, tol=1e-11, maxiter=80)
    cut = solve(b[1:, :, 1:].contiguous(), eps[1:].contiguous(), 2, einsum_ladder, tol=1e-11, maxiter=80)
    full = solve(b, eps, 3, einsum_ladder, tol=1e-11, maxiter=80)
    assert frozen["converged"] and tuple(frozen["t2"].shape) == (2, 2, 4, 4) and tuple(frozen["t1"].shape) == (2, 4)
    for k in ("t1", "t2", "e_corr", "e_mp2"):
        assert torch.equal(frozen[k], cut[k])
    assert frozen["niter"] == cut["niter"] and abs(float(frozen["e_corr"])) < abs(float(full["e_corr"]))
    # the reference on the tensors of the active orbitals agrees
    e_ref, _ = ccsd_reference(b[1:, :, 1:].contiguous(), eps[1:], 2, tol=1e-12)
    diff, bar = abs(float(frozen["e_corr"]) - float(e_ref)), _bound(b[1:, :, 1:], eps[1:], 2, 1e-11)
    print("frozen=1 of 3: e_corr %.12f (all active %.12f), reference on the cut tensors: |diff| %.2e (bar %.2e)"
          % (float(frozen["e_corr"]), float(full["e_corr"]), diff, bar))
    assert diff <= bar


def _host_qc(**kw):
    """the stand-in of tests/test_mp2_cpu.py with what `ccsd` reads on top: a closed-shell Hartree-Fock calculation of 3 occupied and 4
    virtual orbitals on a fitted-exchange Hamiltonian"""
    qc = _fake_qc(**kw)
    if "weights" not in kw:
        qc._engine.orb_weight = torch.tensor([2.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0])
    qc._engine.is_ks = False
    qc._engine.shape = (7, 7)
    qc._engine.hamilton.df.exchange = True
    return qc


def test_too_few_iterations_warn_and_say_so(monkeypatch):
    mod = sys.modules["dqc_amd.ccsd"]
    b, eps = _model(3, 4, 15, 77)
    df = SimpleNamespace(_b=torch.zeros((15, 1, 1)))
    monkeypatch.setattr(mod, "_compute", lambda qc, frozen, auxbasis, tol, maxiter, diis: (
        df, solve(b, eps, 3, einsum_ladder, tol=tol, maxiter=maxiter, diis=diis)))
    qc = _host_qc()
    qc._has_run, qc._fock, qc.energy = True, object(), lambda: torch.tensor(-1.0, dtype=torch.float64)
    with pytest.warns(UserWarning, match=r"ccsd: not converged in 3 iterations: the largest residual is \d\.\d+e-\d+"):
        r = dqc_amd.ccsd(qc, maxiter=3)
    assert isinstance(r, CCSD) and not r.converged and r.niter == 3 and r.residual > 1e-8 and r.naux == 15
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ok = dqc_amd.ccsd(qc, tol=1e-9)
    assert ok.converged and ok.residual < 1e-9 and ok is dqc_amd.ccsd(qc, tol=1e-9)        # memoised per argument set
    assert abs(float(ok.e_tot) - (-1.0 + float(ok.e_corr))) < 1e-15 and ok.frozen == 0
    assert abs(ok.t1_diagnostic - float(ok.t1.norm()) / 3 ** 0.5) < 1e-15
    # the residual reported is that of the returned amplitudes
    o1, o2, _ = residuals(b, eps, 3, r.t1, r.t2, einsum_ladder)
    assert r.residual == max(float(o1.abs().max()), float(o2.abs().max()))


class _Untouchable:
    """a calculation whose state may not be looked at: every refusal below is raised from the arguments and the engine's attributes"""

    def __init__(self, qc):
        self._engine = qc._engine

    def __getattr__(self, name):
        raise AssertionError("ccsd looked at qc.%s before refusing" % name)


def test_refusals_before_anything_is_computed():
    ccsd = dqc_amd.ccsd
    u = SimpleNamespace(u=torch.tensor([1.0, 0.0]), d=torch.tensor([1.0, 0.0]))
    with pytest.raises(NotImplementedError, match="ccsd: an unrestricted"):
        ccsd(_Untouchable(_host_qc(weights=u, polarized=True)))
    ks = _host_qc()
    ks._engine.is_ks = True
    with pytest.raises(NotImplementedError, match="ccsd: a Kohn-Sham reference"):
        ccsd(_Untouchable(ks))
    jonly = _host_qc()
    jonly._engine.hamilton.df.exchange = False
    with pytest.raises(NotImplementedError, match="ccsd: .*Coulomb term only.*auxbasis"):
        ccsd(_Untouchable(jonly))
    # everything postscf.unsupported refuses, in the name of ccsd
    with pytest.raises(NotImplementedError, match="ccsd: .*shard_over"):
        ccsd(_Untouchable(_host_qc(sharded=True)))
    with pytest.raises(NotImplementedError, match="ccsd: .*overlap"):
        ccsd(_Untouchable(_host_qc(method="overlap")))
    with pytest.raises(NotImplementedError, match="ccsd: .*user-given"):
        ccsd(_Untouchable(_host_qc(user_weights=object())))
    with pytest.raises(NotImplementedError, match="ccsd: .*restricted open-shell"):
        ccsd(_Untouchable(_host_qc(weights=torch.tensor([2.0, 2.0, 1.0, 0.0]))))
    with pytest.raises(NotImplementedError, match="ccsd: .*fractional"):
        ccsd(_Untouchable(_host_qc(weights=torch.tensor([2.0, 0.5, 0.0]))))
    # nothing left to correlate
    with pytest.raises(NotImplementedError, match="ccsd: no occupied orbital is left after freezing 3 of 3"):
        ccsd(_Untouchable(_host_qc()), frozen=3)
    with pytest.raises(NotImplementedError, match="ccsd: .*no virtual"):
        full = _host_qc()
        full._engine.shape = (3, 3)
        ccsd(_Untouchable(full))
    # the arguments
    for kw, what in (({"frozen": -1}, "frozen"), ({"tol": 0.0}, "tol"), ({"tol": -1e-8}, "tol"), ({"maxiter": 0}, "maxiter")):
        with pytest.raises(ValueError, match="ccsd: " + what):
            ccsd(_Untouchable(_host_qc()), **kw)
