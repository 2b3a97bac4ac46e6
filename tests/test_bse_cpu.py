"""BSE@G0W0 without a GPU: the yardsticks of dqc_amd/bse.py against brute force and closed forms, the quasiparticle ladder and the
refusals.

  * `exchange_reference` against the explicit five-index einsum, noise in the padding columns: 1e-12 sum |terms| per element, the
    standing bar of the fp64 contractions;
  * the static W identity on the synthetic spectra of tests/test_gw_cpu.py: `static_w_reference` with M = (1 + Q(0))^-1 by Cholesky
    against the closed form (ij|ab) - sum_s 2 w^s_ij w^s_ab / Om_s of `gw.spectral_reference`, 1e-12 of the largest element (the bar
    of the W identity there);
  * a one-occupied, one-virtual model, where A and B are numbers;
  * `bse_reference`: full = TDA when B vanishes; TDA singlets above triplets state by state (A_s - A_t = 2 v >= 0, Weyl), slack 1e-12;
    M = 1, E = eps against the textbook TDHF A and B from (ia|jb), (ij|ab), (ib|ja), 1e-13."""
import math
from types import SimpleNamespace

import pytest
import torch

from dqc_amd.bse import (bse, bse_matrices, bse_reference, exchange_reference, quasiparticle_ladder, solve_dense, static_w_reference,
                         window_orbitals)
from dqc_amd.gw import spectral_reference
from dqc_amd.rpa import response_reference
from tests.test_gw_cpu import _spectrum
from tests.test_mp2_cpu import _fake_qc


@pytest.mark.parametrize("np_,nq,nr,ns,naux,nvec", [(1, 1, 1, 1, 1, 1), (2, 3, 5, 4, 3, 2), (3, 7, 7, 6, 5, 1)])
def test_exchange_reference_against_brute_force(np_, nq, nr, ns, naux, nvec):
    g = torch.Generator().manual_seed(500 + naux)
    l = torch.randn((np_, naux, nr + 3), dtype=torch.float64, generator=g)   # (three padding columns of noise: ignored)
    r = torch.randn((nq, naux, ns + 2), dtype=torch.float64, generator=g)
    x = torch.randn((nvec, nr, ns), dtype=torch.float64, generator=g)
    t = torch.einsum("pPr,vrs,qPs->vpqPrs", l[:, :, :nr], x, r[:, :, :ns])
    ref, mag = t.sum((3, 4, 5)), t.abs().sum((3, 4, 5))
    out = exchange_reference(l, x, r, nr, ns)
    assert tuple(out.shape) == (nvec, np_, nq)
    assert torch.all((out - ref).abs() <= 1e-12 * mag)
    lz = l.clone()
    lz[:, :, nr:] = 0.0
    assert torch.equal(out, exchange_reference(lz, x, r, nr, ns))


def _static_m(bov, eps, no):
    q0 = response_reference(bov, eps[:no], eps[no:], torch.zeros(1, dtype=torch.float64), 4.0)[0]
    eye = torch.eye(q0.shape[0], dtype=torch.float64)
    return torch.cholesky_solve(eye, torch.linalg.cholesky(q0 + eye))


@pytest.mark.parametrize("no,nv,naux,amp,side", [(3, 6, 24, 0.3, True), (2, 7, 24, 0.1, False), (1, 1, 3, 0.5, True)])
def test_static_w_is_the_closed_form(no, nv, naux, amp, side):
    """W_ij,ab = (ij|ab) + (ij| Wc(0) |ab) with the spectral form of Wc at w = 0: -sum_s w^s_ij w^s_ab 2 / Om_s"""
    bnm, bov, eps = _spectrum(no, nv, naux, 11 + no, amp, side)
    nmo = no + nv
    m = _static_m(bov, eps, no)
    boo, bvv = bnm[:no, :, :no], bnm[no:, :, no:nmo]
    w = static_w_reference(boo, bvv, m)
    sp = spectral_reference([(bnm, bov, eps)])
    ws = sp.w[0]                                                          # (nexc, nmo, nmo): w^s_nm
    closed = torch.einsum("ipj,apb->ijab", boo, bvv) - torch.einsum("s,sij,sab->ijab", 2.0 / sp.omega, ws[:, :no, :no], ws[:, no:, no:])
    err, big = float((w - closed).abs().max()), float(closed.abs().max())
    print("static W (no %d, nv %d, naux %d): largest |W - closed form| %.2e of %.3e" % (no, nv, naux, err, big))
    assert err <= 1e-12 * big
    assert float((w - torch.einsum("ipj,apb->ijab", boo, bvv)).abs().max()) > 1e-6 * big   # (the screening is not nothing)


def test_one_occupied_one_virtual_by_hand():
    g = torch.Generator().manual_seed(3)
    naux = 4
    bf = torch.randn((naux, 2, 2), dtype=torch.float64, generator=g) * 0.4
    bf = 0.5 * (bf + bf.transpose(1, 2))
    bmo = bf.permute(1, 0, 2).contiguous()                                # [p, P, q]
    eps = torch.tensor([-0.5, 0.3], dtype=torch.float64)
    mm = torch.randn((naux, naux), dtype=torch.float64, generator=g) * 0.1
    m = torch.eye(naux, dtype=torch.float64) - mm @ mm.t() * 0.5          # symmetric, positive definite, not 1
    d = 0.8
    v = float((bf[:, 0, 1] ** 2).sum())                                   # (ia|ia)
    wd = float(bf[:, 0, 0] @ m @ bf[:, 1, 1])                             # W_ii,aa
    wx = float(bf[:, 0, 1] @ m @ bf[:, 0, 1])                             # W_ia,ia
    for spin, c in (("singlet", 2.0), ("triplet", 0.0)):
        a, b = d + c * v - wd, c * v - wx
        w_tda, x = bse_reference(bmo, eps, 1, m, spin, True)
        w_full, xpy = bse_reference(bmo, eps, 1, m, spin, False)
        assert abs(float(w_tda[0]) - a) < 1e-14 and abs(abs(float(x[0, 0])) - 1.0) < 1e-14
        assert a - b > 0 and a + b > 0
        assert abs(float(w_full[0]) - math.sqrt((a - b) * (a + b))) < 1e-14
        assert abs(abs(float(xpy[0, 0])) - math.sqrt((a - b) / float(w_full[0]))) < 1e-14   # (X+Y)(X-Y) = 1, (A+B)(X+Y) = w (X-Y)


def test_bse_reference_consistency():
    bnm, bov, eps = _spectrum(3, 6, 24, 14, 0.05, True)                # (integrals small against the gaps: a stable reference)
    no, nmo = 3, 9
    eps = eps.clone()
    eps[:no] = torch.linspace(-1.2, -0.4, no, dtype=torch.float64)        # (a spectrum on which A - B stays positive definite)
    eps[no:] = torch.linspace(0.3, 2.0, nmo - no, dtype=torch.float64)
    m = _static_m(bov, eps, no)
    bmo = bnm[:, :, :nmo].contiguous()
    # full = TDA when B vanishes (no occupied-virtual block: v = 0, W_ib,ja = 0)
    bz = bmo.clone()
    bz[:no, :, no:] = 0.0
    bz[no:, :, :no] = 0.0
    for spin in ("singlet", "triplet"):
        a, b = bse_matrices(bz, eps, no, m, spin)
        assert float(b.abs().max()) == 0.0
        wt, wf = bse_reference(bz, eps, no, m, spin, True)[0], bse_reference(bz, eps, no, m, spin, False)[0]
        assert float((wt - wf).abs().max()) < 1e-12
    # TDA: singlet above triplet, state by state
    ws, wt = bse_reference(bmo, eps, no, m, "singlet", True)[0], bse_reference(bmo, eps, no, m, "triplet", True)[0]
    assert bool(torch.all(ws >= wt - 1e-12)) and float((ws - wt).max()) > 1e-6
    # M = 1, E = eps: the textbook TDHF matrices
    n, nv = no * (nmo - no), nmo - no
    boo, bo, bvv = bmo[:no, :, :no], bmo[:no, :, no:], bmo[no:, :, no:]
    iajb = torch.einsum("ipa,jpb->iajb", bo, bo)                          # (ia|jb)
    ijab = torch.einsum("ipj,apb->ijab", boo, bvv)                        # (ij|ab)
    d = torch.diag((eps[None, no:] - eps[:no, None]).reshape(n))
    for spin, c in (("singlet", 2.0), ("triplet", 0.0)):
        a, b = bse_matrices(bmo, eps, no, None, spin)
        a_ref = d + c * iajb.reshape(n, n) - ijab.permute(0, 2, 1, 3).reshape(n, n)                 # A_ia,jb = D + c (ia|jb) - (ij|ab)
        b_ref = c * iajb.reshape(n, n) - iajb.permute(0, 3, 2, 1).reshape(n, n)                     # B_ia,jb = c (ia|jb) - (ib|ja)
        assert float((a - a_ref).abs().max()) < 1e-13 and float((b - b_ref).abs().max()) < 1e-13
        w, xpy = solve_dense(a, b)
        # the full problem's own equation: (A - B)(A + B)(X + Y) = w^2 (X + Y)
        lhs = (a - b) @ (a + b) @ xpy.t()
        assert float((lhs - xpy.t() * (w * w)[None, :]).abs().max()) < 1e-11
    assert nv == 6


def test_quasiparticle_ladder():
    eps = torch.tensor([-20.0, -1.3, -0.7, -0.5, 0.2, 0.3, 0.9, 1.5], dtype=torch.float64)
    nocc = 4
    # the window inside, the scissor outside on both sides
    orbs = window_orbitals(nocc, 8, (2, 2))
    assert orbs == [2, 3, 4, 5]
    qp = torch.tensor([-0.75, -0.58, 0.26, 0.33], dtype=torch.float64)
    e = quasiparticle_ladder(eps, nocc, orbs, qp)
    assert torch.equal(e[2:6], qp)
    assert float(e[0]) == -20.0 + (-0.75 - -0.7) and float(e[1]) == -1.3 + (-0.75 - -0.7)     # the lowest corrected occupied orbital's
    assert float(e[6]) == 0.9 + (0.33 - 0.3) and float(e[7]) == 1.5 + (0.33 - 0.3)            # the highest corrected virtual orbital's
    assert torch.equal(eps, torch.tensor([-20.0, -1.3, -0.7, -0.5, 0.2, 0.3, 0.9, 1.5], dtype=torch.float64))   # (the input is left alone)
    # a window larger than the orbital count: clipped, every orbital its own energy
    orbs = window_orbitals(nocc, 8, (10, 10))
    assert orbs == list(range(8))
    qp = eps + torch.linspace(-0.1, 0.1, 8, dtype=torch.float64)
    assert torch.equal(quasiparticle_ladder(eps, nocc, orbs, qp), qp)
    # a window with no virtual side: the virtual orbitals keep eps
    orbs = window_orbitals(nocc, 8, (3, 0))
    assert orbs == [1, 2, 3]
    e = quasiparticle_ladder(eps, nocc, orbs, torch.tensor([-1.4, -0.8, -0.6], dtype=torch.float64))
    assert torch.equal(e[4:], eps[4:]) and float(e[0]) == -20.0 + (-1.4 - -1.3) and torch.equal(e[1:4], torch.tensor([-1.4, -0.8, -0.6], dtype=torch.float64))
    # and none on the occupied side
    e = quasiparticle_ladder(eps, nocc, [4], torch.tensor([0.25], dtype=torch.float64))
    assert torch.equal(e[:4], eps[:4]) and float(e[4]) == 0.25 and float(e[7]) == 1.5 + (0.25 - 0.2)
    for bad in (lambda: quasiparticle_ladder(eps, nocc, [2, 3], torch.zeros(3, dtype=torch.float64)),
                lambda: quasiparticle_ladder(eps, nocc, [2, 2], torch.zeros(2, dtype=torch.float64)),
                lambda: quasiparticle_ladder(eps, nocc, [8], torch.zeros(1, dtype=torch.float64))):
        with pytest.raises(ValueError, match="quasiparticle_ladder"):
            bad()


class _Untouchable:
    """a calculation whose state may not be looked at: every refusal below is raised from the arguments alone"""

    def __init__(self, qc):
        self._engine = qc._engine

    def __getattr__(self, name):
        raise AssertionError("bse looked at qc.%s before refusing" % name)


def test_refusals_before_anything_is_computed():
    qc = _Untouchable(_fake_qc())
    qc._engine.shape = (7, 7)
    for spin in ("quintet", None, "Singlet"):
        with pytest.raises(ValueError, match="spin"):
            bse(qc, spin=spin)
    for window in ((4,), (4, 4, 4), (-1, 4), (0, 0), (2.5, 1), 4, ("a", "b")):
        with pytest.raises(ValueError, match="window"):
            bse(qc, window=window)
    for qp in (torch.zeros(6, dtype=torch.float64), torch.zeros((7, 1), dtype=torch.float64), [0.0] * 8):
        with pytest.raises(ValueError, match="qp"):
            bse(qc, qp=qp)
    u = SimpleNamespace(u=torch.tensor([1.0, 0.0]), d=torch.tensor([1.0, 0.0]))
    with pytest.raises(NotImplementedError, match="unrestricted"):
        bse(_Untouchable(_fake_qc(weights=u, polarized=True)))
    # the references mp2 refuses are refused here too
    with pytest.raises(NotImplementedError, match="shard_over"):
        bse(_Untouchable(_fake_qc(sharded=True)))
    with pytest.raises(NotImplementedError, match="restricted open-shell"):
        bse(_Untouchable(_fake_qc(weights=torch.tensor([2.0, 2.0, 1.0]))))
