"""G0W0 on the host: the torch yardsticks of dqc_amd/gw.py against brute force and against the closed (spectral) form, the Pade
continuation, the quasiparticle solver, the refusals.  No GPU.

Bars:
  * `screened_diag_reference` against the explicit (k, n, m, P, R) products: 1e-12 sum |terms| per element, both sides fp64 sums of
    the same <= 7 * 7 terms in different orders.
  * the identity W[k, n, m] = -sum_s (w^s_nm)^2 2 Om_s / (Om_s^2 + w_k^2) between the quadrature side (Q, its Cholesky factor, the
    contraction) and the closed form: 1e-12 of the largest element, restricted and unrestricted (measured 8e-16 and 1.4e-15 here) and on
    the one-occupied, one-virtual model, where Om = sqrt(D (D + 4 V)) is known by hand.
  * the self-energy on the imaginary axis against the closed form, synthetic spectra in the style of test_gpu_mp2._side -- occupied
    -20 ... -0.03, virtual 0.02 ... 5: gaps from 0.05 to 25 Ha, the two frontier orbitals 0.025 Ha from the Fermi level -- the tensor
    scaled (0.05) so that the HOMO shifts by 7e-3 Ha, less than the gap.  Worst error over every point of the defaults (0 and the
    nodes below 2 Ha) and every orbital, measured here (restricted / unrestricted alpha / unrestricted beta):

        nfreq   product integration (what `gw` uses)     the plain quadrature
           48   5.1e-10 / 6.8e-10 / 8.2e-10 Ha           3.5e-3 Ha
           64   3.0e-12 / 3.1e-12 / 4.6e-12 Ha           2.5e-3 Ha
          100   5.5e-15 / 5.0e-15 / 5.7e-16 Ha           1.3e-3 Ha          (largest |Sc| 9.8e-3 Ha)

    The plain quadrature sum_k wt_k W_k z / (z^2 + w_k^2) cannot resolve a kernel whose poles lie 0.025 Ha from the axis, at any
    sigma_wmax above 0.1 Ha; `self_energy_reference(..., scale=)` interpolates W alone and integrates its product with the kernel
    exactly, and is at the accuracy of the grid itself (test_rpa_cpu: 1.3e-10 relative at 48 points).  The bar is 10 x the worst
    measured value per grid -- 9e-9, 5e-11, 6e-14 Ha -- plus 1e-12 of the largest |Sc|, the round-off bar of W above carried through
    the (linear) frequency integral; at the defaults (100 points) the worst value, 5.5e-15 Ha, is far below the 1e-8 Ha asked for.
    On a spectrum whose orbitals all lie 0.5 Ha or more from the Fermi level both rules are at the closed form to 2e-16 Ha (asserted at 1e-11, the
    bar of the 100-point grid above with its round-off term).
  * `pade_thiele`: a sum of N = 4 poles from 2 N = 8 points on the imaginary axis is a rational function of degrees (3, 4), which
    8 points determine: recovered at real arguments inside the gap to 2.3e-13 relative here (value and derivative); bar 1e-10, for the
    conditioning of the continued fraction on another machine's round-off.
  * the quasiparticle solver on that function: the Newton solution and the linearised one against their definitions evaluated on the
    exact function, 1e-10 Ha."""
import math

import pytest
import torch

import dqc_amd
from dqc_amd.gw import (correlation_part, pade_thiele, quasiparticle_solve, screened_diag_reference, self_energy_reference, sigma_points,
                        spectral_reference)
from dqc_amd.rpa import frequency_grid, response_reference
from tests.test_mp2_cpu import _fake_qc, _inputs

SIGMA_MEASURED = {48: 8.2e-10, 64: 4.6e-12, 100: 5.5e-15}   # module docstring
SIGMA_BAR = {48: 9e-9, 64: 5e-11, 100: 6e-14}


def _spectrum(no, nv, naux, seed, amp, side=True):
    """(bnm (nmo, naux, nmo + 3: three padding columns of noise), bov (no, naux, nv), eps): one symmetric tensor B[P, p, q] over all
    orbitals; side=True: the energies of test_gpu_mp2._side, else those of test_mp2_cpu._inputs"""
    g = torch.Generator().manual_seed(seed)
    nmo = no + nv
    bf = torch.randn((naux, nmo, nmo), dtype=torch.float64, generator=g) * amp
    bf = 0.5 * (bf + bf.transpose(1, 2))
    if side:
        eo = torch.linspace(-20.0, -0.03, no, dtype=torch.float64) if no > 1 else torch.full((no,), -0.03, dtype=torch.float64)
        ev = torch.linspace(0.02, 5.0, nv, dtype=torch.float64) if nv > 1 else torch.full((nv,), 0.02, dtype=torch.float64)
    else:
        _, eo, ev = _inputs(no, nv, 1, seed)
    bov = bf[:, :no, no:].permute(1, 0, 2).contiguous()
    bnm = torch.cat([bf.permute(1, 0, 2), torch.randn((nmo, naux, 3), dtype=torch.float64, generator=g)], dim=2).contiguous()
    return bnm, bov, torch.cat([eo, ev])


def _fermi(spins):
    return 0.5 * (max(float(e[b.shape[0] - 1]) for _, b, e in spins) + min(float(e[b.shape[0]]) for _, b, e in spins))


def _screened(spins, freqs):
    """per spin W (nfreq, nmo, nmo) by the quadrature route: Q of both spins, Wc, the contraction"""
    scale = 4.0 if len(spins) == 1 else 2.0
    q = sum(response_reference(bov, e[:bov.shape[0]], e[bov.shape[0]:], freqs, scale) for _, bov, e in spins)
    wc = correlation_part(q)
    return [screened_diag_reference(wc, bnm, e.numel()) for bnm, _, e in spins]


def _pair(amp, side):
    a, b = _spectrum(3, 6, 24, 5, amp, side), _spectrum(2, 7, 24, 6, amp, side)
    return [a, (b[0], b[1], b[2] * 1.1 + 0.001)]


@pytest.mark.parametrize("nfreq,ntarget,nm,naux", [(1, 1, 1, 1), (2, 2, 3, 5), (3, 3, 7, 7)])
def test_screened_diag_reference_against_brute_force(nfreq, ntarget, nm, naux):
    g = torch.Generator().manual_seed(400 + naux)
    bn = torch.randn((ntarget, naux, nm + 3), dtype=torch.float64, generator=g)   # (three padding columns of noise: ignored)
    wc = torch.randn((nfreq, naux, naux), dtype=torch.float64, generator=g)
    wc = 0.5 * (wc + wc.transpose(1, 2))
    t = torch.einsum("npm,kpr,nrm->knmpr", bn[:, :, :nm], wc, bn[:, :, :nm])
    ref, mag = t.sum((3, 4)), t.abs().sum((3, 4))
    w = screened_diag_reference(wc, bn, nm)
    print("screened_diag_reference vs brute force (%d, %d, %d, %d): worst |diff| / sum|terms| %.2e" % (nfreq, ntarget, nm, naux,
                                                                                                    float(((w - ref).abs() / mag).max())))
    assert tuple(w.shape) == (nfreq, ntarget, nm)
    assert torch.all((w - ref).abs() <= 1e-12 * mag)


@pytest.mark.parametrize("polarized", [False, True])
def test_screened_interaction_identity(polarized):
    """the quadrature route and the closed form give the same W at every frequency: every factor of both"""
    spins = _pair(0.3, False) if polarized else [_spectrum(3, 6, 24, 5, 0.3, False)]
    f = torch.tensor([0.0, 0.05, 0.7, 3.0, 60.0], dtype=torch.float64)
    sp = spectral_reference(spins)
    assert bool(torch.all(sp.omega > 0)) and sp.omega.numel() == sum(b.shape[0] * (e.numel() - b.shape[0]) for _, b, e in spins)
    for s, w in enumerate(_screened(spins, f)):
        ref = sp.screened(s, f)
        err = float((w - ref).abs().max() / ref.abs().max())
        print("W identity, %s spin %d: worst |diff| / largest element %.2e" % ("unrestricted" if polarized else "restricted", s, err))
        assert bool(torch.all(ref <= 0.0)) and err <= 1e-12


def test_two_orbital_model():
    """one occupied, one virtual orbital, V = (ia|ia): Om = sqrt(D (D + 4 V)), (X + Y) = sqrt(D / Om), w_nm = sqrt 2 (nm|ia) (X + Y)"""
    g = torch.Generator().manual_seed(3)
    bf = torch.randn((3, 2, 2), dtype=torch.float64, generator=g)
    bf = 0.5 * (bf + bf.transpose(1, 2))
    eps = torch.tensor([-0.6, 0.45], dtype=torch.float64)
    bnm, bov = bf.permute(1, 0, 2).contiguous(), bf[:, :1, 1:].permute(1, 0, 2).contiguous()
    d, v = 1.05, float((bf[:, 0, 1] ** 2).sum())
    om = math.sqrt(d * (d + 4.0 * v))
    sp = spectral_reference([(bnm, bov, eps)])
    assert abs(float(sp.omega[0]) - om) <= 1e-14
    wnm = math.sqrt(2.0 * d / om) * torch.einsum("pnm,p->nm", bf, bf[:, 0, 1])
    assert float((sp.w[0][0].abs() - wnm.abs()).abs().max()) <= 1e-14      # (the sign of an eigenvector is free)
    f = torch.tensor([0.0, 0.4, 7.0], dtype=torch.float64)
    ref = -(wnm ** 2)[None] * (2.0 * om / (om * om + f * f))[:, None, None]
    w = _screened([(bnm, bov, eps)], f)[0]
    assert float((w - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # and the self-energy of the model at one imaginary point, by hand
    z = -0.075 + 0.3j
    sc = wnm[:, 0] ** 2 / (z - eps[0] + om) + wnm[:, 1] ** 2 / (z - eps[1] - om)
    assert float((sp.sigma_c(0, torch.tensor([z], dtype=torch.complex128))[:, 0] - sc).abs().max()) <= 1e-14


@pytest.mark.parametrize("polarized", [False, True])
def test_self_energy_against_the_closed_form(polarized):
    spins = _pair(0.05, True) if polarized else [_spectrum(3, 6, 24, 5, 0.05, True)]
    sp = spectral_reference(spins)
    ef = _fermi(spins)
    assert abs(ef + 0.005) < 1e-3                                       # the frontier orbitals lie 0.025 Ha from it
    for nfreq in (48, 64, 100):
        f, wt = frequency_grid(nfreq, 1.0)
        pts = sigma_points(f, 2.0)
        assert float(pts[0]) == 0.0 and float(pts.max()) < 2.0 and pts.numel() == 1 + int((f < 2.0).sum())
        for s, w in enumerate(_screened(spins, f)):
            eps = spins[s][2]
            exact = sp.sigma_c(s, ef + 1j * pts)
            sc = self_energy_reference(w, eps, ef, f, wt, pts, scale=1.0)
            plain = self_energy_reference(w, eps, ef, f, wt, pts)
            err, big = float((sc - exact).abs().max()), float(exact.abs().max())
            print("Sc(iw), %s spin %d, nfreq %d, %d points: worst error %.2e Ha (bar %.1e + 1e-12 * %.2e); plain quadrature %.2e Ha"
                  % ("unrestricted" if polarized else "restricted", s, nfreq, pts.numel(), err, SIGMA_BAR[nfreq], big,
                     float((plain - exact).abs().max())))
            assert tuple(sc.shape) == (eps.numel(), pts.numel()) and sc.dtype == torch.complex128
            assert SIGMA_BAR[nfreq] <= 11.0 * SIGMA_MEASURED[nfreq] and SIGMA_MEASURED[100] <= 1e-8
            assert err <= SIGMA_BAR[nfreq] + 1e-12 * big
    # the HOMO moves by less than the gap (the quasiparticle equation keeps a root next to eps)
    shift = float(sp.sigma_c(0, spins[0][2][2:3].to(torch.complex128))[2, 0].real)
    assert abs(shift) < 0.05


def test_plain_quadrature_on_a_wide_gap():
    """every orbital 0.5 Ha or more from the Fermi level: the plain rule (the formula as it is written) resolves its kernel, and the
    product rule gives the same numbers"""
    bnm, bov, eps = _spectrum(3, 6, 24, 5, 0.1, False)
    eps = torch.where(eps < 0, eps - 0.3, eps + 0.4)
    spins = [(bnm, bov, eps)]
    ef = _fermi(spins)
    assert float((eps - ef).abs().min()) >= 0.5
    f, wt = frequency_grid(100, 1.0)
    pts = sigma_points(f, 2.0)
    w = _screened(spins, f)[0]
    exact = spectral_reference(spins).sigma_c(0, ef + 1j * pts)
    plain, prod = self_energy_reference(w, eps, ef, f, wt, pts), self_energy_reference(w, eps, ef, f, wt, pts, scale=1.0)
    # the formula itself, term by term
    z = (ef - eps)[None, :] + 1j * pts[:, None]
    brute = -(1.0 / math.pi) * torch.einsum("k,knm,jkm->nj", wt.to(torch.complex128), w.to(torch.complex128),
                                            z[:, None, :] / (z[:, None, :] ** 2 + (f ** 2)[None, :, None]))
    print("wide gap: plain - closed form %.2e  product - closed form %.2e  plain - brute force %.2e Ha" % (
        float((plain - exact).abs().max()), float((prod - exact).abs().max()), float((plain - brute).abs().max())))
    assert float((plain - brute).abs().max()) <= 1e-14
    assert float((plain - exact).abs().max()) <= 1e-11 and float((prod - exact).abs().max()) <= 1e-11


def _poles():
    """a self-energy-like function with N = 4 poles outside the gap (-0.4, 0.5) (arguments measured from ef = 0)"""
    res = torch.tensor([[0.02, 0.05, 0.03, 0.01], [0.04, 0.01, 0.02, 0.06]], dtype=torch.float64)
    pos = torch.tensor([[-1.3, -0.6, 0.8, 1.9], [-2.0, -0.9, 0.7, 1.1]], dtype=torch.float64)

    def fcn(x, derivative=False):
        x = torch.as_tensor(x).to(torch.complex128)
        den = x[..., None] - pos[:, None, :]
        val = (res[:, None, :] / den).sum(-1)
        return (val, -(res[:, None, :] / (den * den)).sum(-1)) if derivative else val
    return fcn


def test_pade_recovers_a_sum_of_poles():
    fcn = _poles()
    z = 1j * torch.tensor([0.0, 0.1, 0.25, 0.45, 0.7, 1.0, 1.4, 1.9], dtype=torch.float64)
    p = pade_thiele(z, fcn(z[None, :].expand(2, -1)))
    x = torch.linspace(-0.35, 0.45, 9, dtype=torch.float64)[None, :].expand(2, -1)
    (v, dv), (ev, edv) = p(x, derivative=True), fcn(x, derivative=True)
    err, derr = float(((v - ev).abs() / ev.abs()).max()), float(((dv - edv).abs() / edv.abs()).max())
    print("pade_thiele, 4 poles from 8 points, real arguments inside the gap: worst relative error %.2e (derivative %.2e)" % (err, derr))
    assert err <= 1e-10 and derr <= 1e-10
    assert float((p(z[None, :].expand(2, -1)) - fcn(z[None, :].expand(2, -1))).abs().max()) <= 1e-14   # it interpolates
    assert abs(complex(pade_thiele(z, fcn(z[None, :].expand(2, -1))[0])(0.2)) - complex(fcn(torch.tensor([[0.2], [0.2]]))[0, 0])) <= 1e-12
    with pytest.raises(ValueError):
        pade_thiele(z, torch.zeros(3, dtype=torch.complex128))


def test_quasiparticle_solver():
    fcn = _poles()
    z = 1j * torch.tensor([0.0, 0.1, 0.25, 0.45, 0.7, 1.0, 1.4, 1.9], dtype=torch.float64)
    p = pade_thiele(z, fcn(z[None, :].expand(2, -1)))
    ef = -0.1
    eps, f_hf = torch.tensor([-0.3, 0.25], dtype=torch.float64), torch.tensor([-0.33, 0.29], dtype=torch.float64)
    e, zf, ok = quasiparticle_solve(p, eps, f_hf, ef)
    resid = e - f_hf - torch.diagonal(fcn((e - ef)[None, :].expand(2, -1))).real
    s0, d0 = (torch.diagonal(t) for t in fcn((eps - ef)[None, :].expand(2, -1), derivative=True))
    z_exact = 1.0 / (1.0 - d0.real)
    lin, zl, okl = quasiparticle_solve(p, eps, f_hf, ef, linearized=True)
    lin_exact = eps + z_exact * (f_hf - eps + s0.real)
    print("quasiparticle solver: residual of the Newton solution on the exact function %.2e  linearised - exact %.2e  Z %s" % (
        float(resid.abs().max()), float((lin - lin_exact).abs().max()), zf.tolist()))
    assert bool(ok.all()) and bool(okl.all())
    assert float(resid.abs().max()) <= 1e-10 and float((lin - lin_exact).abs().max()) <= 1e-10
    assert float((zf - z_exact).abs().max()) <= 1e-10 and torch.equal(zf, zl)
    assert bool(torch.all((zf > 0) & (zf < 1)))
    assert float((e - lin).abs().max()) < 1e-2 and float((e - eps).abs().min()) > 1e-3     # two different, nearby answers


def test_refusals_and_argument_checks():
    """the refusals of mp2 pass through gw (the check reads the calculation's attributes only); bad arguments are refused first"""
    assert dqc_amd.gw.screened_diag_reference is screened_diag_reference and dqc_amd.gw.self_energy_reference is self_energy_reference
    assert dqc_amd.gw.pade_thiele is pade_thiele and dqc_amd.gw.spectral_reference is spectral_reference
    assert dqc_amd.GW.__name__ == "GW"
    assert "NOT for core states" in dqc_amd.gw.__doc__
    with pytest.raises(NotImplementedError, match="shard_over"):
        dqc_amd.gw(_fake_qc(sharded=True))
    with pytest.raises(NotImplementedError, match="overlap"):
        dqc_amd.gw(_fake_qc(method="overlap"))
    with pytest.raises(NotImplementedError, match="user-given"):
        dqc_amd.gw(_fake_qc(user_weights=object()))
    with pytest.raises(NotImplementedError, match="restricted open-shell"):
        dqc_amd.gw(_fake_qc(weights=torch.tensor([2.0, 2.0, 1.0])))
    with pytest.raises(NotImplementedError, match="fractional"):
        dqc_amd.gw(_fake_qc(weights=torch.tensor([2.0, 0.5])))
    with pytest.raises(ValueError, match="nfreq"):
        dqc_amd.gw(_fake_qc(), nfreq=0)
    with pytest.raises(ValueError, match="freq_scale"):
        dqc_amd.gw(_fake_qc(), freq_scale=0.0)
    with pytest.raises(ValueError, match="sigma_wmax"):
        dqc_amd.gw(_fake_qc(), sigma_wmax=0.0)
    with pytest.raises(ValueError, match="orbs"):
        dqc_amd.gw(_fake_qc(), orbs=[-1])
    with pytest.raises(ValueError, match="orbs"):
        dqc_amd.gw(_fake_qc(), orbs=[])
    with pytest.raises(ValueError, match="orbs"):
        dqc_amd.gw(_fake_qc(), orbs=[1, 1])
    qc = _fake_qc()
    qc._engine.shape = (13, 13)
    with pytest.raises(ValueError, match="orbs"):
        dqc_amd.gw(qc, orbs=[3, 13])
