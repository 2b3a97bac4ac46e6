"""RI-dRPA on the host: the frequency grid, the torch yardsticks of dqc_amd/rpa.py against a brute-force einsum and against the
closed form (plasmon formula), the spin conventions, the refusals.  No GPU.

Bars:
  * the grid: sum_k w_k g_D(w_k) g_D'(w_k) against pi / (2 (D + D')) for D, D' in {0.05, 0.3, 5, 25}.  Measured here with the default
    grid (48 points, scale 1): worst relative error 1.28e-10 (at D = D' = 25; a scan of 40 x 40 gaps between 0.05 and 25 has the same
    worst case; 32 points: 5.8e-7, 64 points: 2e-14).  The bar is 10 x that: GRID48_BAR = 1.3e-9 relative.
  * the response: 1e-12 sum |terms| per element, both sides fp64 sums of the same <= 3 * 17 terms in different orders.
  * energies at 96 points against the closed form in 40-digit arithmetic: 1e-10 relative (the grid itself is at round-off there:
    2e-14).
  * energies at the default grid: GRID48_BAR relative to the second-order energy -- e_corr_2nd is a sum of same-signed terms
    V^2 int g g, each integrated to GRID48_BAR relative, and |ln(1 + x) - x| <= x^2 / 2 bounds the RPA integrand by the second-order
    one (|e_corr| <= |e_dmp2|), whose quadrature error it tracks.
  * identical spins: 1e-12 relative (the same sums, doubled)."""
import math

import pytest
import torch

import dqc_amd
from dqc_amd.mp2 import pair_energies_reference
from dqc_amd.rpa import dmp2_from_pairs, energy_from_response, frequency_grid, plasmon_reference, response_reference
from tests.test_mp2_cpu import _fake_qc, _inputs

GRID48_BAR = 1.3e-9   # module docstring
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 17, 7)]


def test_frequency_grid_integrates_the_pair_kernel():
    f, w = frequency_grid(48, 1.0)
    assert f.dtype == torch.float64 and tuple(f.shape) == (48,) and bool(torch.all(f > 0)) and bool(torch.all(w > 0))
    assert bool(torch.all(f[1:] > f[:-1]))
    worst = 0.0
    for d1 in (0.05, 0.3, 5.0, 25.0):
        for d2 in (0.05, 0.3, 5.0, 25.0):
            v = float((w * (d1 / (d1 * d1 + f * f)) * (d2 / (d2 * d2 + f * f))).sum())
            exact = math.pi / (2.0 * (d1 + d2))
            worst = max(worst, abs(v - exact) / exact)
    print("frequency_grid(48, 1): worst relative error of int g g %.3e (bar %.1e)" % (worst, GRID48_BAR))
    assert worst <= GRID48_BAR
    f2, w2 = frequency_grid(5, 2.0)   # the scale maps points and weights alike
    f1, w1 = frequency_grid(5, 1.0)
    assert torch.allclose(f2, 2.0 * f1, rtol=1e-15) and torch.allclose(w2, 2.0 * w1, rtol=1e-15)
    with pytest.raises(ValueError):
        frequency_grid(0)
    with pytest.raises(ValueError):
        frequency_grid(4, 0.0)


def _brute(b, eo, ev, freq, scale):
    """(Q, sum |terms|) from the explicit (nfreq, i, a, P, R) products"""
    bb = b[:, :, :ev.numel()]
    d = ev[None, :] - eo[:, None]
    g = d[None] / (d[None] ** 2 + freq[:, None, None] ** 2)
    t = scale * torch.einsum("ipa,kia,ira->kiapr", bb, g, bb)
    return t.sum((1, 2)), t.abs().sum((1, 2))


@pytest.mark.parametrize("no,nv,naux", SHAPES)
def test_response_reference_against_brute_force(no, nv, naux):
    b, eo, ev = _inputs(no, nv, naux, 200 + nv, pad=3)   # (three padding columns of noise: ignored)
    freq = torch.tensor([0.0, 0.3, 2.0, 40.0], dtype=torch.float64)
    q = response_reference(b, eo, ev, freq, 4.0)
    ref, mag = _brute(b, eo, ev, freq, 4.0)
    print("response_reference vs brute force (%d, %d, %d): worst |diff| / sum|terms| %.2e" % (no, nv, naux, float(((q - ref).abs() / mag).max())))
    assert tuple(q.shape) == (4, naux, naux)
    assert torch.all((q - ref).abs() <= 1e-12 * mag)
    assert float((q - q.transpose(1, 2)).abs().max()) <= 1e-12 * float(mag.max())
    assert bool(torch.all(torch.linalg.eigvalsh(q) >= -1e-12 * float(mag.max())))   # positive semidefinite


@pytest.mark.parametrize("no,nv,naux", SHAPES)
def test_energies_against_the_closed_forms(no, nv, naux):
    b, eo, ev = _inputs(no, nv, naux, 300 + nv, pad=2)
    exact = float(plasmon_reference([(b, eo, ev)], digits=40))   # (fp64: 1e-16 absolute, the whole energy of the smallest case)
    dmp2 = float(dmp2_from_pairs(pair_energies_reference(b, b, eo, eo, ev, ev, True)[0]))
    assert dmp2 < 0.0 and exact < 0.0 and abs(exact) < abs(dmp2)   # ln(1 + x) - x >= -x^2 / 2
    for nfreq, bar_rpa, bar_2nd in ((96, 1e-10 * abs(exact), 1e-10 * abs(dmp2)), (48, GRID48_BAR * abs(dmp2), GRID48_BAR * abs(dmp2))):
        f, w = frequency_grid(nfreq, 1.0)
        q = response_reference(b, eo, ev, f, 4.0)
        e, e2, integrand = energy_from_response(q, w)
        print("(%d, %d, %d) nfreq %d: e_corr %.12f (closed form diff %.2e, bar %.1e)  e_corr_2nd %.12f (analytic diff %.2e, bar %.1e)"
              % (no, nv, naux, nfreq, float(e), float(e) - exact, bar_rpa, float(e2), float(e2) - dmp2, bar_2nd))
        assert tuple(integrand.shape) == (nfreq,)
        assert abs(float(e) - exact) <= bar_rpa
        assert abs(float(e2) - dmp2) <= bar_2nd


def test_two_orbital_closed_form():
    """one occupied, one virtual orbital, V = (ia|ia): W = sqrt(D (D + 4 V)), e_corr = (W - D - 2 V) / 2"""
    b = torch.tensor([[[0.3], [-0.7], [0.2]]], dtype=torch.float64)
    eo, ev = torch.tensor([-0.6], dtype=torch.float64), torch.tensor([0.45], dtype=torch.float64)
    v, d = float((b[0, :, 0] ** 2).sum()), 1.05
    assert abs(float(plasmon_reference([(b, eo, ev)])) - 0.5 * (math.sqrt(d * (d + 4 * v)) - d - 2 * v)) <= 1e-15


def test_spin_forms():
    b, eo, ev = _inputs(3, 6, 9, 31)
    f, w = frequency_grid(96, 1.0)
    r, r2, _ = energy_from_response(response_reference(b, eo, ev, f, 4.0), w)
    # identical spins: Q = 2 (Q_a + Q_b) is the restricted Q; the spin-orbital closed form is the singlet one (the triplet block has no K)
    q = response_reference(b, eo, ev, f, 2.0) + response_reference(b.clone(), eo.clone(), ev.clone(), f, 2.0)
    u, u2, _ = energy_from_response(q, w)
    assert abs(float(u - r)) <= 1e-12 * abs(float(r)) and abs(float(u2 - r2)) <= 1e-12 * abs(float(r2))
    same = [(b, eo, ev), (b.clone(), eo.clone(), ev.clone())]
    assert abs(float(plasmon_reference(same)) - float(plasmon_reference(same[:1]))) <= 1e-12 * abs(float(r))
    os_r = pair_energies_reference(b, b, eo, eo, ev, ev, True)[0]
    assert abs(float(dmp2_from_pairs((os_r, os_r), os_r)) - float(dmp2_from_pairs(os_r))) <= 1e-12 * abs(float(r2))
    # different spins: the spin-orbital closed form, and the second-order term from the three pair matrices
    b2, eo2, ev2 = _inputs(2, 7, 9, 32)
    q = response_reference(b, eo, ev, f, 2.0) + response_reference(b2, eo2, ev2, f, 2.0)
    u, u2, _ = energy_from_response(q, w)
    exact = float(plasmon_reference([(b, eo, ev), (b2, eo2, ev2)]))
    os_ab = pair_energies_reference(b, b2, eo, eo2, ev, ev2, False)[0]
    os_bb = pair_energies_reference(b2, b2, eo2, eo2, ev2, ev2, True)[0]
    dmp2 = float(dmp2_from_pairs((os_r, os_bb), os_ab))
    print("two spins: e_corr %.12f (closed form diff %.2e)  e_corr_2nd %.12f (analytic diff %.2e)" % (float(u), float(u) - exact, float(u2),
                                                                                                 float(u2) - dmp2))
    assert abs(float(u) - exact) <= 1e-10 * abs(exact) and abs(float(u2) - dmp2) <= 1e-10 * abs(dmp2)
    # frozen orbitals are dropped from the closed form
    assert abs(float(plasmon_reference([(b, eo, ev)], frozen=1)) - float(plasmon_reference([(b[1:], eo[1:], ev)]))) == 0.0
    assert float(plasmon_reference([(b, eo, ev)], frozen=3)) == 0.0


def test_dense_integrals_in_place_of_the_tensor():
    b, eo, ev = _inputs(2, 3, 5, 77)
    v = torch.einsum("ipa,jpb->iajb", b, b)
    assert abs(float(plasmon_reference([(v, eo, ev)])) - float(plasmon_reference([(b, eo, ev)]))) <= 1e-13


def test_closed_form_in_extended_precision():
    """digits=40: the same closed form in 40-digit arithmetic; the fp64 one agrees to its own round-off, 1e-15 of the sums it is the
    difference of (sum D + 2 tr K), one and two spins"""
    b, eo, ev = _inputs(3, 6, 9, 31)
    b2, eo2, ev2 = _inputs(2, 7, 9, 32)
    for spins in ([(b, eo, ev)], [(b, eo, ev), (b2, eo2, ev2)]):
        scale = sum(float((v[None, :] - o[:, None]).sum() + 2.0 * (t[:, :, :v.numel()] ** 2).sum()) for t, o, v in spins)
        e64, e40 = float(plasmon_reference(spins)), float(plasmon_reference(spins, digits=40))
        print("closed form fp64 - 40 digits: %.2e (sums of %.1f)" % (e64 - e40, scale))
        assert abs(e64 - e40) <= 1e-14 * scale


def test_refusals_and_argument_checks():
    """the refusals of mp2 pass through rpa (the check reads the calculation's attributes only); bad arguments are refused first"""
    assert dqc_amd.rpa.response_reference is response_reference and dqc_amd.rpa.plasmon_reference is plasmon_reference
    assert dqc_amd.rpa.frequency_grid is frequency_grid and dqc_amd.rpa.energy_from_response is energy_from_response
    assert dqc_amd.RPA.__name__ == "RPA"
    with pytest.raises(NotImplementedError, match="shard_over"):
        dqc_amd.rpa(_fake_qc(sharded=True))
    with pytest.raises(NotImplementedError, match="overlap"):
        dqc_amd.rpa(_fake_qc(method="overlap"))
    with pytest.raises(NotImplementedError, match="user-given"):
        dqc_amd.rpa(_fake_qc(user_weights=object()))
    with pytest.raises(NotImplementedError, match="restricted open-shell"):
        dqc_amd.rpa(_fake_qc(weights=torch.tensor([2.0, 2.0, 1.0])))
    with pytest.raises(NotImplementedError, match="fractional"):
        dqc_amd.rpa(_fake_qc(weights=torch.tensor([2.0, 0.5])))
    with pytest.raises(ValueError, match="frozen"):
        dqc_amd.rpa(_fake_qc(), frozen=-1)
    with pytest.raises(ValueError, match="nfreq"):
        dqc_amd.rpa(_fake_qc(), nfreq=0)
    with pytest.raises(ValueError, match="freq_scale"):
        dqc_amd.rpa(_fake_qc(), freq_scale=0.0)
