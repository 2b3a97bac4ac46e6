"""RI-MP2 one-particle densities on the host: the torch yardstick `density_reference` (dqc_amd/mp2.py) against finite differences of
`pair_energies_reference`, its structural identities, and the refusals of `mp2_density`.  No GPU.

Diagonal against finite differences: with T = V / D at fixed V, e(eps) = sum_ij (c_os pair_os + c_ss pair_ss) and P_pp = d e / d eps_p.
Central differences with step h = 1e-4 carry a truncation error ~ h^2 e''' / 6; the step-2h estimate carries four times that, so
|FD(h) - FD(2h)| is three times the error of FD(h).  Bound: 10 x |FD(h) - FD(2h)| + 1e-10 (the round-off of a difference of two
energies of order one divided by 2e-4: ~1e-16 / 2e-4 = 5e-13, with margin)."""
from types import SimpleNamespace

import pytest
import torch

from dqc_amd.mp2 import density_reference, mp2_density, pair_energies_reference

NO, NV, NAUX = 3, 5, 7
SCALINGS = [(1.0, 1.0), (1.2, 1.0 / 3.0)]


def _inputs(seed=11, pad=0):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn((NO, NAUX, NV + pad), dtype=torch.float64, generator=g)
    eo = torch.tensor([-2.9, -1.7, -0.6], dtype=torch.float64) + 0.1 * torch.rand(NO, dtype=torch.float64, generator=g)
    ev = torch.tensor([0.3, 0.9, 1.6, 2.2, 3.1], dtype=torch.float64) + 0.1 * torch.rand(NV, dtype=torch.float64, generator=g)
    return b, eo, ev


def _energy(b, eo, ev, c_os, c_ss):
    pos, pss = pair_energies_reference(b, b, eo, eo, ev, ev, True)
    return float((c_os * pos + c_ss * pss).sum())


@pytest.mark.parametrize("c_os,c_ss", SCALINGS)
def test_diagonal_against_finite_differences(c_os, c_ss):
    b, eo, ev = _inputs()
    p_oo, p_vv, _ = density_reference(b, eo, ev, c_os, c_ss)
    h = 1e-4

    def fd(which, p, step):
        lo, hi = [eo.clone(), ev.clone()], [eo.clone(), ev.clone()]
        lo[which][p] -= step
        hi[which][p] += step
        return (_energy(b, hi[0], hi[1], c_os, c_ss) - _energy(b, lo[0], lo[1], c_os, c_ss)) / (2.0 * step)

    for which, mat, n in ((0, p_oo, NO), (1, p_vv, NV)):
        for p in range(n):
            f1, f2 = fd(which, p, h), fd(which, p, 2.0 * h)
            bound = 10.0 * abs(f1 - f2) + 1e-10
            print("c_os %.3g c_ss %.3g  %s %d: P %.12f  FD(h) %.12f  |P - FD| %.2e  bound %.2e" % (
                c_os, c_ss, "occ" if which == 0 else "vir", p, float(mat[p, p]), f1, abs(float(mat[p, p]) - f1), bound))
            assert abs(float(mat[p, p]) - f1) <= bound


@pytest.mark.parametrize("c_os,c_ss", SCALINGS)
def test_structure(c_os, c_ss):
    b, eo, ev = _inputs()
    p_oo, p_vv, gamma = density_reference(b, eo, ev, c_os, c_ss)
    assert tuple(p_oo.shape) == (NO, NO) and tuple(p_vv.shape) == (NV, NV) and tuple(gamma.shape) == (NO, NAUX, NV)
    scale = float(p_vv.trace())
    assert scale > 0.0 and abs(float(p_oo.trace() + p_vv.trace())) <= 1e-13 * scale
    assert torch.equal(p_oo, p_oo.t()) and torch.equal(p_vv, p_vv.t())
    e = _energy(b, eo, ev, c_os, c_ss)
    assert abs(float((gamma * b).sum()) - e) <= 1e-13 * abs(e)
    if (c_os, c_ss) == (1.0, 1.0):
        assert float(torch.linalg.eigvalsh(p_vv).min()) >= -1e-14 * scale
        assert float(torch.linalg.eigvalsh(p_oo).max()) <= 1e-14 * scale


def test_padding_columns_do_not_enter():
    b, eo, ev = _inputs()
    noisy = torch.cat([b, torch.randn((NO, NAUX, 11), dtype=torch.float64, generator=torch.Generator().manual_seed(5))], dim=2)
    for x, y in zip(density_reference(b, eo, ev, 1.2, 1.0 / 3.0), density_reference(noisy, eo, ev, 1.2, 1.0 / 3.0)):
        assert torch.equal(x, y)


def _fake_qc(polarized=False, is_ks=False):
    ham = SimpleNamespace(sharded=False, df=None)
    eng = SimpleNamespace(hamilton=ham, polarized=polarized, is_ks=is_ks, orb_weight=torch.tensor([2.0, 2.0, 0.0]),
                          get_system=lambda: SimpleNamespace(_user_weights=None))
    return SimpleNamespace(_engine=eng, _has_run=True)


def test_refusals_each_with_its_own_message():
    """what a GPU-less machine can show of the refusals: they read the calculation's attributes only, before any device work"""
    with pytest.raises(NotImplementedError, match="unrestricted"):
        mp2_density(_fake_qc(polarized=True))
    with pytest.raises(NotImplementedError, match="unrestricted"):
        mp2_density(_fake_qc(polarized=True), relaxed=False)
    with pytest.raises(NotImplementedError, match="frozen"):
        mp2_density(_fake_qc(), frozen=1)
    with pytest.raises(NotImplementedError, match="Kohn-Sham"):
        mp2_density(_fake_qc(is_ks=True))
    with pytest.raises(NotImplementedError, match="auxbasis="):
        mp2_density(_fake_qc())   # (no resident exact-integral tiles on this stand-in)
    with pytest.raises(ValueError):
        mp2_density(_fake_qc(), frozen=-1)
