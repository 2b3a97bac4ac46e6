"""RI-MP2 on the host: the torch yardstick `pair_energies_reference` against a brute-force four-index einsum, closed forms, the
spin and scaling conventions of dqc_amd/mp2.py.  No GPU.

Bar 1e-12 per pair, relative to the sum of the magnitudes of the pair's terms sum_ab |V ... / D|: both sides are fp64 sums of the same
<= 17 * 17 terms over <= 7 auxiliary functions in different orders (round-off ~ 1e-15 of that sum); relative to the value itself the
same-spin sum, whose terms cancel, would have no fixed bar."""
from types import SimpleNamespace

import pytest
import torch

from dqc_amd.mp2 import MP2, _unsupported, components, energies_reference, pair_energies_reference


def _inputs(no, nv, naux, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn((no, naux, nv + pad), dtype=torch.float64, generator=g)
    eo = (-0.3 - torch.rand(no, dtype=torch.float64, generator=g) * 5.0).sort().values   # occupied: below -0.3, ascending
    ev = (0.2 + torch.rand(nv, dtype=torch.float64, generator=g) * 3.0).sort().values    # virtual: above 0.2, ascending
    return b, eo, ev


def _brute(bi, bj, eoi, eoj, eva, evb, same):
    """(pair_os, pair_ss, sum |os terms|, sum |ss terms|) from the explicit (noi, noj, nva, nvb) integrals"""
    v = torch.einsum("ipa,jpb->ijab", bi[:, :, :eva.numel()], bj[:, :, :evb.numel()])
    d = eoi[:, None, None, None] + eoj[None, :, None, None] - eva[None, None, :, None] - evb[None, None, None, :]
    t_os = v * v / d
    if not same:
        return t_os.sum((2, 3)), None, t_os.abs().sum((2, 3)), None
    t_ss = v * (v - v.transpose(2, 3)) / d
    a_ss = t_ss.abs().sum((2, 3))
    # i == j: V is symmetric and every same-spin term is zero analytically -- what t_ss holds there is the round-off of v - v^T, no
    # scale for an error: for these pairs the magnitudes of the two products each term is the difference of
    idx = torch.arange(v.shape[0])
    a_ss[idx, idx] = (v.abs() * (v.abs() + v.transpose(2, 3).abs()) / d.abs()).sum((2, 3))[idx, idx]
    return t_os.sum((2, 3)), t_ss.sum((2, 3)), t_os.abs().sum((2, 3)), a_ss


@pytest.mark.parametrize("no,nv,naux", [(1, 1, 1), (2, 3, 5), (3, 17, 7)])
def test_reference_against_brute_force_same_mode(no, nv, naux):
    b, eo, ev = _inputs(no, nv, naux, 100 + nv, pad=3)   # (three padding columns of noise: ignored)
    pos, pss = pair_energies_reference(b, b, eo, eo, ev, ev, True)
    ros, rss, aos, ass = _brute(b, b, eo, eo, ev, ev, True)
    worst = max(float(((pos - ros).abs() / aos).max()), float(((pss - rss).abs() / ass.clamp_min(1e-300)).max()))
    print("reference vs brute force (%d, %d, %d): worst |diff| / sum|terms| %.2e" % (no, nv, naux, worst))
    assert torch.all((pos - ros).abs() <= 1e-12 * aos) and torch.all((pss - rss).abs() <= 1e-12 * ass)
    assert float((pos - pos.t()).abs().max()) <= 1e-12 * float(aos.max())   # symmetric
    assert float((pss - pss.t()).abs().max()) <= 1e-12 * float(ass.max())
    assert float(pos.sum()) <= 0.0 and float(pss.sum()) <= 0.0   # every denominator is negative
    assert tuple(pos.shape) == (no, no) and tuple(pss.shape) == (no, no)


def test_reference_against_brute_force_opposite_mode():
    bi, eoi, eva = _inputs(2, 3, 6, 7)
    bj, eoj, evb = _inputs(1, 5, 6, 8, pad=2)
    pos, pss = pair_energies_reference(bi, bj, eoi, eoj, eva, evb, False)
    ros, _, aos, _ = _brute(bi, bj, eoi, eoj, eva, evb, False)
    assert pss is None and tuple(pos.shape) == (2, 1)
    assert torch.all((pos - ros).abs() <= 1e-12 * aos)
    assert float(pos.sum()) <= 0.0
    with pytest.raises(ValueError):
        pair_energies_reference(bi, bj, eoi, eoj, eva, evb, True)


def test_two_orbital_closed_form():
    """one occupied, one virtual orbital: e_os = -V^2 / (2 (eps_a - eps_i)), e_ss = 0 exactly"""
    b = torch.tensor([[[0.3], [-0.7], [0.2]]], dtype=torch.float64)   # (1, 3, 1)
    eo, ev = torch.tensor([-0.6], dtype=torch.float64), torch.tensor([0.45], dtype=torch.float64)
    v = float((b[0, :, 0] ** 2).sum())
    e_os, e_ss, pos, pss = energies_reference([(b, eo, ev)])
    assert abs(float(e_os) + v * v / (2 * (0.45 + 0.6))) <= 1e-15
    assert float(e_ss) == 0.0 and float(pss[0, 0]) == 0.0


def test_spin_consistency():
    """the same orbitals in both spin channels: e_ab = e_os(restricted), e_aa + e_bb = e_ss(restricted)"""
    b, eo, ev = _inputs(3, 6, 9, 31)
    ros, rss, _, _ = energies_reference([(b, eo, ev)])
    uos, uss, pos, pss = energies_reference([(b, eo, ev), (b.clone(), eo.clone(), ev.clone())])
    assert abs(float(uos - ros)) <= 1e-13 * abs(float(ros)) and abs(float(uss - rss)) <= 1e-13 * abs(float(ros))
    assert isinstance(pss, tuple) and torch.equal(pss[0], pss[1])
    # different channels: the alpha-beta matrix is rectangular and the same-spin parts differ
    b2, eo2, ev2 = _inputs(2, 7, 9, 32)
    uos, uss, pos, pss = energies_reference([(b, eo, ev), (b2, eo2, ev2)])
    assert tuple(pos.shape) == (3, 2) and tuple(pss[0].shape) == (3, 3) and tuple(pss[1].shape) == (2, 2)
    assert abs(float(uss) - float(pss[0].sum() + pss[1].sum())) <= 1e-15


def test_component_arithmetic_and_frozen_core():
    b, eo, ev = _inputs(4, 5, 8, 41)
    e_os, e_ss, pos, pss = energies_reference([(b, eo, ev)])
    e_scf = torch.tensor([-76.0], dtype=torch.float64)
    df = SimpleNamespace(_b=torch.zeros((8, 1, 1)))
    r = MP2(e_scf, e_os, e_ss, pos, pss, 1.0, 1.0, 0, df)
    assert float(r.e_corr) == float(e_os + e_ss) and float(r.e_tot) == float(e_scf + e_os + e_ss) and r.naux == 8
    scs = MP2(e_scf, e_os, e_ss, pos, pss, 1.2, 1.0 / 3.0, 0, df)
    assert abs(float(scs.e_corr) - (1.2 * float(e_os) + float(e_ss) / 3.0)) <= 1e-15
    assert abs(float(scs.e_tot) - (float(e_scf) + float(scs.e_corr))) <= 1e-13
    assert float(MP2(e_scf, e_os, e_ss, pos, pss, 0.0, 0.0, 0, df).e_tot) == float(e_scf)
    assert components(pos, pss, False)[0].shape == (1,)
    # frozen = k: the pair energies of the remaining orbitals do not change, so the energy is the sum over the trailing block
    for k in (1, 2, 4):
        fos, fss, fpos, fpss = energies_reference([(b, eo, ev)], frozen=k)
        sos, sss = pair_energies_reference(b[k:], b[k:], eo[k:], eo[k:], ev, ev, True)
        assert torch.equal(fpos, sos) and torch.equal(fpss, sss)
        assert abs(float(fos) - float(pos[k:, k:].sum())) <= 1e-13 * abs(float(e_os))
        assert abs(float(fss) - float(pss[k:, k:].sum())) <= 1e-13 * abs(float(e_os))
    assert float(energies_reference([(b, eo, ev)], frozen=4)[0]) == 0.0


def _fake_qc(sharded=False, method="coulomb", user_weights=None, weights=None, polarized=False):
    w = torch.tensor([2.0, 2.0]) if weights is None else weights
    ham = SimpleNamespace(sharded=sharded, df=SimpleNamespace(dfinfo=SimpleNamespace(method=method)))
    eng = SimpleNamespace(hamilton=ham, polarized=polarized, orb_weight=w, get_system=lambda: SimpleNamespace(_user_weights=user_weights))
    return SimpleNamespace(_engine=eng)


def test_refusals_each_with_its_own_message():
    """what a GPU-less machine can show of the refusals: the check reads the calculation's attributes only"""
    _unsupported(_fake_qc())
    with pytest.raises(NotImplementedError, match="shard_over"):
        _unsupported(_fake_qc(sharded=True))
    with pytest.raises(NotImplementedError, match="overlap"):
        _unsupported(_fake_qc(method="overlap"))
    with pytest.raises(NotImplementedError, match="user-given"):
        _unsupported(_fake_qc(user_weights=object()))
    with pytest.raises(NotImplementedError, match="restricted open-shell"):
        _unsupported(_fake_qc(weights=torch.tensor([2.0, 2.0, 1.0])))
    with pytest.raises(NotImplementedError, match="fractional"):
        _unsupported(_fake_qc(weights=torch.tensor([2.0, 0.5])))
    u = SimpleNamespace(u=torch.tensor([1.0]), d=torch.tensor([0.0]))   # (an empty spin-down channel keeps one empty orbital)
    _unsupported(_fake_qc(weights=u, polarized=True))
