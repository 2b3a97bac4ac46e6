"""CPU tests of the host-side pieces of the basis-parameter gradient (dqc_amd.gradient.basis_gradient): the primitive-row <->
shell map of make_tables, the per-primitive companion table, and the chain from the table's rows (exponent, normalised
coefficient) to the caller's CGTOBasis tensors through wfnormalize_."""
import numpy as np
import torch

from dqc_amd.basis import companion_tables, make_tables, primitive_rows, table_parameters
from dqc_amd.utils.datastruct import AtomCGTOBasis, CGTOBasis

_SHELLS = [[(0, [4.0, 0.9, 0.3], [0.5, 0.6, 0.2]), (2, [1.1], [1.0]), (1, [1.3, 0.5], [0.6, 0.5])],
           [(1, [1.7, 0.45], [0.6, 0.5]), (3, [0.9, 0.4], [1.0, 0.3])]]


def _t(x, grad=False):
    return torch.tensor(x, dtype=torch.float64, requires_grad=grad)


def _atombases(grad=False):
    return [AtomCGTOBasis(atomz=z, bases=[CGTOBasis(l, _t(a, grad), _t(c, grad)) for l, a, c in sh], pos=_t(p))
            for z, sh, p in zip((8, 1), _SHELLS, ([0.0, 0.0, 0.0], [0.0, 0.0, 1.8]))]


def test_primitive_rows_follow_the_table_shell_by_shell():
    atm, bas, env, _ = make_tables(_atombases())
    prim_shell, shell_off = primitive_rows(bas)
    assert prim_shell.tolist() == [0, 0, 0, 1, 2, 2, 3, 3, 4, 4]
    assert shell_off.tolist() == [0, 3, 4, 6, 8, 10]
    flat = [a for sh in _SHELLS for _, al, _ in sh for a in al]
    for row, ish in enumerate(prim_shell):
        k = row - shell_off[ish]
        assert 0 <= k < bas[ish, 2]
        assert env[bas[ish, 5] + k] == flat[row]  # the row's exponent is primitive k of its shell


def test_companion_table_lists_every_primitive_twice():
    atm, bas, env, _ = make_tables(_atombases())
    prim_shell, shell_off = primitive_rows(bas)
    catm, cbas, cenv = companion_tables(atm, bas, env)
    P = len(prim_shell)
    assert cbas.shape == (2 * P, 8) and np.array_equal(catm, atm)
    assert np.array_equal(cenv[:len(env)], env)  # the original entries stay where the atoms point
    for up in (0, 1):
        for row, ish in enumerate(prim_shell):
            c = cbas[up * P + row]
            k = row - shell_off[ish]
            assert c[0] == bas[ish, 0] and c[1] == bas[ish, 1] + 2 * up and c[2] == 1 and c[3] == 1
            assert cenv[c[5]] == env[bas[ish, 5] + k]
            assert cenv[c[6]] == (-env[bas[ish, 6] + k] if up else 1.0)


def _normalised(l, a, c):
    return CGTOBasis(l, a, c).wfnormalize_().coeffs


def test_table_parameters_are_the_table_rows_and_chain_through_the_normalisation():
    abs_ = _atombases(grad=True)
    shells = [(sh.angmom, sh.alphas, sh.coeffs, sh.normalized) for ab in abs_ for sh in ab.bases]
    atm, bas, env, _ = make_tables(abs_)  # (normalises the shells in place; `shells` keeps the caller's tensors)
    al, co = table_parameters(shells)
    prim_shell, shell_off = primitive_rows(bas)
    assert np.array_equal(al.detach().numpy(), np.concatenate([env[b[5]:b[5] + b[2]] for b in bas]))
    assert np.array_equal(co.detach().numpy(), np.concatenate([env[b[6]:b[6] + b[2]] for b in bas]))
    rng = np.random.default_rng(0)
    g = _t(rng.standard_normal((len(prim_shell), 2)))
    leaves = [t for _, a, c, _ in shells for t in (a, c)]
    got = torch.autograd.grad((g[:, 0] * al).sum() + (g[:, 1] * co).sum(), leaves)
    for ish, (l, a, c, _) in enumerate(shells):
        gs = g[shell_off[ish]:shell_off[ish + 1]]
        a2, c2 = a.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
        ra, rc = torch.autograd.grad((gs[:, 0] * a2).sum() + (gs[:, 1] * _normalised(l, a2, c2)).sum(), (a2, c2))
        assert torch.allclose(got[2 * ish], ra, rtol=1e-13, atol=0) and torch.allclose(got[2 * ish + 1], rc, rtol=1e-13, atol=0)
        # the normalisation alone against finite differences
        assert torch.autograd.gradcheck(lambda x, y: _normalised(l, x, y), (a2, c2))


def test_a_shell_normalised_by_an_earlier_table_keeps_the_callers_coefficients():
    sh = CGTOBasis(1, _t([1.3, 0.5], True), _t([0.6, 0.5], True))
    raw = sh.coeffs
    make_tables([AtomCGTOBasis(atomz=1, bases=[sh], pos=_t([0.0, 0.0, 0.0]))])
    assert sh.normalized and sh._raw_coeffs is raw
    al, co = table_parameters([(1, sh.alphas, sh._raw_coeffs, False)])
    assert torch.equal(co.detach(), sh.coeffs.detach())


def test_shared_tensors_accumulate():
    a, c = _t([1.3, 0.5], True), _t([0.6, 0.5], True)
    shells = [(0, a, c, False), (0, a, c, False)]
    al, co = table_parameters(shells)
    g = _t(np.random.default_rng(1).standard_normal((4, 2)))
    ga, gc = torch.autograd.grad((g[:, 0] * al).sum() + (g[:, 1] * co).sum(), (a, c))
    one_a, one_c = table_parameters(shells[:1])
    ha, hc = torch.autograd.grad(((g[:2, 0] + g[2:, 0]) * one_a).sum() + ((g[:2, 1] + g[2:, 1]) * one_c).sum(), (a, c))
    assert torch.allclose(ga, ha, rtol=1e-14, atol=0) and torch.allclose(gc, hc, rtol=1e-14, atol=0)
