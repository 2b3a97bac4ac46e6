"""CPU tests (no GPU) of the CIS / TDHF excited-state gradient: the gates dqc_eri_grad2 takes before its first HIP call, and the
algebra of dqc_amd/excited.py (difference density, transition densities, Z-vector right-hand side, energy-weighted density) driven
with dense oracle integrals on H2O / STO-3G -- the right-hand side against finite differences of w under orbital rotations, the
whole gradient against finite differences of E_SCF + w over nuclear displacements.  The excitation problem is solved densely here
(numpy, MO integrals), independently of the AO-basis form the module uses.  `eri_grad2_reference` is the dense yardstick of the
bilinear derivative pass that tests/test_gpu_excited_gradient.py imports."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import basis as ob, hamilton as oh, natives as nat
from tests import molecules as M

# H2O, distorted (no symmetry left): the geometry of the gradient tests
ZS = [8, 1, 1]
POS = [[0.0, 0.0, 0.2217], [0.0, 1.4309, -0.8867], [0.1, -1.4309, -0.8867]]
NO = 5
CASES = {"cis-singlet": (True, False), "tdhf-singlet": (False, False), "cis-triplet": (True, True), "tdhf-triplet": (False, True)}


# ------------------------------------------------------------------------------------------------ the dense yardstick of the kernel
def dense_eri_ip(t, cart=False):
    """(3, n, n, n, n): (d/dA a b|c d), A the centre of a, for the whole table from the oracle's derivative quartets"""
    ls = [int(l) for l in t.bas[:, 1]]
    dims = [(l + 1) * (l + 2) // 2 if cart else 2 * l + 1 for l in ls]
    offs = np.concatenate([[0], np.cumsum(dims)])
    ns = len(ls)
    quartets = [(a, b, c, d) for a in range(ns) for b in range(ns) for c in range(ns) for d in range(ns)]
    blocks = nat.int2e_ip_quartets(t, quartets, cart=cart)
    n = int(offs[-1])
    out = np.zeros((3, n, n, n, n))
    for (a, b, c, d), blk in zip(quartets, blocks):
        out[:, offs[a]:offs[a + 1], offs[b]:offs[b + 1], offs[c]:offs[c + 1], offs[d]:offs[d + 1]] = blk
    return out


def eri_grad2_reference(t, a, b, jscale, kscale, cart=False, ip=None):
    """(natm, 3): sum_{a on atom A} sum_bcd (d_A a b|c d) [jscale (A_ab B_cd + B_ab A_cd) - kscale / 2 (A_ac B_bd + B_ac A_bd)] from the
    dense derivative integrals (`ip`: those of dense_eri_ip when the caller holds them), no symmetry of A or B used"""
    ip = dense_eri_ip(t, cart) if ip is None else ip
    per = np.zeros((ip.shape[1], 3))
    if jscale != 0.0:
        per += jscale * (np.einsum("xpqrs,pq,rs->px", ip, a, b, optimize=True) + np.einsum("xpqrs,pq,rs->px", ip, b, a, optimize=True))
    if kscale != 0.0:
        per -= 0.5 * kscale * (np.einsum("xpqrs,pr,qs->px", ip, a, b, optimize=True) + np.einsum("xpqrs,pr,qs->px", ip, b, a, optimize=True))
    g = np.zeros((t.natm, 3))
    np.add.at(g, nat.ao_atom(t, cart), per)
    return g


def test_eri_grad2_reference_diagonal_is_the_quadratic_oracle():
    """eri_grad2_reference(D, D, j, k) is the oracle's own quadratic contraction orc_eri_grad (spherical and Cartesian)"""
    t = ob.make_tables((ZS, POS), "sto-3g")
    rng = np.random.default_rng(5)
    for cart in (False, True):
        n = nat.ao_count(t, cart)
        d = rng.standard_normal((n, n))
        d = d + d.T
        for j, k in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0)):
            ref = nat.eri_grad(t, d, j, k, cart=cart)
            got = eri_grad2_reference(t, d, d, j, k, cart=cart)
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (cart, j, k)


# ------------------------------------------------------------------------------------------------ gates
def test_eri_grad2_host_gates_without_a_gpu():
    """the gates of dqc_eri_grad2 before its first HIP call (raw ctypes, null device pointers and stream, H2O / STO-3G): a wrong
    matrix dimension, a parity that is not +-1, a mixed-parity pair and an antisymmetric pair with a Coulomb part are refused with
    their messages and nothing launched; a success of another entry point in between shows each message is new"""
    from dqc_amd import build, lib
    build.build()
    so = ctypes.CDLL(lib.libpath())
    so.dqc_last_error.restype = ctypes.c_char_p
    t = ob.make_tables(M.H2O, "sto-3g")
    atm = np.ascontiguousarray(t.atm, dtype=np.int32)
    bas = np.ascontiguousarray(t.bas, dtype=np.int32)
    env = np.ascontiguousarray(t.env, dtype=np.float64)
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    I, V, D = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    so.dqc_eri_grad2.argtypes = [V, V, V, I, I, I, D, D, ip, I, ip, I, dp, I, V]
    so.dqc_eri_grad.argtypes = [V, V, D, D, ip, I, ip, I, dp, I, V]
    tab = (atm.ctypes.data_as(ip), atm.shape[0], bas.ctypes.data_as(ip), bas.shape[0], env.ctypes.data_as(dp), env.shape[0])
    ncart = sum((int(l) + 1) * (int(l) + 2) // 2 for l in bas[:, 1])
    err = lambda: so.dqc_last_error().decode()  # noqa: E731

    def g2(n, pa, pb, j, k):
        return so.dqc_eri_grad2(None, None, None, n, pa, pb, j, k, *tab, None)

    def ok_between():
        assert so.dqc_eri_grad(None, None, 1.0, 1.0, *tab[:3], 0, *tab[4:], None) == 0

    assert g2(ncart + 1, 1, 1, 1.0, 1.0) == -1
    assert err() == "dqc_eri_grad2: the matrices are (%d, %d), the table has %d Cartesian functions" % (ncart + 1, ncart + 1, ncart)
    ok_between()
    assert g2(ncart, 1, -1, 0.0, 1.0) == -1 and g2(ncart, -1, 1, 0.0, 1.0) == -1
    assert err() == "dqc_eri_grad2: one matrix is symmetric and the other antisymmetric (the bilinear form needs a same-parity pair)"
    ok_between()
    assert g2(ncart, -1, -1, 1.0, 1.0) == -1
    assert err() == "dqc_eri_grad2: an antisymmetric pair has no Coulomb part (jscale must be 0)"
    ok_between()
    assert g2(ncart, 0, 1, 1.0, 1.0) == -1 and err() == "dqc_eri_grad2: a parity is +1 (symmetric) or -1 (antisymmetric)"
    ok_between()
    # past the gates: null operands are refused, too, before anything is uploaded
    assert g2(ncart, 1, 1, 1.0, 1.0) == -1 and err() == "dqc_eri_grad2: null pointer"
    assert g2(ncart, -1, -1, 0.0, 1.0) == -1 and err() == "dqc_eri_grad2: null pointer"


# ------------------------------------------------------------------------------------------------ dense SCF and response
_SCF = {}


def _scf(pos):
    """oracle RHF of H2O / STO-3G at `pos` (memoised): dict with the tables, E_SCF, canonical C (AO basis) and eps, h_core and the
    dense ERIs"""
    key = tuple(tuple(float(x) for x in p) for p in pos)
    if key not in _SCF:
        e, eng = oh.run_scf((ZS, [list(p) for p in key]), "sto-3g", tol=1e-12, maxiter=200)
        t = eng.t
        x = eng.h.X.numpy()
        d = x @ eng.dm.numpy() @ x.T
        hcore = nat.int1e("kin", t) + nat.int1e("nuc", t)
        eri = nat.int2e(t)
        f = hcore + np.einsum("pqrs,rs->pq", eri, d) - 0.5 * np.einsum("prqs,rs->pq", eri, d)
        eps, c = np.linalg.eigh(x.T @ f @ x)
        _SCF[key] = dict(t=t, e=e, c=x @ c, eps=eps, hcore=hcore, eri=eri, d=d)
    return _SCF[key]


def _ab(c, hcore, eri, triplet):
    """((A+B), (A-B)) as (no nv, no nv) matrices, rows (i, a), for ANY orthonormal orbitals c (the Fock blocks in full): the MO-integral
    form of the module docstring of dqc_amd/excited.py"""
    n, no = c.shape[1], NO
    nv = n - no
    co = c[:, :no]
    d = 2.0 * co @ co.T
    f = c.T @ (hcore + np.einsum("pqrs,rs->pq", eri, d) - 0.5 * np.einsum("prqs,rs->pq", eri, d)) @ c
    mo = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, c, c, c, c, optimize=True)
    ovov, oovv = mo[:no, no:, :no, no:], mo[:no, :no, no:, no:]
    diag = np.einsum("ij,ab->iajb", np.eye(no), f[no:, no:]) - np.einsum("ab,ij->iajb", np.eye(nv), f[:no, :no])
    ex1, ex2 = ovov.transpose(0, 3, 2, 1), oovv.transpose(0, 2, 1, 3)          # (ib|ja), (ij|ab)
    apb = diag + (0.0 if triplet else 4.0) * ovov - ex1 - ex2
    amb = diag + ex1 - ex2
    return apb.reshape(no * nv, no * nv), amb.reshape(no * nv, no * nv)


def _states(s, tda, triplet):
    """(w (all roots), U, V): the dense excitation problem at the SCF point `s`; U[k], V[k] (no, nv), U . V = 1 (TDA: U = V = X)"""
    apb, amb = _ab(s["c"], s["hcore"], s["eri"], triplet)
    nv = s["c"].shape[1] - NO
    if tda:
        w, x = np.linalg.eigh(0.5 * (apb + amb))
        u = v = x.T.reshape(-1, NO, nv)
    else:
        dd, q = np.linalg.eigh(amb)
        rt, irt = (q * np.sqrt(dd)) @ q.T, (q / np.sqrt(dd)) @ q.T
        w2, z = np.linalg.eigh(rt @ apb @ rt)
        w = np.sqrt(w2)
        u, v = ((rt @ z) / np.sqrt(w)).T.reshape(-1, NO, nv), ((irt @ z) * np.sqrt(w)).T.reshape(-1, NO, nv)
    return w, u, v


def _pick_state(w):
    """the lowest root more than 1e-2 Ha away from both neighbours"""
    for k in range(len(w)):
        if (k == 0 or w[k] - w[k - 1] > 1e-2) and (k == len(w) - 1 or w[k + 1] - w[k] > 1e-2):
            return k
    raise AssertionError("no isolated root")


def _omega(c, u, v, hcore, eri, triplet):
    apb, amb = _ab(c, hcore, eri, triplet)
    return 0.5 * (u.reshape(-1) @ apb @ u.reshape(-1) + v.reshape(-1) @ amb @ v.reshape(-1))


def _tt(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64)


def _jk_dense(eri):
    """the contract of lib.jk_multi on dense integrals: plain J and K of the symmetrised densities, the flagged exchange densities
    antisymmetrised"""
    e = _tt(eri)

    def jk(dms_j, dms_k, flags):
        dj = 0.5 * (dms_j + dms_j.transpose(1, 2))
        dk = torch.stack([0.5 * (m - m.T) if f else 0.5 * (m + m.T) for m, f in zip(dms_k, flags)])
        return torch.einsum("pqrs,nrs->npq", e, dj), torch.einsum("prqs,nrs->npq", e, dk)
    return jk


def _rhs(s, u, v, triplet):
    from dqc_amd import excited
    c = s["c"]
    return excited.lagrangian_rhs(_tt(u), _tt(v), _tt(c[:, :NO]), _tt(c[:, NO:]), _jk_dense(s["eri"]), triplet=triplet)


@pytest.mark.parametrize("case", sorted(CASES))
def test_rhs_is_the_orbital_rotation_derivative(case):
    """R_ai of excited.lagrangian_rhs against the central finite difference of w[C exp(kappa - kappa^T), X, Y] in every kappa_ai at
    fixed X, Y, w from the MO-integral form of A+B and A-B with the full Fock blocks.  Richardson extrapolation of the steps 1e-3 and
    2e-3; bound 10 |FD(h) - FD(2h)| + 1e-10"""
    tda, triplet = CASES[case]
    s = _scf(POS)
    w, us, vs = _states(s, tda, triplet)
    k = _pick_state(w)
    u, v = us[k], vs[k]
    assert abs(_omega(s["c"], u, v, s["hcore"], s["eri"], triplet) - w[k]) < 1e-12
    assert abs((u * v).sum() - 1.0) < 1e-12
    rhs = _rhs(s, u, v, triplet)[0].numpy()
    n = s["c"].shape[1]
    nv = n - NO
    worst = 0.0
    for a in range(nv):
        for i in range(NO):
            fd = []
            for h in (1e-3, 2e-3):
                vals = []
                for sign in (1.0, -1.0):
                    rot = s["c"].copy()          # exp(kappa - kappa^T) of one kappa_ai is a plane rotation of the columns i and a
                    ci, ca = s["c"][:, i], s["c"][:, NO + a]
                    rot[:, i] = np.cos(h) * ci + sign * np.sin(h) * ca
                    rot[:, NO + a] = np.cos(h) * ca - sign * np.sin(h) * ci
                    vals.append(_omega(rot, u, v, s["hcore"], s["eri"], triplet))
                fd.append((vals[0] - vals[1]) / (2 * h))
            rich = (4.0 * fd[0] - fd[1]) / 3.0
            bound = 10.0 * abs(fd[0] - fd[1]) + 1e-10
            worst = max(worst, abs(rhs[a, i] - rich))
            assert abs(rhs[a, i] - rich) <= bound, (case, a, i, rhs[a, i], rich, bound)
    print("rhs %s state %d: max |R| %.3e worst |R - richardson| %.2e" % (case, k, np.abs(rhs).max(), worst))
    assert np.abs(rhs).max() > 1e-3


def _nuclear_repulsion_gradient(pos):
    pos = np.asarray(pos)
    g = np.zeros_like(pos)
    for a in range(len(ZS)):
        for b in range(len(ZS)):
            if a != b:
                r = pos[a] - pos[b]
                g[a] -= ZS[a] * ZS[b] * r / np.linalg.norm(r) ** 3
    return g


def _analytic(s, u, v, triplet, with_z=True):
    """d(E_SCF + w) / dR (natm, 3) from the host functions of dqc_amd/excited.py, a dense Z-vector solve and the oracle's derivative
    integrals; also the SCF part"""
    from dqc_amd import excited
    c, eps, t, eri = s["c"], s["eps"], s["t"], s["eri"]
    co, cv = _tt(c[:, :NO]), _tt(c[:, NO:])
    nv = c.shape[1] - NO
    rhs, parts = _rhs(s, u, v, triplet)
    z = None
    if with_z:
        hess = 4.0 * _ab(c, s["hcore"], eri, False)[0]                       # the singlet orbital Hessian, rows (i, a)
        z = _tt(np.linalg.solve(hess, -rhs.numpy().T.reshape(-1)).reshape(NO, nv).T)
    p = excited.relaxed_density_mo(parts["t_oo"], parts["t_vv"], z)
    call = _tt(c)
    pbar = call @ p @ call.T
    jk = _jk_dense(eri)
    jp, kp = jk(pbar[None], pbar[None], [0])
    w2 = excited.energy_weighted(p, _tt(eps), parts["coupling"], jp[0] - 0.5 * kp[0], co, cv)
    ip = dense_eri_ip(t)
    d, sm, nm, pb = s["d"], parts["s"].numpy(), parts["n"].numpy(), pbar.numpy()
    assert np.abs(sm - sm.T).max() == 0.0 and np.abs(nm + nm.T).max() == 0.0
    exc = nat.int1e_grad(t, pb, w2.numpy())
    exc += eri_grad2_reference(t, d, pb, 2.0, 2.0, ip=ip)
    exc += eri_grad2_reference(t, sm, sm, 0.0 if triplet else 4.0, 4.0, ip=ip)
    exc += eri_grad2_reference(t, nm, nm, 0.0, 4.0, ip=ip)
    w_scf = 2.0 * (c[:, :NO] * eps[:NO]) @ c[:, :NO].T
    scf = nat.int1e_grad(t, d, w_scf) + nat.eri_grad(t, d, 1.0, 1.0) + _nuclear_repulsion_gradient(POS)
    return scf + exc, scf


@pytest.mark.parametrize("case", ["cis-singlet", "tdhf-singlet", "cis-triplet"])
def test_gradient_on_oracle_integrals_against_finite_differences(case):
    """d(E_SCF + w) / dR assembled from excited.lagrangian_rhs / relaxed_density_mo / energy_weighted, a dense Z-vector solve, the
    oracle's one-electron derivative contraction and the dense bilinear reference, against Richardson-extrapolated central differences
    (h = 1e-3, 2e-3 Bohr) of oracle SCF energies plus the dense excitation energy of the same root.  Components (O, z), (H1, y),
    (H2, x); bound 10 |FD(h) - FD(2h)| + 1e-9.  Without the Z-vector the same assembly misses the bound (the test sees the relaxation)"""
    tda, triplet = CASES[case]
    s = _scf(POS)
    w, us, vs = _states(s, tda, triplet)
    k = _pick_state(w)
    grad, scf = _analytic(s, us[k], vs[k], triplet)
    noz, _ = _analytic(s, us[k], vs[k], triplet, with_z=False)
    assert np.abs(grad.sum(0)).max() < 1e-10 and np.abs(scf.sum(0)).max() < 1e-10

    def e_tot(pos):
        sp = _scf(pos)
        return sp["e"] + _states(sp, tda, triplet)[0][k]

    missed = 0
    for atom, d in ((0, 2), (1, 1), (2, 0)):
        fd = []
        for h in (1e-3, 2e-3):
            pp, pm = np.array(POS), np.array(POS)
            pp[atom, d] += h
            pm[atom, d] -= h
            fd.append((e_tot(pp.tolist()) - e_tot(pm.tolist())) / (2 * h))
        rich = (4.0 * fd[0] - fd[1]) / 3.0
        bound = 10.0 * abs(fd[0] - fd[1]) + 1e-9
        print("excited gradient %s state %d atom %d dir %d: analytic % .10e (scf % .10e) richardson % .10e |diff| %.2e bound %.2e "
              "without Z |diff| %.2e" % (case, k, atom, d, grad[atom, d], scf[atom, d], rich, abs(grad[atom, d] - rich), bound,
                                         abs(noz[atom, d] - rich)))
        assert abs(grad[atom, d] - rich) <= bound, (case, atom, d, grad[atom, d], rich, bound)
        missed += abs(noz[atom, d] - rich) > bound
    assert missed > 0, "the assembly without the Z-vector passes as well: the test cannot see the relaxation"
