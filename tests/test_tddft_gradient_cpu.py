"""CPU tests (no GPU) of the TDDFT / TDA excited-state gradient:

  * the Kohn-Sham right-hand side of dqc_amd/excited.py (lagrangian_rhs with its `xc` callable and exchange fraction) against finite
    differences of w[C] under every orbital rotation, on H2O / STO-3G with dense oracle integrals and a TOY exchange-correlation
    functional: a few hundred fixed points with positive weights, e(rho, sigma) of lda_x and of PBE from the torch namespace of
    oracle/xc_exact.py, V_xc, V1 and V2 by autograd through the AO values.  The toy SCF is converged first (R has no Fock term only for
    canonical orbitals), the excitation problem solved densely; the same comparison without 2 V2[S, S] misses its bound;
  * the third-order fixture tests/golden/xc_kxc_exact_unpol.npz against itself: steps 1e-20 and 1e-15 of the truth agree to 1e-25, the
    torch-double rows reproduce the recorded errors, which are within the bars the GPU test uses wherever a bar is above its floor;
  * the gates of dqc_xc_eval_kxc before its first HIP call (raw ctypes, null pointers)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import natives as nat, xc_exact as xe
from tests.test_excited_gradient_cpu import NO, POS, _jk_dense, _pick_state, _scf, _tt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_xc_kxc_golden as kg  # noqa: E402

TOYS = {"lda": ["lda_x"], "pbe": ["gga_x_pbe", "gga_c_pbe"]}


# ------------------------------------------------------------------------------------------------ the toy functional
class Toy:
    """E_xc[D] = sum_g w_g e(rho_D(r_g), |grad rho_D(r_g)|^2) on fixed points; everything else by autograd in D"""

    def __init__(self, t, names, seed=11):
        rng = np.random.default_rng(seed)
        pts = np.concatenate([np.asarray(p) + 0.8 * rng.standard_normal((120, 3)) for p in POS])
        self.w = _tt(0.05 * rng.uniform(0.5, 1.5, pts.shape[0]))
        self.phi = _tt(nat.eval_gto(t, pts, 0))                 # (nao, ng)
        self.dphi = _tt(nat.eval_gto(t, pts, 1))                # (3, nao, ng)
        self.names = names
        self.ns = xe.TD()

    def energy(self, d):
        rho = torch.einsum("pq,pg,qg->g", d, self.phi, self.phi)
        grho = torch.einsum("pq,pg,xqg->xg", d, self.phi, self.dphi) + torch.einsum("pq,xpg,qg->xg", d, self.dphi, self.phi)
        sigma = (grho * grho).sum(0)
        e = 0.0
        for nm in self.names:
            parts = xe.FUNCS[nm](self.ns, *xe.unpolarised(rho, sigma), 0.0)
            e = e + sum(parts[1:], parts[0])
        return (self.w * e).sum()

    def _d(self, d):
        return _tt(d).clone().requires_grad_(True)

    def vxc(self, d):
        x = self._d(d)
        return torch.autograd.grad(self.energy(x), x)[0].detach()

    def e2(self, d, s, x=None):
        """the second directional derivative d2/dt2 E[D + t S] = tr[S V1[S]] (as a graph in x when x is given)"""
        x = self._d(d) if x is None else x
        s = _tt(s)
        g = torch.autograd.grad(self.energy(x), x, create_graph=True)[0]
        g2 = torch.autograd.grad((g * s).sum(), x, create_graph=True)[0]
        return (g2 * s).sum()

    def v1(self, d, m):
        x = self._d(d)
        g = torch.autograd.grad(self.energy(x), x, create_graph=True)[0]
        return torch.autograd.grad((g * _tt(m)).sum(), x)[0].detach()

    def v2(self, d, s):
        x = self._d(d)
        return torch.autograd.grad(self.e2(d, s, x), x)[0].detach()


_KS = {}


def _toy_scf(toy_name, a):
    """the converged toy Kohn-Sham calculation of H2O / STO-3G (exact-exchange fraction a): canonical C, eps, the pieces of _scf"""
    key = (toy_name, a)
    if key not in _KS:
        s = _scf(POS)
        t, hcore, eri = s["t"], s["hcore"], s["eri"]
        toy = Toy(t, TOYS[toy_name])
        ovlp = nat.int1e("ovlp", t)
        se, sv = np.linalg.eigh(ovlp)
        x = sv / np.sqrt(se)
        d = s["d"].copy()
        for it in range(2000):
            f = hcore + np.einsum("pqrs,rs->pq", eri, d) - 0.5 * a * np.einsum("prqs,rs->pq", eri, d) + toy.vxc(d).numpy()
            eps, c = np.linalg.eigh(x.T @ f @ x)
            c = x @ c
            dn = 2.0 * c[:, :NO] @ c[:, :NO].T
            step = np.abs(dn - d).max()
            d = 0.5 * (d + dn)
            if step < 1e-13:
                break
        assert step < 1e-12, "the toy SCF did not converge (%s, a = %g): %.2e" % (toy_name, a, step)
        f = hcore + np.einsum("pqrs,rs->pq", eri, d) - 0.5 * a * np.einsum("prqs,rs->pq", eri, d) + toy.vxc(d).numpy()
        eps, c = np.linalg.eigh(x.T @ f @ x)
        _KS[key] = dict(t=t, hcore=hcore, eri=eri, toy=toy, c=x @ c, eps=eps, a=a)
    return _KS[key]


def _sym_s(c, u):
    r = c[:, :NO] @ u @ c[:, NO:].T
    return 0.5 * (r + r.T)


def _ab_ks(ks, c):
    """((A+B), (A-B)) of the toy Kohn-Sham calculation for ANY orthonormal orbitals c, rows (i, a): the MO form of the module docstring
    of dqc_amd/excited.py, the Fock blocks in full, the f_xc block from V1 of every product density"""
    hcore, eri, toy, a = ks["hcore"], ks["eri"], ks["toy"], ks["a"]
    n, no = c.shape[1], NO
    nv = n - no
    d = 2.0 * c[:, :no] @ c[:, :no].T
    f = c.T @ (hcore + np.einsum("pqrs,rs->pq", eri, d) - 0.5 * a * np.einsum("prqs,rs->pq", eri, d) + toy.vxc(d).numpy()) @ c
    mo = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, c, c, c, c, optimize=True)
    ovov, oovv = mo[:no, no:, :no, no:], mo[:no, :no, no:, no:]
    diag = np.einsum("ij,ab->iajb", np.eye(no), f[no:, no:]) - np.einsum("ab,ij->iajb", np.eye(nv), f[:no, :no])
    ex1, ex2 = ovov.transpose(0, 3, 2, 1), oovv.transpose(0, 2, 1, 3)          # (ib|ja), (ij|ab)
    fxc = np.zeros((no, nv, no, nv))
    for j in range(no):
        for b in range(nv):
            e = np.zeros((no, nv))
            e[j, b] = 1.0
            fxc[:, :, j, b] = c[:, :no].T @ toy.v1(d, _sym_s(c, e)).numpy() @ c[:, no:]
    apb = diag + 4.0 * ovov + 4.0 * fxc - a * (ex1 + ex2)
    amb = diag + a * (ex1 - ex2)
    return apb.reshape(no * nv, no * nv), amb.reshape(no * nv, no * nv)


def _omega_ks(ks, c, u, v):
    """w[C, U, V] without the f_xc matrix: its quadratic form is 2 d2/dt2 E_xc[D + t S]"""
    hcore, eri, toy, a = ks["hcore"], ks["eri"], ks["toy"], ks["a"]
    no = NO
    d = 2.0 * c[:, :no] @ c[:, :no].T
    f = c.T @ (hcore + np.einsum("pqrs,rs->pq", eri, d) - 0.5 * a * np.einsum("prqs,rs->pq", eri, d) + toy.vxc(d).numpy()) @ c
    mo = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, c, c, c, c, optimize=True)
    ovov, oovv = mo[:no, no:, :no, no:], mo[:no, :no, no:, no:]
    ex1, ex2 = ovov.transpose(0, 3, 2, 1), oovv.transpose(0, 2, 1, 3)
    w = 0.0
    for x, two in ((u, 4.0 * ovov - a * (ex1 + ex2)), (v, a * (ex1 - ex2))):
        w += 0.5 * (np.einsum("ia,ab,ib->", x, f[no:, no:], x) - np.einsum("ia,ij,ja->", x, f[:no, :no], x)
                    + np.einsum("ia,iajb,jb->", x, two, x))
    return w + 2.0 * float(toy.e2(d, _sym_s(c, u)).detach())


def _ks_states(ks, tda):
    apb, amb = _ab_ks(ks, ks["c"])
    nv = ks["c"].shape[1] - NO
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


def _rhs_ks(ks, u, v, with_v2=True):
    from dqc_amd import excited
    c, toy = ks["c"], ks["toy"]
    d = 2.0 * c[:, :NO] @ c[:, :NO].T

    def xc(ms, s):
        v2 = toy.v2(d, s.numpy()) if with_v2 else torch.zeros_like(s)
        return torch.stack([toy.v1(d, m.numpy()) for m in ms]), v2

    return excited.lagrangian_rhs(_tt(u), _tt(v), _tt(c[:, :NO]), _tt(c[:, NO:]), _jk_dense(ks["eri"]), xc=xc, kfrac=ks["a"])


@pytest.mark.parametrize("tda", [True, False], ids=["tda", "full"])
@pytest.mark.parametrize("a", [0.0, 0.25])
@pytest.mark.parametrize("toy_name", sorted(TOYS))
def test_ks_rhs_is_the_orbital_rotation_derivative(toy_name, a, tda):
    """R_ai of lagrangian_rhs(..., xc=..., kfrac=a) against the Richardson central difference (steps 1e-3, 2e-3) of w[C exp(kappa -
    kappa^T), X, Y] in every kappa_ai at fixed X, Y; bound 10 |FD(h) - FD(2h)| + 1e-10 (tests/test_excited_gradient_cpu.py).  D, and with
    it V_xc and f_xc, follow the rotated orbitals.  Without 2 V2[S, S] the same comparison misses the bound"""
    ks = _toy_scf(toy_name, a)
    w, us, vs = _ks_states(ks, tda)
    k = _pick_state(w)
    u, v = us[k], vs[k]
    c = ks["c"]
    assert abs(_omega_ks(ks, c, u, v) - w[k]) < 1e-10 and abs((u * v).sum() - 1.0) < 1e-12
    rhs, parts = _rhs_ks(ks, u, v)
    rhs = rhs.numpy()
    no_v2 = _rhs_ks(ks, u, v, with_v2=False)[0].numpy()
    assert parts["v2"] is not None and float(parts["v2"].abs().max()) > 1e-6
    nv = c.shape[1] - NO
    worst = missed = 0
    for av in range(nv):
        for i in range(NO):
            fd = []
            for h in (1e-3, 2e-3):
                vals = []
                for sign in (1.0, -1.0):
                    rot = c.copy()
                    ci, ca = c[:, i], c[:, NO + av]
                    rot[:, i] = np.cos(h) * ci + sign * np.sin(h) * ca
                    rot[:, NO + av] = np.cos(h) * ca - sign * np.sin(h) * ci
                    vals.append(_omega_ks(ks, rot, u, v))
                fd.append((vals[0] - vals[1]) / (2 * h))
            rich = (4.0 * fd[0] - fd[1]) / 3.0
            bound = 10.0 * abs(fd[0] - fd[1]) + 1e-10
            worst = max(worst, abs(rhs[av, i] - rich))
            assert abs(rhs[av, i] - rich) <= bound, (toy_name, a, tda, av, i, rhs[av, i], rich, bound)
            missed += abs(no_v2[av, i] - rich) > bound
    print("KS rhs %s a = %.2f %s state %d: w %.6f  max |R| %.3e  worst |R - richardson| %.2e  max |R - R(no V2)| %.2e  elements that miss "
          "without V2: %d of %d" % (toy_name, a, "TDA" if tda else "full", k, w[k], np.abs(rhs).max(), worst, np.abs(rhs - no_v2).max(),
                                    missed, NO * nv))
    assert missed > 0, "the right-hand side without 2 V2[S, S] passes as well: the test cannot see the third-order term"


def test_rhs_defaults_are_the_hartree_fock_arithmetic():
    """xc=None, kfrac=1.0 give the tensors of a call without the new arguments, bit for bit"""
    from dqc_amd import excited
    s = _scf(POS)
    rng = np.random.default_rng(3)
    nv = s["c"].shape[1] - NO
    u, v = rng.standard_normal((NO, nv)), rng.standard_normal((NO, nv))
    args = (_tt(u), _tt(v), _tt(s["c"][:, :NO]), _tt(s["c"][:, NO:]), _jk_dense(s["eri"]))
    for triplet in (False, True):
        r0, p0 = excited.lagrangian_rhs(*args, triplet=triplet)
        r1, p1 = excited.lagrangian_rhs(*args, triplet=triplet, xc=None, kfrac=1.0)
        assert torch.equal(r0, r1) and all(torch.equal(p0[k], p1[k]) for k in p0 if p0[k] is not None) and p0["v2"] is None
        # and they are the formulas of the parent: G[Tbar] = J - K / 2, G+ = 4 J - 2 K, G- = -2 K
        J, K = args[4](torch.stack([p0["tbar"]] if triplet else [p0["tbar"], p0["s"]]), torch.stack([p0["tbar"], p0["s"], p0["n"]]), [0, 0, 1])
        assert torch.equal(p0["g_t"], J[0] - 0.5 * K[0])


# ------------------------------------------------------------------------------------------------ the fixture
def test_kxc_fixture_self_check(golden_dir):
    f = np.load(os.path.join(golden_dir, "xc_kxc_exact_unpol.npz"))
    p = {k[2:]: f[k] for k in f.files if k.startswith("p_")}
    q = kg.kxc_points()
    assert all(np.array_equal(p[k], q[k]) for k in q), "the points of the fixture are not those of the generator"
    zero_g = (np.abs(p["grho"]).sum(0) == 0.0) & (p["rho"] > xe.DENS_THRESHOLD)
    assert int(f["n_excluded"]) == 2 * int(zero_g.sum()) == 64      # gga_x_g96 at the zero-gradient points, both outputs; nothing else
    import mpmath as mp
    for name in xe.NAMES:
        val = f[name + "_val"]
        assert float(f[name + "_step_agreement"]) <= 1e-15
        err, bad = kg.class_errors(name, p, val, kg.double_rows(name, p))
        rec = f[name + "_double_err"]
        assert bad == int(f[name + "_double_nonfinite"]) == 0
        assert np.all(err <= 1.5 * rec + 1e-16) and np.all(rec <= 1.5 * err + 1e-16), (name, err, rec)   # (another libm may round otherwise)
        bar = np.maximum(kg.FLOOR, 10.0 * rec)
        assert np.all(err < bar)
        loose = [(kg.OUTPUTS[j], c, rec[j, c]) for j in range(2) for c in range(kg.NCLS) if 10.0 * rec[j, c] > kg.FLOOR]
        if loose:
            print("KXC bars above the floor, %s: %s" % (name, ", ".join("%s class %d: torch-double %.1e" % x for x in loose)))
    # the step of the truth: 1e-20 against 1e-15, in mpmath, to 1e-25 of the scale (a bulk point, a seam point, the tail)
    for name in ("gga_c_pbe", "gga_x_b88", "gga_c_lyp", "lda_c_vwn"):
        for i in (3, 100, 258, 264):
            g = p["grho"][:, i]
            x, dz, dps, zero = xe.effective_point_unpol(p["rho"][i], float((g * g).sum()))
            a, b, _ = kg.directions(p, i)
            xf = [float(t) for t in x]
            sa, sb = (2.0 ** np.ceil(np.log2(max(1.0, abs(d[0]) / xf[0], abs(d[1]) / xf[1]))) for d in (a, b))
            a, b = [t / sa for t in a], [t / sb for t in b]
            fine = kg.third_rows(name, x, dz, a, b, kg.third_dps(dps), zero, kg.H_REL)
            coarse = kg.third_rows(name, x, dz, a, b, kg.third_dps(dps), zero, kg.H_CHECK)
            for (t1, s1), (t2, _) in zip(fine, coarse):
                assert abs(t1 - t2) <= mp.mpf(1e-25) * s1, (name, i, float(abs(t1 - t2) / s1))


# ------------------------------------------------------------------------------------------------ gates
def test_xc_eval_kxc_host_gates_without_a_gpu():
    """the gates of dqc_xc_eval_kxc before its first HIP call (raw ctypes, null device pointers and stream): more than 8 terms, a GGA
    id without the gradient pointers, a meta-GGA id, a negative number of pairs -- each refused with its message, nothing launched; a
    success (n = 0) in between shows each message is new"""
    from dqc_amd import build, lib
    build.build()
    so = ctypes.CDLL(lib.libpath())
    so.dqc_last_error.restype = ctypes.c_char_p
    I, V = ctypes.c_int, ctypes.c_void_p
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    so.dqc_xc_eval_kxc.argtypes = [V] * 8 + [I, I, ip, dp, I, V]
    err = lambda: so.dqc_last_error().decode()  # noqa: E731

    def call(ids, n, npair, nterm=None):
        ids_c = (ctypes.c_int * max(len(ids), 1))(*ids)
        cfs = (ctypes.c_double * max(len(ids), 1))(*([1.0] * len(ids)))
        return so.dqc_xc_eval_kxc(None, None, None, None, None, None, None, None, n, npair, ids_c, cfs, len(ids) if nterm is None else nterm, None)

    lda, pbe, scan = lib.XC_IDS["lda_x"], lib.XC_IDS["gga_x_pbe"], lib.XC_IDS["mgga_x_scan"]
    ok = lambda: call([lda], 0, 1) == 0  # noqa: E731
    assert ok()
    assert call([lda] * 9, 16, 1) != 0 and err() == "dqc_xc_eval_kxc: at most 8 functional terms"
    assert ok()
    assert call([lda], 16, 1, nterm=-1) != 0 and err() == "dqc_xc_eval_kxc: at most 8 functional terms"
    assert ok()
    assert call([lda, pbe], 16, 1) != 0 and "dqc_xc_eval_kxc: GGA functional needs the density gradients" in err()
    assert ok()
    assert call([scan], 16, 1) != 0 and err() == "dqc_xc_eval_kxc: only the LDA / GGA functional ids have a second-order kernel"
    assert ok()
    assert call([lda], 16, -1) != 0 and err() == "dqc_xc_eval_kxc: negative number of trial vectors"
    assert ok() and call([lda], 16, 0) == 0
