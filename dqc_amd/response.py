"""Orbital-Hessian products of a converged HF / KS calculation: SCF stability and static response.

Variables: the real virtual <- occupied rotations kappa_ai of C(kappa) = C exp(kappa - kappa^T) (the non-redundant parameters;
occupied-occupied and virtual-virtual rotations leave the energy of integer occupations unchanged and are not variables).
One block for a restricted calculation, the alpha and beta blocks concatenated for an unrestricted one; a trial vector is the
row-major flattening (a, i) of its block(s).

    restricted (occupations 2):    D = 2 C_o C_o^T,        dD = 2 (C_v kappa C_o^T + transpose)
        dE/dkappa_ai = 4 F_ai
        (H kappa)_ai = 4 [ (F_vv kappa - kappa F_oo)_ai + (C_v^T G[dD] C_o)_ai ],     G[dD] = J[dD] - (a / 2) K[dD] + f_xc[rho] . d rho

    unrestricted (occupations 1):  D_s = C_os C_os^T,      dD_s = C_vs kappa_s C_os^T + transpose
        dE/dkappa_s,ai = 2 F_s,ai
        (H kappa)_s,ai = 2 [ (F_s,vv kappa_s - kappa_s F_s,oo)_ai + (C_vs^T G_s C_os)_ai ],
        G_s = J[dD_u + dD_d] - a K[dD_s] + sum_s' f_xc^(s s') . d rho_s'

a is the exact-exchange fraction (1 for Hartree-Fock, the functional's for Kohn-Sham, 0 for a pure functional); K is the plain
exchange matrix K[D]_pq = (pr|qs) D_rs.  The orbitals are the canonical ones (eigenvectors of the converged Fock matrix), so
F_vv kappa - kappa F_oo = (eps_a - eps_i) kappa_ai.  Everything is formed in the AO basis (C = X C_orth), where the projection is
C_v^T G C_o without a change of basis.

A call of `mm` on nvec trial vectors is: kappa -> dD (two tile-parallel launches for the whole block, csrc/fock.hip), ONE pass over
the ERI tiles for all J and K (lib.jk_multi), per trial vector one density pass and one Vxc GEMM, one launch of the second-order
functional kernel per functional term for the whole block (csrc/xc.hip: dqc_xc_eval_fxc), and the projection with the diagonal term
(two launches for the block).

Linear response (excited states).  In the language of TDHF / TDDFT the Hessian is pref (A + B), pref = 4 restricted, 2
unrestricted; excitation energies need the second operator A - B as well, which carries the exchange of an ANTISYMMETRIC density:

    restricted     (A-B) kappa = (eps_a - eps_i) kappa_ai - (a / 2) [C_v^T K[dD-] C_o]_ai,     dD- = 2 (C_v kappa C_o^T - transpose)
    unrestricted   (A-B)_s kappa_s = (eps_a - eps_i) kappa_s,ai - a [C_vs^T K[dD_s-] C_os]_ai,   dD_s- = C_vs kappa_s C_os^T - transpose
    restricted triplet (spin="triplet": dD_u = -dD_d = dD+ / 2)
                   (A+B)^T kappa = (eps_a - eps_i) kappa_ai + [C_v^T G^T C_o]_ai,   G^T = -(a / 2) K[dD+] + d v_u   (no Coulomb term),
                   d v_u from csrc/xc.hip: dqc_xc_eval_fxc_triplet;   (A-B)^T = (A-B)^S

`mm_minus` is pref (A - B) -- the diagonal, without a tile pass, for a pure functional (a = 0) -- and `mm_pair` returns both products
from ONE `jk_multi` call: K[dD+] and K[dD-] of a trial vector share an NK = 2 pass (lib.jk_multi(..., k_antisym=...)).
`response_eigs` solves (A-B)(A+B)(X+Y) = w^2 (X+Y) with one trial space for both operators; `OrbitalHessian.excite` drives it (or
`davidson_lowest` for the Hermitian cases: TDA, and a = 0 where the problem is Delta^(1/2) (A+B) Delta^(1/2) Z = w^2 Z).

`davidson_lowest`, `response_eigs` and `pcg_solve` are plain torch on any device (the subspace matrices are small);
`OrbitalHessian.lowest`, `.excite` and `.solve` hand them the products and the preconditioner (eps_a - eps_i)."""
import warnings

import torch

from . import lib
from .xc import LibXC


# ---------------------------------------------------------------------------------------------------------------- solvers
def _orthonormalise(t, basis, drop):
    """rows of t orthogonalised against the rows of `basis` (twice) and among themselves; rows whose norm falls below `drop`
    times what it was are dropped"""
    out = []
    for x in t:
        n0 = float(x.norm())
        if n0 == 0.0:
            continue
        for _ in range(2):
            if basis is not None and basis.shape[0]:
                x = x - (basis @ x) @ basis
            for y in out:
                x = x - (y @ x) * y
        n1 = float(x.norm())
        if n1 > drop * n0:
            out.append(x / n1)
    return torch.stack(out) if out else t[:0]


def davidson_lowest(mm, diag, neig=1, tol=1e-8, maxiter=200, max_space=None):
    """the `neig` lowest eigenpairs of the symmetric operator `mm` ((nvec, n) -> (nvec, n)) by block Davidson with the diagonal
    preconditioner `diag` (n,).  Returns (eigenvalues (neig,), eigenvectors (neig, n), largest residual norm).  Converged when every
    residual norm |H x - theta x| is below `tol`; a subspace that has grown to the whole space is exact."""
    n = diag.numel()
    neig = min(neig, n)
    max_space = max_space or max(8 * neig, 24)
    start = min(n, max(2 * neig, neig + 3))
    idx = torch.argsort(diag)[:start]
    V = torch.zeros((start, n), dtype=diag.dtype, device=diag.device)
    V[torch.arange(start), idx] = 1.0
    W = mm(V)
    res = float("inf")
    for _ in range(maxiter):
        Hs = V @ W.T
        theta, y = torch.linalg.eigh((Hs + Hs.T) * 0.5)
        theta, y = theta[:neig], y[:, :neig]
        x, hx = y.T @ V, y.T @ W
        r = hx - theta[:, None] * x
        rn = r.norm(dim=1)
        res = float(rn.max())
        if res < tol or V.shape[0] >= n:
            break
        den = theta[:, None] - diag[None, :]
        den = torch.where(den.abs() < 1e-3, torch.where(den < 0, -1e-3, 1e-3).to(den.dtype), den)
        t = (r / den)[rn >= tol]
        if V.shape[0] + t.shape[0] > max_space:  # restart from the current Ritz vectors
            V, W = x, hx
            V = _orthonormalise(V, None, 1e-12)
            W = mm(V)
        t = _orthonormalise(t, V, 1e-8)
        if t.shape[0] == 0:
            break
        V = torch.cat([V, t])
        W = torch.cat([W, mm(t)])
    return theta, x, res


def response_eigs(mm_pair, diag, neig=1, tol=1e-6, maxiter=200, max_space=None):
    """the `neig` lowest solutions of the linear-response problem (A-B)(A+B)(X+Y) = w^2 (X+Y), both operators symmetric positive
    definite, by block Davidson with ONE trial space b for both: `mm_pair` ((nvec, n) -> ((A+B) v, (A-B) v)), `diag` (n,) the
    diagonal of either (eps_a - eps_i: the preconditioner).  Reduced problem: M+ = b (A+B) b^T, M- = b (A-B) b^T, eigenpairs of
    M-^(1/2) M+ M-^(1/2); X+Y = b^T M-^(1/2) z / sqrt(w), X-Y = sqrt(w) b^T M-^(-1/2) z, so that (X+Y) . (X-Y) = 1.
    Residuals (A+B)(X+Y) - w (X-Y) and (A-B)(X-Y) - w (X+Y); converged when both norms are below `tol` for every state; a subspace
    that has grown to the whole space is exact.  A reduced M- or M+ that is not positive definite raises RuntimeError.
    Returns (w (neig,), X+Y (neig, n), X-Y (neig, n), largest residual norm)."""
    n = diag.numel()
    neig = min(neig, n)
    max_space = max_space or max(8 * neig, 24)
    start = min(n, max(2 * neig, neig + 3))
    idx = torch.argsort(diag)[:start]
    V = torch.zeros((start, n), dtype=diag.dtype, device=diag.device)
    V[torch.arange(start), idx] = 1.0
    P, Q = mm_pair(V)
    res = float("inf")

    def reduced():
        mp, mq = V @ P.T, V @ Q.T
        mp, mq = (mp + mp.T) * 0.5, (mq + mq.T) * 0.5
        d, u = torch.linalg.eigh(mq)
        if not float(d[0]) > 0.0:
            raise RuntimeError("response_eigs: A - B is not positive definite in the trial space (lowest eigenvalue %.3e); the SCF "
                               "state is not a minimum (is_orb_min)" % float(d[0]))
        rt, irt = (u * d.sqrt()) @ u.T, (u / d.sqrt()) @ u.T
        w2, z = torch.linalg.eigh(rt @ mp @ rt)
        if not float(w2[0]) > 0.0:
            raise RuntimeError("response_eigs: A + B is not positive definite in the trial space (lowest w^2 %.3e): the SCF state is "
                               "not a minimum in this spin channel (is_orb_min; triplet=True for spin=\"triplet\")" % float(w2[0]))
        w = w2[:neig].sqrt()
        return w, (rt @ z[:, :neig] / w.sqrt()).T, (irt @ z[:, :neig] * w.sqrt()).T  # coefficients of X+Y, X-Y in the trial space

    for _ in range(maxiter):
        w, cp, cm = reduced()
        xpy, xmy = cp @ V, cm @ V
        rp = cp @ P - w[:, None] * xmy
        rm = cm @ Q - w[:, None] * xpy
        rn = torch.maximum(rp.norm(dim=1), rm.norm(dim=1))
        res = float(rn.max())
        if res < tol or V.shape[0] >= n:
            break
        den = w[:, None] - diag[None, :]
        den = torch.where(den.abs() < 1e-3, torch.where(den < 0, -1e-3, 1e-3).to(den.dtype), den)
        live = rn >= tol
        t = torch.cat([(rp / den)[live], (rm / den)[live]])
        if V.shape[0] + t.shape[0] > max_space:  # restart from the span of the current X+Y and X-Y
            V = _orthonormalise(torch.cat([xpy, xmy]), None, 1e-12)
            P, Q = mm_pair(V)
        t = _orthonormalise(t, V, 1e-8)
        if t.shape[0] == 0:
            break
        if V.shape[0] + t.shape[0] > n:
            t = t[:n - V.shape[0]]
        V = torch.cat([V, t])
        pt, qt = mm_pair(t)
        P, Q = torch.cat([P, pt]), torch.cat([Q, qt])
    return w, xpy, xmy, res


def pcg_solve(mm, diag, rhs, tol=1e-8, maxiter=200):
    """H x = rhs for the rows of rhs (nrhs, n) by conjugate gradients preconditioned with `diag` (n,), every right-hand side with
    its own step lengths; H symmetric positive definite (a search direction of non-positive curvature raises RuntimeError).
    Converged when |H x - b| <= tol |b| for every row.  Returns (x, largest relative residual)."""
    b = rhs
    bn = b.norm(dim=1).clamp_min(1e-300)
    x = torch.zeros_like(b)
    r = b.clone()
    z = r / diag
    p = z.clone()
    rz = (r * z).sum(1)
    rel = float((r.norm(dim=1) / bn).max())
    for _ in range(maxiter):
        if rel <= tol:
            break
        live = (r.norm(dim=1) / bn > tol).to(b.dtype)  # a converged row (or a zero right-hand side) rests: its steps would be 0 / 0
        hp = mm(p)
        php = (p * hp).sum(1)
        if bool(torch.any((php <= 0) & (live > 0))):  # conjugate gradients would step along a direction of non-positive curvature
            raise RuntimeError("pcg_solve: the operator is not positive definite (p . H p = %.3e for a search direction); for an "
                               "orbital Hessian the SCF state is not a minimum (is_orb_min)" % float(php[live > 0].min()))
        alpha = live * rz / torch.where(php == 0, torch.ones_like(php), php)
        x = x + alpha[:, None] * p
        r = r - alpha[:, None] * hp
        rel = float((r.norm(dim=1) / bn).max())
        z = r / diag
        rz_new = (r * z).sum(1)
        p = z + (live * rz_new / torch.where(rz == 0, torch.ones_like(rz), rz))[:, None] * p
        rz = rz_new
    return x, rel


# ---------------------------------------------------------------------------------------------------------------- the operator
def _unsupported(qc):
    eng = qc._engine
    h = eng.hamilton
    if h.df is not None:
        raise NotImplementedError("OrbitalHessian: density fitting is not supported (the response needs the exact J and K)")
    if getattr(h, "sharded", False):
        raise NotImplementedError("OrbitalHessian: a Hamiltonian sharded over several GPUs (shard_over) is not supported")
    if getattr(h, "_direct", False) or getattr(h, "_tiles_store", None) is None:
        raise NotImplementedError("OrbitalHessian: direct SCF is not supported (the response streams the resident ERI tiles)")
    if eng.is_ks:
        if not isinstance(eng.xc, LibXC):
            raise NotImplementedError("OrbitalHessian: only functionals of the kernel set (LibXC objects) have a second-order kernel, "
                                      "not %s" % type(eng.xc).__name__)
        for _, name in eng.xc.terms:
            if name.startswith("mgga_"):
                raise NotImplementedError("OrbitalHessian: no second-order kernel for the meta-GGA functional %s" % name)
    full = 1.0 if eng.polarized else 2.0
    for w in ((eng.orb_weight.u, eng.orb_weight.d) if eng.polarized else (eng.orb_weight,)):
        if not bool(torch.all(w == full)):
            if not eng.polarized and bool(torch.all((w == 2.0) | (w == 1.0))):
                raise NotImplementedError("OrbitalHessian: restricted open-shell occupations (2, ..., 2, 1, ..., 1) are not supported")
            raise NotImplementedError("OrbitalHessian: fractional or user-given occupations are not supported (integer occupations "
                                      "%g only)" % full)


class _Spin:
    """one block of variables: occupied / virtual AO coefficients and orbital energies"""

    def __init__(self, c_ao, eps, nocc):
        self.co, self.cv = c_ao[:, :nocc].contiguous(), c_ao[:, nocc:].contiguous()
        self.eo, self.ev = eps[:nocc].contiguous(), eps[nocc:].contiguous()
        self.no, self.nv = nocc, c_ao.shape[1] - nocc
        self.n = self.no * self.nv


class OrbitalHessian:
    """d2E / dkappa2 of a converged `HF` or `KS` calculation as an operator (module docstring for the variables and prefactors).
    `orbitals`: (C_ao, eps) -- or a pair of them per spin -- to use instead of the eigenvectors of the converged Fock matrix
    (canonical orbitals of the same calculation, AO basis, all n orbitals as columns, occupied first).
    `spin`: "singlet" (the Hessian; the only channel of an unrestricted calculation) or "triplet" (restricted only): the spin-flip
    response dD_u = -dD_d of the closed shell, `mm` is then 4 (A+B)^T -- the Hessian along the RHF -> UHF directions."""

    def __init__(self, qc, orbitals=None, spin="singlet"):
        assert qc._has_run, "run() the calculation first"
        if spin not in ("singlet", "triplet"):
            raise ValueError("OrbitalHessian: spin is \"singlet\" or \"triplet\", not %r" % (spin,))
        if spin == "triplet" and qc._engine.polarized:
            raise ValueError("OrbitalHessian: the triplet (spin-flip) response is defined for a restricted closed-shell calculation only; "
                             "spin-flip response of an unrestricted reference is not provided")
        _unsupported(qc)
        self.triplet = spin == "triplet"
        eng = self.eng = qc._engine
        h = self.h = eng.hamilton
        self.polarized = eng.polarized
        self.a = float(eng.exx) if eng.is_ks else 1.0
        self.terms = list(eng.xc.terms) if eng.is_ks else []
        self.nao = h._nao_ao
        if orbitals is None:
            focks = (qc._fock[0], qc._fock[1]) if self.polarized else (qc._fock,)
            orbitals = []
            for f in focks:
                e, c = eng._eigpairs(f)
                orbitals.append((h._orthozer @ c, e))
        elif not self.polarized:
            orbitals = [orbitals]
        nocc = (eng.norb.u, eng.norb.d) if self.polarized else (eng.norb,)
        dev = h.device
        self.spins = [_Spin(torch.as_tensor(c, dtype=torch.float64).to(dev), torch.as_tensor(e, dtype=torch.float64).to(dev), n)
                      for (c, e), n in zip(orbitals, nocc)]
        for s in self.spins:
            if s.nv == 0 or s.no == 0:
                raise NotImplementedError("OrbitalHessian: a spin channel without occupied or without virtual orbitals has no rotations")
        self.occ = 1.0 if self.polarized else 2.0
        self.pref = 2.0 if self.polarized else 4.0
        self.n = sum(s.n for s in self.spins)
        self.diag = torch.cat([(self.pref * (s.ev[:, None] - s.eo[None, :])).reshape(-1) for s in self.spins])
        self.gga = bool(self.terms) and h.xcfamily == 2
        self._rho = None
        if self.terms:  # ground-state density on the grid, once
            self._rho = [lib.grid_density(h._ao, self.nao, lib.pad_matrix(self.occ * (s.co @ s.co.T), h._ld), self.gga) for s in self.spins]

    # -- pieces
    def _split(self, k):
        out, off = [], 0
        for s in self.spins:
            out.append(k[:, off:off + s.n].reshape(-1, s.nv, s.no))
            off += s.n
        return out

    def _vxc_response(self, dds):
        """dds: per spin (nvec, nao, nao) AO response densities -> per spin (nvec, nao, nao) f_xc . d rho in the AO basis"""
        h, nvec = self.h, dds[0].shape[0]
        dens = [[lib.grid_density(h._ao, self.nao, lib.pad_matrix(dd[v], h._ld), self.gga) for v in range(nvec)] for dd in dds]
        drho = [torch.stack([d[0] for d in ds]) for ds in dens]
        dgrho = [torch.stack([d[1] for d in ds]) if self.gga else None for ds in dens]
        if self.triplet:
            pots = [lib.xc_eval_fxc_triplet(self.terms, self._rho[0][0], self._rho[0][1], drho[0], dgrho[0])]
        elif not self.polarized:
            dv, dvg = lib.xc_eval_fxc(self.terms, self._rho[0][0], self._rho[0][1], drho[0], dgrho[0])
            pots = [(dv, dvg)]
        else:
            (ru, gu), (rd, gd) = self._rho
            (dvu, dvd), (dgu, dgd) = lib.xc_eval_fxc_pol(self.terms, ru, rd, gu, gd, drho[0], drho[1], dgrho[0], dgrho[1])
            pots = [(dvu, dgu), (dvd, dgd)]
        n = self.nao
        return [torch.stack([lib.grid_vxc(h._ao, n, h.dvolume, dv[v], None if dvg is None else dvg[v])[:n, :n] for v in range(nvec)])
                for dv, dvg in pots]

    def _products(self, k, plus, minus):
        """(pref (A+B) k, pref (A-B) k) for a block of trial vectors, either None when not asked for; all exchange matrices -- and the
        Coulomb ones of the singlet A+B -- from ONE jk_multi call"""
        k = torch.as_tensor(k, dtype=torch.float64).to(self.h.device)
        assert k.dim() == 2 and k.shape[1] == self.n, "trial vectors are rows of length %d" % self.n
        nvec = k.shape[0]
        if minus and self.a == 0.0:  # a pure functional: A - B is the diagonal, no tile pass
            out_m, minus = self.diag[None, :] * k, False
            if not plus:
                return None, out_m
        else:
            out_m = None
        ks = self._split(k.contiguous())
        nsp = len(self.spins)
        if minus:
            pm = [lib.resp_kappa2dm_pm(kk, s.cv, s.co, self.occ, plus=plus) for kk, s in zip(ks, self.spins)]
            dds, dms = [p[0] for p in pm], [p[1] for p in pm]
        else:
            dds, dms = [lib.resp_kappa2dm(kk, s.cv, s.co, self.occ) for kk, s in zip(ks, self.spins)], None
        tot = None
        if plus and not self.triplet:
            tot = dds[0] if not self.polarized else dds[0] + dds[1]
        # exchange right-hand sides: the spins one after the other, per spin [dD+ (nvec)] or [dD- (nvec)] or, for both, the pairs
        # (dD+[v], dD-[v]) interleaved: a pair shares an NK = 2 pass
        dk, flags = None, None
        if self.a != 0.0:
            if plus and minus:
                dk = torch.cat([torch.stack([dp, dm], dim=1).reshape(2 * nvec, self.nao, self.nao) for dp, dm in zip(dds, dms)])
                flags = [0, 1] * (nvec * nsp)
            elif plus:
                dk = dds[0] if nsp == 1 else torch.cat(dds)
            else:
                dk = dms[0] if nsp == 1 else torch.cat(dms)
                flags = [1] * (nvec * nsp)
        J = K = None
        if tot is not None or dk is not None:
            J, K = lib.jk_multi(self.h._tiles, tot, dk, self.h._multi_work(0 if tot is None else nvec, 0 if dk is None else dk.shape[0]),
                                k_antisym=flags)
        kfac = self.a if self.polarized else 0.5 * self.a
        per = (2 if plus and minus else 1) * nvec  # exchange matrices per spin
        out_p = None
        if plus:
            gs = []
            for i in range(nsp):
                g = J.clone() if (J is not None and i > 0) else J
                if dk is not None:
                    kp = K[i * per:(i + 1) * per]
                    kp = kp[0::2] if minus else kp
                    g = -kfac * kp if g is None else g - kfac * kp
                gs.append(g)
            if self.terms:
                for i, v in enumerate(self._vxc_response(dds)):
                    gs[i] = v if gs[i] is None else gs[i] + v
            out_p = torch.cat([lib.resp_project(g, s.cv, s.co, self.pref, s.ev, s.eo, kk).reshape(nvec, -1)
                               for g, s, kk in zip(gs, self.spins, ks)], dim=1)
        if minus:
            outs = []
            for i, (s, kk) in enumerate(zip(self.spins, ks)):
                km = K[i * per:(i + 1) * per]
                km = km[1::2] if plus else km
                outs.append(lib.resp_project((-kfac) * km, s.cv, s.co, self.pref, s.ev, s.eo, kk).reshape(nvec, -1))
            out_m = torch.cat(outs, dim=1)
        return out_p, out_m

    def mm(self, k):
        """H k = pref (A+B) k for a block of trial vectors k (nvec, n) -> (nvec, n)  [spin="triplet": pref (A+B)^T k]"""
        return self._products(k, True, False)[0]

    def mm_minus(self, k):
        """pref (A-B) k, the scaling of `mm`; the diagonal pref (eps_a - eps_i), without a tile pass, when the exchange fraction is 0"""
        return self._products(k, False, True)[1]

    def mm_pair(self, k):
        """(mm(k), mm_minus(k)) from ONE jk_multi call: K[dD+] and K[dD-] of a trial vector share a pass over the tiles"""
        return self._products(k, True, True)

    def gradient_of(self, op_ao):
        """d2E / dkappa dlambda for a one-electron perturbation lambda . op_ao (AO matrices (m, nao, nao)): pref C_v^T op C_o -> (m, n)"""
        m = op_ao.shape[0]
        return torch.cat([lib.resp_project(op_ao.contiguous(), s.cv, s.co, self.pref).reshape(m, -1) for s in self.spins], dim=1)

    # -- solvers
    def lowest(self, neig=1, tol=1e-6, maxiter=200):
        """the `neig` lowest eigenvalues and eigenvectors of the Hessian (block Davidson, preconditioner pref (eps_a - eps_i));
        `tol`: residual norm |H x - theta x|"""
        theta, x, res = davidson_lowest(self.mm, self.diag, neig=neig, tol=tol, maxiter=maxiter)
        self.last_residual = res
        if not res < tol:  # a Ritz value that has not converged is only an upper bound of the lowest eigenvalue
            warnings.warn("OrbitalHessian.lowest: the Davidson iteration stopped at the residual %.2e (tol %.1e); the value returned "
                          "is an upper bound of the lowest eigenvalue, a stability verdict from it is not safe" % (res, tol))
        return theta, x

    def excite(self, nstates=5, tda=False, tol=1e-6, maxiter=200):
        """the `nstates` lowest excitation energies w (Hartree, ascending) with X+Y and X-Y, rows normalised (X+Y) . (X-Y) = 1
        [tda: A X = w X, X . X = 1, X-Y is None].  Full response with exact exchange: `response_eigs` on `mm_pair`; a pure functional
        (A - B = Delta diagonal): the Hermitian Delta^(1/2) (A+B) Delta^(1/2) Z = w^2 Z by `davidson_lowest`, X+Y = Delta^(1/2) Z /
        sqrt(w); TDA: `davidson_lowest` on ((A+B) + (A-B)) / 2.  `tol`: residual norms.  RuntimeError when an operator is not positive
        definite (the state is not a minimum in this spin channel: is_orb_min)."""
        delta = self.diag / self.pref
        ip = 1.0 / self.pref
        if tda:
            def op(v):
                p, m = self.mm_pair(v)
                return (0.5 * ip) * (p + m)
            w, x, res = davidson_lowest(op, delta, neig=nstates, tol=tol, maxiter=maxiter)
            if not float(w[0]) > 0.0:
                raise RuntimeError("OrbitalHessian.excite: the lowest TDA excitation energy is %.3e, not positive: the SCF state is not "
                                   "a minimum in this spin channel (is_orb_min)" % float(w[0]))
            xpy, xmy = x, None
        elif self.a == 0.0:
            if not float(delta.min()) > 0.0:
                raise RuntimeError("OrbitalHessian.excite: A - B (the orbital-energy differences) is not positive definite: not an "
                                   "aufbau state (is_orb_min)")
            rt = delta.sqrt()
            w2, z, res = davidson_lowest(lambda v: ip * rt * self.mm(rt * v), delta * delta, neig=nstates, tol=tol, maxiter=maxiter)
            if not float(w2[0]) > 0.0:
                raise RuntimeError("OrbitalHessian.excite: A + B is not positive definite (lowest w^2 %.3e): the SCF state is not a "
                                   "minimum in this spin channel (is_orb_min; triplet=True for spin=\"triplet\")" % float(w2[0]))
            w = w2.sqrt()
            xpy, xmy = rt * z / w.sqrt()[:, None], z / rt * w.sqrt()[:, None]
        else:
            def pair(v):
                p, m = self.mm_pair(v)
                return ip * p, ip * m
            w, xpy, xmy, res = response_eigs(pair, delta, neig=nstates, tol=tol, maxiter=maxiter)
        self.last_residual = res
        if not res < tol:
            warnings.warn("OrbitalHessian.excite: the Davidson iteration stopped at the residual %.2e (tol %.1e); the excitation "
                          "energies are not converged" % (res, tol))
        return w, xpy, xmy

    def solve(self, rhs, tol=1e-8, maxiter=200):
        """H x = rhs (rows) by preconditioned conjugate gradients; needs a stable (positive definite) Hessian: RuntimeError when a
        search direction meets non-positive curvature"""
        x, rel = pcg_solve(self.mm, self.diag, torch.as_tensor(rhs, dtype=torch.float64).to(self.h.device), tol=tol, maxiter=maxiter)
        self.last_residual = rel
        if not rel <= tol:
            warnings.warn("OrbitalHessian.solve: conjugate gradients stopped at the relative residual %.2e (tol %.1e)" % (rel, tol))
        return x


def state_memo(qc):
    """the dictionary that holds what has been derived from the CONVERGED STATE `qc` holds now.  Every run() stores a new Fock
    tensor on the calculation (scfloop.store_result), so the memo is tied to the identity of that tensor (a reference to it is kept:
    its id cannot be reused while the memo lives): after another run() -- from another dm0, say, once `is_orb_min` has said no -- the
    memo starts empty."""
    assert qc._has_run, "run() the calculation first"
    held = qc.__dict__.get("_response_memo")
    if held is None or held[0] is not qc._fock:
        held = qc.__dict__["_response_memo"] = (qc._fock, {})
    return held[1]


def orbital_hessian(qc, spin="singlet"):
    """the OrbitalHessian of the converged state of `qc`, memoised on it until the next run()"""
    memo = state_memo(qc)
    key = "operator" if spin == "singlet" else ("operator", spin)
    if key not in memo:
        memo[key] = OrbitalHessian(qc, spin=spin)
    return memo[key]


__all__ = ["OrbitalHessian", "orbital_hessian", "state_memo", "davidson_lowest", "response_eigs", "pcg_solve"]
