"""Coupled-cluster singles and doubles (CCSD) correlation energy of a converged restricted closed-shell Hartree-Fock calculation, every
two-electron integral from the density-fitted tensor (DF-CCSD):  (pq|rs) = sum_P B[p, P, q] B[r, P, s],  B the MO transform of
B[P, mu, nu] (dqc_amd/df.py).  Orbitals i, j, k, l occupied (active), a, b, c, d virtual, real; eps the canonical orbital energies.

THE EQUATIONS AS BUILT: the T1-transformed closed-shell equations (Koch, Christiansen, Sanchez de Meras, Helgaker 1994; Helgaker,
Jorgensen, Olsen ch. 13.7; with fitted integrals DePrince and Sherrill 2013).  Amplitudes t1[i, a] and t2[i, j, a, b] = t_ij^ab
(i -> a, j -> b; t2[i, j, a, b] = t2[j, i, b, a]), u = 2 t2 - t2^T(ab).  The singles enter through dressed orbitals,

    X = 1 - T1^T,  Y = 1 + T1  (T1[a, i] = t1[i, a]),     B~[p, P, q] = sum_p'q' X[p', p] B[p', P, q'] Y[q', q],
    h = diag(eps) - G[B],   G_pq = sum_k 2 (pq|kk) - (pk|kq),      h~ = X^T h Y,      F~ = h~ + G[B~]

(B~ is not symmetric in its outer indices; B~ov = Bov; ~ marks integrals from B~), and the residuals are

    singles  O_ai   = F~_ai + sum_ck u_ik^ac F~_kc + sum_Pd B~vv[a, P, d] Gam[i, P, d] - sum_Pk B~oo[k, P, i] Gam[k, P, a],
                      Gam[i, P, a] = sum_kc u_ik^ac Bov[k, P, c]
    doubles  O_aibj = (ai|bj)~ + sum_cd (ac|bd)~ t_ij^cd                                    the ladder: `ladder`, csrc/cc.hip
                    + sum_kl t_kl^ab [ (ki|lj)~ + sum_cd t_ij^cd (kc|ld) ]
                    + P { -(1/2 + P_ij) sum_ck t_kj^bc [ (ki|ac)~ - 1/2 sum_dl t_li^ad (kd|lc) ]
                          + 1/2 sum_ck u_jk^bc [ L~_aikc + 1/2 sum_dl u_il^ad L_ldkc ]
                          + sum_c t_ij^ac [ F~_bc - sum_dkl u_kl^bd (ld|kc) ] - sum_k t_ik^ab [ F~_kj + sum_cdl u_lj^cd (kd|lc) ] }
    L_pqrs = 2 (pq|rs) - (ps|rq),    P f_aibj = f_aibj + f_bjai,    P_ij: i <-> j
    e_corr = sum_iajb (t_ij^ab + t_i^a t_j^b) L_iajb

The ladder is the only term with four virtual indices; it is evaluated for the pairs i <= j only (W[a, b, c, d] = W[b, a, d, c] because
both factors are the one tensor B~vv: the block (j, i) is the transpose) by a callable `ladder(l, r, x) -> out`, l = r = B~vv as
(nvir, naux, nvir) slabs, x (nvir, nvir, npair) with THE PAIR INDEX LAST, out (npair, nvir, nvir): `lib.cc_ladder` in `ccsd`, an einsum
in the CPU tests.  No tensor with four virtual indices is allocated, and none of nocc nvir^3 either: the three-virtual integrals of the
singles equation are contracted through Gam.  Iteration: t <- t - O / D (D = eps_a - eps_i, eps_a + eps_b - eps_i - eps_j), DIIS on
(t1, t2) with the steps as error vectors; the first iterate is the RI-MP2 amplitudes.  `residual` is max |O| of the returned amplitudes.

Limits: energies and amplitudes only -- no gradient, no density, no Lambda solve, no (T), no unrestricted or Kohn-Sham reference (the
f_ov terms of a non-canonical reference are not built), no autograd (the result is detached).  Memory: B over all active orbitals and
its dressed copy, B~vv padded, about ten tensors of nocc^2 nvir^2 and 2 `diis` more for the history must fit on the device at once.

`ccsd_reference` is the yardstick in another formulation: the spin-orbital equations of Stanton, Gauss, Watts and Bartlett (1991) on
dense antisymmetrised integrals from the same B, plain torch on any device, O(n^4) memory: small cases only."""
import warnings

import torch

from . import lib
from .postscf import aux_key, b_tensor, free_bytes, memoised, orbitals, transform_ov, unsupported


# ---------------------------------------------------------------------------------------------------------------- DIIS
class _Diis:
    """Pulay extrapolation on flat vectors: the last `n` (vector, step) pairs"""

    def __init__(self, n):
        self.n, self.vs, self.es = int(n), [], []

    def __call__(self, v, e):
        if self.n < 2:
            return v
        self.vs.append(v)
        self.es.append(e)
        if len(self.vs) > self.n:
            self.vs.pop(0)
            self.es.pop(0)
        m = len(self.vs)
        if m < 2:
            return v
        a = torch.zeros((m + 1, m + 1), dtype=v.dtype)
        for i in range(m):
            for j in range(i + 1):
                a[i, j] = a[j, i] = float(torch.dot(self.es[i], self.es[j]))
        a[:m, :m] /= a[:m, :m].diagonal().abs().max().clamp_min(1e-300)
        a[m, :m] = a[:m, m] = 1.0
        rhs = torch.zeros(m + 1, dtype=v.dtype)
        rhs[m] = 1.0
        try:
            c = torch.linalg.solve(a, rhs)[:m]
        except RuntimeError:      # a singular history: start it again from this vector
            self.vs, self.es = [v], [e]
            return v
        return sum(float(ci) * vi for ci, vi in zip(c, self.vs))


# ---------------------------------------------------------------------------------------------------------------- the algebra
def einsum_ladder(l, r, x):
    """the contract of `ladder` in plain torch, W stored: l (np, naux, nr), r (nq, naux, ns), x (nr, ns, nvec) -> (nvec, np, nq)"""
    return torch.einsum("pqrs,rsv->vpq", torch.einsum("pkr,qks->pqrs", l, r), x)


def _mean_field(b, no):
    """G_pq = sum_k 2 (pq|kk) - (pk|kq) of a (dressed) tensor b[p, P, q], k over its first `no` orbitals"""
    d = torch.einsum("kpk->p", b[:no, :, :no])
    return 2.0 * torch.einsum("xpq,p->xq", b, d) - torch.einsum("xpk,kpq->xq", b[:, :, :no], b[:no])


def residuals(bmo, eps, nocc, t1, t2, ladder):
    """(O1 (nocc, nvir), O2 (nocc, nocc, nvir, nvir), e_corr) of the module docstring at the amplitudes (t1, t2): bmo (nmo, naux, nmo)
    the tensor over the active orbitals [p, P, q], occupied first, eps (nmo) their energies"""
    no, nmo = int(nocc), int(eps.numel())
    nv = nmo - no
    o, v = slice(0, no), slice(no, nmo)
    x = torch.eye(nmo, dtype=bmo.dtype, device=bmo.device)
    y = x.clone()
    x[o, v] -= t1
    y[v, o] += t1.t()
    bt = torch.einsum("xp,xky->pky", x, torch.einsum("xkz,zy->xky", bmo, y))
    h = torch.diag(eps) - _mean_field(bmo, no)
    f = x.t() @ h @ y + _mean_field(bt, no)
    boo, bov, bvo, bvv = bt[o, :, o], bmo[o, :, v], bt[v, :, o], bt[v, :, v].contiguous()
    u = 2.0 * t2 - t2.transpose(2, 3)
    ovov = torch.einsum("kpc,lpd->kcld", bov, bov)                         # (kc|ld), undressed
    lov = 2.0 * ovov - ovov.transpose(1, 3)                                 # L_kcld
    e_corr = torch.einsum("ijab,iajb->", t2 + torch.einsum("ia,jb->ijab", t1, t1), lov)
    # ---- singles
    gam = torch.einsum("ikac,kpc->ipa", u, bov)
    o1 = f[v, o].t() + torch.einsum("ikac,kc->ia", u, f[o, v]) + torch.einsum("apd,ipd->ia", bvv, gam) - torch.einsum("kpi,kpa->ia", boo, gam)
    # ---- doubles: the ladder on the pairs i <= j
    ii, jj = torch.triu_indices(no, no, device=bmo.device)
    lad = ladder(bvv, bvv, t2[ii, jj].permute(1, 2, 0).contiguous())       # (npair, a, b)
    o2 = torch.einsum("api,bpj->ijab", bvo, bvo)
    o2[jj, ii] += lad.transpose(1, 2)
    off = ii != jj
    o2[ii[off], jj[off]] += lad[off]
    # the hole-hole ladder
    woooo = torch.einsum("kpi,lpj->kilj", boo, boo) + torch.einsum("ijcd,kcld->kilj", t2, ovov)
    o2 += torch.einsum("klab,kilj->ijab", t2, woooo)
    # the symmetrised terms
    cint = torch.einsum("kpi,apc->kiac", boo, bvv) - 0.5 * torch.einsum("liad,kdlc->kiac", t2, ovov)
    yc = torch.einsum("kjbc,kiac->ijab", t2, cint)
    s = -(0.5 * yc + yc.transpose(0, 1))
    dint = 2.0 * torch.einsum("api,kpc->aikc", bvo, bov) - torch.einsum("apc,kpi->aikc", bvv, boo) + 0.5 * torch.einsum("ilad,ldkc->aikc", u, lov)
    s += 0.5 * torch.einsum("jkbc,aikc->ijab", u, dint)
    evv = f[v, v] - torch.einsum("klbd,ldkc->bc", u, ovov)
    eoo = f[o, o] + torch.einsum("ljcd,kdlc->kj", u, ovov)
    s += torch.einsum("ijac,bc->ijab", t2, evv) - torch.einsum("ikab,kj->ijab", t2, eoo)
    o2 += s + s.permute(1, 0, 3, 2)
    return o1, o2, e_corr


def solve(bmo, eps, nocc, ladder, frozen=0, tol=1e-8, maxiter=50, diis=8):
    """the CCSD iteration on plain tensors, on their device: bmo (nmo, naux, nmo) the tensor over ALL orbitals [p, P, q] in energy
    order, eps (nmo), nocc occupied ones of which the lowest `frozen` are left out (the calculation on the tensors without them) ->
    a dict with t1, t2 (the amplitudes `residual` belongs to; active orbitals), e_corr, e_mp2 (the energy of the first iterate), niter
    (residual evaluations), residual (max |O1|, |O2|), converged (residual < tol)"""
    frozen = int(frozen)
    if frozen:
        bmo, eps, nocc = bmo[frozen:, :, frozen:].contiguous(), eps[frozen:].contiguous(), int(nocc) - frozen
    no, nmo = int(nocc), int(eps.numel())
    nv = nmo - no
    eo, ev = eps[:no], eps[no:]
    d1 = ev[None, :] - eo[:, None]
    d2 = d1[:, None, :, None] + d1[None, :, None, :]
    t1 = torch.zeros((no, nv), dtype=bmo.dtype, device=bmo.device)
    t2 = torch.zeros((no, no, nv, nv), dtype=bmo.dtype, device=bmo.device)
    hist = _Diis(diis)
    e_mp2 = e_corr = None
    res, niter, done = float("inf"), 0, False
    while niter < int(maxiter):
        o1, o2, e = residuals(bmo, eps, no, t1, t2, ladder)
        niter += 1
        res = max(float(o1.abs().max()), float(o2.abs().max()))
        if niter > 1:
            e_corr = e
            if niter == 2:
                e_mp2 = e
            if res < tol:
                done = True
                break
        n1, n2 = t1 - o1 / d1, t2 - o2 / d2
        step = torch.cat([(n1 - t1).reshape(-1), (n2 - t2).reshape(-1)])
        vec = hist(torch.cat([n1.reshape(-1), n2.reshape(-1)]), step) if niter > 1 else torch.cat([n1.reshape(-1), n2.reshape(-1)])
        t1, t2 = vec[:no * nv].view(no, nv).clone(), vec[no * nv:].view(no, no, nv, nv).clone()
    if e_corr is None or not done:   # the amplitudes of the last update have not been looked at: their energy and residual
        o1, o2, e_corr = residuals(bmo, eps, no, t1, t2, ladder)
        res = max(float(o1.abs().max()), float(o2.abs().max()))
        e_mp2 = e_corr if e_mp2 is None else e_mp2
        done = res < tol
    return {"t1": t1, "t2": t2, "e_corr": e_corr.reshape(1), "e_mp2": e_mp2.reshape(1), "niter": niter, "residual": res, "converged": done}


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def spin_orbital_amplitudes(t1, t2):
    """the spin-adapted (t1 (no, nv), t2 (no, no, nv, nv)) in spin orbitals, alpha block first: (2 no, 2 nv), (2 no, 2 no, 2 nv, 2 nv)"""
    no, nv = (int(n) for n in t1.shape)
    s1 = torch.zeros((2 * no, 2 * nv), dtype=t1.dtype, device=t1.device)
    s2 = torch.zeros((2 * no, 2 * no, 2 * nv, 2 * nv), dtype=t1.dtype, device=t1.device)
    a, b = slice(0, no), slice(no, 2 * no)
    av, bv = slice(0, nv), slice(nv, 2 * nv)
    s1[a, av] = s1[b, bv] = t1
    same = t2 - t2.transpose(2, 3)
    s2[a, a, av, av] = s2[b, b, bv, bv] = same
    s2[a, b, av, bv] = s2[b, a, bv, av] = t2
    s2[a, b, bv, av] = s2[b, a, av, bv] = -t2.transpose(2, 3)
    return s1, s2


def ccsd_reference(bmo, eps, nocc, tol=1e-10, maxiter=200):
    """(e_corr, residual_fn) of the spin-orbital CCSD equations of Stanton, Gauss, Watts and Bartlett (J. Chem. Phys. 94, 4334 (1991))
    on dense antisymmetrised integrals <pq||rs> from bmo (nmo, naux, nmo), Fock matrix diag(eps), spin orbitals alpha block first
    within the occupied and within the virtual ones.  e_corr: the equations iterated here (their own amplitudes, DIIS) until the
    largest residual is below tol.  residual_fn(t1 (2 no, 2 nv), t2 (2 no, 2 no, 2 nv, 2 nv)) -> (r1, r2): the UNSCALED residuals
    <ia|Hbar|0>, <ijab|Hbar|0> of any amplitudes (`spin_orbital_amplitudes` expands spin-adapted ones)."""
    no, nmo = int(nocc), int(eps.numel())
    nv = nmo - no
    dt, dev = bmo.dtype, bmo.device
    sp = torch.cat([torch.arange(no), torch.arange(no), torch.arange(no, nmo), torch.arange(no, nmo)]).to(dev)
    spin = torch.cat([torch.zeros(no), torch.ones(no), torch.zeros(nv), torch.ones(nv)]).to(dev)
    bs = bmo[sp][:, :, sp]
    same = (spin[:, None] == spin[None, :]).to(dt)
    chem = torch.einsum("pkr,qks->prqs", bs * same[:, None, :], bs * same[:, None, :])     # (pr|qs) with the spin deltas
    phys = chem.permute(0, 2, 1, 3)                                                         # <pq|rs>
    g = (phys - phys.permute(0, 1, 3, 2)).contiguous()
    fd = eps[sp]
    n = 2 * no
    o, v = slice(0, n), slice(n, 2 * nmo)
    d1 = fd[o, None] - fd[None, v]
    d2 = d1[:, None, :, None] + d1[None, :, None, :]
    fov = torch.zeros((n, 2 * nv), dtype=dt, device=dev)       # canonical orbitals: the Fock matrix is diagonal
    pab = lambda z: z - z.permute(0, 1, 3, 2)  # noqa: E731
    pij = lambda z: z - z.permute(1, 0, 2, 3)  # noqa: E731

    def residual_fn(t1, t2):
        tt = torch.einsum("ia,jb->ijab", t1, t1)
        tt = tt - tt.permute(0, 1, 3, 2)
        taut, tau = t2 + 0.5 * tt, t2 + tt
        oovv = g[o, o, v, v]
        fae = -0.5 * torch.einsum("me,ma->ae", fov, t1) + torch.einsum("mf,mafe->ae", t1, g[o, v, v, v]) - 0.5 * torch.einsum("mnaf,mnef->ae", taut, oovv)
        fmi = 0.5 * torch.einsum("ie,me->mi", t1, fov) + torch.einsum("ne,mnie->mi", t1, g[o, o, o, v]) + 0.5 * torch.einsum("inef,mnef->mi", taut, oovv)
        fme = fov + torch.einsum("nf,mnef->me", t1, oovv)
        wmnij = g[o, o, o, o] + (lambda z: z - z.permute(0, 1, 3, 2))(torch.einsum("je,mnie->mnij", t1, g[o, o, o, v])) + 0.25 * torch.einsum("ijef,mnef->mnij", tau, oovv)
        wabef = g[v, v, v, v] - (lambda z: z - z.permute(1, 0, 2, 3))(torch.einsum("mb,amef->abef", t1, g[v, o, v, v])) + 0.25 * torch.einsum("mnab,mnef->abef", tau, oovv)
        wmbej = g[o, v, v, o] + torch.einsum("jf,mbef->mbej", t1, g[o, v, v, v]) - torch.einsum("nb,mnej->mbej", t1, g[o, o, v, o]) \
            - torch.einsum("jnfb,mnef->mbej", 0.5 * t2 + torch.einsum("jf,nb->jnfb", t1, t1), oovv)
        r1 = fov + torch.einsum("ie,ae->ia", t1, fae) - torch.einsum("ma,mi->ia", t1, fmi) + torch.einsum("imae,me->ia", t2, fme) \
            - torch.einsum("nf,naif->ia", t1, g[o, v, o, v]) - 0.5 * torch.einsum("imef,maef->ia", t2, g[o, v, v, v]) \
            - 0.5 * torch.einsum("mnae,nmei->ia", t2, g[o, o, v, o]) - d1 * t1
        r2 = oovv + pab(torch.einsum("ijae,be->ijab", t2, fae - 0.5 * torch.einsum("mb,me->be", t1, fme))) \
            - pij(torch.einsum("imab,mj->ijab", t2, fmi + 0.5 * torch.einsum("je,me->mj", t1, fme))) \
            + 0.5 * torch.einsum("mnab,mnij->ijab", tau, wmnij) + 0.5 * torch.einsum("ijef,abef->ijab", tau, wabef) \
            + pij(pab(torch.einsum("imae,mbej->ijab", t2, wmbej) - torch.einsum("ie,ma,mbej->ijab", t1, t1, g[o, v, v, o]))) \
            + pij(torch.einsum("ie,abej->ijab", t1, g[v, v, v, o])) - pab(torch.einsum("ma,mbij->ijab", t1, g[o, v, o, o])) - d2 * t2
        return r1, r2

    def energy(t1, t2):
        return 0.25 * torch.einsum("ijab,ijab->", g[o, o, v, v], t2) + 0.5 * torch.einsum("ijab,ia,jb->", g[o, o, v, v], t1, t1)

    t1 = torch.zeros((n, 2 * nv), dtype=dt, device=dev)
    t2 = torch.zeros((n, n, 2 * nv, 2 * nv), dtype=dt, device=dev)
    hist = _Diis(8)
    for _ in range(int(maxiter)):
        r1, r2 = residual_fn(t1, t2)
        if max(float(r1.abs().max()), float(r2.abs().max())) < tol:
            break
        s1, s2 = r1 / d1, r2 / d2
        vec = hist(torch.cat([(t1 + s1).reshape(-1), (t2 + s2).reshape(-1)]), torch.cat([s1.reshape(-1), s2.reshape(-1)]))
        t1, t2 = vec[:t1.numel()].view(t1.shape).clone(), vec[t1.numel():].view(t2.shape).clone()
    else:
        raise RuntimeError("ccsd_reference: not converged in %d iterations" % int(maxiter))
    return energy(t1, t2), residual_fn


# ---------------------------------------------------------------------------------------------------------------- the method
class CCSD:
    """what `ccsd` returns (detached tensors): `e_corr`, `e_tot = qc.energy() + e_corr`, `e_mp2` (the energy of the first iterate: the
    RI-MP2 correlation energy) -- one-element tensors; `t1` (nocc, nvir), `t2` (nocc, nocc, nvir, nvir) with t2[i, j, a, b] =
    t2[j, i, b, a] (active orbitals); `t1_diagnostic` = |t1|_F / sqrt(nocc); `converged`, `niter`, `residual` (the largest absolute
    element of the residual equations at these amplitudes, not of the last step); `naux`, `frozen`; `df`: the DFMI355 object whose
    tensor was used"""

    def __init__(self, e_scf, sol, frozen, df):
        self.e_corr, self.e_mp2, self.t1, self.t2 = sol["e_corr"], sol["e_mp2"], sol["t1"], sol["t2"]
        self.e_scf = e_scf
        self.e_tot = e_scf + self.e_corr
        self.t1_diagnostic = float(self.t1.norm()) / max(int(self.t1.shape[0]), 1) ** 0.5
        self.converged, self.niter, self.residual = bool(sol["converged"]), int(sol["niter"]), float(sol["residual"])
        self.frozen, self.df, self.naux = int(frozen), df, int(df._b.shape[0])

    def __repr__(self):
        return "CCSD(e_corr=%.10f, e_mp2=%.10f, e_tot=%.10f, t1_diagnostic=%.4f, niter=%d, residual=%.1e, converged=%s, frozen=%d, naux=%d)" % (
            float(self.e_corr), float(self.e_mp2), float(self.e_tot), self.t1_diagnostic, self.niter, self.residual, self.converged,
            self.frozen, self.naux)


def _refusals(qc, frozen, auxbasis, tol, maxiter):
    """everything `ccsd` refuses, from the attributes of the calculation alone"""
    if frozen < 0:
        raise ValueError("ccsd: frozen must be >= 0, got %d" % frozen)
    if not tol > 0.0:
        raise ValueError("ccsd: tol must be positive, got %g" % tol)
    if maxiter < 1:
        raise ValueError("ccsd: maxiter must be >= 1, got %d" % maxiter)
    eng = qc._engine
    if eng.polarized:
        raise NotImplementedError("ccsd: an unrestricted calculation is not supported (restricted closed shell only; run the closed "
                                  "shell restricted)")
    if getattr(eng, "is_ks", False):
        raise NotImplementedError("ccsd: a Kohn-Sham reference is not supported (the Fock matrix of the Hartree-Fock operator is not "
                                  "diagonal in Kohn-Sham orbitals and the f_ov terms are not built); run Hartree-Fock")
    unsupported(qc, "ccsd")
    df = getattr(eng.hamilton, "df", None)
    if df is not None and not getattr(df, "exchange", False) and auxbasis is None:
        raise NotImplementedError("ccsd: the Hamiltonian's density fit is for the Coulomb term only (densityfit() without "
                                  "exchange=True); pass auxbasis= for the tensor of the correlation treatment")
    w = eng.orb_weight
    nocc = int((w != 0).sum())
    if nocc - frozen < 1:
        raise NotImplementedError("ccsd: no occupied orbital is left after freezing %d of %d" % (frozen, nocc))
    nmo = getattr(eng, "shape", (None,))[-1]
    if nmo is not None and int(nmo) - nocc < 1:
        raise NotImplementedError("ccsd: the calculation has no virtual orbitals (%d orbitals, %d occupied)" % (int(nmo), nocc))


def _compute(qc, frozen, auxbasis, tol, maxiter, diis):
    df = b_tensor(qc, auxbasis)
    b = df._b
    co, cv, eo, ev = orbitals(qc, 0)[0]
    nocc, nv, naux = int(co.shape[1]), int(cv.shape[1]), int(b.shape[0])
    no = nocc - frozen
    if no < 1 or nv < 1:
        raise NotImplementedError("ccsd: no occupied or no virtual orbitals are left (nocc = %d, frozen = %d, nvir = %d)" % (nocc, frozen, nv))
    nmo, ldv = nocc + nv, (nv + 15) // 16 * 16
    sizes = (8 * nv * naux * ldv, 8 * nmo * naux * nmo, 8 * no * no * nv * nv)
    need = sizes[0] + 3 * sizes[1] + (10 + 2 * max(int(diis), 0)) * sizes[2]
    free = free_bytes(b.device)
    if need > free:
        raise lib.DqcAmdError(
            "ccsd: the padded tensor Bvv (nvir = %d, naux = %d, padded to %d: %.2f GB), three tensors of the size of B over the %d "
            "orbitals (%.2f GB each) and %d tensors of nocc^2 nvir^2 (active nocc = %d: %.2f GB each, the DIIS history among them) need %.2f GB "
            "but only %.2f GB of device memory are free: freeze more orbitals, use a smaller auxiliary basis or a shorter DIIS history"
            % (nv, naux, ldv, sizes[0] / 1e9, nmo, sizes[1] / 1e9, 10 + 2 * max(int(diis), 0), no, sizes[2] / 1e9, need / 1e9, free / 1e9))
    c = torch.cat([co, cv], dim=1)
    bmo = transform_ov(b, c, c)[:, :, :nmo].contiguous()
    pad = torch.zeros((nv, naux, ldv), dtype=b.dtype, device=b.device)

    def ladder(l, r, x):   # (l is r: the dressed Bvv) the slabs padded to the kernel's leading dimension
        pad[:, :, :nv] = l
        return lib.cc_ladder(pad, pad, x, nv, nv)

    sol = solve(bmo, torch.cat([eo, ev]), nocc, ladder, frozen=frozen, tol=tol, maxiter=maxiter, diis=diis)
    return df, {k: (t.detach() if torch.is_tensor(t) else t) for k, t in sol.items()}


def ccsd(qc, frozen=0, auxbasis=None, tol=1e-8, maxiter=50, diis=8):
    """CCSD correlation energy and amplitudes of the converged restricted closed-shell Hartree-Fock calculation `qc` with density-fitted
    integrals (module docstring): a `CCSD` result object.
    frozen: the lowest `frozen` occupied orbitals are left out of the correlation treatment.  auxbasis: as `mp2` takes it (used when
    the Hamiltonian carries no fitted-exchange tensor; a Hamiltonian built with densityfit(exchange=True) uses its own; a Coulomb-only
    fit needs it).  tol: the largest absolute element of the residual equations at convergence; maxiter: residual evaluations at
    most -- a calculation that has not converged warns (UserWarning, with the residual) and returns converged=False; diis: length of
    the DIIS history (< 2: none).  The particle-particle ladder runs on the fused kernel dqc_cc_ladder (csrc/cc.hip), once per
    iteration; everything else is library GEMMs.  Memoised on the converged state per argument set; nothing is differentiable."""
    frozen, tol, maxiter, diis = int(frozen), float(tol), int(maxiter), int(diis)
    _refusals(qc, frozen, auxbasis, tol, maxiter)
    assert qc._has_run, "run() the calculation first"
    key = ("ccsd", frozen, aux_key(qc, auxbasis), tol, maxiter, diis)
    df, sol = memoised(qc, key, lambda: _compute(qc, frozen, auxbasis, tol, maxiter, diis))
    if not sol["converged"]:
        warnings.warn("ccsd: not converged in %d iterations: the largest residual is %.3e (tol %.1e); raise maxiter"
                      % (sol["niter"], sol["residual"], tol), UserWarning, stacklevel=2)
    memo_key = ("ccsd_result",) + key[1:]
    return memoised(qc, memo_key, lambda: CCSD(qc.energy().detach().reshape(1), sol, frozen, df))


# `dqc_amd.ccsd` is this function once the package has imported it: the algebra and the yardstick stay reachable as dqc_amd.ccsd.solve ...
ccsd.solve = solve
ccsd.residuals = residuals
ccsd.einsum_ladder = einsum_ladder
ccsd.ccsd_reference = ccsd_reference
ccsd.spin_orbital_amplitudes = spin_orbital_amplitudes

__all__ = ["ccsd", "CCSD", "solve", "residuals", "einsum_ladder", "ccsd_reference", "spin_orbital_amplitudes"]
