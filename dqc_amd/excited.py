"""Analytic nuclear gradients and relaxed one-particle properties of CIS and TDHF excited states (restricted closed-shell
Hartree-Fock reference): d(E_SCF + w) / dR by the Z-vector method (Furche and Ahlrichs, J. Chem. Phys. 117, 7433 (2002), without
the exchange-correlation terms), with the two-electron part on the bilinear derivative pass dqc_eri_grad2 (csrc/grad.hip, grad2.hip).

Variables: those of dqc_amd/response.py -- spatial orbitals, U = X+Y and V = X-Y as (nocc, nvir) matrices with U . V = 1 (TDA / CIS:
U = V = X, X . X = 1).  i, j occupied, a, b virtual, p, q any orbital; mu, nu, ... AOs.  The functional

    w[C, U, V] = 1/2 [U^T (A+B) U + V^T (A-B) V]
    singlet  (A+B)_ia,jb = d_ij F_ab - d_ab F_ij + 4 (ia|jb) - (ib|ja) - (ij|ab)        (A-B)_ia,jb = d_ij F_ab - d_ab F_ij + (ib|ja) - (ij|ab)
    triplet  the same without 4 (ia|jb)

is stationary in U and V under the normalisation (its value there is the excitation energy) but not in the orbitals.  Written in the
AO basis with  R+- = C_o (U, V) C_v^T,  S = (R+ + R+^T) / 2  (symmetric),  N = (R- - R-^T) / 2  (antisymmetric):

    w = tr[T F] + E2,     T_ab = 1/2 sum_i (U_ia U_ib + V_ia V_ib),    T_ij = -1/2 sum_a (U_ia U_ja + V_ia V_ja)      (no ov block)
    E2 = sum (ab|cd) [2 S_ab S_cd - S_ac S_bd - N_ac N_bd]         (triplet: without 2 S S; the cross terms S . N vanish)
       = 1/2 tr[S G+] + 1/2 tr[N^T G-],      G+ = 4 J[S] - 2 K[S]  (triplet -2 K[S]),   G- = -2 K[N]   (K[M]_pq = (pr|qs) M_rs; G- antisymmetric)

[sum_ijab U_ia U_jb (ia|jb) = sum S S (ab|cd);  sum S_ac S_bd (ab|cd) = 1/2 sum U U [(ij|ab) + (ib|ja)];  sum N_ac N_bd (ab|cd) = 1/2 sum V V
[(ij|ab) - (ib|ja)].]  F = h + G[D], G[D] = J[D] - K[D] / 2, D = 2 C_o C_o^T, so tr[T F] = tr[Tbar h] + tr[D G[Tbar]], Tbar = C T C^T.

Derivative by the orbitals, as the matrix Gm[p, q] = C_p^T dw / dC_q (canonical orbitals):

    Gm[p, q]  = 2 eps_p T_pq                                                 (the outer orbitals of tr[T C^T F C])
    Gm[p, i] += 4 (C^T G[Tbar] C_o)_pi                                       (F follows D)
    Gm[p, i] += sum_a (g+_pa U_ia + g-_pa V_ia)      Gm[p, a] += sum_i (g+_ip U_ia + g-_ip V_ia)      g+- = C^T G+- C     (`coupling`)

(dE2 = sum dR+_ab G+_ab + sum dR-_ab G-_ab: the symmetric / antisymmetric parts select themselves.)  Under a rotation kappa_ai (dC_i =
sum_a C_a kappa_ai, dC_a = -sum_i C_i kappa_ai: response.OrbitalHessian) w changes by R . kappa with

    R_ai = Gm[a, i] - Gm[i, a] = 4 (C_v^T G[Tbar] C_o)_ai + sum_b (g+_ab U_ib + g-_ab V_ib) - sum_j (g+_ji U_ja + g-_ji V_ja)

The SCF condition 4 F_ai = 0 moves the orbitals with a perturbation; the Lagrangian w + sum_ai z_ai 4 F_ai is stationary in kappa for

    H z = -R      (H = 4 (A+B) of the SINGLET channel -- the orbital Hessian -- for triplet states too: the relaxation is a singlet),

and sum z_ai 4 F_ai = tr[Z F] with Z_ai = Z_ia = 2 z_ai: the relaxed difference density is P = T + Z, and everything above holds for the
Lagrangian with P in place of T in the first two lines of Gm.  What is left of dC / dR is the re-orthonormalisation dC = -1/2 C (C^T dS C),
which meets the Lagrangian through W = C 1/4 (Gm + Gm^T) C^T.  With Pbar = C P C^T:

    d w / dR = tr[Pbar dh] - tr[W dS]                                                                          -> lib.int1e_grad
             + separable       d_integrals tr[Pbar G[D]]    = 2 eri_grad2(D, Pbar, 1, 1)                        -> lib.eri_grad2
             + non-separable   d_integrals E2               = eri_grad2(S, S, 4, 4) + eri_grad2(N, N, 0, 4)    (triplet: (S, S, 0, 4))

[eri_grad2(A, B, j, k) = sum_{a on the atom} (d a b|c d) [j (A_ab B_cd + B_ab A_cd) - k / 2 (A_ac B_bd + B_ac A_bd)]; a two-particle density
invariant under (ab) <-> (cd) and a <-> b, c <-> d has a quarter of its derivative on the first index, so sum (ab|cd) Gamma_abcd
differentiates to 4 sum (d a b|c d) Gamma_abcd: Gamma = 1/2 (P_ab D_cd + D_ab P_cd) - 1/4 (P_ac D_bd + D_ac P_bd) and Gamma = 2 S S - S S - N N
give the factors above.]  A one-electron perturbation lambda O has d w / d lambda = tr[Pbar O]: the relaxed excited-state dipole moment is
that of D + Pbar.

The algebra lives in functions of plain tensors (`difference_density`, `transition_densities`, `lagrangian_rhs` here; `relaxed_density_mo`
and `energy_weighted` in dqc_amd/postscf.py, which the MP2 gradient shares with this one, as it does the Z-vector solve and the terms of
a relaxed density) that take a callable for J and K, so that tests/test_excited_gradient_cpu.py drives them with dense oracle integrals;
the factors are held against finite differences there and in tests/test_gpu_excited_gradient.py.

KOHN-SHAM references (LDA, GGA, global hybrids; singlet states; `tddft_gradient`).  a = the exact-exchange fraction; on the grid, with
(v, u) the potentials of the ground state (v_rho, 2 v_sigma grad rho), V1[M] = the f_xc matrix of rho_M (OrbitalHessian._vxc_response;
per point (v1, u1)[M] = lib.xc_eval_fxc) and V2[M, M'] = the matrix of the second-order change (v2, u2) = lib.xc_eval_kxc of the
potentials under (rho_M, rho_M') (csrc/xc.hip: the third functional derivative), both through lib.grid_vxc:

    (A+-B): every exchange integral times a;   4 (ia|jb) -> 4 (ia|jb) + 4 (ia|f_xc|jb)
    E2 += 2 tr[S V1[S]]          G+ = 4 J[S] - 2 a K[S] + 4 V1[S]          G- = -2 a K[N]          G[X] = J[X] - a / 2 K[X] + V1[X]
    f_xc follows D:  dE2_xc / dD = 2 V2[S, S],  D = 2 C_o C_o^T   =>   G[Tbar] -> G[Tbar] + 2 V2[S, S]  in R, and so in the g_pbar of W

    d w / dR = tr[Pbar dh] - tr[W dS] + eri_grad2(D, Pbar, 2, 2 a) + eri_grad2(S, S, 4, 4 a) + eri_grad2(N, N, 0, 4 a)   (a = 0: no N pass)
             + dL_xc,     L_xc = sum_g w_g { v rho_Pbar + u . grad rho_Pbar + 2 (v1[S] rho_S + u1[S] . grad rho_S) }
    dL_xc = G(Pbar; v, u) + G(S; 4 v1[S], 4 u1[S]) + G(D; v1[Pbar] + 2 v2, u1[Pbar] + 2 u2) + sum_g dw_g {...}

G(M; a, b) = sum_g w [a d rho_M + b . d grad rho_M] at fixed M with AO centres and grid points riding on their atoms
(gradient._xc_potential_gradient: the terms (ii), (iii) of gradient._xc_gradient); the third G is the change of the potentials with
rho_D, moved onto D by the symmetry of the second and third derivatives; the last term is the Becke-weight derivative with {...} held
fixed (gradient._xc_weight_gradient).  The factors are held against orbital rotations of a toy grid functional
(tests/test_tddft_gradient_cpu.py) and against finite differences (tests/test_gpu_tddft_gradient.py).  Triplets of a Kohn-Sham
reference need the spin-polarised third-order kernel, meta-GGAs an orbital response: both are refused."""
import torch

from . import lib
from .postscf import cart_part, energy_weighted, memoised, relaxed_density_mo, relaxed_terms, stage_clock, z_vector  # noqa: F401


# ------------------------------------------------------------------------------------------------ algebra on plain tensors
def difference_density(u, v):
    """(T_oo (no, no), T_vv (nv, nv)): the unrelaxed difference density of the module docstring; u = X+Y, v = X-Y as (no, nv)"""
    return -0.5 * (u @ u.T + v @ v.T), 0.5 * (u.T @ u + v.T @ v)


def transition_densities(u, v, co, cv):
    """(S, N): the symmetric part of R+ = C_o (X+Y) C_v^T and the antisymmetric part of R- = C_o (X-Y) C_v^T, AO basis"""
    rp, rm = co @ u @ cv.T, co @ v @ cv.T
    return 0.5 * (rp + rp.T), 0.5 * (rm - rm.T)


def lagrangian_rhs(u, v, co, cv, jk, triplet=False, xc=None, kfrac=1.0):
    """(R (nv, no), parts): R_ai = dw / dkappa_ai at fixed X, Y, from the Fock-type matrices G+[S], G-[N] and G[Tbar] of ONE call
    jk(dms_j (nj, nao, nao), dms_k (nk, nao, nao), k_antisym) -> (J, K) -- the contract of lib.jk_multi: plain J and K, the flagged
    exchange densities antisymmetric.  parts: what the gradient needs again (t_oo, t_vv, tbar, s, n, g_t = G[Tbar], coupling = the
    (n, n) MO matrix of the g+- terms of Gm).  Kohn-Sham (singlet): kfrac = the exact-exchange fraction a on every K, and xc(ms (m, nao,
    nao), s) -> (V1[ms] (m, nao, nao), V2[s, s] (nao, nao)), the f_xc matrices of the densities ms and the third-order matrix of
    (rho_s, rho_s): G[Tbar] gains V1[Tbar] + 2 V2[S, S], G+ gains 4 V1[S] (module docstring); parts gains v2.  With the defaults
    (Hartree-Fock) the arithmetic is what it was without them, bit for bit."""
    no = int(co.shape[1])
    t_oo, t_vv = difference_density(u, v)
    tbar = cv @ t_vv @ cv.T + co @ t_oo @ co.T
    s, n = transition_densities(u, v, co, cv)
    dms_j = torch.stack([tbar] if triplet else [tbar, s])
    J, K = jk(dms_j, torch.stack([tbar, s, n]), [0, 0, 1])
    g_t = J[0] - (0.5 * kfrac) * K[0]
    g_p = (-2.0 * kfrac) * K[1] if triplet else 4.0 * J[1] - (2.0 * kfrac) * K[1]
    g_m = (-2.0 * kfrac) * K[2]
    v2 = None
    if xc is not None:
        assert not triplet, "the exchange-correlation terms are those of the singlet Lagrangian"
        v1, v2 = xc(torch.stack([tbar, s]), s)
        g_t = g_t + v1[0] + 2.0 * v2
        g_p = g_p + 4.0 * v1[1]
    c = torch.cat([co, cv], dim=1)
    gp, gm = c.T @ g_p @ c, c.T @ g_m @ c
    coupling = torch.cat([gp[:, no:] @ u.T + gm[:, no:] @ v.T, gp[:no, :].T @ u + gm[:no, :].T @ v], dim=1)
    rhs = 4.0 * (cv.T @ g_t @ co) + coupling[no:, :no] - coupling[:no, no:].T
    return rhs, dict(t_oo=t_oo, t_vv=t_vv, tbar=tbar, s=s, n=n, g_t=g_t, coupling=coupling, v2=v2)


# ------------------------------------------------------------------------------------------------ the calculation
class ExcitedDensity:
    """the relaxed difference density of an excited state (detached tensors on the device of the calculation): `dm_mo` (n, n) = P = T + Z
    in the basis of the canonical orbitals (energy order), `unrelaxed_mo` = T alone, `dm_ao` = the SCF density plus C P C^T;
    `dipole(unit)`: the relaxed excited-state dipole moment"""

    def __init__(self, dm_mo, unrelaxed_mo, dm_ao, dip_au):
        self.dm_mo, self.unrelaxed_mo, self.dm_ao, self._dip_au = dm_mo, unrelaxed_mo, dm_ao, dip_au

    def dipole(self, unit="Debye"):
        """electric dipole moment (3,) of the excited state, nuclear part included: sign and units of `properties.edipole`"""
        from .properties import _DIPOLE_UNITS, _unit
        return self._dip_au * _unit(_DIPOLE_UNITS, unit, "dipole")


class ExcitedGradient:
    """what `excited_gradient` returns (detached tensors on the device of the calculation): `gradient` (natm, 3) = d(E_SCF + w) / dR in
    Hartree / Bohr, `scf` (equal to qc.nuclear_gradient()) and `excitation` = dw / dR; `omega` (one element) and `e_tot` = qc.energy() +
    omega; `xpy`, `xmy` (nv * no,) as `excitations` returns them (TDA: xmy = xpy = X); `density`: the `ExcitedDensity`; `z_residual` (the
    relative residual the Z-vector solve stopped at); `state`, `spin`, `tda`"""

    def __init__(self, gradient, scf, omega, e_tot, xpy, xmy, density, z_residual, state, spin, tda):
        self.gradient, self.scf, self.excitation = gradient, scf, gradient - scf
        self.omega, self.e_tot, self.xpy, self.xmy, self.density = omega, e_tot, xpy, xmy, density
        self.z_residual, self.state, self.spin, self.tda = z_residual, int(state), spin, bool(tda)

    def __repr__(self):
        return "ExcitedGradient(state %d, %s%s, omega=%.8f, max |g| = %.3e, max |dw/dR| = %.3e)" % (
            self.state, self.spin, ", TDA" if self.tda else "", float(self.omega), float(self.gradient.abs().max()),
            float(self.excitation.abs().max()))


def _refusals(qc, who, spin, kohn_sham):
    """what `who` (excited_gradient, tddft_gradient) refuses before anything runs; kohn_sham: whether it takes a Kohn-Sham reference"""
    from .response import _unsupported
    if spin not in ("singlet", "triplet"):
        raise ValueError("%s: spin is \"singlet\" or \"triplet\", not %r" % (who, spin))
    eng = qc._engine
    if eng.is_ks and not kohn_sham:
        raise NotImplementedError(who + ": a Kohn-Sham reference (hybrid functionals included) is not taken here: the TDDFT "
                                  "Lagrangian with the third-order exchange-correlation kernel is behind its own name -- use tddft_gradient")
    if eng.polarized:
        raise NotImplementedError(who + ": unrestricted calculations are not supported (the restricted closed-shell "
                                  "Lagrangian only; the spin-resolved one is not built)")
    if eng.is_ks:
        if spin == "triplet":
            raise NotImplementedError(who + ": triplet states of a Kohn-Sham reference are not supported: they need the "
                                      "spin-polarised third-order exchange-correlation kernel, which is not built (singlets only)")
        if any(name.startswith("mgga_") for _, name in getattr(eng.xc, "terms", ())):
            raise NotImplementedError(who + ": meta-GGA functionals are not supported (they have no orbital response: "
                                      "no second- or third-order kernel)")
    _unsupported(qc)


def _xc_matrices(op, with_kxc):
    """the `xc` callable of lagrangian_rhs on the grid of the Hamiltonian, from the singlet OrbitalHessian `op` of a Kohn-Sham
    calculation: V1 = its f_xc matrices, V2[S, S] = dqc_xc_eval_kxc at (rho_S, rho_S) -> dqc_grid_vxc (zero with with_kxc=False)"""
    h, nao = op.h, op.nao

    def xc(ms, s):
        v1 = op._vxc_response([ms.contiguous()])[0]
        if not with_kxc:
            return v1, torch.zeros_like(s)
        rs, gs = lib.grid_density(h._ao, nao, lib.pad_matrix(s, h._ld), op.gga)
        rho, grho = op._rho[0]
        gs1 = gs.unsqueeze(0) if op.gga else None
        d2v, d2vg = lib.xc_eval_kxc(op.terms, rho, grho if op.gga else None, rs.unsqueeze(0), gs1, rs.unsqueeze(0), gs1)
        return v1, lib.grid_vxc(h._ao, nao, h.dvolume, d2v[0], None if d2vg is None else d2vg[0])[:nao, :nao]
    return xc


def _xc_gradient_terms(qc, op, pbar, s, d_scf, with_kxc, clock):
    """(dL_xc (natm, 3), seconds of the three grid passes, seconds of the weight term): the exchange-correlation terms of the
    TDDFT gradient (module docstring, last section)"""
    from .gradient import _xc_potential_gradient, _xc_weight_gradient
    from .utils.datastruct import ValGrad
    eng = qc._engine
    h = eng.hamilton
    gga, nao = op.gga, op.nao
    tic = clock()
    ao = lib.eval_gto(h._tab, h.rgrid, 3 if gga else 1)       # once for the three passes: (10 | 4, ngrid, ld)
    dens = lambda m: lib.grid_density(ao[:4], nao, lib.pad_matrix(m, h._ld), gga)  # noqa: E731
    rho, grho = dens(d_scf)
    (rp, gp), (rs, gs) = dens(pbar), dens(s)
    pot = h.xc.get_vxc(ValGrad(value=rho, grad=grho if gga else None))
    v, u = pot.value, pot.grad if gga else None
    v1, u1 = lib.xc_eval_fxc(op.terms, rho, grho, torch.stack([rp, rs]), torch.stack([gp, gs]) if gga else None)
    vd, ud = v1[0], u1[0] if gga else None
    if with_kxc:
        gs1 = gs.unsqueeze(0) if gga else None
        v2, u2 = lib.xc_eval_kxc(op.terms, rho, grho, rs.unsqueeze(0), gs1, rs.unsqueeze(0), gs1)
        vd, ud = vd + 2.0 * v2[0], ud + 2.0 * u2[0] if gga else None
    g = _xc_potential_gradient(eng, ao, pbar, v, u)
    g = g + _xc_potential_gradient(eng, ao, s, 4.0 * v1[1], 4.0 * u1[1] if gga else None)
    g = g + _xc_potential_gradient(eng, ao, d_scf, vd, ud)
    t_grid = clock() - tic
    tic = clock()
    fixed = v * rp + 2.0 * v1[1] * rs
    if gga:
        fixed = fixed + (u * gp).sum(0) + 2.0 * (u1[1] * gs).sum(0)
    g = g + _xc_weight_gradient(eng, fixed)
    return g, t_grid, clock() - tic


def _gradient(qc, state, spin, tda, nstates, tol, ztol, with_z=True, times=None, with_kxc=True, who="excited_gradient"):
    """the ExcitedGradient.  with_z=False leaves the Z-vector out of P and W (NOT a gradient of anything:
    tests/test_gpu_excited_gradient.py shows with it that the relaxation is not skipped); with_kxc=False leaves the third-order
    exchange-correlation kernel out of a Kohn-Sham gradient in the same way (tests/test_gpu_tddft_gradient.py); times: a dict that
    receives the wall time of the stages (tools/gpu_excited_gradient_time.py, tools/gpu_tddft_gradient_time.py); who: the public
    function that asks, for the messages"""
    from .gradient import _pulay_densities
    from .properties import dipole_au, excitations
    from .response import orbital_hessian
    eng = qc._engine
    h = eng.hamilton
    dev = h.device
    ks = bool(eng.is_ks)
    a = float(eng.exx) if ks else 1.0         # the exact-exchange fraction on every K
    clock = stage_clock(times, dev)
    scf = qc.nuclear_gradient().detach()     # (raises what nuclear_gradient refuses: a field, vext)
    tic = clock()
    ex = excitations(qc, nstates=state + 1 if nstates is None else int(nstates), spin=spin, tda=tda, tol=tol)
    t_exc = clock() - tic
    nroots = int(ex.energies.numel())
    if not 0 <= state < nroots:
        raise ValueError("%s: state %d is outside the %d roots found (nstates=%s)" % (who, state, nroots, nstates))
    if not ex.residual < tol:
        raise RuntimeError("%s: the excitation vectors are not converged (residual %.2e, tol %.1e): the gradient "
                           "formula needs a stationary excitation energy" % (who, ex.residual, tol))
    op = orbital_hessian(qc, spin)           # the operator `excitations` used: its orbitals define the vectors
    sp = op.spins[0]
    co, cv, eo, ev = sp.co, sp.cv, sp.eo, sp.ev
    no, nv, nao = sp.no, sp.nv, int(co.shape[0])
    xpy = ex.xpy[state]
    xmy = xpy if ex.xmy is None else ex.xmy[state]
    u, v = xpy.reshape(nv, no).T, xmy.reshape(nv, no).T

    def jk(dms_j, dms_k, flags):
        if a == 0.0:  # a pure functional: no exchange matrix is used (every K carries the factor a), none is built
            J, _ = lib.jk_multi(h._tiles, dms_j.contiguous(), None, h._multi_work(dms_j.shape[0], 0))
            return J, torch.zeros_like(dms_k)
        return lib.jk_multi(h._tiles, dms_j.contiguous(), dms_k.contiguous(), h._multi_work(dms_j.shape[0], dms_k.shape[0]), k_antisym=flags)

    tic = clock()
    if ks:
        rhs, parts = lagrangian_rhs(u, v, co, cv, jk, xc=_xc_matrices(op, with_kxc), kfrac=a)
    else:
        rhs, parts = lagrangian_rhs(u, v, co, cv, jk, triplet=spin == "triplet")
    # the orbital relaxation is a singlet for either spin; on the orbitals of the vectors (the memoised singlet operator holds the same
    # ones unless the eigensolver returned the Fock eigenvectors in another phase)
    z, z_residual = z_vector(qc, (co, cv, eo, ev), rhs, ztol, op if spin == "singlet" else orbital_hessian(qc))
    t_z = clock() - tic
    t_mo = relaxed_density_mo(parts["t_oo"], parts["t_vv"])
    p = relaxed_density_mo(parts["t_oo"], parts["t_vv"], z if with_z else None)
    c = torch.cat([co, cv], dim=1)
    pbar = c @ p @ c.T
    g_pbar = parts["g_t"]
    if with_z:
        zbar = (pbar - parts["tbar"]).reshape(1, nao, nao)
        jz, kz = jk(zbar, zbar, [0])
        g_pbar = g_pbar + jz[0] - (0.5 * a) * kz[0]
        if ks:
            g_pbar = g_pbar + op._vxc_response([zbar.contiguous()])[0][0]
    w2 = energy_weighted(p, torch.cat([eo, ev]), parts["coupling"], g_pbar, co, cv)
    _, d_scf, _ = _pulay_densities(qc)
    d_scf = d_scf.detach()
    T = lib.cart2sph_matrix(h._tab, dev)
    tic = clock()
    exc = relaxed_terms(h, T, d_scf, pbar, w2, a)                                    # one-electron and separable: 2 eri_grad2(D, Pbar, 1, a)
    sc, nc = cart_part(T, parts["s"]), cart_part(T, parts["n"], -1.0)
    lib.eri_grad2(exc, sc, sc, 0.0 if spin == "triplet" else 4.0, 4.0 * a, h._tab)   # non-separable, symmetric part
    if a != 0.0:
        lib.eri_grad2(exc, nc, nc, 0.0, 4.0 * a, h._tab)                             # non-separable, antisymmetric part: exchange only
    t_pass = clock() - tic
    t_grid = t_wts = 0.0
    if ks:
        gxc, t_grid, t_wts = _xc_gradient_terms(qc, op, pbar, parts["s"], d_scf, with_kxc, clock)
        exc += gxc
    dm_ao = d_scf + pbar
    dip = dipole_au(h, qc.get_system(), dm_ao).detach()
    if times is not None:
        times.update(excitations=t_exc, z_vector=t_z, passes=t_pass)
        if ks:
            times.update(grid_passes=t_grid, weight_term=t_wts)
    omega = ex.energies[state].detach().reshape(1)
    dens = ExcitedDensity(p, t_mo, dm_ao, dip)
    return ExcitedGradient(scf + exc, scf, omega, qc.energy().detach().reshape(1) + omega, xpy, xmy, dens, z_residual, state, spin, tda)


def _entry(who, kohn_sham, qc, state, spin, tda, nstates, tol, ztol):
    """the memoised `_gradient` behind both public names, under the key of `who`; refuses before anything reaches the library"""
    assert qc._has_run, "run() the calculation first"
    state = int(state)
    if state < 0:
        raise ValueError("%s: state must be >= 0, got %d" % (who, state))
    _refusals(qc, who, spin, kohn_sham)
    key = (who, state, spin, bool(tda), None if nstates is None else int(nstates), float(tol), float(ztol))
    return memoised(qc, key, lambda: _gradient(qc, state, spin, bool(tda), nstates, float(tol), float(ztol), who=who))


def excited_gradient(qc, state=0, spin="singlet", tda=False, nstates=None, tol=1e-8, ztol=1e-9):
    """Analytic nuclear gradient d(E_SCF + w_state) / dR of an excited state of the converged restricted Hartree-Fock calculation `qc`,
    with its relaxed difference density (module docstring): an `ExcitedGradient`.  tda=True: CIS, False: TDHF; spin: "singlet" or
    "triplet" excitations; state: index into the roots of `excitations(qc, nstates, spin, tda, tol)` (ascending energies; nstates=None
    asks for state + 1 of them -- a root is followed by its INDEX, not through crossings); tol: residual norm of the excitation vectors,
    which must be met (RuntimeError otherwise: the formula needs a stationary w); ztol: relative residual of the Z-vector solve.
    For what `excitations` and `nuclear_gradient` take, on a Hartree-Fock reference: a Kohn-Sham one (NotImplementedError: it is taken by
    `tddft_gradient`, which has the third-order exchange-correlation kernel) and an unrestricted one are refused.  The two-electron part
    is three passes of the bilinear derivative kernel (lib.eri_grad2).  Memoised on the converged state per argument set; detached."""
    return _entry("excited_gradient", False, qc, state, spin, tda, nstates, tol, ztol)


def tddft_gradient(qc, state=0, spin="singlet", tda=False, nstates=None, tol=1e-8, ztol=1e-9):
    """Analytic nuclear gradient d(E_SCF + w_state) / dR of an excited state of the converged restricted calculation `qc`, Kohn-Sham
    (LDA, GGA and global hybrids: TDDFT, tda=True: TDA) or Hartree-Fock, with its relaxed difference density: an `ExcitedGradient`;
    arguments as `excited_gradient`.  Kohn-Sham: singlet states; the exchange-correlation terms of the Lagrangian and of the gradient
    (module docstring, last section) on the third-order kernel lib.xc_eval_kxc, the Becke-weight derivative included; two passes of
    lib.eri_grad2 for a pure functional, three for a hybrid.  Hartree-Fock: both spins, the path and the numbers of `excited_gradient`.
    Refused before anything runs: Kohn-Sham triplets (the polarised third-order kernel is not built), meta-GGA functionals,
    unrestricted references, and what `OrbitalHessian` and `nuclear_gradient` refuse.  Memoised under its own key; detached."""
    return _entry("tddft_gradient", True, qc, state, spin, tda, nstates, tol, ztol)


__all__ = ["excited_gradient", "tddft_gradient", "ExcitedGradient", "ExcitedDensity", "difference_density", "transition_densities", "lagrangian_rhs",
           "relaxed_density_mo", "energy_weighted"]
