"""Second-order Moller-Plesset correlation energy with density-fitted integrals (RI-MP2) on a converged HF or KS calculation.

    (ia|jb) ~ sum_P B[P, i, a] B[P, j, b],      B[P, mu, nu] = sum_Q (C^-1)[P, Q] (mu nu|Q),  (P|Q) = C C^T      (dqc_amd/df.py)

    V^{ij}_{ab} = (ia|jb),   D^{ij}_{ab} = eps_i + eps_j - eps_a - eps_b
    pair_os[i, j] = sum_ab V_ab^2 / D_ab                  pair_ss[i, j] = sum_ab V_ab (V_ab - V_ba) / D_ab

Conventions (the ones under which c_os = 1.2, c_ss = 1 / 3 is SCS-MP2, and UMP2 of a closed shell has the RMP2 components):

    restricted      e_os = sum_ij pair_os,   e_ss = sum_ij pair_ss              (E_MP2 = sum V (2 V - V^T) / D = e_os + e_ss)
    unrestricted    e_os = e_ab = sum_{i in a, j in b} V^2 / D
                    e_ss = e_aa + e_bb,   e_ss' = 1/2 sum_ij sum_ab V (V - V^T) / D   within one spin
    e_corr = c_os e_os + c_ss e_ss,     e_tot = qc.energy() + e_corr

Orbitals and orbital energies are the eigenpairs of the converged Fock matrix (matrices), as OrbitalHessian takes them; on a Kohn-Sham
reference they are the Kohn-Sham ones (the second-order term of a double hybrid: B2PLYP is
KS(xc="0.53 * hf + 0.47 * gga_x_b88 + 0.73 * gga_c_lyp") and mp2(qc, c_os=0.27, c_ss=0.27)).

Steps: the tensor B (the Hamiltonian's own when it was built with densityfit(exchange=True), otherwise a DFMI355 built here from
`auxbasis`); Bov[i, P, a] = sum_mu,nu C_mu,i B[P, mu, nu] C_nu,a by library matmuls over chunks of P (O(o n^2 naux)); the pair
energies by the fused kernel dqc_mp2_pair_energies (csrc/mp2.hip, O(o^2 v^2 naux): the (ia|jb) are never stored).  `Bov` must fit
in device memory; there is no batching over occupied blocks.  No autograd: the result is detached.

`pair_energies_reference` is the yardstick of the kernel: plain torch on any device, V formed per occupied orbital i.

One-particle densities (`mp2_density`, restricted): the unrelaxed occupied-occupied and virtual-virtual blocks and, for Hartree-Fock on
exact integrals, the orbital-relaxed density (natural orbitals, dipole moments) -- formulas and factors above `density_reference`, the
yardstick of that path.  The amplitudes come from dqc_mp2_amplitudes one block of occupied orbitals at a time (that path IS batched).

Nuclear gradients (`mp2_gradient`, the scope of the relaxed density): formulas and factors above `three_index_densities`; the
non-separable part runs through the three-index-density derivative pass dqc_df_grad3 (csrc/grad.hip)."""
import torch

from . import lib
from .postscf import (aux_key, b_tensor, energy_weighted, free_bytes, memoised, orbitals, pair_energy_blocks, relaxed_density_mo,
                      relaxed_terms, stage_clock, transform_ov, unsupported, z_vector)

# the names under which tests/test_mp2_cpu.py and tests/test_gpu_mp2_density.py, written when these lived here, import them
_unsupported, _b_tensor, _orbitals = unsupported, b_tensor, orbitals


def pair_energies_reference(bi, bj, eps_oi, eps_oj, eps_va, eps_vb, same):
    """(pair_os (noi, noj), pair_ss (noi, noj) or None) of the module docstring in plain torch, on the device of the inputs.
    bi (noi, naux, >= nva), bj (noj, naux, >= nvb): columns past the number of virtual energies (padding) are ignored.  same=True:
    both sides share the virtual space (nva == nvb) and pair_ss is formed too; False: pair_os only.  V^{i.} is formed explicitly,
    one occupied orbital i at a time -- (noj, nva, nvb) doubles."""
    nva, nvb = eps_va.numel(), eps_vb.numel()
    noi, noj = bi.shape[0], bj.shape[0]
    if same and nva != nvb:
        raise ValueError("pair_energies_reference: same=True needs one virtual space on both sides")
    bj = bj[:, :, :nvb]
    pair_os = torch.zeros((noi, noj), dtype=bi.dtype, device=bi.device)
    pair_ss = torch.zeros_like(pair_os) if same else None
    for i in range(noi):
        v = torch.einsum("pa,jpb->jab", bi[i, :, :nva], bj)
        d = eps_oi[i] + eps_oj[:, None, None] - eps_va[None, :, None] - eps_vb[None, None, :]
        pair_os[i] = (v * v / d).sum(dim=(1, 2))
        if same:
            pair_ss[i] = (v * (v - v.transpose(1, 2)) / d).sum(dim=(1, 2))
    return pair_os, pair_ss


class MP2:
    """what `mp2` returns: `e_os`, `e_ss` (opposite- and same-spin correlation energies, unscaled), `e_corr = c_os e_os + c_ss e_ss`,
    `e_tot = qc.energy() + e_corr` (one-element detached tensors); `pair_os`, `pair_ss`: the pair energies they are the sums of --
    restricted: (nocc, nocc) each; unrestricted: pair_os (nocc_a, nocc_b), pair_ss = (aa, bb) with their 1/2.  `c_os`, `c_ss`,
    `frozen`, `naux`; `df`: the DFMI355 object whose tensor was used (kept for reuse)"""

    def __init__(self, e_scf, e_os, e_ss, pair_os, pair_ss, c_os, c_ss, frozen, df):
        self.e_os, self.e_ss, self.pair_os, self.pair_ss = e_os, e_ss, pair_os, pair_ss
        self.c_os, self.c_ss, self.frozen, self.df = float(c_os), float(c_ss), int(frozen), df
        self.naux = int(df._b.shape[0])
        self.e_scf = e_scf
        self.e_corr = self.c_os * e_os + self.c_ss * e_ss
        self.e_tot = e_scf + self.e_corr

    def __repr__(self):
        return "MP2(e_corr=%.10f, e_os=%.10f, e_ss=%.10f, e_tot=%.10f, c_os=%g, c_ss=%g, frozen=%d, naux=%d)" % (
            float(self.e_corr), float(self.e_os), float(self.e_ss), float(self.e_tot), self.c_os, self.c_ss, self.frozen, self.naux)


def components(pair_os, pair_ss, polarized):
    """(e_os, e_ss) from pair energies in the conventions of the module docstring.  restricted: the two (nocc, nocc) matrices;
    unrestricted: pair_os the alpha-beta matrix, pair_ss = (aa, bb), each already carrying its 1/2"""
    if polarized:
        return pair_os.sum().reshape(1), (pair_ss[0].sum() + pair_ss[1].sum()).reshape(1)
    return pair_os.sum().reshape(1), pair_ss.sum().reshape(1)


def energies_reference(spins, frozen=0):
    """(e_os, e_ss, pair_os, pair_ss) through `pair_energies_reference`: `spins` holds one (restricted) or two (unrestricted: alpha,
    beta) tuples (bov (nocc, naux, >= nvir), eps_occ, eps_vir); the lowest `frozen` occupied orbitals of each are dropped"""
    spins = [(b[frozen:], eo[frozen:], ev) for b, eo, ev in spins]
    if len(spins) == 1:
        b, eo, ev = spins[0]
        pair_os, pair_ss = pair_energies_reference(b, b, eo, eo, ev, ev, True)
    else:
        (ba, eoa, eva), (bb, eob, evb) = spins
        pair_os, _ = pair_energies_reference(ba, bb, eoa, eob, eva, evb, False)
        pair_ss = tuple(0.5 * pair_energies_reference(b, b, eo, eo, ev, ev, True)[1] for b, eo, ev in spins)
    return components(pair_os, pair_ss, len(spins) == 2) + (pair_os, pair_ss)


def _compute(qc, frozen, auxbasis):
    eng = qc._engine
    df = b_tensor(qc, auxbasis)
    b = df._b
    spins = orbitals(qc, frozen)
    bovs = [transform_ov(b, co, cv) for co, cv, _, _ in spins]
    os_ab, same = pair_energy_blocks(bovs, spins)
    if not eng.polarized:
        pair_os, pair_ss = same[0]
    else:
        pair_os, pair_ss = os_ab, tuple(0.5 * ss for _, ss in same)
    e_os, e_ss = components(pair_os, pair_ss, eng.polarized)
    return df, pair_os, pair_ss, e_os, e_ss


def mp2(qc, frozen=0, auxbasis=None, c_os=1.0, c_ss=1.0):
    """RI-MP2 correlation energy of the converged HF / KS calculation `qc` (module docstring): an `MP2` result object.
    frozen: the lowest `frozen` occupied orbitals of each spin are left out of the correlation treatment.
    auxbasis: used when the Hamiltonian carries no fitted-exchange tensor (exact integrals, a J-only fit, direct SCF) -- as
    Mol.densityfit takes it; None: the set Mol.densityfit() would use (when that is the set GENERATED from a small orbital basis it
    fits J, not correlation: 7.8e-3 Ha off on H2O / 3-21G where "etb" is 7e-6 Ha off).  A Hamiltonian built with
    densityfit(exchange=True) uses its own.
    c_os, c_ss: scaling of the opposite- and same-spin parts (1.2 and 1 / 3: SCS-MP2; 0.27 both: the B2PLYP term).
    Memoised on the converged state: another scaling, or a second call, does not run the kernel again."""
    assert qc._has_run, "run() the calculation first"
    frozen = int(frozen)
    if frozen < 0:
        raise ValueError("mp2: frozen must be >= 0, got %d" % frozen)
    unsupported(qc)
    df, pair_os, pair_ss, e_os, e_ss = memoised(qc, ("mp2", frozen, aux_key(qc, auxbasis)), lambda: _compute(qc, frozen, auxbasis))
    e_scf = qc.energy().detach().reshape(1)
    return MP2(e_scf, e_os, e_ss, pair_os, pair_ss, c_os, c_ss, frozen, df)


# ------------------------------------------------------------------------------------------------ one-particle densities
# Restricted closed shell; i, j, k active occupied, a, b, c virtual; T = V / D, Tt = (c_os + c_ss) T - c_ss T^T (2 T - T^T for MP2):
#
#     e_corr = sum_ijab V^{ij}_{ab} Tt^{ij}_{ab}
#     P_ab =  2 sum_ij sum_c T^{ij}_{ac} Tt^{ij}_{bc}          P_ij = -2 sum_k sum_ab T^{ki}_{ab} Tt^{kj}_{ab}       (both symmetrised)
#     Gamma[i, P, a] = sum_jb Tt^{ij}_{ab} Bov[j, P, b]          (sum Gamma Bov = e_corr)
#
# P_oo and P_vv are the derivatives of the Hylleraas functional by the occupied-occupied and virtual-virtual Fock blocks (P_aa =
# d e_corr / d eps_a, P_ii = d e_corr / d eps_i), the UNRELAXED density.  The relaxed one adds the response of the SCF orbitals: under
# a rotation kappa_ai (the variables of response.OrbitalHessian: dC_i = sum_a C_a kappa_ai, dC_a = -sum_i C_i kappa_ai) the functional
# changes by L . kappa,
#
#     L_ai = 4 [ (C_v^T G[Pbar] C_o)_ai + X_ai - Y_ai ],     Pbar = C_v P_vv C_v^T + C_o P_oo C_o^T,   G[D] = J[D] - K[D] / 2
#     X_ci = sum_aP Gamma[i, P, a] B^P_ca,      Y_ak = sum_iP Gamma[i, P, a] B^P_ik
#
# (the first term: the Fock blocks follow the SCF density; X - Y: 2 sum Tt dV), and a one-electron perturbation lambda O moves the
# orbitals by d kappa / d lambda = -4 H^-1 O_vo (H = 4 (A + B), the Hessian of OrbitalHessian, whose gradient is 4 F_ai).  So
#
#     H z = -L,     P_ai = P_ia = 2 z_ai,     d E_MP2 / d lambda = tr[(D_SCF + C P C^T) O]
#
# X is evaluated through the AO tensor -- Gamma back-transformed in its virtual index, contracted with B[P, mu, nu] over chunks of P --
# and Y from B^P_ik, so no B_vv is ever stored.  tests/test_gpu_mp2_density.py holds the factors against finite-field derivatives.


def density_reference(bov, eo, ev, c_os=1.0, c_ss=1.0):
    """(P_oo (no, no), P_vv (nv, nv), Gamma (no, naux, nv)) of the formulas above in plain torch, on the device of the inputs: the
    yardstick of `mp2_density`.  bov (no, naux, >= nv): columns past the number of virtual energies (padding) are ignored.  The dense
    T^{i.} is formed one occupied orbital i at a time -- (no, nv, nv) doubles"""
    no, nv = int(bov.shape[0]), int(ev.numel())
    b = bov[:, :, :nv]
    p_oo = torch.zeros((no, no), dtype=b.dtype, device=b.device)
    p_vv = torch.zeros((nv, nv), dtype=b.dtype, device=b.device)
    gamma = torch.zeros((no, int(b.shape[1]), nv), dtype=b.dtype, device=b.device)
    for i in range(no):
        v = torch.einsum("pa,jpb->jab", b[i], b)
        t = v / (eo[i] + eo[:, None, None] - ev[None, :, None] - ev[None, None, :])
        tt = (c_os + c_ss) * t - c_ss * t.transpose(1, 2)
        p_vv += 2.0 * torch.einsum("jac,jbc->ab", t, tt)
        p_oo -= 2.0 * torch.einsum("jab,kab->jk", t, tt)
        gamma[i] = torch.einsum("jab,jpb->pa", tt, b)
    return 0.5 * (p_oo + p_oo.t()), 0.5 * (p_vv + p_vv.t()), gamma


class MP2Density:
    """what `mp2_density` returns (detached tensors on the device of the calculation):
    `dm_mo` (n, n): the correction to the SCF density in the basis of the canonical orbitals (all of them, in energy order; the rows
    and columns of frozen orbitals are zero); occupied-occupied and virtual-virtual blocks always, the occupied-virtual ones when relaxed;
    `dm_ao`: the SCF density plus the correction, AO basis; `natural_occupations` (descending, they sum to the electron count) and
    `natural_orbitals` (AO coefficients, columns, C^T S C = 1) of it; `dipole(unit)`; `e_corr` = sum Gamma Bov (equal to mp2().e_corr);
    `relaxed`, `z_residual` (the relative residual the Z-vector solve stopped at; None when unrelaxed); `c_os`, `c_ss`, `frozen`,
    `naux`, `block` (occupied orbitals per amplitude block)"""

    def __init__(self, dm_mo, dm_ao, occ, orbs, dip_au, e_corr, relaxed, z_residual, c_os, c_ss, frozen, naux, block):
        self.dm_mo, self.dm_ao, self.natural_occupations, self.natural_orbitals = dm_mo, dm_ao, occ, orbs
        self._dip_au, self.e_corr, self.relaxed, self.z_residual = dip_au, e_corr, bool(relaxed), z_residual
        self.c_os, self.c_ss, self.frozen, self.naux, self.block = float(c_os), float(c_ss), int(frozen), int(naux), int(block)

    def dipole(self, unit="Debye"):
        """electric dipole moment (3,) of the MP2 density, nuclear part included: sign and units of `properties.edipole`"""
        from .properties import _DIPOLE_UNITS, _unit
        return self._dip_au * _unit(_DIPOLE_UNITS, unit, "dipole")

    def __repr__(self):
        return "MP2Density(%s, e_corr=%.10f, c_os=%g, c_ss=%g, frozen=%d, naux=%d)" % (
            "relaxed" if self.relaxed else "unrelaxed", float(self.e_corr), self.c_os, self.c_ss, self.frozen, self.naux)


def unrelaxed_blocks(bov, eo, ev, c_os=1.0, c_ss=1.0, block=None, amplitudes=None):
    """(P_oo, P_vv (nv, nv), Gamma (no, naux, ldv), occupied orbitals per block) from the amplitude kernel, one occupied block at a
    time: per block lib.mp2_amplitudes, then library GEMMs on the padded shapes -- P_vv += 2 T^T Tt over the rows (k, j, c), split [by
    T^{kj}_{ca} = T^{jk}_{ac} the sum over all blocks is the P_ab above], P_oo -= 2 sum_k T[k] Tt[k]^T over (a, b), Gamma[blk] +=
    Tt[:, j] Bov[j]^T for every j.  Only Bov and Gamma (the same size) stay resident; the two amplitude buffers are reused.
    `amplitudes`: a stand-in with the signature of lib.mp2_amplitudes (tools/gpu_mp2_density_time.py times an all-torch one)"""
    amplitudes = lib.mp2_amplitudes if amplitudes is None else amplitudes
    no, naux, ldv = (int(x) for x in bov.shape)
    nv = int(ev.numel())
    per = 2 * 8 * no * ldv * ldv + 8 * ldv * naux          # T and Tt of one occupied orbital, its slab of Gamma^T
    if block is None:
        fixed = 8 * no * naux * ldv * 2 + 8 * ldv * ldv    # Gamma, Bov transposed
        block = (free_bytes(bov.device) - fixed) // 2 // max(per, 1)
    nb = max(1, min(no, int(block)))
    p_oo = torch.zeros((no, no), dtype=bov.dtype, device=bov.device)
    p_vv = torch.zeros((ldv, ldv), dtype=bov.dtype, device=bov.device)
    gamma = torch.empty_like(bov)
    bovt = bov.transpose(1, 2).contiguous()                # [j, b, P]
    out = None
    if amplitudes is lib.mp2_amplitudes:
        out = tuple(torch.empty(nb * no * ldv * ldv, dtype=bov.dtype, device=bov.device) for _ in range(2))
    for i0 in range(0, no, nb):
        ni = min(nb, no - i0)
        t, tt = amplitudes(bov, eo, ev, i0, ni, c_os, c_ss, out=out)
        # both sums are long (ni no ldv and ldv^2 terms) with small results: as single GEMMs they run on a handful of workgroups (20 and
        # 5 ms at nocc 46, ldv 176 against 0.7 and 1.3 ms), so the sum is split into batches and the partial results added
        split = max(d for d in range(1, min(ni * no, 128) + 1) if (ni * no) % d == 0)
        p_vv += 2.0 * torch.bmm(t.view(split, -1, ldv).transpose(1, 2), tt.view(split, -1, ldv)).sum(0)
        for k in range(ni):   # batches: the first virtual index
            p_oo -= 2.0 * torch.bmm(t[k].transpose(0, 1), tt[k].permute(1, 2, 0)).sum(0)
        g = torch.zeros((ni, ldv, naux), dtype=bov.dtype, device=bov.device)
        for j in range(no):
            g.baddbmm_(tt[:, j], bovt[j].expand(ni, ldv, naux))
        gamma[i0:i0 + ni] = g.transpose(1, 2)
    return 0.5 * (p_oo + p_oo.t()), (0.5 * (p_vv + p_vv.t()))[:nv, :nv].contiguous(), gamma, nb


def _lagrangian(h, b, co, cv, p_oo, p_vv, gamma, parts=None):
    """L_ai (nv, no) of the comment above; b (naux, nao, nao), gamma (no, naux, ldv), all orbitals active.  parts: a dict that
    receives X and Y (nv, no), which the nuclear gradient needs again"""
    no, nv, naux, nao = int(co.shape[1]), int(cv.shape[1]), int(b.shape[0]), int(b.shape[1])
    pbar = (cv @ p_vv @ cv.t() + co @ p_oo @ co.t()).reshape(1, nao, nao).contiguous()
    jm, km = lib.jk_multi(h._tiles, pbar, pbar, h._multi_work(1, 1))
    lag = cv.t() @ (jm[0] - 0.5 * km[0]) @ co
    w = torch.zeros((nao, no), dtype=b.dtype, device=b.device)   # W[mu, i] = sum_P,nu B[P, mu, nu] Gamma^P[i, nu]
    y = torch.zeros((nv, no), dtype=b.dtype, device=b.device)
    step = max(1, min(naux, (1 << 25) // max(nao * max(nao, no), 1)))
    cvt = cv.t().contiguous()
    for p0 in range(0, naux, step):
        bp = b[p0:p0 + step]
        gp = gamma[:, p0:p0 + step, :nv]                                  # (no, pc, nv)
        gao = torch.matmul(gp, cvt)                                       # (no, pc, nao): the virtual index back in the AO basis
        w += torch.einsum("pmn,ipn->mi", bp, gao)
        boo = torch.matmul(co.t(), torch.matmul(bp, co))                  # (pc, no, no): B^P_ik
        y += torch.einsum("ipa,pik->ak", gp, boo)
    if parts is not None:
        parts.update(x=cv.t() @ w, y=y)
    return 4.0 * (lag + cv.t() @ w - y)


def _density(qc, frozen, auxbasis, c_os, c_ss, relaxed, tol, block, parts=None):
    """the MP2Density; parts: a dict that receives what the nuclear gradient takes from this build (df, co, cv, eo, ev, bov, gamma,
    p_oo, p_vv and, relaxed, z, x, y), so that nothing of it is computed twice"""
    from .properties import _total_ao_density, dipole_au
    h = qc._engine.hamilton
    df = b_tensor(qc, auxbasis)
    b = df._b
    co, cv, eo, ev = orbitals(qc, frozen)[0]
    c_frozen = orbitals(qc, 0)[0][0][:, :frozen]
    bov = transform_ov(b, co, cv)
    p_oo, p_vv, gamma, nb = unrelaxed_blocks(bov, eo, ev, c_os, c_ss, block)
    e_corr = (gamma * bov).sum().reshape(1)
    if parts is not None:
        parts.update(df=df, co=co, cv=cv, eo=eo, ev=ev, bov=bov, gamma=gamma, p_oo=p_oo, p_vv=p_vv)
    nf, no, nv = int(c_frozen.shape[1]), int(co.shape[1]), int(cv.shape[1])
    n = nf + no + nv
    z = z_residual = None
    if relaxed:
        z, z_residual = z_vector(qc, (co, cv, eo, ev), _lagrangian(h, b, co, cv, p_oo, p_vv, gamma, parts), tol)
        if parts is not None:
            parts.update(z=z)
    dm_mo = torch.zeros((n, n), dtype=b.dtype, device=b.device)
    dm_mo[nf:, nf:] = relaxed_density_mo(p_oo, p_vv, z)
    c_all = torch.cat([c_frozen, co, cv], dim=1)
    _, d_scf = _total_ao_density(qc)
    d_scf = d_scf.detach()
    dm_ao = d_scf + c_all @ dm_mo @ c_all.t()
    occ_mo = dm_mo.clone()
    occ_mo.diagonal()[:nf + no] += 2.0
    occ, u = torch.linalg.eigh(occ_mo)
    occ, orbs = occ.flip(0), (c_all @ u).flip(1)
    dip = dipole_au(h, qc.get_system(), dm_ao).detach()
    return MP2Density(dm_mo, dm_ao, occ, orbs.contiguous(), dip, e_corr, relaxed, z_residual, c_os, c_ss, frozen, b.shape[0], nb)


def _density_refusals(qc, who, frozen, relaxed):
    """what `mp2_density` refuses, in the name of `who` (mp2_gradient takes exactly the calculations of the relaxed density)"""
    eng = qc._engine
    if eng.polarized:
        raise NotImplementedError(who + ": unrestricted calculations are not supported (restricted closed shell only)")
    if relaxed and frozen > 0:
        raise NotImplementedError(who + ": the relaxed density with frozen orbitals is not supported (the frozen-active rotations "
                                  "are not in the Z-vector equations); use frozen=0 or relaxed=False")
    if relaxed and eng.is_ks:
        raise NotImplementedError(who + ": the relaxed density on a Kohn-Sham reference is not supported (the double-hybrid response "
                                  "needs exchange-correlation terms in the Lagrangian); use relaxed=False")
    unsupported(qc, "mp2" if who == "mp2_density" else who)
    h = eng.hamilton
    if relaxed:
        if h.df is not None or getattr(h, "_direct", False) or getattr(h, "_tiles_store", None) is None:
            raise NotImplementedError(who + ": the relaxed density needs the orbital Hessian over the resident exact integrals, which a "
                                      "density-fitted or direct-SCF Hamiltonian does not have: pass an exact-integral calculation and "
                                      "`auxbasis=`, or use relaxed=False")


def mp2_density(qc, frozen=0, auxbasis=None, c_os=1.0, c_ss=1.0, relaxed=True, tol=1e-9, block=None):
    """RI-MP2 one-particle density of the converged restricted HF / KS calculation `qc`: an `MP2Density` (natural orbitals and occupation
    numbers, dipole moment).  `frozen`, `auxbasis`, `c_os`, `c_ss` as `mp2` takes them.  relaxed=True adds the response of the SCF
    orbitals (the density whose expectation values are the derivatives of the MP2 energy: a Z-vector solve on the orbital Hessian,
    `tol` its relative residual) -- for Hartree-Fock on the exact-integral tile store without frozen orbitals; relaxed=False: the
    occupied-occupied and virtual-virtual blocks alone (any reference `mp2` takes, restricted).  The amplitudes are formed one block of
    occupied orbitals at a time (csrc/mp2.hip: dqc_mp2_amplitudes) and never held as a whole: only Bov and a tensor of its size stay
    resident; `block`: occupied orbitals per block (None: as many as the free device memory holds; any value >= 1 gives the same
    matrices to round-off).  Memoised on the converged state per argument set; nothing is differentiable: the result is detached."""
    assert qc._has_run, "run() the calculation first"
    frozen = int(frozen)
    if frozen < 0:
        raise ValueError("mp2_density: frozen must be >= 0, got %d" % frozen)
    _density_refusals(qc, "mp2_density", frozen, relaxed)
    key = ("mp2_density", frozen, aux_key(qc, auxbasis), float(c_os), float(c_ss), bool(relaxed), float(tol) if relaxed else None,
           None if block is None else int(block))
    return memoised(qc, key, lambda: _density(qc, frozen, auxbasis, float(c_os), float(c_ss), bool(relaxed), float(tol), block))


# ------------------------------------------------------------------------------------------------ nuclear gradient
# d e_tot / dR of restricted closed-shell RI-MP2 on a Hartree-Fock reference, all orbitals active.  With T held at its stationary value
# the Lagrangian is  E_SCF + E_2[C, integrals] + sum_ai z_ai 4 F_ai,  E_2 the Hylleraas functional, whose differential is
#
#     d E_2 = 4 sum_iPa Gamma[i, P, a] d Bov[i, P, a] + sum_pq P_pq d F_pq          (P_oo, P_vv; with z: P_ai = P_ia = 2 z_ai)
#
# and it is stationary in the orbital rotations (H z = -L).  What is left of dC / dR is the re-orthonormalisation dC = -1/2 C (C^T dS C),
# which meets the functional through the symmetric part of C^T dLagrangian / dC: an energy-weighted density.  Terms, (p, q) over all
# orbitals, P the relaxed `dm_mo`, Pbar = C P C^T, D the SCF density:
#
#   the SCF energy   qc.nuclear_gradient(): tr[D dh] - tr[W_SCF dS] + Q(D) + nuclear repulsion,
#       Q(D) = sum (d a b|c d) [2 D_ab D_cd - D_ac D_bd] = d[1/2 D.G.D]
#   one-electron   tr[Pbar dh] - tr[W2 dS]                                                               -> postscf.relaxed_terms
#       W2 = C 1/4 (Gm + Gm^T) C^T,   Gm[p, q] = C_p^T dLagrangian / dC_q  (correlation part; postscf.energy_weighted):
#       Gm[p, q] = 2 eps_p P_pq                       (the outer orbitals of tr[P C^T F C])
#       Gm[p, i] += 4 (C^T G[Pbar] C_o)_pi            (F follows D = 2 C_o C_o^T)
#       Gm[k, i] += 4 sum_Pa Bov[k, P, a] Gamma[i, P, a]     Gm[c, i] += 4 X_ci                           (`orbital_coupling`)
#       Gm[k, a] += 4 Y_ak                                    Gm[c, a] += 4 sum_iP Bov[i, P, c] Gamma[i, P, a]
#   separable two-electron   Q(D + Pbar) - Q(D) - Q(Pbar) = 2 eri_grad2(D, Pbar, 1, 1): one bilinear pass   -> postscf.relaxed_terms
#   non-separable   4 sum Gamma d Bov at fixed orbitals, Bov = C^-1 (Q|ia), (P|Q) = C C^T  (`chol` below is this C):
#       sum Z[mu, nu, Q] d(mu nu|Q) - 1/2 sum G[P, Q] d(P|Q)                                              -> lib.df_grad3
#       Gt = C^-T Gamma,  Bt = C^-T Bov  (triangular solves over the auxiliary index),  gam[P, Q] = sum_ia Bt[i, P, a] Gt[i, Q, a]
#       Z = 4 sym_mu,nu (C_o Gt C_v^T),   G = 4 sym(gam)
#       (d C^-1 = -C^-1 dC C^-1, and N = sum Gamma Bov^T is symmetric, so tr[N C^-1 dC] = 1/2 tr[C^-T N C^-1 d(P|Q)])
#
# tests/test_mp2_gradient_cpu.py and tests/test_gpu_mp2_gradient.py hold the factors against finite differences.


def _aux_solve(chol, t):
    """C^-T t over the auxiliary (middle) index of t (no, naux, nv): (naux, no, nv)"""
    no, naux, nv = (int(x) for x in t.shape)
    x = torch.linalg.solve_triangular(chol.t(), t.transpose(0, 1).reshape(naux, no * nv), upper=True)
    return x.reshape(naux, no, nv)


def _z_block(gt, co, cv):
    """Z[mu, nu, Q] = 4 sym_mu,nu sum_ia co[mu, i] gt[Q, i, a] cv[nu, a] for the rows Q of gt handed in: (nao, nao, nq)"""
    zq = torch.matmul(torch.matmul(co, gt), cv.t())     # (nq, nao, nao)
    return (2.0 * (zq + zq.transpose(1, 2))).permute(1, 2, 0).contiguous()


def three_index_densities(gamma, bov, chol, co, cv):
    """(Z (nao, nao, naux), G (naux, naux)) of the comment above in the spherical basis, in plain torch on the device of the inputs:
    the densities that meet d(mu nu|Q) and -1/2 d(P|Q) in the change of e_corr at fixed orbitals.  gamma, bov (no, naux, >= nv):
    columns past the virtual orbitals of cv (padding) are ignored; chol: the lower Cholesky factor of (P|Q)"""
    nv = int(cv.shape[1])
    gt, bt = _aux_solve(chol, gamma[:, :, :nv]), _aux_solve(chol, bov[:, :, :nv])
    naux = int(gt.shape[0])
    gam = bt.reshape(naux, -1) @ gt.reshape(naux, -1).t()
    return _z_block(gt, co, cv), 2.0 * (gam + gam.t())


def _nonseparable_gradient(df, gamma, bov, co, cv, natm, block, times=None):
    """(natm, 3): three_index_densities taken to the Cartesian basis of the concatenated table and contracted by lib.df_grad3 -- G in one
    call, Z in blocks of `block` auxiliary shells (None: what a quarter of the free device memory holds); the twice-listed atoms folded"""
    import time
    dev = co.device
    tab, orb, aux = df._tab, df._orb_range, df._aux_range
    nao, nv = int(co.shape[0]), int(cv.shape[1])
    T = lib.cart2sph_matrix(tab, dev)                        # all shells: orbital, then auxiliary
    nco = sum((int(l) + 1) * (int(l) + 2) // 2 for l in tab.bas[orb[0]:orb[1], 1])
    to, tx = T[:nao, :nco].contiguous(), T[nao:, nco:].contiguous()
    tic = time.perf_counter()
    gt, bt = _aux_solve(df._chol_j2c, gamma[:, :, :nv]), _aux_solve(df._chol_j2c, bov[:, :, :nv])
    naux = int(gt.shape[0])
    gam = bt.reshape(naux, -1) @ gt.reshape(naux, -1).t()
    gc = (tx.t() @ (2.0 * (gam + gam.t())) @ tx).contiguous()
    del bt
    t_form, t_pass = time.perf_counter() - tic, 0.0
    gbig = torch.zeros((tab.natm, 3), dtype=co.dtype, device=dev)
    tic = time.perf_counter()
    lib.df_grad3(gbig, None, gc, tab, orb, aux)
    t_pass += time.perf_counter() - tic
    ls = [int(l) for l in tab.bas[aux[0]:aux[1], 1]]
    if block is None:
        per = 8 * 15 * (3 * nco * nco + 2 * nao * nao)       # one g shell of Z, Cartesian and spherical, with the transform's temporaries
        block = (free_bytes(dev) // 4) // max(per, 1)
    nb = max(1, min(len(ls), int(block)))
    s0 = c0 = 0                                              # spherical / Cartesian offset inside the auxiliary range
    for k in range(0, len(ls), nb):
        ns = sum(2 * l + 1 for l in ls[k:k + nb])
        nc = sum((l + 1) * (l + 2) // 2 for l in ls[k:k + nb])
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        tic = time.perf_counter()
        z = _z_block(gt[s0:s0 + ns], co, cv)                                   # (nao, nao, ns)
        z = torch.matmul(z, tx[s0:s0 + ns, c0:c0 + nc])                        # (nao, nao, nc)
        z = torch.matmul(to.t(), z.reshape(nao, nao * nc)).reshape(nco, nao, nc)
        z = torch.matmul(to.t(), z).contiguous()                               # (nco, nco, nc)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t_form += time.perf_counter() - tic
        tic = time.perf_counter()
        lib.df_grad3(gbig, z, None, tab, orb, (aux[0] + k, aux[0] + min(k + nb, len(ls))))
        t_pass += time.perf_counter() - tic
        s0, c0 = s0 + ns, c0 + nc
    if times is not None:
        times.update(form=t_form, three_index=t_pass, aux_blocks=(len(ls) + nb - 1) // nb)
    return gbig[:natm] + gbig[natm:]


def orbital_coupling(bov, gamma, x, y, nv):
    """the (n, n) MO matrix of the four Gamma blocks of Gm in the comment above (the `coupling` of postscf.energy_weighted), in plain
    torch on the device of the inputs: bov, gamma (no, naux, >= nv) -- columns past nv (padding) are ignored -- and X, Y (nv, no)"""
    oo = torch.einsum("kpa,ipa->ki", bov, gamma)
    vv = torch.einsum("ipc,ipa->ca", bov, gamma)[:nv, :nv]
    return 4.0 * torch.cat([torch.cat([oo, y.t()], dim=1), torch.cat([x, vv], dim=1)], dim=0)


def _gradient(qc, auxbasis, c_os, c_ss, tol, block, with_z=True, times=None):
    """(MP2Density, scf (natm, 3), total (natm, 3)) of the comment above.  with_z=False leaves the Z-vector blocks out of P (NOT a
    gradient of anything: tests/test_gpu_mp2_gradient.py shows with it that the relaxation is not skipped); times: a dict that receives
    the wall time of the stages (tools/gpu_mp2_gradient_time.py)"""
    from .gradient import _pulay_densities
    h = qc._engine.hamilton
    dev = h.device
    clock = stage_clock(times, dev)
    scf = qc.nuclear_gradient().detach()     # (raises what nuclear_gradient refuses: a field, vext)
    tic = clock()
    parts = {}
    dens = _density(qc, 0, auxbasis, c_os, c_ss, True, tol, block, parts)
    t_density = clock() - tic
    co, cv, eo, ev, bov, gamma = (parts[k] for k in ("co", "cv", "eo", "ev", "bov", "gamma"))
    nv, nao = int(cv.shape[1]), int(co.shape[0])
    c_all = torch.cat([co, cv], dim=1)
    p = dens.dm_mo if with_z else relaxed_density_mo(parts["p_oo"], parts["p_vv"])
    pbar = c_all @ p @ c_all.t()
    pb = pbar.reshape(1, nao, nao).contiguous()
    jm, km = lib.jk_multi(h._tiles, pb, pb, h._multi_work(1, 1))
    w2 = energy_weighted(p, torch.cat([eo, ev]), orbital_coupling(bov, gamma, parts["x"], parts["y"], nv), jm[0] - 0.5 * km[0], co, cv)
    _, d_scf, _ = _pulay_densities(qc)
    tic = clock()
    grad = scf + relaxed_terms(h, lib.cart2sph_matrix(h._tab, dev), d_scf.detach(), pbar, w2)
    t_sep = clock() - tic
    ns_times = {} if times is not None else None
    grad += _nonseparable_gradient(parts["df"], gamma, bov, co, cv, h._tab.natm, block, ns_times)
    if times is not None:
        times.update(ns_times, density=t_density, separable=t_sep)
    return dens, scf, grad


class MP2Gradient:
    """what `mp2_gradient` returns (detached tensors on the device of the calculation): `gradient` (natm, 3) = d mp2().e_tot / dR in
    Hartree / Bohr, `scf` (equal to qc.nuclear_gradient()) and `correlation` = gradient - scf; `density`: the relaxed `MP2Density` it
    used; `z_residual` (the relative residual the Z-vector solve stopped at), `c_os`, `c_ss`, `naux`"""

    def __init__(self, gradient, scf, density):
        self.gradient, self.scf, self.correlation, self.density = gradient, scf, gradient - scf, density
        self.z_residual, self.c_os, self.c_ss, self.naux = density.z_residual, density.c_os, density.c_ss, density.naux

    def __repr__(self):
        return "MP2Gradient(max |g| = %.3e, max |g_corr| = %.3e, c_os=%g, c_ss=%g, naux=%d)" % (
            float(self.gradient.abs().max()), float(self.correlation.abs().max()), self.c_os, self.c_ss, self.naux)


def mp2_gradient(qc, auxbasis=None, c_os=1.0, c_ss=1.0, tol=1e-9, block=None):
    """Nuclear gradient of the RI-MP2 (c_os, c_ss: SCS-MP2) total energy of the converged calculation `qc`: an `MP2Gradient`.  For what
    `mp2_density(relaxed=True)` takes -- restricted closed-shell Hartree-Fock on the exact-integral tile store, all orbitals active,
    `auxbasis=` for the correlation part -- and `nuclear_gradient` does not refuse (a field, an external potential, shard_over).  The
    formulas stand above `three_index_densities`; the non-separable part is the three-index-density derivative pass dqc_df_grad3
    (csrc/grad.hip).  tol: relative residual of the Z-vector solve; block: the blocking of both batched steps, occupied orbitals per
    amplitude block and auxiliary shells per derivative pass (None: what the free device memory holds; any value >= 1 gives the same
    gradient to round-off).  Memoised on the converged state per argument set; detached."""
    assert qc._has_run, "run() the calculation first"
    _density_refusals(qc, "mp2_gradient", 0, True)
    key = ("mp2_gradient", aux_key(qc, auxbasis), float(c_os), float(c_ss), float(tol), None if block is None else int(block))

    def compute():
        dens, scf, grad = _gradient(qc, auxbasis, float(c_os), float(c_ss), float(tol), block)
        return MP2Gradient(grad, scf, dens)

    return memoised(qc, key, compute)


# `dqc_amd.mp2` is this function once the package has imported it: the yardstick stays reachable as dqc_amd.mp2.pair_energies_reference
mp2.pair_energies_reference = pair_energies_reference
mp2.density_reference = density_reference
mp2.three_index_densities = three_index_densities
mp2.orbital_coupling = orbital_coupling

__all__ = ["mp2", "MP2", "pair_energies_reference", "energies_reference", "components", "transform_ov", "mp2_density", "MP2Density",
           "density_reference", "unrelaxed_blocks", "mp2_gradient", "MP2Gradient", "three_index_densities", "orbital_coupling"]
