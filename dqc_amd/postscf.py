"""What the post-SCF methods on the density-fitted tensor share on the host (dqc_amd/mp2.py, rpa.py, gw.py): the refusals, the tensor B
and its occupied-virtual transform, the orbitals of the converged Fock matrix, the memo on the converged state, and the two loops over
the fused kernels that more than one method runs -- the response matrix in frequency batches and the MP2 pair-energy blocks.  And what
the relaxed-density nuclear gradients share (mp2.py, excited.py): the relaxed MO density, its energy-weighted density, the Z-vector
solve, the gradient terms of a relaxed difference density, and the stage clock."""
import time

import torch

from . import lib


def unsupported(qc, who="mp2"):
    """raise for the calculations no post-SCF method here takes; who: the prefix of the messages (rpa and gw refuse in the name of mp2,
    whose references they take)"""
    eng = qc._engine
    h = eng.hamilton
    if getattr(h, "sharded", False):
        raise NotImplementedError(who + ": a Hamiltonian sharded over several GPUs (shard_over) is not supported")
    df = getattr(h, "df", None)
    if df is not None and df.dfinfo.method == "overlap":
        raise NotImplementedError(who + ": density fitting with method=\"overlap\" is not supported (the Coulomb metric only)")
    if getattr(eng.get_system(), "_user_weights", None) is not None:
        raise NotImplementedError(who + ": user-given occupations (orb_weights) are not supported")
    full = 1.0 if eng.polarized else 2.0
    for w in ((eng.orb_weight.u, eng.orb_weight.d) if eng.polarized else (eng.orb_weight,)):
        occ = w[w != 0]
        if not bool(torch.all(occ == full)):
            if not eng.polarized and bool(torch.all((occ == 2.0) | (occ == 1.0))):
                raise NotImplementedError(who + ": restricted open-shell occupations (2, ..., 2, 1, ..., 1) are not supported; run the "
                                          "calculation unrestricted")
            raise NotImplementedError(who + ": fractional occupations are not supported (integer occupations %g only)" % full)


def check_frequency_args(who, nfreq, freq_scale, scale_name="freq_scale"):
    """the refusals of a frequency quadrature: points and scale of `rpa.frequency_grid` (scale_name: what `who` calls the scale)"""
    if nfreq < 1:
        raise ValueError("%s: nfreq must be >= 1, got %d" % (who, nfreq))
    if not freq_scale > 0.0:
        raise ValueError("%s: %s must be positive, got %g" % (who, scale_name, freq_scale))


def aux_key(qc, auxbasis):
    """what a memo key holds for `auxbasis`: None where the Hamiltonian's own tensor is used whatever it is, a named set by its name,
    anything else by identity"""
    h = qc._engine.hamilton
    if h.df is not None and h.df.exchange:
        return None
    return auxbasis if isinstance(auxbasis, str) or auxbasis is None else id(auxbasis)


def memoised(qc, key, compute):
    """memo[key] of the converged state of `qc`, from compute() (run without autograd) the first time"""
    from .response import state_memo
    memo = state_memo(qc)
    if key not in memo:
        with torch.no_grad():
            memo[key] = compute()
    return memo[key]


def b_tensor(qc, auxbasis):
    """the DFMI355 object that holds B[P, mu, nu]: the Hamiltonian's own, or one built here (and remembered per auxiliary basis)"""
    h = qc._engine.hamilton
    if h.df is not None and h.df.exchange:
        return h.df

    def build():
        from .basis import make_aux_atombases
        from .df import DFMI355
        from .utils.datastruct import DensityFitInfo
        mol = qc.get_system()
        # None: the set Mol.densityfit() resolves its default to (the named fitting set when its tables are there, else the generated one)
        auxbases = make_aux_atombases(mol._atomzs, mol._atompos, "cc-pvtz-jkfit" if auxbasis is None else auxbasis, mol._atombases, {})
        info = DensityFitInfo(method="coulomb", auxbases=auxbases, exchange=True)
        return DFMI355(info, h.atombases, h._orthozer, h.device).build()

    return memoised(qc, ("mp2_df", aux_key(qc, auxbasis)), build)


def free_bytes(dev):
    free, _total = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)  # (cached blocks are reusable)


def transform_ov(b, co, cv):
    """Bov[i, P, a] = sum_mu,nu co[mu, i] B[P, mu, nu] cv[nu, a], a padded with zero columns to a multiple of 16: (no, naux, ldv).
    Library matmuls over chunks of P, occupied index first (the cheaper order); no temporary is larger than the result"""
    naux, nao = int(b.shape[0]), int(b.shape[1])
    no, nv = int(co.shape[1]), int(cv.shape[1])
    ldv = (nv + 15) // 16 * 16
    need = 8 * no * naux * ldv
    free = free_bytes(b.device)
    step = max(1, min(naux, naux * ldv // (4 * max(nao, ldv, 1)))) if naux else 1  # the two temporaries: a quarter of Bov each at most
    tmp = 8 * step * no * (nao + ldv)
    if need + tmp > free:
        raise lib.DqcAmdError(
            "mp2: the occupied-virtual tensor Bov (nocc = %d, naux = %d, nvir = %d padded to %d) needs %.2f GB and %.2f GB of "
            "temporaries but only %.2f GB of device memory are free: freeze more orbitals or use a smaller auxiliary basis (there is "
            "no batching over occupied blocks)" % (no, naux, nv, ldv, need / 1e9, tmp / 1e9, free / 1e9))
    cvp = torch.zeros((nao, ldv), dtype=b.dtype, device=b.device)
    cvp[:, :nv] = cv
    cot = co.t().contiguous()
    bov = torch.empty((no, naux, ldv), dtype=b.dtype, device=b.device)
    for p0 in range(0, naux, step):
        half = torch.matmul(cot, b[p0:p0 + step])                       # (pc, no, nao)
        bov[:, p0:p0 + step] = torch.matmul(half, cvp).transpose(0, 1)  # (pc, no, ldv) -> [i, P, a]
    return bov


def orbitals(qc, frozen):
    """per spin (C_occ (nao, no), C_vir (nao, nv), eps_occ, eps_vir) in the AO basis, the lowest `frozen` occupied ones dropped"""
    eng = qc._engine
    h = eng.hamilton
    focks = (qc._fock[0], qc._fock[1]) if eng.polarized else (qc._fock,)
    weights = (eng.orb_weight.u, eng.orb_weight.d) if eng.polarized else (eng.orb_weight,)
    out = []
    for f, w in zip(focks, weights):
        e, c = eng._eigpairs(f.detach())
        c = h._orthozer @ c
        nocc = int((w != 0).sum())
        lo = min(frozen, nocc)
        out.append((c[:, lo:nocc].contiguous(), c[:, nocc:].contiguous(), e[lo:nocc].contiguous(), e[nocc:].contiguous()))
    return out


def response_batches(bovs, spins, freqs_dev, scale, tensors_per_batch, batch=None):
    """an iterator over (k0, n, Q (n, naux, naux)) for the frequencies [k0, k0 + n) of `freqs_dev` in turn: lib.rpa_response with the
    spins of `orbitals` accumulated, into one buffer that every batch reuses.  batch: frequencies per batch (None: as many as half the
    device memory that is free NOW, at the call, holds when the caller keeps `tensors_per_batch` tensors of the size of Q alive per
    batch, Q among them); Q itself is allocated when the first batch is asked for"""
    naux, nfreq = int(bovs[0].shape[1]), int(freqs_dev.numel())
    if batch is None:
        batch = (free_bytes(bovs[0].device) // 2) // max(tensors_per_batch * 8 * naux * naux, 1)
    nk = max(1, min(nfreq, int(batch)))

    def batches():
        q = torch.empty((nk, naux, naux), dtype=bovs[0].dtype, device=bovs[0].device)
        for k0 in range(0, nfreq, nk):
            n = min(nk, nfreq - k0)
            for s, (bov, (_, _, eo, ev)) in enumerate(zip(bovs, spins)):
                lib.rpa_response(bov, eo, ev, freqs_dev[k0:k0 + n].contiguous(), scale, out=q[:n], accumulate=s > 0)
            yield k0, n, q[:n]

    return batches()


def pair_energy_blocks(bovs, spins):
    """(os_ab, same): lib.mp2_pair_energies on the spins of `orbitals` -- os_ab the alpha-beta e_os matrix (None: restricted), same the
    (e_os, e_ss) matrices within each spin, unscaled"""
    os_ab = None
    if len(spins) == 2:
        (_, _, eoa, eva), (_, _, eob, evb) = spins
        os_ab = lib.mp2_pair_energies(bovs[0], bovs[1], eoa, eob, eva, evb, False)[0]
    return os_ab, [lib.mp2_pair_energies(bov, bov, eo, eo, ev, ev, True) for bov, (_, _, eo, ev) in zip(bovs, spins)]


# ------------------------------------------------------------------------------------------------ relaxed-density gradients
def stage_clock(times, dev):
    """clock() -> seconds, for the wall time of the stages of a gradient: synchronises the device first when `times` (the dict that
    receives them) is asked for, and only then"""
    def clock():
        if times is not None:
            torch.cuda.synchronize(dev)
        return time.perf_counter()
    return clock


def relaxed_density_mo(t_oo, t_vv, z=None):
    """P (n, n) in the MO basis: T in its diagonal blocks and, with z (nv, no) the Z-vector, 2 z in the off-diagonal ones"""
    no, nv = int(t_oo.shape[0]), int(t_vv.shape[0])
    p = torch.zeros((no + nv, no + nv), dtype=t_oo.dtype, device=t_oo.device)
    p[:no, :no], p[no:, no:] = t_oo, t_vv
    if z is not None:
        p[no:, :no], p[:no, no:] = 2.0 * z, 2.0 * z.T
    return p


def energy_weighted(p, eps, coupling, g_pbar, co, cv):
    """W (nao, nao) = C 1/4 (Gm + Gm^T) C^T, Gm[p, q] = C_p^T dLagrangian / dC_q = 2 eps_p P_pq + (4 C^T G[Pbar] C_o on the occupied
    columns) + coupling: p the (relaxed) difference density in the MO basis, eps all orbital energies, coupling (n, n) the blocks of the
    method (excited.lagrangian_rhs, mp2.orbital_coupling), g_pbar = G[C p C^T] in the AO basis (Kohn-Sham: G of the last section of the
    docstring of dqc_amd/excited.py, J - a / 2 K + V1, plus 2 V2[S, S] -- `parts["g_t"]` of lagrangian_rhs(..., xc=...) holds both for Tbar)"""
    no = int(co.shape[1])
    c = torch.cat([co, cv], dim=1)
    gm = 2.0 * eps.unsqueeze(1) * p + coupling
    gm[:, :no] += 4.0 * (c.T @ g_pbar @ co)
    w = c @ (0.25 * (gm + gm.T)) @ c.T
    return 0.5 * (w + w.T)                    # (the two GEMMs leave round-off asymmetry: W is handed out exactly symmetric)


def z_vector(qc, orbitals, rhs, tol, op=None):
    """(z (nv, no), the relative residual the solve stopped at) of H z = -rhs, H the singlet orbital Hessian (response.OrbitalHessian)
    on orbitals = (co, cv, eo, ev).  op: an OrbitalHessian that may hold these very orbitals; it is used when they are bit-identical,
    otherwise (and with None) one is built on them"""
    from .response import OrbitalHessian
    co, cv, eo, ev = orbitals
    if op is None or not (torch.equal(op.spins[0].co, co) and torch.equal(op.spins[0].cv, cv)):
        op = OrbitalHessian(qc, orbitals=(torch.cat([co, cv], dim=1), torch.cat([eo, ev])))
    z = op.solve(-rhs.reshape(1, -1), tol=tol).reshape(rhs.shape)
    return z, float(op.last_residual)


def cart_part(T, m, sign=1.0):
    """the symmetric (sign = 1) or antisymmetric (-1) part of T^T m T, the Cartesian-basis image of the AO matrix m; contiguous and
    EXACTLY of that parity: the gate of lib.eri_grad2"""
    x = T.T @ m @ T
    return (0.5 * (x + sign * x.T)).contiguous()


def relaxed_terms(h, T, d_scf, pbar, w2, kfrac=1.0):
    """(natm, 3): what every relaxed difference density Pbar = C P C^T with its energy-weighted density W2 adds to the gradient of the
    SCF energy of density d_scf --  tr[Pbar dh] - tr[W2 dS]  (lib.int1e_grad)  +  the separable two-electron term
    d_integrals tr[Pbar G[D]] = eri_grad2(D, Pbar, 2, 2 kfrac)  (one bilinear pass; kfrac: the exact-exchange fraction).
    T = lib.cart2sph_matrix of the table."""
    out = torch.zeros((h._tab.natm, 3), dtype=torch.float64, device=h.device)
    pc = cart_part(T, pbar)
    lib.int1e_grad(out, pc, cart_part(T, w2), h._tab, h._zs)
    lib.eri_grad2(out, cart_part(T, d_scf), pc, 2.0, 2.0 * kfrac, h._tab)
    return out
