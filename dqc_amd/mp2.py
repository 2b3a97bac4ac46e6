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
in device memory; there is no batching over occupied blocks.  No gradient and no autograd: the result is detached.

`pair_energies_reference` is the yardstick of the kernel: plain torch on any device, V formed per occupied orbital i."""
import torch

from . import lib


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


def _unsupported(qc):
    eng = qc._engine
    h = eng.hamilton
    if getattr(h, "sharded", False):
        raise NotImplementedError("mp2: a Hamiltonian sharded over several GPUs (shard_over) is not supported")
    df = getattr(h, "df", None)
    if df is not None and df.dfinfo.method == "overlap":
        raise NotImplementedError("mp2: density fitting with method=\"overlap\" is not supported (the Coulomb metric only)")
    if getattr(eng.get_system(), "_user_weights", None) is not None:
        raise NotImplementedError("mp2: user-given occupations (orb_weights) are not supported")
    full = 1.0 if eng.polarized else 2.0
    for w in ((eng.orb_weight.u, eng.orb_weight.d) if eng.polarized else (eng.orb_weight,)):
        occ = w[w != 0]
        if not bool(torch.all(occ == full)):
            if not eng.polarized and bool(torch.all((occ == 2.0) | (occ == 1.0))):
                raise NotImplementedError("mp2: restricted open-shell occupations (2, ..., 2, 1, ..., 1) are not supported; run the "
                                          "calculation unrestricted")
            raise NotImplementedError("mp2: fractional occupations are not supported (integer occupations %g only)" % full)


def _b_tensor(qc, auxbasis):
    """the DFMI355 object that holds B[P, mu, nu]: the Hamiltonian's own, or one built here (and remembered per auxiliary basis)"""
    from .response import state_memo
    h = qc._engine.hamilton
    if h.df is not None and h.df.exchange:
        return h.df
    key = ("mp2_df", auxbasis if isinstance(auxbasis, str) or auxbasis is None else id(auxbasis))
    memo = state_memo(qc)
    if key not in memo:
        from .basis import make_aux_atombases
        from .df import DFMI355
        from .utils.datastruct import DensityFitInfo
        mol = qc.get_system()
        # None: the set Mol.densityfit() resolves its default to (the named fitting set when its tables are there, else the generated one)
        auxbases = make_aux_atombases(mol._atomzs, mol._atompos, "cc-pvtz-jkfit" if auxbasis is None else auxbasis, mol._atombases, {})
        info = DensityFitInfo(method="coulomb", auxbases=auxbases, exchange=True)
        memo[key] = DFMI355(info, h.atombases, h._orthozer, h.device).build()
    return memo[key]


def transform_ov(b, co, cv):
    """Bov[i, P, a] = sum_mu,nu co[mu, i] B[P, mu, nu] cv[nu, a], a padded with zero columns to a multiple of 16: (no, naux, ldv).
    Library matmuls over chunks of P, occupied index first (the cheaper order); no temporary is larger than the result"""
    naux, nao = int(b.shape[0]), int(b.shape[1])
    no, nv = int(co.shape[1]), int(cv.shape[1])
    ldv = (nv + 15) // 16 * 16
    need = 8 * no * naux * ldv
    free, _total = torch.cuda.mem_get_info(b.device)
    free += torch.cuda.memory_reserved(b.device) - torch.cuda.memory_allocated(b.device)  # (cached blocks are reusable)
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


def _orbitals(qc, frozen):
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


def _compute(qc, frozen, auxbasis):
    eng = qc._engine
    df = _b_tensor(qc, auxbasis)
    b = df._b
    spins = _orbitals(qc, frozen)
    bovs = [transform_ov(b, co, cv) for co, cv, _, _ in spins]
    if not eng.polarized:
        (_, _, eo, ev), bov = spins[0], bovs[0]
        pair_os, pair_ss = lib.mp2_pair_energies(bov, bov, eo, eo, ev, ev, True)
    else:
        (_, _, eoa, eva), (_, _, eob, evb) = spins
        pair_os, _ = lib.mp2_pair_energies(bovs[0], bovs[1], eoa, eob, eva, evb, False)
        pair_ss = tuple(0.5 * lib.mp2_pair_energies(bov, bov, eo, eo, ev, ev, True)[1] for bov, (_, _, eo, ev) in zip(bovs, spins))
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
    _unsupported(qc)
    from .response import state_memo
    memo = state_memo(qc)
    h = qc._engine.hamilton
    own = h.df is not None and h.df.exchange
    key = ("mp2", frozen, None if own else (auxbasis if isinstance(auxbasis, str) or auxbasis is None else id(auxbasis)))
    if key not in memo:
        with torch.no_grad():
            memo[key] = _compute(qc, frozen, auxbasis)
    df, pair_os, pair_ss, e_os, e_ss = memo[key]
    e_scf = qc.energy().detach().reshape(1)
    return MP2(e_scf, e_os, e_ss, pair_os, pair_ss, c_os, c_ss, frozen, df)


# `dqc_amd.mp2` is this function once the package has imported it: the yardstick stays reachable as dqc_amd.mp2.pair_energies_reference
mp2.pair_energies_reference = pair_energies_reference

__all__ = ["mp2", "MP2", "pair_energies_reference", "energies_reference", "components", "transform_ov"]
