"""HF / KS drivers with the reference's surface -- HF(mol).run().energy(), KS(mol, xc=...).run().energy(),
.aodm(), .dm2energy(dm) -- and the same engine data flow:

   _HFEngine / _KSEngine:  dm2scp (Fock build), scp2dm (diagonalise, occupy), dm2energy
        dqc/qccalc/hf.py:93-119, 166-247 ; dqc/qccalc/ks.py:110-130, 157-187
   SCF_QCCalc.run: dm0 = "1e" core guess, then the fixed point F = dm2scp(scp2dm(F))
        dqc/qccalc/scf_qccalc.py:84-116 (reference: xitorch Broyden-1, alpha=-0.5, maxiter=50)

Everything runs on the device; the self-consistent parameter is the Fock matrix in the orthogonalised basis,
as in the reference.  The fixed-point solver is Pulay DIIS on the commutator [F, D] (any convergent mixer
gives the same fixed point; only converged energies are compared).  Restricted closed-shell and
unrestricted (UHF/UKS, SpinParam densities, stacked Fock matrices) are implemented."""
import os
import warnings
from typing import Optional

import numpy as np
import torch

from . import scfloop
from .utils.datastruct import SpinParam
from .xc import exx_fraction_of, get_xc


_DIIS_SCALE = os.environ.get("DQC_AMD_DIIS_SCALE", "1") != "0"


class _Engine:
    def __init__(self, system, xc=None, is_ks=False, restricted=None):
        self._system = system
        self.hamilton = system.get_hamiltonian()
        self.is_ks = is_ks
        self.xc = get_xc(xc) if is_ks else None
        # exact-exchange fraction of a hybrid functional, read ONCE as a float (not a trainable parameter); 0.0: every path below is
        # the pure Kohn-Sham / Hartree-Fock one
        self.exx = exx_fraction_of(self.xc) if is_ks else 0.0
        # hf.py:49-53: polarised iff spin != 0 unless `restricted` says otherwise
        self.polarized = bool(system.spin != 0) if restricted is None else (not restricted)
        # spin != 0 with restricted=True: one set of orbitals with occupations [2, ..., 2, 1, ..., 1] (mol.py:421-443) -- the
        # reference's restricted open-shell treatment; non-uniform occupations take the eigh step (no purification)
        # hf.py:55-57 / ks.py:69-71: the grid is needed by KS always and by HF when the system carries an external
        # potential (vext is integrated on the grid inside build())
        if not system.requires_grid():
            self.hamilton.build()  # first: the ERI tile fill runs on a side stream underneath the grid setup that follows
        if is_ks or system.requires_grid():
            system.setup_grid()
            self.hamilton.setup_grid(system.get_grid(), self.xc)
        self.hamilton.build()
        self.orb_weight = system.get_orbweight(polarized=self.polarized)
        self.norb = SpinParam.apply_fcn(lambda w: int(w.shape[-1]), self.orb_weight)
        self.knvext = self.hamilton.get_kinnucl()
        self.shape = self.knvext.shape
        self.dtype, self.device = self.knvext.dtype, self.knvext.device
        # (detached: the energy's derivatives come from dqc_amd.autograd, not from a graph through the SCF)
        self._enuc = torch.as_tensor(system.get_nuclei_energy()).detach().to(device=self.device, dtype=self.dtype)  # on the device once
        # Mol(orthogonalize_basis=False): the Fock matrix lives in the raw AO basis and `diagonalize` is the generalised problem
        # F C = S C e (hf.py:227-247: lsymeig(A=fock, M=ovlp)).  Solved through S^-1/2: C = S^-1/2 U, U from eigh(S^-1/2 F S^-1/2)
        self.ovlp, self._sinvh = None, None
        if not getattr(self.hamilton, "orthogonalized", True):
            self.ovlp = self.hamilton.get_overlap().fullmatrix()
            ev, evec = torch.linalg.eigh(self.ovlp)
            self._sinvh = (evec * ev ** -0.5) @ evec.transpose(-2, -1)

    def _eigpairs(self, fock):
        """(eigenvalues ascending, eigenvectors) of the symmetrised Fock matrix; S-orthonormal vectors of F C = S C e when the
        basis is not orthogonal"""
        fock = (fock + fock.transpose(-2, -1)) * 0.5
        if self._sinvh is None:
            return torch.linalg.eigh(fock)
        e, u = torch.linalg.eigh(self._sinvh @ fock @ self._sinvh)
        return e, self._sinvh @ u

    def _eigvecs(self, fock):
        return self._eigpairs(fock)[1]

    def get_system(self):
        return self._system

    def _core_matrix(self):
        """the one-electron part of the Fock matrix as a contiguous tensor (handed to the Hamiltonian's fused build, which adds it in
        the launch that forms X^T (J - K / 2 + V) X)"""
        c = getattr(self, "_core_cache", None)
        if c is None:
            c = self._core_cache = self.knvext.fullmatrix().contiguous()
        return c

    # Fock build -- THE hot path (hf.py:182-201, ks.py:176-187)
    def dm2scp(self, dm):
        """F = h + J + Vxc[D] (Kohn-Sham), h + J + get_exchange(D) (Hartree-Fock) or h + J + a get_exchange(D) + Vxc[D] (a hybrid,
        a = self.exx).  One (nao, nao) density or pair: one build of the Hamiltonian (hamilton.py: _fock2e, _fock2e_pol), the core
        Hamiltonian added in its last launch; batched densities, and what the builds do not cover, through the operators' own sum"""
        h, a = self.hamilton, self.exx
        if self.polarized:  # scp = stacked (F_u, F_d)  (hf.py:93-103)
            if not isinstance(dm, SpinParam):
                dm = SpinParam(u=dm[0], d=dm[1])
            if dm.u.dim() == 2 and a != 0.0:
                return h.get_elrep_plus_exchange_plus_vxc_pol(dm, core=self._core_matrix())
            if dm.u.dim() == 2 and self.is_ks and h.tiles_resident:
                return h.get_elrep_plus_vxc_pol(dm, core=self._core_matrix())
            if dm.u.dim() == 2 and not self.is_ks and h.df is None:
                # J[D_u + D_d], -K[2 D_u]/2, -K[2 D_d]/2 from ONE pass over the ERI tiles instead of three
                J, kx = h.get_elrep_exchange_pol(dm)
                hj = self.knvext.fullmatrix() + J
                return torch.stack([hj + kx.u, hj + kx.d])
            hj = self.knvext + h.get_elrep(dm.u + dm.d)
            v = h.get_vxc(dm) if self.is_ks else h.get_exchange(dm)
            fock = [(hj + v.u).fullmatrix(), (hj + v.d).fullmatrix()]
            if a != 0.0:
                k = h.get_exchange(dm)
                fock = [fock[0] + a * k.u.fullmatrix(), fock[1] + a * k.d.fullmatrix()]
            return torch.stack(fock)
        if dm.dim() == 2 and a != 0.0:
            return h.get_elrep_plus_exchange_plus_vxc(dm, core=self._core_matrix())
        if dm.dim() == 2 and self.is_ks:
            return h.get_elrep_plus_vxc(dm, core=self._core_matrix())
        if dm.dim() == 2 and (h.df is None or h.df.exchange):  # (fitted J and K: the same build in its torch form)
            return h.get_elrep_plus_exchange(dm, core=self._core_matrix())
        fock = (self.knvext + h.get_elrep(dm) + (h.get_vxc(dm) if self.is_ks else h.get_exchange(dm))).fullmatrix()
        return fock if a == 0.0 else fock + a * h.get_exchange(dm).fullmatrix()

    def scp2dm(self, scp):
        if self.polarized:
            out = []
            for f, w, n in ((scp[0], self.orb_weight.u, self.norb.u), (scp[1], self.orb_weight.d, self.norb.d)):
                out.append(self.hamilton.ao_orb2dm(self._eigvecs(f)[..., :n], w))
            return SpinParam(u=out[0], d=out[1])
        return self.hamilton.ao_orb2dm(self.scp2orb(scp), self.orb_weight)

    def scp2orb(self, scp):
        """occupied orbitals of a (restricted) Fock matrix: the `diagonalize` step of hf.py:227-247"""
        # generalised problem F C = S C e; S = identity in the orthogonalised basis
        return self._eigvecs(scp)[..., :self.norb]

    def scp2scp(self, scp):
        return self.dm2scp(self.scp2dm(scp))

    def dm2energy(self, dm):
        h = self.hamilton
        tot = SpinParam.sum(dm)  # hf.py:166-172 / ks.py:157-166: core and Coulomb terms see the total density
        e = h.get_e_hcore(tot) + h.get_e_elrep(tot) + (h.get_e_xc(dm) if self.is_ks else h.get_e_exchange(dm))
        if self.exx != 0.0:  # a E_K of the hybrid functional (a by-product of the build of this density)
            e = e + h.get_e_exchange_hybrid(dm)
        return e + self._enuc

    def energy_parts(self, dm):
        h = self.hamilton
        tot = SpinParam.sum(dm)
        p = {"e_core": float(h.get_e_hcore(tot)), "e_elrep": float(h.get_e_elrep(tot)),
             "e_nuc": float(self._system.get_nuclei_energy())}
        p["e_xc" if self.is_ks else "e_exch"] = float(h.get_e_xc(dm) if self.is_ks else h.get_e_exchange(dm))
        if self.exx != 0.0:
            p["e_exch"] = float(h.get_e_exchange_hybrid(dm))
        p["e_tot"] = sum(p.values())
        return p


def _commutator(fock, dm, ovlp):
    """[F, D] (S = 1) or F D S - S D F, S the overlap of a non-orthogonalised basis (None: identity); stacked over the spin
    channels of an unrestricted pair"""
    d = torch.stack([dm.u, dm.d]) if isinstance(dm, SpinParam) else dm
    return fock @ d - d @ fock if ovlp is None else fock @ d @ ovlp - ovlp @ d @ fock


class _HostDIIS:
    """Pulay mixing of the host-driven loop: Fock matrices and error vectors stay on the device, the Gram matrix lives on the
    host and grows by the row the loop reads each iteration"""

    def __init__(self, history):
        self.history = int(history)
        self.reset()

    def reset(self):
        self.fs, self.es, self.gram = [], [], np.zeros((0, 0))

    def gram_row(self, ev):
        """(device) the error vector `ev` against the stored ones that survive its insertion, and itself"""
        hist = self.es[-(self.history - 1):] if self.history > 1 else []
        return (torch.stack(hist + [ev]) * ev).sum(-1)

    def mix(self, fock, ev, grow):
        """store (fock, ev) with the host copy `grow` of gram_row(ev); returns the Pulay mix of the stored Fock matrices"""
        self.fs.append(fock)
        self.es.append(ev)
        if len(self.fs) > self.history:
            self.fs.pop(0)
            self.es.pop(0)
        m = len(self.fs)
        # the Gram matrix lives on the host and grows by the row just read (broadcast-multiply-reduce on the device:
        # the GEMM form E @ E.T hits a pathological rocBLAS path for the tall-skinny fp64 shape, 7 ms for 8 x 43264)
        keep = m - 1  # the stored vectors that survive
        gram = np.zeros((m, m))
        if keep:
            gram[:keep, :keep] = self.gram[-keep:, -keep:]
        gram[keep, :] = grow
        gram[:, keep] = grow
        self.gram = gram
        if m == 1:
            return fock
        B = np.zeros((m + 1, m + 1))
        # the Pulay coefficients do not change when the Gram block is scaled (only the multiplier does): normalised to
        # a unit largest diagonal, otherwise lstsq's rank cut (eps x largest singular value, set by the +-1 border)
        # discards the whole Gram block once the errors fall below ~1e-8 and the mix degrades to a plain average
        B[:m, :m] = gram / max(float(np.max(np.diag(gram))), 1e-300) if _DIIS_SCALE else gram
        B[m, :m] = -1
        B[:m, m] = -1
        rhs = np.zeros(m + 1)
        rhs[m] = -1
        # (m+1) x (m+1) Pulay system on the host with numpy: torch's CPU lstsq costs ~7 ms per call on a
        # 256-thread box (thread-pool wake-up), several times the whole Fock build
        try:
            c = np.linalg.lstsq(B, rhs, rcond=None)[0][:m] if np.isfinite(B).all() else None
        except np.linalg.LinAlgError:  # (LAPACK's SVD gives up on an ill-scaled or non-finite Gram block)
            c = None
        if c is None or not np.isfinite(c).all():
            # a Pulay system that cannot be solved: forget the history and take the plain step from this Fock matrix (the next
            # iterations rebuild the history; a non-finite commutator is caught at the top of the loop)
            self.fs, self.es, self.gram = [fock], [ev], np.array([[float(grow[-1])]])
            c = np.ones(1)
        c = torch.as_tensor(c, dtype=fock.dtype).to(fock.device)
        return (c.reshape((-1,) + (1,) * fock.dim()) * torch.stack(self.fs)).sum(0)


def _choose_step(eng, opts, purification):
    """(GraphedSCFStep or None, GraphedFock or None): how the host-driven loop gets from a mixed Fock matrix to the next pair.
    Restricted engines replay the Fock build as one hipGraph (dqc_amd/graph.py); "graph": False runs it eagerly.
    "diag": "purify" (default for uniform occupations) replaces eigh by GEMM-only purification inside the same graph
    (dqc_amd/purify.py); "eigh" keeps the reference's diagonalise-and-occupy step (hf.py:105-113)"""
    # (direct SCF builds allocate stream-ordered scratch and upload pair tables per call: not captured)
    # (nor the builds of a Hamiltonian sharded over several GPUs: they hold collectives)
    # A direct-SCF engine still takes the purification step, launched eagerly: the 412 x 412 eigh of naphthalene / cc-pVTZ is
    # 6 ms of rocSOLVER launches per iteration against ~1 ms of GEMMs
    ham = getattr(eng, "hamilton", None)
    direct = bool(getattr(ham, "_direct", False))
    if not opts["graph"] or getattr(ham, "sharded", False):
        return None, None
    from .graph import GraphedFock, GraphedSCFStep
    if opts["diag"] == "purify" and scfloop.uniform_occupations(eng) and getattr(eng, "ovlp", None) is None and purification:
        return GraphedSCFStep(eng, capture=not direct), None
    if not eng.polarized and not direct:
        return None, GraphedFock(eng)
    return None, None


def _take_step(eng, fmix, purified, graphed):
    """(fock, dm, projector error or None) of the step from the mixed Fock matrix `fmix`"""
    if purified is not None:
        f_out, d_out, perr = purified(fmix)
        if purified.graph is None:  # eager step (direct SCF): fresh tensors, and the Hamiltonian's caches stay keyed on them
            return f_out, d_out, perr
        # static buffers of the graph: copy out
        dm = SpinParam(u=d_out.u.clone(), d=d_out.d.clone()) if eng.polarized else d_out.clone()
        return f_out.clone(), dm, perr.clone()
    if graphed is not None:
        fock = graphed(eng.scp2orb(fmix)).clone()
        return fock, graphed.density_matrix().clone(), None
    dm = eng.scp2dm(fmix)
    return eng.dm2scp(dm), dm, None


class SCF_QCCalc:
    def __init__(self, engine):
        self._engine = engine
        self._has_run = False
        self.niter = 0
        self.converged = False   # max|[F, D]| < f_tol
        self.stalled = False     # stopped at the round-off floor of the Fock build, above f_tol (see run())
        self.scf_error = float("inf")  # max|[F, D]| of the returned iterate -- the achieved error, whatever the exit
        self.fock_residual = None      # the reference's own fixed-point residual max|F_out - F_in| (host-driven loop)
        self.driver_used = None        # "device" / "host": which loop produced the result (diagnostics / tests)
        self.eigh_fallbacks = 0        # purification steps redone through eigh (accumulates over run() calls; lockstep resets it)
        self.purification_dropped = False  # a run gave up the purification step for eigh steps from the core guess (sticky)
        self._devloop = None           # the DeviceLoop of this object, kept for the next run()
        self._dm = self._fock = self._energy = None

    @property
    def accepted(self):
        """the run ended at a fixed point: either `converged` (f_tol met) or `stalled` at the round-off floor with
        `scf_error` < 100 f_tol; `scf_error` says what was achieved"""
        return self.converged or self.stalled

    def get_system(self):
        return self._engine.get_system()

    def run(self, dm0="1e", eigen_options=None, fwd_options=None, bck_options=None):
        """the SCF loop, driven synchronously: every host read of the generator below is a blocking device -> host copy.
        dqc_amd.batch.run_concurrent drives many of these generators at once, one stream per molecule."""
        # one molecule, core guess, purification step: the whole iteration replays as ONE hipGraph and the host only looks at two
        # doubles per iteration, one iteration late (dqc_amd/devscf.py); everything else takes the host-driven generator below,
        # and so does what the device loop hands over (a projector failure mid-run, a wandering purification)
        from . import devscf
        opts = scfloop.options(fwd_options)
        handover = None
        if self._engine.device.type == "cuda" and devscf.eligible(self._engine, dm0, opts):
            if self._devloop is None or self._devloop.H != int(opts["history"]):
                self._devloop = devscf.DeviceLoop(self._engine, int(opts["history"]))
            handover = self._devloop.run(self, opts)
            if handover is None:
                self.driver_used = "device"
                return self
        self.driver_used = "host"
        # a Hamiltonian sharded over several GPUs (HamiltonMI355.shard_over) runs this loop on every rank: the scalars the
        # driver decides on are rank 0's, so that every rank takes the same branch and issues the same collectives
        sync = getattr(getattr(self._engine, "hamilton", None), "sync_scalars", lambda t: t)
        scfloop.drive(self._run_gen(dm0, fwd_options, handover), sync)
        return self

    def _initial_density(self, dm0):
        eng = self._engine
        if isinstance(dm0, str):
            if dm0 != "1e":
                raise RuntimeError("Unknown dm0: %s" % dm0)
            dm = eng.scp2dm(scfloop.core_guess_fock(eng))
        elif dm0 is None:
            raise RuntimeError("dm0 must be '1e' or a density matrix")
        else:
            dm = SpinParam.apply_fcn(lambda d: d.to(eng.device), dm0)
        if eng.polarized and not isinstance(dm, SpinParam):  # scf_qccalc.py:97-100
            dm = SpinParam(u=dm * 0.5, d=dm * 0.5)
        return dm

    def _run_gen(self, dm0="1e", fwd_options=None, handover=None):
        """generator form of run(): yields the (small) device tensor it needs on the host -- ONE per SCF iteration -- and is
        resumed with that tensor's numpy copy; everything else is enqueued on the current stream without synchronising.
        `handover`: what the device loop left (scfloop.Handover) when it could not finish this run"""
        opts = scfloop.options(fwd_options)
        eng = self._engine
        handover = handover or scfloop.Handover()
        dm = self._initial_density(dm0 if handover.dm is None else handover.dm)
        fock = eng.dm2scp(dm)
        if not handover.purification:  # (the device loop wandered: eigh steps from the start)
            self.purification_dropped = True
        purified, graphed = _choose_step(eng, opts, handover.purification)
        ovlp = getattr(eng, "ovlp", None)
        diis = _HostDIIS(opts["history"])
        progress = scfloop.Progress(opts["f_tol"])
        perr = fprev = None
        self.converged = self.stalled = False
        # iteration budget: `maxiter` steps -- and `maxiter` more from the restart, once, when the purification step is dropped (the
        # reference's diagonalise-and-occupy iteration gets the cap the caller set; the steps the purification wandered do not count)
        it, it_end = -1, int(opts["maxiter"])
        nfail = handover.projector_failures
        while it + 1 < it_end:
            it += 1
            self.niter = it + 1
            err = _commutator(fock, dm, ovlp)
            # ONE host read per iteration: max |[F, D]|, the projector error of the step just taken, and the new row of the
            # DIIS Gram matrix (this error vector against the stored ones) travel together
            ev = err.reshape(-1)
            zero = torch.zeros((), dtype=fock.dtype, device=fock.device)
            # the reference's own fixed-point residual max|F_out - F_in| (scp2scp(y) - y, scf_qccalc.py:109-113) rides along
            fres_t = (fock - fprev).abs().max() if fprev is not None else zero + float("inf")
            head = torch.stack([err.abs().max(), perr if perr is not None else zero, fres_t])
            host = yield torch.cat([head, diis.gram_row(ev)])
            emax, pe, fres, grow = float(host[0]), float(host[1]), float(host[2]), host[3:]
            self.fock_residual = fres
            if opts["trace"]:
                print("scf it %2d  max|[F,D]| %.2e  max|F_out-F_in| %.2e" % (it, emax, fres), flush=True)
            if perr is not None and scfloop.projector_failed(pe):
                # purification did not converge (vanishing gap): redo this step through eigh
                self.eigh_fallbacks += 1
                nfail += 1
                dm = eng.scp2dm(fprev)
                fock = eng.dm2scp(dm)
                perr = None
                err = _commutator(fock, dm, ovlp)
                ev = err.reshape(-1)
                h2 = yield torch.cat([err.abs().max().reshape(1), diis.gram_row(ev)])
                emax, grow = float(h2[0]), h2[1:]
            if purified is not None and (not scfloop.finite(emax) or progress.wandering(emax, it)
                                         or nfail >= scfloop.MAX_PROJECTOR_FAILURES
                                         or (it + 1 >= it_end and scfloop.far_off(emax))):
                # The purification step has no preferred basis inside a degenerate Fermi level (open p shells, ...): every step then
                # lands on another rotation of the degenerate orbitals, the iteration wanders for ever and the DIIS system eventually
                # blows up (UKS SCAN on the oxygen triplet: NaN after 88 steps, or -26 Ha).  The reference diagonalises (hf.py:105-113),
                # which fixes the orbitals: after 40 steps without progress -- or at the first non-finite error -- the loop drops the
                # purification and starts again from the core guess with eigh steps and a fresh history
                self.purification_dropped = True
                purified = graphed = perr = fprev = None
                diis.reset()
                # (from the core guess again: continued from the best wandering iterate the eigh steps did not settle in 160 more
                # iterations on that system, from the core guess they converge in 23)
                dm = eng.scp2dm(scfloop.core_guess_fock(eng))
                fock = eng.dm2scp(dm)
                progress = scfloop.Progress(opts["f_tol"], start=it)
                it_end = it + 1 + int(opts["maxiter"])
                continue
            self.scf_error = emax  # max |[F, D]| of the last iterate
            progress.note(emax, it)  # (AFTER the wander check above; the device loop notes before its own -- kept as found)
            # (the reference's fixed-point residual max|F_out - F_in|, kept in self.fock_residual, runs ~3x the commutator;
            # stopping on it as well -- 3e-9 or SURVEY.md 8d's 1e-8 -- saves 1-7 % of the iterations but costs a digit in the
            # non-variational energy components that the goldens pin to 1e-7: not done)
            if progress.converged(emax):
                self.converged = True
                break
            # an iterate that is within 100 f_tol and has not improved for 8 steps ends the loop as `stalled` -- `converged`
            # keeps meaning f_tol, `scf_error` reports what was achieved
            if progress.stalled(emax, it):
                self.stalled = True
                scfloop.warn_stalled(emax, opts["f_tol"])
                break
            fprev = diis.mix(fock, ev, grow)
            fock, dm, perr = _take_step(eng, fprev, purified, graphed)
        scfloop.store_result(self, fock, dm, None, opts["f_tol"])

    def energy(self):
        """the converged energy; differentiable (torch.autograd) with respect to the caller's positions, floating-point charges,
        efield, vext, orb_weights and the parameters of a torch.nn.Module functional (dqc_amd/autograd.py) -- when none of them
        requires grad, or grad mode is off, the plain detached tensor"""
        assert self._has_run
        e = self._energy  # the lockstep and device-loop drivers keep dm2energy(dm) of the final Fock build (same call, same dm)
        if e is None:
            e = self._engine.dm2energy(self._dm)
        from . import autograd
        return autograd.energy(self, e)

    def aodm(self):
        assert self._has_run
        return self._dm

    def nuclear_gradient(self):
        """dE/dR (natm, 3) of the converged energy -- what the reference gets from torch.autograd.grad(energy, atompos)
        (test_hf.py:78-111, test_ks.py:114-137); restricted HF and LDA (dqc_amd/gradient.py)"""
        assert self._has_run
        if not self.accepted:  # the analytic gradient has no orbital-response terms: it is only valid at a fixed point
            warnings.warn("nuclear_gradient() of an unconverged SCF (max|[F,D]| = %.2e) is not the derivative of its energy"
                          % self.scf_error)
        from .gradient import nuclear_gradient
        return nuclear_gradient(self)

    def basis_gradient(self):
        """dE/d(exponent), dE/d(normalised coefficient) of every primitive of the basis table, (nprim_total, 2), of the converged
        energy (dqc_amd/gradient.py); torch.autograd.grad(energy, CGTOBasis tensors) chains it to the caller's tensors"""
        assert self._has_run
        if not self.accepted:
            warnings.warn("basis_gradient() of an unconverged SCF (max|[F,D]| = %.2e) is not the derivative of its energy"
                          % self.scf_error)
        from .gradient import basis_gradient
        return basis_gradient(self)

    def dm2energy(self, dm):
        return self._engine.dm2energy(dm)


class HF(SCF_QCCalc):
    def __init__(self, system, restricted: Optional[bool] = None, variational: bool = False):
        if variational:
            raise NotImplementedError("the variational solver is out of scope (SURVEY.md 2, row 3)")
        super().__init__(_Engine(system, None, is_ks=False, restricted=restricted))
        self._ctor_kwargs = {"restricted": restricted}  # to rebuild the same calculation on another geometry


class KS(SCF_QCCalc):
    def __init__(self, system, xc, restricted: Optional[bool] = None, variational: bool = False):
        if variational:
            raise NotImplementedError("the variational solver is out of scope (SURVEY.md 2, row 3)")
        super().__init__(_Engine(system, xc, is_ks=True, restricted=restricted))
        self._ctor_kwargs = {"xc": xc, "restricted": restricted}
