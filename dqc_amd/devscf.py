"""Device-resident SCF loop of ONE molecule: every iteration is ONE hipGraph replay, the host never waits for the device.

The reference drives one self-consistency loop per molecule from the host (dqc/qccalc/scf_qccalc.py:84-116: `equilibrium` over
scp2scp = dm2scp(scp2dm(.)), engine steps hf.py:105-113 / ks.py:176-187).  Mirrored literally on a GPU -- dqc_amd/qccalc.py's
`_run_gen` -- every iteration ends in a blocking device -> host read (max|[F, D]| + the new DIIS Gram row), then the host solves
the Pulay system with numpy, uploads the coefficients, mixes, and only then launches the next step: measured on MI355X
(tools/gpu_one_molecule_iteration.py) 3.1 ms per iteration for a 20-atom cc-pVDZ molecule against 2.4 ms for the step's own
graph, 1.8 against 0.8 ms for benzene LDA and 1.2 against 0.6 ms for benzene RHF -- the device idles while the host thinks.

Here the whole iteration lives on the device and is captured ONCE:

    E = F D - D F, max|E|                      (the commutator of the entering pair)
    history rings, Gram row / column           index_copy_ with a DEVICE slot counter
    c = Pulay coefficients                     dqc_diis_solve_dev (valid slots read from the device counter)
    F_mix = sum_k c_k F_k
    P = projector(F_mix), Q = orth(P Omega)    GEMM-only purification (dqc_amd/purify.py), Cholesky QR
    D' = ao_orb2dm(Q, n), F' = dm2scp(D'), E_tot(D')   the Fock build (hcgto.py:204-269, 371-495)
    ring[k % 2] <- entering (F, D, E_tot);  pinned host <- (max|E|, projector error)      asynchronous copy

and the host loop is `replay(); look at the scalars of the iteration BEFORE the one just launched`.  The queue never drains: while
the device runs iteration k the host reads iteration k - 1's two doubles from pinned memory.  Convergence is therefore seen one
iteration late -- one speculative replay at the end -- and the converged pair is taken from the ring (the later iteration writes
the other slot).  Same numbers as `_run_gen`: same error vector, same history length, same minimum-norm Pulay solve, same
purification; the step from the core guess goes through eigh when its purification fails (degenerate bare-nucleus levels), a
later step that fails hands the run to `_run_gen` (vanishing gap: eigh needed), which also takes
everything it does not cover (a user dm0, non-uniform occupations, a raw AO basis, direct / sharded Hamiltonians).
"""
import torch

from . import lib, scfloop
from .utils.datastruct import SpinParam


def eligible(engine, dm0, opts) -> bool:
    """can `DeviceLoop` run this calculation?  (otherwise the host-driven generator of qccalc.py does); `opts`: scfloop.options"""
    if not isinstance(dm0, str) or dm0 != "1e":
        return False
    if not opts["graph"] or opts["driver"] != "device" or opts["diag"] != "purify":
        return False
    h = engine.hamilton
    if getattr(h, "_direct", False) or getattr(h, "sharded", False) or getattr(engine, "ovlp", None) is not None:
        return False
    return 1 <= int(opts["history"]) <= 16 and scfloop.uniform_occupations(engine) and not torch.cuda.is_current_stream_capturing()


class DeviceLoop:
    def __init__(self, engine, history: int = 12):
        from .graph import GraphedSCFStep
        self.eng = eng = engine
        self.pol = bool(eng.polarized)
        self.H = H = int(history)
        n, dev, dt = eng.shape[-1], eng.device, eng.dtype
        self.n, self.S = n, (2 if self.pol else 1)
        S = self.S
        self.step = GraphedSCFStep(eng, capture=False)
        # state of the loop (all static: the graph holds their addresses)
        self.fock = torch.zeros((S, n, n), dtype=dt, device=dev)
        self.dm = torch.zeros((S, n, n), dtype=dt, device=dev)
        self.etot = torch.zeros((), dtype=dt, device=dev)
        self.perr = torch.zeros((), dtype=dt, device=dev)          # projector error of the step that made (fock, dm)
        self.fh = torch.zeros((H, S * n * n), dtype=dt, device=dev)
        self.eh = torch.zeros((H, S * n * n), dtype=dt, device=dev)
        self.gram = torch.zeros((1, H, H), dtype=dt, device=dev)
        self.coef = torch.zeros((1, H), dtype=dt, device=dev)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)  # iterations done = vectors stored
        self.ring_f = torch.zeros((2, S, n, n), dtype=dt, device=dev)
        self.ring_d = torch.zeros((2, S, n, n), dtype=dt, device=dev)
        self.ring_e = torch.zeros(2, dtype=dt, device=dev)
        self.stats = torch.zeros((2, 2), dtype=dt, device=dev)      # per parity: max|[F, D]|, projector error of the entering pair
        self.host = torch.zeros((2, 2), dtype=dt).pin_memory()
        self.graph = None

    # ------------------------------------------------------------------ pieces
    def _load(self, fock, dm):
        """(fock, dm, etot) <- a pair as the engine returns it"""
        if self.pol:  # an unrestricted engine evaluates dm2energy of the final densities once, after the loop
            self.fock.copy_(fock)
            self.dm[0].copy_(dm.u)
            self.dm[1].copy_(dm.d)
        else:  # the two-electron parts are by-products of the build just made (the Hamiltonian's memo)
            self.fock[0].copy_(fock)
            self.dm[0].copy_(dm)
            self.etot.copy_(self.eng.dm2energy(dm))

    def _build_from(self, fmix):
        """(fock, dm, etot, perr) <- one step from the mixed Fock matrix (purification + Fock build)"""
        st = self.step
        st.f_in.copy_(fmix if self.pol else fmix[0])
        f_out, d_out, perr = st._body()
        self._load(f_out, d_out)
        self.perr.copy_(perr)

    def _iteration(self):
        H, S, n = self.H, self.S, self.n
        slot = self.count % H                       # (1,) int64 on the device
        par = self.count % 2
        a = torch.bmm(self.fock, self.dm)
        err = a - a.transpose(-2, -1)               # [F, D] per spin (both symmetric)
        ev = err.reshape(1, -1)
        self.eh.index_copy_(0, slot, ev)
        self.fh.index_copy_(0, slot, self.fock.reshape(1, -1))
        row = (self.eh * ev).sum(-1)                # scalar products with every stored error vector (unused slots hold zeros)
        self.gram[0].index_copy_(0, slot, row.reshape(1, H))
        self.gram[0].index_copy_(1, slot, row.reshape(H, 1))
        # the entering pair and its scalars go to the ring slot of this iteration's parity
        self.ring_f.index_copy_(0, par, self.fock.unsqueeze(0))
        self.ring_d.index_copy_(0, par, self.dm.unsqueeze(0))
        self.ring_e.index_copy_(0, par, self.etot.reshape(1))
        self.stats.index_copy_(0, par, torch.stack([err.abs().max(), self.perr]).reshape(1, 2))
        self.count += 1
        lib.diis_solve_dev(self.gram, self.count, self.coef)
        fmix = (self.coef[0].unsqueeze(-1) * self.fh).sum(0).reshape(S, n, n)
        self._build_from(fmix)
        self.host.copy_(self.stats, non_blocking=True)

    def _capture(self):
        dev = self.eng.device
        # warm-up on a side stream (allocator, lazy kernel attributes), from a scratch copy of the state; then capture
        state = (self.fock, self.dm, self.etot, self.perr, self.fh, self.eh, self.gram, self.count)
        keep = [t.clone() for t in state]
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            self._iteration()
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        for t, k in zip(state, keep):
            t.copy_(k)
        getattr(self.eng.hamilton, "_tiles", None) if self.eng.hamilton.df is None else None  # (retires the tile-fill event)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._iteration()
        for t, k in zip(state, keep):
            t.copy_(k)  # (a capture does not execute: belt and braces)
        self.eng.hamilton.clear_memos()

    # ------------------------------------------------------------------ the loop
    def _scalars(self, j):
        """(max|[F, D]|, projector error) of the entering pair of iteration j, from pinned memory (valid once the event recorded
        behind iteration j has completed)"""
        return float(self.host[j % 2, 0]), float(self.host[j % 2, 1])

    def run(self, qc, opts):
        """drive `qc` (an SCF_QCCalc) to convergence with `opts` (scfloop.options); returns None, or the scfloop.Handover with
        which the host-driven loop has to take over (a purification that did not converge: the step needs eigh)"""
        eng, n, S, dev = self.eng, self.n, self.S, self.eng.device
        f_tol, maxiter = float(opts["f_tol"]), int(opts["maxiter"])
        if maxiter < 1:
            raise RuntimeError("maxiter must be >= 1")
        # core guess (scf_qccalc.py:88-91): F0 = dm2scp(0), occupy its lowest orbitals -- the first step, eagerly
        f0 = scfloop.core_guess_fock(eng)
        self._build_from(f0.reshape(S, n, n))
        for t in (self.fh, self.eh, self.gram, self.count):
            t.zero_()
        if scfloop.projector_failed(float(self.perr)):   # (the one synchronisation before the loop)
            # the bare-nucleus Hamiltonian often has a degenerate or vanishing gap at the Fermi level (open pi shells, ...): this one
            # step through eigh, as the reference's (hf.py:137-150) -- later steps that fail hand the run to the host-driven loop
            qc.eigh_fallbacks += 1
            dm = eng.scp2dm(f0)
            self._load(eng.dm2scp(dm), dm)
            self.perr.zero_()
        if self.graph is None:
            self._capture()
        evs = [torch.cuda.Event(), torch.cuda.Event()]
        progress = scfloop.Progress(f_tol)
        qc.converged = qc.stalled = False
        stream = torch.cuda.current_stream(dev)

        def look(j):
            """host-side bookkeeping of iteration j: None to go on, or how the loop ends"""
            evs[j % 2].synchronize()
            emax, pe = self._scalars(j)
            qc.niter, qc.scf_error = j + 1, emax
            if opts["trace"]:
                print("scf it %2d  max|[F,D]| %.2e  (device loop)" % (j, emax), flush=True)
            if not scfloop.finite(emax):  # the host-driven loop starts over with eigh steps
                return "restart"
            if scfloop.projector_failed(pe):  # (vanishing gap): the host-driven loop resumes from the last good density
                return "fallback"
            progress.note(emax, j)  # (BEFORE the wander check; the host-driven loop notes after its own -- kept as found)
            if progress.wandering(emax, j):
                # the wander guard of the host-driven loop (qccalc.py): inside a degenerate Fermi level the purification step has no
                # preferred basis and the iteration never settles (UKS SCAN, oxygen triplet) -- hand over, eigh steps from the core guess
                return "restart"
            if progress.converged(emax):
                qc.converged = True
                return "done"
            if progress.stalled(emax, j):
                qc.stalled = True
                scfloop.warn_stalled(emax, f_tol)
                return "done"
            return None

        verdict = None
        for k in range(maxiter):
            self.graph.replay()
            evs[k % 2].record(stream)
            if k >= 1:
                verdict = look(k - 1)
                if verdict:
                    done_at = k - 1
                    break
        if verdict is None:
            verdict = look(maxiter - 1)
            done_at = maxiter - 1
            if verdict is None and scfloop.far_off(qc.scf_error):
                # out of iterations far from a fixed point: the reference's diagonalise-and-occupy step (hf.py:105-113) gets its turn
                # before the run is reported as not converged (the degenerate-level wander needs 40 steps to be told from slow progress)
                verdict = "restart"
        torch.cuda.synchronize(dev)
        # the entering pair of iteration `done_at` (the iteration launched after it wrote the other ring slot)
        p = done_at % 2
        if verdict == "restart":
            # wandering or non-finite: nothing of this run is worth resuming from (a non-finite commutator means the entering pair of
            # iteration `done_at` is already non-finite) -- the host-driven loop starts at the core guess WITHOUT the purification step
            return scfloop.Handover(purification=False)
        if verdict == "fallback":
            # a projector failure with a finite error: the entering density of the failing iteration is the last good iterate (every
            # earlier step passed its projector check) -- the host-driven loop resumes from it instead of the core guess
            if done_at < 1:
                return scfloop.Handover()
            d = self.ring_d[p]
            return scfloop.Handover(dm=SpinParam(u=d[0].clone(), d=d[1].clone()) if self.pol else d[0].clone(), projector_failures=1)
        scfloop.store_result(qc, self.ring_f[p], self.ring_d[p], self.ring_e[p], f_tol, stacked=True)
        return None
