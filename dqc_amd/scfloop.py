"""What the three SCF drivers decide alike: the host generator (qccalc.py), the device loop (devscf.py) and the lockstep batch
(lockstep.py) take their options, the core guess, the convergence policy, the stored result and the hand-over from here.
Policy and bookkeeping only: no tensor of an iteration lives here and nothing is launched except the core guess's Fock build."""
import math
import os
import warnings
from dataclasses import dataclass

import torch

from .utils.datastruct import SpinParam

# the convergence policy: one set of numbers for the three loops
IMPROVED = 0.9                 # an error below IMPROVED x the best so far counts as progress
STALL_BAND = 100               # x f_tol: how close to the tolerance an iterate without progress is accepted as `stalled`
STALL_STEPS = 8                # steps without progress before that
WANDER_STEPS = 40              # steps without progress ...
FAR_OFF = 1e-6                 # ... above this error: the purification step wanders (a degenerate Fermi level)
PROJECTOR_TOL = 1e-9           # projector error above which a purification step is redone through eigh
MAX_PROJECTOR_FAILURES = 3     # of one run, before the host loop drops the purification step


def options(fwd_options=None):
    """fwd_options over the defaults (the reference's xitorch solver: maxiter 50) and over the environment's fall-backs, read
    when a run starts; "trace" is a switch of the environment alone"""
    env = os.environ
    opts = {"maxiter": 50, "f_tol": 1e-9, "history": 12, "graph": env.get("DQC_AMD_GRAPH", "1") != "0",
            "diag": env.get("DQC_AMD_DIAG", "purify"), "driver": env.get("DQC_AMD_SCF_DRIVER", "device")}
    opts.update(fwd_options or {})
    opts["trace"] = bool(env.get("DQC_AMD_SCF_TRACE"))
    return opts


def core_guess_fock(engine):
    """F0 = dm2scp(0): the Fock matrix of the "1e" core guess (scf_qccalc.py:88-91)"""
    n = engine.shape[-1]
    z = torch.zeros((n, n), dtype=engine.dtype, device=engine.device)
    return engine.dm2scp(SpinParam(u=z, d=z) if engine.polarized else z)


def spin_channels(engine):
    """[(n_occ, occupation)] per spin channel (one entry for a restricted engine), or None when a channel's occupations are
    not uniform; an empty channel (the reference keeps one orbital of weight 0 there, mol.py:437-441) counts as n_occ = 0"""
    ws = [engine.orb_weight.u, engine.orb_weight.d] if engine.polarized else [engine.orb_weight]
    out = []
    for w in ws:
        occ = w.tolist()  # (one device -> host read per channel)
        if not any(occ):
            out.append((0, 0.0))
        elif all(o == occ[0] for o in occ):
            out.append((len(occ), occ[0]))
        else:
            return None
    return out


def uniform_occupations(engine) -> bool:
    """the purification step needs one occupation number per spin channel"""
    return spin_channels(engine) is not None


def finite(err) -> bool:
    return math.isfinite(err)


def far_off(err) -> bool:
    return err > FAR_OFF


def projector_failed(perr) -> bool:
    return not perr < PROJECTOR_TOL  # (a NaN has failed)


class Progress:
    """best max|[F, D]| of one molecule's run and the questions the drivers ask about it (each in its own order)"""

    def __init__(self, f_tol, start=0):
        self.f_tol = f_tol
        self.best_err, self.best_it = float("inf"), start

    def note(self, err, it):
        if err < self.best_err * IMPROVED:
            self.best_err, self.best_it = err, it

    def converged(self, err) -> bool:
        return err < self.f_tol

    def stalled(self, err, it, steps=STALL_STEPS) -> bool:
        """the commutator bottoms out at the round-off floor of the Fock build (fp64 atomics; ~1e-9 for ~200 AOs, growing with
        the matrix size): within STALL_BAND f_tol and `steps` steps without progress"""
        return err < STALL_BAND * self.f_tol and it - self.best_it >= steps

    def wandering(self, err, it) -> bool:
        return it - self.best_it >= WANDER_STEPS and far_off(err)


def drive(gen, sync=lambda t: t):
    """run a driver's generator (SCF_QCCalc._run_gen, LockstepSCF._run_gen) to its end synchronously: every device tensor it yields
    is answered with its numpy copy, a blocking device -> host read; `sync` sees the tensor first"""
    try:
        req = next(gen)
        while True:
            req = gen.send(sync(req).cpu().numpy())
    except StopIteration:
        pass


def warn_stalled(err, f_tol):
    warnings.warn("SCF stopped at the round-off floor of the Fock build: max|[F,D]| = %.2e (f_tol %.1e)" % (err, f_tol))


def store_result(qc, fock, dm, energy, f_tol, stacked=False):
    """the final iterate onto the calculation object.  `stacked`: (S, n, n) slices of a driver's state, copied out (S = 2: F_u,
    F_d and a SpinParam density, whose energy() evaluates dm2energy of the stored densities; S = 1: `energy` is dm2energy(dm) as
    evaluated with the Fock build of this very dm); otherwise the host loop's own tensors, kept"""
    if stacked:
        if dm.shape[0] == 2:
            fock, dm, energy = fock.clone(), SpinParam(u=dm[0].clone(), d=dm[1].clone()), None
        else:
            fock, dm, energy = fock[0].clone(), dm[0].clone(), energy.clone()
    qc._fock, qc._dm, qc._energy, qc._has_run = fock, dm, energy, True
    if not qc.accepted:  # the reference's xitorch solver emits a ConvergenceWarning here
        warnings.warn("SCF did not converge in %d iterations: max|[F,D]| = %.2e (f_tol %.1e); energy() and "
                      "nuclear_gradient() of this object refer to a non-stationary density" % (qc.niter, qc.scf_error, f_tol))


@dataclass
class Handover:
    """what the device loop leaves to the host loop when it cannot finish a run"""
    dm: object = None               # the last good density to resume from (None: the core guess)
    purification: bool = True       # may the host loop still take purification steps?  (False: the device loop wandered)
    projector_failures: int = 0     # so far in this run
