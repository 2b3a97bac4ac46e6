"""Neutral (optical) excitations from the Bethe-Salpeter equation with static screening on G0W0 quasiparticle energies (BSE@G0W0), with
density-fitted integrals on a converged restricted HF or KS calculation.  Orbitals i, j occupied, a, b virtual, real.

    D_ia    = E_a - E_i                                                   E: quasiparticle energies (below)
    M       = (1 + Q(0))^-1                                               the static dielectric inverse in the auxiliary basis; Q(0) the
                                                                          dRPA response of dqc_amd/rpa.py at w = 0 on the SCF energies
    W_ij,ab = sum_PR B_ij^P M_PR B_ab^R                                   the statically screened interaction, never formed
    (Wd X)_ia = sum_jb W_ij,ab X_jb = sum_P sum_jb (M Boo)[i, P, j] X[j, b] Bvv[a, P, b]                        (csrc/bse.hip)
    (Wx X)_ia = sum_jb W_ib,ja X_jb = sum_P sum_bj (M Bov)[i, P, b] X^T[b, j] Bvo[a, P, j]                      (csrc/bse.hip)
    (v X)_ia  = sum_P Bov[i, P, a] (sum_jb Bov[j, P, b] X_jb)                                                   (two library GEMMs)
    singlet  A = D + 2 v - Wd,  B = 2 v - Wx;          triplet  A = D - Wd,  B = -Wx

TDA solves A X = w X (`response.davidson_lowest`); the full problem hands (A + B) = D + 2 c v - Wd - Wx and (A - B) = D - Wd + Wx
(c = 2 singlet, 0 triplet) to `response.response_eigs`, whose "not positive definite" errors are the right answer to a triplet
instability.  With M = 1 and E = eps this is RI-TDHF / RI-CIS (`screened=False`): the link to `dqc_amd.excitations`.  Transition dipoles
and oscillator strengths as there: mu = sqrt 2 (X + Y) . r_ia, f = 2 / 3 w |mu|^2, zero for triplets.

QUASIPARTICLE ENERGIES.  `gw` continues the self-energy from the imaginary axis, which is reliable near the Fermi level only
(dqc_amd/gw.py), so it is asked for a window of the highest window[0] occupied and the lowest window[1] virtual orbitals only.  The
occupied orbitals below the window are shifted rigidly by the correction E - eps of the lowest corrected occupied orbital, the virtual
ones above it by that of the highest corrected virtual orbital (a scissor: `quasiparticle_ladder`).  A target orbital whose
quasiparticle equation did not converge raises.  `qp=` takes all nmo energies as they are.

Limits: static screening only (no dynamical kernel), restricted closed shell, no gradient and no autograd (the result is detached).
Memory: Bvv (nvir, naux, nvir padded), Bvo, Bov, Boo and the screened copies of the last two must fit in device memory at once; there
is no batching over virtual blocks.

`exchange_reference`, `static_w_reference` and `bse_reference` are the yardsticks: plain torch on any device."""
import torch

from . import lib
from .postscf import aux_key, b_tensor, free_bytes, memoised, orbitals, transform_ov, unsupported
from .properties import Excitations
from .response import davidson_lowest, response_eigs


# ---------------------------------------------------------------------------------------------------------------- yardsticks
def exchange_reference(l, x, r, nr, ns):
    """out[v, p, q] = sum_P sum_{r < nr} sum_{s < ns} l[p, P, r] x[v, r, s] r[q, P, s] in plain torch, on the device of the inputs:
    the yardstick of dqc_bse_exchange.  l (np, naux, >= nr), r (nq, naux, >= ns): columns past nr and ns (padding) are ignored;
    x (nvec, nr, ns) -> (nvec, np, nq).  One vector at a time, the intermediate Z[r, q, P] stored"""
    nr, ns = int(nr), int(ns)
    np_, naux, nq, nvec = int(l.shape[0]), int(l.shape[1]), int(r.shape[0]), int(x.shape[0])
    lm = l[:, :, :nr].reshape(np_, naux * nr)
    rm = r[:, :, :ns].reshape(nq * naux, ns)
    out = torch.zeros((nvec, np_, nq), dtype=l.dtype, device=l.device)
    for v in range(nvec):
        z = torch.matmul(x[v], rm.t()).view(nr, nq, naux)                       # Z[r, q, P]
        out[v] = torch.matmul(lm, z.permute(2, 0, 1).reshape(naux * nr, nq))
    return out


def static_w_reference(boo_like, bvv_like, m):
    """the dense W[i, j, a, b] = sum_PR boo_like[i, P, j] m[P, R] bvv_like[a, R, b] from two slab tensors (n1, naux, n2) taken as they
    are (no padding columns) and the matrix m (naux, naux)"""
    return torch.einsum("ipj,pr,arb->ijab", boo_like, m, bvv_like)


def bse_matrices(bmo, eps_qp, nocc, m=None, spin="singlet"):
    """the dense (A, B) of the module docstring over the whole occupied-virtual space, (i, a) flattened row-major: bmo (nmo, naux, >= nmo)
    the tensor over ALL orbitals [p, P, q], eps_qp (nmo) the energies in D, nocc, m (naux, naux) the dielectric inverse (None: 1)"""
    if spin not in ("singlet", "triplet"):
        raise ValueError("bse_reference: spin is \"singlet\" or \"triplet\", not %r" % (spin,))
    eps_qp = torch.as_tensor(eps_qp, dtype=bmo.dtype).to(bmo.device)
    no, nmo = int(nocc), int(eps_qp.numel())
    n = no * (nmo - no)
    boo, bov, bvv = bmo[:no, :, :no], bmo[:no, :, no:nmo], bmo[no:nmo, :, no:nmo]
    if m is None:
        m = torch.eye(int(bmo.shape[1]), dtype=bmo.dtype, device=bmo.device)
    v = torch.einsum("ipa,jpb->iajb", bov, bov).reshape(n, n)
    wd = static_w_reference(boo, bvv, m).permute(0, 2, 1, 3).reshape(n, n)          # [ia, jb] = W_ij,ab
    wx = static_w_reference(bov, bov, m).permute(0, 3, 2, 1).reshape(n, n)          # W[i, b, j, a] -> [ia, jb] = W_ib,ja
    c = 2.0 if spin == "singlet" else 0.0
    d = (eps_qp[None, no:] - eps_qp[:no, None]).reshape(n)
    return torch.diag(d) + c * v - wd, c * v - wx


def solve_dense(a, b, tda=False):
    """(w (n), xpy (n, n): one state per row, normalised as `bse` does) of dense symmetric A and B: TDA by eigh(A), the full problem by
    the symmetric form (A - B)^1/2 (A + B) (A - B)^1/2 Z = w^2 Z, X + Y = (A - B)^1/2 Z / sqrt(w)"""
    a, b = 0.5 * (a + a.t()), 0.5 * (b + b.t())
    if tda:
        w, x = torch.linalg.eigh(a)
        return w, x.t().contiguous()
    e, u = torch.linalg.eigh(a - b)
    if not float(e[0]) > 0.0:
        raise RuntimeError("bse_reference: A - B is not positive definite (lowest eigenvalue %.3e)" % float(e[0]))
    rt = (u * e.sqrt()) @ u.t()
    w2, z = torch.linalg.eigh(rt @ (a + b) @ rt)
    if not float(w2[0]) > 0.0:
        raise RuntimeError("bse_reference: A + B is not positive definite (lowest w^2 %.3e)" % float(w2[0]))
    w = w2.sqrt()
    return w, ((rt @ z) / w.sqrt()[None, :]).t().contiguous()


def bse_reference(bmo, eps_qp, nocc, m=None, spin="singlet", tda=False):
    """every excitation energy with X + Y from dense A and B over the whole occupied-virtual space: `solve_dense` on `bse_matrices`
    (their arguments) -> (w (n), xpy (n, n)).  O((o v)^3), for small ov spaces"""
    return solve_dense(*bse_matrices(bmo, eps_qp, nocc, m, spin), tda=tda)


def quasiparticle_ladder(eps, nocc, orbs, qp):
    """all nmo quasiparticle energies from those of a window: eps (nmo) the orbital energies, orbs the corrected orbitals (indices in
    energy order), qp their quasiparticle energies.  A corrected orbital takes its own energy; an occupied orbital that is not
    corrected is shifted by the correction E - eps of the LOWEST corrected occupied orbital, a virtual one by that of the HIGHEST
    corrected virtual orbital (the scissor of the module docstring); a side without a corrected orbital keeps eps"""
    eps = torch.as_tensor(eps, dtype=torch.float64)
    qp = torch.as_tensor(qp, dtype=torch.float64).to(eps.device)
    orbs, nocc, nmo = [int(o) for o in orbs], int(nocc), int(eps.numel())
    if qp.dim() != 1 or int(qp.numel()) != len(orbs) or len(set(orbs)) != len(orbs) or any(o < 0 or o >= nmo for o in orbs):
        raise ValueError("quasiparticle_ladder: %d energies for the orbitals %s of %d" % (int(qp.numel()), orbs, nmo))
    out = eps.clone()
    occ = [j for j, o in enumerate(orbs) if o < nocc]
    vir = [j for j, o in enumerate(orbs) if o >= nocc]
    if occ:
        j = min(occ, key=lambda k: orbs[k])
        out[:nocc] = eps[:nocc] + (qp[j] - eps[orbs[j]])
    if vir:
        j = max(vir, key=lambda k: orbs[k])
        out[nocc:] = eps[nocc:] + (qp[j] - eps[orbs[j]])
    for j, o in enumerate(orbs):
        out[o] = qp[j]
    return out


def window_orbitals(nocc, nmo, window):
    """the orbitals of the quasiparticle window: the highest window[0] occupied and the lowest window[1] virtual ones, clipped to what exists"""
    return list(range(max(nocc - int(window[0]), 0), min(nocc + int(window[1]), nmo)))


# ---------------------------------------------------------------------------------------------------------------- the method
class BSE(Excitations):
    """what `bse` returns (detached tensors on the host): the fields of `properties.Excitations` -- `energies` (nstates) in Hartree,
    ascending; `transition_dipoles` (nstates, 3), `osc_strengths` (nstates) (length gauge; zero for triplets); `xpy`, `xmy`
    (nstates, nocc nvir): X + Y and X - Y, the pair (i, a) flattened row-major (OCCUPIED index first, as the kernel writes them), (X + Y) .
    (X - Y) = 1 (TDA: xpy = X, X . X = 1, xmy None); `spin`, `tda`, `residual` -- and `qp_energies` (nmo: the energies in D, after the
    ladder), `window_orbs` (the orbitals `gw` was asked for; None without it), `gw` (the `GW` object, or None), `screened`, `naux`,
    `df` (the DFMI355 object whose tensor was used)"""

    def __init__(self, energies, transition_dipoles, osc_strengths, xpy, xmy, spin, tda, residual, qp_energies, window_orbs, gw, screened,
                 df):
        super().__init__(energies, transition_dipoles, osc_strengths, xpy, xmy, spin, tda, residual)
        self.qp_energies, self.window_orbs, self.gw, self.screened, self.df = qp_energies, window_orbs, gw, bool(screened), df
        self.naux = int(df._b.shape[0])

    def __repr__(self):
        return "BSE(%s%s%s, energies=%s, osc_strengths=%s, naux=%d)" % (
            self.spin, ", TDA" if self.tda else "", "" if self.screened else ", unscreened", self.energies.tolist(),
            self.osc_strengths.tolist(), self.naux)


def _tensors(qc, auxbasis, screened):
    """what every product needs, on the device: the four slab tensors, the screened copies of Boo and Bov (the same objects when
    screened is False), Bov as a (naux, nocc nvir) matrix for the Coulomb term, Q(0) and the Cholesky factor of 1 + Q(0)"""
    df = b_tensor(qc, auxbasis)
    b = df._b
    co, cv, eo, ev = orbitals(qc, 0)[0]
    no, nv, naux = int(co.shape[1]), int(cv.shape[1]), int(b.shape[0])
    if no == 0 or nv == 0:
        raise NotImplementedError("bse: a calculation without occupied or without virtual orbitals has no excitations")
    ldo, ldv = (no + 15) // 16 * 16, (nv + 15) // 16 * 16
    k = 2 if screened else 1
    need = 8 * naux * (nv * ldv + nv * ldo + k * no * (ldv + ldo) + no * nv) + (3 * 8 * naux * naux if screened else 0)
    free = free_bytes(b.device)
    if need > free:
        raise lib.DqcAmdError(
            "bse: the tensors Bvv (nvir = %d, naux = %d, padded to %d: %.2f GB), Bvo, Bov, Boo%s need %.2f GB but only %.2f GB of device "
            "memory are free: use a smaller auxiliary basis (there is no batching over virtual blocks)"
            % (nv, naux, ldv, 8 * naux * nv * ldv / 1e9, " and the screened copies" if screened else "", need / 1e9, free / 1e9))
    bov, boo = transform_ov(b, co, cv), transform_ov(b, co, co)
    bvv, bvo = transform_ov(b, cv, cv), transform_ov(b, cv, co)
    rov = bov[:, :, :nv].permute(1, 0, 2).reshape(naux, no * nv).contiguous()
    q0 = chol = None
    mboo, mbov = boo, bov
    if screened:
        q0 = lib.rpa_response(bov, eo, ev, torch.zeros(1, dtype=b.dtype, device=b.device), 4.0)[0]
        chol = torch.linalg.cholesky(q0 + torch.eye(naux, dtype=b.dtype, device=b.device))
        # M over the auxiliary index of the smaller tensors by Cholesky solve, not by an explicit inverse (gw.correlation_part)
        solve = lambda s3: torch.cholesky_solve(s3.permute(1, 0, 2).reshape(naux, -1), chol).view(naux, s3.shape[0], s3.shape[2]).permute(1, 0, 2).contiguous()  # noqa: E731
        mboo, mbov = solve(boo), solve(bov)
    return {"df": df, "co": co, "cv": cv, "eps": torch.cat([eo, ev]), "no": no, "nv": nv, "boo": boo, "bov": bov, "bvv": bvv, "bvo": bvo,
            "mboo": mboo, "mbov": mbov, "rov": rov, "q0": q0, "chol": chol}


def _check_args(qc, spin, window, qp):
    if spin not in ("singlet", "triplet"):
        raise ValueError("bse: spin is \"singlet\" or \"triplet\", not %r" % (spin,))
    try:
        window = tuple(window)
        ok = len(window) == 2 and all(int(w) == w and int(w) >= 0 for w in window) and sum(int(w) for w in window) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("bse: window is a pair of non-negative orbital counts (occupied, virtual), not both zero, got %r" % (window,))
    if qp is not None:
        qp = torch.as_tensor(qp, dtype=torch.float64).detach()
        nmo = getattr(qc._engine, "shape", (None,))[-1]
        if qp.dim() != 1 or (nmo is not None and int(qp.numel()) != int(nmo)):
            raise ValueError("bse: qp must hold one energy per orbital (%s), got the shape %s" % ("nmo" if nmo is None else int(nmo), tuple(qp.shape)))
    if qc._engine.polarized:
        raise NotImplementedError("bse: an unrestricted calculation is not supported (restricted closed shell only; run the closed "
                                  "shell restricted)")
    return (int(window[0]), int(window[1])), qp


def bse(qc, nstates=5, spin="singlet", tda=False, screened=True, qp=None, window=(4, 4), auxbasis=None, nfreq=100, freq_scale=1.0,
        sigma_wmax=2.0, linearized=False, tol=1e-6):
    """the `nstates` lowest neutral excitations of the converged restricted HF / KS calculation `qc` from the Bethe-Salpeter equation
    with static screening on G0W0 quasiparticle energies (module docstring): a `BSE` result object.
    spin: "singlet" or "triplet"; tda: the Tamm-Dancoff approximation.  screened=False: the bare interaction (M = 1) and, unless `qp`
    is given, the SCF orbital energies: RI-TDHF / RI-CIS.  qp: all nmo quasiparticle energies, used as given (None: G0W0 for the
    `window` = (highest occupied, lowest virtual) orbital counts, clipped to what exists, and the scissor outside it).  `auxbasis` as
    `mp2` takes it (the same references, the same refusals; a Hamiltonian built with densityfit(exchange=True) uses its own tensor);
    nfreq, freq_scale, sigma_wmax, linearized go to `gw` unchanged.  tol: residual norm of the Davidson iterations; `nstates` is
    clipped to nocc nvir.  RuntimeError when a window orbital's quasiparticle equation did not converge, or when the reference is
    unstable in the channel (`response_eigs`).  The tensors, Q(0), its factor and the `gw` call are memoised on the converged state;
    nothing is differentiable: the result is detached."""
    window, qp = _check_args(qc, spin, window, qp)
    unsupported(qc)
    assert qc._has_run, "run() the calculation first"
    screened, tda = bool(screened), bool(tda)
    with torch.no_grad():
        t = memoised(qc, ("bse_tensors", aux_key(qc, auxbasis), screened), lambda: _tensors(qc, auxbasis, screened))
        no, nv, eps = t["no"], t["nv"], t["eps"]
        nmo, n, dev = no + nv, no * nv, eps.device
        g = orbs = None
        if qp is not None:
            if int(qp.numel()) != nmo:
                raise ValueError("bse: qp must hold one energy per orbital (%d), got the shape %s" % (nmo, tuple(qp.shape)))
            e_qp = qp.to(dev)
        elif not screened:
            e_qp = eps
        else:
            from .gw import gw
            orbs = window_orbitals(no, nmo, window)
            key = ("bse_gw", tuple(orbs), aux_key(qc, auxbasis), int(nfreq), float(freq_scale), float(sigma_wmax), bool(linearized))
            g = memoised(qc, key, lambda: gw(qc, orbs=orbs, auxbasis=auxbasis, nfreq=nfreq, freq_scale=freq_scale, sigma_wmax=sigma_wmax,
                                             linearized=linearized))
            for j, o in enumerate(orbs):
                if not bool(g.converged[j]):
                    raise RuntimeError("bse: the quasiparticle equation of orbital %d did not converge in gw; use linearized=True or a "
                                       "smaller window (window=%r)" % (o, window))
            e_qp = quasiparticle_ladder(eps.cpu(), no, orbs, g.qp_energies).to(dev)
        delta = (e_qp[None, no:] - e_qp[:no, None]).reshape(n).contiguous()
        c = 2.0 if spin == "singlet" else 0.0
        rov, work = t["rov"], [torch.empty(0, dtype=eps.dtype, device=dev)]

        def fused(l, r, x, nr, ns):   # one work buffer for every product, grown to what the largest block of vectors asks for
            need = int(lib.load().dqc_bse_work_doubles(int(l.shape[0]), int(r.shape[0]), nr, ns, int(l.shape[1]), int(x.shape[0])))
            if work[0].numel() < need:
                work[0] = torch.empty(need, dtype=x.dtype, device=x.device)
            return lib.bse_exchange(l, r, x, nr, ns, work=work[0])

        def direct(x):      # (nvec, no, nv) -> Wd x
            return fused(t["mboo"], t["bvv"], x, no, nv).reshape(-1, n)

        def exchange(x):    # (nvec, no, nv) -> Wx x
            return fused(t["mbov"], t["bvo"], x.transpose(1, 2).contiguous(), nv, no).reshape(-1, n)

        def coulomb(v):     # (nvec, n) -> v x
            return torch.matmul(torch.matmul(v, rov.t()), rov)

        nst = min(int(nstates), n)
        if tda:
            def op(v):
                v = v.contiguous()
                out = delta[None, :] * v - direct(v.view(-1, no, nv))
                return out + c * coulomb(v) if c else out
            w, xpy, res = davidson_lowest(op, delta, neig=nst, tol=tol)
            xmy = None
        else:
            def pair(v):
                v = v.contiguous()
                x = v.view(-1, no, nv)
                d, wd, wx = delta[None, :] * v, direct(x), exchange(x)
                plus = d - wd - wx
                return (plus + 2.0 * c * coulomb(v) if c else plus), d - wd + wx
            w, xpy, xmy, res = response_eigs(pair, delta, neig=nst, tol=tol)
        if spin == "triplet":
            mu = torch.zeros((int(w.numel()), 3), dtype=w.dtype, device=dev)
        else:
            h = qc.get_system().get_hamiltonian()
            r = torch.matmul(torch.matmul(t["co"].t(), lib.int1e("r0", h._tab, h.device)), t["cv"]).reshape(3, n)   # r_ia
            mu = 2.0 ** 0.5 * (xpy @ r.t())
        f = (2.0 / 3.0) * w * (mu * mu).sum(1)
        host = lambda x: None if x is None else x.detach().cpu()  # noqa: E731
        return BSE(host(w), host(mu), host(f), host(xpy), host(xmy), spin, tda, res, host(e_qp), orbs, g, screened, t["df"])


# `dqc_amd.bse` is this function once the package has imported it: the yardsticks stay reachable as dqc_amd.bse.exchange_reference ...
bse.exchange_reference = exchange_reference
bse.static_w_reference = static_w_reference
bse.bse_reference = bse_reference
bse.bse_matrices = bse_matrices
bse.solve_dense = solve_dense
bse.quasiparticle_ladder = quasiparticle_ladder

__all__ = ["bse", "BSE", "exchange_reference", "static_w_reference", "bse_reference", "bse_matrices", "solve_dense", "quasiparticle_ladder", "window_orbitals"]
