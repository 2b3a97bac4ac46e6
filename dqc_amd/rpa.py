"""Direct random-phase-approximation correlation energy with density-fitted integrals (RI-dRPA) on a converged HF or KS calculation:
EXX + dRPA, e.g. RPA@PBE.

    D_ia = eps_a - eps_i > 0,   g_ia(w) = D_ia / (D_ia^2 + w^2)                                            per spin
    Q(w)[P, R] = s sum_spin sum_ia Bov[i, P, a] g_ia(w) Bov[i, R, a]       s = 4 restricted, 2 per spin unrestricted
    e_corr     = 1 / (2 pi) int_0^inf dw { ln det(1 + Q(w)) - tr Q(w) }
    e_corr_2nd = 1 / (2 pi) int_0^inf dw { -1/2 tr Q(w)^2 }                 (the second-order term: direct MP2)

Q is symmetric positive semidefinite: ln det(1 + Q) - tr Q = sum_n [log1p(l_n) - l_n] over its eigenvalues (`energy_from_response`).
By int_0^inf g_ia g_jb dw = pi / (2 (D_ia + D_jb)) the second-order term is known in closed form from the opposite-spin-type pair sums of the MP2 kernel,

    e_dmp2 = 2 sum_ij pair_os                              restricted
           = 1/2 (os_aa + os_bb) + os_ab                   unrestricted (os_ss: the full (i, j) sum of the same=True e_os matrix)

so quadrature_error = |e_corr_2nd - e_dmp2| is a per-call estimate of the error of the frequency quadrature, at no cost.
Quadrature: Gauss-Legendre x_k, w_k on (-1, 1) mapped to w = w0 (1 + x) / (1 - x), weight 2 w0 w_k / (1 - x)^2 (`frequency_grid`).

Steps: the tensor B and Bov[i, P, a] as dqc_amd/mp2.py makes them; Q on the whole grid by the fused kernel dqc_rpa_response
(csrc/rpa.hip, O(o v naux^2 nfreq): no frequency-scaled copy of Bov is stored, only the lower triangle is computed), once per spin;
batched eigenvalues of Q, the second-order trace as multiply-and-reduce.  `Bov` must fit in device memory; Q is formed in frequency
batches when nfreq naux^2 doubles do not.  Energies only: no gradient and no autograd, the result is detached.  dRPA is not self-correlation free (the
correlation energy of a one-electron system is not zero) and, without exchange in the kernel, overbinds short-range correlation:
total correlation energies are too negative, energy differences are what the method is used for.

`response_reference`, `frequency_grid`, `energy_from_response` and `plasmon_reference` are the yardsticks: plain torch on any device.
`plasmon_reference` is the closed form: with K[ia, jb] = sum_P Bov[i, P, a] Bov[j, P, b] over spin orbitals (all spin blocks),

    M = D^1/2 (D + 2 K) D^1/2,   W = sqrt(eig M),   e_corr = 1/2 (sum W - sum D - tr K)

(restricted, singlet block alone: D + 4 K_spatial and 1/2 (sum W - sum D - 2 tr K_spatial)) -- O((o v)^3), for small ov spaces."""
import math

import torch

from .postscf import (aux_key, b_tensor, check_frequency_args, memoised, orbitals, pair_energy_blocks, response_batches, transform_ov,
                      unsupported)


def frequency_grid(nfreq, scale=1.0):
    """(freqs, weights), float64 on the host: the nfreq Gauss-Legendre points x_k of (-1, 1) mapped to w = scale (1 + x) / (1 - x) on
    (0, inf), ascending, with the weights 2 scale w_k / (1 - x)^2"""
    import numpy as np
    nfreq = int(nfreq)
    check_frequency_args("frequency_grid", nfreq, float(scale), "the scale")
    x, w = np.polynomial.legendre.leggauss(nfreq)
    x, w = torch.from_numpy(x), torch.from_numpy(w)
    return float(scale) * (1.0 + x) / (1.0 - x), 2.0 * float(scale) * w / (1.0 - x) ** 2


def response_reference(bov, eo, ev, freq, scale=1.0):
    """Q (nfreq, naux, naux) of the module docstring in plain torch, on the device of the inputs: the yardstick of dqc_rpa_response.
    bov (no, naux, >= nv): columns past the number of virtual energies (padding) are ignored.  One occupied orbital at a time."""
    nv = int(ev.numel())
    naux = int(bov.shape[1])
    freq = freq.to(device=bov.device, dtype=bov.dtype)
    q = torch.zeros((int(freq.numel()), naux, naux), dtype=bov.dtype, device=bov.device)
    for i in range(int(bov.shape[0])):
        d = ev - eo[i]
        g = d[None, :] / (d[None, :] ** 2 + freq[:, None] ** 2)        # (nfreq, nv)
        b = bov[i, :, :nv]
        q += torch.matmul(b[None] * g[:, None, :], b.t())
    return scale * q


def energy_from_response(q, weights):
    """(e_corr, e_corr_2nd, integrand) from Q (nfreq, naux, naux) and the quadrature weights: one-element tensors and the nfreq values
    ln det(1 + Q_k) - tr Q_k, on the device of q.  The integrand is sum_n [log1p(l_n) - l_n] over the eigenvalues l_n of Q_k (batched
    torch.linalg.eigvalsh), not 2 sum log diag of a Cholesky factor of 1 + Q minus the trace: forming 1 + Q rounds every diagonal
    element to 1e-16 ABSOLUTE however small Q is, and the weights of the highest frequencies, where Q vanishes, reach 4e3 -- measured
    1e-12 Ha of noise at naux 101 against 4e-16 Ha this way (an error dl of an eigenvalue enters only as l dl / (1 + l)).  The
    second-order term by multiply-and-reduce"""
    w = weights.to(device=q.device, dtype=q.dtype)
    lam = torch.linalg.eigvalsh(q)
    integrand = (torch.log1p(lam) - lam).sum(-1)
    second = -0.5 * (q * q.transpose(-2, -1)).sum((-2, -1))
    return ((w * integrand).sum() / (2.0 * math.pi)).reshape(1), ((w * second).sum() / (2.0 * math.pi)).reshape(1), integrand


def plasmon_reference(spins, frozen=0, digits=None):
    """e_corr (a one-element tensor) in closed form (module docstring): `spins` as mp2.energies_reference takes it -- one (restricted)
    or two (unrestricted: alpha, beta) tuples (bov (nocc, naux, >= nvir), eps_occ, eps_vir), or, in place of bov, the dense
    (nocc, nvir, nocc, nvir) integrals (ia|jb) of a restricted calculation; the lowest `frozen` occupied orbitals are dropped.
    In fp64 the form is a difference of sums of order sum D (200 Ha for ten electrons with a core orbital): good to about 1e-14 Ha.
    digits=n: the same form from the same fp64 inputs in n-digit arithmetic (mpmath, on the host; seconds for ov = 40)"""
    if len(spins) == 1 and spins[0][0].dim() == 4:
        v, eo, ev = spins[0]
        v, eo = v[frozen:, :, frozen:], eo[frozen:]
        d = (ev[None, :] - eo[:, None]).reshape(-1)
        k = v.reshape(d.numel(), d.numel())
        r = None
        fac = 4.0
    else:
        rows, ds = [], []
        for b, eo, ev in spins:
            nv = int(ev.numel())
            b, eo = b[frozen:, :, :nv], eo[frozen:]
            rows.append(b.permute(0, 2, 1).reshape(-1, b.shape[1]))   # [(i, a), P]
            ds.append((ev[None, :] - eo[:, None]).reshape(-1))
        r, d = torch.cat(rows), torch.cat(ds)
        k = r @ r.t()
        fac = 4.0 if len(spins) == 1 else 2.0
    if d.numel() == 0:
        return torch.zeros(1, dtype=d.dtype, device=d.device)
    if digits is not None:
        return torch.tensor([_plasmon_mp(d, k, r, fac, int(digits))], dtype=d.dtype, device=d.device)
    s = d.sqrt()
    m = s[:, None] * (torch.diag(d) + fac * k) * s[None, :]
    om = torch.linalg.eigvalsh(0.5 * (m + m.t())).sqrt()
    return (0.5 * (om.sum() - d.sum() - 0.5 * fac * k.diagonal().sum())).reshape(1)


def _plasmon_mp(d, k, r, fac, digits):
    """the closed form in `digits`-digit arithmetic; K from the factor r when there is one (its fp64 product is itself rounded)"""
    import mpmath as mp
    with mp.workdps(digits):
        n = int(d.numel())
        dd = [mp.mpf(float(x)) for x in d.cpu()]
        if r is not None:
            rm = mp.matrix(r.cpu().tolist())
            km = rm * rm.T
        else:
            km = mp.matrix(k.cpu().tolist())
        sq = [mp.sqrt(x) for x in dd]
        m = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                m[i, j] = sq[i] * ((dd[i] if i == j else 0) + fac * km[i, j]) * sq[j]
        om = mp.eigsy(m, eigvals_only=True)
        e = (sum(mp.sqrt(x) for x in om) - sum(dd) - fac / 2 * sum(km[i, i] for i in range(n))) / 2
        return float(e)


def dmp2_from_pairs(os_same, os_ab=None):
    """the second-order (direct MP2) energy from opposite-spin-type pair sums: restricted 2 sum pair_os; unrestricted
    1/2 (os_aa + os_bb) + os_ab, os_same = (os_aa, os_bb) the same=True e_os matrices of the two spins"""
    if os_ab is None:
        return (2.0 * os_same.sum()).reshape(1)
    return (0.5 * (os_same[0].sum() + os_same[1].sum()) + os_ab.sum()).reshape(1)


class RPA:
    """what `rpa` returns (one-element detached tensors): `e_corr` (dRPA correlation energy), `e_corr_2nd` (its second-order term by
    the same quadrature), `e_dmp2` (that term in closed form), `quadrature_error` = |e_corr_2nd - e_dmp2| (a float), `e_exx` (the
    SCF energy expression with 100 % exact exchange and no exchange-correlation functional on the converged density; qc.energy() for
    Hartree-Fock; None where the Hamiltonian cannot form K: a J-only fit), `e_tot = e_exx + e_corr` (None likewise); `freqs`,
    `weights`, `integrand` (nfreq values each: ln det(1 + Q) - tr Q); `frozen`, `naux`, `nfreq`; `df`: the DFMI355 object whose
    tensor was used"""

    def __init__(self, e_corr, e_corr_2nd, e_dmp2, e_exx, freqs, weights, integrand, frozen, df):
        self.e_corr, self.e_corr_2nd, self.e_dmp2, self.e_exx = e_corr, e_corr_2nd, e_dmp2, e_exx
        self.quadrature_error = abs(float(e_corr_2nd) - float(e_dmp2))
        self.e_tot = None if e_exx is None else e_exx + e_corr
        self.freqs, self.weights, self.integrand = freqs, weights, integrand
        self.frozen, self.df, self.nfreq = int(frozen), df, int(freqs.numel())
        self.naux = int(df._b.shape[0])

    def __repr__(self):
        return "RPA(e_corr=%.10f, e_dmp2=%.10f, quadrature_error=%.1e, e_exx=%s, e_tot=%s, frozen=%d, naux=%d, nfreq=%d)" % (
            float(self.e_corr), float(self.e_dmp2), self.quadrature_error, "None" if self.e_exx is None else "%.10f" % float(self.e_exx),
            "None" if self.e_tot is None else "%.10f" % float(self.e_tot), self.frozen, self.naux, self.nfreq)


def _e_exx(qc):
    """the Hartree-Fock energy expression on the converged density (None: a J-only fit has no K)"""
    eng = qc._engine
    h = eng.hamilton
    if h.df is not None and not h.df.exchange:
        return None
    from .utils.datastruct import SpinParam
    dm = qc.aodm()
    tot = SpinParam.sum(dm)
    e = h.get_e_hcore(tot) + h.get_e_elrep(tot) + h.get_e_exchange(dm) + eng._enuc
    return e.detach().reshape(1)


def _compute(qc, frozen, auxbasis, nfreq, freq_scale, batch=None):
    eng = qc._engine
    df = b_tensor(qc, auxbasis)
    b = df._b
    spins = orbitals(qc, frozen)
    bovs = [transform_ov(b, co, cv) for co, cv, _, _ in spins]
    freqs, weights = frequency_grid(nfreq, freq_scale)
    fd, wd = freqs.to(b.device), weights.to(b.device)
    # Q, the copy the eigenvalue solver works in and its workspace: three (nk, naux, naux) tensors per batch
    batches = response_batches(bovs, spins, fd, 2.0 if eng.polarized else 4.0, 3, batch)
    e_corr = torch.zeros(1, dtype=b.dtype, device=b.device)
    e_2nd = torch.zeros_like(e_corr)
    integrand = torch.empty(nfreq, dtype=b.dtype, device=b.device)
    for k0, n, qk in batches:
        e1, e2, integrand[k0:k0 + n] = energy_from_response(qk, wd[k0:k0 + n])
        e_corr += e1
        e_2nd += e2
    os_ab, same = pair_energy_blocks(bovs, spins)
    if not eng.polarized:
        e_dmp2 = dmp2_from_pairs(same[0][0])
    else:
        e_dmp2 = dmp2_from_pairs(tuple(os for os, _ in same), os_ab)
    return df, e_corr, e_2nd, e_dmp2, freqs, weights, integrand


def rpa(qc, frozen=0, auxbasis=None, nfreq=48, freq_scale=1.0):
    """RI-dRPA correlation energy of the converged HF / KS calculation `qc` (module docstring): an `RPA` result object.
    `frozen` and `auxbasis` as `mp2` takes them (the same references, the same refusals; a Hamiltonian built with
    densityfit(exchange=True) uses its own tensor).  nfreq, freq_scale: points and scale w0 of the frequency quadrature; the defaults
    keep `quadrature_error` below 1e-8 Ha on gaps from 0.06 to 25 Ha -- read it off the result: a smaller gap wants more points.
    Memoised on the converged state per argument set; nothing is differentiable: the result is detached."""
    frozen, nfreq, freq_scale = int(frozen), int(nfreq), float(freq_scale)
    if frozen < 0:
        raise ValueError("rpa: frozen must be >= 0, got %d" % frozen)
    check_frequency_args("rpa", nfreq, freq_scale)
    unsupported(qc)
    assert qc._has_run, "run() the calculation first"
    df, e_corr, e_2nd, e_dmp2, freqs, weights, integrand, e_exx = memoised(
        qc, ("rpa", frozen, aux_key(qc, auxbasis), nfreq, freq_scale),
        lambda: _compute(qc, frozen, auxbasis, nfreq, freq_scale) + (_e_exx(qc),))
    return RPA(e_corr, e_2nd, e_dmp2, e_exx, freqs, weights, integrand, frozen, df)


# `dqc_amd.rpa` is this function once the package has imported it: the yardsticks stay reachable as dqc_amd.rpa.response_reference ...
rpa.response_reference = response_reference
rpa.frequency_grid = frequency_grid
rpa.energy_from_response = energy_from_response
rpa.plasmon_reference = plasmon_reference

__all__ = ["rpa", "RPA", "response_reference", "frequency_grid", "energy_from_response", "plasmon_reference", "dmp2_from_pairs"]
