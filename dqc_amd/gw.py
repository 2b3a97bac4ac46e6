"""G0W0 quasiparticle energies by analytic continuation (AC-G0W0) with density-fitted integrals on a converged HF or KS calculation:
ionisation potentials, electron affinities and the fundamental gap, e.g. G0W0@PBE.

    Q(iw)   the dRPA response matrix of dqc_amd/rpa.py (lib.rpa_response, both spins accumulated)
    Wc(iw)  = (1 + Q)^-1 - 1 = -(1 + Q)^-1 Q                              the correlation part of the screened interaction, auxiliary basis
    W[k, n, m] = sum_PR Bn[n, P, m] Wc(iw_k)[P, R] Bn[n, R, m]            (n m| Wc |m n), per spin                          (csrc/gw.hip)
    Sc_n(iw) = -1 / pi sum_k wt_k sum_m W[k, n, m] z_m / (z_m^2 + w_k^2),      z_m = ef + iw - eps_m
    E_n = F_HF,nn + Re Sc_n(E_n - ef),      F_HF,nn = <n| h + J[D] - K[D] |n> = eps_n - vxc_nn + Sx_nn

Sc_n(iw) = -1 / (2 pi) int dw' sum_m G0_m(iw + iw') W_nm(iw') with G0_m(iw) = 1 / (iw + ef - eps_m); W is even in w', which folds the
integral to (0, inf): the nodes are those of `rpa.frequency_grid`, on which Q is formed.  The kernel z / (z^2 + w'^2) peaks at w' = w
with the width |eps_m - ef|, which the nodes do not resolve once that is below their spacing (a 0.05 Ha gap: 10 % off above 0.1 Ha),
so the sum above is not taken as it stands: W, the smooth factor, is interpolated through the nodes and its product with the kernel --
a simple pole in the grid's variable -- is integrated exactly (`self_energy_reference(..., scale=)`, Legendre functions of the second
kind), which is as accurate as the grid is for Q itself (docs/LOG_r24.md).  ef is the midpoint of the highest occupied and the lowest
virtual orbital energy over both spins.  Sc is evaluated at iw = 0 and at i times the quadrature nodes below `sigma_wmax`, continued to
the real axis by a Thiele continued-fraction Pade approximant through all points (`pade_thiele`), and the quasiparticle equation is
solved by Newton's method from eps_n (or linearised: E_n = eps_n + Z_n (F_HF,nn - eps_n + Re Sc_n(eps_n - ef)),
Z_n = 1 / (1 - d Re Sc_n / dE)).

CONTINUATION FROM THE IMAGINARY AXIS IS RELIABLE NEAR THE FERMI LEVEL ONLY: for the frontier orbitals, whose quasiparticle energy lies
in or next to the gap where Sc has no poles, the Pade error is of the order of 1e-10 Ha; a few orbitals further out it is 1e-3 Ha, and
for core states the method is not usable at all (their self-energy has poles between the state and the Fermi level; that needs contour
deformation, which is not here).

The static part is the Hartree-Fock Fock expectation value on the converged density from the Hamiltonian's own operators, so no
separate v_xc matrix is needed, hybrids are right as they stand and F_HF,nn = eps_n for Hartree-Fock.  A J-only fit cannot form K:
there Sx_nn = -sum_i sum_P Bn[n, P, i]^2 comes from the tensor.

Cost: the screened-interaction diagonal is the one O(nfreq ntarget nmo naux^2) step -- the fused kernel dqc_gw_screened_diag keeps
Y = Wc Bn in accumulators and reads the lower triangle of Wc only.  `Bn` (ntarget, naux, nmo) per spin and Bov must fit in device memory;
Q and Wc are formed in frequency batches when nfreq naux^2 doubles do not.  No gradient and no autograd: the result is detached.

`screened_diag_reference`, `self_energy_reference`, `pade_thiele` and `spectral_reference` are the yardsticks: plain torch on any
device.  `spectral_reference` is the closed form: with K and D as in `rpa.plasmon_reference`, M = D^1/2 (D + fac K) D^1/2 = Z Om^2 Z^T
(fac = 4: restricted singlet block, 2: spin orbitals), (X + Y)^s = D^1/2 Z_s / sqrt(Om_s), w^s_nm = c sum_jb (n m|j b) (X + Y)^s_jb
(c = sqrt 2 restricted, 1 spin orbitals),

    Sc_n(z) = sum_s [ sum_i^occ (w^s_ni)^2 / (z - eps_i + Om_s) + sum_a^vir (w^s_na)^2 / (z - eps_a - Om_s) ]
    W[k, n, m] = -sum_s (w^s_nm)^2 2 Om_s / (Om_s^2 + w_k^2)

-- O((o v)^3), for small ov spaces."""
import math

import torch

from . import lib
from .postscf import aux_key, b_tensor, check_frequency_args, memoised, orbitals, response_batches, transform_ov, unsupported
from .rpa import frequency_grid


def screened_diag_reference(wc, bn, nm):
    """W (nfreq, ntarget, nm) of the module docstring in plain torch, on the device of the inputs: the yardstick of
    dqc_gw_screened_diag.  wc (nfreq, naux, naux) is taken as it is (both triangles); bn (ntarget, naux, >= nm): columns past nm
    (padding) are ignored.  One target orbital at a time"""
    nm = int(nm)
    w = torch.zeros((int(wc.shape[0]), int(bn.shape[0]), nm), dtype=bn.dtype, device=bn.device)
    for n in range(int(bn.shape[0])):
        b = bn[n, :, :nm]
        w[:, n] = (b[None] * torch.matmul(wc, b)).sum(1)
    return w


def _legendre_pole_sums(x, y):
    """S[k, p] = sum_{l < n} (2 l + 1) P_l(x_k) Q_l(y_p) for the n Gauss-Legendre nodes x (real) and poles y (complex, off [-1, 1]):
    int_-1^1 f(x) / (y - x) dx = sum_k w_k f(x_k) S[k, p] exactly for polynomials f of degree < n (Neumann: int P_l / (y - x) = 2 Q_l;
    Heine: the full sum is 1 / (y - x_k), which is what the plain Gauss rule uses).  Q_l, the minimal solution of Legendre's recurrence,
    falls off as rho^-l with rho = |y + sqrt(y^2 - 1)| >= 1: forward recurrence from Q_0 = 1/2 ln((y + 1) / (y - 1)), Q_1 = y Q_0 - 1
    while rho^n < 10 (it loses rho^2n), Miller's backward recurrence from l = n + 40 / ln rho otherwise, and where rho^n > 1e9 the plain
    value 1 / (y - x_k): the Gauss rule is exact to round-off there (its error is of the order rho^-2n)"""
    n = int(x.numel())
    s = 1.0 / (y[None, :] - x[:, None])
    t = y + torch.sqrt(y * y - 1.0)
    lr = t.abs().log().abs()                              # ln rho
    near = n * lr <= math.log(1e9)
    if not bool(near.any()):
        return s
    yn, lrn = y[near], lr[near]
    fwd = n * lrn < math.log(10.0)
    q = torch.empty((n, int(yn.numel())), dtype=y.dtype, device=y.device)
    # forward
    qf = torch.empty_like(q)
    qf[0] = 0.5 * torch.log((yn + 1.0) / (yn - 1.0))
    if n > 1:
        qf[1] = yn * qf[0] - 1.0
    for l in range(1, n - 1):
        qf[l + 1] = ((2 * l + 1) * yn * qf[l] - l * qf[l - 1]) / (l + 1)
    # backward: every pole from its own start (seeded there; zero above it), normalised by Q_0
    start = (n + torch.ceil(40.0 / lrn.clamp_min(math.log(10.0) / n))).to(torch.int64)
    hi, cur = torch.zeros_like(yn), torch.zeros_like(yn)  # r_{l + 1}, r_l
    for l in range(int(start.max()), 0, -1):
        cur = torch.where(start == l, torch.full_like(cur, 1e-30), cur)
        if l < n:
            q[l] = cur
        hi, cur = cur, ((2 * l + 1) * yn * cur - (l + 1) * hi) / l
    q[0] = cur
    q = q * (qf[0] / cur)[None, :]
    q = torch.where(fwd[None, :], qf, q)
    ls = torch.arange(n, dtype=x.dtype, device=x.device)
    p = torch.empty((n, n), dtype=x.dtype, device=x.device)     # P_l(x_k)
    p[0] = 1.0
    if n > 1:
        p[1] = x
    for l in range(1, n - 1):
        p[l + 1] = ((2 * l + 1) * x * p[l] - l * p[l - 1]) / (l + 1)
    s[:, near] = ((2.0 * ls + 1.0)[:, None] * p).t().to(y.dtype) @ q
    return s


def self_energy_reference(w, eps, ef, freqs, weights, points, scale=None):
    """Sc_n(i points_j), complex (ntarget, npoints), from W (nfreq, ntarget, nmo) on the quadrature (freqs, weights), the orbital
    energies eps (nmo) and the Fermi level ef (module docstring); on the device of w.
    scale=None: the quadrature as it stands, sum_k wt_k W_k z / (z^2 + w_k^2).  Its kernel 1/2 [1 / (z + i w') + 1 / (z - i w')] has
    poles at the distance |eps_m - ef| from the axis of integration, which the nodes resolve only while that is more than their spacing
    (at a gap of 0.05 Ha the result is 10 % off above 0.1 Ha).
    scale=s: the nodes are those of `rpa.frequency_grid(nfreq, s)`, and the smooth factor W alone is interpolated through them
    (a polynomial in x = (w' - s) / (w' + s) times the Jacobian, the function class the grid integrates to round-off); its product with
    the kernel, a simple pole in x, is integrated exactly (`_legendre_pole_sums`).  Far poles: the same numbers as the plain rule."""
    cd = torch.complex128
    eps, freqs, weights, points = (torch.as_tensor(t, dtype=w.dtype).to(w.device) for t in (eps, freqs, weights, points))
    z = (float(ef) - eps)[None, :].to(cd) + 1j * points[:, None].to(cd)                               # (npoints, nmo)
    if scale is None:
        f = weights[None, :, None] * z[:, None, :] / (z[:, None, :] ** 2 + (freqs ** 2)[None, :, None])   # (npoints, nfreq, nmo)
    else:
        # 1 / (z -+ i w') dw' = (1 - x) / (A - B x) (2 s / (1 - x)^2) dx,  (A, B) = (z -+ i s, z +- i s):
        # (1 - x) / (A - B x) = 1 / B [1 + (B - A) / B * 1 / (A / B - x)]
        s = float(scale)
        x = (freqs - s) / (freqs + s)
        f = torch.zeros((int(points.numel()), int(freqs.numel()), int(eps.numel())), dtype=cd, device=w.device)
        for sign in (-1.0, 1.0):
            a, b = z + sign * 1j * s, z - sign * 1j * s
            sums = _legendre_pole_sums(x, (a / b).reshape(-1)).reshape(int(freqs.numel()), *z.shape).permute(1, 0, 2)
            f += 0.5 * weights[None, :, None] * (1.0 + ((b - a) / b)[:, None, :] * sums) / b[:, None, :]
    nfreq, ntarget, nmo = (int(x) for x in w.shape)
    wn = w.permute(1, 0, 2).reshape(ntarget, nfreq * nmo)
    ft = f.reshape(-1, nfreq * nmo).t()
    return torch.complex(wn @ ft.real.contiguous(), wn @ ft.imag.contiguous()) * (-1.0 / math.pi)


class Pade:
    """what `pade_thiele` returns: the approximant through (z_p, f_p), P(x) = a_1 / (1 + a_2 (x - z_1) / (1 + a_3 (x - z_2) / ...)).
    `p(x)` and `p(x, derivative=True)` -> (P, dP/dx): x complex, a scalar or of the shape of the batch plus one trailing dimension"""

    def __init__(self, z, a):
        self.z, self.a = z, a

    def __call__(self, x, derivative=False):
        a, z = self.a, self.z
        x = torch.as_tensor(x).to(dtype=a.dtype, device=a.device)
        scalar = x.dim() == 0
        if scalar:
            x = x.reshape((1,) * a.dim())
        shape = a.shape[:-1] + x.shape[-1:]
        big, dbig = torch.ones(shape, dtype=a.dtype, device=a.device), torch.zeros(shape, dtype=a.dtype, device=a.device)
        for p in range(int(a.shape[-1]) - 1, 0, -1):
            ap = a[..., p:p + 1]
            t = ap * (x - z[p - 1])
            big, dbig = 1.0 + t / big, ap / big - t * dbig / (big * big)
        val, der = a[..., 0:1] / big, -a[..., 0:1] * dbig / (big * big)
        if scalar:
            val, der = val[..., 0], der[..., 0]
        return (val, der) if derivative else val


def pade_thiele(z, f):
    """the Thiele continued-fraction Pade approximant through the points (z_p, f[..., p]) (Vidberg and Serene 1977): z (n) complex,
    distinct; f (..., n) complex, one function per leading index -> `Pade`.  n points determine a rational function of degrees
    (n / 2 - 1, n / 2) (n even) exactly; complex128 throughout"""
    z = torch.as_tensor(z).to(torch.complex128)
    g = torch.as_tensor(f).to(dtype=torch.complex128, device=z.device).clone()
    n = int(z.numel())
    if g.shape[-1] != n or n < 1:
        raise ValueError("pade_thiele: %d points for values of shape %s" % (n, tuple(g.shape)))
    a = torch.empty_like(g)
    a[..., 0] = g[..., 0]
    for p in range(1, n):
        prev = a[..., p - 1:p]
        g[..., p:] = (prev - g[..., p:]) / ((z[p:] - z[p - 1]) * g[..., p:])
        a[..., p] = g[..., p]
    return Pade(z, a)


def quasiparticle_solve(pade, eps, f_hf, ef, linearized=False, tol=1e-11, maxiter=60):
    """(E, Z, converged) per orbital: the solution of E = f_hf + Re Sc(E - ef) by Newton's method from eps, Sc = `pade` (one function
    per orbital); Z = 1 / (1 - d Re Sc / dE) at eps; linearized=True: E = eps + Z (f_hf - eps + Re Sc(eps - ef)), converged all True"""
    eps = torch.as_tensor(eps, dtype=torch.float64).cpu()
    f_hf = torch.as_tensor(f_hf, dtype=torch.float64).cpu()
    s, ds = pade((eps - ef)[:, None], derivative=True)
    zfac = 1.0 / (1.0 - ds[:, 0].real)
    if linearized:
        return eps + zfac * (f_hf - eps + s[:, 0].real), zfac, torch.ones_like(eps, dtype=torch.bool)
    e = eps.clone()
    done = torch.zeros_like(eps, dtype=torch.bool)
    for _ in range(int(maxiter)):
        s, ds = pade((e - ef)[:, None], derivative=True)
        step = (e - f_hf - s[:, 0].real) / (1.0 - ds[:, 0].real)
        step = torch.where(done | ~torch.isfinite(step), torch.zeros_like(step), step)
        e = e - step
        done = done | (step.abs() <= tol)
        if bool(done.all()):
            break
    resid = e - f_hf - pade((e - ef)[:, None])[:, 0].real
    return e, zfac, done & (resid.abs() <= 100.0 * tol)


class SpectralSigma:
    """what `spectral_reference` returns: `omega` (nexc) the dRPA excitation energies, per spin `w[s]` (nexc, ntarget, nmo) the
    couplings w^s_nm, `eps[s]` (nmo), `nocc[s]`; `sigma_c(s, z)`: Sc_n at the complex ENERGIES z (measured from zero, not from ef)
    -> (ntarget, len(z)), with derivative=True also dSc/dz; `screened(s, freqs)`: W[k, n, m] at the imaginary frequencies"""

    def __init__(self, omega, w, eps, nocc):
        self.omega, self.w, self.eps, self.nocc = omega, w, eps, nocc

    def sigma_c(self, s, z, derivative=False):
        cd = torch.complex128
        z = torch.as_tensor(z).to(dtype=cd, device=self.omega.device).reshape(-1)
        eps, no = self.eps[s], self.nocc[s]
        sign = torch.ones_like(eps)
        sign[no:] = -1.0
        # poles at eps_i - Om_s (occupied) and eps_a + Om_s (virtual)
        pole = eps[None, :] - sign[None, :] * self.omega[:, None]                          # (nexc, nmo)
        den = z[:, None, None] - pole[None].to(cd)                                         # (npts, nexc, nmo)
        w2 = (self.w[s] ** 2).to(cd)                                                       # (nexc, ntarget, nmo)
        val = torch.einsum("snm,jsm->nj", w2, 1.0 / den)
        if derivative:
            return val, -torch.einsum("snm,jsm->nj", w2, 1.0 / (den * den))
        return val

    def screened(self, s, freqs):
        f = torch.as_tensor(freqs, dtype=self.omega.dtype).to(self.omega.device)
        k = 2.0 * self.omega[None, :] / (self.omega[None, :] ** 2 + f[:, None] ** 2)      # (nfreq, nexc)
        return -torch.einsum("ks,snm->knm", k, self.w[s] ** 2)


def spectral_reference(spins):
    """the closed form of the module docstring: `spins` holds one (restricted) or two (unrestricted: alpha, beta) tuples
    (bnm (ntarget, naux, >= nmo), bov (nocc, naux, >= nvir), eps (nmo)) -- the target slabs over ALL orbitals, the occupied-virtual
    tensor and all orbital energies of the spin, nvir = nmo - nocc -> `SpectralSigma`"""
    rows, ds = [], []
    for _, bov, eps in spins:
        no = int(bov.shape[0])
        nv = int(eps.numel()) - no
        rows.append(bov[:, :, :nv].permute(0, 2, 1).reshape(no * nv, -1))   # [(i, a), P]
        ds.append((eps[None, no:] - eps[:no, None]).reshape(-1))
    r, d = torch.cat(rows), torch.cat(ds)
    restricted = len(spins) == 1
    fac, c = (4.0, math.sqrt(2.0)) if restricted else (2.0, 1.0)
    sq = d.sqrt()
    m = sq[:, None] * (torch.diag(d) + fac * (r @ r.t())) * sq[None, :]
    om2, zv = torch.linalg.eigh(0.5 * (m + m.t()))
    omega = om2.sqrt()
    xpy = sq[:, None] * zv / omega.sqrt()[None, :]                          # [(j, b), s]
    ws = []
    for bnm, _, eps in spins:
        nmo = int(eps.numel())
        t = torch.einsum("npm,xp->nmx", bnm[:, :, :nmo], r)                 # (n m|j b)
        ws.append((c * torch.matmul(t, xpy)).permute(2, 0, 1).contiguous())
    return SpectralSigma(omega, ws, [eps for _, _, eps in spins], [int(bov.shape[0]) for _, bov, _ in spins])


class GW:
    """what `gw` returns (detached tensors on the host).  Restricted: `qp_energies`, `mo_energies`, `sigma_x`, `vxc`, `z`, `converged`
    (ntarget each; vxc = eps - <n|h + J|n>, the generalised Kohn-Sham potential including any exact-exchange fraction; z the
    renormalisation factor at eps_n), `sigma_c_iw` (complex, ntarget x npoints: Sc_n at i `sigma_points`); unrestricted: each of them
    a pair (alpha, beta), wherever `mp2` returns pairs.  `orbs` (the target orbitals, indices into the orbitals in energy order),
    `sigma_points` (0 and the quadrature nodes below sigma_wmax), `ef`; `homo`, `lumo`, `gap` (floats: the quasiparticle energy of
    the highest occupied and the lowest virtual target orbital over both spins and their difference; None when `orbs` holds no
    occupied or no virtual orbital); `freqs`, `weights`, `naux`, `nfreq`, `linearized`; `df`: the DFMI355 object whose tensor was used"""

    def __init__(self, per_spin, orbs, nocc, points, ef, freqs, weights, linearized, df):
        pick = (lambda key: per_spin[0][key]) if len(per_spin) == 1 else (lambda key: tuple(p[key] for p in per_spin))
        self.qp_energies, self.mo_energies, self.sigma_x, self.vxc = pick("qp"), pick("eps"), pick("sigma_x"), pick("vxc")
        self.sigma_c_iw, self.z, self.converged = pick("sigma_c_iw"), pick("z"), pick("converged")
        self.orbs, self.sigma_points, self.ef = list(orbs), points, float(ef)
        self.freqs, self.weights, self.linearized, self.df = freqs, weights, bool(linearized), df
        self.nfreq, self.naux = int(freqs.numel()), int(df._b.shape[0])
        occ = [float(p["qp"][j]) for p, no in zip(per_spin, nocc) for j, o in enumerate(orbs) if o < no]
        vir = [float(p["qp"][j]) for p, no in zip(per_spin, nocc) for j, o in enumerate(orbs) if o >= no]
        self.homo, self.lumo = (max(occ) if occ else None), (min(vir) if vir else None)
        self.gap = None if self.homo is None or self.lumo is None else self.lumo - self.homo

    def __repr__(self):
        f = lambda x: "None" if x is None else "%.8f" % x  # noqa: E731
        return "GW(homo=%s, lumo=%s, gap=%s, ef=%.6f, targets=%d, naux=%d, nfreq=%d, points=%d%s)" % (
            f(self.homo), f(self.lumo), f(self.gap), self.ef, len(self.orbs), self.naux, self.nfreq, int(self.sigma_points.numel()),
            ", linearized" if self.linearized else "")


def correlation_part(q):
    """Wc = -(1 + Q)^-1 Q of a batch of response matrices by Cholesky factorisation, not inv(1 + Q) - 1, which cancels where Q vanishes"""
    eye = torch.eye(int(q.shape[-1]), dtype=q.dtype, device=q.device)
    return -torch.cholesky_solve(q, torch.linalg.cholesky(q + eye))


def sigma_points(freqs, sigma_wmax):
    """the imaginary points the self-energy is evaluated at: 0 and the quadrature nodes below sigma_wmax"""
    return torch.cat([torch.zeros(1, dtype=freqs.dtype), freqs[freqs < float(sigma_wmax)]])


def _static_parts(qc, eps, c_orth, bn_occ):
    """per spin ((h + J)_nn, Sx_nn) for ALL orbitals: the Hamiltonian's own operators on the converged density, in the basis the Fock
    matrix lives in; Sx from the tensor (bn_occ[s]: (nmo, naux, nocc), or None) where the Hamiltonian cannot form K"""
    from .utils.datastruct import SpinParam
    eng = qc._engine
    h = eng.hamilton
    dm = qc.aodm()
    tot = SpinParam.sum(dm)
    hj = (h.get_kinnucl().fullmatrix() + h.get_elrep(tot).fullmatrix()).detach()
    no_k = h.df is not None and not h.df.exchange
    if not no_k:
        ex = h.get_exchange(dm)
        ks = [ex.u.fullmatrix().detach(), ex.d.fullmatrix().detach()] if eng.polarized else [ex.fullmatrix().detach()]
    out = []
    for s, c in enumerate(c_orth):
        hjn = ((c.t() @ hj) * c.t()).sum(1)
        if no_k:
            sx = -(bn_occ[s] ** 2).sum((1, 2))
        else:
            sx = ((c.t() @ ks[s]) * c.t()).sum(1)
        out.append((hjn, sx))
    return out


def _compute(qc, orbs, auxbasis, nfreq, freq_scale, sigma_wmax, batch=None):
    eng = qc._engine
    h = eng.hamilton
    df = b_tensor(qc, auxbasis)
    b = df._b
    spins = orbitals(qc, 0)
    focks = (qc._fock[0], qc._fock[1]) if eng.polarized else (qc._fock,)
    c_orth = [eng._eigpairs(f.detach())[1] for f in focks]
    c_all = [torch.cat([co, cv], dim=1) for co, cv, _, _ in spins]
    eps = [torch.cat([eo, ev]) for _, _, eo, ev in spins]
    nocc = [int(eo.numel()) for _, _, eo, _ in spins]
    nmo = int(eps[0].numel())
    orbs = list(range(nmo)) if orbs is None else orbs
    if max(orbs) >= nmo:
        raise ValueError("gw: orbs must lie in [0, %d), got %d" % (nmo, max(orbs)))
    ef = 0.5 * (max(float(eo[-1]) for _, _, eo, _ in spins if eo.numel()) + min(float(ev[0]) for _, _, _, ev in spins if ev.numel()))
    freqs, weights = frequency_grid(nfreq, freq_scale)
    points = sigma_points(freqs, sigma_wmax)
    fd = freqs.to(b.device)
    bovs = [transform_ov(b, co, cv) for co, cv, _, _ in spins]
    bns = [transform_ov(b, c[:, orbs].contiguous(), c) for c in c_all]
    # Q, Wc, the Cholesky factor and the solver's copy: four (nk, naux, naux) tensors per batch
    batches = response_batches(bovs, spins, fd, 2.0 if eng.polarized else 4.0, 4, batch)
    ws = [torch.empty((nfreq, len(orbs), nmo), dtype=b.dtype, device=b.device) for _ in spins]
    for k0, n, qk in batches:
        wc = correlation_part(qk).contiguous()
        for w, bn in zip(ws, bns):
            lib.gw_screened_diag(wc, bn, nmo, out=w[k0:k0 + n])
        del wc
    bn_occ = None
    if h.df is not None and not h.df.exchange:   # the exchange self-energy of ALL orbitals from the tensor
        bn_occ = [transform_ov(b, c, c[:, :no].contiguous())[:, :, :no] for c, no in zip(c_all, nocc)]
    static = _static_parts(qc, eps, c_orth, bn_occ)
    per_spin = []
    for s in range(len(spins)):
        sc = self_energy_reference(ws[s], eps[s], ef, fd, weights.to(b.device), points.to(b.device), scale=freq_scale).cpu()
        hjn, sx = static[s]
        e = eps[s].cpu()
        per_spin.append({"eps": e[orbs], "sigma_x": sx.cpu()[orbs], "vxc": (e - hjn.cpu())[orbs], "sigma_c_iw": sc,
                         "f_hf": (hjn + sx).cpu()[orbs]})
    return df, per_spin, orbs, nocc, points, ef, freqs, weights


def _solve(per_spin, points, ef, linearized):
    out = []
    for p in per_spin:
        pade = pade_thiele(1j * points.to(torch.complex128), p["sigma_c_iw"])
        e, z, ok = quasiparticle_solve(pade, p["eps"], p["f_hf"], ef, linearized)
        out.append(dict(p, qp=e, z=z, converged=ok))
    return out


def gw(qc, orbs=None, auxbasis=None, nfreq=100, freq_scale=1.0, sigma_wmax=2.0, linearized=False):
    """G0W0 quasiparticle energies of the converged HF / KS calculation `qc` (module docstring): a `GW` result object.
    orbs: the target orbitals, indices into the orbitals in energy order, the same for both spins of an unrestricted calculation
    (None: every orbital -- but continuation from the imaginary axis is reliable near the Fermi level only, NOT for core states).
    `auxbasis` as `mp2` takes it (the same references, the same refusals; a Hamiltonian built with densityfit(exchange=True) uses its
    own tensor).  nfreq, freq_scale: points and scale of the frequency quadrature (`rpa.frequency_grid`); sigma_wmax: the self-energy
    is continued from 0 and the nodes below this many Ha.  linearized=True: one Newton step from eps_n with the renormalisation factor
    Z instead of the solution of the quasiparticle equation.  Memoised on the converged state per argument set (the two ways to
    solve share everything but the last step); nothing is differentiable: the result is detached."""
    nfreq, freq_scale, sigma_wmax = int(nfreq), float(freq_scale), float(sigma_wmax)
    check_frequency_args("gw", nfreq, freq_scale)
    if not sigma_wmax > 0.0:
        raise ValueError("gw: sigma_wmax must be positive, got %g" % sigma_wmax)
    if orbs is not None:
        orbs = [int(o) for o in orbs]
        nmo = getattr(qc._engine, "shape", (None,))[-1]
        if not orbs or min(orbs) < 0 or len(set(orbs)) != len(orbs) or (nmo is not None and max(orbs) >= int(nmo)):
            raise ValueError("gw: orbs must be distinct orbital indices in [0, %s), got %s" % ("nmo" if nmo is None else int(nmo), orbs))
    unsupported(qc)
    assert qc._has_run, "run() the calculation first"
    key = ("gw", None if orbs is None else tuple(orbs), aux_key(qc, auxbasis), nfreq, freq_scale, sigma_wmax)
    df, per_spin, orbs, nocc, points, ef, freqs, weights = memoised(
        qc, key, lambda: _compute(qc, orbs, auxbasis, nfreq, freq_scale, sigma_wmax))
    return GW(_solve(per_spin, points, ef, bool(linearized)), orbs, nocc, points, ef, freqs, weights, linearized, df)


# `dqc_amd.gw` is this function once the package has imported it: the yardsticks stay reachable as dqc_amd.gw.screened_diag_reference ...
gw.screened_diag_reference = screened_diag_reference
gw.self_energy_reference = self_energy_reference
gw.pade_thiele = pade_thiele
gw.spectral_reference = spectral_reference

__all__ = ["gw", "GW", "screened_diag_reference", "self_energy_reference", "pade_thiele", "Pade", "spectral_reference", "SpectralSigma",
           "quasiparticle_solve", "correlation_part", "sigma_points"]
