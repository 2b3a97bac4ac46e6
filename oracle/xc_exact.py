"""An independent restatement of the 20 LDA / GGA functionals of the kernel set, for a POINTWISE reference.

Every functional is written ONCE, as the spin-polarised energy density e(rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd), over a small
namespace `ns` of elementary operations (cbrt, sqrt, log, log1p, exp, expm1, atan, asinh, pow, where, the constant pi).  The same
text runs on two backends:

    MP   mpmath: the truth, good to 50 digits in the value.  Derivatives are central differences with a relative step of 1e-20
         (mp.diff's scheme with an explicit step; all additive parts are differenced in one pass): first order
         (f(x+h) - f(x-h)) / 2h, and the product of the Hessian with a direction d as the mixed difference of
         e(x +- h e_k +- t d).  80 digits are carried for them, more where the variables differ by orders of magnitude
         (_work_dps).  The step is far inside the closest approach to a seam (1e-12) and small against exp(-0.27 s^2) at s = 100;
         halving it changes nothing at 1e-20 of the scale (checked by tests/test_xc_exact_cpu.py).
    TD   torch float64 with torch.autograd (second order: a second backward): the yardstick for what plain double arithmetic
         attains on the same formula.

Constants come from the papers cited in dqc_amd/csrc/xc_funcs.hpp in the libxc parametrisation named there; derived constants
(powers of pi, f''(0), ...) are computed in the backend.  This module imports neither dqc_amd nor oracle.xc.

A functional returns its value as a TUPLE OF ADDITIVE PARTS (the two spin channels of an exchange functional, for RPBE each split
into its constant and its exponential; rho eps_LDA and rho H
for PBE / P86 correlation; the four terms of the VWN / PW92 spin interpolation; the terms of LYP -- the -a... term and every term of
the -a b omega [...] bracket, which cancels completely for a fully polarised density).  The value is the sum of the parts; the SCALE
of a quantity at a point is the sum of the absolute values of the same derivative of every part, and errors are measured as
|got - truth| / scale: this does not punish the cancellation of eps + H at large s, and it punishes everything else pointwise.

Thresholds are those of libxc, which the kernels and this reference share as part of the functionals' definition: every output is
zero where rho_u + rho_d <= 1e-15; a spin density is raised to 0.5e-15; zeta enters the correlation functionals through its value
clamped to 1 -+ 1e-10 with the derivatives of the unclamped zeta (a constant offset `dz`).  `ns.switch(x)` is a series threshold:
x in double, 0 at 50 digits (the truth never takes a truncated series).  A gradient that is exactly zero is evaluated at a reduced
gradient of 1e-30, where every functional is smooth (the derivatives by sigma of gga_x_g96 diverge at sigma = 0: see the tests).

THE FOUR META-GGAS (MGGA_NAMES: mgga_x_scan, mgga_c_scan, mgga_x_tpss, mgga_c_tpss; value and first order) are written the same way
over (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd, tau_u, tau_d), from Sun, Ruzsinszky, Perdew, PRL 115, 036402 (2015) and Tao,
Perdew, Staroverov, Scuseria, PRL 91, 146401 (2003) with libxc's constants as dqc_amd/csrc/xc.hip names them.  Both correlation
functionals see tau_u + tau_d only; the exchange functionals are spin-scaled, one channel per spin at (2 rho_s, 4 sigma_ss, 2 tau_s).
Additive parts:
    exchange, per spin      SCAN: e_x^unif h1 g and e_x^unif f(alpha) (h0 - h1) g; TPSS: one part (its F_x has no cancellation)
    mgga_c_scan             rho eps_LSDA, rho H1, rho f(alpha) eps0, -rho f(alpha) eps1
    mgga_c_tpss             rho eps_LSDA and rho H of PBE; the same two times C(zeta, xi) z^2; the sum over the spins of
                            max(eps_PBE(n_s, 0), eps_PBE), again as its LSDA and its gradient part (eps_LSDA + H cancels at large s, and every
                            term that holds eps_PBE inherits that cancellation); d eps_revPKZB^2 z^3
Conventions shared with the kernels, part of the functionals' definition here:
    the density cutoff 1e-15 and the spin floor 0.5e-15, as above
    tau is raised to TAU_THRESHOLD = 1e-20, libxc's default: each exchange channel sees max(2 tau_s, 1e-20), the correlation
        functionals max(tau_u + tau_d, 1e-20), and the derivatives are those at the raised value (the offsets of effective_point)
    where tau_W > tau (z = tau_W / tau > 1) TPSS exchange takes the CONSTANTS z = 1, alpha = 0, TPSS correlation the constant z = 1
        (d/dtau = 0); SCAN applies no clamp on alpha < 0.  A constant is a branch decided at the point: the steps of the differences
        (1e-20) never reach from the closest approach sampled (1e-12) to z = 1, so the branch is the same at x + h and x - h
    these two are the project's own, UNPINNED against libxc as xc.hip says of them: the reference holds no literal of either
The sigma floor of the kernels is NOT a convention: the truth takes sigma as given, and an exact zero at a reduced gradient of TINY_S.
The alpha = 1 seam: f(alpha) and all its derivatives vanish from both sides (exp(-0.64e12) at the edge of the 1e-12 window in which
the kernels and the double backend return 0); a central difference may straddle it and changes nothing (step halving is tested on
both sides down to |1 - alpha| = 1e-14).  At a point with an exactly zero gradient the scale of every first derivative of a meta-GGA
is at least TINY_S of scale(e) / |x_k|: d/dtau through z is of the order sigma^2 there and its limit is 0 (mp_eval).
"""
from fractions import Fraction as Fr

import mpmath as mp

NAMES = ["lda_x", "lda_c_pw", "lda_c_pw_mod", "lda_c_vwn", "lda_c_pz", "gga_x_pbe", "gga_x_pbe_r", "gga_x_pbe_sol", "gga_x_rpbe",
         "gga_c_pbe", "gga_c_pbe_sol", "gga_x_b88", "gga_c_lyp", "gga_c_p86", "gga_x_pw91", "gga_x_b86", "gga_x_g96", "gga_x_pw86",
         "gga_x_optx", "gga_x_wc"]
DPS = 50
DENS_THRESHOLD, ZETA_THRESHOLD, TINY_S = 1e-15, 1e-10, 1e-30
TAU_THRESHOLD = 1e-20  # libxc's default: the kinetic energy density a meta-GGA sees is raised to it


# ------------------------------------------------------------------------------------------------ the two backends
class MP:
    """mpmath scalars at DPS digits"""
    name = "mpmath"

    def __init__(self, dps=DPS):
        mp.mp.dps = dps
        self.pi = +mp.pi

    cbrt = staticmethod(mp.cbrt)
    sqrt = staticmethod(mp.sqrt)
    log = staticmethod(mp.log)
    log1p = staticmethod(mp.log1p)
    exp = staticmethod(mp.exp)
    expm1 = staticmethod(mp.expm1)
    atan = staticmethod(mp.atan)
    asinh = staticmethod(mp.asinh)

    @staticmethod
    def pow(a, e):
        return mp.power(a, mp.mpf(e.numerator) / e.denominator)

    @staticmethod
    def where(c, a, b):
        return a if c else b

    @staticmethod
    def switch(x):
        return 0.0


class TD:
    """torch float64 tensors (torch is imported on first use: the truth needs mpmath only)"""
    name = "torch-double"

    def __init__(self):
        import math
        import torch
        self.t = torch
        self.pi = math.pi

    def _t(self, a):
        return a if isinstance(a, self.t.Tensor) else self.t.as_tensor(a, dtype=self.t.float64)

    def cbrt(self, a):
        return self._t(a).pow(1.0 / 3.0)

    def sqrt(self, a):
        return self._t(a).sqrt()

    def log(self, a):
        return self._t(a).log()

    def log1p(self, a):
        return self._t(a).log1p()

    def exp(self, a):
        return self._t(a).exp()

    def expm1(self, a):
        return self._t(a).expm1()

    def atan(self, a):
        return self._t(a).atan()

    def asinh(self, a):
        return self._t(a).asinh()

    def pow(self, a, e):
        return self._t(a).pow(float(e))

    def where(self, c, a, b):
        return self.t.where(c, self._t(a), self._t(b))

    @staticmethod
    def switch(x):
        return x


# ------------------------------------------------------------------------------------------------ exchange
def _x_parts(ns, F, ru, rd, suu, sdd):
    """spin-scaled exchange: e = sum_s -(3/4)(3/pi)^(1/3) 2^(1/3) rho_s^(4/3) F(x_s^2), x_s = |grad rho_s| / rho_s^(4/3)"""
    ax = -0.75 * ns.cbrt(3.0 / ns.pi) * ns.cbrt(2.0)
    out = []
    for r, s in ((ru, suu), (rd, sdd)):
        r43 = r * ns.cbrt(r)
        f = F(s / (r43 * r43))
        out += [ax * r43 * t for t in (f if isinstance(f, tuple) else (f,))]
    return tuple(out)


def _x2s2(ns):  # s^2 = x_s^2 / (4 (6 pi^2)^(2/3))
    c = ns.cbrt(6.0 * ns.pi * ns.pi)
    return 1.0 / (4.0 * c * c)


def _cx(ns):  # (3/2) (3 / (4 pi))^(1/3), Becke's C_x = libxc's X_FACTOR_C
    return 1.5 * ns.cbrt(3.0 / (4.0 * ns.pi))


_BETA_PBE = 0.06672455060314922  # libxc's beta of PBE; mu = beta pi^2 / 3


def _mu_pbe(ns):
    return _BETA_PBE * ns.pi * ns.pi / 3.0


def lda_x(ns, ru, rd, suu, sud, sdd, dz=0.0):
    return _x_parts(ns, lambda y: 1.0, ru, rd, suu, sdd)


def _pbe_x(kappa, mu_of, rpbe=False):
    def f(ns, ru, rd, suu, sud, sdd, dz=0.0):
        mu, c = mu_of(ns), _x2s2(ns)
        if rpbe:  # Hammer, Hansen, Norskov, PRB 59, 7413 (1999); two parts: the exponential is all of the gradient dependence
            return _x_parts(ns, lambda y: (1.0 + kappa, -kappa * ns.exp(-(mu / kappa) * (c * y))), ru, rd, suu, sdd)
        return _x_parts(ns, lambda y: 1.0 + kappa - kappa / (1.0 + (mu / kappa) * (c * y)), ru, rd, suu, sdd)
    return f


gga_x_pbe = _pbe_x(0.804, _mu_pbe)             # Perdew, Burke, Ernzerhof, PRL 77, 3865 (1996)
gga_x_pbe_r = _pbe_x(1.245, _mu_pbe)           # Zhang, Yang, PRL 80, 890 (1998)
gga_x_pbe_sol = _pbe_x(0.804, lambda ns: 10.0 / 81.0)  # Perdew et al., PRL 100, 136406 (2008)
gga_x_rpbe = _pbe_x(0.804, _mu_pbe, rpbe=True)


def _asinh_over_x(ns, y):
    """asinh(x) / x, x = sqrt(y), as a function of y: the quotient above the series threshold, its Taylor series below"""
    thr = ns.switch(1e-4)  # in y: x < 1e-2
    ys = ns.where(y > thr, y, 1.0)
    x = ns.sqrt(ys)
    series = 1.0 + y * (-1.0 / 6.0 + y * (3.0 / 40.0 + y * (-15.0 / 336.0 + y * (105.0 / 3456.0 + y * (-945.0 / 42240.0)))))
    return ns.where(y > thr, ns.asinh(x) / x, series)


def gga_x_b88(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Becke, PRA 38, 3098 (1988)
    beta, cx = 0.0042, _cx(ns)
    # _x_parts' prefactor is -(3/4)(3/pi)^(1/3) 2^(1/3) = -C_x: F = 1 + (beta / C_x) x^2 / (1 + 6 beta x asinh x)
    return _x_parts(ns, lambda y: 1.0 + (beta / cx) * y / (1.0 + 6.0 * beta * y * _asinh_over_x(ns, y)), ru, rd, suu, sdd)


def gga_x_pw91(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Perdew, Wang (1991/92); libxc: bt = 0.0042, alpha = 100, expo = 4
    bt, alpha = 0.0042, 100.0
    c2, cx = _x2s2(ns), _cx(ns)  # X2S^2, X_FACTOR_C
    x2s = ns.sqrt(c2)
    beta = 5.0 * ns.pow(36.0 * ns.pi, Fr(-5, 3))
    a, c, d, f = 6.0 * bt / x2s, bt / (cx * c2), -(bt - beta) / (cx * c2), 1.0e-6 / (cx * c2 * c2)

    def F(y):  # y = x_s^2 = s^2 / X2S^2; b s = x_s
        s2 = c2 * y
        s4 = s2 * s2
        sas = a * x2s * y * _asinh_over_x(ns, y)  # a s asinh(b s)
        return 1.0 + ((c + d * ns.exp(-alpha * s2)) * s2 - f * s4) / (1.0 + sas + f * s4)
    return _x_parts(ns, F, ru, rd, suu, sdd)


def gga_x_b86(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Becke, JCP 84, 4524 (1986)
    cx = _cx(ns)
    return _x_parts(ns, lambda y: 1.0 + (0.0036 / cx) * y / (1.0 + 0.004 * y), ru, rd, suu, sdd)


def gga_x_g96(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Gill, Mol. Phys. 89, 433 (1996)
    cx = _cx(ns)
    return _x_parts(ns, lambda y: 1.0 + ns.pow(y, Fr(3, 4)) / (137.0 * cx), ru, rd, suu, sdd)


def gga_x_pw86(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Perdew, Wang, PRB 33, 8800 (1986)
    c = _x2s2(ns)

    def F(y):
        s2 = c * y
        return ns.pow(1.0 + 1.296 * s2 + 14.0 * s2 * s2 + 0.2 * s2 * s2 * s2, Fr(1, 15))
    return _x_parts(ns, F, ru, rd, suu, sdd)


def gga_x_optx(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Handy, Cohen, Mol. Phys. 99, 403 (2001)
    cx = _cx(ns)

    def F(y):
        u = 0.006 * y / (1.0 + 0.006 * y)
        return 1.05151 + (1.43169 / cx) * u * u
    return _x_parts(ns, F, ru, rd, suu, sdd)


def gga_x_wc(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Wu, Cohen, PRB 73, 235116 (2006)
    kappa, mu, c2 = 0.804, _mu_pbe(ns), _x2s2(ns)
    c = (146.0 / 2025.0) * (4.0 / 9.0) - (73.0 / 405.0) * (2.0 / 3.0) + (mu - 10.0 / 81.0)

    def F(y):
        s2 = c2 * y
        x = (10.0 / 81.0) * s2 + (mu - 10.0 / 81.0) * s2 * ns.exp(-s2) + ns.log1p(c * s2 * s2)
        return 1.0 + kappa - kappa / (1.0 + x / kappa)
    return _x_parts(ns, F, ru, rd, suu, sdd)


# ------------------------------------------------------------------------------------------------ LDA correlation
def _rs_zeta(ns, ru, rd, dz):
    rho = ru + rd
    return rho, ns.cbrt(3.0 / (4.0 * ns.pi * rho)), (ru - rd) / rho + dz


def _fzeta(ns, zeta):  # f(zeta) = ((1 + zeta)^(4/3) + (1 - zeta)^(4/3) - 2) / (2^(4/3) - 2)
    p, m = 1.0 + zeta, 1.0 - zeta
    return (p * ns.cbrt(p) + m * ns.cbrt(m) - 2.0) / (2.0 * ns.cbrt(2.0) - 2.0)


def _fz20(ns):  # f''(0) = 4 / (9 (2^(1/3) - 1)) = 1.709920934161365617...
    return 4.0 / (9.0 * (ns.cbrt(2.0) - 1.0))


def _spin_interpolation(ns, rho, zeta, e_p, e_f, alpha_c):
    """rho [e_P + alpha_c f (1 - zeta^4) / f''(0) + (e_F - e_P) f zeta^4] as its four terms (VWN eq. 4.4 ff., PW92 eq. 8)"""
    f = _fzeta(ns, zeta)
    z2 = zeta * zeta
    z4 = z2 * z2
    return (rho * e_p, rho * alpha_c * f * (1.0 - z4) / _fz20(ns), rho * e_f * f * z4, -(rho * e_p * f * z4))


def _pw92_g(ns, rs, a, alpha1, b1, b2, b3, b4):  # Perdew, Wang, PRB 45, 13244 (1992), eq. 10 with p = 1
    sq = ns.sqrt(rs)
    q1 = 2.0 * a * (b1 * sq + b2 * rs + b3 * rs * sq + b4 * rs * rs)
    return -2.0 * a * (1.0 + alpha1 * rs) * ns.log1p(1.0 / q1)


_PW92_FIT = ((0.21370, 7.5957, 3.5876, 1.6382, 0.49294), (0.20548, 14.1189, 6.1977, 3.3662, 0.62517),
             (0.11125, 10.357, 3.6231, 0.88026, 0.49671))


def _pw92_parts(ns, ru, rd, dz, mod):
    rho, rs, zeta = _rs_zeta(ns, ru, rd, dz)
    if mod:  # libxc's lda_c_pw_mod: the exact A of the three fits
        a1 = (1.0 - ns.log(2.0)) / (ns.pi * ns.pi)
        a3 = (a1, 0.5 * a1, 1.0 / (6.0 * ns.pi * ns.pi))
    else:    # the six printed digits of the paper
        a3 = (0.0310907, 0.01554535, 0.0168869)
    g = [_pw92_g(ns, rs, a3[i], *_PW92_FIT[i]) for i in range(3)]
    return _spin_interpolation(ns, rho, zeta, g[0], g[1], -g[2])  # the third fit is of -alpha_c


def lda_c_pw(ns, ru, rd, suu, sud, sdd, dz=0.0):
    return _pw92_parts(ns, ru, rd, dz, False)


def lda_c_pw_mod(ns, ru, rd, suu, sud, sdd, dz=0.0):
    return _pw92_parts(ns, ru, rd, dz, True)


def _vwn_fit(ns, x, A, b, c, x0):  # Vosko, Wilk, Nusair, Can. J. Phys. 58, 1200 (1980), eq. 4.4; x = sqrt(rs)
    Q = ns.sqrt(4.0 * c - b * b)
    X0 = x0 * x0 + b * x0 + c
    X = x * x + b * x + c
    at = ns.atan(Q / (2.0 * x + b))
    xm = x - x0
    return A * (ns.log(x * x / X) + (2.0 * b / Q) * at - (b * x0 / X0) * (ns.log(xm * xm / X) + (2.0 * (b + 2.0 * x0) / Q) * at))


def lda_c_vwn(ns, ru, rd, suu, sud, sdd, dz=0.0):  # VWN5
    rho, rs, zeta = _rs_zeta(ns, ru, rd, dz)
    x = ns.sqrt(rs)
    e_p = _vwn_fit(ns, x, 0.0310907, 3.72744, 12.9352, -0.10498)
    e_f = _vwn_fit(ns, x, 0.01554535, 7.06042, 18.0578, -0.32500)
    a_c = _vwn_fit(ns, x, -1.0 / (6.0 * ns.pi * ns.pi), 1.13107, 13.0045, -0.0047584)
    return _spin_interpolation(ns, rho, zeta, e_p, e_f, a_c)


def _pz81_channel(ns, rs, gam, b1, b2, A, B, C, D):  # Perdew, Zunger, PRB 23, 5048 (1981), appendix C
    low = gam / (1.0 + b1 * ns.sqrt(rs) + b2 * rs)
    lr = ns.log(rs)
    high = A * lr + B + C * rs * lr + D * rs
    return ns.where(rs >= 1.0, low, high)


def _pz81_parts(ns, rho, rs, zeta):
    e_p = _pz81_channel(ns, rs, -0.1423, 1.0529, 0.3334, 0.0311, -0.048, 0.0020, -0.0116)
    e_f = _pz81_channel(ns, rs, -0.0843, 1.3981, 0.2611, 0.01555, -0.0269, 0.0007, -0.0048)
    f = _fzeta(ns, zeta)
    return (rho * e_p, rho * e_f * f, -(rho * e_p * f))


def lda_c_pz(ns, ru, rd, suu, sud, sdd, dz=0.0):
    rho, rs, zeta = _rs_zeta(ns, ru, rd, dz)
    return _pz81_parts(ns, rho, rs, zeta)


# ------------------------------------------------------------------------------------------------ GGA correlation
def gga_c_p86(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Perdew, PRB 33, 8822 (1986)
    rho, rs, zeta = _rs_zeta(ns, ru, rd, dz)
    lda = _pz81_parts(ns, rho, rs, zeta)
    a, b, g, d, ft = 0.023266, 7.389e-6, 8.723, 0.472, 0.11
    rs2 = rs * rs
    cn = 0.001667 + (0.002568 + a * rs + b * rs2) / (1.0 + g * rs + d * rs2 + 1.0e4 * b * rs2 * rs)
    cinf = 0.001667 + 0.002568
    sig = suu + 2.0 * sud + sdd
    phi = 1.745 * ft * (cinf / cn) * ns.sqrt(sig) / ns.pow(rho, Fr(7, 6))
    dzeta = ns.cbrt(2.0) * ns.sqrt(ns.pow(0.5 * (1.0 + zeta), Fr(5, 3)) + ns.pow(0.5 * (1.0 - zeta), Fr(5, 3)))
    H = ns.exp(-phi) * cn * sig / (dzeta * rho * ns.cbrt(rho))
    return (lda[0] + lda[1] + lda[2], H)


def _pbe_c(beta):
    def f(ns, ru, rd, suu, sud, sdd, dz=0.0):  # Perdew, Burke, Ernzerhof, PRL 77, 3865 (1996), eqs. 3, 7, 8
        rho, rs, zeta = _rs_zeta(ns, ru, rd, dz)
        lda = _pw92_parts(ns, ru, rd, dz, True)
        eps = (lda[0] + lda[1] + lda[2] + lda[3]) / rho
        gamma = (1.0 - ns.log(2.0)) / (ns.pi * ns.pi)
        p, m = ns.cbrt(1.0 + zeta), ns.cbrt(1.0 - zeta)
        phi = 0.5 * (p * p + m * m)
        phi3 = phi * phi * phi
        kf = ns.cbrt(3.0 * ns.pi * ns.pi * rho)
        sig = suu + 2.0 * sud + sdd
        t2 = sig / (4.0 * phi * phi * (4.0 * kf / ns.pi) * rho * rho)
        A = (beta / gamma) / ns.expm1(-eps / (gamma * phi3))
        at2 = A * t2
        H = gamma * phi3 * ns.log1p((beta / gamma) * t2 * (1.0 + at2) / (1.0 + at2 + at2 * at2))
        return (rho * eps, rho * H)
    return f


gga_c_pbe = _pbe_c(_BETA_PBE)
gga_c_pbe_sol = _pbe_c(0.046)


def gga_c_lyp(ns, ru, rd, suu, sud, sdd, dz=0.0):
    """Lee, Yang, Parr, PRB 37, 785 (1988) in the form of Miehlich, Savin, Stoll, Preuss, CPL 157, 200 (1989), eq. 2"""
    a, b, c, d = 0.04918, 0.132, 0.2533, 0.349
    k = ns.cbrt(3.0 * ns.pi * ns.pi)
    cf = 0.3 * k * k
    rho = ru + rd
    ir13 = 1.0 / ns.cbrt(rho)
    den = 1.0 + d * ir13
    delta = c * ir13 + d * ir13 / den
    r2 = rho * rho
    om = -a * b * ns.exp(-c * ir13) / (den * ns.pow(rho, Fr(11, 3)))
    sig = suu + 2.0 * sud + sdd
    ab = ru * rd
    ra83, rb83 = ru * ru * ns.pow(ru, Fr(2, 3)), rd * rd * ns.pow(rd, Fr(2, 3))
    return (-4.0 * a * ab / (rho * den),
            om * ab * (ns.pow(2.0, Fr(11, 3)) * cf) * (ra83 + rb83),
            om * ab * (47.0 / 18.0 - 7.0 * delta / 18.0) * sig,
            -(om * ab * (2.5 - delta / 18.0) * (suu + sdd)),
            -(om * ab * ((delta - 11.0) / 9.0) * (ru / rho * suu + rd / rho * sdd)),
            -(om * (2.0 / 3.0) * r2 * sig),
            om * ((2.0 / 3.0) * r2 - ru * ru) * sdd,
            om * ((2.0 / 3.0) * r2 - rd * rd) * suu)


# ------------------------------------------------------------------------------------------------ meta-GGA
# e(rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd, tau_u, tau_d); `off` = (dz, dc): the offset of zeta and the offset that turns
# tau_u + tau_d into what the correlation functionals see (effective_point)
def _kf2(ns, n):  # (3 pi^2 n)^(2/3)
    k = ns.cbrt(3.0 * ns.pi * ns.pi * n)
    return k * k


def _mx_parts(ns, F, ru, rd, suu, sdd, tu, td):
    """spin-scaled meta-GGA exchange: e = sum_s (1/2) e_x^unif(n) F(p, z, alpha) at n = 2 rho_s, |grad n|^2 = 4 sigma_ss, tau = 2 tau_s,
    with p = s^2 = |grad n|^2 / (4 (3 pi^2)^(2/3) n^(8/3)), z = tau_W / tau, alpha = (tau - tau_W) / tau_unif, tau_W = |grad n|^2 / (8 n),
    tau_unif = (3/10) (3 pi^2)^(2/3) n^(5/3); F returns the factors of the additive parts"""
    ax = -0.75 * ns.cbrt(3.0 / ns.pi)
    out = []
    for r, s, t in ((ru, suu, tu), (rd, sdd, td)):
        n, sg, ta = 2.0 * r, 4.0 * s, 2.0 * t
        kf2 = _kf2(ns, n)
        tw = sg / (8.0 * n)
        f = F(sg / (4.0 * kf2 * n * n), tw / ta, (ta - tw) / (0.3 * kf2 * n))
        out += [0.5 * ax * n * ns.cbrt(n) * v for v in f]
    return tuple(out)


def _scan_switch(ns, alpha, c1, c2, d):
    """f(alpha) = exp(-c1 alpha / (1 - alpha)) for alpha < 1, -d exp(c2 / (1 - alpha)) for alpha > 1: flat to all orders at alpha = 1, where
    the double backend takes 0 inside |1 - alpha| < 1e-12 (exp(-0.64e12) at its edge); the truth has no window"""
    om = 1.0 - alpha
    near = om * om < ns.switch(1e-24)
    lo = alpha < 1.0
    om_lo = ns.where(near, 1.0, ns.where(lo, om, 1.0))
    om_hi = ns.where(near, -1.0, ns.where(lo, -1.0, om))
    f_lo = ns.exp(-c1 * ns.where(near, 0.5, ns.where(lo, alpha, 0.5)) / om_lo)
    f_hi = -d * ns.exp(c2 / om_hi)
    return ns.where(near, 0.0, ns.where(lo, f_lo, f_hi))


def mgga_x_scan(ns, ru, rd, suu, sud, sdd, tu, td, off=(0.0, 0.0)):
    """Sun, Ruzsinszky, Perdew, PRL 115, 036402 (2015), eqs. 1-8 and the supplementary material; no clamp on alpha < 0.
    Parts per spin: e_x^unif h1 g and e_x^unif f (h0 - h1) g"""
    a1, c1x, c2x, dx, k1, h0, b3, mu = 4.9479, 0.667, 0.8, 1.24, 0.065, 1.174, 0.5, 10.0 / 81.0
    b2 = ns.sqrt(5913.0 / 405000.0)
    b1 = (511.0 / 13500.0) / (2.0 * b2)
    b4 = mu * mu / k1 - 1606.0 / 18225.0 - b1 * b1

    def F(p, z, alpha):
        om = 1.0 - alpha
        y = b1 * p + b2 * om * ns.exp(-b3 * om * om)
        x = mu * p * (1.0 + (b4 * p / mu) * ns.exp(-(abs(b4) / mu) * p)) + y * y
        h1 = 1.0 + k1 * (x / (k1 + x))  # = 1 + k1 - k1 / (1 + x / k1), exactly 1 at x = 0
        g = -ns.expm1(-a1 / ns.pow(p, Fr(1, 4)))
        f = _scan_switch(ns, alpha, c1x, c2x, dx)
        return (h1 * g, f * (h0 - h1) * g)
    return _mx_parts(ns, F, ru, rd, suu, sdd, tu, td)


def mgga_x_tpss(ns, ru, rd, suu, sud, sdd, tu, td, off=(0.0, 0.0)):
    """Tao, Perdew, Staroverov, Scuseria, PRL 91, 146401 (2003), eqs. 5-10; where tau_W > tau: the constants z = 1, alpha = 0.
    One part per spin"""
    kappa, b, c, e, mu = 0.804, 0.40, 1.59096, 1.537, 0.21951
    se = ns.sqrt(e)

    def F(p, z, alpha):
        over = z > 1.0
        z, alpha = ns.where(over, 1.0, z), ns.where(over, 0.0, alpha)
        qb = (9.0 / 20.0) * (alpha - 1.0) / ns.sqrt(1.0 + b * alpha * (alpha - 1.0)) + 2.0 * p / 3.0
        z2 = z * z
        w = 0.36 * z2  # (3 z / 5)^2
        num = ((10.0 / 81.0 + c * z2 / ((1.0 + z2) * (1.0 + z2))) * p + (146.0 / 2025.0) * qb * qb
               - (73.0 / 405.0) * qb * ns.sqrt(0.5 * w + 0.5 * p * p) + ((10.0 / 81.0) * (10.0 / 81.0) / kappa) * p * p
               + 2.0 * se * (10.0 / 81.0) * w + e * mu * p * p * p)
        x = num / ((1.0 + se * p) * (1.0 + se * p))
        return (1.0 + kappa * (x / (kappa + x)),)  # = 1 + kappa - kappa / (1 + x / kappa), exactly 1 at x = 0
    return _mx_parts(ns, F, ru, rd, suu, sdd, tu, td)


def mgga_c_scan(ns, ru, rd, suu, sud, sdd, tu, td, off=(0.0, 0.0)):
    """Sun, Ruzsinszky, Perdew, PRL 115, 036402 (2015), eqs. 9-17 and the supplementary material, libxc's constants; no clamp on
    alpha < 0.  Parts: rho eps_LSDA, rho H1, rho f eps0, -rho f eps1"""
    b1c, b2c, b3c, c1c, c2c, dc_, chi_inf, gcnst = 0.0285764, 0.0889, 0.125541, 0.64, 1.5, 0.7, 0.12802585262625815, 2.3631
    dz, dc = off
    rho, rs, zeta = _rs_zeta(ns, ru, rd, dz)
    lda = _pw92_parts(ns, ru, rd, dz, True)
    eps = (lda[0] + lda[1] + lda[2] + lda[3]) / rho
    gamma = (1.0 - ns.log(2.0)) / (ns.pi * ns.pi)
    zp, zm = 1.0 + zeta, 1.0 - zeta
    cp, cm = ns.cbrt(zp), ns.cbrt(zm)
    phi = 0.5 * (cp * cp + cm * cm)
    phi3 = phi * phi * phi
    dxz = 0.5 * (zp * cp + zm * cm)
    dsz = 0.5 * (zp * cp * cp + zm * cm * cm)
    kf = ns.cbrt(3.0 * ns.pi * ns.pi * rho)
    sig = suu + 2.0 * sud + sdd
    s2 = sig / (4.0 * kf * kf * rho * rho)
    alpha = ((tu + td + dc) - sig / (8.0 * rho)) / (0.3 * kf * kf * rho * dsz)
    f = _scan_switch(ns, alpha, c1c, c2c, dc_)
    beta = 0.066725 * (1.0 + 0.1 * rs) / (1.0 + 0.1778 * rs)
    t2 = sig / (4.0 * phi * phi * (4.0 * kf / ns.pi) * rho * rho)
    w1 = ns.expm1(-eps / (gamma * phi3))
    # 1 - (1 + y)^(-1/4) without the cancellation at small y
    h1 = gamma * phi3 * ns.log1p(-w1 * ns.expm1(-0.25 * ns.log1p(4.0 * (beta / (gamma * w1)) * t2)))
    e0 = -b1c / (1.0 + b2c * ns.sqrt(rs) + b3c * rs)
    w0 = ns.expm1(-e0 / b1c)
    z2 = zeta * zeta
    z6 = z2 * z2 * z2
    gc = (1.0 - gcnst * (dxz - 1.0)) * (1.0 - z6 * z6)
    eps0 = (e0 + b1c * ns.log1p(-w0 * ns.expm1(-0.25 * ns.log1p(4.0 * chi_inf * s2)))) * gc
    return (rho * eps, rho * h1, rho * f * eps0, -(rho * f * (eps + h1)))


def _pbe_eps(ns, rho, eps, phi, sig):
    """(eps_LSDA, H) of PBE correlation (PRL 77, 3865, eqs. 3, 7, 8) of a density rho with the LSDA energy eps and the spin factor phi"""
    gamma, bg = (1.0 - ns.log(2.0)) / (ns.pi * ns.pi), _BETA_PBE * ns.pi * ns.pi / (1.0 - ns.log(2.0))
    phi3 = phi * phi * phi
    kf = ns.cbrt(3.0 * ns.pi * ns.pi * rho)
    t2 = sig / (4.0 * phi * phi * (4.0 * kf / ns.pi) * rho * rho)
    at2 = bg / ns.expm1(-eps / (gamma * phi3)) * t2
    return eps, gamma * phi3 * ns.log1p(bg * t2 * (1.0 + at2) / (1.0 + at2 + at2 * at2))


def mgga_c_tpss(ns, ru, rd, suu, sud, sdd, tu, td, off=(0.0, 0.0)):
    """Tao, Perdew, Staroverov, Scuseria, PRL 91, 146401 (2003), eqs. 11-14:
        eps_revPKZB = eps_PBE [1 + C z^2] - [1 + C] z^2 sum_s (n_s / n) max(eps_PBE(n_s, 0, grad n_s, 0), eps_PBE),  z = tau_W / tau,
        e = n eps_revPKZB [1 + d eps_revPKZB z^3],  d = 2.8,  C(zeta, xi) = (0.53 + 0.87 zeta^2 + 0.50 zeta^4 + 2.26 zeta^6)
        / {1 + xi^2 [(1 + zeta)^(-4/3) + (1 - zeta)^(-4/3)] / 2}^4,  xi = |grad zeta| / (2 (3 pi^2 n)^(1/3));
    where z > 1: the constant z = 1.  Parts: n eps_LSDA and n H (the two of PBE); the same two times C z^2; the sum of the maxima, again
    as its LSDA and its gradient part (eps_LSDA + H cancels at large s, and every term that holds eps_PBE inherits that); the d term"""
    dz, dc = off
    rho, rs, zeta = _rs_zeta(ns, ru, rd, dz)
    lda = _pw92_parts(ns, ru, rd, dz, True)
    zp, zm = 1.0 + zeta, 1.0 - zeta
    cp, cm = ns.cbrt(zp), ns.cbrt(zm)
    sig = suu + 2.0 * sud + sdd
    el, hl = _pbe_eps(ns, rho, (lda[0] + lda[1] + lda[2] + lda[3]) / rho, 0.5 * (cp * cp + cm * cm), sig)
    eps = el + hl
    ferro = 1.0 / ns.cbrt(2.0)  # phi(zeta = 1); the LSDA energy there is PW92's ferromagnetic fit
    a_f = 0.5 * (1.0 - ns.log(2.0)) / (ns.pi * ns.pi)
    etl, eth = [], []  # the maxima, as their LSDA and gradient parts
    for r, s in ((ru, suu), (rd, sdd)):
        e1 = _pbe_eps(ns, r, _pw92_g(ns, ns.cbrt(3.0 / (4.0 * ns.pi * r)), a_f, *_PW92_FIT[1]), ferro, s)
        one = e1[0] + e1[1] >= eps
        etl.append(ns.where(one, e1[0], el))
        eth.append(ns.where(one, e1[1], hl))
    z2_ = zeta * zeta
    c0 = 0.53 + 0.87 * z2_ + 0.50 * z2_ * z2_ + 2.26 * z2_ * z2_ * z2_
    xi2 = (zm * zm * suu - 2.0 * zm * zp * sud + zp * zp * sdd) / (rho * rho) / (4.0 * _kf2(ns, rho))
    cd = 1.0 + 0.5 * xi2 * (1.0 / (zp * cp) + 1.0 / (zm * cm))
    C = c0 / (cd * cd * cd * cd)
    z = sig / (8.0 * rho * (tu + td + dc))
    z = ns.where(z > 1.0, 1.0, z)
    zz = z * z
    czz, mzz = C * zz, -((1.0 + C) * zz)
    p4l, p4h = mzz * (ru * etl[0] + rd * etl[1]) / rho, mzz * (ru * eth[0] + rd * eth[1]) / rho
    erev = (el + hl) + (el * czz + hl * czz) + (p4l + p4h)
    return (rho * el, rho * hl, rho * el * czz, rho * hl * czz, rho * p4l, rho * p4h, rho * 2.8 * erev * erev * zz * z)


MGGA_NAMES = ["mgga_x_scan", "mgga_c_scan", "mgga_x_tpss", "mgga_c_tpss"]
FUNCS = {n: globals()[n] for n in NAMES}
MGGA_FUNCS = {n: globals()[n] for n in MGGA_NAMES}
ALL_FUNCS = dict(FUNCS, **MGGA_FUNCS)
IS_GGA = {n: n.startswith("gga_") for n in NAMES}


# ------------------------------------------------------------------------------------------------ inputs and thresholds
def _work_dps(rhos, sigmas):
    """digits to carry at a point.  The steps are relative to each variable, and a functional may depend on it only through a
    sum with a much larger one (rho_u + rho_d, sigma_uu + 2 sigma_ud + sigma_dd) or through 1 + O(s^2): a second difference then
    resolves the square of the ratio, so twice its decimal exponent is added for the densities, the gradients and s^2 < 1"""
    extra = 0.0
    for v in (rhos, sigmas):
        extra += 2.0 * float(mp.log10(max(v) / min(v)))
    s2 = min([mp.mpf(1)] + [sg / mp.power(r, mp.mpf(8) / 3) for r, sg in zip(rhos, sigmas)])
    extra += 2.0 * float(-mp.log10(s2))
    return DPS + 30 + int(extra)  # 30: a second difference with steps of 1e-20 leaves 40 digits of the function behind


def _mgga_dps(rhos, sigmas, taus):
    """digits to carry at a meta-GGA point: first order only, so the decimal exponent of each ratio is added once"""
    extra = sum(float(mp.log10(max(v) / min(v))) for v in (rhos, sigmas, taus))
    s2 = min([mp.mpf(1)] + [sg / mp.power(r, mp.mpf(8) / 3) for r, sg in zip(rhos, sigmas)])
    return DPS + 30 + int(extra + float(-mp.log10(s2)))


def _effective_point_mgga(ru, rd, suu, sud, sdd, tu, td):
    """effective_point with tau: (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd, tau_u, tau_d) with each 2 tau_s raised to TAU_THRESHOLD (what
    the spin-scaled exchange sees), and the offsets (dz, dc): the correlation functionals see tau_u + tau_d + dc = max(tau_u + tau_d,
    TAU_THRESHOLD) of the taus given"""
    mp.mp.dps = 4 * DPS
    if not (float(ru) + float(rd) > DENS_THRESHOLD):
        return None
    x, dz, _, zero = effective_point(ru, rd, suu, sud, sdd)
    mp.mp.dps = 4 * DPS
    tu, td = mp.mpf(float(tu)), mp.mpf(float(td))
    thr = mp.mpf(TAU_THRESHOLD)
    eu, ed = max(2 * tu, thr) / 2, max(2 * td, thr) / 2
    dc = max(mp.mpf(float(tu) + float(td)), thr) - (eu + ed)  # the kernels add in double
    return x + (eu, ed), (dz, dc), _mgga_dps(x[:2], (x[2], x[4]), (eu, ed)), zero


def effective_point(ru, rd, suu, sud, sdd, tu=None, td=None):
    """the point the functional is evaluated at, the offset of zeta, the digits to carry and the variables that stand for a zero: libxc's thresholds (see the module
    docstring), exact zero gradients replaced by a reduced gradient of TINY_S.  Exact arithmetic on the doubles given; None below
    the density cutoff.  With tu, td: the seven variables of a meta-GGA and the offsets (dz, dc) (_effective_point_mgga)."""
    if tu is not None:
        return _effective_point_mgga(ru, rd, suu, sud, sdd, tu, td)
    mp.mp.dps = 4 * DPS
    ru, rd, suu, sud, sdd = (mp.mpf(float(v)) for v in (ru, rd, suu, sud, sdd))
    if not (float(ru) + float(rd) > DENS_THRESHOLD):  # the kernels add in double
        return None
    ru, rd = max(ru, mp.mpf(0.5 * DENS_THRESHOLD)), max(rd, mp.mpf(0.5 * DENS_THRESHOLD))
    tiny = mp.mpf(TINY_S) ** 2
    zero = [k for k, v in ((2, suu), (4, sdd)) if v == 0]
    if suu == 0:
        suu = tiny * mp.power(ru, mp.mpf(8) / 3)
    if sdd == 0:
        sdd = tiny * mp.power(rd, mp.mpf(8) / 3)
    zeta = (ru - rd) / (ru + rd)
    lim = 1 - mp.mpf(ZETA_THRESHOLD)
    dz = min(max(zeta, -lim), lim) - zeta
    return (ru, rd, suu, sud, sdd), dz, _work_dps((ru, rd), (suu, sdd)), (zero + [3] if len(zero) == 2 else zero)


def unpolarised(rho, sigma, tau=None):
    """the unpolarised form is the polarised form at rho_u = rho_d = rho / 2, sigma_uu = sigma_ud = sigma_dd = sigma / 4
    (and tau_u = tau_d = tau / 2 for a meta-GGA)"""
    x = (0.5 * rho, 0.5 * rho, 0.25 * sigma, 0.25 * sigma, 0.25 * sigma)
    return x if tau is None else x + (0.5 * tau, 0.5 * tau)


def effective_point_unpol(rho, sigma, tau=None):
    """(rho, sigma) of a closed-shell point with the same conventions; None below the density cutoff.  With tau: (rho, sigma, tau)
    with tau raised to TAU_THRESHOLD, and the offsets (dz, dc) = (0, 0) of a meta-GGA"""
    mp.mp.dps = 4 * DPS
    rho, sigma = mp.mpf(float(rho)), mp.mpf(float(sigma))
    if not (float(rho) > DENS_THRESHOLD):
        return None
    zero = [1] if sigma == 0 else []
    if sigma == 0:
        sigma = mp.mpf(TINY_S) ** 2 * 4 * mp.power(rho / 2, mp.mpf(8) / 3)
    if tau is not None:
        tau = max(mp.mpf(float(tau)), mp.mpf(TAU_THRESHOLD))
        return (rho, sigma, tau), (mp.mpf(0), mp.mpf(0)), _mgga_dps((rho / 2,), (sigma / 4,), (tau,)), zero
    return (rho, sigma), mp.mpf(0), _work_dps((rho / 2,), (sigma / 4,)), zero


# ------------------------------------------------------------------------------------------------ the truth
H_REL = 1e-20
# Underflow: a term more than DBL_MIN / DBL_EPSILON = 1e-292 below the terms it is added to cannot be carried by a double (exp(-z)
# is subnormal or zero for z > 708, as in the RPBE enhancement factor at s > 50 and LYP's omega at rho < 1e-10).  The scale of a
# derivative by x_k is therefore at least 1e-292 scale(e) / |x_k|, that of (H d)_k at least that times max_j |d_j / x_j|.
# Where sigma stands for an exact zero (TINY_S^2 of its natural size) the constant is TINY_S^3: the reference is the limit to TINY_S.
SCALE_FLOOR = 2.2250738585072014e-308 / 2.220446049250313e-16


def _steps(x):
    """the step of each variable: relative to its own size; sigma_ud (which may vanish or be negative) relative to sigma_uu + sigma_dd"""
    if len(x) in (2, 3):
        return [abs(v) for v in x]
    return [abs(x[0]), abs(x[1]), abs(x[2]), abs(x[2]) + abs(x[4]), abs(x[4])] + [abs(v) for v in x[5:]]


def _shift(x, k, h):
    y = list(x)
    y[k] = y[k] + h
    return y


def _re(v):
    return v.real if isinstance(v, mp.mpc) else v


def _embed(y):
    return y if len(y) in (5, 7) else unpolarised(*y)


def mp_eval(name, x, dz, delta=None, h_rel=H_REL, variables=None, dps=DPS, number=float, zero=()):
    """truth and scale of e, of every first derivative (by the variables listed) and of the product of the Hessian with `delta`
    (one component per variable, or None) at x = (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd) or the closed-shell (rho, sigma)
    -> {"e": (truth, scale), "d1": {k: (truth, scale)}, "d2": {k: (truth, scale)}} as floats (number=mp.mpf: as they are); mpmath central
    differences of every part at once"""
    ns = MP(max(dps, DPS + 30))
    f = ALL_FUNCS[name]
    variables = range(len(x)) if variables is None else variables

    def parts(y):
        return [_re(p) for p in f(ns, *_embed(y), dz)]

    def combine(vals):
        return number(mp.fsum(vals)), number(mp.fsum(abs(v) for v in vals))

    st = _steps(x)
    out = {"e": combine(parts(x)), "d1": {}, "d2": {}}
    # a variable that stands for an exact zero is TINY_S^2 of its natural size, and the truth there is TINY_S from the limit
    # (TINY_S of the derivative's natural size, scale(e) / sigma at a reduced gradient of 1).  Meta-GGA, len(x) = 3 or 7: the other
    # derivatives at such a point as well, TINY_S of scale(e) / |x_k| -- d/dtau through z = tau_W / tau is of the order sigma^2 / tau^3
    # there, its limit is 0, and with tau at its threshold the truth at TINY_S is not yet at that limit
    near_limit = bool(zero) and len(x) in (3, 7)
    floor = [mp.mpf(TINY_S ** 3 if k in zero else TINY_S if near_limit else SCALE_FLOOR) * out["e"][1] for k in range(len(x))]

    def floored(ts, lo):
        return ts[0], max(ts[1], number(lo))

    hh = mp.mpf(h_rel)
    for k in variables:
        h = hh * st[k]
        p, m = parts(_shift(x, k, h)), parts(_shift(x, k, -h))
        out["d1"][k] = floored(combine([(a - b) / (2 * h) for a, b in zip(p, m)]), floor[k] / st[k])
    if delta is not None:
        dl = [mp.mpf(float(v)) for v in delta]
        t = hh
        xp = [a + t * b for a, b in zip(x, dl)]
        xm = [a - t * b for a, b in zip(x, dl)]
        for k in variables:
            h = hh * st[k]
            pp, pm = parts(_shift(xp, k, h)), parts(_shift(xp, k, -h))
            mp_, mm = parts(_shift(xm, k, h)), parts(_shift(xm, k, -h))
            out["d2"][k] = floored(combine([(a - b - c + d) / (4 * h * t) for a, b, c, d in zip(pp, pm, mp_, mm)]),
                                   floor[k] / st[k] * max(abs(b) / c for b, c in zip(dl, st)))
    return out


# ------------------------------------------------------------------------------------------------ the double yardstick
def td_eval(name, x, dz, delta=None):
    """the same quantities from the torch-double backend for a batch of points: x (5, n) or (2, n), dz (n,), delta like x or None
    -> e (n,), d1, d2 (or None) shaped like x, as numpy arrays (value = sum of the parts, in the order of the tuple)"""
    import numpy as np
    import torch
    ns = TD()
    xs = [torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in x]
    dzt = torch.tensor(np.asarray(dz, dtype=np.float64))
    parts = ALL_FUNCS[name](ns, *_embed(xs), dzt)
    e = sum(parts[1:], parts[0])
    g = torch.autograd.grad(e.sum(), xs, create_graph=True, allow_unused=True)
    g = [torch.zeros_like(xs[0]) if a is None else a for a in g]
    d2 = None
    if delta is not None:
        dl = [torch.tensor(np.asarray(v, dtype=np.float64)) for v in delta]
        gd = sum(a * b for a, b in zip(g, dl))
        hv = torch.autograd.grad(gd.sum(), xs, allow_unused=True) if gd.requires_grad else [None] * len(xs)
        d2 = np.stack([(torch.zeros_like(xs[0]) if a is None else a).detach().numpy() for a in hv])
    return e.detach().numpy(), np.stack([a.detach().numpy() for a in g]), d2


# ------------------------------------------------------------------------------------------------ outputs of the kernels
# what the entry points of dqc_amd/csrc/xc.hip return, composed from the rows of the fixtures (tools/make_xc_exact_golden.py):
# v_grad = 2 v_sigma grad rho (per spin 2 v_ss grad rho_s + v_ud grad rho_s') and its response; with absolute=True the same
# formulas with absolute values, which turn the scales of the rows into the scales of the outputs
UNPOL_OUTPUTS = ("e", "vrho", "vgrad", "dvrho", "dvgrad", "t_dvrho", "t_dvgrad")
POL_OUTPUTS = ("e", "vrho_u", "vrho_d", "vgrad_u", "vgrad_d", "dvrho_u", "dvrho_d", "dvgrad_u", "dvgrad_d")


MGGA_UNPOL_OUTPUTS = ("e", "vrho", "vgrad", "vtau")
MGGA_POL_OUTPUTS = ("e", "vrho_u", "vrho_d", "vgrad_u", "vgrad_d", "vtau_u", "vtau_d")


def unpol_excluded(name, p):
    """{output: bool mask over the points} of what a comparison leaves out (p: rho, grho): the d v_grad of gga_x_g96 where grad rho
    is exactly zero -- its v_sigma ~ sigma^(-1/4) does not exist there (v_grad itself is compared, and is 0).  Meta-GGA: nothing"""
    import numpy as np
    if name in MGGA_FUNCS:
        return {o: np.zeros(p["rho"].shape[0], dtype=bool) for o in MGGA_UNPOL_OUTPUTS}
    zero_g = (np.abs(p["grho"]).sum(0) == 0.0) & (p["rho"] > DENS_THRESHOLD)
    m = {o: np.zeros(p["rho"].shape[0], dtype=bool) for o in UNPOL_OUTPUTS}
    if name == "gga_x_g96":
        m["dvgrad"] = m["t_dvgrad"] = zero_g
    return m


def pol_excluded(name, p):
    """the same for a polarised point set (p: rho_u, rho_d, grho_u, grho_d): the outputs of the empty spin at fully polarised points
    (rho_d = 0), and the d v_grad of gga_x_g96 of a spin whose gradient is exactly zero"""
    import numpy as np
    live = p["rho_u"] + p["rho_d"] > DENS_THRESHOLD
    full = (p["rho_d"] == 0.0) & live
    if name in MGGA_FUNCS:  # the empty spin only; the v_tau of a correlation functional is one number for both spins and is compared
        m = {o: np.zeros(p["rho_u"].shape[0], dtype=bool) for o in MGGA_POL_OUTPUTS}
        for o in ("vrho_d", "vgrad_d") + (("vtau_d",) if name.startswith("mgga_x_") else ()):
            m[o] = full.copy()
        return m
    m = {o: np.zeros(p["rho_u"].shape[0], dtype=bool) for o in POL_OUTPUTS}
    for o in ("vrho_d", "vgrad_d", "dvrho_d", "dvgrad_d"):
        m[o] = full.copy()
    if name == "gga_x_g96":
        m["dvgrad_u"] = m["dvgrad_u"] | ((np.abs(p["grho_u"]).sum(0) == 0.0) & live)
        m["dvgrad_d"] = m["dvgrad_d"] | ((np.abs(p["grho_d"]).sum(0) == 0.0) & live)
    return m


def output_class(output):
    """0: e, 1: first order, 2: second order"""
    return 0 if output == "e" else 2 if "dv" in output else 1


def compose_unpol(r, grho, dgrho, absolute=False):
    """rows (10, n): e; e_rho, e_sigma; (H d)_rho, (H d)_sigma; the spin-flip (H d)_rho_u, _sigma_uu, _sigma_ud and e_sigma_uu, e_sigma_ud of
    the polarised form at rho_u = rho_d (grad rho_u = grad rho_d = g / 2, grad d rho_u = -grad d rho_d = dg / 2)"""
    import numpy as np
    if len(r) == 4:  # meta-GGA, first order: e; e_rho, e_sigma, e_tau
        return {"e": r[0], "vrho": r[1], "vgrad": 2.0 * r[2] * (np.abs(grho) if absolute else grho), "vtau": r[3]}
    g, dg, sgn = (np.abs(grho), np.abs(dgrho), 1.0) if absolute else (grho, dgrho, -1.0)
    return {"e": r[0], "vrho": r[1], "vgrad": 2.0 * r[2] * g, "dvrho": r[3], "dvgrad": 2.0 * r[4] * g + 2.0 * r[2] * dg, "t_dvrho": r[5],
            "t_dvgrad": r[6] * g + r[8] * dg + 0.5 * r[7] * g + sgn * 0.5 * r[9] * dg}


def compose_pol(r, gu, gd, dgu, dgd, absolute=False):
    """rows (11, n): e; the gradient by (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd); the Hessian times the response"""
    import numpy as np
    if len(r) == 8:  # meta-GGA, first order: e; the gradient by (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd, tau_u, tau_d)
        if absolute:
            gu, gd = np.abs(gu), np.abs(gd)
        return {"e": r[0], "vrho_u": r[1], "vrho_d": r[2], "vgrad_u": 2.0 * r[3] * gu + r[4] * gd, "vgrad_d": 2.0 * r[5] * gd + r[4] * gu,
                "vtau_u": r[6], "vtau_d": r[7]}
    if absolute:
        gu, gd, dgu, dgd = np.abs(gu), np.abs(gd), np.abs(dgu), np.abs(dgd)
    return {"e": r[0], "vrho_u": r[1], "vrho_d": r[2], "vgrad_u": 2.0 * r[3] * gu + r[4] * gd, "vgrad_d": 2.0 * r[5] * gd + r[4] * gu,
            "dvrho_u": r[6], "dvrho_d": r[7], "dvgrad_u": 2.0 * r[8] * gu + 2.0 * r[3] * dgu + r[9] * gd + r[4] * dgd,
            "dvgrad_d": 2.0 * r[10] * gd + 2.0 * r[5] * dgd + r[9] * gu + r[4] * dgu}


def scaled_error(got, truth, scale, excluded=None):
    """the largest |got - truth| / scale over the points that are compared (scale > 0, not excluded); where the scale is zero (a
    product with a gradient that is exactly zero, a point below the density cutoff) the output has to be exactly zero: else inf"""
    import numpy as np
    got, truth, scale = np.broadcast_arrays(np.asarray(got, dtype=np.float64), truth, scale)
    keep = np.ones(scale.shape, dtype=bool) if excluded is None else ~np.broadcast_to(excluded, scale.shape)
    if not np.all(np.isfinite(got)):
        return np.inf
    if np.any(keep & (scale == 0.0) & (got != 0.0)):
        return np.inf
    m = keep & (scale > 0.0)
    return float((np.abs(got - truth)[m] / scale[m]).max()) if m.any() else 0.0
