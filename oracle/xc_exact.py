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
"""
from fractions import Fraction as Fr

import mpmath as mp

NAMES = ["lda_x", "lda_c_pw", "lda_c_pw_mod", "lda_c_vwn", "lda_c_pz", "gga_x_pbe", "gga_x_pbe_r", "gga_x_pbe_sol", "gga_x_rpbe",
         "gga_c_pbe", "gga_c_pbe_sol", "gga_x_b88", "gga_c_lyp", "gga_c_p86", "gga_x_pw91", "gga_x_b86", "gga_x_g96", "gga_x_pw86",
         "gga_x_optx", "gga_x_wc"]
DPS = 50
DENS_THRESHOLD, ZETA_THRESHOLD, TINY_S = 1e-15, 1e-10, 1e-30


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


FUNCS = {n: globals()[n] for n in NAMES}
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


def effective_point(ru, rd, suu, sud, sdd):
    """the point the functional is evaluated at, the offset of zeta, the digits to carry and the variables that stand for a zero: libxc's thresholds (see the module
    docstring), exact zero gradients replaced by a reduced gradient of TINY_S.  Exact arithmetic on the doubles given; None below
    the density cutoff."""
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


def unpolarised(rho, sigma):
    """the unpolarised form is the polarised form at rho_u = rho_d = rho / 2, sigma_uu = sigma_ud = sigma_dd = sigma / 4"""
    return 0.5 * rho, 0.5 * rho, 0.25 * sigma, 0.25 * sigma, 0.25 * sigma


def effective_point_unpol(rho, sigma):
    """(rho, sigma) of a closed-shell point with the same conventions; None below the density cutoff"""
    mp.mp.dps = 4 * DPS
    rho, sigma = mp.mpf(float(rho)), mp.mpf(float(sigma))
    if not (float(rho) > DENS_THRESHOLD):
        return None
    zero = [1] if sigma == 0 else []
    if sigma == 0:
        sigma = mp.mpf(TINY_S) ** 2 * 4 * mp.power(rho / 2, mp.mpf(8) / 3)
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
    if len(x) == 2:
        return [abs(x[0]), abs(x[1])]
    return [abs(x[0]), abs(x[1]), abs(x[2]), abs(x[2]) + abs(x[4]), abs(x[4])]


def _shift(x, k, h):
    y = list(x)
    y[k] = y[k] + h
    return y


def _re(v):
    return v.real if isinstance(v, mp.mpc) else v


def _embed(y):
    return y if len(y) == 5 else unpolarised(y[0], y[1])


def mp_eval(name, x, dz, delta=None, h_rel=H_REL, variables=None, dps=DPS, number=float, zero=()):
    """truth and scale of e, of every first derivative (by the variables listed) and of the product of the Hessian with `delta`
    (one component per variable, or None) at x = (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd) or the closed-shell (rho, sigma)
    -> {"e": (truth, scale), "d1": {k: (truth, scale)}, "d2": {k: (truth, scale)}} as floats (number=mp.mpf: as they are); mpmath central
    differences of every part at once"""
    ns = MP(max(dps, DPS + 30))
    f = FUNCS[name]
    variables = range(len(x)) if variables is None else variables

    def parts(y):
        return [_re(p) for p in f(ns, *_embed(y), dz)]

    def combine(vals):
        return number(mp.fsum(vals)), number(mp.fsum(abs(v) for v in vals))

    st = _steps(x)
    out = {"e": combine(parts(x)), "d1": {}, "d2": {}}
    # a variable that stands for an exact zero is TINY_S^2 of its natural size, and the truth there is TINY_S from the limit
    floor = [mp.mpf(TINY_S ** 3 if k in zero else SCALE_FLOOR) * out["e"][1] for k in range(len(x))]

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
    parts = FUNCS[name](ns, *_embed(xs), dzt)
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


def unpol_excluded(name, p):
    """{output: bool mask over the points} of what a comparison leaves out (p: rho, grho): the d v_grad of gga_x_g96 where grad rho
    is exactly zero -- its v_sigma ~ sigma^(-1/4) does not exist there (v_grad itself is compared, and is 0)"""
    import numpy as np
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
    g, dg, sgn = (np.abs(grho), np.abs(dgrho), 1.0) if absolute else (grho, dgrho, -1.0)
    return {"e": r[0], "vrho": r[1], "vgrad": 2.0 * r[2] * g, "dvrho": r[3], "dvgrad": 2.0 * r[4] * g + 2.0 * r[2] * dg, "t_dvrho": r[5],
            "t_dvgrad": r[6] * g + r[8] * dg + 0.5 * r[7] * g + sgn * 0.5 * r[9] * dg}


def compose_pol(r, gu, gd, dgu, dgd, absolute=False):
    """rows (11, n): e; the gradient by (rho_u, rho_d, sigma_uu, sigma_ud, sigma_dd); the Hessian times the response"""
    import numpy as np
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
