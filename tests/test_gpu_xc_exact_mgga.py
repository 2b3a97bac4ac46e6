"""The four meta-GGA functionals of dqc_amd/csrc/xc.hip (mgga_x_scan, mgga_c_scan, mgga_x_tpss, mgga_c_tpss), value and first order,
POINTWISE against the 50-digit reference of oracle/xc_exact.py (fixtures tests/golden/xc_exact_mgga_unpol.npz, xc_exact_mgga_pol.npz
of tools/make_xc_exact_golden.py), through every entry point and instantiation that evaluates them.

Every error is |got - truth| / scale at one point (scale: the sum of the absolute values of the same derivative of the additive
parts of the functional, composed into the scale of an output with the formula of the output).  Tolerance of a (functional, point
class, output class): max(1e-13, 10 x double_err), double_err what the torch-double backend of the REFERENCE attains on the same
formula over the points of that class (recorded in the fixture, never measured on the kernels); for a term list the largest of its
terms.  Point classes: bulk (rho 1e-14 ... 1e4, s 0 and 1e-6 ... 1e2, alpha 0 ... 1e4), the alpha = 1 seam from 1e-14 to 0.1 on both
sides, iso-orbital (tau -> tau_W, and tau < tau_W), the tau floor and tau = 0, zero gradient, the stationary point (s = 0, alpha = 1),
the density cutoff; polarised down to 1 - |zeta| = 1e-10, fully polarised, one electron.  Left out (asserted <= 2 % of the triples by
tests/test_xc_exact_cpu.py): the tight comparison of the empty spin's outputs at fully polarised points (finite, v_rho within
rtol = 1e-5, atol = 1e-7).

Which term list reaches which instantiation of xc_mgga_kernel<EXT, PAIR> (dqc_xc_eval_mgga):
    [mgga_x_scan]                                   <false, 1>      [mgga_x_scan, mgga_c_scan]                  <false, 2>
    the same with a second / in reverse order       <false, 0>      any list with a round-4 (EXT) id, e.g. lda_c_pz   <true, 0>"""
import os

import numpy as np
import pytest
import torch

from oracle import xc_exact as xe

pytestmark = pytest.mark.gpu

FLOOR = (1e-13, 1e-13)  # e, first order: of tests/test_gpu_xc_exact.py
NBULK = 256  # the bulk class comes first in the closed-shell fixture; the kernels are grid-stride loops of 256 threads
LENGTHS = (1, NBULK - 1, NBULK, NBULK + 1)
SCAN1 = [[(1.0, "mgga_x_scan")], [(0.7, "mgga_x_scan")]]                                               # <false, 1>
SCAN2 = [[(1.0, "mgga_x_scan"), (1.0, "mgga_c_scan")], [(0.7, "mgga_x_scan"), (1.3, "mgga_c_scan")]]  # <false, 2>
EXT_LISTS = [[(0.6, "gga_x_b88"), (0.4, "mgga_x_tpss"), (0.9, "mgga_c_tpss"), (0.1, "lda_c_pz")],      # <true>: lda_c_pz is an EXT id
             [(1.0, "mgga_x_scan"), (0.5, "gga_x_pw91")]]                                              # <true>: an EXT GGA
HALVES = {"vrho_u": "vrho", "vrho_d": "vrho", "vgrad_u": "vgrad", "vgrad_d": "vgrad", "vtau_u": "vtau", "vtau_d": "vtau"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


class Fixture:
    def __init__(self, golden_dir, kind):
        self.kind = kind
        self.f = np.load(os.path.join(golden_dir, "xc_exact_mgga_%s.npz" % kind))
        self.p = {k[2:]: self.f[k] for k in self.f.files if k.startswith("p_")}
        self.cls, self.classes = self.p["cls"], [str(c) for c in self.f["classes"]]
        self.n = self.cls.shape[0]
        self._memo = {}

    def compose(self, rows, absolute=False):
        p = self.p
        if self.kind == "unpol":
            return xe.compose_unpol(rows, p["grho"], None, absolute)
        return xe.compose_pol(rows, p["grho_u"], p["grho_d"], None, None, absolute)

    def excluded(self, name):
        """the empty spin at fully polarised points (for an LDA / GGA term of a list: the same rule)"""
        if self.kind == "unpol":
            return xe.unpol_excluded("mgga_c_scan", self.p)
        m = xe.pol_excluded(name if name in xe.MGGA_FUNCS else "mgga_x_scan", self.p)
        return m

    def ref(self, name):
        """truth, scale and exclusion masks of every output of one functional"""
        if name not in self._memo:
            v = self.f[name + "_val"]
            self._memo[name] = (self.compose(v[0]), self.compose(v[1], absolute=True), self.excluded(name))
        return self._memo[name]

    def ref_terms(self, terms):
        """the weighted sum of the truths of a term list, the weighted sum of the scales, the union of the exclusions"""
        truth = scale = exc = None
        for c, nm in terms:
            t, s, x = self.ref(nm)
            truth = {o: c * t[o] for o in t} if truth is None else {o: truth[o] + c * t[o] for o in t}
            scale = {o: abs(c) * s[o] for o in s} if scale is None else {o: scale[o] + abs(c) * s[o] for o in s}
            exc = dict(x) if exc is None else {o: exc[o] | x[o] for o in x}
        return truth, scale, exc

    def tol(self, terms, c, k):
        return max(FLOOR[k], 10.0 * max(float(self.f[nm + "_double_err"][c, k]) for _, nm in terms))

    def dead(self):
        p = self.p
        return ~((p["rho"] if self.kind == "unpol" else p["rho_u"] + p["rho_d"]) > xe.DENS_THRESHOLD)


@pytest.fixture(scope="module")
def fxu(golden_dir):
    return Fixture(golden_dir, "unpol")


@pytest.fixture(scope="module")
def fxp(golden_dir):
    return Fixture(golden_dir, "pol")


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _label(terms):
    return "+".join(("" if c == 1.0 else "%g*" % c) + nm for c, nm in terms)


def _check(fx, entry, terms, got, rename=None):
    """compare the outputs `got` {output: array or None} of one entry point with the reference of the term list, class by class;
    points below the density cutoff are exactly zero in every output"""
    truth, scale, exc = fx.ref_terms(terms)
    dead, failed = fx.dead(), []
    for o, g in got.items():
        if g is not None:
            r = (rename or {}).get(o, o)
            assert g.shape == truth[r].shape and np.all(g[..., dead] == 0.0), "%s %s %s: not exactly zero below the cutoff" % (entry, _label(terms), o)
    for c, cn in enumerate(fx.classes):
        worst = [0.0, 0.0]
        for o, g in got.items():
            if g is None:
                continue
            r = (rename or {}).get(o, o)
            k = xe.output_class(r)
            err = xe.scaled_error(g, truth[r], scale[r], exc[r] | (fx.cls != c))
            worst[k] = max(worst[k], err)
            if not err < fx.tol(terms, c, k):
                failed.append("%s %s %.2e >= %.2e" % (cn, o, err, fx.tol(terms, c, k)))
        print("XCEXACT-MGGA | %-26s | %-50s | %-15s | %s | %s" % (entry, _label(terms), cn, " | ".join("%.1e" % w for w in worst),
                                                                   " | ".join("%.1e" % fx.tol(terms, c, k) for k in range(2))))
    assert not failed, "%s %s: %s" % (entry, _label(terms), "; ".join(failed))


def _flat(out):
    res = []
    for o in out:
        res += list(o) if isinstance(o, tuple) else [o]
    return res


def _prefix_equal(full, part, n, what):
    """the outputs at a point do not depend on the length of the arrays"""
    for a, b in zip(_flat(full), _flat(part)):
        assert torch.equal(a[..., :n], b), "%s: the first %d points differ from the run over all points" % (what, n)


def _wants(fn, args, full, what):
    """want_e=False / want_v=False: what is asked for is bit-equal to the full call, the rest is None"""
    full = _flat(full)
    only_e, only_v = _flat(fn(*args, want_v=False)), _flat(fn(*args, want_e=False))
    assert torch.equal(only_e[0], full[0]) and all(a is None for a in only_e[1:]), what + ": want_v=False"
    assert only_v[0] is None and all(torch.equal(a, b) for a, b in zip(only_v[1:], full[1:])), what + ": want_e=False"


def _t(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


# ------------------------------------------------------------------------------------------------ closed shell: dqc_xc_eval_mgga
def _eval_unpol(dev, fx, terms):
    from dqc_amd import lib
    rho, grho, tau = _t(dev, fx.p["rho"]), _t(dev, fx.p["grho"]), _t(dev, fx.p["tau"])
    full = lib.xc_eval_mgga(terms, rho, grho, tau)
    for n in LENGTHS:
        _prefix_equal(full, lib.xc_eval_mgga(terms, rho[:n].contiguous(), grho[:, :n].contiguous(), tau[:n].contiguous()), n,
                      "xc_eval_mgga " + _label(terms))
    _wants(lib.xc_eval_mgga, (terms, rho, grho, tau), full, "xc_eval_mgga " + _label(terms))
    _check(fx, "xc_eval_mgga", terms, dict(zip(xe.MGGA_UNPOL_OUTPUTS, map(_np, full))))
    return full


@pytest.mark.parametrize("name", xe.MGGA_NAMES)
def test_xc_eval_mgga_single_functional(dev, fxu, name):
    """mgga_x_scan alone is the instantiation <false, 1>, each of the others alone the generic <false, 0>"""
    _eval_unpol(dev, fxu, [(1.0, name)])


@pytest.mark.parametrize("terms", SCAN1[1:] + SCAN2, ids=_label)
def test_xc_eval_mgga_fixed_instantiations(dev, fxu, terms):
    """<false, 1> with a coefficient, <false, 2> with unit and with other coefficients"""
    _eval_unpol(dev, fxu, terms)


@pytest.mark.parametrize("fixed", SCAN1 + SCAN2, ids=_label)
def test_xc_eval_mgga_generic_agrees_with_the_fixed_instantiations(dev, fxu, fixed):
    """the same functional through the generic <false, 0>: the pair in reverse order, the single term with a second term of
    coefficient zero; against the truth, and against the fixed instantiation within the same tolerance"""
    generic = fixed[::-1] if len(fixed) == 2 else fixed + [(0.0, "mgga_x_tpss")]
    a, b = _eval_unpol(dev, fxu, fixed), _eval_unpol(dev, fxu, generic)
    _, scale, _ = fxu.ref_terms(fixed)
    for o, x, y in zip(xe.MGGA_UNPOL_OUTPUTS, map(_np, a), map(_np, b)):
        k = xe.output_class(o)
        for c in range(len(fxu.classes)):
            err = xe.scaled_error(x, y, scale[o], fxu.cls != c)
            assert err < fxu.tol(fixed, c, k), (o, fxu.classes[c], err)


@pytest.mark.parametrize("terms", EXT_LISTS, ids=_label)
def test_xc_eval_mgga_ext_lists(dev, fxu, terms):
    """<true>: meta-GGA, GGA and LDA terms in one list; the truth of the list is the weighted sum of the truths"""
    _eval_unpol(dev, fxu, terms)


# ------------------------------------------------------------------------------------------------ polarised correlation kernels
def _empty_spin(fx, terms, got):
    """fully polarised points: the outputs of the empty spin are finite, its v_rho close to the reference at libxc's thresholds"""
    full = (fx.p["rho_d"] == 0.0) & ~fx.dead()
    truth = fx.ref_terms(terms)[0]
    for o in ("vrho_d", "vgrad_d", "vtau_d"):
        assert np.all(np.isfinite(got[o][..., full])), o
    assert np.allclose(got["vrho_d"][full], truth["vrho_d"][full], rtol=1e-5, atol=1e-7)


def _pol_outputs(out, shared_grad):
    e, (vu, vd), vg, vt = out
    gu, gd = (vg, vg) if shared_grad else vg
    return dict(zip(xe.MGGA_POL_OUTPUTS, map(_np, (e, vu, vd, gu, gd, vt, vt))))


def _eval_pol(dev, fxp, fxu, fn, entry, terms, shared_grad):
    p = fxp.p
    args = (terms,) + tuple(_t(dev, p[k]) for k in ("rho_u", "rho_d", "grho_u", "grho_d", "tau_u", "tau_d"))
    full = fn(*args)
    _wants(fn, args, full, entry + " " + _label(terms))
    got = _pol_outputs(full, shared_grad)
    _check(fxp, entry, terms, got)
    _empty_spin(fxp, terms, got)
    # the closed-shell points as rho / 2, grad rho / 2, tau / 2 per spin: the unpolarised truth
    q = fxu.p
    rho, grho, tau = _t(dev, 0.5 * q["rho"]), _t(dev, 0.5 * q["grho"]), _t(dev, 0.5 * q["tau"])
    full = fn(terms, rho, rho, grho, grho, tau, tau)
    for n in LENGTHS:
        rn, gn, tn = rho[:n].contiguous(), grho[:, :n].contiguous(), tau[:n].contiguous()
        _prefix_equal(full, fn(terms, rn, rn, gn, gn, tn, tn), n, entry + " " + _label(terms))
    _check(fxu, entry + " (rho / 2)", terms, _pol_outputs(full, shared_grad), rename=HALVES)


@pytest.mark.parametrize("terms", [[(1.0, "mgga_c_scan")], [(0.7, "mgga_c_scan")]], ids=_label)
def test_xc_eval_mgga_pol(dev, fxp, fxu, terms):
    from dqc_amd import lib
    _eval_pol(dev, fxp, fxu, lib.xc_eval_mgga_pol, "xc_eval_mgga_pol", terms, True)


@pytest.mark.parametrize("terms", [[(1.0, "mgga_c_scan")], [(1.0, "mgga_c_tpss")], [(0.7, "mgga_c_scan"), (1.3, "mgga_c_tpss")]], ids=_label)
def test_xc_eval_mgga_pol2(dev, fxp, fxu, terms):
    from dqc_amd import lib
    _eval_pol(dev, fxp, fxu, lib.xc_eval_mgga_pol2, "xc_eval_mgga_pol2", terms, False)


# ------------------------------------------------------------------------------------------------ the public polarised path
@pytest.mark.parametrize("xcstr", ["mgga_x_scan", "mgga_x_tpss", "mgga_x_tpss+mgga_c_tpss+0.3*gga_c_pbe"])
def test_polarised_meta_gga_through_get_xc(dev, fxp, xcstr):
    """dqc_amd.xc.LibXC._pol_mgga through get_edensityxc / get_vxc: the only place where the spin-scaled exchange (the closed-shell
    kernel at 2 rho_s), the polarised correlation kernel and the polarised LDA / GGA kernel are summed"""
    from dqc_amd.utils.datastruct import SpinParam, ValGrad
    from dqc_amd.xc import get_xc
    xc = get_xc(xcstr)
    p = fxp.p
    dens = SpinParam(u=ValGrad(value=_t(dev, p["rho_u"]), grad=_t(dev, p["grho_u"]), lapl=None, kin=_t(dev, p["tau_u"])),
                     d=ValGrad(value=_t(dev, p["rho_d"]), grad=_t(dev, p["grho_d"]), lapl=None, kin=_t(dev, p["tau_d"])))
    e, v = xc.get_edensityxc(dens), xc.get_vxc(dens)
    got = dict(zip(xe.MGGA_POL_OUTPUTS, map(_np, (e, v.u.value, v.d.value, v.u.grad, v.d.grad, v.u.kin, v.d.kin))))
    _check(fxp, "get_xc (polarised)", xc.terms, got)
    _empty_spin(fxp, xc.terms, got)
