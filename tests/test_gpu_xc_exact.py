"""The LDA / GGA functional kernels of dqc_amd/csrc/xc.hip, first and second order, POINTWISE against the 50-digit reference of
oracle/xc_exact.py (fixtures tests/golden/xc_exact_unpol.npz, xc_exact_pol.npz of tools/make_xc_exact_golden.py).

Every error is |got - truth| / scale at one point, scale = sum of the absolute values of the same derivative of the additive parts
of the functional (composed into the scale of an output with the formula of the output): a wrong digit in the density tail or at
the nuclei weighs as much as one at the largest value.  Tolerance of a functional and output class (e, first order, second order):
max(floor, 10 x double_err) with floor = 1e-13, 1e-13, 1e-12 and double_err what the torch-double backend of the REFERENCE attains
on the same formula (recorded in the fixture, never measured on the kernels); 10 is the standing margin over a recorded estimate
(tests/test_gpu_orb_hessian.py), here for another libm and another order of the operations.  Each functional is tested alone.

Range: rho in [1e-14, 1e4], s in [1e-6, 1e2] and grad rho = 0 (bulk), both sides of r_s = 1, of the x asinh x series switch and of the
density cutoff; polarised 1 - |zeta| down to 1e-8, zeta = 0, parallel / antiparallel / orthogonal / vanishing spin gradients, fully
polarised points.  Left out (<= 2 % of the (functional, point, output) triples, asserted by tests/test_xc_exact_cpu.py): the
d v_grad of gga_x_g96 where the gradient of the spin is exactly zero, the tight comparison of the empty spin's outputs at fully
polarised points (finite, v_rho within rtol = 1e-5, atol = 1e-7)."""
import os

import numpy as np
import pytest
import torch

from oracle import xc_exact as xe

pytestmark = pytest.mark.gpu

NAMES = xe.NAMES
FLOOR = (1e-13, 1e-13, 1e-12)
NBULK = 256  # the bulk class comes first in the closed-shell fixture; the kernels are grid-stride loops of 256 threads
LENGTHS = (1, NBULK - 1, NBULK, NBULK + 1)
PAIRS = [[(0.7, "gga_x_pbe"), (1.3, "gga_c_pbe")], [(0.7, "lda_x"), (1.3, "lda_c_pw")]]
MIXED = [(0.6, "gga_x_b88"), (0.4, "gga_x_pw91"), (0.9, "gga_c_lyp"), (0.1, "lda_c_pz")]  # EXT and non-EXT terms in one list
LISTS = PAIRS + [MIXED]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


class Fixture:
    def __init__(self, golden_dir, kind):
        self.kind = kind
        self.f = np.load(os.path.join(golden_dir, "xc_exact_%s.npz" % kind))
        self.p = {k[2:]: self.f[k] for k in self.f.files if k.startswith("p_")}
        self.n = self.p["cls"].shape[0]
        self._memo = {}

    def compose(self, rows, absolute=False):
        p = self.p
        if self.kind == "unpol":
            return xe.compose_unpol(rows, p["grho"], p["dgrho"], absolute)
        return xe.compose_pol(rows, p["grho_u"], p["grho_d"], p["dgrho_u"], p["dgrho_d"], absolute)

    def ref(self, name):
        """truth, scale and exclusion masks of every output of one functional"""
        if name not in self._memo:
            v = self.f[name + "_val"]
            exc = (xe.unpol_excluded if self.kind == "unpol" else xe.pol_excluded)(name, self.p)
            self._memo[name] = (self.compose(v[0]), self.compose(v[1], absolute=True), exc)
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

    def tol(self, terms, cls):
        return max(FLOOR[cls], 10.0 * max(float(self.f[nm + "_double_err"][cls]) for _, nm in terms))

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
    return "+".join(nm for _, nm in terms)


def _check(fx, entry, terms, got, rename=None):
    """compare the outputs `got` {output: array or None} of one entry point with the reference of the term list; points below the
    density cutoff are exactly zero in every output"""
    truth, scale, exc = fx.ref_terms(terms)
    dead, worst, failed = fx.dead(), [0.0, 0.0, 0.0], []
    for o, g in got.items():
        if g is None:
            continue
        r = (rename or {}).get(o, o)
        c = xe.output_class(r)
        assert g.shape == truth[r].shape and np.all(g[..., dead] == 0.0), "%s %s %s: not exactly zero below the cutoff" % (entry, _label(terms), o)
        err = xe.scaled_error(g, truth[r], scale[r], exc[r])
        worst[c] = max(worst[c], err)
        if not err < fx.tol(terms, c):
            failed.append("%s %.2e >= %.2e" % (o, err, fx.tol(terms, c)))
    print("XCEXACT | %-22s | %-24s | %s | %s" % (entry, _label(terms), " | ".join("%.1e" % w for w in worst),
                                                   " | ".join("%.1e" % fx.tol(terms, c) for c in range(3))))
    assert not failed, "%s %s: %s" % (entry, _label(terms), "; ".join(failed))


def _prefix_equal(full, part, n, what):
    """the outputs at a point do not depend on the length of the arrays"""
    for a, b in zip(full, part):
        if a is None:
            assert b is None
            continue
        assert torch.equal(a[..., :n], b), "%s: the first %d points differ from the run over all points" % (what, n)


def _flat(out):
    res = []
    for o in out:
        res += list(o) if isinstance(o, tuple) else [o]
    return res


def _gga(terms):
    return any(xe.IS_GGA[nm] for _, nm in terms)


# ------------------------------------------------------------------------------------------------ first order, closed shell
def _eval_unpol(dev, fx, terms):
    from dqc_amd import lib
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    gga = _gga(terms)
    rho, grho = t(fx.p["rho"]), t(fx.p["grho"])
    full = lib.xc_eval(terms, rho, grho if gga else None)
    for n in LENGTHS:
        _prefix_equal(full, lib.xc_eval(terms, rho[:n].contiguous(), grho[:, :n].contiguous() if gga else None), n, "xc_eval " + _label(terms))
    _check(fx, "xc_eval", terms, dict(zip(("e", "vrho", "vgrad"), map(_np, full))))
    # the quadrature epilogue must not touch the potentials
    w = t(np.linspace(0.5, 1.5, fx.n))
    _, v, vg = lib.xc_eval_quad(terms, rho, grho if gga else None, w)
    assert torch.equal(v, full[1]) and (vg is None if full[2] is None else torch.equal(vg, full[2])), "xc_eval_quad " + _label(terms)


@pytest.mark.parametrize("name", NAMES)
def test_xc_eval_single_functional(dev, fxu, name):
    _eval_unpol(dev, fxu, [(1.0, name)])


@pytest.mark.parametrize("terms", LISTS, ids=_label)
def test_xc_eval_term_lists(dev, fxu, terms):
    """the PBE and LDA pairs select the PAIR kernels, the mixed list the EXT kernel with terms of both kinds"""
    _eval_unpol(dev, fxu, terms)


# ------------------------------------------------------------------------------------------------ first order, polarised
HALVES = {"vrho_u": "vrho", "vrho_d": "vrho", "vgrad_u": "vgrad", "vgrad_d": "vgrad", "dvrho_u": "dvrho", "dvrho_d": "dvrho",
          "dvgrad_u": "dvgrad", "dvgrad_d": "dvgrad"}


def _empty_spin(fx, terms, got):
    """fully polarised points: the outputs of the empty spin are finite, its v_rho close to the reference at libxc's thresholds"""
    full = (fx.p["rho_d"] == 0.0) & ~fx.dead()
    truth = fx.ref_terms(terms)[0]
    for o in ("vrho_d", "vgrad_d", "dvrho_d", "dvgrad_d"):
        if got.get(o) is not None:
            assert np.all(np.isfinite(got[o][..., full])), o
    if got.get("vrho_d") is not None:
        assert np.allclose(got["vrho_d"][full], truth["vrho_d"][full], rtol=1e-5, atol=1e-7)


def _eval_pol(dev, fxp, fxu, terms):
    from dqc_amd import lib
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    gga = _gga(terms)
    g = (lambda a: t(a)) if gga else (lambda a: None)
    p = fxp.p
    e, (vu, vd), (gu, gd) = lib.xc_eval_pol(terms, t(p["rho_u"]), t(p["rho_d"]), g(p["grho_u"]), g(p["grho_d"]))
    got = dict(zip(("e", "vrho_u", "vrho_d", "vgrad_u", "vgrad_d"), map(_np, (e, vu, vd, gu, gd))))
    _check(fxp, "xc_eval_pol", terms, got)
    _empty_spin(fxp, terms, got)
    # the closed-shell points as rho / 2, grad rho / 2 per spin
    rho, grho = t(0.5 * fxu.p["rho"]), g(0.5 * fxu.p["grho"])
    full = lib.xc_eval_pol(terms, rho, rho, grho, grho)
    for n in LENGTHS:
        gn = grho[:, :n].contiguous() if gga else None
        _prefix_equal(_flat(full), _flat(lib.xc_eval_pol(terms, rho[:n].contiguous(), rho[:n].contiguous(), gn, gn)), n,
                      "xc_eval_pol " + _label(terms))
    got = dict(zip(("e", "vrho_u", "vrho_d", "vgrad_u", "vgrad_d"), map(_np, _flat(full))))
    _check(fxu, "xc_eval_pol (rho / 2)", terms, got, rename=HALVES)


@pytest.mark.parametrize("name", NAMES)
def test_xc_eval_pol_single_functional(dev, fxp, fxu, name):
    _eval_pol(dev, fxp, fxu, [(1.0, name)])


def test_xc_eval_pol_pbe_pair(dev, fxp, fxu):
    _eval_pol(dev, fxp, fxu, PAIRS[0])


# ------------------------------------------------------------------------------------------------ second order
@pytest.mark.parametrize("name", NAMES)
def test_xc_eval_fxc_single_functional(dev, fxu, name):
    from dqc_amd import lib
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    terms, gga, p = [(1.0, name)], xe.IS_GGA[name], fxu.p
    rho, grho, drho, dgrho = t(p["rho"]), t(p["grho"]), t(p["drho"]), t(p["dgrho"])
    for entry, fn, outs in (("xc_eval_fxc", lib.xc_eval_fxc, ("dvrho", "dvgrad")), ("xc_eval_fxc_triplet", lib.xc_eval_fxc_triplet, ("t_dvrho", "t_dvgrad"))):
        dv, dvg = fn(terms, rho, grho if gga else None, drho[None], dgrho[None] if gga else None)
        assert (dvg is None) == (not gga)
        for n in LENGTHS:
            pv, pg = fn(terms, rho[:n].contiguous(), grho[:, :n].contiguous() if gga else None, drho[None, :n].contiguous(),
                        dgrho[None, :, :n].contiguous() if gga else None)
            _prefix_equal((dv, dvg), (pv, pg), n, entry + " " + name)
        _check(fxu, entry, terms, {outs[0]: _np(dv[0]), outs[1]: None if dvg is None else _np(dvg[0])})


@pytest.mark.parametrize("name", NAMES)
def test_xc_eval_fxc_pol_single_functional(dev, fxp, fxu, name):
    from dqc_amd import lib
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    terms, gga, p = [(1.0, name)], xe.IS_GGA[name], fxp.p
    g = (lambda a: t(a)) if gga else (lambda a: None)
    (dvu, dvd), (dgu, dgd) = lib.xc_eval_fxc_pol(terms, t(p["rho_u"]), t(p["rho_d"]), g(p["grho_u"]), g(p["grho_d"]), t(p["drho_u"][None]),
                                                 t(p["drho_d"][None]), g(p["dgrho_u"][None]), g(p["dgrho_d"][None]))
    got = {"dvrho_u": _np(dvu[0]), "dvrho_d": _np(dvd[0]), "dvgrad_u": None if dgu is None else _np(dgu[0]),
           "dvgrad_d": None if dgd is None else _np(dgd[0])}
    _check(fxp, "xc_eval_fxc_pol", terms, got)
    _empty_spin(fxp, terms, got)
    # the closed-shell points with the response split evenly: both spins see the restricted response
    q = fxu.p
    rho, grho, drho, dgrho = t(0.5 * q["rho"]), g(0.5 * q["grho"]), t(0.5 * q["drho"][None]), g(0.5 * q["dgrho"][None])
    full = lib.xc_eval_fxc_pol(terms, rho, rho, grho, grho, drho, drho, dgrho, dgrho)
    for n in LENGTHS:
        gn, dn = (grho[:, :n].contiguous(), dgrho[:, :, :n].contiguous()) if gga else (None, None)
        rn, vn = rho[:n].contiguous(), drho[:, :n].contiguous()
        _prefix_equal(_flat(full), _flat(lib.xc_eval_fxc_pol(terms, rn, rn, gn, gn, vn, vn, dn, dn)), n, "xc_eval_fxc_pol " + name)
    got = dict(zip(("dvrho_u", "dvrho_d", "dvgrad_u", "dvgrad_d"), (None if a is None else _np(a[0]) for a in _flat(full))))
    _check(fxu, "xc_eval_fxc_pol (rho / 2)", terms, got, rename=HALVES)
