"""The third-order functional kernel dqc_xc_eval_kxc (dqc_amd/csrc/xc.hip, restricted closed shell): the second-order change of
(v_rho, 2 v_sigma grad rho) under two responses.

POINTWISE against the reference of oracle/xc_exact.py (fixture tests/golden/xc_kxc_exact_unpol.npz of tools/make_xc_kxc_golden.py:
mpmath third differences carried at >= 120 digits), all 20 LDA / GGA functionals on the closed-shell point set of the first- and
second-order fixture.  Error: |kernel - truth| / scale at one point, scale = the sum of the absolute values of the additive parts.
Bar per functional, output and point class: max(1e-11, 10 x what torch float64 triple autograd attains on the same formula, recorded
in the fixture) -- 1e-11 continues the floors 1e-13 (first order) and 1e-12 (second order) of tests/test_gpu_xc_exact.py, 10 is the
standing margin over a recorded estimate.  Left out: gga_x_g96 where grad rho is exactly zero (its v_sigma ~ sigma^(-1/4) does not exist
there; at this order it is in d2vrho too, as (d v_sigma / d rho) d2 sigma), and nothing else.

Against the parent's kernel: d2v = the Richardson central difference of lib.xc_eval_fxc(.., d rho_1) under rho -> rho +- t d rho_2.
Structure: symmetry in the two responses, term lists, npair, the density cutoff, the grid-stride tail.  Gates: no launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import xc_exact as xe

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_xc_kxc_golden as kg  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = xe.NAMES
CLASSES = ("bulk", "r_s = 1", "x asinh x (b88)", "x asinh x (pw91)", "above the cutoff", "below the cutoff")
FD_LISTS = [[(1.0, "lda_x"), (1.0, "lda_c_pw")], [(1.0, "gga_x_pbe"), (1.0, "gga_c_pbe")], [(0.72, "gga_x_b88"), (0.81, "gga_c_lyp")],
            [(1.0, "gga_x_pw86")]]
MIXED = [(0.6, "gga_x_b88"), (0.4, "gga_x_pw91")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


@pytest.fixture(scope="module")
def fx(golden_dir):
    f = np.load(os.path.join(golden_dir, "xc_kxc_exact_unpol.npz"))
    return f, {k[2:]: f[k] for k in f.files if k.startswith("p_")}


def _t(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def _inputs(dev, p, gga, sel=slice(None)):
    """rho, grho, (drho1, dgrho1), (drho2, dgrho2) with npair = 1"""
    g = (lambda a: _t(dev, a[:, sel])) if gga else (lambda a: None)
    g1 = (lambda a: _t(dev, a[:, sel])[None]) if gga else (lambda a: None)
    return (_t(dev, p["rho"][sel]), g(p["grho"]), _t(dev, p["drho"][sel])[None], g1(p["dgrho"]), _t(dev, p["drho2"][sel])[None],
            g1(p["dgrho2"]))


def _kxc(terms, rho, grho, dr1, dg1, dr2, dg2):
    from dqc_amd import lib
    return lib.xc_eval_kxc(terms, rho, grho, dr1, dg1, dr2, dg2)


@pytest.mark.parametrize("name", NAMES)
def test_kxc_pointwise_against_the_reference(dev, fx, name):
    f, p = fx
    gga = xe.IS_GGA[name]
    d2v, d2vg = _kxc([(1.0, name)], *_inputs(dev, p, gga))
    got = {"d2vrho": d2v[0].cpu().numpy(), "d2vgrad": d2vg[0].cpu().numpy() if gga else None}
    val = f[name + "_val"]
    truth, scale, exc = kg.compose_kxc(val[0], p), kg.compose_kxc(val[1], p, absolute=True), kg.excluded(name, p)
    dead = ~(p["rho"] > xe.DENS_THRESHOLD)
    zero_g = (np.abs(p["grho"]).sum(0) == 0.0) & ~dead
    nexc = sum(int(m.sum()) for m in exc.values())
    # left out: gga_x_g96 at the 32 live points whose gradient is exactly zero, both outputs; nothing else
    assert nexc == (2 * int(zero_g.sum()) if name == "gga_x_g96" else 0) and (name != "gga_x_g96" or nexc == 64)
    failed = []
    for j, o in enumerate(kg.OUTPUTS):
        if got[o] is None:
            continue
        assert np.all(got[o][..., dead] == 0.0) and not np.any(np.signbit(got[o][..., dead])), "%s %s: not +0.0 below the cutoff" % (name, o)
        for c, label in enumerate(CLASSES):
            bar = max(kg.FLOOR, 10.0 * float(f[name + "_double_err"][j, c]))
            err = xe.scaled_error(got[o], truth[o], scale[o], exc[o] | (p["cls"] != c))
            print("KXC | %-14s | %-7s | %-18s | err %.1e | bar %.1e | torch-double %.1e" % (name, o, label, err, bar,
                                                                                         float(f[name + "_double_err"][j, c])))
            if not err < bar:
                failed.append("%s, %s: %.2e >= %.2e" % (o, label, err, bar))
    assert not failed, "%s: %s" % (name, "; ".join(failed))


@pytest.mark.parametrize("terms", FD_LISTS, ids=lambda t: "+".join(n for _, n in t))
def test_kxc_is_the_derivative_of_the_second_order_kernel(dev, fx, terms):
    """d2v[d rho_1, d rho_2] = d/dt f_xc[rho + t d rho_2] . d rho_1 at t = 0: Richardson (4 FD(t) - FD(2t)) / 3 of the parent's
    kernel on the bulk points whose gradient is not zero; bound 10 |FD(t) - FD(2t)| + 1e-9 x scale"""
    from dqc_amd import lib
    f, p = fx
    gga = any(xe.IS_GGA[n] for _, n in terms)
    # (where |grad rho| < 1e-3 rho the fixture's grad d rho is far above grad rho: a step of t would leave the neighbourhood)
    sel = np.where((p["cls"] == 0) & (np.linalg.norm(p["grho"], axis=0) >= 1e-3 * p["rho"]))[0]
    assert sel.size >= 32
    rho, grho, dr1, dg1, dr2, dg2 = _inputs(dev, p, gga, sel)
    got = _kxc(terms, rho, grho, dr1, dg1, dr2, dg2)

    def fd(t):
        hi = lib.xc_eval_fxc(terms, rho + t * dr2[0], grho + t * dg2[0] if gga else None, dr1, dg1)
        lo = lib.xc_eval_fxc(terms, rho - t * dr2[0], grho - t * dg2[0] if gga else None, dr1, dg1)
        return [None if a is None else (a - b) / (2.0 * t) for a, b in zip(hi, lo)]

    t = 1e-3  # the responses are up to 30 % of the ground state: rho moves by 3e-4 of itself
    f1, f2 = fd(t), fd(2.0 * t)
    sub = {k: v[..., sel] for k, v in p.items()}
    for o, g, a, b in zip(kg.OUTPUTS, got, f1, f2):
        if g is None:
            continue
        scale = sum(abs(c) * kg.compose_kxc(f[n + "_val"][1][:, sel], sub, absolute=True)[o] for c, n in terms)
        rich = (4.0 * a - b) / 3.0
        miss = ((g - rich).abs() - 10.0 * (a - b).abs() - 1e-9 * _t(dev, scale)).max()
        print("KXC-FD | %-22s | %-7s | max |kxc - Richardson| / scale %.1e | max |FD(t) - FD(2t)| / scale %.1e"
              % ("+".join(n for _, n in terms), o, float(((g - rich).abs() / _t(dev, scale)).max()), float(((a - b).abs() / _t(dev, scale)).max())))
        assert float(miss) <= 0.0, "%s %s: off the finite difference of xc_eval_fxc by %.2e beyond the bound" % (terms, o, float(miss))


def test_kxc_structure(dev, fx):
    f, p = fx
    for terms in ([(1.0, "lda_c_vwn")], [(0.7, "gga_x_pbe"), (1.3, "gga_c_pbe")], MIXED):
        gga = any(xe.IS_GGA[n] for _, n in terms)
        rho, grho, dr1, dg1, dr2, dg2 = _inputs(dev, p, gga)
        full = _kxc(terms, rho, grho, dr1, dg1, dr2, dg2)
        swap = _kxc(terms, rho, grho, dr2, dg2, dr1, dg1)
        parts = [_kxc([tm], rho, grho, dr1, dg1, dr2, dg2) for tm in terms]
        for k, o in enumerate(kg.OUTPUTS):
            if full[k] is None:
                assert not gga
                continue
            scale = _t(dev, sum(abs(c) * kg.compose_kxc(f[n + "_val"][1], p, absolute=True)[o] for c, n in terms))
            ulp = 2.220446049250313e-16 * scale
            assert bool(((full[k][0] - swap[k][0]).abs() <= 4.0 * ulp).all()), "%s %s: not symmetric in the two responses" % (terms, o)
            tot = sum(q[k] for q in parts[1:]) if len(parts) > 1 else None
            tot = parts[0][k] if tot is None else parts[0][k] + tot
            assert bool(((full[k][0] - tot[0]).abs() <= 4.0 * ulp).all()), "%s %s: a term list is not the sum of its terms" % (terms, o)
        # npair = 3 is three calls, bit for bit (the pairs: (1, 2), (2, 1), (1, 1))
        st = lambda *a: None if a[0] is None else torch.cat(a)  # noqa: E731
        three = _kxc(terms, rho, grho, st(dr1, dr2, dr1), st(dg1, dg2, dg1), st(dr2, dr1, dr1), st(dg2, dg1, dg1))
        one = _kxc(terms, rho, grho, dr1, dg1, dr1, dg1)
        for k in range(2):
            if full[k] is not None:
                assert torch.equal(three[k][0], full[k][0]) and torch.equal(three[k][1], swap[k][0]) and torch.equal(three[k][2], one[k][0])
        # lengths: one point, one short of a block, one over, and the grid-stride tail (4096 blocks of 256 threads, + 3)
        n0 = p["rho"].shape[0]
        for n in (1, 255, 257, 4096 * 256 + 3):
            rep = lambda a: None if a is None else (a.repeat_interleave((n + n0 - 1) // n0, dim=-1)[..., :n].contiguous() if n > n0  # noqa: E731
                                                    else a[..., :n].contiguous())
            out = _kxc(terms, rep(rho), rep(grho), rep(dr1), rep(dg1), rep(dr2), rep(dg2))
            for k in range(2):
                if full[k] is not None:
                    assert torch.equal(out[k], rep(full[k])), "%s: n = %d differs from the run over the fixture" % (terms, n)
        dead = _t(dev, (~(p["rho"] > xe.DENS_THRESHOLD)).astype(np.float64)) > 0
        for a in full:
            if a is not None:
                assert bool((a[..., dead] == 0.0).all()) and not bool(torch.signbit(a[..., dead]).any())


def test_kxc_gates_raise_without_a_launch(dev, fx):
    from dqc_amd import lib
    f, p = fx
    rho, grho, dr1, dg1, dr2, dg2 = _inputs(dev, p, True)
    n = rho.shape[0]
    nine = [(0.1, "lda_x")] * 9
    with pytest.raises(lib.DqcAmdError, match="at most 8 functional terms"):
        _kxc(nine, rho, None, dr1, None, dr2, None)
    for args in ((rho, None, dr1, dg1, dr2, dg2), (rho, grho, dr1, None, dr2, dg2), (rho, grho, dr1, dg1, dr2, None)):
        with pytest.raises(lib.DqcAmdError, match="GGA functional needs the density gradients"):
            _kxc([(1.0, "gga_x_pbe")], *args)
    with pytest.raises(NotImplementedError, match="meta-GGA"):  # the wrapper's own gate, shared with xc_eval_fxc
        _kxc([(1.0, "mgga_x_scan")], rho, grho, dr1, dg1, dr2, dg2)
    # the C entry itself, with real operands and outputs full of a sentinel: an error, and neither the zeroing nor a kernel ran
    L = lib.load()
    out_r = torch.full((1, n), 7.0, dtype=torch.float64, device=dev)
    out_g = torch.full((1, 3, n), 7.0, dtype=torch.float64, device=dev)
    ptr = lib._ptr

    def raw(ids, npair, gr=grho, o_g=out_g, nterm=None):
        ids_c = (ctypes.c_int * len(ids))(*ids)
        cfs = (ctypes.c_double * len(ids))(*([1.0] * len(ids)))
        with lib.call_trace() as tr, torch.cuda.device(dev):
            rc = L.dqc_xc_eval_kxc(ptr(out_r), ptr(o_g), ptr(rho), ptr(gr), ptr(dr1), ptr(dg1), ptr(dr2), ptr(dg2), n, npair, ids_c, cfs,
                                   len(ids) if nterm is None else nterm, None)
        assert not tr.rows
        return rc, L.dqc_last_error().decode()

    pbe, scan = lib.XC_IDS["gga_x_pbe"], lib.XC_IDS["mgga_x_scan"]
    for rc, msg, want in (raw([pbe] * 9, 1) + ("at most 8",), raw([pbe], 1, nterm=-1) + ("at most 8",), raw([pbe], -1) + ("negative number",),
                          raw([scan], 1) + ("only the LDA / GGA functional ids",), raw([pbe], 1, gr=None) + ("needs the density gradients",),
                          raw([pbe], 1, o_g=None) + ("needs the density gradients",)):
        assert rc != 0 and want in msg and "dqc_xc_eval_kxc" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((out_r == 7.0).all()) and bool((out_g == 7.0).all())
    # a good call afterwards is right
    name = "gga_x_pbe"
    d2v, d2vg = _kxc([(1.0, name)], rho, grho, dr1, dg1, dr2, dg2)
    val = f[name + "_val"]
    truth, scale = kg.compose_kxc(val[0], p), kg.compose_kxc(val[1], p, absolute=True)
    assert xe.scaled_error(d2v[0].cpu().numpy(), truth["d2vrho"], scale["d2vrho"]) < 1e-9
    assert xe.scaled_error(d2vg[0].cpu().numpy(), truth["d2vgrad"], scale["d2vgrad"]) < 1e-9
