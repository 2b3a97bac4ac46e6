"""The deterministic mode (dqc_set_deterministic: cross-block sums as 64-bit fixed-point integers, csrc/common.hpp acc_add / det_value)
against independent references, across input magnitudes.

Fixed point is exact in any summation order; how accurate it is depends on a scale that has to fit the data, and the three users of the
mode choose it in three ways: J / K per call from the densities, Vxc on the constant 2^47 after the Python
entry points have divided the potential by a power of two that bounds the call's own sums (dqc_amd/lib.py: _vxc_det_unit), the
purification trace on the constant 2^46.  Every reference here is a plain fp64 GEMM / einsum on the HOST from the same arrays (never
the device, never the fp64-atomic mode of the kernel under test); every magnitude factor is a power of two, so scaling a reference is
exact and one reference per shape serves every magnitude.  The bars are the ones the same kernels meet with fp64 atomics: 1e-12 of the
largest element (Vxc, J, K), the purification test's own 1e-12 / 1e-11."""
import json
import os

import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

VXC_NAO = [7, 48, 170, 240]  # vxc_ws_kernel on one panel and with several tiles per wave, vxc_wsu / vxc_wsd (145 ... 208), vxc_ws2 (> 208)
VXC_NGRID = [17, 4099]
VXC_MAGS = [-40, -20, 0, 20]  # the potentials are scaled by 2^k


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    return torch.device("cuda")


class _Det:
    """`with _Det():` -- the mode on inside, the previous setting back afterwards"""

    def __enter__(self):
        from dqc_amd import lib
        self.prev = lib.set_deterministic(True)

    def __exit__(self, *a):
        from dqc_amd import lib
        lib.set_deterministic(self.prev)
        return False


# ------------------------------------------------------------------------------------------------ a. - c. the Vxc family
_VXC = {}


def _vxc_case(dev, nao, ngrid):
    """synthetic arrays as in test_grid_kernels_shape_sweep_vs_torch (seeded), the device copies, and the four host references at
    magnitude 1 (made once per shape, never written to)"""
    from dqc_amd import lib
    key = (nao, ngrid)
    if key not in _VXC:
        gen = torch.Generator(device="cpu").manual_seed(1000 * nao + ngrid)
        a = torch.randn((4, ngrid, nao), dtype=torch.float64, generator=gen)
        w = torch.rand(ngrid, dtype=torch.float64, generator=gen)
        v = torch.randn(ngrid, dtype=torch.float64, generator=gen)
        vg = torch.randn((3, ngrid), dtype=torch.float64, generator=gen)
        _VXC[key] = {"host": (a, w, v, vg), "ref": _vxc_refs(a, w, v, vg), "ao": lib.ao_from(a.to(dev)), "w": w.to(dev), "v": v.to(dev),
                     "vg": vg.to(dev)}
    return _VXC[key]


def _vxc_refs(a, w, v, vg):
    """host fp64: sym(Phi^T (w v Phi + 2 sum_d w vg_d dPhi_d)), sym(Phi^T w v Phi), sym(dPhi_x^T w v dPhi_y)"""
    def sym(m):
        return 0.5 * (m + m.T)
    psi = (w * v)[:, None] * a[0] + 2 * (w[None, :, None] * vg[:, :, None] * a[1:]).sum(0)
    return {"gga": sym(a[0].T @ psi), "lda": sym(a[0].T @ ((w * v)[:, None] * a[0])), "pair": sym(a[1].T @ ((w * v)[:, None] * a[2]))}


def _decode_raw(raw, scale, nao):
    """the raw cross-block sums of grid_vxc_raw -> V on the host: fixed-point integers of the returned scale, (M + M^T) / 2"""
    m = raw.cpu()
    m = m.view(torch.int64).to(torch.float64) / scale if scale != 0.0 else m
    return (0.5 * (m + m.T))[:nao, :nao]


def _vxc_outputs(c, nao, v, vg, raw=True):
    """{variant: (nao, nao) host result} of the entry points of the family on the potentials v, vg; padding, finiteness and
    repeatability are asserted on the way"""
    from dqc_amd import lib
    ao, w = c["ao"], c["w"]
    calls = {"gga": lambda: lib.grid_vxc(ao, nao, w, v, vg), "lda": lambda: lib.grid_vxc(ao[0], nao, w, v, None),
             "pair": lambda: lib.grid_vxc_pair(ao[1], ao[2], nao, w, v)}
    out = {}
    for what, call in calls.items():
        o1, o2 = call(), call()
        assert torch.equal(o1, o2), (what, "two calls differ")
        assert bool(torch.isfinite(o1).all()), (what, "not finite")
        assert o1.shape[0] == o1.shape[1] == lib.padded_nao(nao) and not bool(o1[nao:].any()) and not bool(o1[:, nao:].any()), (what, "padding")
        out[what] = o1[:nao, :nao].cpu()
    if raw:
        for what, g in (("raw gga", vg), ("raw lda", None)):
            (r1, s1), (r2, s2) = (lib.grid_vxc_raw(ao if g is not None else ao[0], nao, w, v, g) for _ in range(2))
            # (compared as the integers they are: read as doubles, the negative ones are NaNs and equal nothing)
            assert s1 == s2 and s1 != 0.0 and torch.equal(r1.view(torch.int64), r2.view(torch.int64)), (what, "two calls differ")
            out[what] = _decode_raw(r1, s1, nao)
            assert bool(torch.isfinite(out[what]).all()), (what, "not finite")
    return out


def _vxc_check(out, refs, factor, tag):
    """every variant within 1e-12 max|ref| of its (exactly scaled) host reference; all figures are printed before the first assert"""
    rows = []
    for what, got in out.items():
        ref = refs[what.replace("raw ", "")] * factor
        rows.append((what, float((got - ref).abs().max()) / float(ref.abs().max())))
    print("%s: %s" % (tag, "  ".join("%s %.2e" % r for r in rows)))
    for what, err in rows:
        assert err < 1e-12, (tag, what, err)


@pytest.mark.parametrize("mag", VXC_MAGS, ids=["s=2^%d" % k for k in VXC_MAGS])
@pytest.mark.parametrize("ngrid", VXC_NGRID)
@pytest.mark.parametrize("nao", VXC_NAO)
def test_vxc_family_vs_host_reference_across_magnitudes(dev, nao, ngrid, mag):
    """a. grid_vxc (GGA and without the gradient term), grid_vxc_pair and grid_vxc_raw in deterministic mode on potentials scaled by
    2^-40 ... 2^20: 1e-12 of the largest element, exact zeros in the padding, two calls bit-equal, everything finite.
    grid_vxc_raw sums the potential as it is on the constant scale 2^47 -- its contract (include/dqc_amd.h: dqc_grid_vxc_raw, DESIGN.md
    section 4) is a potential with max |w v| of order one, which is how the fused Fock build uses it -- so its rows are checked at
    magnitude 1 only; at the parent of this file the other three entry points shared that limit (docs/LOG_r12.md)."""
    c = _vxc_case(dev, nao, ngrid)
    s = 2.0 ** mag
    with _Det():
        out = _vxc_outputs(c, nao, c["v"] * s, c["vg"] * s, raw=(mag == 0))
    _vxc_check(out, c["ref"], s, "nao %d ngrid %d s 2^%d" % (nao, ngrid, mag))


def test_vxc_mixed_magnitudes_zero_potential_and_empty_grid(dev):
    """b. potentials whose size varies over 2^-30 ... 1 from point to point inside ONE call (the bar stays relative to the largest
    element of the result); the zero potential and an empty grid give exact zeros"""
    from dqc_amd import lib
    nao, ngrid = 48, 4099
    c = _vxc_case(dev, nao, ngrid)
    a, w, v, vg = c["host"]
    u = torch.rand(ngrid, dtype=torch.float64, generator=torch.Generator(device="cpu").manual_seed(7))
    f = torch.exp2(-30.0 * u)
    refs = _vxc_refs(a, w, v * f, vg * f)
    with _Det():
        out = _vxc_outputs(c, nao, (v * f).to(dev), (vg * f).to(dev), raw=False)
        _vxc_check(out, refs, 1.0, "mixed magnitudes")
        zero = _vxc_outputs(c, nao, torch.zeros_like(c["v"]), torch.zeros_like(c["vg"]))
        for what, got in zero.items():
            assert float(got.abs().max()) == 0.0, ("zero potential", what)
        e = {"ao": lib.ao_from(torch.zeros((4, 0, nao), dtype=torch.float64, device=dev)), "w": c["w"][:0]}
        empty = _vxc_outputs(e, nao, c["v"][:0], c["vg"][:, :0].contiguous())
        for what, got in empty.items():
            assert got.shape == (nao, nao) and float(got.abs().max()) == 0.0, ("empty grid", what)


def test_vxc_two_streams_two_magnitudes(dev):
    """c. two grid_vxc calls of magnitudes 1 and 2^-20 issued back to back on two streams: each meets the bar of (a) and equals its
    own single-stream result bit for bit -- a per-call scale kept in state that the calls share would break one of them"""
    from dqc_amd import lib
    nao, ngrid = 170, 4099
    c = _vxc_case(dev, nao, ngrid)
    s = 2.0 ** -20
    with _Det():
        vs, vgs = c["v"] * s, c["vg"] * s
        alone = [lib.grid_vxc(c["ao"], nao, c["w"], c["v"], c["vg"]), lib.grid_vxc(c["ao"], nao, c["w"], vs, vgs)]
        torch.cuda.synchronize()
        st = [torch.cuda.Stream(), torch.cuda.Stream()]
        with torch.cuda.stream(st[0]):
            o0 = lib.grid_vxc(c["ao"], nao, c["w"], c["v"], c["vg"])
        with torch.cuda.stream(st[1]):
            o1 = lib.grid_vxc(c["ao"], nao, c["w"], vs, vgs)
        torch.cuda.synchronize()
    _vxc_check({"gga": o0[:nao, :nao].cpu()}, c["ref"], 1.0, "stream 0, s 1")
    _vxc_check({"gga": o1[:nao, :nao].cpu()}, c["ref"], s, "stream 1, s 2^-20")
    assert torch.equal(o0, alone[0]) and torch.equal(o1, alone[1])


# ------------------------------------------------------------------------------------------------ d. J / K from tiles
JK_CASES = [("h2o-sto3g", M.H2O, "sto-3g", 7), ("h2o-ccpvdz", M.H2O, "cc-pvdz", 24)]
_JK = {}


def _jk_case(dev, name, mol, basis):
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    if name not in _JK:
        t = ob.make_tables(mol, basis)
        tab = lib.Tables(t.atm, t.bas, t.env)
        S = nat.int1e("ovlp", t)
        dms = [M.seeded_dm_ao(tab.nao, 10, S, seed) for seed in (11, 12)]
        _JK[name] = {"tab": tab, "eri": nat.int2e(t), "tiles": lib.eri_tiles(tab, dev), "dms": dms}
    return _JK[name]


def _jk_ref(eri, d):
    """the einsum strings of test_integral_kernels_vs_oracle on the oracle's dense tensor"""
    return np.einsum("ij,ijkl->kl", d, eri), np.einsum("il,ijkl->jk", d, eri)


def _cu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name,mol,basis,nao", JK_CASES, ids=[c[0] for c in JK_CASES])
def test_jk_from_tiles_vs_oracle_tensor_across_magnitudes(dev, name, mol, basis, nao):
    """d. lib.jk and lib.jk_multi in deterministic mode against einsums on the oracle's (ij|kl): one density scaled by 2^-40, 1, 2^27
    to 1e-12; the zero density gives exact zeros (the scale kernel clamps its bound at 1e-300 and exp2 of the result is infinite: the
    outcome must still be 0, not NaN)"""
    from dqc_amd import lib
    c = _jk_case(dev, name, mol, basis)
    assert c["tab"].nao == nao
    work = lib.jk_workspace(nao, dev)
    d = c["dms"][0]
    jr, kr = _jk_ref(c["eri"], d)
    rows = []
    with _Det():
        for mag in (-40, 0, 27):
            s = 2.0 ** mag
            ds = _cu(d * s)
            J, K = lib.jk(c["tiles"], ds, work, True)
            J1, K1 = lib.jk(c["tiles"], ds, work, True)
            assert torch.equal(J, J1) and torch.equal(K, K1)
            Jo, none = lib.jk(c["tiles"], ds, work, False)
            Jm, Km = lib.jk_multi(c["tiles"], ds[None], ds[None])
            assert none is None
            for what, got, ref in (("jk J", J, jr), ("jk K", K, kr), ("jk J only", Jo, jr), ("jk_multi J", Jm[0], jr), ("jk_multi K", Km[0], kr)):
                rows.append(("2^%d %s" % (mag, what), float(np.abs(got.cpu().numpy() - ref * s).max() / np.abs(ref * s).max())))
        z = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
        zero = list(lib.jk(c["tiles"], z, work, True)) + list(lib.jk_multi(c["tiles"], z[None], z[None]))
    print("%s: %s" % (name, "  ".join("%s %.2e" % r for r in rows)))
    for what, err in rows:
        assert err < 1e-12, (name, what, err)
    for got in zero:
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) == 0.0, (name, "zero density")


@pytest.mark.parametrize("ratio", [-10, -27], ids=["ratio=2^-10", "ratio=2^-27"])
@pytest.mark.parametrize("name,mol,basis,nao", JK_CASES, ids=[c[0] for c in JK_CASES])
def test_jk_multi_shared_scale_contract(dev, name, mol, basis, nao, ratio):
    """d. the contract of lib.jk_multi: the densities of one pass share ONE fixed-point scale, set by the largest.  Two slots of
    ratio 2^-10 and 2^-27, in the grid form (two Coulomb and two exchange densities) and the stream form (exchange only): every
    slot's error is below 1e-12 of the largest reference of the pass, and the large slot equals bit for bit what it is beside a
    partner of its own size (test_antisymmetric_exchange_matches_einsum checks that at ratio 2)"""
    from dqc_amd import lib
    c = _jk_case(dev, name, mol, basis)
    big, other = c["dms"]
    assert np.abs(big).sum() > np.abs(0.5 * other).sum()  # the large slot sets the scale beside either partner
    small = other * 2.0 ** ratio
    refs = [_jk_ref(c["eri"], big), _jk_ref(c["eri"], small)]
    pair, peer = torch.stack([_cu(big), _cu(small)]), torch.stack([_cu(big), _cu(0.5 * other)])
    rows = []
    with _Det():
        for form, dj in (("grid", True), ("stream", False)):
            J, K = lib.jk_multi(c["tiles"], pair if dj else None, pair)
            Jp, Kp = lib.jk_multi(c["tiles"], peer if dj else None, peer)
            assert torch.equal(K[0], Kp[0]) and (not dj or torch.equal(J[0], Jp[0])), (form, "the large slot follows its partner")
            for q in range(2):
                for what, got, col in (("J", J, 0), ("K", K, 1)):
                    if got is not None:
                        top = max(np.abs(refs[0][col]).max(), np.abs(refs[1][col]).max())
                        rows.append(("%s %s[%d]" % (form, what, q), float(np.abs(got[q].cpu().numpy() - refs[q][col]).max() / top)))
    print("%s ratio 2^%d: %s" % (name, ratio, "  ".join("%s %.2e" % r for r in rows)))
    for what, err in rows:
        assert err < 1e-12, (name, ratio, what, err)


# ------------------------------------------------------------------------------------------------ e. purification
@pytest.mark.parametrize("n", [24, 208])
def test_purification_vs_host_eigh(dev, n):
    """e. the TC2 projector in deterministic mode (traces as fixed-point integers on 2^46) of a synthetic Fock matrix with a clear
    gap -- the persistent kernel (projector_from_fock) and the one-launch-per-iteration form (lib.purify_tc2) -- against
    torch.linalg.eigh on the host, to the bar of test_purification_equals_eigh_projector; two runs bit-equal"""
    from dqc_amd import lib
    from dqc_amd.purify import projector_from_fock
    nocc = n // 4
    gen = torch.Generator(device="cpu").manual_seed(n)
    q, _ = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, generator=gen))
    eig = torch.cat([torch.linspace(-1.0, -0.5, nocc, dtype=torch.float64), torch.linspace(0.5, 1.5, n - nocc, dtype=torch.float64)])
    f = (q * eig) @ q.T
    f = 0.5 * (f + f.T)
    _, c = torch.linalg.eigh(f)
    pref = c[:, :nocc] @ c[:, :nocc].T
    fd = f.to(dev)

    def launches():
        # what projector_from_fock does around lib.purify_tc2 when the persistent kernel is not taken
        diag = torch.diagonal(fd)
        rad = fd.abs().sum(-1) - diag.abs()
        emin, emax = (diag - rad).min(), (diag + rad).max()
        ld, iters = lib.padded_nao(n), 64
        xp = torch.zeros((ld, ld), dtype=torch.float64, device=dev)
        xp[:n, :n] = (emax * torch.eye(n, dtype=torch.float64, device=dev) - fd) / (emax - emin)
        lib.purify_tc2(xp, torch.empty_like(xp), nocc, iters, 1e-13, torch.empty(2 * (iters + 2), dtype=torch.float64, device=dev))
        x = xp[:n, :n]
        for _ in range(2):
            x2 = x @ x
            x = 3.0 * x2 - 2.0 * (x2 @ x)
        x = 0.5 * (x + x.T)
        return x, ((x @ x) - x).abs().max() + (torch.trace(x) - nocc).abs()

    with _Det():
        for what, run in (("persistent", lambda: projector_from_fock(fd, nocc, fused=True)), ("launches", launches)):
            (p1, e1), (p2, e2) = run(), run()
            diff = float((p1.cpu() - pref).abs().max())
            print("n %d %s: idempotency %.2e  max|P - eigh| %.2e" % (n, what, float(e1), diff))
            assert torch.equal(p1, p2), (what, "two runs differ")
            assert float(e1) < 1e-12 and diff < 1e-11, what


# ------------------------------------------------------------------------------------------------ f. the two callers
def test_get_vext_of_large_potential(dev):
    """f. HamiltonMI355.get_vext sends a caller's potential of any size through lib.grid_vxc: a uniform 3.0 * 2^20 in
    deterministic mode is 2^20 times the fp64-atomic result for 3.0 to 1e-12, and its diagonal is the constant
    (test_hamiltonian_api_surface)"""
    import dqc_amd
    from dqc_amd import lib
    mol = dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2")
    h = mol.get_hamiltonian()
    h.build()
    mol.setup_grid()
    h.setup_grid(mol.get_grid(), dqc_amd.get_xc("gga_x_pbe"))
    ngrid, s = mol.get_grid().get_rgrid().shape[0], 2.0 ** 20
    vext = torch.full((ngrid,), 3.0, dtype=torch.float64, device=dev)
    prev = lib.set_deterministic(False)
    try:
        plain = h.get_vext(vext).fullmatrix()
        lib.set_deterministic(True)
        small, large = h.get_vext(vext).fullmatrix(), h.get_vext(vext * s).fullmatrix()
    finally:
        lib.set_deterministic(prev)
    top = float(plain.abs().max())
    errs = float((small - plain).abs().max()) / top, float((large - plain * s).abs().max()) / (top * s)
    print("get_vext deterministic vs fp64 atomics: 3.0 %.2e   3.0 * 2^20 %.2e" % errs)
    assert errs[0] < 1e-12 and errs[1] < 1e-12
    for m, const in ((small, 3.0), (large, 3.0 * s)):
        dv = torch.diagonal(m)
        assert torch.allclose(dv, torch.full_like(dv, const), rtol=2e-3)  # sg2 quadrature error


def test_polarizability_in_deterministic_mode(dev, golden_dir):
    """f. the h2o_lda case of test_polarizability_matches_oracle_finite_field with the mode on (every trial vector of the conjugate-
    gradient solve sends f_xc . d rho through lib.grid_vxc, and the search directions shrink with the residual): same fixture,
    same tolerance; two runs give the same tensor bit for bit"""
    import dqc_amd
    from dqc_amd.response import state_memo
    g = np.load(os.path.join(golden_dir, "oracle_orb_hessian.npz"))
    case, m = "h2o_lda", json.loads(str(g["meta"]))["h2o_lda"]
    assert m["spin"] is None
    with _Det():
        mol = dqc_amd.Mol((m["atomzs"], m["atompos"]), basis=m["basis"], grid=m["grid"])
        qc = dqc_amd.KS(mol, xc=m["xc"])
        h = qc._engine.hamilton
        sx = h._ovlp_ao @ h._orthozer
        qc.run(dm0=(sx.T @ _cu(g[case + "_dm_ao_0"]) @ sx).contiguous(), fwd_options={"f_tol": 1e-11, "maxiter": 300})
        assert qc.accepted
        alphas = []
        for _ in range(2):
            state_memo(qc).clear()  # the operator and the tensor are kept on the calculation: compute them afresh
            alphas.append(dqc_amd.polarizability(qc))
    alpha = alphas[0].cpu().numpy()
    tol = 10.0 * float(g[case + "_alpha_error"])
    err = np.abs(alpha - g[case + "_alpha"]).max()
    print("%-12s deterministic: max|alpha - finite field| %.2e  (tolerance %.2e)" % (case, err, tol))
    assert alpha.shape == (3, 3) and err < tol
    assert np.abs(alpha - alpha.T).max() < 1e-7
    assert torch.equal(alphas[0], alphas[1])
