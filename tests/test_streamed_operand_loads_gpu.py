"""The loads of once-read operands in the three hot kernel families, at the EDGES of the arrays they read: the rows of the AO arrays
in the density pass (density_roles_kernel, density_lr_kernel: streamed past the caches with csrc/grid_common.hpp load_once16 /
load_once8) and in the Vxc families (vxc_wsd, vxc_ws, vxc_ws2: buffer loads), and the ERI tiles of the Coulomb stream
(j_stream_kernel) -- the sites whose cache policy round 18 measured (docs/LOG_r18.md).  A cache policy changes no value, so the
bounds are those of the neighbouring tests of the same entry points (max |error| < 1e-12 max |ref| against fp64 torch); the shapes
are a lone point, a partial 16-point chunk, a partial 64-point tile, one point over a tile and many blocks with a ragged last slab,
row strides below the staged width (nao 150: lda 152 < ld 160, the slack past a row's end is read) and a last AO block of width 4.
Every AO array is allocated at exactly dqc_ao_doubles (lib.ao_from), so a load past the slack would leave the allocation.
Deterministic mode: two calls equal bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NGRID = [1, 15, 63, 65, 4099]
BOUND = 1e-12
DEN_CASES = [(208, 46), (150, 37)]  # (nao, factor columns): density_roles_kernel<3, 13>; density_lr_kernel<3, 10>
VXC_GGA_NAO = [208, 150, 100, 212]  # vxc_wsd T = 13, vxc_wsd T = 10, vxc_ws, vxc_ws2
VXC_LDA_NAO = [100, 212]            # vxc_ws, vxc_ws2
J_NAO = [20, 24]                    # last AO block of width 4 / a full one

_AO = {}
_DEN = {}
_VXC = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    return torch.device("cuda")


def _ao(dev, nao, ngrid):
    """seeded AO values and gradients in the kernels' layout: exactly dqc_ao_doubles doubles (made once per shape, never written to)"""
    from dqc_amd import lib
    key = (nao, ngrid)
    if key not in _AO:
        gen = torch.Generator(device="cpu").manual_seed(104729 * nao + ngrid)
        vals = torch.randn((4, ngrid, nao), dtype=torch.float64, generator=gen)
        w = torch.rand(ngrid, dtype=torch.float64, generator=gen)
        v = torch.randn(ngrid, dtype=torch.float64, generator=gen)
        vg = torch.randn((3, ngrid), dtype=torch.float64, generator=gen)
        ao = lib.ao_from(vals.to(dev))
        ao0 = lib.ao_from(vals[0].to(dev))  # the value array on its own: its slack is the end of the allocation too
        assert ao.untyped_storage().nbytes() == 8 * lib.load().dqc_ao_doubles(4, ngrid, nao)
        assert ao0.untyped_storage().nbytes() == 8 * lib.load().dqc_ao_doubles(1, ngrid, nao)
        assert torch.equal(ao0, ao[0])
        _AO[key] = (ao, w.to(dev), v.to(dev), vg.to(dev), ao0)
    return _AO[key]


def _den_case(dev, nao, ncol, ngrid):
    from dqc_amd import lib
    key = (nao, ncol, ngrid)
    if key not in _DEN:
        ao = _ao(dev, nao, ngrid)[0]
        gen = torch.Generator(device="cpu").manual_seed(31 * nao + ncol)
        l_ao = (torch.randn((nao, ncol), dtype=torch.float64, generator=gen) / nao ** 0.5).to(dev)
        factor = lib.pad_factor(l_ao, lib.padded_nao(nao))
        assert factor is not None
        a = ao[:, :, :nao]
        b = (a[0] @ l_ao) @ l_ao.T
        _DEN[key] = (factor, (b * a[0]).sum(-1), 2.0 * (b[None] * a[1:]).sum(-1))
    return _DEN[key]


def _vxc_ref(dev, nao, ngrid, gga):
    key = (nao, ngrid, gga)
    if key not in _VXC:
        ao, w, v, vg = _ao(dev, nao, ngrid)[:4]
        a = ao[:, :, :nao]
        psi = (w * v)[:, None] * a[0]
        if gga:
            psi = psi + 2 * (w[None, :, None] * vg[:, :, None] * a[1:]).sum(0)
        m = a[0].T @ psi
        _VXC[key] = 0.5 * (m + m.T)
    return _VXC[key]


def _decode_raw(raw, scale, nao):
    """the raw cross-block sums of grid_vxc_raw -> V: fixed-point integers of the returned scale (0: doubles), (M + M^T) / 2"""
    m = raw.view(torch.int64).to(torch.float64) / scale if scale != 0.0 else raw
    return (0.5 * (m + m.T))[:nao, :nao]


def _bits(x):
    return x.contiguous().view(torch.int64)


@pytest.mark.parametrize("gga", [True, False], ids=["gradient", "value"])
@pytest.mark.parametrize("nao,ncol", DEN_CASES, ids=["nao208-roles", "nao150-lr"])
def test_density_streamed_rows_vs_torch(dev, nao, ncol, gga):
    from dqc_amd import lib
    assert (lib.ao_stride(nao), lib.padded_nao(nao)) == ((208, 208) if nao == 208 else (152, 160))
    rows = []
    for ngrid in NGRID:
        ao, ao0 = _ao(dev, nao, ngrid)[0], _ao(dev, nao, ngrid)[4]
        factor, rho_ref, grho_ref = _den_case(dev, nao, ncol, ngrid)
        arg = ao if gga else ao0
        rho, grho = lib.grid_density_lr(arg, nao, factor, gga)
        prev = lib.set_deterministic(True)
        try:
            d1, d2 = lib.grid_density_lr(arg, nao, factor, gga), lib.grid_density_lr(arg, nao, factor, gga)
        finally:
            lib.set_deterministic(prev)
        e_rho = float((rho - rho_ref).abs().max()) / float(rho_ref.abs().max())
        e_g = float((grho - grho_ref).abs().max()) / float(grho_ref.abs().max()) if gga else 0.0
        same = torch.equal(_bits(d1[0]), _bits(d2[0])) and (not gga or torch.equal(_bits(d1[1]), _bits(d2[1])))
        rows.append((ngrid, e_rho, e_g, same, (grho is None) == (not gga)))
    print("density nao %d r %d gga %d: %s" % (nao, ncol, gga, "  ".join("ngrid %d: %.2e %.2e" % r[:3] for r in rows)))
    for ngrid, e_rho, e_g, same, shape_ok in rows:
        assert e_rho < BOUND, (nao, ngrid, "rho", e_rho)
        assert e_g < BOUND, (nao, ngrid, "grad rho", e_g)
        assert same, (nao, ngrid, "two deterministic calls differ")
        assert shape_ok, (nao, ngrid)


def _vxc_check(dev, nao, gga):
    from dqc_amd import lib
    ld = lib.padded_nao(nao)
    rows = []
    for ngrid in NGRID:
        ao, w, v, vg, ao0 = _ao(dev, nao, ngrid)
        ref = _vxc_ref(dev, nao, ngrid, gga)
        args = (ao, nao, w, v, vg) if gga else (ao0, nao, w, v, None)
        scale = float(ref.abs().max())
        out = lib.grid_vxc(*args)
        raw, rs = lib.grid_vxc_raw(*args)
        prev = lib.set_deterministic(True)
        try:
            d1, d2 = lib.grid_vxc(*args), lib.grid_vxc(*args)
            (r1, s1), (r2, s2) = lib.grid_vxc_raw(*args), lib.grid_vxc_raw(*args)
        finally:
            lib.set_deterministic(prev)
        errs = (float((out[:nao, :nao] - ref).abs().max()) / scale, float((_decode_raw(raw, rs, nao) - ref).abs().max()) / scale,
                float((d1[:nao, :nao] - ref).abs().max()) / scale, float((_decode_raw(r1, s1, nao) - ref).abs().max()) / scale)
        same = torch.equal(_bits(d1), _bits(d2)) and s1 == s2 and torch.equal(_bits(r1), _bits(r2))
        pad_zero = out.shape == (ld, ld) and not bool(out[nao:].any()) and not bool(out[:, nao:].any())
        rows.append((ngrid, errs, same, pad_zero))
    print("vxc nao %d gga %d (lda %d, ld %d): %s" % (nao, gga, lib.ao_stride(nao), ld,
                                                     "  ".join("ngrid %d: %s" % (r[0], " ".join("%.1e" % e for e in r[1])) for r in rows)))
    for ngrid, errs, same, pad_zero in rows:
        for what, e in zip(("grid_vxc", "grid_vxc_raw", "deterministic grid_vxc", "deterministic grid_vxc_raw"), errs):
            assert e < BOUND, (nao, ngrid, what, e)
        assert same, (nao, ngrid, "two deterministic calls differ")
        assert pad_zero, (nao, ngrid, "padding rows / columns are not exactly zero")


@pytest.mark.parametrize("nao", VXC_GGA_NAO)
def test_vxc_gga_streamed_rows_vs_torch(dev, nao):
    _vxc_check(dev, nao, True)


@pytest.mark.parametrize("nao", VXC_LDA_NAO)
def test_vxc_lda_streamed_rows_vs_torch(dev, nao):
    _vxc_check(dev, nao, False)


def _j_tables(nao):
    from oracle import basis as ob
    from dqc_amd import lib
    # two centres of 10 (s s p d) or 12 (s p p d) functions
    s1, s2, p1, p2, d1 = (0, [3.1, 0.7], [0.4, 0.7]), (0, [0.25], [1.0]), (1, [1.3, 0.35], [0.5, 0.6]), (1, [0.2], [1.0]), (2, [0.8], [1.0])
    shells = {20: [s1, s2, p1, d1], 24: [s1, p1, p2, d1]}[nao]
    t = ob.make_tables(([7, 6], np.array([[0.1, -0.2, 0.3], [0.9, 0.7, 1.6]])), [shells, shells])
    tab = lib.Tables(t.atm, t.bas, t.env)
    assert tab.nao == nao
    return tab


@pytest.mark.parametrize("nao", J_NAO)
def test_coulomb_stream_streamed_tiles_vs_dense(dev, nao):
    """J only (j_stream_kernel) against the dense contraction of the tile store it streams"""
    from dqc_amd import lib
    tab = _j_tables(nao)
    tiles = lib.eri_tiles(tab, dev)
    assert tiles.numel() == lib.eri_store_doubles(nao)
    dense = lib.eri_dense(tiles, nao)
    gen = torch.Generator(device="cpu").manual_seed(nao)
    d = torch.randn((nao, nao), dtype=torch.float64, generator=gen).to(dev)
    ds = 0.5 * (d + d.T)
    ref = torch.einsum("ij,ijkl->kl", ds, dense)
    work = lib.jk_workspace(nao, dev)
    j, k = lib.jk(tiles, d, work, False)
    prev = lib.set_deterministic(True)
    try:
        j1, j2 = lib.jk(tiles, d, work, False)[0], lib.jk(tiles, d, work, False)[0]
    finally:
        lib.set_deterministic(prev)
    scale = float(ref.abs().max())
    e, e_det = float((j - ref).abs().max()) / scale, float((j1 - ref).abs().max()) / scale
    print("J nao %d: %.2e  deterministic %.2e" % (nao, e, e_det))
    assert k is None
    assert e < BOUND and e_det < BOUND, (nao, e, e_det)
    assert torch.equal(_bits(j1), _bits(j2)), (nao, "two deterministic calls differ")
