"""vxc_wsd_kernel (GGA Vxc, 10 <= T <= 13 tile rows, nao 145 ... 208) with the compile-time tile ownership and the per-wave fragment
sets (csrc/grid_vxc.hip: WSD_OWNER, WsdChunk): every T at its smallest and its largest nao (row stride of the AO arrays below and
equal to the staged width 16 T) x grid sizes with fewer points than blocks, one chunk + 1 and ragged slabs, against the fp64 torch
expression of test_grid_kernels_shape_sweep_vs_torch with its bound, max |error| < 1e-12 max |ref|; the raw split-K sums with the
symmetrisation on the host; the deterministic mode (two calls equal bit for bit, within the same bound of the fp64-atomic result)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAO = [145, 160, 161, 176, 177, 192, 193, 208]  # T = 10, 11, 12, 13: the smallest and the largest nao of each
NGRID = [1, 17, 4099, 20011]
RAW_NAO = [150, 208]
DET_NAO = [150, 180, 208]
DET_NGRID = 4099
BOUND = 1e-12

_CASES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    return torch.device("cuda")


def _case(dev, nao, ngrid):
    """seeded synthetic arrays in the kernels' layout and the fp64 torch reference (made once per shape, never written to)"""
    from dqc_amd import lib
    key = (nao, ngrid)
    if key not in _CASES:
        gen = torch.Generator(device="cpu").manual_seed(7919 * nao + ngrid)
        ao = torch.randn((4, ngrid, nao), dtype=torch.float64, generator=gen)
        w = torch.rand(ngrid, dtype=torch.float64, generator=gen)
        v = torch.randn(ngrid, dtype=torch.float64, generator=gen)
        vg = torch.randn((3, ngrid), dtype=torch.float64, generator=gen)
        ao, w, v, vg = (x.to(dev) for x in (ao, w, v, vg))
        ao = lib.ao_from(ao)
        a = ao[:, :, :nao]
        psi = (w * v)[:, None] * a[0] + 2 * (w[None, :, None] * vg[:, :, None] * a[1:]).sum(0)
        m = a[0].T @ psi
        _CASES[key] = (ao, w, v, vg, 0.5 * (m + m.T))
    return _CASES[key]


def _decode_raw(raw, scale, nao):
    """the raw cross-block sums of grid_vxc_raw -> V: fixed-point integers of the returned scale (0: doubles), (M + M^T) / 2"""
    m = raw.view(torch.int64).to(torch.float64) / scale if scale != 0.0 else raw
    return (0.5 * (m + m.T))[:nao, :nao]


@pytest.mark.parametrize("nao", NAO)
def test_wsd_shapes_vs_torch(dev, nao):
    from dqc_amd import lib
    ld = lib.padded_nao(nao)
    assert 10 <= ld // 16 <= 13
    rows = []
    for ngrid in NGRID:
        ao, w, v, vg, ref = _case(dev, nao, ngrid)
        out = lib.grid_vxc(ao, nao, w, v, vg)
        rows.append((ngrid, float((out[:nao, :nao] - ref).abs().max()) / float(ref.abs().max()),
                     out.shape == (ld, ld) and not bool(out[nao:].any()) and not bool(out[:, nao:].any())))
    print("nao %d (lda %d, ld %d): %s" % (nao, lib.ao_stride(nao), ld, "  ".join("ngrid %d: %.2e" % r[:2] for r in rows)))
    for ngrid, err, pad_zero in rows:
        assert err < BOUND, (nao, ngrid, err)
        assert pad_zero, (nao, ngrid, "padding rows / columns are not exactly zero")


@pytest.mark.parametrize("nao", RAW_NAO)
def test_wsd_raw_sums_symmetrised_on_host(dev, nao):
    from dqc_amd import lib
    for ngrid in (17, 4099):
        ao, w, v, vg, ref = _case(dev, nao, ngrid)
        raw, scale = lib.grid_vxc_raw(ao, nao, w, v, vg)
        err = float((_decode_raw(raw, scale, nao) - ref).abs().max()) / float(ref.abs().max())
        print("raw nao %d ngrid %d: %.2e" % (nao, ngrid, err))
        assert err < BOUND, (nao, ngrid, err)


@pytest.mark.parametrize("nao", DET_NAO)
def test_wsd_deterministic_mode(dev, nao):
    from dqc_amd import lib
    ao, w, v, vg, ref = _case(dev, nao, DET_NGRID)
    prev = lib.set_deterministic(False)
    try:
        atomic = lib.grid_vxc(ao, nao, w, v, vg)
        lib.set_deterministic(True)
        d1, d2 = lib.grid_vxc(ao, nao, w, v, vg), lib.grid_vxc(ao, nao, w, v, vg)
        (r1, s1), (r2, s2) = (lib.grid_vxc_raw(ao, nao, w, v, vg) for _ in range(2))
    finally:
        lib.set_deterministic(prev)
    scale = float(ref.abs().max())
    e_atomic = float((d1 - atomic).abs().max()) / scale
    e_ref = float((d1[:nao, :nao] - ref).abs().max()) / scale
    e_raw = float((_decode_raw(r1, s1, nao) - ref).abs().max()) / scale
    print("det nao %d: vs fp64 atomics %.2e  vs torch %.2e  raw vs torch %.2e" % (nao, e_atomic, e_ref, e_raw))
    assert torch.equal(d1, d2), (nao, "two deterministic calls differ")
    # (compared as the integers they are: read as doubles, the negative ones are NaNs and equal nothing)
    assert s1 == s2 and s1 != 0.0 and torch.equal(r1.view(torch.int64), r2.view(torch.int64)), (nao, "two raw calls differ")
    assert e_atomic < BOUND, (nao, e_atomic)
    assert e_ref < BOUND, (nao, e_ref)
    assert e_raw < BOUND, (nao, e_raw)
    assert not bool(d1[nao:].any()) and not bool(d1[:, nao:].any()), (nao, "padding")
