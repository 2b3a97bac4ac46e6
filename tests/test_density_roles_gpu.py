"""The role-split factor-form density kernel (density_roles_kernel, grid_density.hip) against density_lr_kernel.

dqc_grid_density_lr picks the role-split kernel for the GGA shapes it is instantiated for (norb_pad 48 and 13 AO tiles: the C5
shape) unless DQC_DENSITY_ROLES=0 is in the environment.  The new kernel issues the same MFMAs in the same order per accumulator
and runs the same row-dot epilogue in the same order per lane, so rho and grad rho are required to be BIT-EQUAL to the old
kernel's, point for point, on every shape below; a shape the new kernel does not serve must dispatch to the old one.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAOS = [208, 114, 412, 197]          # C5, benzene, a two-panel shape, and one that is not a multiple of 16 (13 tiles, lda 200)
NOCCS = [5, 21, 40]                  # factor widths that pad to 1, 2 and 3 row tiles
NGRIDS = [64 * 313, 20011]           # a multiple of 64 and a ragged one; both more tiles than the chip has CUs
CASES = [(n, r, g) for n in NAOS for r in NOCCS for g in NGRIDS] + [(208, 40, 64 * 1500 + 37), (197, 33, 64 * 1100 + 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    return torch.device("cuda")


@pytest.fixture()
def roles_env():
    old = os.environ.get("DQC_DENSITY_ROLES")
    yield
    if old is None:
        os.environ.pop("DQC_DENSITY_ROLES", None)
    else:
        os.environ["DQC_DENSITY_ROLES"] = old


def _inputs(dev, nao, nocc, ngrid):
    from dqc_amd import lib
    g = torch.Generator(device="cpu").manual_seed(1000 * nao + 10 * nocc + ngrid % 7)
    ao = lib.ao_empty(4, ngrid, nao, dev, zero=True)
    ao[..., :nao] = torch.randn((4, ngrid, nao), dtype=torch.float64, generator=g).to(dev)
    L = (torch.randn((nao, nocc), dtype=torch.float64, generator=g) / np.sqrt(nao)).to(dev)
    fac = lib.pad_factor(L, lib.padded_nao(nao))
    return ao, fac


def _run(ao, nao, fac, on):
    from dqc_amd import lib
    os.environ["DQC_DENSITY_ROLES"] = "1" if on else "0"
    rho, grho = lib.grid_density_lr(ao, nao, fac, True)
    torch.cuda.synchronize()
    return rho.cpu().numpy(), grho.cpu().numpy()


def _served(nao, rp):
    # what this pull request claims to serve: NRT = 3, 13 AO tiles
    return rp == 48 and (nao + 15) // 16 == 13


@pytest.mark.parametrize("nao,nocc,ngrid", CASES)
def test_roles_kernel_bit_equal_to_density_lr_kernel(dev, roles_env, nao, nocc, ngrid):
    from dqc_amd import lib
    ao, fac = _inputs(dev, nao, nocc, ngrid)
    rp = fac[0].shape[1]
    c = lib.load()
    os.environ["DQC_DENSITY_ROLES"] = "1"
    assert c.dqc_grid_density_lr_roles(nao, rp, 1) == (1 if _served(nao, rp) else 0)
    assert c.dqc_grid_density_lr_roles(nao, rp, 0) == 0  # value-only form: always the old kernel
    os.environ["DQC_DENSITY_ROLES"] = "0"
    assert c.dqc_grid_density_lr_roles(nao, rp, 1) == 0
    rho0, g0 = _run(ao, nao, fac, False)
    rho1, g1 = _run(ao, nao, fac, True)
    assert np.isfinite(rho0).all() and np.isfinite(g0).all()
    nd_rho, nd_g = int((rho0 != rho1).sum()), int((g0 != g1).sum())
    worst = max(float(np.abs(rho1 - rho0).max() / np.abs(rho0).max()), float(np.abs(g1 - g0).max() / np.abs(g0).max()))
    print("nao %d rp %d ngrid %d served %d: differing rho %d grho %d, worst relative difference %.3e"
          % (nao, rp, ngrid, _served(nao, rp), nd_rho, nd_g, worst))
    assert np.array_equal(rho0, rho1) and np.array_equal(g0, g1)


@pytest.mark.parametrize("nao,nocc,ngrid", [(208, 40, 20011), (197, 40, 64 * 313), (114, 21, 20011)])
def test_roles_kernel_deterministic_mode_reproducible(dev, roles_env, nao, nocc, ngrid):
    from dqc_amd import lib
    ao, fac = _inputs(dev, nao, nocc, ngrid)
    prev = lib.set_deterministic(True)
    try:
        a = _run(ao, nao, fac, True)
        b = _run(ao, nao, fac, True)
        c = _run(ao, nao, fac, False)
    finally:
        lib.set_deterministic(prev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
