"""Density-fitted exchange (RI-K): Mol.densityfit(exchange=True), dqc_df_exchange, HF and hybrids on a fitted Hamiltonian.

The reference has no fitted exchange.  Yardsticks:
  * the contraction: K_ref = sum (mu lam|P) [j2c^-1 (nu sig|.)]_P D_lam,sig in numpy (np.linalg.solve, no explicit inverse) from the
    Hamiltonian's own j2c / j3c copied to the host -- the integrals are pinned elsewhere (test_gpu_parity).  Bar 1e-10, the standing
    bar for K elements: on the CPU the stable-solve form and the Cholesky-whitened factor form agree to 6e-14 on benzene / cc-pVDZ
    (|K| ~ 2-4); the explicit-inverse form is off by 9e-11, hence no inverse on either side;
  * Fock builds: 1e-9 (the bar of the hybrid builds: 1e-10 on J and K, 1e-9 on Vxc);
  * converged energies: tests/golden/oracle_dfk.json (tools/make_dfk_golden.py: the oracle's fitted J, a numpy K_df, the oracle's
    Vxc, iterated to 1e-11), 1e-8 Ha, the standing bar."""
import json
import os

import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

TIGHT = {"f_tol": 1e-11, "maxiter": 300}
H2 = ([1, 1], [[0, 0, 0], [0, 0, 1.4]])
# name: (molecule, basis, nao, naux or None, rank of the seeded density, seed)
SHAPES = {
    "h2-321g": (H2, "3-21G", 4, 40, 1, 21),
    "h2o-321g": (M.H2O, "3-21G", 13, 101, 5, 22),
    "h2o-ccpvdz": (M.H2O, "cc-pvdz", 24, None, 5, 23),
    "benzene-ccpvdz": (M.benzene(), "cc-pvdz", 114, 486, 21, 24),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "oracle_dfk.json")))


def _k_ref(h, dao):
    """K_ref[mu, nu] = sum (mu lam|P) [j2c^-1 (nu sig|.)]_P D[lam, sig] on the host"""
    j3c, j2c = h.df.j3c.cpu().numpy(), h.df.j2c.cpu().numpy()
    nao, naux = j3c.shape[0], j3c.shape[2]
    cfit = np.linalg.solve(j2c, j3c.reshape(-1, naux).T).reshape(naux, nao, nao)  # [P, nu, sig]
    t = (j3c.transpose(0, 2, 1).reshape(nao * naux, nao) @ dao).reshape(nao, naux * nao)          # [mu, (P, sig)]
    return t @ cfit.transpose(1, 0, 2).reshape(nao, naux * nao).T


_CACHE = {}


def _case(name):
    """(Hamiltonian, orbitals, weights, K_ref of their density) of one shape: built once, shared, never modified"""
    if name not in _CACHE:
        import dqc_amd
        mol, basis, nao, naux, r, seed = SHAPES[name]
        h = dqc_amd.Mol(mol, basis=basis).densityfit(auxbasis="etb", exchange=True).get_hamiltonian().build()
        assert h._nao_ao == nao and (naux is None or h.df.j2c.shape[0] == naux)
        S = h._ovlp_ao.cpu().numpy()
        sx = h._ovlp_ao @ h._orthozer
        d = sx.T @ torch.as_tensor(M.seeded_dm_ao(nao, 2 * r, S, seed), device=h.device) @ sx
        w, c = torch.linalg.eigh((d + d.T) * 0.5)
        orb, w = c[:, -r:].contiguous(), w[-r:].contiguous()   # the seeded density has rank r: its r positive eigenpairs
        dao = (h._orthozer @ (orb * w) @ orb.T @ h._orthozer.T).cpu().numpy()
        _CACHE[name] = (h, orb, w, _k_ref(h, (dao + dao.T) * 0.5))
    return _CACHE[name]


def _orth_dm(h, d_ao):
    sx = h._ovlp_ao @ h._orthozer
    return (sx.T @ torch.as_tensor(d_ao, device=h.device) @ sx).contiguous()


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_vs_host_reference(dev, name):
    """dqc_df_exchange on the orbital factor of an ao_orb2dm density == K_ref to 1e-10; symmetric; the kernel ran"""
    from dqc_amd import lib
    h, orb, w, kref = _case(name)
    dm = h.ao_orb2dm(orb, w)
    fac = h._factor_of(dm)
    assert fac is not None and len(fac) == 1
    with lib.call_trace() as tr:
        k = h.df.exchange_ao(None, fac)
    assert any(r[0] == "dqc_df_exchange" for r in tr.rows)
    err = np.abs(k.cpu().numpy() - kref).max()
    asym = float((k - k.T).abs().max())
    print("df_exchange %s: nao %d naux %d rp %d  max|K| %.3f  max|K - K_ref| %.2e  asym %.1e"
          % (name, h._nao_ao, h.df.j2c.shape[0], fac[0][0].shape[1], np.abs(kref).max(), err, asym))
    assert err < 1e-10
    assert asym <= 1e-13 * max(1.0, np.abs(kref).max())
    # and through the operator: -K/2 in the orthogonalised basis
    kx = h.get_exchange(dm).fullmatrix()
    sx = h._ovlp_ao @ h._orthozer
    assert np.abs((sx @ kx @ sx.T).cpu().numpy() + 0.5 * kref).max() < 1e-10


@pytest.mark.parametrize("r", [40, 60, 90, 100])
def test_every_factor_width_and_lds_chunking(dev, r):
    """benzene with wider seeded factors: the padded widths 48, 64, 96 and 128 (the kernel's other instantiations), and at 128 a factor
    that no longer fits one LDS chunk (three chunks of factor rows at ld = 128)"""
    from dqc_amd import lib
    h = _case("benzene-ccpvdz")[0]
    rng = np.random.default_rng(100 + r)
    orb = torch.linalg.qr(torch.as_tensor(rng.standard_normal((h.nao, r)), device=dev))[0].contiguous()
    w = torch.as_tensor(rng.uniform(0.1, 2.0, r), device=dev)
    dm = h.ao_orb2dm(orb, w)
    fac = h._factor_of(dm)
    assert fac is not None and len(fac) == 1 and fac[0][0].shape[1] == lib.padded_norb(r)
    dao = (h._orthozer @ (orb * w) @ orb.T @ h._orthozer.T).cpu().numpy()
    kref = _k_ref(h, (dao + dao.T) * 0.5)
    k = h.df.exchange_ao(None, fac).cpu().numpy()
    print("df_exchange benzene r %d rp %d: max|K| %.3f  max|K - K_ref| %.2e" % (r, fac[0][0].shape[1], np.abs(kref).max(), np.abs(k - kref).max()))
    assert np.abs(k - kref).max() < 1e-10


def test_factor_panels(dev):
    """the benzene factor split into two panels (11 + 10 columns) gives the K of one panel to 1e-12"""
    from dqc_amd import lib
    h, orb, w, kref = _case("benzene-ccpvdz")
    one = h._factor_of(h.ao_orb2dm(orb, w))
    l_ao = one[0][0][:h._nao_ao, :orb.shape[1]]
    panels = [lib.pad_factor(l_ao[:, :11].contiguous(), h._ld), lib.pad_factor(l_ao[:, 11:].contiguous(), h._ld)]
    k1, k2 = h.df.exchange_ao(None, one), h.df.exchange_ao(None, panels)
    print("panels: max|K_2 - K_1| %.2e" % float((k1 - k2).abs().max()))
    assert float((k1 - k2).abs().max()) < 1e-12
    assert np.abs(k2.cpu().numpy() - kref).max() < 1e-10


def test_anonymous_density_takes_the_torch_form(dev):
    """a density that did not come from ao_orb2dm: sum_P B_P D B_P as batched matmul, the same 1e-10 bar, no kernel call"""
    from dqc_amd import lib
    for name in ("h2o-321g", "benzene-ccpvdz"):
        h, orb, w, kref = _case(name)
        dm = ((orb * w) @ orb.T).contiguous()
        assert h._factor_of(dm) is None
        before = dict(h.grid_path_counts)
        with lib.call_trace() as tr:
            kx = h.get_exchange(dm).fullmatrix()
        assert not any(r[0] == "dqc_df_exchange" for r in tr.rows)
        assert h.grid_path_counts == before
        sx = h._ovlp_ao @ h._orthozer
        err = np.abs((sx @ kx @ sx.T).cpu().numpy() + 0.5 * kref).max()
        print("torch form %s: max|K - K_ref| / 2 %.2e" % (name, err))
        assert err < 0.5e-10


def test_deterministic_mode_is_bit_reproducible(dev):
    from dqc_amd import lib
    h, orb, w, kref = _case("benzene-ccpvdz")
    fac = h._factor_of(h.ao_orb2dm(orb, w))
    k0 = h.df.exchange_ao(None, fac).clone()
    prev = lib.set_deterministic(True)
    try:
        k1 = h.df.exchange_ao(None, fac).clone()
        k2 = h.df.exchange_ao(None, fac).clone()
    finally:
        lib.set_deterministic(prev)
    assert torch.equal(k1, k2)
    print("deterministic: max|K_det - K| %.2e" % float((k1 - k0).abs().max()))
    assert float((k1 - k0).abs().max()) < 1e-10
    assert np.abs(k1.cpu().numpy() - kref).max() < 1e-10


# ------------------------------------------------------------------------------------------------ 2. Fock builds
@pytest.fixture(scope="module")
def h2o_builds(dev):
    """H2O / cc-pVDZ: the fitted Hamiltonian's J_df and K_ref of seeded densities, AO basis, on the host"""
    import dqc_amd
    m = dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2").densityfit(auxbasis="etb", exchange=True)
    h = m.get_hamiltonian().build()
    S = h._ovlp_ao.cpu().numpy()
    ds = {seed: M.seeded_dm_ao(h._nao_ao, nel, S, seed) * sc for seed, nel, sc in ((31, 10, 1.0), (32, 10, 0.5), (33, 8, 0.5))}
    j = {seed: h.df.coulomb_ao(torch.as_tensor(d, device=dev)).cpu().numpy() for seed, d in ds.items()}
    k = {seed: _k_ref(h, d) for seed, d in ds.items()}
    return m, ds, j, k


def _ao_op(h, m):
    sx = h._ovlp_ao @ h._orthozer
    return (sx @ m @ sx.T).cpu().numpy()


def test_rhf_build(dev, h2o_builds):
    """HF on the fitted Hamiltonian: dm2scp - core == X^T (J_df - K_ref / 2) X, and dm2energy == the sum of energy_parts"""
    import dqc_amd
    m, ds, j, k = h2o_builds
    eng = dqc_amd.HF(m)._engine
    h = eng.hamilton
    dm = _orth_dm(h, ds[31])
    f = eng.dm2scp(dm) - eng._core_matrix()
    err = np.abs(_ao_op(h, f) - (j[31] - 0.5 * k[31])).max()
    p = eng.energy_parts(dm)
    de = abs(float(eng.dm2energy(dm)) - p["e_tot"])
    print("RI-HF build: max|dF| %.2e  |dm2energy - sum parts| %.2e" % (err, de))
    assert err < 1e-9 and de < 1e-9
    assert abs(p["e_exch"] + 0.25 * float(np.sum(k[31] * ds[31]))) < 1e-9
    # the same density through ao_orb2dm: the build takes the kernel, same Fock matrix
    from dqc_amd import lib
    w, c = torch.linalg.eigh((dm + dm.T) * 0.5)
    dm2 = h.ao_orb2dm(c[:, -5:].contiguous(), w[-5:].contiguous())
    with lib.call_trace() as tr:
        f2 = eng.dm2scp(dm2) - eng._core_matrix()
    assert any(r[0] == "dqc_df_exchange" for r in tr.rows)
    assert np.abs(_ao_op(h, f2) - (j[31] - 0.5 * k[31])).max() < 1e-9


def test_uhf_build(dev, h2o_builds):
    """the unrestricted pair: J_df of the total density, -K_ref[D_s] per spin"""
    import dqc_amd
    from dqc_amd.utils.datastruct import SpinParam
    m, ds, j, k = h2o_builds
    eng = dqc_amd.HF(m, restricted=False)._engine
    h = eng.hamilton
    pair = SpinParam(u=_orth_dm(h, ds[32]), d=_orth_dm(h, ds[33]))
    f = eng.dm2scp(pair) - eng._core_matrix()
    jt = j[32] + j[33]
    errs = [np.abs(_ao_op(h, f[s]) - (jt - k[seed])).max() for s, seed in enumerate((32, 33))]
    p = eng.energy_parts(pair)
    de = abs(float(eng.dm2energy(pair)) - p["e_tot"])
    print("RI-UHF build: max|dF| %s  |dm2energy - sum parts| %.2e" % (errs, de))
    assert max(errs) < 1e-9 and de < 1e-9


@pytest.mark.parametrize("restricted", [True, False])
def test_pbe0_build_equals_the_operators_sum(dev, h2o_builds, restricted):
    """RI-PBE0: dm2scp == core + get_elrep + 0.25 get_exchange + get_vxc of the same Hamiltonian; dm2energy == sum of parts"""
    import dqc_amd
    from dqc_amd.utils.datastruct import SpinParam
    m, ds, j, k = h2o_builds
    eng = dqc_amd.KS(m, xc="pbe0", restricted=restricted)._engine
    h = eng.hamilton
    assert eng.exx == 0.25
    if restricted:
        dm = _orth_dm(h, ds[31])
        f = eng.dm2scp(dm)
        d2 = dm.clone()
        ref = (h.get_kinnucl() + h.get_elrep(d2) + h.get_vxc(d2)).fullmatrix() + 0.25 * h.get_exchange(d2).fullmatrix()
        err = float((f - ref).abs().max())
        # and the exchange part against the host reference
        kx = _ao_op(h, h.get_exchange(d2).fullmatrix())
        assert np.abs(kx + 0.5 * k[31]).max() < 1e-10
    else:
        dm = SpinParam(u=_orth_dm(h, ds[32]), d=_orth_dm(h, ds[33]))
        f = eng.dm2scp(dm)
        d2 = SpinParam(u=dm.u.clone(), d=dm.d.clone())
        core = (h.get_kinnucl() + h.get_elrep(d2.u + d2.d)).fullmatrix()
        v, kx = h.get_vxc(d2), h.get_exchange(d2)
        ref = torch.stack([core + v.u.fullmatrix() + 0.25 * kx.u.fullmatrix(), core + v.d.fullmatrix() + 0.25 * kx.d.fullmatrix()])
        err = float((f - ref).abs().max())
        assert max(np.abs(_ao_op(h, kx.u.fullmatrix()) + k[32]).max(), np.abs(_ao_op(h, kx.d.fullmatrix()) + k[33]).max()) < 1e-10
    p = eng.energy_parts(dm)
    de = abs(float(eng.dm2energy(dm)) - p["e_tot"])
    print("RI-PBE0 build restricted=%s: max|dF| %.2e  |dm2energy - sum parts| %.2e" % (restricted, err, de))
    assert err < 1e-9 and de < 1e-9


# ------------------------------------------------------------------------------------------------ 3. converged energies
@pytest.mark.parametrize("name", ["h2o-ccpvdz-rihf", "h2o-ccpvdz-ripbe0", "ch3-321g-riuhf", "ch3-321g-riupbe0"])
def test_converged_energies(dev, golden, name):
    import dqc_amd
    c = golden["converged"][name]
    spin = c["spin"]
    m = dqc_amd.Mol((c["atomzs"], c["atompos"]), basis=c["basis"], grid=c["grid"], **({"spin": spin} if spin else {}))
    m.densityfit(auxbasis="etb", exchange=True)
    assert m.get_hamiltonian().df.exchange
    qc = dqc_amd.HF(m) if c["functional"] == "hf" else dqc_amd.KS(m, xc=c["functional"])
    qc.run(fwd_options=TIGHT)
    assert qc.accepted
    e = float(qc.energy())
    p = qc._engine.energy_parts(qc.aodm())
    print("%s: E %.10f  golden %.10f  diff %.2e  (driver %s, %d iterations)" % (name, e, c["e_tot"], e - c["e_tot"], qc.driver_used, qc.niter))
    assert m.get_hamiltonian().df.j2c.shape[0] == c["naux"]
    assert abs(e - c["e_tot"]) < 1e-8
    print("   e_exch %.10f  golden %.10f" % (p["e_exch"], c["e_exch"]))
    if name.startswith("h2o"):  # E_K of the converged density (a E_K in the golden file of the hybrid)
        a = 1.0 if c["functional"] == "hf" else 0.25
        assert abs(a * float(m.get_hamiltonian().get_e_exchange(qc.aodm())) - c["e_exch"]) < 1e-8


def test_eager_and_graph_drivers_agree(dev, golden):
    """RI-PBE0 on H2O through the eager host loop (graph: False) == the golden energy as well"""
    import dqc_amd
    c = golden["converged"]["h2o-ccpvdz-ripbe0"]
    m = dqc_amd.Mol((c["atomzs"], c["atompos"]), basis=c["basis"], grid=c["grid"]).densityfit(auxbasis="etb", exchange=True)
    qc = dqc_amd.KS(m, xc="pbe0").run(fwd_options=dict(TIGHT, graph=False))
    assert qc.accepted and qc.driver_used == "host"
    assert abs(float(qc.energy()) - c["e_tot"]) < 1e-8
    m2 = dqc_amd.Mol((c["atomzs"], c["atompos"]), basis=c["basis"], grid=c["grid"]).densityfit(auxbasis="etb", exchange=True)
    qm = dqc_amd.KS(m2, xc="0.25 * hf + 0.75 * gga_x_pbe + gga_c_pbe").run(fwd_options=TIGHT)
    assert abs(float(qm.energy()) - c["e_tot"]) < 1e-8


# ------------------------------------------------------------------------------------------------ 4. refusals and defaults
def test_refusals_and_defaults(dev):
    import dqc_amd
    from dqc_amd import lib
    m = dqc_amd.Mol(H2, basis="3-21G").densityfit(auxbasis="etb")
    h = m.get_hamiltonian().build()
    assert h.df is not None and not h.df.exchange and not h.df.dfinfo.exchange
    dm = torch.eye(h.nao, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError):
        h.get_exchange(dm)
    with pytest.raises(NotImplementedError):
        dqc_amd.KS(dqc_amd.Mol(H2, basis="3-21G", grid="sg2").densityfit(auxbasis="etb"), xc="pbe0")
    with pytest.raises(NotImplementedError):
        dqc_amd.Mol(H2, basis="3-21G").densityfit(method="overlap", auxbasis="etb", exchange=True).get_hamiltonian().build()
    mk = dqc_amd.Mol(H2, basis="3-21G").densityfit(auxbasis="etb", exchange=True)
    qc = dqc_amd.HF(mk).run()
    with pytest.raises(NotImplementedError, match="fitted exchange"):
        qc.nuclear_gradient()
    # argument checks of the binding: nothing is launched
    hk, orb, w, _ = _case("h2-321g")
    pair = hk._factor_of(hk.ao_orb2dm(orb, w))[0]
    with pytest.raises(lib.DqcAmdError):
        lib.df_exchange(hk.df._b, pair, naux=-1)
    tall = (torch.zeros((pair[0].shape[0] + 16, pair[0].shape[1]), dtype=torch.float64, device=dev), None)
    with pytest.raises(lib.DqcAmdError):
        lib.df_exchange(hk.df._b, tall)
    L = lib.load()
    assert L.dqc_df_exchange(None, None, None, None, 4, -1, 16, None, None) != 0   # the C entry point refuses a negative naux itself
    assert L.dqc_df_exchange(None, None, None, None, 4, 40, 20, None, None) != 0   # and a width that is no padded factor width
