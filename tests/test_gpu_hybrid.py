"""Hybrid Kohn-Sham functionals (exact-exchange fraction a: PBE0, B3LYP5, "a * hf + ...") on the GPU.

The reference has no hybrid functionals, so the yardstick is a CPU hybrid SCF composed from the oracle's own, separately pinned
operators, F = h + J + a get_exchange(D) + Vxc[f_a](D) (tools/make_hybrid_golden.py -> tests/golden/oracle_hybrid.json and
oracle_hybrid_builds.npz).  Tolerances: 1e-9 on a Fock matrix (the parity suite holds 1e-10 on J and K, 1e-9 on Vxc), 1e-8 Ha on
energies (the standing bar for converged energies), 2e-6 on forces against the oracle's h = 1e-3 central differences (the O(h^2)
error of the stencil), 1e-6 against central differences of the GPU energy."""
import json
import os

import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

TIGHT = {"f_tol": 1e-11, "maxiter": 300}
XC = {"pbe0": "pbe0", "b3lyp5": "hyb_gga_xc_b3lyp5", "hf37pbe": "0.37 * hf + 0.63 * gga_x_pbe + gga_c_pbe"}
FRACTION = {"pbe0": 0.25, "b3lyp5": 0.2, "hf37pbe": 0.37}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "oracle_hybrid.json")))


def _orth_dm(h, d_ao):
    """AO-basis density (numpy) -> the orthogonalised basis of the Hamiltonian `h`"""
    sx = h._ovlp_ao @ h._orthozer
    return (sx.T @ torch.as_tensor(d_ao, device=h.device) @ sx).contiguous()


def _ao_op(h, m):
    sx = h._ovlp_ao @ h._orthozer
    return (sx @ m @ sx.T).cpu().numpy()


def _mol(c, **kw):
    import dqc_amd
    spin = c.get("spin")
    return dqc_amd.Mol((c["atomzs"], c["atompos"]), basis=c["basis"], grid=c["grid"], **({"spin": spin} if spin else {}), **kw)


# ------------------------------------------------------------------------------------------------ 1. single build
@pytest.mark.parametrize("fn", ["pbe0", "b3lyp5", "hf37pbe"])
@pytest.mark.parametrize("name", ["h2o", "benzene"])
def test_single_hybrid_build_equals_oracle_composition(dev, golden_dir, name, fn):
    """the fused hybrid Fock matrix (dqc_fock_finish_hybrid behind the J + K tile pass and the grid passes) and the energy parts
    of a seeded density == the oracle composition; restricted, and for H2O both spin blocks of the unrestricted build"""
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.utils.datastruct import SpinParam
    g = np.load(os.path.join(golden_dir, "oracle_hybrid_builds.npz"))
    mol, seed = {"h2o": (M.H2O, 11), "benzene": (M.benzene(), 12)}[name]
    nel = int(sum(mol[0]))
    m = dqc_amd.Mol(mol, basis="cc-pvdz", grid="sg2")
    qc = dqc_amd.KS(m, xc=XC[fn])
    eng, h = qc._engine, qc._engine.hamilton
    assert eng.exx == FRACTION[fn] and h.exx_fraction == FRACTION[fn]
    S = h._ovlp_ao.cpu().numpy()
    dm = _orth_dm(h, M.seeded_dm_ao(h._nao_ao, nel, S, seed))
    with lib.call_trace() as tr:
        f = eng.dm2scp(dm)
    assert any(r[0] == "dqc_fock_finish_hybrid" for r in tr.rows)  # the new kernel ran, not a torch sum
    p = eng.energy_parts(dm)
    ref_f, ref_p = g["%s_%s_fock_ao" % (name, fn)], g["%s_%s_parts" % (name, fn)]
    err_f = np.abs(_ao_op(h, f) - ref_f).max()
    got = np.array([p["e_core"], p["e_elrep"], p["e_exch"], p["e_xc"]])
    print("single build %s %s: max|dF| %.2e  |dE parts| %s" % (name, fn, err_f, np.abs(got - ref_p)))
    assert err_f < 1e-9
    assert np.abs(got - ref_p).max() < 1e-8
    # the build's own by-products == the operators' separate energies
    assert abs(float(eng.dm2energy(dm)) - (got.sum() + p["e_nuc"])) < 1e-9
    if name != "h2o":
        return
    qu = dqc_amd.KS(m, xc=XC[fn], restricted=False)
    eu, hu = qu._engine, qu._engine.hamilton
    du = _orth_dm(hu, M.seeded_dm_ao(hu._nao_ao, nel, S, seed + 100)) * 0.5
    dd = _orth_dm(hu, M.seeded_dm_ao(hu._nao_ao, nel - 2, S, seed + 200)) * 0.5
    pair = SpinParam(u=du, d=dd)
    fu = eu.dm2scp(pair)
    pu = eu.energy_parts(pair)
    ref_f, ref_p = g["h2o_%s_ufock_ao" % fn], g["h2o_%s_uparts" % fn]
    errs = [np.abs(_ao_op(hu, fu[s]) - ref_f[s]).max() for s in range(2)]
    got = np.array([pu["e_core"], pu["e_elrep"], pu["e_exch"], pu["e_xc"]])
    print("single build h2o %s unrestricted: max|dF| %s  |dE parts| %s" % (fn, errs, np.abs(got - ref_p)))
    assert max(errs) < 1e-9
    assert np.abs(got - ref_p).max() < 1e-8


def test_fused_and_torch_forms_of_the_hybrid_build_agree(dev, monkeypatch):
    """DQC_AMD_FUSED_FOCK=0 takes the torch form of the same sum (what the fused kernels are tested against)"""
    import dqc_amd
    m = dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2")
    eng = dqc_amd.KS(m, xc="pbe0")._engine
    h = eng.hamilton
    dm = _orth_dm(h, M.seeded_dm_ao(h._nao_ao, 10, h._ovlp_ao.cpu().numpy(), 5))
    f1, e1 = eng.dm2scp(dm), float(eng.dm2energy(dm))
    monkeypatch.setenv("DQC_AMD_FUSED_FOCK", "0")
    dm2 = dm.clone()
    f2, e2 = eng.dm2scp(dm2), float(eng.dm2energy(dm2))
    assert float((f1 - f2).abs().max()) < 1e-11 and abs(e1 - e2) < 1e-10
    # and the operators' own sum
    a = eng.exx
    dm3 = dm.clone()
    f3 = (h.get_kinnucl() + h.get_elrep(dm3) + h.get_vxc(dm3)).fullmatrix() + a * h.get_exchange(dm3).fullmatrix()
    assert float((f1 - f3).abs().max()) < 1e-11


# ------------------------------------------------------------------------------------------------ 2. limits
def test_pure_hf_limit_and_zero_fraction_limit(dev):
    """"1.0 * hf" alone is Hartree-Fock: Fock matrix and energy of dqc_amd.HF on the same density to 1e-12 (run in deterministic
    mode, so that the two tile passes accumulate in the same order and the comparison sees the finish kernels alone);
    "0 * hf + gga_x_pbe + gga_c_pbe" takes the pure-PBE path: bit for bit in deterministic mode"""
    import dqc_amd
    from dqc_amd import lib
    prev = lib.set_deterministic(True)
    try:
        m = dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2")
        hf = dqc_amd.HF(m)._engine
        hy = dqc_amd.KS(m, xc="1.0 * hf")._engine
        assert hy.exx == 1.0
        h = hf.hamilton
        d_ao = M.seeded_dm_ao(h._nao_ao, 10, h._ovlp_ao.cpu().numpy(), 3)
        d1, d2 = _orth_dm(h, d_ao), _orth_dm(hy.hamilton, d_ao)
        f1, f2 = hf.dm2scp(d1), hy.dm2scp(d2)
        e1, e2 = float(hf.dm2energy(d1)), float(hy.dm2energy(d2))
        print("a = 1 limit: max|dF| %.2e  |dE| %.2e" % (float((f1 - f2).abs().max()), abs(e1 - e2)))
        assert float((f1 - f2).abs().max()) < 1e-12 and abs(e1 - e2) < 1e-12
        p = hy.energy_parts(d2)
        assert p["e_xc"] == 0.0 and abs(p["e_exch"] - float(h.get_e_exchange(d1))) < 1e-12
        # a = 0: the old path, the old bits
        m2 = dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2")
        pure = dqc_amd.KS(m2, xc="gga_x_pbe + gga_c_pbe")._engine
        zero = dqc_amd.KS(m2, xc="0 * hf + gga_x_pbe + gga_c_pbe")._engine
        assert zero.exx == 0.0
        da, db = _orth_dm(pure.hamilton, d_ao), _orth_dm(zero.hamilton, d_ao)
        with lib.call_trace() as tr:
            fb = zero.dm2scp(db)
        assert not any(r[0] == "dqc_fock_finish_hybrid" for r in tr.rows)
        fa = pure.dm2scp(da)
        assert torch.equal(fa, fb)
        assert float(pure.dm2energy(da)) == float(zero.dm2energy(db))
    finally:
        lib.set_deterministic(prev)


def test_closed_shell_uks_hybrid_equals_rks_hybrid(dev):
    import dqc_amd
    m = dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2")
    r = dqc_amd.KS(m, xc="pbe0").run(fwd_options=TIGHT)
    u = dqc_amd.KS(m, xc="pbe0", restricted=False).run(fwd_options=TIGHT)
    assert r.accepted and u.accepted
    print("closed shell: E(RKS) %.12f  E(UKS) %.12f" % (float(r.energy()), float(u.energy())))
    assert abs(float(r.energy()) - float(u.energy())) < 1e-9


# ------------------------------------------------------------------------------------------------ 3. converged energies
RESTRICTED = ["h2o-321g-pbe0", "h2o-321g-b3lyp5", "lih-321g-pbe0", "lih-321g-b3lyp5", "h2o-ccpvdz-pbe0"]
UNRESTRICTED = ["ch3-321g-upbe0", "ch3-321g-ub3lyp5"]


@pytest.mark.parametrize("driver", ["host", "device"])
@pytest.mark.parametrize("name", RESTRICTED + UNRESTRICTED)
def test_converged_hybrid_energy_equals_golden(dev, golden, name, driver):
    """PBE0 and B3LYP5, restricted and unrestricted, through the host-driven loop and the device-resident (one hipGraph per
    iteration) loop: total energy, energy parts, and the converged AO density"""
    import dqc_amd
    c = golden["converged"][name]
    qc = dqc_amd.KS(_mol(c), xc=XC[c["functional"]]).run(fwd_options={"f_tol": 1e-10, "maxiter": 200, "driver": driver})
    assert qc.accepted
    if driver == "host" or name == "h2o-ccpvdz-pbe0":  # (the device loop may hand a run over to the host loop; this one it finishes)
        assert qc.driver_used == driver
    e = float(qc.energy())
    p = qc._engine.energy_parts(qc.aodm())
    print("%s [%s]: E %.12f  golden %.12f  diff %.2e  niter %d" % (name, driver, e, c["e_tot"], e - c["e_tot"], qc.niter))
    assert abs(e - c["e_tot"]) < 1e-8
    for k in ("e_core", "e_elrep", "e_exch", "e_xc"):
        assert abs(p[k] - c[k]) < 1e-6, k  # (non-variational parts: first order in the density error)
    h = qc._engine.hamilton
    x = h._orthozer
    dm = qc.aodm()
    ds = [dm.u, dm.d] if c["spin"] is not None else [dm]
    ref = c["dm_ao"] if c["spin"] is not None else [c["dm_ao"]]
    for d, r in zip(ds, ref):
        assert np.abs((x @ d @ x.T).cpu().numpy() - np.array(r)).max() < 1e-6


def test_lockstep_batch_of_hybrid_molecules(dev, golden):
    """run_lockstep with a mixed batch: two functionals on two restricted molecules (each bucket advances in lockstep), and the
    unrestricted radical"""
    import dqc_amd
    from dqc_amd.batch import run_lockstep
    names = ["h2o-321g-pbe0", "h2o-321g-b3lyp5", "lih-321g-pbe0", "lih-321g-b3lyp5", "ch3-321g-upbe0", "ch3-321g-ub3lyp5"]
    qcs = [dqc_amd.KS(_mol(golden["converged"][n]), xc=XC[golden["converged"][n]["functional"]]) for n in names]
    run_lockstep(qcs, fwd_options={"f_tol": 1e-10, "maxiter": 200})
    for n, qc in zip(names, qcs):
        e, ref = float(qc.energy()), golden["converged"][n]["e_tot"]
        print("lockstep %s: E %.12f  diff %.2e  niter %d" % (n, e, e - ref, qc.niter))
        assert qc.accepted
        assert abs(e - ref) < 1e-8


# ------------------------------------------------------------------------------------------------ 4. forces
@pytest.mark.parametrize("name", ["h2o-321g-pbe0", "ch3-321g-upbe0"])
def test_hybrid_forces_vs_oracle_finite_differences_and_autograd(dev, golden, name):
    """nuclear_gradient() of PBE0 == central differences (h = 1e-3) of the oracle-composed SCF energy, Becke cut off on both
    sides as in test_nuclear_gradient_vs_oracle_finite_differences; translational invariance; torch.autograd.grad == the same"""
    import dqc_amd
    import dqc_amd.grid as G
    c = golden["gradients"][name]
    G._BECKE_CUT = 2.0
    try:
        pos = torch.tensor(c["atompos"], dtype=torch.float64, requires_grad=True)
        m = dqc_amd.Mol((c["atomzs"], pos), basis=c["basis"], grid=c["grid"], **({"spin": c["spin"]} if c["spin"] else {}))
        qc = dqc_amd.KS(m, xc=XC[c["functional"]]).run(fwd_options=TIGHT)
        assert qc.accepted
        g = qc.nuclear_gradient().cpu()
        ga, = torch.autograd.grad(qc.energy(), pos)
    finally:
        G._BECKE_CUT = 0.74
    ref = np.array(c["gradient"])
    print("%s: max|g - fd| %.2e  |sum g| %.2e  |autograd - g| %.2e" % (name, np.abs(g.numpy() - ref).max(),
                                                                        float(g.sum(0).abs().max()), float((ga - g).abs().max())))
    assert float(g.sum(0).abs().max()) < 1e-10
    assert np.abs(g.numpy() - ref).max() < 2e-6
    assert float((ga - g).abs().max()) < 1e-12


def test_hybrid_forces_water_ccpvdz_vs_gpu_finite_differences(dev):
    """d shells in the derivative kernels with the exchange scale a: PBE0 against central differences of the GPU energy"""
    import dqc_amd
    import dqc_amd.grid as G
    zs, pos0 = [8, 1, 1], np.array([[0, 0, 0.2217], [0, 1.4309, -0.8867], [0.1, -1.4309, -0.8867]])
    G._BECKE_CUT = 2.0
    try:
        def run(p):
            m = dqc_amd.Mol((zs, p.tolist()), basis="cc-pvdz", grid="sg2")
            return dqc_amd.KS(m, xc="pbe0").run(fwd_options={"f_tol": 1e-11, "maxiter": 200})
        g = run(pos0).nuclear_gradient().cpu().numpy()
        gfd = np.zeros_like(pos0)
        for a in range(3):
            for d in range(3):
                e = []
                for sgn in (1, -1):
                    p = pos0.copy()
                    p[a, d] += sgn * 1e-3
                    e.append(float(run(p).energy()))
                gfd[a, d] = (e[0] - e[1]) / 2e-3
    finally:
        G._BECKE_CUT = 0.74
    print("cc-pVDZ PBE0: max|g - fd(GPU)| %.2e  |sum g| %.2e" % (np.abs(g - gfd).max(), np.abs(g.sum(0)).max()))
    assert np.abs(g - gfd).max() < 1e-6 and np.abs(g.sum(0)).max() < 1e-10


def test_xc_parameter_derivative_of_a_module_functional_with_fixed_fraction(dev):
    """a torch.nn.Module functional that sets exx_fraction itself: the SCF is a hybrid one, and dE/dp of its parameter is the
    central difference of the energy (the fraction is read as a float, it is not a parameter)"""
    import dqc_amd
    from dqc_amd.xc import BaseXC, get_xc

    class ScaledPBE(torch.nn.Module, BaseXC):
        exx_fraction = 0.25
        family = 2

        def __init__(self, p):
            super().__init__()
            self.p = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
            self.base = get_xc("0.75 * gga_x_pbe + gga_c_pbe")

        def get_edensityxc(self, densinfo):
            # (the 0-dim parameter enters as a scalar operand, as in the reference's PBE-like test functional: no host -> device
            # copy, which a graph capture of the SCF iteration would not allow)
            return self.base.get_edensityxc(densinfo) * self.p

        def get_vxc(self, densinfo):
            from dqc_amd.utils.datastruct import SpinParam
            return SpinParam.apply_fcn(lambda v: v * float(self.p.detach()), self.base.get_vxc(densinfo))

    def run(p):
        xc = ScaledPBE(p)
        m = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3)
        return dqc_amd.KS(m, xc=xc).run(fwd_options=TIGHT), xc

    qc, xc = run(1.0)
    assert qc._engine.exx == 0.25 and qc.accepted
    e = qc.energy()
    ref = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid=3), xc="pbe0").run(fwd_options=TIGHT)
    assert abs(float(e) - float(ref.energy())) < 1e-9
    g, = torch.autograd.grad(e, xc.p)
    # five-point central difference with h = 2e-2: the converged energies carry ~1e-10 Ha of SCF noise (seen against the goldens), which
    # a two-point stencil with h = 1e-4 turns into ~1e-6 of derivative noise; here the noise is ~1e-8 and the O(h^4) truncation error
    # h^4 / 30 |E^(5)| = 5e-9 |E^(5)|, both far inside the 1e-6 bound
    hh = 2e-2
    en = {k: float(run(1.0 + k * hh)[0].energy()) for k in (-2, -1, 1, 2)}
    fd = (-en[2] + 8 * en[1] - 8 * en[-1] + en[-2]) / (12 * hh)
    print("dE/dp %.10f  fd %.10f" % (float(g), fd))
    assert abs(float(g) - fd) < 1e-6


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(dev, monkeypatch):
    import dqc_amd
    m = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3)
    with pytest.raises(ValueError, match="hyb_gga_xc_b3lyp5"):
        dqc_amd.KS(m, xc="hyb_gga_xc_b3lyp")
    mdf = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3).densityfit(auxbasis="etb")
    with pytest.raises(NotImplementedError, match="fits the Coulomb operator J only"):
        dqc_amd.KS(mdf, xc="pbe0")
    dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid=3).densityfit(auxbasis="etb"), xc="gga_x_pbe + gga_c_pbe")  # (pure: still fine)
    monkeypatch.setenv("DQC_AMD_ERI", "direct")
    with pytest.raises(NotImplementedError, match="direct SCF"):
        dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid=3), xc="pbe0")
    monkeypatch.delenv("DQC_AMD_ERI")
    # a sharded Hamiltonian: the check itself (no multi-GPU machine: the rank count is set by hand)
    h = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3).get_hamiltonian()
    h._pworld = 2
    try:
        with pytest.raises(NotImplementedError, match="shard_over"):
            h._check_hybrid(0.25)
        h._check_hybrid(0.0)
    finally:
        h._pworld = 1


# ------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("restricted", [True, False])
def test_deterministic_hybrid_builds_are_bit_equal(dev, restricted):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.utils.datastruct import SpinParam
    prev = lib.set_deterministic(True)
    try:
        m = dqc_amd.Mol(M.benzene(), basis="cc-pvdz", grid="sg2")
        eng = dqc_amd.KS(m, xc="hyb_gga_xc_b3lyp5", restricted=restricted)._engine
        h = eng.hamilton
        S = h._ovlp_ao.cpu().numpy()
        if restricted:
            mk = lambda: _orth_dm(h, M.seeded_dm_ao(h._nao_ao, 42, S, 7))  # noqa: E731
        else:
            mk = lambda: SpinParam(u=_orth_dm(h, M.seeded_dm_ao(h._nao_ao, 42, S, 7)) * 0.5,  # noqa: E731
                                   d=_orth_dm(h, M.seeded_dm_ao(h._nao_ao, 40, S, 8)) * 0.5)
        d1, d2 = mk(), mk()
        f1, e1 = eng.dm2scp(d1), eng.dm2energy(d1)
        f2, e2 = eng.dm2scp(d2), eng.dm2energy(d2)
        assert torch.equal(f1, f2) and torch.equal(e1, e2)
    finally:
        lib.set_deterministic(prev)
