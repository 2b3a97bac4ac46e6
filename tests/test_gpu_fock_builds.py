"""The two-electron Fock builds of HamiltonMI355 (`_fock2e`, `_fock2e_pol` behind the public get_elrep_plus_* names), flavour by
flavour: Hartree-Fock, LDA, GGA, meta-GGA, a hybrid, and the two unrestricted ones, each with a density whose orbital factor is
known (ao_orb2dm) and with an anonymous clone of it, fused (csrc/fock.hip) and in the torch form (DQC_AMD_FUSED_FOCK=0).

1. The library entry points one build + dm2energy goes through, in order, are pinned as literals (SEQUENCES).  They were recorded
   before the six hand-written builds were folded into two: the same entry points in the same order are the same launches with
   the same host work between them.  A sequence that differs is a finding about the build, not a literal to update.
2. The same numbers as the operators' own sum (1e-11 on the matrix, 1e-10 Ha on the energy: the bounds
   test_fused_and_torch_forms_of_the_hybrid_build_agree holds).
3. The exact-exchange energy remembered by an unrestricted hybrid build goes when the functional changes.
4. timed_fock_kernels is the restricted Kohn-Sham build with its six stages marked.

Fixture: H2O / cc-pVDZ / sg2 (nao 24: d shells, a real grid, every functional family), seeded densities (molecules.seeded_dm_ao)."""
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

PBE = "gga_x_pbe + gga_c_pbe"
# flavour -> (functional or None: Hartree-Fock, restricted)
FLAVOURS = {"rhf": (None, True), "lda": ("lda_x + lda_c_pw", True), "pbe": (PBE, True), "scan": ("mgga_x_scan + mgga_c_scan", True),
            "pbe0": ("pbe0", True), "upbe": (PBE, False), "upbe0": ("pbe0", False)}
HF37PBE = "0.37 * hf + 0.63 * gga_x_pbe + gga_c_pbe"

# (flavour, factor known, fused) -> the entry points of eng.dm2scp(dm); eng.dm2energy(dm), as lib.call_trace names them
SEQUENCES = {
    ("rhf", True, True): ["dqc_fock_prep", "dqc_jk_from_tiles", "dqc_fock_finish"],
    ("rhf", True, False): ["dqc_jk_from_tiles"],
    ("rhf", False, True): ["dqc_fock_prep", "dqc_jk_from_tiles", "dqc_fock_finish"],
    ("rhf", False, False): ["dqc_jk_from_tiles"],
    ("lda", True, True): ["dqc_fock_prep", "dqc_jk_from_tiles[J only]", "dqc_grid_density_lr[value only]", "dqc_xc_eval_quad",
                          "dqc_grid_vxc[no gradient term]", "dqc_fock_finish"],
    ("lda", True, False): ["dqc_jk_from_tiles", "dqc_grid_density_lr[value only]", "dqc_xc_eval_quad", "dqc_grid_vxc[no gradient term]"],
    ("lda", False, True): ["dqc_fock_prep", "dqc_jk_from_tiles[J only]", "dqc_grid_density[value only]", "dqc_xc_eval_quad",
                           "dqc_grid_vxc[no gradient term]", "dqc_fock_finish"],
    ("lda", False, False): ["dqc_jk_from_tiles", "dqc_grid_density[value only]", "dqc_xc_eval_quad", "dqc_grid_vxc[no gradient term]"],
    ("pbe", True, True): ["dqc_fock_prep", "dqc_jk_from_tiles[J only]", "dqc_grid_density_lr", "dqc_xc_eval_quad", "dqc_grid_vxc",
                          "dqc_fock_finish"],
    ("pbe", True, False): ["dqc_jk_from_tiles", "dqc_grid_density_lr", "dqc_xc_eval_quad", "dqc_grid_vxc"],
    ("pbe", False, True): ["dqc_fock_prep", "dqc_jk_from_tiles[J only]", "dqc_grid_density", "dqc_xc_eval_quad", "dqc_grid_vxc",
                           "dqc_fock_finish"],
    ("pbe", False, False): ["dqc_jk_from_tiles", "dqc_grid_density", "dqc_xc_eval_quad", "dqc_grid_vxc"],
    ("scan", True, True): ["dqc_fock_prep", "dqc_jk_from_tiles[J only]", "dqc_grid_density_lr_tau", "dqc_xc_eval_mgga", "dqc_grid_vxc",
                           "dqc_grid_vxc_pair[three gradient components]", "dqc_fock_finish", "dqc_grid_density_lr_tau",
                           "dqc_xc_eval_mgga"],
    ("scan", True, False): ["dqc_jk_from_tiles", "dqc_grid_density_lr_tau", "dqc_xc_eval_mgga", "dqc_grid_vxc",
                            "dqc_grid_vxc_pair[three gradient components]", "dqc_grid_density_lr_tau", "dqc_xc_eval_mgga"],
    ("scan", False, True): ["dqc_fock_prep", "dqc_jk_from_tiles[J only]", "dqc_grid_density", "dqc_grid_density_pair",
                            "dqc_grid_density_pair", "dqc_grid_density_pair", "dqc_grid_density_pair", "dqc_xc_eval_mgga", "dqc_grid_vxc",
                            "dqc_grid_vxc_pair[three gradient components]", "dqc_fock_finish", "dqc_grid_density",
                            "dqc_grid_density_pair", "dqc_grid_density_pair", "dqc_grid_density_pair", "dqc_grid_density_pair",
                            "dqc_xc_eval_mgga"],
    ("scan", False, False): ["dqc_jk_from_tiles", "dqc_grid_density", "dqc_grid_density_pair", "dqc_grid_density_pair",
                             "dqc_grid_density_pair", "dqc_grid_density_pair", "dqc_xc_eval_mgga", "dqc_grid_vxc",
                             "dqc_grid_vxc_pair[three gradient components]", "dqc_grid_density", "dqc_grid_density_pair",
                             "dqc_grid_density_pair", "dqc_grid_density_pair", "dqc_grid_density_pair", "dqc_xc_eval_mgga"],
    ("pbe0", True, True): ["dqc_fock_prep", "dqc_jk_from_tiles", "dqc_grid_density_lr", "dqc_xc_eval_quad", "dqc_grid_vxc",
                           "dqc_fock_finish_hybrid"],
    ("pbe0", True, False): ["dqc_jk_from_tiles", "dqc_grid_density_lr", "dqc_xc_eval_quad", "dqc_grid_vxc"],
    ("pbe0", False, True): ["dqc_fock_prep", "dqc_jk_from_tiles", "dqc_grid_density", "dqc_xc_eval_quad", "dqc_grid_vxc",
                            "dqc_fock_finish_hybrid"],
    ("pbe0", False, False): ["dqc_jk_from_tiles", "dqc_grid_density", "dqc_xc_eval_quad", "dqc_grid_vxc"],
    ("upbe", True, True): ["dqc_fock_prep", "dqc_jk_from_tiles[J only]", "dqc_grid_density_lr_pol", "dqc_xc_eval_pol", "dqc_grid_vxc",
                           "dqc_grid_vxc", "dqc_fock_finish", "dqc_fock_finish", "dqc_jk_from_tiles", "dqc_grid_density_lr_pol",
                           "dqc_xc_eval_pol"],
    ("upbe", True, False): ["dqc_jk_from_tiles", "dqc_grid_density_lr_pol", "dqc_xc_eval_pol", "dqc_grid_vxc", "dqc_grid_vxc",
                            "dqc_jk_from_tiles", "dqc_grid_density_lr_pol", "dqc_xc_eval_pol"],
    ("upbe", False, True): ["dqc_jk_from_tiles", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol", "dqc_grid_vxc",
                            "dqc_grid_vxc", "dqc_jk_from_tiles", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol"],
    ("upbe", False, False): ["dqc_jk_from_tiles", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol", "dqc_grid_vxc",
                             "dqc_grid_vxc", "dqc_jk_from_tiles", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol"],
    ("upbe0", True, True): ["dqc_jk_from_tiles_multi", "dqc_grid_density_lr_pol", "dqc_xc_eval_pol", "dqc_grid_vxc", "dqc_grid_vxc",
                            "dqc_jk_from_tiles", "dqc_grid_density_lr_pol", "dqc_xc_eval_pol"],
    ("upbe0", True, False): ["dqc_jk_from_tiles_multi", "dqc_grid_density_lr_pol", "dqc_xc_eval_pol", "dqc_grid_vxc", "dqc_grid_vxc",
                             "dqc_jk_from_tiles", "dqc_grid_density_lr_pol", "dqc_xc_eval_pol"],
    ("upbe0", False, True): ["dqc_jk_from_tiles_multi", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol", "dqc_grid_vxc",
                             "dqc_grid_vxc", "dqc_jk_from_tiles", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol"],
    ("upbe0", False, False): ["dqc_jk_from_tiles_multi", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol", "dqc_grid_vxc",
                              "dqc_grid_vxc", "dqc_jk_from_tiles", "dqc_grid_density", "dqc_grid_density", "dqc_xc_eval_pol"],
}

_ENGINES, _REFS = {}, {}


def engine(flavour):
    """one engine (its own Mol and Hamiltonian) per flavour, shared by the cases"""
    import dqc_amd
    if flavour not in _ENGINES:
        xc, restricted = FLAVOURS[flavour]
        m = dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2")
        qc = dqc_amd.HF(m, restricted=restricted) if xc is None else dqc_amd.KS(m, xc=xc, restricted=restricted)
        _ENGINES[flavour] = qc._engine
    return _ENGINES[flavour]


def _with_factor(h, nel, seed, scale=1.0):
    """`scale` x the seeded density in the orthogonalised basis, out of ao_orb2dm: its eigenvectors of non-zero weight are the 'orbitals'"""
    sx = h._ovlp_ao @ h._orthozer
    d = sx.T @ torch.as_tensor(M.seeded_dm_ao(h._nao_ao, nel, h._ovlp_ao.cpu().numpy(), seed) * scale, device=h.device) @ sx
    w, v = torch.linalg.eigh((d + d.T) * 0.5)
    r = nel // 2
    dm = h.ao_orb2dm(v[:, -r:].contiguous(), w[-r:].contiguous())
    assert h._factor_of(dm) is not None
    return dm


def density(eng, known):
    """a density (restricted) or pair (unrestricted) for `eng`; `known`: its factor is remembered by the Hamiltonian, else a clone"""
    from dqc_amd.utils.datastruct import SpinParam
    h = eng.hamilton
    if eng.polarized:
        dm = SpinParam(u=_with_factor(h, 10, 111, 0.5), d=_with_factor(h, 8, 211, 0.5))
        return dm if known else SpinParam(u=dm.u.clone(), d=dm.d.clone())
    dm = _with_factor(h, 10, 11)
    return dm if known else dm.clone()


def operators_sum(eng, dm):
    """(Fock matrix from the operators' own sum, dm2energy) of a density nothing is remembered of"""
    from dqc_amd.utils.datastruct import SpinParam
    h, a = eng.hamilton, eng.exx if eng.is_ks else 1.0
    if eng.polarized:
        d = SpinParam(u=dm.u.clone(), d=dm.d.clone())
        core, v = h.get_kinnucl() + h.get_elrep(d.u + d.d), h.get_vxc(d)
        f = torch.stack([(core + v.u).fullmatrix(), (core + v.d).fullmatrix()])
        if a != 0.0:
            k = h.get_exchange(d)
            f = f + a * torch.stack([k.u.fullmatrix(), k.d.fullmatrix()])
    else:
        d = dm.clone()
        f = (h.get_kinnucl() + h.get_elrep(d)).fullmatrix()
        if a != 0.0:
            f = f + a * h.get_exchange(d).fullmatrix()
        if eng.is_ks:
            f = f + h.get_vxc(d).fullmatrix()
    return f, float(eng.dm2energy(d))


def traced_build(eng, dm):
    from dqc_amd import lib
    with lib.call_trace() as tr:
        f = eng.dm2scp(dm)
        e = eng.dm2energy(dm)
    return [r[0] for r in tr.rows], f, float(e)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    _ENGINES.clear()
    _REFS.clear()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
@pytest.mark.parametrize("known", [True, False], ids=["factor", "anonymous"])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_build_takes_the_pinned_calls_and_equals_the_operators_sum(dev, monkeypatch, flavour, known, fused):
    monkeypatch.setenv("DQC_AMD_FUSED_FOCK", "1" if fused else "0")
    eng = engine(flavour)
    dm = density(eng, known)
    calls, f, e = traced_build(eng, dm)
    if flavour not in _REFS:  # (once per flavour: the four cases see the same numbers)
        _REFS[flavour] = operators_sum(eng, dm)
    f_ref, e_ref = _REFS[flavour]
    err_f, err_e = float((f - f_ref).abs().max()), abs(e - e_ref)
    print("%s factor %d fused %d: max|dF| %.2e  |dE| %.2e  calls %s" % (flavour, known, fused, err_f, err_e, calls))
    assert calls == SEQUENCES[(flavour, known, fused)]
    assert err_f < 1e-11
    assert err_e < 1e-10


def test_exchange_energy_of_an_unrestricted_hybrid_build_goes_with_the_functional(dev):
    """a pair built with PBE0, then another hybrid (a = 0.37) set on the same grid of the same Hamiltonian: get_e_exchange_hybrid(pair)
    is 0.37 E_K.  While the unrestricted build kept its a E_K in a memo of its own, which the change of functional did not clear,
    this returned the 0.25 E_K of the PBE0 build"""
    import dqc_amd
    from dqc_amd.xc import get_xc
    eng = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg2"), xc="pbe0", restricted=False)._engine
    h = eng.hamilton
    pair = density(eng, True)
    eng.dm2scp(pair)
    assert abs(float(h.get_e_exchange_hybrid(pair)) - 0.25 * float(h.get_e_exchange(pair))) < 1e-10
    h.setup_grid(h.grid, get_xc(HF37PBE))
    assert h.exx_fraction == 0.37
    got, ref = float(h.get_e_exchange_hybrid(pair)), 0.37 * float(h.get_e_exchange(pair))
    print("a E_K after the change of functional: %.12f  0.37 E_K: %.12f" % (got, ref))
    assert abs(got - ref) < 1e-10


def test_timed_fock_kernels_names_its_six_stages(dev):
    eng = engine("pbe")
    names, ev = eng.hamilton.timed_fock_kernels(density(eng, True), eng.knvext.fullmatrix())
    assert names == ["orth_transforms", "jk_tiles", "grid_density", "xc_eval", "grid_vxc", "fock_assemble"] and len(ev) == 7
