"""Hybrid functionals, the parts that need no GPU: the functional objects' exact-exchange fraction (dqc_amd/xc.py) and the
consistency of the oracle-composed fixtures (tools/make_hybrid_golden.py -> tests/golden/oracle_hybrid.json)."""
import json
import os

import numpy as np
import pytest

from dqc_amd import xc as X


def test_named_hybrids_resolve_to_their_terms_and_fractions():
    for name in ("pbe0", "hyb_gga_xc_pbeh", "PBE0"):
        f = X.get_xc(name)
        assert f.exx_fraction == 0.25 and f.family == 2
        assert sorted(f.terms) == sorted([(0.75, "gga_x_pbe"), (1.0, "gga_c_pbe")])
    f = X.get_xc("hyb_gga_xc_b3lyp5")
    assert f.exx_fraction == 0.20 and f.family == 2
    assert sorted(f.terms) == sorted([(0.08, "lda_x"), (0.72, "gga_x_b88"), (0.19, "lda_c_vwn"), (0.81, "gga_c_lyp")])


def test_hf_pseudo_term_adds_its_coefficient_and_no_grid_part():
    f = X.get_xc("0.25 * hf + 0.75 * gga_x_pbe + gga_c_pbe")
    assert f.exx_fraction == 0.25 and sorted(f.terms) == sorted(X.get_xc("pbe0").terms)
    assert X.get_xc("0.37*hf+0.63*gga_x_pbe+gga_c_pbe").exx_fraction == 0.37
    g = X.get_xc("1.0 * hf")
    assert g.exx_fraction == 1.0 and g.terms == [] and g.family == 1
    assert X.get_xc("hf + 0.5 * hf").exx_fraction == 1.5
    z = X.get_xc("0 * hf + gga_x_pbe + gga_c_pbe")
    assert z.exx_fraction == 0.0 and z.terms == X.get_xc("gga_x_pbe + gga_c_pbe").terms
    assert X.get_xc("0.5 * pbe0").exx_fraction == 0.125


def test_fraction_arithmetic_of_sum_and_scalar_multiple():
    a, b = X.get_xc("pbe0"), X.get_xc("hyb_gga_xc_b3lyp5")
    assert (a + b).exx_fraction == pytest.approx(0.45, abs=1e-15)
    assert (a * 2).exx_fraction == 0.5 and (2 * a).exx_fraction == 0.5
    assert (a + X.get_xc("lda_x")).exx_fraction == 0.25
    assert (X.get_xc("lda_x") * 3.0).exx_fraction == 0.0

    class Custom(X.BaseXC):  # a user functional that sets the attribute itself
        exx_fraction = 0.4
        family = 1

    c = Custom()
    assert X.exx_fraction_of(c) == 0.4
    assert (c + a).exx_fraction == pytest.approx(0.65, abs=1e-15)   # _SumXC
    assert (c * 0.5).exx_fraction == 0.2                            # _MulXC
    assert (c * 0.5 + a * 2).exx_fraction == pytest.approx(0.7, abs=1e-15)
    assert X.exx_fraction_of(None) == 0.0 and X.exx_fraction_of(object()) == 0.0


def test_every_existing_name_is_a_pure_functional():
    assert len(X._FAMILY) == 24
    for name in X._FAMILY:
        f = X.get_xc(name)
        assert f.exx_fraction == 0.0 and f.terms == [(1.0, name)]
    assert X.get_xc(None).exx_fraction == 0.0
    assert X.get_xc("lda_x + gga_c_pbe").exx_fraction == 0.0


def test_b3lyp_proper_is_refused_and_names_the_vwn5_variant():
    for name in ("hyb_gga_xc_b3lyp", "0.5 * hyb_gga_xc_b3lyp + lda_x"):
        with pytest.raises(ValueError, match="hyb_gga_xc_b3lyp5"):
            X.get_xc(name)


def test_golden_consistency_a1_without_grid_term_is_the_rhf_fixture(golden_dir):
    """the composed SCF with a = 1 and no grid term reproduces the oracle's RHF energy of the committed ref_h2o_sto3g_rhf fixture;
    every stored run is converged and its parts add up"""
    g = json.load(open(os.path.join(golden_dir, "oracle_hybrid.json")))
    ref = np.load(os.path.join(golden_dir, "ref_h2o_sto3g_rhf.npz"))
    c = g["converged"]["h2o-sto3g-hf"]
    assert abs(c["e_tot"] - float(ref["e_tot"])) < 1e-10
    assert abs(c["e_exch"] - float(ref["e_exch"])) < 1e-9 and c["e_xc"] == 0.0
    assert np.abs(np.array(c["dm_ao"]) - ref["dm_conv_ao"]).max() < 1e-8
    for name, c in g["converged"].items():
        assert c["commutator"] < 1e-10, name
        assert abs(c["e_core"] + c["e_elrep"] + c["e_nuc"] + c["e_exch"] + c["e_xc"] - c["e_tot"]) < 1e-12, name
    assert g["functionals"]["pbe0"]["exx_fraction"] == 0.25 and g["functionals"]["b3lyp5"]["exx_fraction"] == 0.20
    # closed shell: the unrestricted composition lands on the restricted one
    assert abs(g["converged"]["h2o-321g-upbe0-closed"]["e_tot"] - g["converged"]["h2o-321g-pbe0"]["e_tot"]) < 1e-9
    for name, c in g["gradients"].items():
        assert np.abs(np.array(c["gradient"]).sum(0)).max() < 1e-7, name  # translational invariance to the stencil's error
