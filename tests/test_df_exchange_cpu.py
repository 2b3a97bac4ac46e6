"""The public switch of density-fitted exchange (Mol.densityfit(exchange=True)) and its golden file: no GPU needed"""
import inspect
import json
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_densityfitinfo_defaults_to_coulomb_only():
    from dqc_amd.utils.datastruct import DensityFitInfo
    info = DensityFitInfo("coulomb", [])
    assert info.exchange is False
    assert DensityFitInfo(method="coulomb", auxbases=[], exchange=True).exchange is True


def test_densityfit_signature():
    from dqc_amd.system import Mol
    sig = inspect.signature(Mol.densityfit)
    assert list(sig.parameters)[1:] == ["method", "auxbasis", "exchange"]
    assert sig.parameters["exchange"].default is False


def test_golden_file_holds_the_four_cases():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_dfk.json")))
    cases = g["converged"]
    assert set(cases) == {"h2o-ccpvdz-rihf", "h2o-ccpvdz-ripbe0", "ch3-321g-riuhf", "ch3-321g-riupbe0"}
    for c in cases.values():
        for key in ("e_tot", "e_core", "e_elrep", "e_exch", "e_xc", "e_nuc"):
            assert math.isfinite(c[key])
        assert abs(c["e_core"] + c["e_elrep"] + c["e_exch"] + c["e_xc"] + c["e_nuc"] - c["e_tot"]) < 1e-12
        assert c["e_exch"] < 0 and c["commutator"] < 1e-10 and c["naux"] > 0
