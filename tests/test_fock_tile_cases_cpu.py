"""The budget guard of tests/fock_tile_cases.py: for every case of the bitwise GPU tests (tests/test_gpu_fock_tiles.py) the float64
reference equals the same chain computed in int64 -- every intermediate asserted below 2^62 in the integers and below 2^53 units
in the floats -- so a bitwise mismatch on the GPU is the kernel's, never the reference's."""
import numpy as np
import pytest

from tests import fock_tile_cases as ftc


def _same_all(ref, fx):
    assert set(ref) == set(fx)
    for k in ref:
        assert ftc.same(ref[k], fx[k]), k


def test_unit_and_budget_helpers():
    assert ftc.unit_exp(np.array([0.75, 2.0, -0.5])) == -2 and ftc.unit_exp(np.array([12.0, 0.0])) == 2
    assert ftc.unit_exp(np.zeros(3)) == 0
    a = ftc.dyadic(np.random.default_rng(0), (50, 40), 3, -2)
    assert np.all(a != 0) and np.all(a * 4 == np.round(a * 4)) and np.abs(a).max() <= 7 / 4
    assert ftc.same(a, ftc.Fx.of(a))
    big = np.full((4, 4), 2.0 ** 26 + 1.0)
    with pytest.raises(ftc.BudgetError):
        ftc.mm(big, big)  # 4 (2^26 + 1)^2 > 2^53 units of 1
    with pytest.raises(ftc.BudgetError):
        ftc.add(np.array([2.0 ** 53]), np.array([1.0]))
    with pytest.raises(ftc.BudgetError):
        ftc.dot(big, big)


def test_case_lists_reach_every_edge():
    ks = {s[2] for s in ftc.GEMM_CASES}
    assert ks == {1, 3, 4, 5, 127, 128, 129, 131, 260}
    assert {s[0] for s in ftc.GEMM_CASES} == {1, 15, 16, 17, 33} == {s[1] for s in ftc.GEMM_CASES}
    assert {s[3] for s in ftc.GEMM_CASES} == {0, 1} and {s[4] for s in ftc.GEMM_CASES} == {1, 3, 17}
    for col in (5, 6, 7, 8):  # every slack both absent and present
        assert {s[col] > 0 for s in ftc.GEMM_CASES} == {False, True}
    assert any(s[9] and s[4] > 1 for s in ftc.GEMM_CASES) and any(s[10] and s[4] > 1 for s in ftc.GEMM_CASES)
    assert {s[11] for s in ftc.GEMM_CASES} == {False, True} and any(s[12] != 1.0 and s[11] for s in ftc.GEMM_CASES)
    assert {s[0] for s in ftc.RESP_CASES} == {5, 17, 131} and {s[1] for s in ftc.RESP_CASES} == {1, 5, 17, 33, 65}
    assert {s[2] for s in ftc.RESP_CASES} == {1, 19, 129} and {s[3] for s in ftc.RESP_CASES} == {1, 4}
    assert [s for s in ftc.RESP_CASES if 2 * s[1] > 128] == [(131, 65, 19, 1)]
    assert ftc.FACTOR_CASES == [(7, 7, 1), (17, 14, 16), (33, 33, 17), (129, 129, 33), (131, 127, 96), (260, 257, 128)]
    assert ftc.FINISH_SHAPES == [(7, 7), (17, 14), (131, 127), (260, 257)] and 260 * 260 > 64 * 256 * 4
    forms = {(bool(k), v, f is not None) for k, v, f, _, _, _ in ftc.FINISH_FORMS.values()}
    assert forms == {(False, None, False), (True, None, False), (True, "sym", False), (False, "sym", False), (False, "raw", False),
                     (True, "sym", True), (True, "raw", True)}
    assert {c for _, _, _, _, c, _ in ftc.FINISH_FORMS.values()} == {False, True}


@pytest.mark.parametrize("spec", ftc.GEMM_CASES, ids=lambda s: "M%d-N%d-K%d-t%d-b%d" % s[:5])
def test_gemm_reference_is_the_integer_one(spec):
    inp, ref = ftc.gemm_case(spec)
    fx = ftc.gemm_chain(**ftc.to_fx(inp))
    assert ftc.same(ref, ftc.Fx(np.broadcast_to(fx.n, ref.shape), fx.e))


@pytest.mark.parametrize("shape", ftc.RESP_CASES, ids=lambda s: "nao%d-no%d-nv%d-nvec%d" % s)
def test_response_references_are_the_integer_ones(shape):
    inp, ref = ftc.resp_case(shape)
    _same_all(ref, ftc.resp_chains(ftc.to_fx(inp)))
    # the properties the GPU test asserts hold in the reference
    assert np.array_equal(ref["plus"], np.swapaxes(ref["plus"], 1, 2)) and np.array_equal(ref["minus"], -np.swapaxes(ref["minus"], 1, 2))
    assert np.all(np.diagonal(ref["minus"], axis1=1, axis2=2) == 0) and np.any(ref["minus"] != 0)


@pytest.mark.parametrize("shape", ftc.FACTOR_CASES + [ftc.FACTOR_MAX], ids=lambda s: "nao%d-north%d-r%d" % s)
def test_factor_and_density_references_are_the_integer_ones(shape):
    inp, ref = ftc.factor_case(shape)  # (raises if the float64 chain leaves the budget anywhere)
    if shape[0] <= 512:
        _same_all(ref, ftc.factor_chain(**ftc.to_fx(inp)))
    else:  # int64 GEMMs of 1024^3 take seconds: D in full, the factor on 32 AO rows, both AO densities on their 32 x 32 = 1024 elements
        rows = np.unique(np.concatenate([[0, shape[0] - 1], np.random.default_rng(5).integers(0, shape[0], 30)]))
        fx = ftc.factor_chain(**ftc.to_fx(dict(inp, x=np.ascontiguousarray(inp["x"][rows]))))
        assert ftc.same(ref["dm"], fx["dm"]) and ftc.same(ref["factor"][rows], fx["factor"]) and len(rows) ** 2 >= 500
        assert ftc.same(ref["dao"][np.ix_(rows, rows)], fx["dao"]) and ftc.same(ref["dao_dm"][np.ix_(rows, rows)], fx["dao_dm"])
    assert np.array_equal(np.sqrt(ref["w"]), inp["sw"])  # the kernel's sqrt(w) is exact
    for k in ("dm", "dao", "dao_dm"):
        assert np.array_equal(ref[k], ref[k].T)


@pytest.mark.parametrize("shape", ftc.FINISH_SHAPES, ids=lambda s: "nao%d-north%d" % s)
def test_finish_references_are_the_integer_ones(shape):
    inp, dao, ref = ftc.finish_case(shape)
    fxi = ftc.to_fx(inp)
    dao_fx = ftc.finish_density(fxi)
    assert ftc.same(dao, dao_fx)
    for form in ftc.FINISH_FORMS:
        _same_all(ref[form], ftc.finish_form_chain(fxi, dao_fx, form))
        assert np.array_equal(ref[form]["f0"], ref[form]["f0"].T)
    # deterministic mode stores the accumulators and the raw Vxc as int64 in units of 1 / scale: the chosen scales keep them integers
    for k, s in (("wj", ftc.DET_SCALE), ("wk", ftc.DET_SCALE), ("vraw", ftc.DET_VSCALE)):
        assert np.all(inp[k] * s == np.round(inp[k] * s)) and np.abs(inp[k] * s).max() < 2.0 ** 52

