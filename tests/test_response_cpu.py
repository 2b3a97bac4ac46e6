"""The solvers of dqc_amd/response.py on CPU tensors (block Davidson, preconditioned CG: plain torch, no GPU), and sanity checks of
the orbital-Hessian fixtures (tools/make_orb_hessian_golden.py -> tests/golden/oracle_orb_hessian.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from dqc_amd.response import davidson_lowest, pcg_solve, state_memo


def _seeded_matrix(n, seed, negative):
    """symmetric positive definite, diagonally dominated (as an orbital Hessian is by its orbital-energy differences), plus -- when
    asked -- one negative mode"""
    rng = np.random.default_rng(seed)
    d = np.sort(rng.uniform(0.5, 8.0, n))
    b = rng.normal(size=(n, n)) * 0.05
    a = np.diag(d) + b @ b.T + 0.05 * (b + b.T)
    if negative:
        u = rng.normal(size=n)
        u /= np.linalg.norm(u)
        a = a - (u @ a @ u + 0.7) * np.outer(u, u)
    return torch.as_tensor((a + a.T) * 0.5)


@pytest.mark.parametrize("n,neig,negative", [(60, 1, True), (60, 3, True), (60, 2, False), (5, 2, True), (2, 1, False)])
def test_davidson_lowest_matches_eigh(n, neig, negative):
    a = _seeded_matrix(n, 100 + n + neig, negative)
    calls = []

    def mm(v):
        calls.append(v.shape[0])
        return v @ a
    theta, x, res = davidson_lowest(mm, torch.diagonal(a).clone(), neig=neig, tol=1e-11)
    ev, evec = torch.linalg.eigh(a)
    assert theta.shape == (min(neig, n),) and x.shape == (min(neig, n), n)
    assert float((theta - ev[:neig]).abs().max()) < 1e-10
    if negative:
        assert float(theta[0]) < -1e-3
    for k in range(min(neig, n)):  # eigenvectors up to sign
        assert abs(abs(float(x[k] @ evec[:, k])) - 1.0) < 1e-8
    assert res < 1e-10 or sum(calls) >= n
    if n == 60:
        assert sum(calls) < n  # fewer products than the dimension: the subspace did not just grow to the whole space


@pytest.mark.parametrize("n,nrhs", [(60, 3), (7, 1)])
def test_pcg_solve_matches_dense_solve(n, nrhs):
    a = _seeded_matrix(n, 200 + n, False)
    b = torch.as_tensor(np.random.default_rng(300 + n).normal(size=(nrhs, n)))
    x, rel = pcg_solve(lambda v: v @ a, torch.diagonal(a).clone(), b, tol=1e-13)
    ref = torch.linalg.solve(a, b.T).T
    assert rel <= 1e-13
    assert float((x - ref).abs().max()) < 1e-10


def test_pcg_solve_zero_right_hand_side_and_early_rows():
    """a zero row (the dipole components a linear molecule has no response to) stays zero and does not poison the others"""
    a = _seeded_matrix(30, 7, False)
    b = torch.as_tensor(np.random.default_rng(8).normal(size=(3, 30)))
    b[1] = 0.0
    x, rel = pcg_solve(lambda v: v @ a, torch.diagonal(a).clone(), b, tol=1e-13)
    assert torch.isfinite(x).all() and float(x[1].abs().max()) == 0.0
    assert float((x - torch.linalg.solve(a, b.T).T).abs().max()) < 1e-10


def test_pcg_solve_refuses_an_indefinite_operator():
    """the response equations of a saddle point: conjugate gradients meets a direction of non-positive curvature and says so"""
    a = _seeded_matrix(30, 9, True)
    assert float(torch.linalg.eigvalsh(a)[0]) < -1e-3
    b = torch.as_tensor(np.random.default_rng(10).normal(size=(2, 30)))
    with pytest.raises(RuntimeError, match="not positive definite"):
        pcg_solve(lambda v: v @ a, torch.diagonal(a).abs(), b, tol=1e-12)


def test_memo_belongs_to_the_converged_state_not_to_the_object():
    """run() stores a new Fock tensor on the calculation: what was derived from the previous state must not be handed out again"""
    class Calc:
        _has_run = True
    qc = Calc()
    qc._fock = torch.zeros(3)
    memo = state_memo(qc)
    memo["lowest"] = -0.5
    assert state_memo(qc) is memo and state_memo(qc)["lowest"] == -0.5
    qc._fock = torch.zeros(3)  # an equal tensor, but another run's
    assert state_memo(qc) == {}
    assert state_memo(qc) is not memo


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_orb_hessian.npz"))
    return g, json.loads(str(g["meta"]))


def test_golden_cases_are_the_ones_the_generator_lists(golden):
    g, meta = golden
    assert sorted(meta) == sorted(["h2o_rhf", "h2o_lda", "h2o_pbe", "h2o_blyp", "h2o_pbe0", "ch3_uhf", "ch3_upbe", "h2_14_uhf", "h2_14_ulda",
                                   "h2_40_uhf", "h2_40_ulda"])
    for case, m in meta.items():
        n = m["n"]
        assert g[case + "_hessian"].shape == (n, n) and 2 <= n <= 94


def test_golden_hessians_are_symmetric_to_their_fd_error(golden):
    g, meta = golden
    for case in meta:
        H, err = g[case + "_hessian"], float(g[case + "_fd_error"])
        asym = np.abs(H - H.T).max()
        print("%-12s asymmetry %.2e  fd_error %.2e" % (case, asym, err))
        assert err == max(float(g[case + "_fd_stencil"]), float(g[case + "_fd_roundoff"]))  # (stencil estimate, round-off estimate)
        assert asym <= err, case
        assert np.abs(H @ g[case + "_kappa"] - g[case + "_hkappa"]).max() < 1e-12
        assert np.abs(np.linalg.eigvalsh((H + H.T) * 0.5)[:3] - g[case + "_eig3"]).max() < 1e-10


def test_golden_stability_of_every_case(golden):
    g, meta = golden
    for case, m in meta.items():
        lowest = float(g[case + "_eig3"][0])
        if m["stable"]:
            assert lowest > -1e-3, case
        else:
            assert lowest < -1e-3, case
    assert not meta["h2_40_uhf"]["stable"] and not meta["h2_40_ulda"]["stable"]
