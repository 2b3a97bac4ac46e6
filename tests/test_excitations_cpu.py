"""Linear-response excited states, the parts that need no GPU: the block solver `response_eigs` of dqc_amd/response.py on dense
symmetric positive definite pairs (A+B, A-B) against numpy.linalg.eig, its error path, the normalisation, and the consistency of the
fixture tests/golden/oracle_excitations.npz (tools/make_excitation_golden.py) with itself."""
import json
import os

import numpy as np
import pytest
import torch


def _pair(n, seed, coupling=0.3):
    """A+B and A-B with the structure of the real ones: a common positive diagonal (orbital-energy differences) plus symmetric
    couplings small enough to keep both positive definite"""
    rng = np.random.default_rng(seed)
    delta = np.sort(rng.uniform(0.3, 3.0, size=n))
    out = []
    for _ in range(2):
        m = rng.normal(size=(n, n)) * coupling / np.sqrt(n)
        m = np.diag(delta) + (m + m.T) * 0.5
        assert np.linalg.eigvalsh(m)[0] > 0.05
        out.append(torch.as_tensor(m))
    return out[0], out[1], torch.as_tensor(delta)


@pytest.mark.parametrize("n,neig,seed", [(6, 6, 0), (40, 5, 1), (150, 4, 2), (150, 9, 3)])
def test_response_eigs_matches_dense_eig(n, neig, seed):
    from dqc_amd.response import response_eigs
    apb, amb, delta = _pair(n, seed)
    calls = []

    def mm_pair(v):
        calls.append(v.shape[0])
        return v @ apb, v @ amb
    w, xpy, xmy, res = response_eigs(mm_pair, delta, neig=neig, tol=1e-9)
    ref = np.sqrt(np.sort(np.linalg.eig((amb @ apb).numpy())[0].real))[:neig]
    print("n %d neig %d: residual %.1e, products %d, max|w - eig| %.1e" % (n, neig, res, sum(calls), np.abs(w.numpy() - ref).max()))
    assert res < 1e-9 or n == neig
    assert np.abs(w.numpy() - ref).max() < 1e-9
    assert np.all(np.diff(w.numpy()) >= 0)
    # normalisation and the two response equations
    assert float(((xpy * xmy).sum(1) - 1.0).abs().max()) < 1e-10
    assert float((xpy @ apb - w[:, None] * xmy).abs().max()) < 1e-8
    assert float((xmy @ amb - w[:, None] * xpy).abs().max()) < 1e-8
    if n > 100:
        assert max(calls) <= 2 * neig + 3  # a block of at most two corrections per state at a time, never the dense matrix


def test_response_eigs_whole_space_is_exact_and_clips_neig():
    from dqc_amd.response import response_eigs
    apb, amb, delta = _pair(3, 5)
    w, xpy, xmy, res = response_eigs(lambda v: (v @ apb, v @ amb), delta, neig=7, tol=1e-12)
    assert w.shape == (3,) and xpy.shape == (3, 3)
    ref = np.sqrt(np.sort(np.linalg.eig((amb @ apb).numpy())[0].real))
    assert np.abs(w.numpy() - ref).max() < 1e-12


@pytest.mark.parametrize("which", ["minus", "plus"])
def test_response_eigs_raises_on_an_indefinite_operator(which):
    from dqc_amd.response import response_eigs
    apb, amb, delta = _pair(12, 7)
    bad = (amb if which == "minus" else apb).clone()
    bad[0, 0] = -0.5  # the lowest diagonal element: in the first trial space
    ops = (apb, bad) if which == "minus" else (bad, amb)
    with pytest.raises(RuntimeError, match="is_orb_min"):
        response_eigs(lambda v: (v @ ops[0], v @ ops[1]), delta, neig=2, tol=1e-8)


def test_fixture_is_consistent(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_excitations.npz"))
    meta = json.loads(str(g["meta"]))
    assert sorted(meta) == sorted(["h2o_rhf", "h2o_lda", "h2o_pbe", "h2o_pbe0", "ch3_uhf", "ch3_upbe", "h2_14_uhf", "h2_14_rhf", "h2_14_rlda",
                                   "h2_40_rhf", "h2_40_rlda"])
    for case, m in meta.items():
        apb, amb, n = g[case + "_apb"], g[case + "_amb"], m["n"]
        assert apb.shape == (n, n) and amb.shape == (n, n)
        nocc = m["nocc"]
        delta = np.concatenate([(g["%s_eps_%d" % (case, s)][no:, None] - g["%s_eps_%d" % (case, s)][None, :no]).reshape(-1)
                                for s, no in enumerate(nocc)])
        if m["exx_fraction"] == 0.0:  # a pure functional: A - B is the diagonal of orbital-energy differences, exactly
            assert np.array_equal(amb, np.diag(delta))
        else:
            assert np.abs(amb - amb.T).max() < 1e-11 and np.abs(amb - np.diag(np.diag(amb))).max() > 1e-3
        # the recorded spectra are those of the recorded matrices
        w2 = np.sort(np.linalg.eig(amb @ ((apb + apb.T) * 0.5))[0].real)
        assert np.abs(np.sqrt(w2) - g[case + "_w_rpa"]).max() < 1e-9
        assert np.abs(np.linalg.eigvalsh(((apb + apb.T) * 0.5 + amb) * 0.5) - g[case + "_w_tda"]).max() < 1e-10
        assert np.all(g[case + "_w_tda"] >= g[case + "_w_rpa"] - 1e-10)  # TDA energies bound the full-response ones from above
        assert np.abs((g[case + "_xpy"] * g[case + "_xmy"]).sum(1) - 1.0).max() < 1e-10
        f = 2.0 / 3.0 * g[case + "_w_rpa"] * (g[case + "_mu_rpa"] ** 2).sum(1)
        assert np.abs(f - g[case + "_f_rpa"]).max() < 1e-13
        # Thomas-Reiche-Kuhn: the oscillator strengths of the full spectrum sum to a basis-set-limited fraction of the electron
        # number; for the pure functionals (no non-local exchange in the response) the sum is that of the bare orbital transitions
        assert 0.0 < f.sum() < sum(nocc) * (2 if m["spin"] is None else 1)
        if m["spin"] is None:
            low = float(g[case + "_apb_t_lowest"])
            assert (low > 0) == m["triplet_stable"]
            assert ((case + "_w_rpa_t") in g.files) == m["triplet_stable"]
