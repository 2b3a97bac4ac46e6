"""Linear-response excited states on the GPU: exchange of antisymmetric right-hand sides in the multi-RHS tile pass
(dqc_jk_from_tiles_multi_asym), the triplet second-order functional kernel (dqc_xc_eval_fxc_triplet), the operator products A+B / A-B
of dqc_amd/response.py, `dqc_amd.excitations` (full response and TDA, singlet and triplet), the sum rule against the analytic
polarizability and the triplet (RHF -> UHF) stability.

Yardsticks: torch.einsum on the oracle's dense ERI tensor; `xc_eval_fxc_pol` fed the halved inputs; tests/golden/
oracle_excitations.npz (tools/make_excitation_golden.py: dense A+B, A-B and their spectra, each with its error estimate) and, for
the triplet stability, the unrestricted Hessians of tests/golden/oracle_orb_hessian.npz.  Tolerances: 1e-10 relative for J / K (the
parity suite's bar) and for the exact A-B; max(1e-9, 10 x fd_error) for products that carry a stencil; energies within
10 x omega_error + the solver tolerance."""
import json
import os

import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

TIGHT = {"f_tol": 1e-11, "maxiter": 300}
NAMES = ["lda_x", "lda_c_pw", "lda_c_pw_mod", "lda_c_vwn", "lda_c_pz", "gga_x_pbe", "gga_x_pbe_r", "gga_x_pbe_sol", "gga_x_rpbe",
         "gga_c_pbe", "gga_c_pbe_sol", "gga_x_b88", "gga_c_lyp", "gga_c_p86", "gga_x_pw91", "gga_x_b86", "gga_x_g96", "gga_x_pw86",
         "gga_x_optx", "gga_x_wc"]
SPECTRUM_CASES = ["h2o_rhf", "h2o_lda", "h2o_pbe", "h2o_pbe0", "ch3_uhf", "ch3_upbe", "h2_14_uhf"]
RESTRICTED = ["h2o_rhf", "h2o_lda", "h2o_pbe", "h2o_pbe0"]
SOLVER_TOL = 1e-9    # residual norm asked of the excitation solvers here (tighter than the default: see the strengths below)
DEFAULT_TOL = 1e-6   # the default `tol` of dqc_amd.excitations: the solver's share of the bounds on energies and strengths
DAVIDSON_TOL = 1e-7  # lowest_eival_orb_hessian, as in test_gpu_orb_hessian.py
H2 = ([1, 1], [[0.0, 0.0, -0.7], [0.0, 0.0, 0.7]])  # 3-21G: 4 AOs, one block -- the only tile is diagonal in every sense


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_excitations.npz"))
    return g, json.loads(str(g["meta"]))


def _cu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. antisymmetric exchange
@pytest.mark.parametrize("mol,basis,nao", [(H2, "3-21G", 4), (M.H2O, "3-21G", 13), (M.CH4, "cc-pvdz", 34)], ids=["h2", "h2o", "ch4"])
def test_antisymmetric_exchange_matches_einsum(dev, mol, basis, nao):
    import dqc_amd
    from dqc_amd import lib
    from oracle import basis as ob, natives
    h = dqc_amd.Mol(mol, basis=basis).get_hamiltonian().build()
    assert h._nao_ao == nao
    eri = _cu(natives.int2e(ob.make_tables(mol, basis)))
    g = torch.Generator().manual_seed(3)
    r = torch.randn((4, nao, nao), generator=g, dtype=torch.float64).to(dev)
    anti, sym = r - r.transpose(-2, -1), r + r.transpose(-2, -1)

    def ref(d):
        return torch.einsum("prqs,rs->pq", eri, d)

    def check(what, got, want):
        scale = float(want.abs().max())
        err = float((got - want).abs().max()) / scale
        print("%-34s nao %2d  max|K - einsum| / max|K| %.2e" % (what, nao, err))
        assert err < 1e-10, what

    def antisymmetric(k):
        assert float((k + k.T).abs().max()) <= 1e-13 * float(k.abs().max())

    # one antisymmetric right-hand side (K only, and beside a Coulomb one)
    _, K = lib.jk_multi(h._tiles, None, anti[:1], k_antisym=[1])
    check("antisymmetric, K only", K[0], ref(anti[0]))
    antisymmetric(K[0])
    J, K = lib.jk_multi(h._tiles, sym[:1], anti[:1], k_antisym=[True])
    check("antisymmetric, with J", K[0], ref(anti[0]))
    # a general matrix is antisymmetrised on the way in
    _, K = lib.jk_multi(h._tiles, None, r[:1], k_antisym=[1])
    check("general matrix, antisymmetrised", K[0], ref(0.5 * anti[0]))
    # a symmetric and an antisymmetric one in ONE pass, both orders, with and without the Coulomb density (stream and grid forms)
    for dj in (None, sym[2:3], sym[2:4]):
        for flags in ([0, 1], [1, 0]):
            dk = torch.stack([anti[1] if f else sym[0] for f in flags])
            _, K = lib.jk_multi(h._tiles, dj, dk, k_antisym=flags)
            for q, f in enumerate(flags):
                check("pair %s nj %d slot %d" % (flags, 0 if dj is None else dj.shape[0], q), K[q], ref(dk[q]))
                if f:
                    antisymmetric(K[q])
    # nk = 3: two passes
    dk, flags = torch.stack([anti[0], sym[1], anti[2]]), [1, 0, 1]
    J, K = lib.jk_multi(h._tiles, sym[3:4], dk, k_antisym=flags)
    for q in range(3):
        check("nk = 3 slot %d" % q, K[q], ref(dk[q]))
    check("nk = 3 J", J[0], torch.einsum("pqrs,rs->pq", eri, sym[3]))
    with pytest.raises(ValueError, match="one flag per exchange density"):
        lib.jk_multi(h._tiles, None, dk, k_antisym=[1])
    # deterministic mode: the symmetric slots are those of dqc_jk_from_tiles_multi bit for bit, the antisymmetric ones reproducible
    lib.set_deterministic(True)
    try:
        J0, K0 = lib.jk_multi(h._tiles, sym[3:4], torch.stack([sym[1], sym[0]]))
        J1, K1 = lib.jk_multi(h._tiles, sym[3:4], torch.stack([sym[1], sym[0]]), k_antisym=[0, 0])
        assert torch.equal(J0, J1) and torch.equal(K0, K1)
        Ja, Ka = lib.jk_multi(h._tiles, None, torch.stack([anti[0], anti[1], anti[2]]), k_antisym=[1, 1, 1])
        Jb, Kb = lib.jk_multi(h._tiles, None, torch.stack([anti[0], anti[1], anti[2]]), k_antisym=[1, 1, 1])
        assert torch.equal(Ka, Kb)
        for q in range(3):
            check("deterministic antisymmetric %d" % q, Ka[q], ref(anti[q]))
            assert torch.equal(Ka[q], -Ka[q].T)
        # a symmetric slot beside an antisymmetric one.  The accumulators are fixed-point integers (sums in any order agree bit for
        # bit) on a scale 2^k set by the largest sum|D| of the pass: 2 sym[1] sets it here, beside anti[0] as beside sym[0] (entries
        # of the same spread, half the size), so the slot must equal that of dqc_jk_from_tiles_multi exactly
        big = 2.0 * sym[1]
        assert float(big.abs().sum()) > float(anti[0].abs().sum()) and float(big.abs().sum()) > float(sym[0].abs().sum())
        _, Km = lib.jk_multi(h._tiles, None, torch.stack([big, anti[0]]), k_antisym=[0, 1])
        _, Ks = lib.jk_multi(h._tiles, None, torch.stack([big, sym[0]]))
        assert torch.equal(Km[0], Ks[0])
        check("deterministic mixed pass, antisymmetric slot", Km[1], ref(anti[0]))
    finally:
        lib.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 2. triplet functional kernel
@pytest.mark.parametrize("name", NAMES)
def test_triplet_fxc_kernel_is_the_polarised_kernel_at_halved_inputs(dev, golden_dir, name):
    from dqc_amd import lib
    fx = np.load(os.path.join(golden_dir, "oracle_fxc_pointwise.npz"))
    gga, nlow = name.startswith("gga_"), int(fx["nlow"])
    rho, grho, drho, dgrho = (_cu(fx["r_" + k]) for k in ("rho", "grho", "drho", "dgrho"))
    blk = torch.stack([drho, -2.0 * drho])
    gblk = torch.stack([dgrho, -2.0 * dgrho])
    g = (lambda t: t) if gga else (lambda t: None)
    dv, dvg = lib.xc_eval_fxc_triplet([(1.0, name)], rho, g(grho), blk, g(gblk))
    (pu, pd), (gu, gd) = lib.xc_eval_fxc_pol([(1.0, name)], 0.5 * rho, 0.5 * rho, g(0.5 * grho), g(0.5 * grho), 0.5 * blk, -0.5 * blk,
                                             g(0.5 * gblk), g(-0.5 * gblk))
    # the scale of an output is its own largest value -- unless the output vanishes: the gradient potential of a correlation
    # functional of the TOTAL sigma only (gga_c_pbe, gga_c_p86) is 2 d v_ss grad rho_u + d v_ud grad rho_d + ... with terms that
    # cancel exactly under d rho_u = -d rho_d, both kernels return their rounding (1e-18) and the scale is that of the terms, taken
    # from the closed-shell singlet response of the same functional
    sv, sg = lib.xc_eval_fxc([(1.0, name)], rho, g(grho), blk, g(gblk))
    for what, got, ref, term in (("dvrho", dv, pu, sv),) + ((("dvgrad", dvg, gu, sg),) if gga else ()):
        own, terms = float(ref.abs().max()), float(term.abs().max())
        scale = own if own > 1e-10 * terms else terms
        err = float((got - ref).abs().max()) / scale
        print("%-14s triplet %-6s max|d| / scale %.2e  (max|ref| %.2e, singlet %.2e)" % (name, what, err, own, terms))
        assert scale > 0 and err < 1e-12
        assert bool(torch.all(got[..., -nlow:] == 0.0)), "points below the density cutoff must be exactly zero"
    if not gga:
        assert dvg is None
    assert float((pu + pd).abs().max()) <= 1e-12 * float(pu.abs().max())  # (the closed-shell spin-flip response: d v_d = -d v_u)


def test_triplet_fxc_term_list_and_meta_gga(dev, golden_dir):
    from dqc_amd import lib
    fx = np.load(os.path.join(golden_dir, "oracle_fxc_pointwise.npz"))
    rho, grho, drho, dgrho = (_cu(fx["r_" + k]) for k in ("rho", "grho", "drho", "dgrho"))
    terms = [(0.75, "gga_x_pbe"), (1.0, "gga_c_pbe"), (0.1, "lda_x")]
    dv, dvg = lib.xc_eval_fxc_triplet(terms, rho, grho, drho[None], dgrho[None])
    sv, sg = 0.0, 0.0
    for c, n in terms:
        v1, g1 = lib.xc_eval_fxc_triplet([(1.0, n)], rho, grho, drho[None], dgrho[None])
        sv, sg = sv + c * v1, sg + c * (g1 if g1 is not None else 0.0)
    assert float((dv - sv).abs().max()) <= 1e-12 * float(sv.abs().max())
    assert float((dvg - sg).abs().max()) <= 1e-12 * float(sg.abs().max())
    with pytest.raises(NotImplementedError, match="mgga_x_scan"):
        lib.xc_eval_fxc_triplet([(1.0, "mgga_x_scan")], rho, grho, drho[None], dgrho[None])


# ------------------------------------------------------------------------------------------------ 3. - 7. operators and spectra
_QC = {}


def _calc(case, gold):
    """the GPU calculation of a fixture case, converged from the oracle's density (kept for the module)"""
    if case in _QC:
        return _QC[case]
    import dqc_amd
    from dqc_amd.utils.datastruct import SpinParam
    g, meta = gold
    m = meta[case]
    spin = m["spin"]
    mol = dqc_amd.Mol((m["atomzs"], m["atompos"]), basis=m["basis"], grid=m["grid"], **({"spin": spin} if spin else {}))
    kw = {} if spin is None else {"restricted": False}
    qc = dqc_amd.HF(mol, **kw) if m["xc"] is None else dqc_amd.KS(mol, xc=m["xc"], **kw)
    h = qc._engine.hamilton
    sx = h._ovlp_ao @ h._orthozer
    dms = [(sx.T @ _cu(g["%s_dm_ao_%d" % (case, s)]) @ sx).contiguous() for s in range(1 if spin is None else 2)]
    qc.run(dm0=dms[0] if spin is None else SpinParam(u=dms[0], d=dms[1]), fwd_options=TIGHT)
    assert qc.accepted
    _QC[case] = qc
    return qc


def _operator(case, gold, spin="singlet"):
    from dqc_amd.response import OrbitalHessian
    g, meta = gold
    qc = _calc(case, gold)
    orbs = [(g["%s_c_ao_%d" % (case, s)], g["%s_eps_%d" % (case, s)]) for s in range(1 if meta[case]["spin"] is None else 2)]
    return OrbitalHessian(qc, orbitals=orbs if len(orbs) == 2 else orbs[0], spin=spin)


@pytest.mark.parametrize("case", SPECTRUM_CASES + ["h2_40_rhf", "h2_40_rlda"])
def test_operator_products_match_the_dense_fixture(dev, gold, case):
    g, meta = gold
    H = _operator(case, gold)
    n = meta[case]["n"]
    assert H.n == n
    kappa = _cu(g[case + "_kappa"])
    tol_p = max(1e-9, 10.0 * float(g[case + "_fd_error"]))
    plus, minus = H.mm_pair(kappa)
    err_p = np.abs(plus.cpu().numpy() / H.pref - g[case + "_kappa"] @ g[case + "_apb"].T).max()
    err_m = np.abs(minus.cpu().numpy() / H.pref - g[case + "_kappa"] @ g[case + "_amb"].T).max()
    print("%-11s max|(A+B) k - dense| %.2e (tolerance %.2e)   max|(A-B) k - dense| %.2e (tolerance 1e-10)" % (case, err_p, tol_p, err_m))
    assert err_p < tol_p and err_m < 1e-10
    # the paired product is the two single ones; a block is its single vectors (unit vectors: the bounds are absolute)
    rng = np.random.default_rng(6)
    blk = rng.normal(size=(3, n))
    blk = _cu(blk / np.linalg.norm(blk, axis=1, keepdims=True))
    pb, mb = H.mm_pair(blk)
    assert float((H.mm(blk) - pb).abs().max()) < 1e-12 and float((H.mm_minus(blk) - mb).abs().max()) < 1e-12
    singles = torch.cat([H.mm_minus(blk[i:i + 1]) for i in range(3)])
    assert float((mb - singles).abs().max()) < 1e-12
    assert abs(float(blk[0] @ mb[1]) - float(blk[1] @ mb[0])) < 1e-10
    if meta[case]["exx_fraction"] == 0.0:
        assert torch.equal(mb, H.diag[None, :] * blk)
    if meta[case]["spin"] is None:
        T = _operator(case, gold, spin="triplet")
        tol_t = max(1e-9, 10.0 * float(g[case + "_fd_error_t"]))
        tp, tm = T.mm_pair(kappa)
        err_t = np.abs(tp.cpu().numpy() / T.pref - g[case + "_kappa"] @ g[case + "_apb_t"].T).max()
        print("%-11s max|(A+B)^T k - dense| %.2e (tolerance %.2e)" % (case, err_t, tol_t))
        assert err_t < tol_t
        tb = T.mm(blk)
        assert float((T.mm_minus(blk) - mb).abs().max()) < 1e-12  # (A-B)^T = (A-B)^S
        assert float((tb - torch.cat([T.mm(blk[i:i + 1]) for i in range(3)])).abs().max()) < 1e-12
        assert abs(float(blk[0] @ tb[1]) - float(blk[1] @ tb[0])) < 1e-10


def _grouped_f(w, f, gap=1e-4):
    """oscillator strengths summed over groups of states closer than `gap`: (first index, sum) per group"""
    out, start = [], 0
    for i in range(1, len(w) + 1):
        if i == len(w) or w[i] - w[i - 1] >= gap:
            out.append((start, i, float(np.sum(f[start:i]))))
            start = i
    return out


@pytest.mark.parametrize("tda", [False, True], ids=["full", "tda"])
@pytest.mark.parametrize("case", SPECTRUM_CASES)
def test_spectra_match_the_fixture(dev, gold, case, tda):
    import dqc_amd
    g, meta = gold
    qc = _calc(case, gold)
    key = "tda" if tda else "rpa"
    nst = 5
    ex = dqc_amd.excitations(qc, nstates=nst, tda=tda, tol=SOLVER_TOL)
    w = ex.energies.cpu().numpy()
    wref, eref = g["%s_w_%s" % (case, key)], g["%s_omega_error_%s" % (case, key)]
    tol = 10.0 * eref[:nst] + DEFAULT_TOL
    print("%-10s %-4s w %s\n%16s |dw| %s\n%16s tol  %s   f %s" % (case, key, w, "", np.abs(w - wref[:nst]), "", tol, ex.osc_strengths.cpu().numpy()))
    assert w.shape == (nst,) and ex.transition_dipoles.shape == (nst, 3) and np.all(np.diff(w) >= 0)
    assert np.all(np.abs(w - wref[:nst]) < tol)
    assert (ex.xmy is None) == tda and ex.spin == "singlet" and ex.tda == tda
    if tda:
        assert float(((ex.xpy * ex.xpy).sum(1) - 1).abs().max()) < 1e-10
    else:
        assert float(((ex.xpy * ex.xmy).sum(1) - 1).abs().max()) < 1e-10
    f, fref = ex.osc_strengths.cpu().numpy(), g["%s_f_%s" % (case, key)]
    for a, b, fsum in _grouped_f(wref, fref):
        if b > nst:  # a group cut by the number of states asked for
            break
        got = float(np.sum(f[a:b]))
        # the same relative bound as for the energies, tol / w, on the scale of the spectrum's strengths (their largest, at least 1:
        # dark states have f = 0 and no scale of their own).  An eigenvector converges only linearly in the residual where the
        # energy converges quadratically: that is why the solver runs at SOLVER_TOL = 1e-9 here, not at the default of the bound
        assert abs(got - fsum) < (tol[a] / wref[a]) * max(fref.max(), 1.0), (a, b, got, fsum)
    if meta[case]["spin"] is None:
        ext = dqc_amd.excitations(qc, nstates=nst, spin="triplet", tda=tda, tol=SOLVER_TOL)
        wt = ext.energies.cpu().numpy()
        wtref, etref = g["%s_w_%s_t" % (case, key)], g["%s_omega_error_%s_t" % (case, key)]
        print("%-10s %-4s triplet w %s |dw| %s" % (case, key, wt, np.abs(wt - wtref[:nst])))
        assert np.all(np.abs(wt - wtref[:nst]) < 10.0 * etref[:nst] + DEFAULT_TOL)
        assert not bool(ext.osc_strengths.any()) and not bool(ext.transition_dipoles.any()) and ext.spin == "triplet"


def test_whole_spectrum_of_a_tiny_case_and_clipping(dev, gold):
    import dqc_amd
    g, meta = gold
    qc = _calc("h2_14_uhf", gold)
    n = meta["h2_14_uhf"]["n"]
    for tda, key in ((False, "rpa"), (True, "tda")):
        ex = dqc_amd.excitations(qc, nstates=n, tda=tda, tol=1e-9)
        assert np.abs(ex.energies.cpu().numpy() - g["h2_14_uhf_w_" + key]).max() < 10.0 * g["h2_14_uhf_omega_error_" + key].max() + DEFAULT_TOL
        assert dqc_amd.excitations(qc, nstates=n + 10, tda=tda, tol=1e-9).energies.shape == (n,)


@pytest.mark.parametrize("case", ["h2o_rhf", "h2o_pbe0", "ch3_upbe"])
def test_sum_rule_gives_the_polarizability(dev, gold, case):
    """sum_n 2 mu_n,e mu_n,d / w_n over the FULL singlet spectrum is the static polarizability (both solved to 1e-9); the TDA
    spectrum must not satisfy it: the two modes are not the same operator"""
    import dqc_amd
    g, meta = gold
    qc = _calc(case, gold)
    n = meta[case]["n"]
    alpha = dqc_amd.polarizability(qc, tol=1e-9)
    ex = dqc_amd.excitations(qc, nstates=n, tol=1e-9)
    mu, w = ex.transition_dipoles, ex.energies
    sos = 2.0 * torch.einsum("ne,nd,n->ed", mu, mu, 1.0 / w)
    err = float((sos - alpha).abs().max())
    print("%-9s max|sum over states - alpha| %.2e\n%s" % (case, err, alpha.cpu().numpy()))
    assert err < 1e-7
    if case == "h2o_rhf":
        ext = dqc_amd.excitations(qc, nstates=n, tda=True, tol=1e-9)
        sos_t = 2.0 * torch.einsum("ne,nd,n->ed", ext.transition_dipoles, ext.transition_dipoles, 1.0 / ext.energies)
        assert float((sos_t - alpha).abs().max()) > 1e-4


@pytest.mark.parametrize("xc", [None, "lda_x + lda_c_pw"], ids=["hf", "lda"])
def test_triplet_stability_of_stretched_h2(dev, gold, golden_dir, xc):
    import dqc_amd
    g, meta = gold
    old = np.load(os.path.join(golden_dir, "oracle_orb_hessian.npz"))
    tag = "hf" if xc is None else "lda"
    qc = _calc("h2_40_r" + tag, gold)
    assert dqc_amd.is_orb_min(qc) is True
    assert dqc_amd.is_orb_min(qc, triplet=True) is False
    ev = dqc_amd.lowest_eival_orb_hessian(qc, tol=DAVIDSON_TOL, triplet=True)
    ucase = "h2_40_u" + tag
    ref = 2.0 * float(old[ucase + "_eig3"][0])  # H^T / 2 = H_uu - H_ud on the symmetric solution
    tol = 10.0 * float(old[ucase + "_fd_error"]) + DAVIDSON_TOL
    print("%s: triplet lowest %.10f, 2 x unrestricted lowest %.10f, |d| %.2e (tolerance %.2e)" % (tag, float(ev[0]), ref, abs(float(ev[0]) - ref), tol))
    assert ev.shape == (1,) and abs(float(ev[0]) - ref) < tol
    assert abs(float(ev[0]) - 4.0 * float(g["h2_40_r%s_apb_t_lowest" % tag])) < max(1e-9, 40.0 * float(g["h2_40_r%s_fd_error_t" % tag])) + DAVIDSON_TOL
    with pytest.raises(RuntimeError, match="is_orb_min"):
        dqc_amd.excitations(qc, nstates=2, spin="triplet")
    # (the Tamm-Dancoff triplet need not fail: A = ((A+B) + (A-B)) / 2 can stay positive where A+B is not -- it does for LDA here)
    assert float(dqc_amd.excitations(qc, nstates=2).energies[0]) > 0.0  # the singlet channel of the same state is fine
    near = _calc("h2_14_r" + tag, gold)
    assert dqc_amd.is_orb_min(near) is True and dqc_amd.is_orb_min(near, triplet=True) is True


def test_refusals_and_memo(dev, gold, monkeypatch):
    import dqc_amd
    g, meta = gold
    qcu = _calc("h2_14_uhf", gold)
    with pytest.raises(ValueError, match="triplet"):
        dqc_amd.excitations(qcu, spin="triplet")
    with pytest.raises(ValueError, match="triplet"):
        dqc_amd.is_orb_min(qcu, triplet=True)
    with pytest.raises(ValueError, match="triplet"):
        dqc_amd.lowest_eival_orb_hessian(qcu, triplet=True)
    with pytest.raises(ValueError, match="spin"):
        dqc_amd.excitations(qcu, spin="quintet")
    qc = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid="sg2"), xc="mgga_x_scan").run()
    with pytest.raises(NotImplementedError, match="mgga_x_scan"):
        dqc_amd.excitations(qc)
    qc = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid="sg2").densityfit(auxbasis="etb"), xc="lda_x").run()
    with pytest.raises(NotImplementedError, match="density fitting"):
        dqc_amd.excitations(qc)
    monkeypatch.setenv("DQC_AMD_ERI", "direct")
    qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G")).run()
    monkeypatch.delenv("DQC_AMD_ERI")
    assert qc._engine.hamilton._direct
    with pytest.raises(NotImplementedError, match="direct SCF"):
        dqc_amd.excitations(qc)
    # memoised on the converged state, dropped by another run()
    m = meta["h2_14_rhf"]
    qc = dqc_amd.HF(dqc_amd.Mol((m["atomzs"], m["atompos"]), basis=m["basis"])).run()
    ex = dqc_amd.excitations(qc, nstates=2)
    assert dqc_amd.excitations(qc, nstates=2) is ex
    assert dqc_amd.excitations(qc, nstates=2, tda=True) is not ex
    qc.run()
    ex2 = dqc_amd.excitations(qc, nstates=2)
    assert ex2 is not ex and float((ex2.energies - ex.energies).abs().max()) < 1e-6
