"""GPU tests (-m gpu) of the integral kernels on contractions deeper than the 8 primitives of the bundled basis sets.  The kernels
choose their launch map and their primitive loop by contraction depth (csrc/eri_core.hpp: screen_bin, eri_split_lanes, the
wave table / run list of the tile fill, one prefix per depth bin in the screened planner, the float-reciprocal index split), and
no other test builds a shell of more than three primitives: depth bin 0 (> 64 primitive pairs), the lane splits only it produces,
primitive-quartet indices above 4096 and the 45-primitive gate are reached here alone.

The deep dimer (tests/test_deep_contractions_cpu.py: SHELLS; its coverage test shows every depth bin occupied, bin 0 by
same-centre and cross-centre pairs): two centres, each with two 12-primitive s contractions over ONE exponent set (the merged
general-contraction tables, 144 primitive pairs), a 9-primitive p, a 3-primitive d, an f, a diffuse s and a two-primitive s, at
R = 1.4, 4.0 and 9.0 along a skew axis -- 38 functions.  Every entry point against the oracle, called at test time, with the
suite's standing bounds: tiles 1e-11 max(1, max|ref|) absolute; J, K, one-electron, 2- and 3-centre integrals and AO values 1e-12
of the largest reference element; gradients 1e-10 max|ref| + 1e-13; Fock 1e-9, energy 1e-8.  The oracle itself is held to a
40-digit closed form on 12-primitive (ss|ss) quartets (2e-14 relative) in the CPU file.

The limit: a 45-primitive s and p on one centre, 2025 primitive pairs per shell pair, primitive-quartet indices up to 45^4 - 1 =
4 100 624 < 2^22 -- against tests/golden/deep_limit_eri.npz (tools/make_deep_limit_golden.py: the oracle takes 8 s for the
(pp|pp) quartet alone), the cheap quartets recomputed by the oracle at test time."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import test_deep_contractions_cpu as DC

pytestmark = pytest.mark.gpu

_WORST = {}
_TAU = 1e-13


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    for k in sorted(_WORST):
        print("WORST %-44s %.3e" % (k, _WORST[k]))


def _worst(key, v):
    _WORST[key] = max(_WORST.get(key, 0.0), float(v))


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def _geo(R):
    """(oracle tables, library tables, the oracle's dense tensor) of the deep dimer at distance R: computed once, never written to"""
    from oracle import natives as nat
    from dqc_amd import lib
    t = DC.deep_tables(R)
    ref = nat.int2e(t)
    ref.setflags(write=False)
    return t, lib.Tables(t.atm, t.bas, t.env), ref


def _density(R, nao):
    D = np.random.default_rng(int(10 * R)).standard_normal((nao, nao))  # not symmetric
    return D, 0.5 * (D + D.T)


def _jk_ref(Ds, ref):
    return np.einsum("ij,ijkl->kl", Ds, ref), np.einsum("il,ijkl->jk", Ds, ref)


def _with_generic(fun):
    from dqc_amd import lib
    prev = lib.set_generic_eri(True)
    try:
        return fun()
    finally:
        lib.set_generic_eri(prev)


# ------------------------------------------------------------------------------------------------
# the deep dimer, per geometry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", DC.GEOS)
def test_deep_dimer_tiles_vs_oracle(dev, R):
    """dqc_eri_fill_tiles through the compile-time classes and with every class through the runtime kernel"""
    from dqc_amd import lib
    t, tab, ref = _geo(R)
    assert tab.nao == DC.NAO and 10.0 < np.abs(ref).max() < 11.0
    bound = 1e-11 * max(1.0, np.abs(ref).max())
    dense = lib.eri_dense(lib.eri_tiles(tab, dev), tab.nao).cpu().numpy()
    dense_rt = _with_generic(lambda: lib.eri_dense(lib.eri_tiles(tab, dev), tab.nao).cpu().numpy())
    for what, got in (("tiles", dense), ("tiles runtime kernel", dense_rt)):
        err = np.abs(got - ref)
        _worst("%s R %.1f" % (what, R), err.max())
        # the quartets of the 12-primitive contractions alone (shells 0, 1 of each centre: 20 736 primitive quartets each)
        deep = np.array([0, 1, t.ao_loc[DC.NSH], t.ao_loc[DC.NSH] + 1])
        _worst("%s R %.1f, 12-primitive (ss|ss)" % (what, R), err[np.ix_(deep, deep, deep, deep)].max())
        print("%s R = %.1f: max error %.3e at %s" % (what, R, err.max(), np.unravel_index(err.argmax(), err.shape)))
        assert err.max() <= bound, (what, R, err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("R", DC.GEOS)
def test_deep_dimer_direct_jk_vs_oracle(dev, R):
    """dqc_jk_direct: J and K of a random non-symmetric density"""
    from dqc_amd import lib
    t, tab, ref = _geo(R)
    D, Ds = _density(R, tab.nao)
    Jr, Kr = _jk_ref(Ds, ref)
    J, K = lib.jk_direct(tab, torch.as_tensor(D, device=dev), True)
    ej, ek = rel(J.cpu().numpy(), Jr), rel(K.cpu().numpy(), Kr)
    J1, none = lib.jk_direct(tab, torch.as_tensor(D, device=dev), False)
    e1 = rel(J1.cpu().numpy(), Jr)
    _worst("direct J R %.1f" % R, max(ej, e1))
    _worst("direct K R %.1f" % R, ek)
    print("direct J / K / J alone R = %.1f: %.3e %.3e %.3e" % (R, ej, ek, e1))
    assert none is None and ej < 1e-12 and ek < 1e-12 and e1 < 1e-12, (R, ej, ek, e1)


@pytest.mark.parametrize("R", DC.GEOS)
def test_deep_dimer_screened_direct_context(dev, R, monkeypatch):
    """dqc_direct_*: the Schwarz bounds against the dense tensor, tau = 0 equal to the unscreened pass, tau = 1e-13 within
    tau npair with and without K -- under every primitive split of the multi-lane classes (DQC_ERI_SPLIT_PER off / finest /
    default) and both entry forms of the one-lane classes (DQC_ERI_FLIP1), whose lane counts follow from the depth bin"""
    from dqc_amd import lib
    from tests.test_gpu_parity import _schwarz_check
    t, tab, ref = _geo(R)
    D, Ds = _density(R, tab.nao)
    Jr, Kr = _jk_ref(Ds, ref)
    Dt = torch.as_tensor(D, device=dev)
    ctx = lib.DirectContext(tab, dev)
    try:
        q, sh = ctx.bounds()
        _schwarz_check(q, sh, ref, t.ao_loc)
        Ju, Ku = lib.jk_direct(tab, Dt, True)
        J0, K0 = ctx.jk(Dt, True, 0.0)
        tot, lau, _ = ctx.stats()
        npair = tab.nbas * (tab.nbas + 1) // 2
        assert tot == lau == npair * (npair + 1) // 2
        e0 = max(rel(J0.cpu().numpy(), Ju.cpu().numpy()), rel(K0.cpu().numpy(), Ku.cpu().numpy()))
        _worst("context tau 0 vs unscreened R %.1f" % R, e0)
        assert e0 < 1e-13, (R, e0)
        ej, ek = rel(J0.cpu().numpy(), Jr), rel(K0.cpu().numpy(), Kr)
        _worst("context J R %.1f" % R, ej)
        _worst("context K R %.1f" % R, ek)
        assert ej < 1e-12 and ek < 1e-12, (R, ej, ek)
        for per in (None, "0", "1", "16"):
            for flip in (None, "0", "1"):
                if (per is None) != (flip is None):
                    continue
                if per is not None:
                    monkeypatch.setenv("DQC_ERI_SPLIT_PER", per)
                    monkeypatch.setenv("DQC_ERI_FLIP1", flip)
                J1, K1 = ctx.jk(Dt, True, _TAU)
                tot, lau, _ = ctx.stats()
                assert 0 < lau <= tot
                J2, none = ctx.jk(Dt, False, _TAU)
                dj = max(float((J1 - Ju).abs().max()), float((J2 - Ju).abs().max()))
                dk = float((K1 - Ku).abs().max())
                _worst("context tau 1e-13 |dJ| R %.1f" % R, dj)
                _worst("context tau 1e-13 |dK| R %.1f" % R, dk)
                print("R = %.1f split %s flip %s: launched %d of %d, |dJ| %.3e |dK| %.3e (bar %.3e)" % (R, per, flip, lau, tot, dj, dk, _TAU * npair))
                assert none is None and dj < _TAU * npair and dk < _TAU * npair, (R, per, flip, dj, dk)
                # ... and still the oracle's J and K
                assert rel(J1.cpu().numpy(), Jr) < 1e-12 and rel(K1.cpu().numpy(), Kr) < 1e-12 and rel(J2.cpu().numpy(), Jr) < 1e-12
    finally:
        ctx.close()


@pytest.mark.parametrize("R", DC.GEOS)
def test_deep_dimer_one_electron_and_ao_values_vs_oracle(dev, R):
    """dqc_int1e (overlap, kinetic, nuclear attraction) and dqc_eval_gto with gradients on 67 points, both nuclei among them"""
    from oracle import natives as nat
    from dqc_amd import lib
    t, tab, _ = _geo(R)
    for w in ("ovlp", "kin", "nuc"):
        e = rel(lib.int1e(w, tab, dev).cpu().numpy(), nat.int1e(w, t))
        _worst("int1e %s" % w, e)
        assert e < 1e-12, (w, R, e)
    rng = np.random.default_rng(3)
    pos = DC.deep_mol(R)[1]
    rg = np.concatenate([pos, pos[rng.integers(0, 2, 65)] + rng.standard_normal((65, 3)) * 10.0 ** rng.uniform(-3, 0.5, (65, 1))])
    assert rg.shape == (67, 3)
    ao = lib.eval_gto(tab, torch.as_tensor(rg, device=dev), 1).cpu().numpy()
    e0 = rel(ao[0][:, :tab.nao], nat.eval_gto(t, rg, 0).T)
    e1 = rel(ao[1:, :, :tab.nao], nat.eval_gto(t, rg, 1).transpose(0, 2, 1))
    _worst("eval_gto values", e0)
    _worst("eval_gto gradients", e1)
    assert e0 < 1e-12 and e1 < 1e-12, (R, e0, e1)
    assert np.abs(ao[:, :, tab.nao:]).max(initial=0.0) == 0.0


@pytest.mark.parametrize("R", DC.GEOS)
def test_deep_dimer_2c_and_3c_integrals_vs_oracle(dev, R):
    """dqc_int2c2e / dqc_int3c2e with the deep shells as the auxiliary set as well"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    tc, orb, aux = ob.make_tables_df(DC.deep_mol(R), [DC.SHELLS, DC.SHELLS], [DC.SHELLS, DC.SHELLS])
    tabc = lib.Tables(tc.atm, tc.bas, tc.env)
    e2 = rel(lib.int2c2e(tabc, aux, dev).cpu().numpy(), nat.int2c2e(tc, aux))
    e3 = rel(lib.int3c2e(tabc, orb, aux, dev).cpu().numpy(), nat.int3c2e(tc, orb, aux))
    _worst("2-centre", e2)
    _worst("3-centre", e3)
    assert e2 < 1e-12 and e3 < 1e-12, (R, e2, e3)


# ------------------------------------------------------------------------------------------------
# derivative kernels (R = 1.4, 4.0)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", DC.GEOS[:2])
def test_deep_dimer_gradients_vs_oracle(dev, R):
    """dqc_eri_grad (compile-time classes and the runtime kernel), dqc_int1e_grad and dqc_df_grad with random symmetric Cartesian
    densities against the oracle's analytic derivative integrals, called and bounded as in tests/test_gpu_gradient_terms.py.
    dqc_eri_grad runs on SHELLS_GRAD -- without the f shell and the second s contraction: the oracle's derivative contraction
    takes 7.6 s for the whole basis and 1.7 s without them, and the gradient kernels do not use the merged tables; the 12-, 9-,
    3- and 2-primitive shells, i.e. every depth bin, stay.  The one-electron and fitted gradients keep the whole basis."""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    from tests.test_gpu_gradient_terms import _check, _k_df, _k_eri, _k_int1e, _sym, _WORST as worst_g
    rng = np.random.default_rng(int(100 * R))
    tg = DC.deep_tables(R, DC.SHELLS_GRAD)
    tabg = lib.Tables(tg.atm, tg.bas, tg.env)
    ncg = nat.ao_count(tg, cart=True)
    D = _sym(rng, ncg)
    ref = nat.eri_grad(tg, D, 1.0, 0.5, cart=True)
    _check("deep eri_grad", _k_eri(dev, tabg, D, 1.0, 0.5), ref)
    _check("deep eri_grad runtime kernel", _with_generic(lambda: _k_eri(dev, tabg, D, 1.0, 0.5)), ref)
    t, tab, _ = _geo(R)
    nc = nat.ao_count(t, cart=True)
    assert nc == 46
    D, W = _sym(rng, nc), _sym(rng, nc)
    _check("deep int1e_grad", _k_int1e(dev, tab, D, W), nat.int1e_grad(t, D, W, cart=True))
    tc, orb, aux = ob.make_tables_df(DC.deep_mol(R), [DC.SHELLS, DC.SHELLS], [DC.SHELLS, DC.SHELLS])
    tabc = lib.Tables(tc.atm, tc.bas, tc.env)
    c = rng.standard_normal(nc)
    dc = np.zeros((2 * nc, 2 * nc))
    dc[:nc, :nc] = D
    cc = np.zeros(2 * nc)
    cc[nc:] = c
    _check("deep df_grad", _k_df(dev, tabc, dc, cc, orb, aux), nat.df_grad(tc, orb, aux, D, c, cart=True))
    for k, v in worst_g.items():
        if k.startswith("deep "):
            _worst(k[5:], v)


_ROWS = 6  # primitives of the deep shell whose perturbed copies share one extended table


def _extended(t, ish, rows, steps):
    """the tables of t with, after the shells of atom 0, one single-primitive s shell (coefficient 1) per row k in `rows` and
    per value alpha_k, alpha_k (1 + s) for s in steps: the contraction with primitive k moved to another exponent or coefficient is
    a linear combination of the shell and these, so that ONE set of oracle integrals serves every step of every row"""
    from oracle import basis as ob

    def shells(ia):
        return [(int(b[1]), t.env[b[5]:b[5] + b[2]].copy(), t.env[b[6]:b[6] + b[2]].copy()) for b in t.bas if int(b[0]) == ia]

    values = []
    for k in rows:
        a = float(t.env[t.bas[ish, 5] + k])
        values += [a] + [a * (1 + s) for s in steps]
    extra = [(0, [v], [1.0]) for v in values]
    return ob.Tables(t.atomzs, t.atompos, [shells(0) + extra, shells(1)]), values


@pytest.mark.parametrize("R", DC.GEOS[:2])
def test_deep_dimer_basis_gradients_vs_differences_of_the_oracle(dev, R):
    """dqc_int1e_grad_basis / dqc_eri_grad_basis: d/dalpha and d/dc of all 12 primitives of the deep s shell of atom 0 against
    Richardson-extrapolated central differences of the oracle's integrals contracted with the same densities -- the step and the
    bar of tests/test_gpu_basis_gradient.py (h = 1e-3; 4 |fd_h - fd_h/2| + 1e-10 max|ref|).  On SHELLS_GRAD, as the gradient
    test above and for the same reason.  The 96 perturbed tables are not integrated one by one: the contraction with one
    primitive moved is the shell plus c_k (g[alpha'] - g[alpha_k]) resp. (c' - c_k) g[alpha_k], so the oracle integrates the basis
    extended by those primitives once per six rows and the perturbed energies follow by linearity (perturbing env directly
    gives the same differences, to the round-off of a difference of whole energies: 4.743113e-4 there against 4.7431159167e-4
    here and 4.74311592e-4 from the kernel for dE1/dalpha of the most diffuse primitive at R = 1.4)"""
    from oracle import natives as nat
    from dqc_amd import lib
    from tests.test_gpu_basis_gradient import _H, _check, _dev, _richardson, _sym, _WORST as worst_b
    t = DC.deep_tables(R, DC.SHELLS_GRAD)
    tab = lib.Tables(t.atm, t.bas, t.env)
    ish, nprim = 0, int(t.bas[0, 2])
    assert nprim == 12 and int(t.bas[0, 0]) == 0 and int(t.bas[0, 1]) == 0
    rng = np.random.default_rng(int(1000 * R))
    n = t.nao
    D, W = _sym(rng, n), _sym(rng, n)
    T = lib.cart2sph_matrix(tab, "cpu").numpy()
    dc, wc = _dev(T.T @ D @ T, dev), _dev(T.T @ W @ T, dev)
    ntot = int(t.bas[:, 2].sum())
    zero = lambda: torch.zeros((ntot, 2), dtype=torch.float64, device=dev)  # noqa: E731
    g1 = lib.int1e_grad_basis(zero(), dc, wc, tab).cpu().numpy()
    gj = lib.eri_grad_basis(zero(), dc, 0.0, tab, jscale=1.0).cpu().numpy()
    gk = lib.eri_grad_basis(zero(), dc, 1.0, tab, jscale=0.0).cpu().numpy()
    steps = [_H, -_H, _H / 2, -_H / 2]
    n0 = int(t.ao_loc[DC.NSH - 2])  # functions of atom 0 (SHELLS_GRAD has two shells fewer per centre)
    assert n0 == n // 2
    refs, bars, got = [], [], []
    for r0 in range(0, nprim, _ROWS):
        rows = list(range(r0, r0 + _ROWS))
        te, values = _extended(t, ish, rows, steps)
        ne = len(values)
        idx = np.array([i if i < n0 else i + ne for i in range(n)])
        h = nat.int1e("kin", te) + nat.int1e("nuc", te)
        s = nat.int1e("ovlp", te)
        eri = nat.int2e(te)

        U0 = np.zeros((n, te.nao))
        U0[np.arange(n), idx] = 1.0
        D0, d0, w0 = U0.T @ D @ U0, U0.T @ D[:, 0], U0.T @ W[:, 0]
        J0, K0 = np.einsum("abcd,cd->ab", eri, D0), np.einsum("abcd,ac->bd", eri, D0)

        def energies(col):
            """[E1, Ej, Ek] (tests/test_gpu_basis_gradient.py: _oracle_energies) with the deep shell plus `col` of the extras,
            MINUS their unperturbed values: function 0 becomes chi_0 + sum_e v_e g_e, so the densities of the extended basis
            change by dD = d0 v^T + v d0^T + D_00 v v^T, and the energies are expanded in dD -- a difference of two whole
            energies would carry 1e-16 |E| / (h theta) = 2e-11 of round-off for the most diffuse primitive (theta = 0.034),
            twice the 1e-10 max|ref| floor of the bar"""
            v = np.zeros(te.nao)
            v[n0:n0 + ne] = col
            dD = np.outer(d0, v) + np.outer(v, d0) + D[0, 0] * np.outer(v, v)
            dW = np.outer(w0, v) + np.outer(v, w0) + W[0, 0] * np.outer(v, v)
            return [np.sum(dD * h) - np.sum(dW * s), np.sum(J0 * dD) + 0.5 * np.einsum("abcd,ab,cd->", eri, dD, dD, optimize=True),
                    -0.5 * np.sum(K0 * dD) - 0.25 * np.einsum("abcd,ac,bd->", eri, dD, dD, optimize=True)]

        for j, k in enumerate(rows):
            ak, ck = float(t.env[t.bas[ish, 5] + k]), float(t.env[t.bas[ish, 6] + k])
            base = j * (len(steps) + 1)

            def e_alpha(v):
                col = np.zeros(ne)
                col[base] = -ck
                col[base + values[base:base + len(steps) + 1].index(v)] += ck  # (the exact value _richardson asks for)
                return energies(col)

            def e_coef(v):
                col = np.zeros(ne)
                col[base] = v - ck
                return energies(col)

            for col, fun, theta in ((0, e_alpha, ak), (1, e_coef, ck)):
                r, b = _richardson(fun, theta)
                refs.append(r)
                bars.append(b)
                got.append([g1[k, col], gj[k, col], gk[k, col]])
    refs, bars, got = np.array(refs), np.array(bars), np.array(got)
    assert refs.shape == (2 * nprim, 3)
    for i, name in enumerate(("int1e", "eri j", "eri k")):
        for cols, par in ((slice(0, None, 2), "alpha"), (slice(1, None, 2), "c")):
            _check("deep %s d/d%s" % (name, par), got[cols, i], refs[cols, i], bars[cols, i])
    for k, v in worst_b.items():
        if k.startswith("deep "):
            _worst("basis gradient " + k[5:], v)


# ------------------------------------------------------------------------------------------------
# one SCF-level case
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["stored", "direct"])
def test_deep_dimer_fock_and_energy_vs_oracle(dev, mode, monkeypatch):
    """HF on Mol(..., basis = the same shells as CGTOBasis lists) at R = 1.4 (13 electrons: spin 1, one set of orbitals): the Fock
    matrix and the energy of a seeded density against the oracle engine, formed as in
    tests/test_gpu_parity.py::test_random_molecules_fock_and_energy_vs_oracle; with the tile store and with DQC_AMD_ERI=direct"""
    import dqc_amd
    from dqc_amd.utils.datastruct import CGTOBasis
    from oracle import hamilton as oh
    from tests import molecules as M
    if mode == "direct":
        monkeypatch.setenv("DQC_AMD_ERI", "direct")
    R = 1.4
    t, _, _ = _geo(R)
    eng_o = oh.Engine(t, eri_mode="dense", spin=1)
    td = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    bases = [[CGTOBasis(l, td(a), td(c)) for l, a, c in DC.SHELLS] for _ in range(2)]
    zs, pos = DC.deep_mol(R)
    m = dqc_amd.Mol((zs, pos.tolist()), basis=bases, spin=1)
    eng_g = dqc_amd.HF(m, restricted=True)._engine
    h = eng_g.hamilton
    assert h.eri_mode_used == ("direct" if mode == "direct" else "tiles")
    assert np.allclose(h._tab.env, t.env, rtol=1e-14, atol=0.0) and np.array_equal(h._tab.bas, t.bas)
    S = h._ovlp_ao.cpu()
    Dao = torch.as_tensor(M.seeded_dm_ao(t.nao, sum(zs), S.numpy(), seed=7))
    Xg, Xo = h._orthozer.cpu(), eng_o.h.X
    assert Xg.shape == Xo.shape == (t.nao, t.nao)  # (the smallest overlap eigenvalue is 3e-4: nothing is dropped)
    dg = ((Xg.T @ S) @ Dao @ (S @ Xg)).to(dev)
    do = (Xo.T @ S) @ Dao @ (S @ Xo)
    Fg = ((S @ Xg) @ eng_g.dm2scp(dg).cpu() @ (S @ Xg).T).numpy()
    Fo = ((S @ Xo) @ eng_o.dm2scp(do) @ (S @ Xo).T).numpy()
    eg, eo = float(eng_g.dm2energy(dg)), float(eng_o.dm2energy(do))
    _worst("Fock %s" % mode, rel(Fg, Fo))
    _worst("energy %s" % mode, abs(eg - eo) / max(1.0, abs(eo)))
    assert rel(Fg, Fo) < 1e-9, (mode, rel(Fg, Fo))
    assert abs(eg - eo) < 1e-8 * max(1.0, abs(eo)), (mode, eg, eo)


# ------------------------------------------------------------------------------------------------
# the limit: 45 primitives
# ------------------------------------------------------------------------------------------------
# shells: 0 = s, 1 = p of the deep centre (45 primitives each), 2 = s, 3 = p of the other centre (one primitive)
_LIMIT_CLASSES = {"(ss|ss)": ((0, 0, 0, 0), (0, 2, 0, 0)), "(ps|ss)": ((1, 0, 0, 0), (1, 2, 0, 0)),
                  "(pp|ss)": ((1, 1, 0, 0), (1, 1, 2, 0)), "(pp|pp)": ((1, 1, 1, 1), (1, 3, 1, 1))}
_ORACLE_AT_TEST_TIME = [(0, 0, 0, 0), (0, 2, 0, 0), (1, 2, 0, 0), (1, 1, 2, 0), (1, 3, 1, 1)]  # 0.1 - 0.4 s each


def _limit_tables():
    from oracle import basis as ob
    return ob.make_tables(([5, 1], np.stack([DC.ORIGIN, DC.ORIGIN + 2.0 * DC.SKEW])), DC.limit_shells())


def test_46_primitives_are_refused_on_the_device_path(dev):
    from oracle import basis as ob
    from dqc_amd import lib
    ex = (2.0e4 * 1.3 ** -np.arange(46.0)).tolist()
    t = ob.make_tables(([5], [[0.0, 0.0, 0.0]]), [[(0, ex, [1.0] * 46)]])
    tab = lib.Tables(t.atm, t.bas, t.env)
    with pytest.raises(lib.DqcAmdError, match=r"1 \.\.\. 45 primitives"):
        lib.eri_tiles(tab, dev)
    with pytest.raises(lib.DqcAmdError, match=r"1 \.\.\. 45 primitives"):
        lib.jk_direct(tab, torch.zeros((1, 1), dtype=torch.float64, device=dev), True)


@functools.lru_cache(maxsize=None)
def _limit(golden_dir):
    """(tables, the oracle's dense tensor from the fixture) of the limit basis; the fixture is tied to the tables of this file and,
    through the quartets the oracle can afford at test time, to the oracle"""
    from oracle import natives as nat
    t = _limit_tables()
    gold = np.load(os.path.join(golden_dir, "deep_limit_eri.npz"))
    assert np.array_equal(gold["atm"], t.atm) and np.array_equal(gold["bas"], t.bas)
    assert np.allclose(gold["env"], t.env, rtol=1e-15, atol=0.0), "the limit basis changed: rerun tools/make_deep_limit_golden.py"
    ref = gold["eri"]
    assert [int(x) for x in t.bas[:, 2]] == [45, 45, 1, 1] and ref.shape == (8,) * 4
    for q, now in zip(_ORACLE_AT_TEST_TIME, nat.int2e_quartets(t, _ORACLE_AT_TEST_TIME)):
        # (1e-13: what the CPU file holds the oracle to; the dense tensor takes the shells of a quartet in another order than
        # int2e_quartets, which moves (1, 1, 2, 0) by 1.2e-14)
        assert np.abs(now - ref[_blk(t, q)]).max() <= 1e-13 * np.abs(ref[_blk(t, q)]).max(), q
    ref.setflags(write=False)
    return t, ref


def _blk(t, q):
    return tuple(slice(int(t.ao_loc[s]), int(t.ao_loc[s + 1])) for s in q)


def test_45_primitive_shells_tiles_vs_oracle(dev, golden_dir):
    """dqc_eri_fill_tiles: the (ss|ss), (ps|ss), (pp|ss) and (pp|pp) quartets wholly on the 45-primitive centre and one mixed
    quartet of each class -- and with them the whole 8-function tensor; the general path walks iq to 45^4 - 1.  0.65 s on the
    MI355X.  (Through the runtime kernel the same table takes 76 s -- one lane group walks the 4.1e6 primitive quartets of a
    quartet -- so that pass is not part of the suite; it was run once: whole tensor 6.5e-13, docs/LOG_r21.md.)"""
    from dqc_amd import lib
    t, ref = _limit(golden_dir)
    tab = lib.Tables(t.atm, t.bas, t.env)
    bound = 1e-11 * max(1.0, np.abs(ref).max())
    err = np.abs(lib.eri_dense(lib.eri_tiles(tab, dev), tab.nao).cpu().numpy() - ref)
    for cls, quartets in _LIMIT_CLASSES.items():
        for q, where in zip(quartets, ("deep centre", "mixed")):
            # non-zero references: the same-centre (ps|ss) vanishes by parity, every other listed block does not
            assert (np.abs(ref[_blk(t, q)]).max() > 0.05) != (q == (1, 0, 0, 0)), (cls, q)
            _worst("limit tiles %s %s" % (cls, where), err[_blk(t, q)].max())
            assert err[_blk(t, q)].max() <= bound, (cls, q, err[_blk(t, q)].max())
    _worst("limit tiles whole tensor", err.max())
    assert err.max() <= bound, (err.max(), np.unravel_index(err.argmax(), err.shape))


def test_45_primitive_shells_direct_jk_vs_oracle(dev, golden_dir):
    """dqc_jk_direct at the limit, with the quartets cut down to what it finishes in a second: the 45-primitive s with the
    partner centre's s and p (the (ss|ss) quartet of 4.1e6 primitive quartets and the mixed ones), J and K of a random
    non-symmetric density against the fixture.  The unscreened pass walks a shell quartet on ONE lane group (no primitive
    split): 1.3 s for this table, 9.3 s for the 45-primitive p alone, 27 s for the whole limit basis (where it was run once:
    J 2.2e-13, K 1.7e-13).  The screened context (dqc_direct_*) needs 45 s for the whole limit basis, bounds included, and is
    not part of the suite either; run once: bounds as the fixture's, J 4.9e-13, K 2.3e-13 at tau = 0 and 1e-13 (docs/LOG_r21.md)"""
    from oracle import basis as ob
    from dqc_amd import lib
    t, ref = _limit(golden_dir)
    deep, other = DC.limit_shells()
    ts = ob.make_tables(([5, 1], np.stack([DC.ORIGIN, DC.ORIGIN + 2.0 * DC.SKEW])), [[deep[0]], other])
    keep = np.array([0, 4, 5, 6, 7])  # the functions of shells 0, 2, 3 of the whole table
    for a, b in zip(ts.bas, t.bas[[0, 2, 3]]):
        assert np.array_equal(ts.env[a[5]:a[5] + 2 * a[2]], t.env[b[5]:b[5] + 2 * b[2]]) and a[1] == b[1]
    sub = ref[np.ix_(keep, keep, keep, keep)]
    tab = lib.Tables(ts.atm, ts.bas, ts.env)
    D = np.random.default_rng(45).standard_normal((5, 5))
    Jr, Kr = _jk_ref(0.5 * (D + D.T), sub)
    J, K = lib.jk_direct(tab, torch.as_tensor(D, device=dev), True)
    ej, ek = rel(J.cpu().numpy(), Jr), rel(K.cpu().numpy(), Kr)
    _worst("limit direct J (45-primitive s)", ej)
    _worst("limit direct K (45-primitive s)", ek)
    assert ej < 1e-12 and ek < 1e-12, (ej, ek)
