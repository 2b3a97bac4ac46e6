"""The Rys root / weight and Boys lookups, and the integral kernels that go through them, over the whole range of
X = rho |PQ|^2: every Chebyshev interval of every root count N = 1 ... 9, the switch to the Hermite form at XMAX = 35 + 5 N,
and far beyond it.  Compact molecules keep X small (the f classes of CH4 / HNO cc-pVTZ stay below X = 10, the g-shell test below
3.5), so nothing else in the suite reads most of the tables.

Part A  the device lookups themselves (dqc_probe_rys: rys_roots, rys_root1, rys_root1_lds, rys_root1_rt, boys01_lds) against
        the 50-digit Boys functions of tests/golden/rys_boys_moments.npz (tools/make_rys_golden.py): sum_r w_r u_r^k = F_k for
        k < 2 N -- the moments an integral consumes -- to 2e-13 F_0, the bound tests/test_oracle_cpu.py holds the table to.
Part B  the kernels end to end on a stretched dimer: two centres with one primitive shell of every l = 0 ... 4 and exponent 1/2,
        so that every quartet with its bra on one centre and its ket on the other has p = q = 1, rho = 1/2 and X = R^2 / 2 in
        all classes at once; R runs over a ladder that puts X into every interval of every N (asserted on the host).
        4-centre tiles through the compile-time classes and through the runtime kernel, direct J / K, nuclear attraction,
        2- and 3-centre integrals and the three gradient entry points against the oracle's McMurchie-Davidson integrals; a
        contracted, mixed-exponent dimer beside the idealised one.

Only the tests that launch kernels carry the gpu mark: the coverage of the ladder is host arithmetic."""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

_WORST = {}
_NMAX = {0: 9, 1: 9, 2: 2, 3: 9, 4: 1}  # root counts a probe variant has
_MOMENT_TOL = 2e-13


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    for k in sorted(_WORST):
        print("WORST %-34s %.3e" % (k, _WORST[k]))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "rys_boys_moments.npz"))


def _worst(key, v):
    _WORST[key] = max(_WORST.get(key, 0.0), float(v))


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------
# part A: the lookups
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_rys_lookup_moments_vs_mpmath(dev, gold, variant):
    """every root count of the variant at every argument of the fixture: 0 < u < 1, w > 0 and the 2 N moments"""
    from dqc_amd import lib
    bad = []
    for n in range(1, _NMAX[variant] + 1):
        x, F = gold["x_n%d" % n], gold["f_n%d" % n]
        u, w = lib.probe_rys(variant, n, torch.as_tensor(x, device=dev))
        u, w = u.cpu().numpy(), w.cpu().numpy()
        assert u.shape == (len(x), n) and w.shape == (len(x), n)
        err = np.stack([np.abs((w * u ** k).sum(1) - F[:, k]) / F[:, 0] for k in range(2 * n)], 1)  # (nx, 2n)
        ok = (u > 0).all(1) & (u < 1).all(1) & (w > 0).all(1) & (err <= _MOMENT_TOL).all(1)
        for i in np.nonzero(~ok)[0]:
            bad.append((n, float(x[i]), float(err[i].max())))
            print("variant %d n %d X = %r: moment error %.3e F_0, u in [%.3e, %.3e], min w %.3e"
                  % (variant, n, float(x[i]), err[i].max(), u[i].min(), u[i].max(), w[i].min()))
        good = err[ok]
        _worst("A moments variant %d n %d" % (variant, n), good.max() if good.size else 0.0)
        print("variant %d n %d: worst moment error %.3e F_0 over %d of %d arguments" % (variant, n, _WORST["A moments variant %d n %d" % (variant, n)],
                                                                                       int(ok.sum()), len(x)))
    assert not bad, bad


@gpu
def test_boys01_lookup_vs_mpmath(dev, gold):
    """boys01_lds, the closed-form path of (ss|ss) and (ps|ss) in place of the N = 1 rule: F_0 and F_1 at every node of its
    table, at every half-way point (the largest Taylor step) and its neighbouring doubles, around the switch at 40 and beyond"""
    from dqc_amd import lib
    x, F = gold["x_boys"], gold["f_boys"]
    f0, f1 = lib.probe_rys(4, 1, torch.as_tensor(x, device=dev))
    f0, f1 = f0.cpu().numpy()[:, 0], f1.cpu().numpy()[:, 0]
    e0, e1 = np.abs(f0 - F[:, 0]) / F[:, 0], np.abs(f1 - F[:, 1]) / F[:, 0]
    _worst("A boys01 F_0", e0.max())
    _worst("A boys01 F_1", e1.max())
    print("boys01_lds: worst |f0 - F_0| %.3e F_0 at X = %r, worst |f1 - F_1| %.3e F_0 at X = %r"
          % (e0.max(), float(x[e0.argmax()]), e1.max(), float(x[e1.argmax()])))
    assert (f0 > 0).all() and (f1 > 0).all()
    assert e0.max() <= _MOMENT_TOL and e1.max() <= _MOMENT_TOL, (e0.max(), e1.max())


# ------------------------------------------------------------------------------------------------
# part B: the stretched dimer
# ------------------------------------------------------------------------------------------------
_ZS = [3, 1]
_ORIGIN = np.array([0.1, -0.2, 0.3])
_SKEW = np.array([0.36, -0.48, 0.8])  # a unit vector with no zero component
_LADDER_X = [2.5 * k + 0.3 for k in range(34)] + [150.0, 400.0]
_GEOS = [(X, _SKEW) for X in _LADDER_X] + [(2.5 * 20 + 0.3, np.array([0.0, 0.0, 1.0]))]  # (X, direction): R = sqrt(2 X)
_GRAD_GEOS = [0, 8, 16, 24, 32, 34]  # X = 0.3, 20.3, 40.3, 60.3, 80.3, 150
_CHUNK = 4
_NCHUNK = (len(_GEOS) + _CHUNK - 1) // _CHUNK
_EXP_ORB, _EXP_NUC, _EXP_AUX = 0.5, 0.25, 1.0


def _shells(e):
    return [[(l, [e], [1.0]) for l in range(5)] for _ in range(2)]


def _mol(ig):
    X, d = _GEOS[ig]
    return (_ZS, np.stack([_ORIGIN, _ORIGIN + np.sqrt(2.0 * X) * d]))


def _x_of(ig, rho):
    """X = rho |PQ|^2 of the quartets (pairs, nuclei) that sit on different centres, from the coordinates the kernels get"""
    pos = _mol(ig)[1]
    return rho * float(((pos[1] - pos[0]) ** 2).sum())


def _bucket(n, X):
    return "asym" if X >= 35.0 + 5.0 * n else int(X / 2.5)


# entry point -> (rho of its cross-centre integrals, largest root count): 4-centre (aa|bb): p = q = 2 a; nuclear attraction of a
# same-centre pair with the other nucleus: p = 2 a'; 2-centre (k|l): rho = b / 2; 3-centre (aa|k): p = 2 a, q = b
_ENTRY = {"4-centre": (_EXP_ORB, 9), "nuclear attraction": (2 * _EXP_NUC, 5), "2-centre": (_EXP_AUX / 2, 5),
          "3-centre": (2 * _EXP_ORB * _EXP_AUX / (2 * _EXP_ORB + _EXP_AUX), 7)}


def test_ladder_reaches_every_interval_of_every_root_count():
    """host arithmetic only: over the geometries, X lands in every Chebyshev interval and in the Hermite branch of every N an
    entry point can reach"""
    assert abs(float(_SKEW @ _SKEW) - 1.0) < 1e-15
    for name, (rho, nmax) in _ENTRY.items():
        assert rho == 0.5, name
        got = {(n, _bucket(n, _x_of(ig, rho))) for ig in range(len(_GEOS)) for n in range(1, nmax + 1)}
        need = {(n, b) for n in range(1, nmax + 1) for b in list(range(14 + 2 * n)) + ["asym"]}
        assert need <= got, (name, sorted(need - got, key=str))
    assert [round(_x_of(ig, 0.5), 6) for ig in _GRAD_GEOS] == [0.3, 20.3, 40.3, 60.3, 80.3, 150.0]
    chunks = [ig for c in range(_NCHUNK) for ig in range(len(_GEOS))[c * _CHUNK:(c + 1) * _CHUNK]]
    assert chunks == list(range(len(_GEOS)))


_L_AO = np.repeat(np.arange(5), 2 * np.arange(5) + 1)  # l of the 25 functions of one centre
# root count of the cross quartets (aa|bb), per element of the (25,)*4 block
_N_CROSS = (_L_AO[:, None, None, None] + _L_AO[None, :, None, None] + _L_AO[None, None, :, None] + _L_AO[None, None, None, :]) // 2 + 1


def _eri_check(what, dense, ref):
    err = np.abs(dense - ref)
    cross = err[:25, :25, 25:, 25:]
    for n in range(1, 10):
        _worst("B %s cross quartets N %d" % (what, n), cross[_N_CROSS == n].max())
    assert err.max() <= 1e-11 * max(1.0, np.abs(ref).max()), (what, err.max(), np.unravel_index(err.argmax(), err.shape))


@gpu
@pytest.mark.parametrize("chunk", range(_NCHUNK))
def test_stretched_dimer_integrals_vs_oracle(dev, chunk):
    """per geometry: the ERI tensor through the compile-time classes (g: runtime kernel) and with every class through the
    runtime kernel, direct J / K of a random density, nuclear attraction, (k|l) and (ij|k)"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    for ig in range(len(_GEOS))[chunk * _CHUNK:(chunk + 1) * _CHUNK]:
        mol = _mol(ig)
        t = ob.make_tables(mol, _shells(_EXP_ORB))
        tab = lib.Tables(t.atm, t.bas, t.env)
        assert tab.nao == 50
        ref = nat.int2e(t)
        # (what the absolute bound bites on: the cross quartets are not negligible)
        if _x_of(ig, 0.5) > 10:
            assert 1e-3 < np.abs(ref[:25, :25, 25:, 25:]).max() < 1.0
        _eri_check("tiles", lib.eri_dense(lib.eri_tiles(tab, dev), tab.nao).cpu().numpy(), ref)
        prev = lib.set_generic_eri(True)
        try:
            dense = lib.eri_dense(lib.eri_tiles(tab, dev), tab.nao).cpu().numpy()
        finally:
            lib.set_generic_eri(prev)
        _eri_check("tiles runtime kernel", dense, ref)
        D = np.random.default_rng(100 + ig).standard_normal((tab.nao, tab.nao))
        Ds = 0.5 * (D + D.T)
        J, K = lib.jk_direct(tab, torch.as_tensor(D, device=dev), True)
        ej, ek = rel(J.cpu().numpy(), np.einsum("ij,ijkl->kl", Ds, ref)), rel(K.cpu().numpy(), np.einsum("il,ijkl->jk", Ds, ref))
        _worst("B direct J", ej)
        _worst("B direct K", ek)
        assert ej < 1e-12 and ek < 1e-12, (ig, ej, ek)
        tn = ob.make_tables(mol, _shells(_EXP_NUC))
        en = rel(lib.int1e("nuc", lib.Tables(tn.atm, tn.bas, tn.env), dev).cpu().numpy(), nat.int1e("nuc", tn))
        _worst("B nuclear attraction", en)
        assert en < 1e-12, (ig, en)
        tc, orb, aux = ob.make_tables_df(mol, _shells(_EXP_ORB), _shells(_EXP_AUX))
        tabc = lib.Tables(tc.atm, tc.bas, tc.env)
        e2 = rel(lib.int2c2e(tabc, aux, dev).cpu().numpy(), nat.int2c2e(tc, aux))
        e3 = rel(lib.int3c2e(tabc, orb, aux, dev).cpu().numpy(), nat.int3c2e(tc, orb, aux))
        _worst("B 2-centre", e2)
        _worst("B 3-centre", e3)
        assert e2 < 1e-12 and e3 < 1e-12, (ig, e2, e3)


def _block_diag_sym(rng, n):
    """symmetric, non-zero in the two same-centre blocks only: products D_ab D_cd pair centre with centre, and the gradient
    comes from the quartets (aa|bb) at X = R^2 / 2"""
    out = np.zeros((2 * n, 2 * n))
    for c in range(2):
        a = rng.standard_normal((n, n))
        out[c * n:(c + 1) * n, c * n:(c + 1) * n] = a + a.T
    return out


@gpu
@pytest.mark.parametrize("ig", _GRAD_GEOS)
def test_stretched_dimer_gradients_vs_oracle(dev, ig):
    """dqc_eri_grad (compile-time classes and the runtime kernel), dqc_int1e_grad and dqc_df_grad with Cartesian densities on
    the same-centre blocks, against the oracle's analytic derivative integrals; called, and bounded, as in
    tests/test_gpu_gradient_terms.py: 1e-10 of the largest reference component plus 1e-13"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    from tests.test_gpu_gradient_terms import _check, _k_df, _k_eri, _k_int1e, _WORST as worst_g
    mol = _mol(ig)
    rng = np.random.default_rng(500 + ig)
    nc = 35  # Cartesian functions of one centre
    t = ob.make_tables(mol, _shells(_EXP_ORB))
    tab = lib.Tables(t.atm, t.bas, t.env)
    assert nat.ao_count(t, cart=True) == 2 * nc
    D = _block_diag_sym(rng, nc)
    ref = nat.eri_grad(t, D, 1.0, 0.5, cart=True)
    _check("rys range eri_grad", _k_eri(dev, tab, D, 1.0, 0.5), ref)
    prev = lib.set_generic_eri(True)
    try:
        g = _k_eri(dev, tab, D, 1.0, 0.5)
    finally:
        lib.set_generic_eri(prev)
    _check("rys range eri_grad runtime kernel", g, ref)
    tn = ob.make_tables(mol, _shells(_EXP_NUC))
    W = _block_diag_sym(rng, nc)
    _check("rys range int1e_grad", _k_int1e(dev, lib.Tables(tn.atm, tn.bas, tn.env), D, W), nat.int1e_grad(tn, D, W, cart=True))
    tc, orb, aux = ob.make_tables_df(mol, _shells(_EXP_ORB), _shells(_EXP_AUX))
    tabc = lib.Tables(tc.atm, tc.bas, tc.env)
    n, naux = nat.ao_count(tc, True, orb), nat.ao_count(tc, True, aux)
    assert (n, naux) == (2 * nc, 2 * nc)
    c = rng.standard_normal(naux)
    dc = np.zeros((n + naux,) * 2)
    dc[:n, :n] = D
    cc = np.zeros(n + naux)
    cc[n:] = c
    _check("rys range df_grad", _k_df(dev, tabc, dc, cc, orb, aux), nat.df_grad(tc, orb, aux, D, c, cart=True))
    for k, v in worst_g.items():
        if k.startswith("rys range"):
            _worst("B " + k[10:], v)


# a contracted, mixed-exponent dimer: two s contractions over one exponent set (merged by the grouped general-contraction path
# when the basis has no g shell: the second basis), a contracted p, and d, f, g
_S_EXP = [50.0, 8.0, 1.5]
_REAL_G = [(0, _S_EXP, [0.15, 0.55, 0.45]), (0, _S_EXP, [-0.05, -0.2, 1.0]), (1, [3.0, 0.6], [0.4, 0.7]), (2, [1.9], [1.0]),
           (3, [1.1], [1.0]), (4, [0.7], [1.0])]


@gpu
@pytest.mark.parametrize("R", [2.0, 6.0, 15.0])
def test_contracted_dimer_integrals_vs_oracle(dev, R):
    """the full tensor and direct J / K at a bonded, a stretched and a far distance, with and without the g shell"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    mol = ([7, 6], np.stack([_ORIGIN, _ORIGIN + R * _SKEW]))
    for name, shells in (("s-g", _REAL_G), ("s-f", _REAL_G[:-1])):
        t = ob.make_tables(mol, [shells, shells])
        tab = lib.Tables(t.atm, t.bas, t.env)
        ref = nat.int2e(t)
        err = np.abs(lib.eri_dense(lib.eri_tiles(tab, dev), tab.nao).cpu().numpy() - ref).max()
        _worst("B contracted dimer tiles " + name, err)
        assert err <= 1e-11 * max(1.0, np.abs(ref).max()), (name, R, err)
        D = np.random.default_rng(int(R)).standard_normal((tab.nao, tab.nao))
        Ds = 0.5 * (D + D.T)
        J, K = lib.jk_direct(tab, torch.as_tensor(D, device=dev), True)
        ej, ek = rel(J.cpu().numpy(), np.einsum("ij,ijkl->kl", Ds, ref)), rel(K.cpu().numpy(), np.einsum("il,ijkl->jk", Ds, ref))
        _worst("B contracted dimer J " + name, ej)
        _worst("B contracted dimer K " + name, ek)
        assert ej < 1e-12 and ek < 1e-12, (name, R, ej, ek)
