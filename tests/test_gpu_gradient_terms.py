"""GPU tests (-m gpu) of the integral-derivative kernels of csrc/grad.hip against the oracle's analytic derivative integrals
(oracle/cint_oracle.c: orc_int1e_ip, orc_eri_grad, orc_df_ip -- themselves pinned to finite differences of the oracle
integrals in tests/test_oracle_cpu.py).

The inputs are NOT SCF densities: a converged density puts little weight on many shell pairs, so a wrong class hides in a
total gradient.  Class-stratified densities (non-zero on a few chosen shells only) isolate every angular-momentum
combination; whole bases take random Cartesian densities and the production form D_cart = T^T D T.  Tolerance: 1e-10 of the
largest reference component (plus a 1e-13 floor), per atom and component."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    for k in sorted(_WORST):
        print("WORST %-28s %.3e" % (k, _WORST[k]))


def _check(what, g, ref, tol=1e-10):
    g, ref = np.asarray(g), np.asarray(ref)
    scale = np.abs(ref).max()
    err = np.abs(g - ref).max()
    _WORST[what] = max(_WORST.get(what, 0.0), err / max(scale, 1e-300))
    assert err <= tol * scale + 1e-13, (what, err, scale)


def _dev(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev).contiguous()


def _ncart(l):
    return (l + 1) * (l + 2) // 2


def _tabs(mol, basis):
    from oracle import basis as ob
    from dqc_amd import lib
    t = ob.make_tables(mol, basis)
    return t, lib.Tables(t.atm, t.bas, t.env)


def _sym(rng, n):
    a = rng.standard_normal((n, n))
    return a + a.T


def _k_int1e(dev, tab, dc, wc, zs=None, g0=None):
    from dqc_amd import lib
    g = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev) if g0 is None else _dev(g0, dev)
    lib.int1e_grad(g, _dev(dc, dev), _dev(wc, dev), tab, zs)
    return g.cpu().numpy()


def _k_eri(dev, tab, dc, js, ks):
    from dqc_amd import lib
    g = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    lib.eri_grad(g, _dev(dc, dev), ks, tab, jscale=js)
    return g.cpu().numpy()


def _k_df(dev, tab, dc, cc, orb, aux):
    from dqc_amd import lib
    g = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    lib.df_grad(g, _dev(dc, dev), _dev(cc, dev), tab, orb, aux)
    return g.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# class-stratified densities: three atoms of M.GRAD3, one contracted (tight + diffuse) shell of every l = 0 ... 4 on each
# ------------------------------------------------------------------------------------------------
_SPEC = [[(l, [2.9 + 0.3 * a, 0.42 + 0.05 * l], [0.55, 0.6]) for l in range(5)] for a in range(3)]


def _strat_cart(full_t, pick, block):
    """a Cartesian matrix of the full stratum basis that is `block` on the picked shells (atom, l) and zero elsewhere"""
    offs = np.concatenate([[0], np.cumsum([_ncart(int(l)) for l in full_t.bas[:, 1]])])
    idx = np.concatenate([np.arange(offs[a * 5 + l], offs[a * 5 + l + 1]) for (a, l) in pick])
    out = np.zeros((offs[-1], offs[-1]))
    out[np.ix_(idx, idx)] = block
    return out


@pytest.fixture(scope="module")
def strat(dev):
    return _tabs(M.GRAD3, _SPEC)


@pytest.mark.parametrize("la", range(5))
def test_int1e_grad_class_strata(dev, strat, la):
    """<d a|S>, <d a|T|b>, <d a|V|b> and the Hellmann-Feynman terms of all three nuclei for every pair (la, lb), D and W
    independent random matrices on the two shells only"""
    from oracle import basis as ob, natives as nat
    ft, ftab = strat
    rng = np.random.default_rng(100 + la)
    for lb in range(5):
        sub = ob.make_tables(M.GRAD3, [[_SPEC[0][la]], [_SPEC[1][lb]], []])  # the third atom: nucleus only
        n = _ncart(la) + _ncart(lb)
        D, W = _sym(rng, n), _sym(rng, n)
        ref = nat.int1e_grad(sub, D, W, cart=True)
        g = _k_int1e(dev, ftab, _strat_cart(ft, [(0, la), (1, lb)], D), _strat_cart(ft, [(0, la), (1, lb)], W))
        _check("int1e strata", g, ref)
        # the same pair with both shells on ONE atom (no basis-centre term survives: only Hellmann-Feynman and the other nuclei)
        sub2 = ob.make_tables(M.GRAD3, [[_SPEC[0][la], _SPEC[0][lb]] if la != lb else [_SPEC[0][la]], [], []])
        n2 = _ncart(la) + (_ncart(lb) if la != lb else 0)
        D2, W2 = _sym(rng, n2), _sym(rng, n2)
        pick = [(0, la), (0, lb)] if la != lb else [(0, la)]
        ref2 = nat.int1e_grad(sub2, D2, W2, cart=True)
        g2 = _k_int1e(dev, ftab, _strat_cart(ft, pick, D2), _strat_cart(ft, pick, W2))
        _check("int1e strata", g2, ref2)


_TRIPLES = [(a, b, c) for a in range(5) for b in range(a, 5) for c in range(b, 5)]


@pytest.mark.parametrize("la", range(5))
def test_eri_grad_class_strata(dev, strat, la):
    """every shell triple (la <= lb <= lc) on three different atoms, D random on those shells only: each J and K term is
    a quartet inside the triple, so every angular combination (up to h companions and the runtime-kernel classes) is
    isolated; jscale and kscale one at a time"""
    from oracle import basis as ob, natives as nat
    ft, ftab = strat
    rng = np.random.default_rng(200 + la)
    for (_, lb, lc) in [x for x in _TRIPLES if x[0] == la]:
        sub = ob.make_tables(M.GRAD3, [[_SPEC[0][la]], [_SPEC[1][lb]], [_SPEC[2][lc]]])
        n = _ncart(la) + _ncart(lb) + _ncart(lc)
        D = _sym(rng, n)
        Df = _strat_cart(ft, [(0, la), (1, lb), (2, lc)], D)
        for js, ks in ((1.0, 0.0), (0.0, 1.0)):
            _check("eri strata", _k_eri(dev, ftab, Df, js, ks), nat.eri_grad(sub, D, js, ks, cart=True))


@pytest.mark.parametrize("lc", range(5))
def test_df_grad_class_strata(dev, lc):
    """orbital pairs (la, lb) up to g on two atoms with auxiliary shells of l = lc on the third and the first atom:
    gmode 2 (the (d k|l) term) alone with D = 0, then both terms"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    rng = np.random.default_rng(300 + lc)
    for la in range(5):
        for lb in range(la, 5):
            orb = [[_SPEC[0][la]], [_SPEC[1][lb]], []]
            aux = [[(lc, [0.8], [1.0])], [], [(lc, [0.6], [1.0])]]
            tc, o, x = ob.make_tables_df(M.GRAD3, orb, aux)
            tab = lib.Tables(tc.atm, tc.bas, tc.env)
            n, naux = _ncart(la) + _ncart(lb), 2 * _ncart(lc)
            D, c = _sym(rng, n), rng.standard_normal(naux)
            dc = np.zeros((n + naux,) * 2)
            cc = np.zeros(n + naux)
            cc[n:] = c
            _check("df strata gmode 2", _k_df(dev, tab, dc, cc, o, x), nat.df_grad(tc, o, x, np.zeros((n, n)), c, cart=True))
            dc[:n, :n] = D
            _check("df strata gmode 1+2", _k_df(dev, tab, dc, cc, o, x), nat.df_grad(tc, o, x, D, c, cart=True))


# ------------------------------------------------------------------------------------------------
# whole bases
# ------------------------------------------------------------------------------------------------
_WHOLE = [("h2o-sto3g", M.H2O, "sto-3g"), ("ch4-ccpvdz", M.CH4, "cc-pvdz"), ("ch4-ccpvtz", M.CH4, "cc-pvtz"),
          ("hno-ccpvtz", M.HNO, "cc-pvtz"), ("co-6311ppgss", ([6, 8], [[-1.0, 0.1, 0], [1.1, 0, 0.05]]), "6-311++G**")]


@pytest.mark.parametrize("name,mol,basis", _WHOLE, ids=[w[0] for w in _WHOLE])
def test_gradient_terms_whole_basis(dev, name, mol, basis):
    """a random symmetric Cartesian D (every Cartesian component independent), and the production form D_cart = T^T D T against
    the spherical oracle; jscale / kscale = (1, 0), (0, 1) and a general pair, which must be the linear combination"""
    from oracle import natives as nat
    from dqc_amd import lib
    t, tab = _tabs(mol, basis)
    rng = np.random.default_rng(7)
    nc = nat.ao_count(t, cart=True)
    Dc, Wc = _sym(rng, nc) / nc, _sym(rng, nc) / nc
    _check("int1e whole cart", _k_int1e(dev, tab, Dc, Wc), nat.int1e_grad(t, Dc, Wc, cart=True))
    _check("eri whole cart", _k_eri(dev, tab, Dc, 1.0, 1.0), nat.eri_grad(t, Dc, 1.0, 1.0, cart=True))
    T = lib.cart2sph_matrix(tab, "cpu").numpy()
    D, W = _sym(rng, t.nao) / t.nao, _sym(rng, t.nao) / t.nao
    _check("int1e whole T^T D T", _k_int1e(dev, tab, T.T @ D @ T, T.T @ W @ T), nat.int1e_grad(t, D, W))
    r10, r01 = nat.eri_grad(t, D, 1.0, 0.0), nat.eri_grad(t, D, 0.0, 1.0)
    g10, g01 = _k_eri(dev, tab, T.T @ D @ T, 1.0, 0.0), _k_eri(dev, tab, T.T @ D @ T, 0.0, 1.0)
    _check("eri whole jscale", g10, r10)
    _check("eri whole kscale", g01, r01)
    g = _k_eri(dev, tab, T.T @ D @ T, 0.37, -1.21)
    _check("eri whole general pair", g, 0.37 * r10 - 1.21 * r01)
    assert np.abs(g - (0.37 * g10 - 1.21 * g01)).max() <= 1e-12 * np.abs(g).max()


def test_df_grad_whole_basis_and_host_fold(dev):
    """dqc_df_grad on CH4 / cc-pVDZ with the even-tempered auxiliary basis (Cartesian random D and c, and the production form);
    gradient._df_coulomb_gradient (fit coefficients, Cartesian transforms, the fold of the twice-listed atoms) against the
    oracle contraction with c = M^-1 t from the oracle's own 3- and 2-centre integrals"""
    import dqc_amd
    from dqc_amd import gradient as G, lib
    from oracle import basis as ob, natives as nat
    tc, orb, aux = ob.make_tables_df(M.CH4, "cc-pvdz", "etb")
    tab = lib.Tables(tc.atm, tc.bas, tc.env)
    rng = np.random.default_rng(9)
    n, naux = nat.ao_count(tc, True, orb), nat.ao_count(tc, True, aux)
    D, c = _sym(rng, n) / n, rng.standard_normal(naux) * 0.1
    dc = np.zeros((n + naux,) * 2)
    dc[:n, :n] = D
    cc = np.zeros(n + naux)
    cc[n:] = c
    _check("df whole cart", _k_df(dev, tab, dc, cc, orb, aux), nat.df_grad(tc, orb, aux, D, c, cart=True))
    # the host assembly of a density-fitted Hamiltonian (of an LDA run: density fitting has no exact exchange)
    m = dqc_amd.Mol(M.CH4, basis="cc-pvdz", grid=3).densityfit(auxbasis="etb")
    h = dqc_amd.KS(m, xc="lda_x").run()._engine.hamilton
    tc2, orb2, aux2 = ob.make_tables_df(M.CH4, "cc-pvdz", "etb")
    ns = nat.ao_count(tc2, False, orb2)
    Ds = _sym(rng, ns) / ns
    j3 = nat.int3c2e(tc2, orb2, aux2)
    csp = np.linalg.solve(nat.int2c2e(tc2, aux2), np.einsum("ijk,ij->k", j3, Ds))
    ref = nat.df_grad(tc2, orb2, aux2, Ds, csp)
    g = torch.zeros((5, 3), dtype=torch.float64, device=dev)
    G._df_coulomb_gradient(h, _dev(Ds, dev), g)
    _check("df host fold", g.cpu().numpy(), ref[:5] + ref[5:], tol=1e-9)


# ------------------------------------------------------------------------------------------------
# edges of dqc_int1e_grad: the y-stride over the nuclei (natm > 32), fractional charges, ghosts, +=, streams
# ------------------------------------------------------------------------------------------------
def _cluster(natm, seed):
    """natm atoms (C and H) on a jittered cubic lattice, 2.4 Bohr apart, with sto-3g; one atom is a Z = 0 ghost carrying the
    hydrogen shells"""
    from oracle import basis as ob
    from dqc_amd import lib
    rng = np.random.default_rng(seed)
    k = int(np.ceil(natm ** (1 / 3)))
    pts = np.array([(i, j, l) for i in range(k) for j in range(k) for l in range(k)][:natm], dtype=float) * 2.4
    pts += rng.uniform(-0.3, 0.3, pts.shape)
    zs = [6 if i % 5 == 0 else 1 for i in range(natm)]
    shells = [ob.loadbasis(z, "sto-3g") for z in zs]
    zs[3] = 0
    t = ob.Tables(zs, pts, shells)
    return t, lib.Tables(t.atm, t.bas, t.env)


@pytest.mark.parametrize("natm", [31, 32, 33, 70])
def test_int1e_grad_many_atoms_fractional_charges_ghost(dev, natm):
    """gridDim.y = min(natm, 32): one nucleus per y-slice up to 32 atoms, the strided loop with per-pair atomics above; integer
    and fractional charges; a Z = 0 ghost with shells; accumulation into a pre-filled gradient"""
    from oracle import natives as nat
    t, tab = _cluster(natm, natm)
    rng = np.random.default_rng(natm)
    nc = nat.ao_count(t, cart=True)
    D, W = _sym(rng, nc) / nc, _sym(rng, nc) / nc
    _check("int1e natm<=32" if natm <= 32 else "int1e natm>32", _k_int1e(dev, tab, D, W), nat.int1e_grad(t, D, W, cart=True))
    zs = t.atomzs.astype(float) + rng.uniform(-0.4, 0.4, natm)
    zs[3] = 0.0
    g0 = rng.standard_normal((natm, 3))
    ref = nat.int1e_grad(t, D, W, zs, cart=True)
    _check("int1e fractional zs", _k_int1e(dev, tab, D, W, zs, g0) - g0, ref)
    assert np.abs(_k_int1e(dev, tab, D, W, zs, g0) - (g0 + ref)).max() <= 1e-10 * np.abs(ref).max() + 1e-13


def test_grad_kernels_on_a_side_stream_accumulate(dev):
    """all three entry points called on a non-default torch stream add to a pre-filled gradient"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    t, tab = _tabs(M.HNO, "cc-pvdz")
    rng = np.random.default_rng(11)
    nc = nat.ao_count(t, cart=True)
    D, W = _sym(rng, nc) / nc, _sym(rng, nc) / nc
    g0 = rng.standard_normal((3, 3))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g1, g2 = _dev(g0, dev), _dev(g0, dev)
        Dd, Wd = _dev(D, dev), _dev(W, dev)
        lib.int1e_grad(g1, Dd, Wd, tab)
        lib.eri_grad(g2, Dd, 0.8, tab, jscale=0.6)
    s.synchronize()
    _check("int1e side stream", g1.cpu().numpy() - g0, nat.int1e_grad(t, D, W, cart=True))
    _check("eri side stream", g2.cpu().numpy() - g0, nat.eri_grad(t, D, 0.6, 0.8, cart=True))
    tc, orb, aux = ob.make_tables_df(M.HNO, "cc-pvdz", "etb")
    tabc = lib.Tables(tc.atm, tc.bas, tc.env)
    n, naux = nat.ao_count(tc, True, orb), nat.ao_count(tc, True, aux)
    dc = np.zeros((n + naux,) * 2)
    dc[:n, :n] = _sym(rng, n) / n
    cc = np.zeros(n + naux)
    cc[n:] = rng.standard_normal(naux) * 0.1
    g06 = rng.standard_normal((6, 3))
    with torch.cuda.stream(s):
        g3 = _dev(g06, dev)
        lib.df_grad(g3, _dev(dc, dev), _dev(cc, dev), tabc, orb, aux)
    s.synchronize()
    _check("df side stream", g3.cpu().numpy() - g06, nat.df_grad(tc, orb, aux, dc[:n, :n], cc[n:], cart=True))


_PATH_WORKER = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from dqc_amd import lib
from oracle import basis as ob
from tests import molecules as M
dev = torch.device("cuda")
t = ob.make_tables(M.CH4, "cc-pvtz")
tab = lib.Tables(t.atm, t.bas, t.env)
T = lib.cart2sph_matrix(tab, dev)
rng = np.random.default_rng(4)
a = rng.standard_normal((t.nao, t.nao))
D = torch.as_tensor((a + a.T) / t.nao, device=dev)
g = torch.zeros((5, 3), dtype=torch.float64, device=dev)
lib.eri_grad(g, (T.T @ D @ T).contiguous(), 0.7, tab, jscale=1.1)
tc, orb, aux = ob.make_tables_df(M.CH4, "cc-pvtz", "etb")
tabc = lib.Tables(tc.atm, tc.bas, tc.env)
Tc = lib.cart2sph_matrix(tabc, dev)
n = t.nao
dbig = torch.zeros((Tc.shape[0],) * 2, dtype=torch.float64, device=dev)
dbig[:n, :n] = D
cbig = torch.zeros(Tc.shape[0], dtype=torch.float64, device=dev)
cbig[n:] = torch.as_tensor(rng.standard_normal(Tc.shape[0] - n) * 0.1, device=dev)
g6 = torch.zeros((10, 3), dtype=torch.float64, device=dev)
lib.df_grad(g6, (Tc.T @ dbig @ Tc).contiguous(), (Tc.T @ cbig).contiguous(), tabc, orb, aux)
torch.cuda.synchronize()
np.save(sys.argv[2], np.concatenate([g.cpu().numpy(), g6.cpu().numpy()]))
"""


def test_eri_grad_side_stream_and_wave_map_paths(dev, tmp_path):
    """DQC_SIDE_STREAMS=0 (every class launch on the caller's stream) and DQC_GRAD_WMAP=1 (the depth-binned wave map for every
    class pair) -- both read once per process, hence fresh worker processes -- give the default path's gradient to the
    round-off of its atomics, and the default path matches the oracle"""
    from oracle import basis as ob, natives as nat
    res = {}
    for name, extra in (("default", {}), ("noside", {"DQC_SIDE_STREAMS": "0"}), ("wmap", {"DQC_GRAD_WMAP": "1"})):
        out = str(tmp_path / ("g_%s.npy" % name))
        env = dict(os.environ, **extra)
        for k in ("DQC_SIDE_STREAMS", "DQC_GRAD_WMAP"):
            if k not in extra:
                env.pop(k, None)
        r = subprocess.run([sys.executable, "-c", _PATH_WORKER, ROOT, out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        res[name] = np.load(out)
    for name in ("noside", "wmap"):
        _check("eri/df path " + name, res[name], res["default"], tol=1e-12)
    t = ob.make_tables(M.CH4, "cc-pvtz")
    rng = np.random.default_rng(4)
    a = rng.standard_normal((t.nao, t.nao))
    _check("eri path default vs oracle", res["default"][:5], nat.eri_grad(t, (a + a.T) / t.nao, 1.1, 0.7))


# ------------------------------------------------------------------------------------------------
# end to end: HF gradients assembled from the oracle's derivative integrals around the GPU's converged D and F
# ------------------------------------------------------------------------------------------------
def _frac_weights():
    from dqc_amd.utils.datastruct import SpinParam
    f = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    return SpinParam(u=f([1, 1, 1, 1, 0.7, 0.3]), d=f([1, 1, 1, 1, 0.55, 0.45]))


_E2E = [("rhf", M.H2O, {}, True), ("uhf", ([7, 1, 1], [[0, 0, 0.1], [0, 1.6, -0.9], [0.2, -1.5, -1.0]]), {"spin": 1}, True),
        ("frac", M.H2O, {"orb_weights": "frac"}, True), ("nonorth", M.H2O, {"orthogonalize_basis": False}, True)]


@pytest.mark.parametrize("name,mol,kw,restricted", _E2E, ids=[e[0] for e in _E2E])
def test_hf_gradient_assembled_from_oracle_integrals(dev, name, mol, kw, restricted):
    """qc.nuclear_gradient() == sum D dh - sum W dS + two-electron term (oracle) + nuclear repulsion, with D the GPU's converged
    density and W from a numpy eigendecomposition of its converged Fock matrix (occupation-weighted): checks tocart, the
    UHF jscale / kscale split, the uniform-occupation shortcut and the eigenvector route (fractional occupations,
    orthogonalize_basis=False)"""
    import scipy.linalg
    import dqc_amd
    from oracle import natives as nat
    if kw.get("orb_weights") == "frac":
        kw = dict(kw, orb_weights=_frac_weights())
    m = dqc_amd.Mol(mol, basis="cc-pvdz", **kw)
    qc = dqc_amd.HF(m).run(fwd_options={"f_tol": 1e-12, "maxiter": 300})
    assert qc.accepted
    g = qc.nuclear_gradient().cpu().numpy()
    eng = qc._engine
    h = eng.hamilton
    X = h._orthozer.cpu().numpy()
    pol = eng.polarized
    dms = [qc._dm.u, qc._dm.d] if pol else [qc._dm]
    focks = [qc._fock[0], qc._fock[1]] if pol else [qc._fock]
    ws = [eng.orb_weight.u, eng.orb_weight.d] if pol else [eng.orb_weight]
    Sb = None if eng._sinvh is None else eng.ovlp.cpu().numpy()
    d_aos, W = [], 0.0
    for dm, f, w in zip(dms, focks, ws):
        d = X @ dm.cpu().numpy() @ X.T
        d_aos.append(0.5 * (d + d.T))
        f = f.cpu().numpy()
        eps, C = scipy.linalg.eigh(0.5 * (f + f.T), Sb)
        w = w.cpu().numpy()
        C = X @ C[:, :len(w)]
        W = W + (C * (w * eps[:len(w)])) @ C.T
    from oracle import basis as ob
    zs, pos = ob.parse_moldesc(mol)
    t = ob.make_tables((zs, pos), "cc-pvdz")
    Dt = sum(d_aos)
    ref = nat.int1e_grad(t, Dt, W)
    if pol:
        ref += nat.eri_grad(t, Dt, 1.0, 0.0) + sum(nat.eri_grad(t, d, 0.0, 2.0) for d in d_aos)
    else:
        ref += nat.eri_grad(t, Dt, 1.0, 1.0)
    dr = pos[:, None, :] - pos[None, :, :]
    r = np.linalg.norm(dr, axis=-1) + np.eye(len(zs))
    f = zs[:, None] * zs[None, :] / r ** 3
    np.fill_diagonal(f, 0.0)
    ref -= (f[..., None] * dr).sum(1)
    err = np.abs(g - ref).max()
    _WORST["hf e2e " + name] = err
    assert err < 1e-9, (name, err)
