"""RI-MP2 nuclear gradients on the GPU: the three-index-density derivative pass dqc_df_grad3 and dqc_amd.mp2_gradient end to end.

Yardsticks:
  * the kernel, class by class: the oracle's analytic derivative integrals (natives.df_ip, Cartesian) contracted here with random
    Z[a, b, k] (symmetric in a, b, otherwise general) and random symmetric G[k, l]; the bar of tests/test_gpu_gradient_terms.py, 1e-10
    of the largest reference component + 1e-13;
  * the kernel against the rank-one pass: with Z = D (x) c, G = c c^T it is dqc_df_grad, the same integrals in another order of the same
    sums, 1e-12 of the largest component; Z walked one auxiliary shell per call, 1e-12;
  * end to end -- the test that fixes the factors: mp2_gradient against the Richardson-extrapolated central difference of
    mp2(HF(Mol(R +- h))).e_tot at h = 1e-3 and 2e-3 Bohr; bound 10 |FD(h) - FD(2h)| + the Z-vector tolerance 1e-9 (the form of the
    bound in tests/test_gpu_mp2_density.py).  Measured on the MI355X: docs/LOG_r29.md."""
import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

TIGHT = {"maxiter": 300, "f_tol": 1e-11}   # (the SCF tolerances of the MP2 tests)
SCS = (1.2, 1.0 / 3.0)
ZTOL = 1e-9
ZS = [8, 1, 1]
POS = [[0.0, 0.0, 0.2217], [0.0, 1.4309, -0.8867], [0.1, -1.4309, -0.8867]]   # H2O, distorted: no symmetry left
_WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    for k in sorted(_WORST):
        print("WORST %-34s %.3e" % (k, _WORST[k]))


def _check(what, g, ref, tol=1e-10, floor=1e-13):
    g, ref = np.asarray(g), np.asarray(ref)
    scale = np.abs(ref).max()
    err = np.abs(g - ref).max()
    _WORST[what] = max(_WORST.get(what, 0.0), err / max(scale, 1e-300))
    assert err <= tol * scale + floor, (what, err, scale)


def _dev(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev).contiguous()


def _ncart(l):
    return (l + 1) * (l + 2) // 2


def _k_grad3(dev, tab, z, g, orb, aux):
    from dqc_amd import lib
    out = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    lib.df_grad3(out, None if z is None else _dev(z, dev), None if g is None else _dev(g, dev), tab, orb, aux)
    return out.cpu().numpy()


class _Ref:
    """sum Z d(ij|k) - 1/2 sum G d(k|l) from the oracle's derivative integrals (computed once per table), rows = atoms of the table
    (natives.df_grad with general densities): orbital centres to the atom of i, the auxiliary centre from its own integrals, (d k|l)
    to the atom of k"""

    def __init__(self, tc, orb, aux, cart=True):
        from oracle import natives as nat
        at = nat.ao_atom(tc, cart)
        n, ao0, ax0 = nat.ao_count(tc, cart, orb), nat.ao_count(tc, cart, (0, orb[0])), nat.ao_count(tc, cart, (0, aux[0]))
        self.natm = tc.natm
        self.orb_at, self.aux_at = at[ao0:ao0 + n], at[ax0:ax0 + nat.ao_count(tc, cart, aux)]
        self.ip3, self.ipk, self.ip2 = (nat.df_ip(w, tc, orb, aux, cart) for w in ("ij|k", "k", "2c"))

    def __call__(self, z, g):
        out = np.zeros((self.natm, 3))
        if z is not None:
            np.add.at(out, self.orb_at, 2.0 * np.einsum("dijk,ijk->id", self.ip3, z))
            np.add.at(out, self.aux_at, np.einsum("dijk,ijk->kd", self.ipk, z))
        if g is not None:
            np.add.at(out, self.aux_at, -np.einsum("dkl,kl->kd", self.ip2, g))
        return out


# ------------------------------------------------------------------------------------------------ 1. the kernel
# one contracted (tight + diffuse) shell of every l = 0 ... 4 per atom: the stratum basis of tests/test_gpu_gradient_terms.py
_SPEC = [[(l, [2.9 + 0.3 * a, 0.42 + 0.05 * l], [0.55, 0.6]) for l in range(5)] for a in range(3)]


@pytest.mark.parametrize("lc", range(5))
def test_df_grad3_class_strata(dev, lc):
    """orbital pairs (la <= lb) up to g on two atoms with auxiliary shells of l = lc on the third and the first atom (the construction
    of test_df_grad_class_strata): every compile-time (la + 1, lb | lc) and (la - 1, lb | lc) class, the runtime kernel for g shells and
    h companions.  Z alone (gmode 3), G alone (gmode 4), both"""
    from oracle import basis as ob
    from dqc_amd import lib
    rng = np.random.default_rng(400 + lc)
    for la in range(5):
        for lb in range(la, 5):
            orb = [[_SPEC[0][la]], [_SPEC[1][lb]], []]
            aux = [[(lc, [0.8], [1.0])], [], [(lc, [0.6], [1.0])]]
            tc, o, x = ob.make_tables_df(M.GRAD3, orb, aux)
            tab = lib.Tables(tc.atm, tc.bas, tc.env)
            n, naux = _ncart(la) + _ncart(lb), 2 * _ncart(lc)
            z = rng.standard_normal((n, n, naux))
            z = z + z.transpose(1, 0, 2)
            g = rng.standard_normal((naux, naux))
            g = g + g.T
            ref = _Ref(tc, o, x)
            _check("grad3 strata Z", _k_grad3(dev, tab, z, None, o, x), ref(z, None))
            _check("grad3 strata G", _k_grad3(dev, tab, None, g, o, x), ref(None, g))
            _check("grad3 strata Z + G", _k_grad3(dev, tab, z, g, o, x), ref(z, g))


def test_df_grad3_equals_the_rank_one_pass_and_walks_in_blocks(dev):
    """CH4 / cc-pVDZ with "etb": Z = D (x) c, G = c c^T against lib.df_grad with (D, c), 1e-12 of the largest component; a general Z one
    auxiliary shell per call (G once, with the first block) against one call, 1e-12; and accumulation into a pre-filled gradient"""
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    tc, orb, aux = ob.make_tables_df(M.CH4, "cc-pvdz", "etb")
    tab = lib.Tables(tc.atm, tc.bas, tc.env)
    rng = np.random.default_rng(19)
    n, naux = nat.ao_count(tc, True, orb), nat.ao_count(tc, True, aux)
    d = rng.standard_normal((n, n)) / n
    d = d + d.T
    c = rng.standard_normal(naux) * 0.1
    dc = np.zeros((n + naux,) * 2)
    dc[:n, :n] = d
    cc = np.zeros(n + naux)
    cc[n:] = c
    g1 = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    lib.df_grad(g1, _dev(dc, dev), _dev(cc, dev), tab, orb, aux)
    g1 = g1.cpu().numpy()
    g3 = _k_grad3(dev, tab, d[:, :, None] * c[None, None, :], np.outer(c, c), orb, aux)
    _check("grad3 = rank-one pass", g3, g1, tol=1e-12, floor=0.0)
    # a general Z, walked
    z = rng.standard_normal((n, n, naux)) / n
    z = z + z.transpose(1, 0, 2)
    gm = rng.standard_normal((naux, naux)) * 0.01
    gm = gm + gm.T
    whole = _k_grad3(dev, tab, z, gm, orb, aux)
    pre = 0.01 * rng.standard_normal((tab.natm, 3))
    out = _dev(pre, dev)
    lib.df_grad3(out, None, _dev(gm, dev), tab, orb, aux)
    c0 = 0
    for k in range(aux[0], aux[1]):
        nc = _ncart(int(tc.bas[k, 1]))
        lib.df_grad3(out, _dev(z[:, :, c0:c0 + nc], dev), None, tab, orb, (k, k + 1))
        c0 += nc
    assert c0 == naux
    _check("grad3 one shell per call", out.cpu().numpy() - pre, whole, tol=1e-12, floor=0.0)


def test_df_grad3_argument_checks_raise_before_any_launch(dev):
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    tc, orb, aux = ob.make_tables_df(M.H2O, "sto-3g", "etb")
    tab = lib.Tables(tc.atm, tc.bas, tc.env)
    n, naux = nat.ao_count(tc, True, orb), nat.ao_count(tc, True, aux)
    grad = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
    z = torch.zeros((n, n, naux), dtype=torch.float64, device=dev)
    g = torch.zeros((naux, naux), dtype=torch.float64, device=dev)
    with lib.call_trace() as tr:
        for bad_z, bad_g, bad_grad in ((z[:, :, :-1].contiguous(), None, grad),      # wrong shape
                                       (z.reshape(naux, n, n), None, grad),
                                       (None, g[:-1].contiguous(), grad),
                                       (z.to(torch.float32), None, grad),            # wrong dtype
                                       (z.cpu(), None, grad),                        # wrong device
                                       (None, g.cpu(), grad),
                                       (z, g, grad[:-1].contiguous()),               # gradient rows: the atoms of the table
                                       (z, g, torch.zeros((3, tab.natm), dtype=torch.float64, device=dev).t())):
            with pytest.raises(lib.DqcAmdError, match="df_grad3"):
                lib.df_grad3(bad_grad, bad_z, bad_g, tab, orb, aux)
        # non-contiguous views of the right shape
        zt = torch.zeros((n, naux, n), dtype=torch.float64, device=dev).transpose(1, 2)
        gt = torch.zeros((naux, 2 * naux), dtype=torch.float64, device=dev)[:, ::2]
        assert tuple(zt.shape) == (n, n, naux) and not zt.is_contiguous() and tuple(gt.shape) == (naux, naux) and not gt.is_contiguous()
        for bad_z, bad_g in ((zt, None), (None, gt)):
            with pytest.raises(lib.DqcAmdError, match="contiguous"):
                lib.df_grad3(grad, bad_z, bad_g, tab, orb, aux)
        # Z of one auxiliary shell handed in for the whole auxiliary range: smaller than the block
        with pytest.raises(lib.DqcAmdError, match="df_grad3"):
            lib.df_grad3(grad, z[:, :, :1].contiguous(), None, tab, orb, aux)
        with pytest.raises(lib.DqcAmdError, match="shell ranges outside the table"):
            lib.df_grad3(grad, z, g, tab, orb, (aux[0], aux[1] + 1))
    assert not tr.rows                               # nothing reached the library
    assert float(grad.abs().max()) == 0.0
    # the C entry point's own size gate, with real operands: an error string, nothing launched, the gradient untouched
    L = lib.load()
    with torch.cuda.device(dev):
        rc = L.dqc_df_grad3(lib._ptr(grad), lib._ptr(z), z.numel() - 1, lib._ptr(g), *tab.args(), orb[0], orb[1], aux[0], aux[1], None)
    assert rc != 0 and "Z is smaller" in L.dqc_last_error().decode()
    assert float(grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. end to end
_RUNS = {}


def _run(basis, atom=None, d=None, m=0):
    """the converged HF calculation of H2O at POS with coordinate (atom, d) moved by m * 1e-3 Bohr, cached"""
    import dqc_amd
    key = (basis, atom, d, m) if m else (basis,)
    if key not in _RUNS:
        pos = [list(p) for p in POS]
        if m:
            pos[atom][d] += m * 1e-3
        qc = dqc_amd.HF(dqc_amd.Mol((ZS, pos), basis=basis))
        qc.run(fwd_options=TIGHT)
        assert qc.accepted
        _RUNS[key] = qc
    return _RUNS[key]


def _fd(basis, atom, d, energy):
    """(FD(h), FD(2h), Richardson) of dE / dR for coordinate (atom, d), h = 1e-3 Bohr"""
    e = {m: energy(_run(basis, atom, d, m)) for m in (1, -1, 2, -2)}
    f1, f2 = (e[1] - e[-1]) / 2e-3, (e[2] - e[-2]) / 4e-3
    return f1, f2, (4.0 * f1 - f2) / 3.0


COMPONENTS = [(0, 2), (1, 1), (2, 0), (2, 2)]     # (O, z), (H1, y), (H2, x), (H2, z)


def test_mp2_gradient_against_finite_differences(dev):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.mp2 import _gradient
    qc = _run("3-21G")
    with lib.call_trace() as tr:
        g = dqc_amd.mp2_gradient(qc, auxbasis="etb", tol=ZTOL)
    assert any(row[0] == "dqc_df_grad3" for row in tr.rows)
    # the separable term is ONE bilinear pass; the quadratic pass is reached through qc.nuclear_gradient() alone (restricted HF: once)
    calls = [row[0] for row in tr.rows]
    assert calls.count("dqc_eri_grad2") == 1 and calls.count("dqc_eri_grad") == 1
    with lib.call_trace() as tr_scf:
        qc.nuclear_gradient()
    assert [row[0] for row in tr_scf.rows].count("dqc_eri_grad") == 1
    assert dqc_amd.mp2_gradient(qc, auxbasis="etb", tol=ZTOL) is g and not g.gradient.requires_grad
    assert isinstance(g, dqc_amd.MP2Gradient) and tuple(g.gradient.shape) == (3, 3)
    assert g.density.relaxed and g.z_residual <= ZTOL and g.naux == dqc_amd.mp2(qc, auxbasis="etb").naux
    assert float((g.scf - qc.nuclear_gradient()).abs().max()) <= 1e-12       # (two runs of the same atomic sums)
    assert float((g.correlation - (g.gradient - g.scf)).abs().max()) == 0.0
    d = dqc_amd.mp2_density(qc, auxbasis="etb", tol=ZTOL)
    assert float((d.dm_mo - g.density.dm_mo).abs().max()) <= 1e-12          # the refactored build gives the density mp2_density gives
    with torch.no_grad():
        _, _, noz = _gradient(qc, "etb", 1.0, 1.0, ZTOL, None, with_z=False)
    grad, scf, corr, noz = g.gradient.cpu(), g.scf.cpu(), g.correlation.cpu(), noz.cpu()
    for atom, k in COMPONENTS:
        s1, s2, sr = _fd("3-21G", atom, k, lambda q: float(q.energy()))
        sbound = 10.0 * abs(s1 - s2) + ZTOL
        print("(%d, %d)  SCF: analytic % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  |diff| %.2e  bound %.2e" % (
            atom, k, float(scf[atom, k]), s1, s2, sr, abs(sr - float(scf[atom, k])), sbound))
        f1, f2, fr = _fd("3-21G", atom, k, lambda q: float(dqc_amd.mp2(q, auxbasis="etb").e_tot))
        bound = 10.0 * abs(f1 - f2) + ZTOL
        print("(%d, %d)  MP2: analytic % .10f  without z % .10f  correlation % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  "
              "|analytic - FD| %.2e  bound %.2e" % (atom, k, float(grad[atom, k]), float(noz[atom, k]), float(corr[atom, k]), f1, f2, fr,
                                                    abs(fr - float(grad[atom, k])), bound))
        assert abs(sr - float(scf[atom, k])) <= sbound                     # the sign and the unit of the finite difference
        assert abs(fr - float(grad[atom, k])) <= bound
        assert abs(float(noz[atom, k]) - float(grad[atom, k])) > bound      # the relaxation is not silently skipped
        assert abs(float(corr[atom, k])) > bound
    tsum = float(grad.sum(0).abs().max())
    print("translational invariance: |sum_A g_A| = %.2e" % tsum)
    assert tsum < 1e-10
    # scaled components
    gs = dqc_amd.mp2_gradient(qc, auxbasis="etb", c_os=SCS[0], c_ss=SCS[1], tol=ZTOL)
    f1, f2, fr = _fd("3-21G", 2, 0, lambda q: float(dqc_amd.mp2(q, auxbasis="etb", c_os=SCS[0], c_ss=SCS[1]).e_tot))
    bound = 10.0 * abs(f1 - f2) + ZTOL
    print("(2, 0)  SCS-MP2: analytic % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  |analytic - FD| %.2e  bound %.2e" % (
        float(gs.gradient[2, 0]), f1, f2, fr, abs(fr - float(gs.gradient[2, 0])), bound))
    assert abs(fr - float(gs.gradient[2, 0])) <= bound
    assert gs.c_os == SCS[0] and gs.c_ss == SCS[1] and abs(float(gs.gradient[2, 0] - g.gradient[2, 0])) > bound
    # one occupied orbital per amplitude block, one auxiliary shell per derivative pass
    g1 = dqc_amd.mp2_gradient(qc, auxbasis="etb", tol=ZTOL, block=1)
    db = float((g1.gradient - g.gradient).abs().max())
    print("block=1 against the default: %.2e" % db)
    assert g1 is not g and g1.density.block == 1 and db <= 1e-12


def test_mp2_gradient_d_shells(dev):
    """cc-pVDZ with "etb": d shells in the orbital basis, auxiliary shells up to f -- the (l + 1, l | f) classes"""
    import dqc_amd
    qc = _run("cc-pvdz")
    g = dqc_amd.mp2_gradient(qc, auxbasis="etb", tol=ZTOL)
    f1, f2, fr = _fd("cc-pvdz", 2, 0, lambda q: float(dqc_amd.mp2(q, auxbasis="etb").e_tot))
    bound = 10.0 * abs(f1 - f2) + ZTOL
    print("(2, 0)  MP2 / cc-pVDZ: analytic % .10f  FD(h) % .10f  FD(2h) % .10f  Richardson % .10f  |analytic - FD| %.2e  bound %.2e" % (
        float(g.gradient[2, 0]), f1, f2, fr, abs(fr - float(g.gradient[2, 0])), bound))
    assert abs(fr - float(g.gradient[2, 0])) <= bound
    assert float(g.gradient.sum(0).abs().max()) < 1e-10


def test_mp2_gradient_refusals(dev, monkeypatch):
    import dqc_amd
    mol = lambda **kw: dqc_amd.Mol((ZS, POS), basis="3-21G", **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match="mp2_gradient: the relaxed density on a Kohn-Sham reference"):
        dqc_amd.mp2_gradient(dqc_amd.KS(mol(grid="sg2"), xc="pbe0").run(), auxbasis="etb")
    with pytest.raises(NotImplementedError, match="mp2_gradient: unrestricted calculations are not supported"):
        dqc_amd.mp2_gradient(dqc_amd.HF(mol(), restricted=False).run(), auxbasis="etb")
    with pytest.raises(NotImplementedError, match="mp2_gradient: the relaxed density needs the orbital Hessian .* `auxbasis=`"):
        dqc_amd.mp2_gradient(dqc_amd.HF(mol().densityfit(auxbasis="etb", exchange=True)).run())
    monkeypatch.setenv("DQC_AMD_ERI", "direct")
    qc = dqc_amd.HF(mol()).run()
    monkeypatch.delenv("DQC_AMD_ERI")
    assert qc._engine.hamilton._direct
    with pytest.raises(NotImplementedError, match="mp2_gradient: the relaxed density needs the orbital Hessian .* `auxbasis=`"):
        dqc_amd.mp2_gradient(qc, auxbasis="etb")
