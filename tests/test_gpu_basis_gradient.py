"""GPU tests (-m gpu) of the derivative of the SCF energy by basis-set exponents and contraction coefficients:
dqc_int1e_grad_basis / dqc_eri_grad_basis (csrc/grad.hip, the basis-parameter branch of the GRAD epilogues), the XC term
(gradient._xc_basis_gradient), gradient.basis_gradient and its autograd chain to the caller's CGTOBasis tensors.

References are central differences, Richardson-extrapolated from relative steps h and h / 2:
    fd_h = (E(theta (1 + h)) - E(theta (1 - h))) / (2 h theta),     ref = (4 fd_{h/2} - fd_h) / 3.
The bar per entry is 4 |fd_h - fd_{h/2}| + 1e-10 max|ref|: |fd_h - fd_{h/2}| is 3/4 of fd_h's own h^2 error, i.e. the reference's
error estimate BEFORE the extrapolation, with a margin of 4.  h = 1e-3: the round-off of a difference, 1e-16 |E| / (h theta), stays
two to three orders under the 1e-10 floor, which matters where E is a low polynomial in the parameter (E is quadratic in a
coefficient in the one-electron terms: fd_h - fd_{h/2} is then round-off alone and the floor is the whole bar)."""
import copy

import numpy as np
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

FD_TOL = {"maxiter": 300, "f_tol": 1e-11}  # (the SCF tolerances of tests/test_gpu_autograd_energy.py)
_H = 1e-3
_WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    for k in sorted(_WORST):
        print("WORST %-34s %.3e" % (k, _WORST[k]))


def _dev(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev).contiguous()


def _sym(rng, n):
    a = rng.standard_normal((n, n))
    return (a + a.T) / n


def _richardson(fun, theta):
    """fun(value) -> array of energies; returns (ref, bar without the floor) for d/dtheta at theta"""
    fd = []
    for h in (_H, _H / 2):
        fd.append((np.asarray(fun(theta * (1 + h))) - np.asarray(fun(theta * (1 - h)))) / (2 * h * theta))
    return (4 * fd[1] - fd[0]) / 3, 4 * np.abs(fd[0] - fd[1])


def _check(what, got, ref, bar):
    got, ref, bar = np.asarray(got), np.asarray(ref), np.asarray(bar)
    bar = bar + 1e-10 * np.abs(ref).max()
    ratio = (np.abs(got - ref) / bar).max()
    _WORST[what + " err/bar"] = max(_WORST.get(what + " err/bar", 0.0), ratio)
    _WORST[what + " err/max|ref|"] = max(_WORST.get(what + " err/max|ref|", 0.0), np.abs(got - ref).max() / np.abs(ref).max())
    assert ratio <= 1.0, (what, got, ref, bar)


# ------------------------------------------------------------------------------------------------
# integral kernels against central differences of the oracle's matrices, one perturbed shell per la
# ------------------------------------------------------------------------------------------------
def _shell(a, l):  # contracted tight + diffuse, the pattern of _SPEC in test_gpu_gradient_terms.py
    return (l, [2.9 + 0.3 * a, 0.42 + 0.05 * l], [0.55, 0.6])


def _sub_basis(la):
    """atom 0: another shell of the same l FIRST (a wrong row map would hit it), then the perturbed shell; atoms 1 and 2: partner
    shells of every l = 0 ... 3, so that the random D reaches every (lb, lc, ld) -- with la = 3 the f + 2 = h runtime classes"""
    return [[(la, [1.9, 0.33], [0.4, 0.7]), _shell(0, la)], [_shell(1, 0), _shell(1, 1)], [_shell(2, 2), _shell(2, 3)]]


def _oracle_energies(t, D, W):
    """[E1, Ej, Ek]: sum D (T + V) - sum W S;  1/2 sum (ab|cd) D_ab D_cd;  -1/4 sum (ab|cd) D_ac D_bd"""
    from oracle import natives as nat
    e1 = np.sum(D * (nat.int1e("kin", t) + nat.int1e("nuc", t))) - np.sum(W * nat.int1e("ovlp", t))
    eri = nat.int2e(t)
    ej = 0.5 * np.einsum("abcd,ab,cd->", eri, D, D, optimize=True)
    ek = -0.25 * np.einsum("abcd,ac,bd->", eri, D, D, optimize=True)
    return [e1, ej, ek]


@pytest.mark.parametrize("la", range(4))
def test_integral_kernels_vs_richardson_differences_of_the_oracle(dev, la):
    """both primitives' alpha and c of the second shell of atom 0 (l = la): the exponent / coefficient entry of the table's env is
    perturbed directly (no normalisation involved); (j, k) = (1, 0), (0, 1) and a general pair, which must be their combination"""
    from oracle import basis as ob
    from dqc_amd import lib
    t = ob.make_tables(M.GRAD3, _sub_basis(la))
    tab = lib.Tables(t.atm, t.bas, t.env)
    rng = np.random.default_rng(400 + la)
    D, W = _sym(rng, t.nao), _sym(rng, t.nao)
    T = lib.cart2sph_matrix(tab, "cpu").numpy()
    dc, wc = _dev(T.T @ D @ T, dev), _dev(T.T @ W @ T, dev)
    nprim = int(t.bas[:, 2].sum())
    zero = lambda: torch.zeros((nprim, 2), dtype=torch.float64, device=dev)  # noqa: E731
    g1 = lib.int1e_grad_basis(zero(), dc, wc, tab).cpu().numpy()
    gj = lib.eri_grad_basis(zero(), dc, 0.0, tab, jscale=1.0).cpu().numpy()
    gk = lib.eri_grad_basis(zero(), dc, 1.0, tab, jscale=0.0).cpu().numpy()
    gg = lib.eri_grad_basis(zero(), dc, -1.21, tab, jscale=0.37).cpu().numpy()
    assert np.abs(gg - (0.37 * gj - 1.21 * gk)).max() <= 1e-12 * np.abs(gg).max()
    ish = 1
    row0 = int(t.bas[:ish, 2].sum())
    refs, bars, got = [], [], []
    for k in range(int(t.bas[ish, 2])):
        for col, ptr in ((0, int(t.bas[ish, 5]) + k), (1, int(t.bas[ish, 6]) + k)):
            def fun(v):
                tp = copy.copy(t)
                tp.env = t.env.copy()
                tp.env[ptr] = v
                return _oracle_energies(tp, D, W)
            r, b = _richardson(fun, t.env[ptr])
            refs.append(r)
            bars.append(b)
            got.append([g1[row0 + k, col], gj[row0 + k, col], gk[row0 + k, col]])
    refs, bars, got = np.array(refs), np.array(bars), np.array(got)
    for i, name in enumerate(("int1e", "eri j", "eri k")):
        for cols, par in ((slice(0, None, 2), "alpha"), (slice(1, None, 2), "c")):
            _check("%s d/d%s" % (name, par), got[cols, i], refs[cols, i], bars[cols, i])


def test_basis_kernels_accumulate_and_run_on_a_side_stream(dev):
    """a non-zero d_out is added to, and a call on a non-default torch stream gives the same result"""
    from oracle import basis as ob
    from dqc_amd import lib
    t = ob.make_tables(M.GRAD3, _sub_basis(1))
    tab = lib.Tables(t.atm, t.bas, t.env)
    rng = np.random.default_rng(12)
    T = lib.cart2sph_matrix(tab, "cpu").numpy()
    D, W = _sym(rng, t.nao), _sym(rng, t.nao)
    dc, wc = _dev(T.T @ D @ T, dev), _dev(T.T @ W @ T, dev)
    nprim = int(t.bas[:, 2].sum())
    g0 = rng.standard_normal((nprim, 2))
    z = torch.zeros((nprim, 2), dtype=torch.float64, device=dev)
    r1 = lib.int1e_grad_basis(z.clone(), dc, wc, tab).cpu().numpy()
    r2 = lib.eri_grad_basis(z.clone(), dc, 0.8, tab, jscale=0.6).cpu().numpy()
    assert np.abs(r1).max() > 0 and np.abs(r2).max() > 0
    a1 = lib.int1e_grad_basis(_dev(g0, dev), dc, wc, tab).cpu().numpy()
    a2 = lib.eri_grad_basis(_dev(g0, dev), dc, 0.8, tab, jscale=0.6).cpu().numpy()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b1 = lib.int1e_grad_basis(_dev(g0, dev), dc, wc, tab)
        b2 = lib.eri_grad_basis(_dev(g0, dev), dc, 0.8, tab, jscale=0.6)
    s.synchronize()
    for r, a, b in ((r1, a1, b1.cpu().numpy()), (r2, a2, b2.cpu().numpy())):
        # (fp64 atomics: the order of the sums differs between calls)
        assert np.abs(a - g0 - r).max() <= 1e-12 * np.abs(r).max()
        assert np.abs(b - g0 - r).max() <= 1e-12 * np.abs(r).max()


def test_basis_kernels_refuse_g_shells_and_wrong_shapes(dev):
    from oracle import basis as ob
    from dqc_amd import lib
    t = ob.make_tables(M.GRAD3, M.GRAD3_BAS)
    tab = lib.Tables(t.atm, t.bas, t.env)
    nc = sum((l + 1) * (l + 2) // 2 for l in t.bas[:, 1])
    d = torch.zeros((nc, nc), dtype=torch.float64, device=dev)
    out = torch.zeros((int(t.bas[:, 2].sum()), 2), dtype=torch.float64, device=dev)
    with pytest.raises(NotImplementedError, match="up to f"):
        lib.eri_grad_basis(out, d, 1.0, tab)
    with pytest.raises(NotImplementedError, match="up to f"):
        lib.int1e_grad_basis(out, d, d, tab)
    t2 = ob.make_tables(M.GRAD3, _sub_basis(0))
    tab2 = lib.Tables(t2.atm, t2.bas, t2.env)
    with pytest.raises(lib.DqcAmdError, match="out must be"):
        lib.eri_grad_basis(out, d, 1.0, tab2)


# ------------------------------------------------------------------------------------------------
# molecules with CGTOBasis leaves: raw (l, alphas, coeffs) lists, two-primitive shells, one d shell on the heavy atom
# ------------------------------------------------------------------------------------------------
_HEAVY = [(0, [38.0, 5.6], [0.35, 0.75]), (0, [1.9, 0.45], [-0.3, 1.1]), (1, [3.1, 0.55], [0.4, 0.75]), (2, [0.9], [1.0])]
_LIGHT = [(0, [5.4, 0.82], [0.16, 0.9]), (0, [0.18], [1.0])]
_NH2 = ([7, 1, 1], [[0, 0, 0.1], [0, 1.6, -0.9], [0.2, -1.5, -1.0]])


def _values():
    """the leaf values: [alphas, coeffs] of every heavy-atom shell, then of every hydrogen shell (shared by both hydrogens)"""
    return [torch.tensor(x, dtype=torch.float64) for _, a, c in _HEAVY + _LIGHT for x in (a, c)]


def _bases(vals):
    from dqc_amd.utils.datastruct import CGTOBasis
    ls = [l for l, _, _ in _HEAVY + _LIGHT]
    sh = [CGTOBasis(l, vals[2 * i], vals[2 * i + 1]) for i, l in enumerate(ls)]
    heavy, light = sh[:len(_HEAVY)], sh[len(_HEAVY):]
    return [heavy, light, light]


def _run(case, vals, **kw):
    import dqc_amd
    mol, xc, molkw = {"rhf": (M.H2O, None, {}), "uhf": (_NH2, None, {"spin": 1}), "lda": (M.H2O, "lda_x", {}),
                      "pbe": (M.H2O, "gga_x_pbe+gga_c_pbe", {}), "pbe0": (M.H2O, "pbe0", {}),
                      "upbe": (_NH2, "gga_x_pbe+gga_c_pbe", {"spin": 1}), "ulda": (_NH2, "lda_x", {"spin": 1})}[case]
    m = dqc_amd.Mol(mol, basis=_bases(vals), grid=3, **dict(molkw, **kw))
    qc = (dqc_amd.KS(m, xc=xc) if xc else dqc_amd.HF(m)).run(fwd_options=FD_TOL)
    assert qc.accepted
    return qc


def _leaves():
    return [v.clone().requires_grad_(True) for v in _values()]


# ------------------------------------------------------------------------------------------------
# XC term at fixed AO density
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lda", "pbe", "ulda", "upbe"])
def test_xc_term_vs_richardson_differences_at_fixed_density(dev, case):
    """gradient._xc_basis_gradient against differences of sum_g w e_xc evaluated through lib.eval_gto, lib.grid_density and the
    functional object on perturbed tables, D fixed (positive semi-definite, so that the density is one)"""
    from dqc_amd import gradient as G, lib
    from dqc_amd.utils.datastruct import SpinParam, ValGrad
    h = _run(case, _values())._engine.hamilton
    tab, nao = h._tab, h._nao_ao
    rng = np.random.default_rng(5)
    d_aos = []
    for _ in range(2 if case[0] == "u" else 1):
        a = rng.standard_normal((nao, 3))
        d_aos.append(_dev(a @ a.T / nao, dev))
    got = G._xc_basis_gradient(h, d_aos).cpu().numpy()
    dpads = [lib.pad_matrix(d, h._ld) for d in d_aos]
    gga = h.xcfamily >= 2

    def exc(ptr, v):
        env = tab.env.copy()
        env[ptr] = v
        ao = lib.eval_gto(lib.Tables(tab.atm, tab.bas, env), h.rgrid, 1)
        infos = []
        for dp in dpads:
            rho, grho = lib.grid_density(ao, nao, dp, True)
            infos.append(ValGrad(value=rho, grad=grho if gga else None))
        dens = infos[0] if len(infos) == 1 else SpinParam(u=infos[0], d=infos[1])
        return float((h.dvolume * h.xc.get_edensityxc(dens)).sum())

    ref, bar = np.zeros_like(got), np.zeros_like(got)
    row = 0
    for b in tab.bas:
        for k in range(int(b[2])):
            for col, ptr in ((0, int(b[5]) + k), (1, int(b[6]) + k)):
                ref[row, col], bar[row, col] = _richardson(lambda v: exc(ptr, v), tab.env[ptr])
            row += 1
    _check("xc %s d/dalpha" % case, got[:, 0], ref[:, 0], bar[:, 0])
    _check("xc %s d/dc" % case, got[:, 1], ref[:, 1], bar[:, 1])


# ------------------------------------------------------------------------------------------------
# whole energies through torch.autograd
# ------------------------------------------------------------------------------------------------
def _directions():
    rng = np.random.default_rng(21)
    out = []
    for _ in range(3):
        d = []
        for i, v in enumerate(_values()):
            r = torch.as_tensor(rng.uniform(-1, 1, v.shape))
            d.append(r * v if i % 2 == 0 else r)  # exponents move relative to their size
        out.append(d)
    return out


@pytest.mark.parametrize("case", ["rhf", "uhf", "lda", "pbe", "pbe0"])
def test_energy_autograd_vs_central_differences_of_converged_energies(dev, case):
    """torch.autograd.grad(qc.energy(), leaves) projected on three fixed random directions in (alpha, c) space against
    (E(x + h d) - E(x - h d)) / 2h of converged energies, h = 1e-4, bar 1e-6"""
    leaves = _leaves()
    e = _run(case, leaves).energy()
    assert e.requires_grad
    g = torch.autograd.grad(e, leaves)
    for v, gi in zip(leaves, g):
        assert gi.shape == v.shape and gi.device == v.device
    h = 1e-4
    for n, d in enumerate(_directions()):
        ana = float(sum((gi * di).sum() for gi, di in zip(g, d)))
        ep = float(_run(case, [v + h * di for v, di in zip(_values(), d)]).energy())
        em = float(_run(case, [v - h * di for v, di in zip(_values(), d)]).energy())
        err = abs((ep - em) / (2 * h) - ana)
        _WORST["energy %s direction" % case] = max(_WORST.get("energy %s direction" % case, 0.0), err)
        assert err < 1e-6, (case, n, ana, (ep - em) / (2 * h))


def test_rhf_grad_basis_gradcheck(dev):
    """H2, two-primitive s shells: exponents and coefficients as in the position gradcheck of test_gpu_autograd_energy.py"""
    import dqc_amd
    from dqc_amd.utils.datastruct import CGTOBasis

    def get_energy(a1, c1, a2, c2):
        bases = [CGTOBasis(0, a1, c1), CGTOBasis(0, a2, c2)]
        mol = dqc_amd.Mol(([1, 1], [[-0.7, 0.0, 0.0], [0.7, 0.0, 0.0]]), basis=[bases, bases])
        return dqc_amd.HF(mol, restricted=True).run(fwd_options=FD_TOL).energy()

    p = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in ([5.4, 0.82], [0.16, 0.9], [0.3, 0.12], [0.7, 0.4])]
    assert torch.autograd.gradcheck(get_energy, p, nondet_tol=1e-10)


# ------------------------------------------------------------------------------------------------
# exact identities
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rhf", "pbe"])
def test_scale_invariance_one_primitive_shells_and_shared_tensors(dev, case):
    """per shell sum_p c_p dE/dc_p = 0 for the caller's unnormalised coefficients (rescaling a shell changes nothing), so a
    one-primitive shell has dE/dc = 0; the hydrogens' shared tensors receive the sum of the two per-atom gradients"""
    leaves = _leaves()
    g = torch.autograd.grad(_run(case, leaves).energy(), leaves)
    scale = float(sum((v.detach() * gi).abs().sum() for i, (v, gi) in enumerate(zip(leaves, g)) if i % 2 == 1))
    worst = 0.0
    for i in range(1, len(leaves), 2):
        worst = max(worst, abs(float((leaves[i].detach() * g[i]).sum())))
        if leaves[i].numel() == 1:
            assert abs(float(g[i])) * abs(float(leaves[i].detach())) <= 1e-9 * scale
    _WORST["scale invariance %s" % case] = worst / scale
    assert worst <= 1e-9 * scale
    # separate tensors for the two hydrogens: their gradients add up to the shared tensors' gradient
    import dqc_amd
    from dqc_amd.utils.datastruct import CGTOBasis
    own = _leaves()
    extra = [v.clone().requires_grad_(True) for v in _values()[2 * len(_HEAVY):]]
    ls = [l for l, _, _ in _HEAVY + _LIGHT]
    sh = [CGTOBasis(l, own[2 * i], own[2 * i + 1]) for i, l in enumerate(ls)]
    sh2 = [CGTOBasis(l, extra[2 * i], extra[2 * i + 1]) for i, (l, _, _) in enumerate(_LIGHT)]
    xc = {"rhf": None, "pbe": "gga_x_pbe+gga_c_pbe"}[case]
    m = dqc_amd.Mol(M.H2O, basis=[sh[:len(_HEAVY)], sh[len(_HEAVY):], sh2], grid=3)
    qc = (dqc_amd.KS(m, xc=xc) if xc else dqc_amd.HF(m)).run(fwd_options=FD_TOL)
    g2 = torch.autograd.grad(qc.energy(), own + extra)
    nh = 2 * len(_HEAVY)
    for i in range(len(extra)):
        tot = g2[nh + i] + g2[len(own) + i]
        assert float((tot - g[nh + i]).abs().max()) <= 1e-9 * scale


# ------------------------------------------------------------------------------------------------
# unchanged behaviour and refusals
# ------------------------------------------------------------------------------------------------
def test_energy_and_forces_do_not_change_with_basis_leaves(dev):
    e0 = _run("rhf", _values()).energy()
    assert not e0.requires_grad and e0.grad_fn is None
    pos = torch.tensor(M.H2O[1], dtype=torch.float64, requires_grad=True)
    import dqc_amd

    def forces(vals):
        m = dqc_amd.Mol((M.H2O[0], pos), basis=_bases(vals), grid=3)
        qc = dqc_amd.HF(m).run(fwd_options=FD_TOL)
        return torch.autograd.grad(qc.energy(), pos)[0], qc
    f0, _ = forces(_values())
    f1, qc = forces(_leaves())
    assert float((f0 - f1).abs().max()) <= 1e-12
    assert float((qc.basis_gradient().cpu() - dqc_amd.gradient.basis_gradient(qc).cpu()).abs().max()) <= 1e-12


def test_direct_scf_gives_the_same_basis_gradient(dev, monkeypatch):
    """DQC_AMD_ERI=direct (no tile store): the contraction builds its own integrals, so the derivative is the stored path's"""
    g0 = _run("rhf", _values()).basis_gradient()
    monkeypatch.setenv("DQC_AMD_ERI", "direct")
    qc = _run("rhf", _values())
    assert qc._engine.hamilton._eri_mode == "direct"
    g1 = qc.basis_gradient()
    assert float((g0 - g1).abs().max()) <= 1e-8 * float(g0.abs().max())  # (two SCF runs converged to f_tol = 1e-11)


def test_basis_gradient_refusals(dev):
    import dqc_amd
    from dqc_amd.gradient import basis_gradient
    m = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3).densityfit(auxbasis="etb")
    with pytest.raises(NotImplementedError, match="density-fitted"):
        basis_gradient(dqc_amd.KS(m, xc="lda_x").run(fwd_options=FD_TOL))
    m = dqc_amd.Mol(M.GRAD3, basis=_g_basis())
    with pytest.raises(NotImplementedError, match="up to f"):
        basis_gradient(dqc_amd.HF(m).run(fwd_options={"maxiter": 300}))
    m = dqc_amd.Mol(M.H2O, basis="3-21G", efield=torch.tensor([1e-3, 0.0, 0.0], dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="electric field"):
        basis_gradient(dqc_amd.HF(m).run(fwd_options=FD_TOL))
    m0 = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3)
    m0.setup_grid()
    rg = m0.get_grid().get_rgrid()
    m = dqc_amd.Mol(M.H2O, basis="3-21G", grid=3, vext=1e-3 * rg[:, 0])
    with pytest.raises(NotImplementedError, match="external potential"):
        basis_gradient(dqc_amd.KS(m, xc="lda_x").run(fwd_options=FD_TOL))


def _g_basis():
    from dqc_amd.utils.datastruct import CGTOBasis
    t = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    return [[CGTOBasis(l, t(a), t(c)) for l, a, c in ab] for ab in M.GRAD3_BAS]
