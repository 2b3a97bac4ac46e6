"""CPU tests (no GPU) of the RI-MP2 nuclear gradient: the gates dqc_df_grad3 takes before its first HIP call, and
mp2.three_index_densities -- the densities Z[mu, nu, Q], G[P, Q] that meet d(mu nu|Q) and -1/2 d(P|Q) in the change of e_corr at
fixed orbitals -- against finite differences of e_corr(R) built from the oracle's integrals."""
import ctypes

import numpy as np
import torch

from oracle import basis as ob, natives as nat
from tests import molecules as M

# H2O, distorted (no symmetry left): the geometry of the gradient tests
ZS = [8, 1, 1]
POS = [[0.0, 0.0, 0.2217], [0.0, 1.4309, -0.8867], [0.1, -1.4309, -0.8867]]
# a small hand-written s, p auxiliary set on each atom
AUX = [[(0, [2.0], [1.0]), (0, [0.5], [1.0]), (1, [1.1], [1.0]), (1, [0.35], [1.0])],
       [(0, [1.2], [1.0]), (0, [0.3], [1.0]), (1, [0.7], [1.0])],
       [(0, [1.2], [1.0]), (0, [0.3], [1.0]), (1, [0.7], [1.0])]]


def test_df_grad3_host_gates_without_a_gpu():
    """the gates of dqc_df_grad3 before its first HIP call (raw ctypes, null device pointers and stream, H2O / STO-3G read as a
    concatenated table): shell ranges outside the table and a Z one double short are refused with their messages; empty ranges and
    two null operands return 0 with nothing touched"""
    from dqc_amd import build, lib
    build.build()
    so = ctypes.CDLL(lib.libpath())
    so.dqc_last_error.restype = ctypes.c_char_p
    t = ob.make_tables(M.H2O, "sto-3g")
    atm = np.ascontiguousarray(t.atm, dtype=np.int32)
    bas = np.ascontiguousarray(t.bas, dtype=np.int32)
    env = np.ascontiguousarray(t.env, dtype=np.float64)
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    I, V, Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    so.dqc_df_grad3.argtypes = [V, V, Z, V, ip, I, ip, I, dp, I, I, I, I, I, V]
    so.dqc_eri_grad.argtypes = [V, V, ctypes.c_double, ctypes.c_double, ip, I, ip, I, dp, I, V]
    tab = (atm.ctypes.data_as(ip), atm.shape[0], bas.ctypes.data_as(ip), bas.shape[0], env.ctypes.data_as(dp), env.shape[0])

    def g3(sh0, sh1, k0, k1, z_doubles=0):
        return so.dqc_df_grad3(None, None, z_doubles, None, *tab, sh0, sh1, k0, k1, None)

    err = lambda: so.dqc_last_error().decode()  # noqa: E731
    nbas = bas.shape[0]
    ncart = lambda a, b: sum((int(l) + 1) * (int(l) + 2) // 2 for l in bas[a:b, 1])  # noqa: E731
    for bad in ((0, nbas + 1, 0, nbas), (3, 2, 0, nbas), (-1, 2, 0, nbas), (0, 2, 2, nbas + 1), (0, 2, 4, 3), (0, 2, -1, 3)):
        assert g3(*bad) == -1 and err() == "dqc_df_grad3: shell ranges outside the table", bad
        assert so.dqc_eri_grad(None, None, 1.0, 1.0, *tab[:3], 0, *tab[4:], None) == 0  # (a success in between: the next message is new)
    # orbital shells [0, 3), auxiliary shells [3, nbas): Z has ncart(0, 3)^2 ncart(3, nbas) doubles
    need = ncart(0, 3) ** 2 * ncart(3, nbas)
    assert need > 1
    assert g3(0, 3, 3, nbas, need - 1) == -1
    assert err() == "dqc_df_grad3: Z is smaller than the (orbital, orbital, auxiliary) Cartesian block of the shell ranges"
    assert g3(0, 3, 3, nbas, 1) == -1
    assert g3(0, 3, 3, nbas, need) == 0      # large enough, both operands null: nothing to do
    assert g3(0, 3, 3, nbas) == 0            # both operands null
    assert g3(2, 2, 3, nbas, 0) == 0         # empty orbital range
    assert g3(0, 3, nbas, nbas, 0) == 0      # empty auxiliary range
    assert g3(2, 2, 3, nbas, 1) == 0         # (an empty range needs no Z)


def _bov(pos, co, cv):
    """(Bov (no, naux, nv), tables, ranges, Cholesky factor) of H2O / sto-3g with AUX at the positions `pos`, oracle integrals"""
    tc, orb, aux = ob.make_tables_df((ZS, pos), "sto-3g", AUX)
    j3 = nat.int3c2e(tc, orb, aux)                     # (nao, nao, naux)
    chol = np.linalg.cholesky(nat.int2c2e(tc, aux))
    b = np.linalg.solve(chol, j3.reshape(-1, j3.shape[2]).T).reshape(-1, j3.shape[0], j3.shape[1])   # C^-1 (Q|mu nu)
    return np.einsum("mi,pmn,na->ipa", co, b, cv), tc, orb, aux, chol


def test_three_index_densities_against_finite_differences():
    """e_corr(R) = sum Gamma Bov of mp2.density_reference on Bov(R) = C_o^T [C^-1 (Q|mu nu)](R) C_v with FIXED C_o (2 columns), C_v (3)
    and orbital energies: its derivative is sum Z d(mu nu|Q) - 1/2 sum G d(P|Q) with the (Z, G) of three_index_densities, the derivative
    integrals from the oracle (natives.df_ip).  Components (O, z), (H, y), (H, x); Richardson-extrapolated central differences at
    h = 1e-3 and 2e-3 Bohr; bound 10 |FD(h) - FD(2h)| + 1e-10 (energies good to 1e-13 Ha over h), every compared component more than
    100 bounds large.  MP2 and SCS-MP2 scalings."""
    from dqc_amd import mp2   # (the function, which carries the yardsticks as attributes)
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.standard_normal((7, 5)))
    co, cv = q[:, :2].copy(), q[:, 2:].copy()
    eo, ev = np.array([-1.3, -0.25]), np.array([0.25, 0.9, 1.7])    # gaps eps_a - eps_i from 0.5 to 3
    gaps = ev[:, None] - eo[None, :]
    assert abs(gaps.min() - 0.5) < 1e-15 and abs(gaps.max() - 3.0) < 1e-15
    tt = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64)  # noqa: E731
    for c_os, c_ss in ((1.0, 1.0), (1.2, 1.0 / 3.0)):
        def e_corr(pos):
            bov = tt(_bov(pos, co, cv)[0])
            _, _, gamma = mp2.density_reference(bov, tt(eo), tt(ev), c_os, c_ss)
            return float((gamma * bov).sum())

        bov, tc, orb, aux, chol = _bov(POS, co, cv)
        _, _, gamma = mp2.density_reference(tt(bov), tt(eo), tt(ev), c_os, c_ss)
        z, g = mp2.three_index_densities(gamma, tt(bov), tt(chol), tt(co), tt(cv))
        z, g = z.numpy(), g.numpy()
        assert z.shape == (7, 7, bov.shape[1]) and g.shape == (bov.shape[1],) * 2
        assert np.abs(z - z.transpose(1, 0, 2)).max() == 0.0 and np.abs(g - g.T).max() == 0.0
        # the contraction dqc_df_grad3 performs, from the oracle's derivative integrals (spherical), rows = atoms of the table
        at = nat.ao_atom(tc)
        n = z.shape[0]
        grad = np.zeros((tc.natm, 3))
        np.add.at(grad, at[:n], 2.0 * np.einsum("dijk,ijk->id", nat.df_ip("ij|k", tc, orb, aux), z))
        np.add.at(grad, at[n:], np.einsum("dijk,ijk->kd", nat.df_ip("k", tc, orb, aux), z))
        np.add.at(grad, at[n:], -np.einsum("dkl,kl->kd", nat.df_ip("2c", tc, orb, aux), g))
        grad = grad[:3] + grad[3:]               # the table lists every atom twice
        assert np.abs(grad.sum(0)).max() < 1e-12
        for atom, d in ((0, 2), (1, 1), (2, 0)):
            fd = []
            for h in (1e-3, 2e-3):
                pp, pm = np.array(POS), np.array(POS)
                pp[atom, d] += h
                pm[atom, d] -= h
                fd.append((e_corr(pp.tolist()) - e_corr(pm.tolist())) / (2 * h))
            rich = (4.0 * fd[0] - fd[1]) / 3.0
            bound = 10.0 * abs(fd[0] - fd[1]) + 1e-10
            print("three_index_densities c_os %.2f c_ss %.2f atom %d dir %d: analytic % .10e richardson % .10e |diff| %.2e bound %.2e"
                  % (c_os, c_ss, atom, d, grad[atom, d], rich, abs(grad[atom, d] - rich), bound))
            assert abs(grad[atom, d]) > 100.0 * bound, (atom, d, grad[atom, d], bound)
            assert abs(grad[atom, d] - rich) <= bound, (atom, d, grad[atom, d], rich, bound)


def test_energy_weighted_with_orbital_coupling_is_the_inline_expression():
    """postscf.energy_weighted(p, eps, mp2.orbital_coupling(...), g_pbar, co, cv) equals the expression mp2._gradient used to hold
    inline -- written out below as the yardstick -- on random operands: no = 2, nv = 3, nao = 7, naux = 5, Bov and Gamma with one padded
    virtual column (filled with numbers, so that a missed [:nv, :nv] slice shows).  Bound 1e-13 max |W2|: the two differ in the order of
    at most four fp64 additions per element and in GEMMs of inner dimension <= 7.  W2 is exactly symmetric."""
    from dqc_amd import excited, mp2
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g)  # noqa: E731
    no, nv, nao, naux = 2, 3, 7, 5
    n = no + nv
    q, _ = torch.linalg.qr(rnd(nao, n))
    co, cv = q[:, :no].contiguous(), q[:, no:].contiguous()
    p = rnd(n, n)
    p = 0.5 * (p + p.t())
    eps, g_pbar = rnd(n), rnd(nao, nao)
    bov, gamma = rnd(no, naux, nv + 1), rnd(no, naux, nv + 1)
    x, y = rnd(nv, no), rnd(nv, no)
    got = excited.energy_weighted(p, eps, mp2.orbital_coupling(bov, gamma, x, y, nv), g_pbar, co, cv)
    # the yardstick: the inline expression of the parent
    c_all = torch.cat([co, cv], dim=1)
    gm = 2.0 * eps.unsqueeze(1) * p
    gm[:, :no] += 4.0 * (c_all.t() @ g_pbar @ co)
    gm[:no, :no] += 4.0 * torch.einsum("kpa,ipa->ki", bov, gamma)
    gm[no:, :no] += 4.0 * x
    gm[:no, no:] += 4.0 * y.t()
    gm[no:, no:] += 4.0 * torch.einsum("ipc,ipa->ca", bov, gamma)[:nv, :nv]
    ref = c_all @ (0.25 * (gm + gm.t())) @ c_all.t()
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print("energy_weighted / orbital_coupling vs inline: max |diff| %.2e, max |W2| %.3e" % (err, scale))
    assert got.shape == (nao, nao) and scale > 1.0
    assert err <= 1e-13 * scale
    assert torch.equal(got, got.t())


def test_dipole_of_an_ao_density(monkeypatch):
    """properties.dipole_au(h, mol, D) = -einsum("dab,ba->d", r, D) + einsum("ad,a->d", pos, Z), exactly: random symmetric D, a random
    (3, n, n) r in place of the multipole integrals, three atoms"""
    from types import SimpleNamespace
    from dqc_amd import lib, properties
    g = torch.Generator().manual_seed(9)
    n = 6
    d = torch.randn(n, n, dtype=torch.float64, generator=g)
    d = 0.5 * (d + d.t())
    r = torch.randn(3, n, n, dtype=torch.float64, generator=g)
    pos = torch.randn(3, 3, dtype=torch.float64, generator=g)
    zs = torch.tensor([8, 1, 1])
    h = SimpleNamespace(_tab=object(), device=torch.device("cpu"))
    asked = []
    monkeypatch.setattr(lib, "int1e", lambda which, tab, device: (asked.append((which, tab is h._tab)), r)[1])
    got = properties.dipole_au(h, SimpleNamespace(atompos=pos, atomzs=zs), d)
    ref = -torch.einsum("dab,ba->d", r, d) + torch.einsum("ad,a->d", pos, zs.to(torch.float64))
    assert asked == [("r0", True)]
    assert got.shape == (3,) and torch.equal(got, ref)
