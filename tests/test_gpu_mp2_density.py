"""RI-MP2 one-particle densities on the GPU: the amplitude kernel dqc_mp2_amplitudes and dqc_amd.mp2_density end to end.

Yardsticks:
  * the kernel: T = V / D and Tt = (c_os + c_ss) T - c_ss T^T in plain torch on the CPU, fp64, on the same synthetic inputs (noise in the
    padding columns, |D| from 0.1 to 50).  Bar per element: |T - ref| <= 1e-12 sum_P |Bov[i,P,a] Bov[j,P,b]| / |D|, twice that for Tt --
    both sides are fp64 sums of the same naux products in different orders, followed by one division (the bound shape of
    tests/test_gpu_mp2.py, per element);
  * unrelaxed end to end: `density_reference` (dqc_amd/mp2.py) evaluated here from the same Bov, 1e-12; block size 1 against one block 1e-13;
  * relaxed end to end -- the test that fixes the factors of the Lagrangian and the Z-vector: the dipole of mp2_density against the
    Richardson-extrapolated central difference of E_tot(F) = mp2(HF(Mol(efield=F))).e_tot at h = 1e-3 and 2e-3 a.u.  The field enters
    the core Hamiltonian as + r . F and the nuclear term is not in the energy, so mu = -dE/dF + sum_A Z_A R_A (first shown for the
    SCF energy against `edipole`).  FD(h) has the truncation error h^2 E''' / 6 and FD(2h) four times that: |FD(h) - FD(2h)| is
    three times the error of FD(h) and far above that of the extrapolated value; bound 10 x |FD(h) - FD(2h)| + the Z-vector tolerance.
    Directions: z and the in-plane axis between y and z (DIRECTIONS below says why not y itself).
    Measured on the MI355X (z component, atomic units): docs/LOG_r20.md section 2."""
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

TIGHT = {"maxiter": 300, "f_tol": 1e-11}   # (the SCF tolerances of tests/test_gpu_basis_gradient.py)
SCS = (1.2, 1.0 / 3.0)
ZTOL = 1e-9
# field directions (the molecule lies in the yz plane, z its symmetry axis): z, and the in-plane axis half way between y and z, along
# which the dipole is mu_z / sqrt(2).  Along y itself the dipole vanishes by symmetry and E(+F) = E(-F): that finite difference is the
# round-off of the SCF energies (1e-11 ... 1e-10 Ha, divided by 2e-3) on both sides of the comparison and on both sides of the bound, a
# coin toss, not a check -- its figures are printed, not asserted
DIRECTIONS = {"z": (0.0, 0.0, 1.0), "yz": (0.0, 0.5 ** 0.5, 0.5 ** 0.5), "y": (0.0, 1.0, 0.0)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _inputs(no, nv, naux, seed, extra=0):
    """synthetic tensors on the host: b (no, naux, ldv) with NOISE in the padding columns (ldv: nv rounded up to 16, plus `extra`),
    energies spread so that |D| runs from 0.1 to 50"""
    g = torch.Generator().manual_seed(seed)
    ldv = (nv + 15) // 16 * 16 + extra
    b = torch.randn((no, naux, ldv), dtype=torch.float64, generator=g)
    eo = torch.linspace(-20.0, -0.03, no, dtype=torch.float64) if no > 1 else torch.full((no,), -0.03, dtype=torch.float64)
    ev = torch.linspace(0.02, 5.0, nv, dtype=torch.float64) if nv > 1 else torch.full((nv,), 0.02, dtype=torch.float64)
    return b, eo, ev


def _reference(b, eo, ev, c_os, c_ss):
    """(T, Tt, bound) on the host, (no, no, nv, nv) each: bound = sum_P |b b| / |D|"""
    nv = ev.numel()
    bb = b[:, :, :nv]
    v = torch.einsum("ipa,jpb->ijab", bb, bb)
    mag = torch.einsum("ipa,jpb->ijab", bb.abs(), bb.abs())
    d = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    t = v / d
    return t, (c_os + c_ss) * t - c_ss * t.transpose(2, 3), mag / d.abs()


# nv: one tile (1, 15, 16), the first off-diagonal tile pair (17, 33), the panel of four tiles full (64), a second panel of one column
# (65), three panels with off-diagonal panel pairs (130); naux: every residue mod 4, more than one LDS chunk of 16 (17, 41); the last two:
# ldv beyond the padded nv (tiles and a whole panel that hold no real virtual are still written, as zeros)
CASES = [(1, 1, 1, 0), (1, 15, 3, 0), (1, 16, 4, 0), (2, 17, 5, 0), (2, 33, 41, 0), (3, 33, 4, 0), (3, 17, 41, 0), (3, 15, 1, 0),
         (2, 16, 3, 0), (1, 33, 5, 0), (3, 1, 5, 0), (2, 15, 41, 0), (2, 64, 17, 0), (2, 65, 5, 0), (3, 130, 3, 0), (2, 17, 4, 16),
         (2, 1, 5, 64)]


@pytest.mark.parametrize("no,nv,naux,extra", CASES)
def test_kernel_against_host_amplitudes(dev, no, nv, naux, extra):
    from dqc_amd import lib
    b, eo, ev = _inputs(no, nv, naux, 1000 * no + 10 * nv + naux, extra)
    ldv = b.shape[2]
    bd, eod, evd = b.to(dev), eo.to(dev), ev.to(dev)
    blocks = sorted({(0, no), (min(1, no - 1), 1), (no - 1, 1)})
    worst = [0.0, 0.0]
    for c_os, c_ss in ((1.0, 1.0), SCS):
        rt, rtt, bound = _reference(b, eo, ev, c_os, c_ss)
        for i0, ni in blocks:
            with lib.call_trace() as tr:
                t, tt = lib.mp2_amplitudes(bd, eod, evd, i0, ni, c_os, c_ss)
            assert any(r[0] == "dqc_mp2_amplitudes" for r in tr.rows)
            assert tuple(t.shape) == (ni, no, ldv, ldv) and tuple(tt.shape) == (ni, no, ldv, ldv)
            t2, tt2 = lib.mp2_amplitudes(bd, eod, evd, i0, ni, c_os, c_ss)
            assert torch.equal(t, t2) and torch.equal(tt, tt2)                                 # launched twice: bit-equal
            for x in (t, tt):                                                                  # the padding: exactly 0.0
                assert float(x[:, :, nv:, :].abs().max() if ldv > nv else 0.0) == 0.0
                assert float(x[:, :, :, nv:].abs().max() if ldv > nv else 0.0) == 0.0
            th, tth, bd_ = t[:, :, :nv, :nv].cpu(), tt[:, :, :nv, :nv].cpu(), bound[i0:i0 + ni]
            et, ett = (th - rt[i0:i0 + ni]).abs(), (tth - rtt[i0:i0 + ni]).abs()
            worst = [max(worst[0], float((et / bd_).max())), max(worst[1], float((ett / bd_).max()))]
            assert torch.all(et <= 1e-12 * bd_) and torch.all(ett <= 2e-12 * bd_)
            if (i0, ni) == (0, no):
                assert torch.equal(t, t.permute(1, 0, 3, 2))                                   # T^{ij}_{ab} and T^{ji}_{ba}: bit-equal
    print("mp2 amplitudes (no %d, nv %d, ldv %d, naux %d): worst |x - ref| / (sum|b b| / |D|)  T %.2e  Tt %.2e" % (
        no, nv, ldv, naux, worst[0], worst[1]))


def test_kernel_output_buffers_and_zero_work(dev):
    from dqc_amd import lib
    b, eo, ev = (x.to(dev) for x in _inputs(3, 17, 5, 3))
    ref_t, ref_tt = lib.mp2_amplitudes(b, eo, ev, 1, 2)
    out = (torch.full((3 * 3 * 32 * 32,), 7.0, dtype=torch.float64, device=dev), torch.full((3 * 3 * 32 * 32,), 7.0, dtype=torch.float64, device=dev))
    t, tt = lib.mp2_amplitudes(b, eo, ev, 1, 2, out=out)                 # a caller's buffer, larger than the block
    assert t.data_ptr() == out[0].data_ptr() and torch.equal(t, ref_t) and torch.equal(tt, ref_tt)
    assert float(out[0][2 * 3 * 32 * 32:].min()) == 7.0                 # nothing is written past the block
    e0 = torch.zeros(0, dtype=torch.float64, device=dev)
    t, tt = lib.mp2_amplitudes(b, eo, ev, 2, 0)                          # an empty block
    assert tuple(t.shape) == (0, 3, 32, 32) and tuple(tt.shape) == (0, 3, 32, 32)
    t, tt = lib.mp2_amplitudes(torch.zeros((0, 5, 16), dtype=torch.float64, device=dev), e0, ev[:3], 0, 0)   # no occupied orbitals
    assert tuple(t.shape) == (0, 0, 16, 16)
    noisy = torch.randn((2, 5, 16), dtype=torch.float64, device=dev)
    t, tt = lib.mp2_amplitudes(noisy, eo[:2], e0, 0, 2)                  # no virtual orbitals: the faces are all padding
    assert tuple(t.shape) == (2, 2, 16, 16) and float(t.abs().max()) == 0.0 and float(tt.abs().max()) == 0.0
    t, tt = lib.mp2_amplitudes(torch.zeros((2, 0, 32), dtype=torch.float64, device=dev), eo[:2], ev, 0, 2)   # no auxiliary functions
    assert tuple(t.shape) == (2, 2, 32, 32) and float(t.abs().max()) == 0.0 and float(tt.abs().max()) == 0.0


def test_argument_checks_raise_before_any_launch(dev):
    from dqc_amd import lib
    b, eo, ev = (x.to(dev) for x in _inputs(2, 5, 6, 2))
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_amplitudes(b[:, :, :5].contiguous(), eo, ev, 0, 2)                       # ldv not a multiple of 16
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_amplitudes(b, eo[:1], ev, 0, 1)                                          # energies that do not match the slabs
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_amplitudes(b, eo, torch.cat([ev, ev, ev, ev]), 0, 2)                     # more virtual energies than columns
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_amplitudes(b, eo, ev, 1, 2)                                              # the block leaves the occupied space
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_amplitudes(b, eo, ev, -1, 1)
    small = torch.empty(2 * 2 * 16 * 16 - 1, dtype=torch.float64, device=dev)
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_amplitudes(b, eo, ev, 0, 2, out=(small, small.clone()))                  # buffers too small
    L = lib.load()
    tail = (1.0, 1.0, None)
    null = [None, None, 1 << 40, None, None, None]
    assert L.dqc_mp2_amplitudes(*null, 2, 5, 16, -1, 0, 2, *tail) != 0                   # the C entry point refuses these itself
    assert L.dqc_mp2_amplitudes(*null, -2, 5, 16, 6, 0, 2, *tail) != 0
    assert L.dqc_mp2_amplitudes(*null, 2, 5, 16, 6, 0, -1, *tail) != 0
    assert L.dqc_mp2_amplitudes(*null, 2, 5, 8, 6, 0, 2, *tail) != 0                     # ldv no multiple of 16
    assert L.dqc_mp2_amplitudes(*null, 2, 17, 16, 6, 0, 2, *tail) != 0                   # ldv < nv
    assert L.dqc_mp2_amplitudes(*null, 2, 5, 16, 6, 1, 2, *tail) != 0                    # i0 + ni > nocc
    assert L.dqc_mp2_amplitudes(None, None, 2 * 2 * 256 - 1, None, None, None, 2, 5, 16, 6, 0, 2, *tail) != 0   # buffers too small
    assert L.dqc_mp2_amplitudes(*null, 2, 5, 16, 6, 0, 2, *tail) != 0                    # null pointers with work to do
    assert L.dqc_mp2_amplitudes(*null, 2, 5, 16, 6, 1, 0, *tail) == 0                    # zero work: nothing is touched
    assert L.dqc_mp2_amplitudes(*null, 0, 5, 16, 6, 0, 0, *tail) == 0


# ------------------------------------------------------------------------------------------------ 2. end to end
_RUNS = {}


def _run(name):
    """converged calculations, built once and shared"""
    if name not in _RUNS:
        import dqc_amd
        if name == "exact":
            qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G"))
        elif name == "pbe0":
            qc = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid="sg2"), xc="pbe0")
        elif name == "df":
            qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G").densityfit(auxbasis="etb", exchange=True))
        else:  # ("field", direction, multiple of h)
            f = [name[2] * 1e-3 * x for x in DIRECTIONS[name[1]]]
            qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G", efield=torch.tensor(f, dtype=torch.float64)))
        qc.run(fwd_options=TIGHT)
        assert qc.accepted
        _RUNS[name] = qc
    return _RUNS[name]


def _host_reference(qc, frozen, c_os, c_ss):
    """`density_reference` on the host from the Bov the library forms for this calculation"""
    from dqc_amd.mp2 import _b_tensor, _orbitals, density_reference, transform_ov
    co, cv, eo, ev = _orbitals(qc, frozen)[0]
    bov = transform_ov(_b_tensor(qc, "etb")._b, co, cv)
    return density_reference(bov.cpu(), eo.cpu(), ev.cpu(), c_os, c_ss) + (bov,)


def test_unrelaxed_end_to_end(dev):
    import dqc_amd
    from dqc_amd import lib
    qc = _run("exact")
    h = qc._engine.hamilton
    with lib.call_trace() as tr:
        r = dqc_amd.mp2_density(qc, auxbasis="etb", relaxed=False)
    assert any(row[0] == "dqc_mp2_amplitudes" for row in tr.rows)
    assert dqc_amd.mp2_density(qc, auxbasis="etb", relaxed=False) is r and not r.relaxed and r.z_residual is None
    assert not r.dm_ao.requires_grad and r.block == 5
    p_oo, p_vv, gamma, bov = _host_reference(qc, 0, 1.0, 1.0)
    no, n = 5, 13
    d_oo, d_vv = float((r.dm_mo[:no, :no].cpu() - p_oo).abs().max()), float((r.dm_mo[no:, no:].cpu() - p_vv).abs().max())
    e_ref = float(dqc_amd.mp2(qc, auxbasis="etb").e_corr)
    print("unrelaxed H2O / 3-21G: |P_oo - ref| %.1e  |P_vv - ref| %.1e  e_corr %.12f (mp2: diff %.1e)  occupations %s" % (
        d_oo, d_vv, float(r.e_corr), float(r.e_corr) - e_ref, " ".join("%.5f" % x for x in r.natural_occupations.tolist())))
    assert tuple(r.dm_mo.shape) == (n, n) and d_oo <= 1e-12 and d_vv <= 1e-12
    assert float(r.dm_mo[:no, no:].abs().max()) == 0.0 and float(r.dm_mo[no:, :no].abs().max()) == 0.0
    assert abs(float(r.e_corr) - e_ref) <= 1e-12
    occ = r.natural_occupations
    assert abs(float(occ.sum()) - 10.0) <= 1e-10 and bool(torch.all(occ[:-1] >= occ[1:]))
    assert float(occ.min()) > -1e-3 and float(occ.max()) < 2.0 + 1e-3
    c = r.natural_orbitals
    assert float((c.t() @ h._ovlp_ao @ c - torch.eye(n, dtype=c.dtype, device=c.device)).abs().max()) <= 1e-10
    assert float((c @ torch.diag(occ) @ c.t() - r.dm_ao).abs().max()) <= 1e-8       # the natural orbitals carry dm_ao (the SCF bar)
    # one occupied orbital per block: the same matrices
    r1 = dqc_amd.mp2_density(qc, auxbasis="etb", relaxed=False, block=1)
    assert r1.block == 1 and r1 is not r
    assert float((r1.dm_mo - r.dm_mo).abs().max()) <= 1e-13 and abs(float(r1.e_corr - r.e_corr)) <= 1e-13
    # frozen core: the frozen row and column are zero, the rest is the reference of the four active orbitals
    f = dqc_amd.mp2_density(qc, frozen=1, auxbasis="etb", relaxed=False)
    fo, fv, _, _ = _host_reference(qc, 1, 1.0, 1.0)
    assert float(f.dm_mo[0].abs().max()) == 0.0 and float(f.dm_mo[:, 0].abs().max()) == 0.0
    assert float((f.dm_mo[1:no, 1:no].cpu() - fo).abs().max()) <= 1e-12 and float((f.dm_mo[no:, no:].cpu() - fv).abs().max()) <= 1e-12
    assert abs(float(f.natural_occupations.sum()) - 10.0) <= 1e-10 and abs(float(f.natural_occupations[0]) - 2.0) <= 1e-12
    # scaled components
    s = dqc_amd.mp2_density(qc, auxbasis="etb", relaxed=False, c_os=SCS[0], c_ss=SCS[1])
    so, sv, _, _ = _host_reference(qc, 0, *SCS)
    assert float((s.dm_mo[:no, :no].cpu() - so).abs().max()) <= 1e-12 and float((s.dm_mo[no:, no:].cpu() - sv).abs().max()) <= 1e-12
    assert abs(float(s.e_corr) - float(dqc_amd.mp2(qc, auxbasis="etb", c_os=SCS[0], c_ss=SCS[1]).e_corr)) <= 1e-12


def test_unrelaxed_on_a_kohn_sham_reference(dev):
    import dqc_amd
    qc = _run("pbe0")
    r = dqc_amd.mp2_density(qc, auxbasis="etb", relaxed=False)
    assert abs(float(r.e_corr) - float(dqc_amd.mp2(qc, auxbasis="etb").e_corr)) <= 1e-12
    assert abs(float(r.natural_occupations.sum()) - 10.0) <= 1e-10 and tuple(r.dipole().shape) == (3,)


def _fd_dipole(direction, energy):
    """(FD(h), FD(2h), Richardson) of mu . e = -dE/dF + sum Z R . e for the field F e, e = DIRECTIONS[direction]; atomic units, h = 1e-3"""
    zs, pos = M.H2O
    ion = sum(z * sum(x * y for x, y in zip(p, DIRECTIONS[direction])) for z, p in zip(zs, pos))
    e = {m: energy(_run(("field", direction, m))) for m in (1, -1, 2, -2)}
    f1, f2 = -(e[1] - e[-1]) / 2e-3 + ion, -(e[2] - e[-2]) / 4e-3 + ion
    return f1, f2, (4.0 * f1 - f2) / 3.0


def test_relaxed_dipole_against_finite_field(dev):
    import dqc_amd
    qc = _run("exact")
    scf = dqc_amd.edipole(qc, unit=None).cpu()
    r = dqc_amd.mp2_density(qc, auxbasis="etb", tol=ZTOL)
    u = dqc_amd.mp2_density(qc, auxbasis="etb", relaxed=False)
    assert r.relaxed and r.z_residual <= ZTOL
    mu, mu_u = r.dipole(unit=None).cpu(), u.dipole(unit=None).cpu()
    assert torch.allclose(r.dipole(), mu.to(r.dm_ao.device) * 2.541746473, rtol=1e-12, atol=0)   # Debye by default, as edipole
    along = lambda v, d: float(sum(x * y for x, y in zip(v.tolist(), DIRECTIONS[d])))  # noqa: E731
    for d in ("z", "yz", "y"):
        s1, s2, sr = _fd_dipole(d, lambda q: float(q.energy()))
        sbound = 10.0 * abs(s1 - s2) + 1e-9
        print("%-2s  SCF: edipole %.10f  FD(h) %.10f  FD(2h) %.10f  Richardson %.10f  |diff| %.2e  bound %.2e" % (
            d, along(scf, d), s1, s2, sr, abs(sr - along(scf, d)), sbound))
        f1, f2, fr = _fd_dipole(d, lambda q: float(dqc_amd.mp2(q, auxbasis="etb").e_tot))
        bound = 10.0 * abs(f1 - f2) + ZTOL
        print("%-2s  MP2: relaxed %.10f  unrelaxed %.10f  FD(h) %.10f  FD(2h) %.10f  Richardson %.10f  |relaxed - FD| %.2e  bound %.2e"
              % (d, along(mu, d), along(mu_u, d), f1, f2, fr, abs(fr - along(mu, d)), bound))
        if d == "y":   # (zero by symmetry: round-off against round-off, see DIRECTIONS)
            assert abs(along(mu, d)) <= 1e-9 and abs(along(scf, d)) <= 1e-9
            continue
        assert abs(sr - along(scf, d)) <= sbound                        # the sign and the unit of the finite difference
        assert abs(fr - along(mu, d)) <= bound
        assert abs(along(mu_u, d) - along(mu, d)) > bound               # the Z-vector is not silently skipped
    # the scaled components, z
    rs = dqc_amd.mp2_density(qc, auxbasis="etb", c_os=SCS[0], c_ss=SCS[1], tol=ZTOL)
    f1, f2, fr = _fd_dipole("z", lambda q: float(dqc_amd.mp2(q, auxbasis="etb", c_os=SCS[0], c_ss=SCS[1]).e_tot))
    bound = 10.0 * abs(f1 - f2) + ZTOL
    ms = float(rs.dipole(unit=None)[2])
    print("z   SCS-MP2: relaxed %.10f  FD(h) %.10f  FD(2h) %.10f  Richardson %.10f  |relaxed - FD| %.2e  bound %.2e" % (
        ms, f1, f2, fr, abs(fr - ms), bound))
    assert abs(fr - ms) <= bound
    occ = r.natural_occupations
    assert abs(float(occ.sum()) - 10.0) <= 1e-10 and float((r.dm_mo - r.dm_mo.t()).abs().max()) <= 1e-14


def test_relaxed_refusals(dev, monkeypatch):
    import dqc_amd
    with pytest.raises(NotImplementedError, match="auxbasis="):
        dqc_amd.mp2_density(_run("df"))
    assert dqc_amd.mp2_density(_run("df"), relaxed=False).naux == _run("df")._engine.hamilton.df._b.shape[0]
    monkeypatch.setenv("DQC_AMD_ERI", "direct")
    qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G")).run()
    monkeypatch.delenv("DQC_AMD_ERI")
    assert qc._engine.hamilton._direct
    with pytest.raises(NotImplementedError, match="auxbasis="):
        dqc_amd.mp2_density(qc, auxbasis="etb")
    with pytest.raises(NotImplementedError, match="frozen"):
        dqc_amd.mp2_density(_run("exact"), frozen=1, auxbasis="etb")
    with pytest.raises(NotImplementedError, match="Kohn-Sham"):
        dqc_amd.mp2_density(_run("pbe0"), auxbasis="etb")
