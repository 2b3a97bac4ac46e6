"""RI-MP2 on the GPU: the fused pair kernel dqc_mp2_pair_energies and dqc_amd.mp2 end to end.

Yardsticks:
  * the kernel: `pair_energies_reference` (dqc_amd/mp2.py) on the CPU in fp64 on the same synthetic inputs.  Bar, per occupied pair:
    |e - ref| <= 1e-12 sum_ab |term|, the standing bar of the fp64 contraction kernels (test_streamed_operand_loads_gpu.py); both sides
    are fp64 sums of the same terms in different orders.  For e_ss of a pair i == j every term vanishes analytically (V is symmetric:
    the kernel returns an exact 0, the reference the round-off of v - v^T), so sum |term| is no scale there and these pairs are held
    against the magnitudes of the two products each term is the difference of (`_abs_terms`);
  * fitted end to end: the same reference evaluated here from the Hamiltonian's B tensor and the eigenpairs of the converged Fock matrix,
    1e-10 Ha; UHF against RHF of a closed shell 1e-8 Ha (two separately converged SCF runs: the SCF bar);
  * exact end to end: MP2 from the dense exact ERIs of the tile store, H2O / 3-21G (e_corr -0.1228254166 Ha).  The difference is the
    RI error of the "etb" auxiliary set (naux 101): measured -7.091e-6 Ha in e_corr -- its parts cancel: +6.055e-5 Ha in e_os,
    -6.764e-5 Ha in e_ss -- and asserted at 3 x the measured value rounded up to one digit: 3e-5 Ha on e_corr, 3e-4 Ha on each part,
    both below the reference's own energy tolerance 1.3e-3 Ha.  The error is deterministic; the margin covers a regenerated set.
    The set Mol.densityfit() GENERATES from this small orbital basis (naux 28, made for fitting J) misses that tolerance: -7.8e-3 Ha
    -- printed, not asserted; MP2 wants "etb" or a real fitting set (README)."""
import pytest
import torch

from tests import molecules as M

pytestmark = pytest.mark.gpu

TIGHT = {"f_tol": 1e-11, "maxiter": 300}
H2 = ([1, 1], [[0, 0, 0], [0, 0, 1.4]])
OH = ([8, 1], [[0, 0, 0], [0, 0, 1.8324]])
RI_ERROR_BOUND, RI_PART_BOUND = 3e-5, 3e-4   # module docstring


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _side(no, nv, naux, seed):
    """one side's synthetic tensors on the host: b (no, naux, ldv) with NOISE in the padding columns, energies spread so that |D| runs
    from 0.1 to 50 (occupied -20 ... -0.03, virtual 0.02 ... 5)"""
    g = torch.Generator().manual_seed(seed)
    ldv = (nv + 15) // 16 * 16
    b = torch.randn((no, naux, ldv), dtype=torch.float64, generator=g)
    eo = torch.linspace(-20.0, -0.03, no, dtype=torch.float64) if no > 1 else torch.full((no,), -0.03, dtype=torch.float64)
    ev = torch.linspace(0.02, 5.0, nv, dtype=torch.float64) if nv > 1 else torch.full((nv,), 0.02, dtype=torch.float64)
    return b, eo, ev


def _abs_terms(bi, bj, eoi, eoj, eva, evb, same):
    v = torch.einsum("ipa,jpb->ijab", bi[:, :, :eva.numel()], bj[:, :, :evb.numel()])
    d = eoi[:, None, None, None] + eoj[None, :, None, None] - eva[None, None, :, None] - evb[None, None, None, :]
    a_os = (v * v / d).abs().sum((2, 3))
    if not same:
        return a_os, None
    a_ss = (v * (v - v.transpose(2, 3)) / d).abs().sum((2, 3))
    # i == j: V is symmetric, every same-spin term is zero analytically and what the line above sums there is the round-off of
    # v - v^T itself (1e-15), no scale to measure an error against: for these pairs the magnitudes of the two products each term is
    # the difference of
    idx = torch.arange(v.shape[0])
    a_ss[idx, idx] = (v.abs() * (v.abs() + v.transpose(2, 3).abs()) / d.abs()).sum((2, 3))[idx, idx]
    return a_os, a_ss


def _zero_padding(b, nv):
    z = b.clone()
    z[:, :, nv:] = 0.0
    return z


# nv: one diagonal tile (1, 15, 16), the first off-diagonal tile pair (17, 33), ragged last tiles; 64 / 65 / 130: the panel of four
# tiles full, a second panel of one column, three panels (off-diagonal panel pairs); naux: every residue mod 4, more than one LDS chunk
# of 16 (17, 41); no: i = j only, the first i < j, more pairs
SAME_CASES = [(1, 1, 1), (1, 15, 3), (1, 16, 4), (2, 17, 5), (2, 33, 41), (3, 33, 4), (3, 17, 41), (3, 15, 1), (2, 16, 3), (1, 33, 5),
              (3, 1, 5), (2, 15, 41), (2, 64, 17), (2, 65, 6), (2, 130, 7)]


@pytest.mark.parametrize("no,nv,naux", SAME_CASES)
def test_kernel_same_mode(dev, no, nv, naux):
    from dqc_amd import lib
    from dqc_amd.mp2 import pair_energies_reference
    b, eo, ev = _side(no, nv, naux, 1000 * no + 10 * nv + naux)
    ros, rss = pair_energies_reference(b, b, eo, eo, ev, ev, True)
    aos, ass = _abs_terms(b, b, eo, eo, ev, ev, True)
    bd, eod, evd = b.to(dev), eo.to(dev), ev.to(dev)
    with lib.call_trace() as tr:
        os1, ss1 = lib.mp2_pair_energies(bd, bd, eod, eod, evd, evd, True)
    assert any(r[0] == "dqc_mp2_pair_energies" for r in tr.rows)
    os2, ss2 = lib.mp2_pair_energies(bd, bd, eod, eod, evd, evd, True)
    assert torch.equal(os1, os2) and torch.equal(ss1, ss2)            # launched twice: bit-equal
    bz = _zero_padding(b, nv).to(dev)
    os3, ss3 = lib.mp2_pair_energies(bz, bz, eod, eod, evd, evd, True)
    assert torch.equal(os1, os3) and torch.equal(ss1, ss3)            # the padding columns do not enter, not by a bit
    assert torch.equal(os1, os1.t()) and torch.equal(ss1, ss1.t())    # mirrored
    r_os = float(((os1.cpu() - ros).abs() / aos).max())
    r_ss = float(((ss1.cpu() - rss).abs() / ass.clamp_min(1e-300)).max())
    print("mp2 kernel same (no %d, nv %d, naux %d): worst |e - ref| / sum|terms|  os %.2e  ss %.2e" % (no, nv, naux, r_os, r_ss))
    assert torch.all((os1.cpu() - ros).abs() <= 1e-12 * aos)
    assert torch.all((ss1.cpu() - rss).abs() <= 1e-12 * ass)


@pytest.mark.parametrize("noi,noj,nva,nvb,naux", [(1, 2, 17, 5, 6), (3, 1, 16, 33, 41), (2, 2, 70, 65, 19)])
def test_kernel_opposite_mode(dev, noi, noj, nva, nvb, naux):
    from dqc_amd import lib
    from dqc_amd.mp2 import pair_energies_reference
    bi, eoi, eva = _side(noi, nva, naux, 7 + nva)
    bj, eoj, evb = _side(noj, nvb, naux, 8 + nvb)
    evb = evb * 1.1 + 0.005
    ros, _ = pair_energies_reference(bi, bj, eoi, eoj, eva, evb, False)
    aos, _ = _abs_terms(bi, bj, eoi, eoj, eva, evb, False)
    args = [t.to(dev) for t in (eoi, eoj, eva, evb)]
    os1, ss1 = lib.mp2_pair_energies(bi.to(dev), bj.to(dev), *args, False)
    os2, _ = lib.mp2_pair_energies(bi.to(dev), bj.to(dev), *args, False)
    os3, _ = lib.mp2_pair_energies(_zero_padding(bi, nva).to(dev), _zero_padding(bj, nvb).to(dev), *args, False)
    assert ss1 is None and tuple(os1.shape) == (noi, noj)
    assert torch.equal(os1, os2) and torch.equal(os1, os3)
    ratio = float(((os1.cpu() - ros).abs() / aos).max())
    print("mp2 kernel opposite (%d|%d, %d|%d, naux %d): worst |e - ref| / sum|terms| %.2e" % (noi, noj, nva, nvb, naux, ratio))
    assert torch.all((os1.cpu() - ros).abs() <= 1e-12 * aos)


def test_kernel_empty_sides(dev):
    """zero occupied or zero virtual orbitals on either side: a legal no-op that writes zeros"""
    from dqc_amd import lib
    bi, eoi, eva = _side(2, 5, 6, 1)
    e0 = torch.zeros(0, dtype=torch.float64, device=dev)
    b_noocc = torch.zeros((0, 6, 16), dtype=torch.float64, device=dev)
    os1, _ = lib.mp2_pair_energies(b_noocc, bi.to(dev), e0, eoi.to(dev), eva.to(dev), eva.to(dev), False)
    assert tuple(os1.shape) == (0, 2)
    b_novir = torch.zeros((1, 6, 0), dtype=torch.float64, device=dev)
    eo1 = torch.full((1,), -0.5, dtype=torch.float64, device=dev)
    os2, _ = lib.mp2_pair_energies(bi.to(dev), b_novir, eoi.to(dev), eo1, eva.to(dev), e0, False)
    assert tuple(os2.shape) == (2, 1) and float(os2.abs().max()) == 0.0
    os3, ss3 = lib.mp2_pair_energies(b_novir, b_novir, eo1, eo1, e0, e0, True)
    assert float(os3.abs().max()) == 0.0 and float(ss3.abs().max()) == 0.0
    b_noaux = torch.zeros((2, 0, 16), dtype=torch.float64, device=dev)
    os4, ss4 = lib.mp2_pair_energies(b_noaux, b_noaux, eoi.to(dev), eoi.to(dev), eva.to(dev), eva.to(dev), True)
    assert float(os4.abs().max()) == 0.0 and float(ss4.abs().max()) == 0.0


def test_argument_checks_raise_before_any_launch(dev):
    from dqc_amd import lib
    b, eo, ev = (t.to(dev) for t in _side(2, 5, 6, 2))
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_pair_energies(b[:, :, :5].contiguous(), b, eo, eo, ev, ev, False)        # ldv not a multiple of 16
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_pair_energies(b, b.clone(), eo, eo, ev, ev, True)                        # same mode: two tensors
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_pair_energies(b, b, eo, eo, ev, torch.cat([ev, ev]), True)               # same mode: differing virtual spaces
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_pair_energies(b, b[:, :4].contiguous(), eo, eo, ev, ev, False)           # differing naux
    with pytest.raises(lib.DqcAmdError):
        lib.mp2_pair_energies(b, b, eo[:1], eo, ev, ev, False)                           # energies that do not match the slabs
    L = lib.load()
    null = [None] * 8
    assert L.dqc_mp2_pair_energies(*null, 2, 2, 5, 5, 16, 16, -1, 1, None, None) != 0    # the C entry point refuses a negative naux itself
    assert L.dqc_mp2_pair_energies(*null, 2, 2, 5, 5, 8, 16, 6, 0, None, None) != 0      # ldv no multiple of 16
    assert L.dqc_mp2_pair_energies(*null, 2, 2, 5, 5, 0, 16, 6, 0, None, None) != 0      # ldv < nv
    assert L.dqc_mp2_pair_energies(*null, 2, 3, 5, 5, 16, 16, 6, 1, None, None) != 0     # same mode, differing shapes
    assert L.dqc_mp2_pair_energies(*null, -1, 3, 5, 5, 16, 16, 6, 0, None, None) != 0
    assert L.dqc_mp2_work_doubles(2, 3, 5, 5, 1) == 0 and L.dqc_mp2_work_doubles(3, 3, 70, 70, 1) == 2 * 6 * 3
    assert L.dqc_mp2_work_doubles(3, 2, 70, 5, 0) == 2 * 6 * 2


# ------------------------------------------------------------------------------------------------ 2. end to end
def _reference(qc, b, frozen=0):
    """(e_os, e_ss) of the yardstick, from a B tensor and the eigenpairs of the converged Fock matrix (matrices), on the host"""
    from dqc_amd.mp2 import energies_reference
    eng = qc._engine
    h = eng.hamilton
    focks = (qc._fock[0], qc._fock[1]) if eng.polarized else (qc._fock,)
    nocc = (eng.norb.u, int((eng.orb_weight.d != 0).sum())) if eng.polarized else (eng.norb,)
    spins = []
    for f, n in zip(focks, nocc):
        e, c = eng._eigpairs(f)
        c = h._orthozer @ c
        bov = torch.einsum("pmn,mi,na->ipa", b, c[:, :n], c[:, n:])
        spins.append((bov.cpu(), e[:n].cpu(), e[n:].cpu()))
    e_os, e_ss = energies_reference(spins, frozen)[:2]
    return float(e_os), float(e_ss)


_RUNS = {}


def _run(name):
    """converged calculations, built once and shared"""
    if name not in _RUNS:
        import dqc_amd
        if name == "h2o-rhf-df":
            qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G").densityfit(auxbasis="etb", exchange=True))
        elif name == "h2o-uhf-df":
            qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G").densityfit(auxbasis="etb", exchange=True), restricted=False)
        elif name == "oh-uhf-df":
            qc = dqc_amd.HF(dqc_amd.Mol(OH, basis="3-21G", spin=1).densityfit(auxbasis="etb", exchange=True))
        elif name == "h2o-rhf-exact":
            qc = dqc_amd.HF(dqc_amd.Mol(M.H2O, basis="3-21G"))
        qc.run(fwd_options=TIGHT)
        assert qc.accepted
        _RUNS[name] = qc
    return _RUNS[name]


def test_fitted_rhf_end_to_end(dev):
    import dqc_amd
    from dqc_amd import lib
    qc = _run("h2o-rhf-df")
    h = qc._engine.hamilton
    with lib.call_trace() as tr:
        r = dqc_amd.mp2(qc)
    assert any(row[0] == "dqc_mp2_pair_energies" for row in tr.rows)
    assert r.df is h.df and r.naux == h.df._b.shape[0]
    e_os, e_ss = _reference(qc, h.df._b)
    print("RI-RMP2 H2O / 3-21G: e_os %.10f (ref diff %.1e)  e_ss %.10f (%.1e)  e_corr %.10f" % (
        float(r.e_os), float(r.e_os) - e_os, float(r.e_ss), float(r.e_ss) - e_ss, float(r.e_corr)))
    assert abs(float(r.e_os) - e_os) < 1e-10 and abs(float(r.e_ss) - e_ss) < 1e-10
    assert abs(float(r.e_tot) - (float(qc.energy()) + e_os + e_ss)) < 1e-10
    assert not r.e_tot.requires_grad and tuple(r.pair_os.shape) == (5, 5)
    assert abs(float(r.pair_os.sum()) - float(r.e_os)) < 1e-14 and abs(float(r.pair_ss.sum()) - float(r.e_ss)) < 1e-14
    # scaling: SCS-MP2 from the memoised pair energies (no second kernel call)
    with lib.call_trace() as tr:
        scs = dqc_amd.mp2(qc, c_os=1.2, c_ss=1.0 / 3.0)
    assert not any(row[0] == "dqc_mp2_pair_energies" for row in tr.rows)
    assert abs(float(scs.e_corr) - (1.2 * e_os + e_ss / 3.0)) < 1e-10
    # frozen core
    f1 = dqc_amd.mp2(qc, frozen=1)
    fo, fs = _reference(qc, h.df._b, frozen=1)
    print("   frozen=1: e_corr %.10f (ref diff %.1e)" % (float(f1.e_corr), float(f1.e_corr) - fo - fs))
    assert abs(float(f1.e_os) - fo) < 1e-10 and abs(float(f1.e_ss) - fs) < 1e-10
    assert tuple(f1.pair_os.shape) == (4, 4) and abs(float(f1.e_corr)) < abs(float(r.e_corr))


def test_fitted_uhf_open_shell(dev):
    """the OH radical: all three spin blocks, five alpha and four beta occupied orbitals"""
    import dqc_amd
    qc = _run("oh-uhf-df")
    assert qc._engine.polarized and (qc._engine.norb.u, qc._engine.norb.d) == (5, 4)
    h = qc._engine.hamilton
    r = dqc_amd.mp2(qc)
    e_os, e_ss = _reference(qc, h.df._b)
    print("RI-UMP2 OH / 3-21G: e_os %.10f (ref diff %.1e)  e_ss %.10f (%.1e)" % (float(r.e_os), float(r.e_os) - e_os, float(r.e_ss),
                                                                                 float(r.e_ss) - e_ss))
    assert abs(float(r.e_os) - e_os) < 1e-10 and abs(float(r.e_ss) - e_ss) < 1e-10
    assert tuple(r.pair_os.shape) == (5, 4) and tuple(r.pair_ss[0].shape) == (5, 5) and tuple(r.pair_ss[1].shape) == (4, 4)
    f1 = dqc_amd.mp2(qc, frozen=1)
    fo, fs = _reference(qc, h.df._b, frozen=1)
    assert abs(float(f1.e_os) - fo) < 1e-10 and abs(float(f1.e_ss) - fs) < 1e-10 and tuple(f1.pair_os.shape) == (4, 3)


def test_uhf_of_a_closed_shell_has_the_rhf_components(dev):
    import dqc_amd
    r, u = dqc_amd.mp2(_run("h2o-rhf-df")), dqc_amd.mp2(_run("h2o-uhf-df"))
    print("UMP2 - RMP2 of H2O: e_os %.1e  e_ss %.1e  e_tot %.1e" % (float(u.e_os - r.e_os), float(u.e_ss - r.e_ss), float(u.e_tot - r.e_tot)))
    assert abs(float(u.e_os - r.e_os)) < 1e-8 and abs(float(u.e_ss - r.e_ss)) < 1e-8 and abs(float(u.e_tot - r.e_tot)) < 1e-8


def test_exact_reference_and_the_ri_error(dev):
    """tile-store RHF, mp2(qc, auxbasis="etb") against MP2 from the dense exact (ov|ov): the difference is the RI error"""
    import dqc_amd
    from dqc_amd import lib
    qc = _run("h2o-rhf-exact")
    eng = qc._engine
    h = eng.hamilton
    assert h.df is None
    nao, no = h._nao_ao, eng.norb
    assert nao == 13
    eri = lib.eri_dense(lib.eri_tiles(h._tab, dev), nao)
    e, c = eng._eigpairs(qc._fock)
    c = h._orthozer @ c
    co, cv = c[:, :no], c[:, no:]
    v = torch.einsum("mnls,mi,na,lj,sb->iajb", eri, co, cv, co, cv).cpu()
    eo, ev = e[:no].cpu(), e[no:].cpu()
    d = eo[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] - ev[None, None, None, :]
    exact_os = float((v * v / d).sum())
    exact_ss = float((v * (v - v.transpose(1, 3)) / d).sum())
    r = dqc_amd.mp2(qc, auxbasis="etb")
    err = float(r.e_corr) - (exact_os + exact_ss)
    print("exact MP2 H2O / 3-21G: e_corr %.10f (os %.10f, ss %.10f);  RI (etb, naux %d): e_corr %.10f  RI error %.3e (os %.3e, ss %.3e)"
          % (exact_os + exact_ss, exact_os, exact_ss, r.naux, float(r.e_corr), err, float(r.e_os) - exact_os, float(r.e_ss) - exact_ss))
    g = dqc_amd.mp2(qc)   # auxbasis=None: the generated set
    print("   generated set (naux %d): RI error %.3e" % (g.naux, float(g.e_corr) - (exact_os + exact_ss)))
    assert RI_ERROR_BOUND < 1.3e-3 and RI_PART_BOUND < 1.3e-3
    assert abs(err) < RI_ERROR_BOUND
    assert abs(float(r.e_os) - exact_os) < RI_PART_BOUND and abs(float(r.e_ss) - exact_ss) < RI_PART_BOUND
    assert r.df is dqc_amd.mp2(qc, auxbasis="etb").df   # the tensor is kept for reuse
    assert abs(float(r.e_tot) - (float(qc.energy()) + float(r.e_corr))) < 1e-12


def test_refusals(dev):
    import dqc_amd
    from dqc_amd.utils.datastruct import SpinParam
    rohf = dqc_amd.HF(dqc_amd.Mol(OH, basis="3-21G", spin=1), restricted=True).run()
    with pytest.raises(NotImplementedError, match="restricted open-shell"):
        dqc_amd.mp2(rohf)
    frac = dqc_amd.HF(dqc_amd.Mol(([1.2, 1.25], H2[1]), basis="3-21G", spin=0)).run()
    with pytest.raises(NotImplementedError, match="fractional"):
        dqc_amd.mp2(frac)
    w = SpinParam(u=torch.tensor([1.0], dtype=torch.float64), d=torch.tensor([1.0], dtype=torch.float64))
    user = dqc_amd.HF(dqc_amd.Mol(H2, basis="3-21G", orb_weights=w)).run()
    with pytest.raises(NotImplementedError, match="user-given"):
        dqc_amd.mp2(user)
    with pytest.raises(ValueError):
        dqc_amd.mp2(_run("h2o-rhf-df"), frozen=-1)
    # (shard_over needs several GPUs and a method="overlap" Hamiltonian cannot be built: their checks are exercised in test_mp2_cpu.py)


def test_b2plyp_recipe(dev):
    """the README's recipe: B2PLYP = the hybrid part spelled for get_xc + 0.27 x MP2 on the Kohn-Sham orbitals"""
    import dqc_amd
    qc = dqc_amd.KS(dqc_amd.Mol(H2, basis="3-21G", grid="sg2").densityfit(auxbasis="etb", exchange=True),
                    xc="0.53 * hf + 0.47 * gga_x_b88 + 0.73 * gga_c_lyp").run(fwd_options=TIGHT)
    assert qc.accepted and abs(qc._engine.exx - 0.53) < 1e-15
    e = float(dqc_amd.mp2(qc, c_os=0.27, c_ss=0.27).e_tot)
    e_os, e_ss = _reference(qc, qc._engine.hamilton.df._b)
    print("B2PLYP H2 / 3-21G: E %.10f  (KS part %.10f, 0.27 x MP2 %.10f)" % (e, float(qc.energy()), 0.27 * (e_os + e_ss)))
    assert abs(e - (float(qc.energy()) + 0.27 * (e_os + e_ss))) < 1e-10
    assert e_os < 0.0 and abs(e_ss) < 1e-14   # one occupied orbital: no same-spin correlation
