"""RI-dRPA on the GPU: the fused response kernel dqc_rpa_response and dqc_amd.rpa end to end.

Yardsticks:
  * the kernel: `response_reference` (dqc_amd/rpa.py) on the CPU in fp64 on the same synthetic inputs (noise in the padding columns,
    gaps from 0.05 to 25).  Bar, per element of Q: |Q - ref| <= 1e-12 sum |terms|, the standing bar of the fp64 contraction kernels;
    both sides are fp64 sums of the same terms in different orders.  Two launches, and noisy against zeroed padding, are bit-equal;
    every Q[k] is bit-symmetric;
  * fitted end to end: the same quadrature evaluated on the CPU from the Hamiltonian's B tensor and the eigenpairs of the converged Fock
    matrix, 1e-10 Ha; the closed form (`plasmon_reference`, ov = 5 x 8) below 1e-8 Ha, and within 10 x the result's own
    `quadrature_error` estimate at coarse grids and at the default grid -- there the estimate is about 1e-15 Ha and the closed form is
    taken in 40-digit arithmetic, its fp64 evaluation being good to 1e-14 Ha only; UHF against RHF of a closed shell 1e-8 Ha (two separately
    converged SCF runs: the SCF bar);
  * exact end to end: the closed form on the dense exact (ia|jb) of the tile store, H2O / 3-21G.  The difference is the RI error of the
    "etb" auxiliary set (naux 101): measured +1.005e-4 Ha in e_corr (exact -0.1383541656 Ha), asserted at 3 x the measured value
    rounded up to one digit: 4e-4 Ha, below the reference's own energy tolerance 1.3e-3 Ha.  The error is deterministic; the margin covers a regenerated set."""
import pytest
import torch

from tests import molecules as M
from tests.test_gpu_mp2 import OH, TIGHT, _run, _side, _zero_padding

pytestmark = pytest.mark.gpu

RI_MEASURED, RI_ERROR_BOUND = 1.005e-4, 4e-4   # module docstring


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _freqs(nfreq, zero_first=False):
    f = torch.logspace(-1.5, 2.0, nfreq, dtype=torch.float64) if nfreq > 1 else torch.full((nfreq,), 0.7, dtype=torch.float64)
    if zero_first:
        f[0] = 0.0
    return f


def _reference(b, eo, ev, f, scale):
    """(Q, sum |terms|) on the host: every g is positive, so the magnitudes are the response of |B|"""
    from dqc_amd.rpa import response_reference
    return response_reference(b, eo, ev, f, scale), response_reference(b.abs(), eo, ev, f, abs(scale))


# (no, nv, naux, nfreq, w_0 = 0).  nv: one chunk of 16 (1, 15, 16), a second with one real column (17), three and five chunks (33,
# 65); naux: one tile (1, 15, 16), a second tile of one row (17), a full panel and its edges (63, 64), a second panel of one row (65:
# the first off-diagonal panel pair), three panels (130); nfreq: one group (1, 3, 4), a ragged second (5), a ragged third (9).
# The (i, a) sum is split over slots of the work buffer wherever there are at least two chunks and few blocks: every case below
# with no > 1 or nv > 16, except the last -- 6 panel pairs x 172 frequency groups are more blocks than the split aims for, so its
# six chunks run in one block each, the form a real molecule takes; "one-chunk" cases (no 1, nv <= 16) take the direct form too.
CASES = {
    "minimal": (1, 1, 1, 1, False),
    "one-chunk-tile-edge": (1, 15, 15, 3, False),
    "one-chunk-three-panels": (1, 16, 130, 4, False),
    "one-chunk-ragged-group": (1, 15, 65, 5, False),
    "full-tile": (2, 16, 16, 4, False),
    "second-tile-second-chunk": (2, 17, 17, 5, False),
    "panel-edge-63": (3, 33, 63, 9, False),
    "full-panel": (1, 65, 64, 4, False),
    "second-panel": (2, 33, 65, 3, False),
    "three-panels": (3, 17, 130, 5, False),
    "three-panels-one-frequency": (2, 15, 130, 1, False),
    "five-chunks": (3, 65, 17, 9, False),
    "one-auxiliary-function": (2, 16, 1, 4, False),
    "zero-frequency": (2, 17, 33, 4, True),
    "no-split-many-blocks": (2, 33, 130, 685, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_reference(dev, name):
    from dqc_amd import lib
    no, nv, naux, nfreq, zero_first = CASES[name]
    b, eo, ev = _side(no, nv, naux, 7000 + 100 * no + 10 * nv + naux)
    f = _freqs(nfreq, zero_first)
    ref, mag = _reference(b, eo, ev, f, 4.0)
    slots = int(lib.load().dqc_rpa_work_doubles(no, nv, naux, nfreq)) // (nfreq * naux * naux)
    if name.startswith("one-chunk") or name in ("minimal", "no-split-many-blocks"):
        assert slots == 0, "this case is meant to take the direct form"
    else:
        assert slots >= 2, "this case is meant to split the (i, a) sum over at least two slots"
    bd, eod, evd, fd = b.to(dev), eo.to(dev), ev.to(dev), f.to(dev)
    with lib.call_trace() as tr:
        q1 = lib.rpa_response(bd, eod, evd, fd, 4.0)
    assert any(r[0] == "dqc_rpa_response" for r in tr.rows)
    assert tuple(q1.shape) == (nfreq, naux, naux)
    q2 = lib.rpa_response(bd, eod, evd, fd, 4.0)
    assert torch.equal(q1, q2)                                          # launched twice: bit-equal
    q3 = lib.rpa_response(_zero_padding(b, nv).to(dev), eod, evd, fd, 4.0)
    assert torch.equal(q1, q3)                                          # the padding columns do not enter, not by a bit
    assert torch.equal(q1, q1.transpose(1, 2))                          # mirrored from the same registers
    ratio = float(((q1.cpu() - ref).abs() / mag).max())
    print("rpa kernel %s (no %d, nv %d, naux %d, nfreq %d, slots %d): worst |Q - ref| / sum|terms| %.2e" % (name, no, nv, naux, nfreq, slots, ratio))
    assert torch.all((q1.cpu() - ref).abs() <= 1e-12 * mag)


@pytest.mark.parametrize("name", ["one-chunk-three-panels", "second-panel", "five-chunks"])
def test_kernel_accumulates_a_second_spin(dev, name):
    from dqc_amd import lib
    no, nv, naux, nfreq, _ = CASES[name]
    f = _freqs(nfreq)
    b1, eo1, ev1 = _side(no, nv, naux, 11)
    b2, eo2, ev2 = _side(no + 1, nv, naux, 12)
    ev2 = ev2 * 1.1 + 0.005
    (r1, m1), (r2, m2) = _reference(b1, eo1, ev1, f, 2.0), _reference(b2, eo2, ev2, f, 2.0)
    fd = f.to(dev)
    qa = lib.rpa_response(b1.to(dev), eo1.to(dev), ev1.to(dev), fd, 2.0)
    qb = lib.rpa_response(b2.to(dev), eo2.to(dev), ev2.to(dev), fd, 2.0)
    out = qa.clone()
    ret = lib.rpa_response(b2.to(dev), eo2.to(dev), ev2.to(dev), fd, 2.0, out=out, accumulate=True)
    assert ret is out
    assert torch.all((out - (qa + qb)).abs().cpu() <= 1e-12 * (m1 + m2))
    assert torch.all((out.cpu() - (r1 + r2)).abs() <= 1e-12 * (m1 + m2))
    assert torch.equal(out, out.transpose(1, 2))
    # out= without accumulate overwrites whatever the tensor held
    junk = torch.full_like(qa, 3.0)
    assert torch.equal(lib.rpa_response(b1.to(dev), eo1.to(dev), ev1.to(dev), fd, 2.0, out=junk), qa)


def test_kernel_empty_sides(dev):
    """zero occupied or virtual orbitals: zeros, or the output as it was with accumulate; zero frequencies or auxiliary functions:
    an empty output"""
    from dqc_amd import lib
    b, eo, ev = (t.to(dev) for t in _side(2, 5, 6, 1))
    f = _freqs(3).to(dev)
    e0 = torch.zeros(0, dtype=torch.float64, device=dev)
    b_noocc = torch.zeros((0, 6, 16), dtype=torch.float64, device=dev)
    q = lib.rpa_response(b_noocc, e0, ev, f, 4.0)
    assert tuple(q.shape) == (3, 6, 6) and float(q.abs().max()) == 0.0
    b_novir = torch.zeros((2, 6, 0), dtype=torch.float64, device=dev)
    q = lib.rpa_response(b_novir, eo, e0, f, 4.0)
    assert tuple(q.shape) == (3, 6, 6) and float(q.abs().max()) == 0.0
    keep = lib.rpa_response(b, eo, ev, f, 4.0)
    out = keep.clone()
    lib.rpa_response(b_noocc, e0, ev, f, 4.0, out=out, accumulate=True)
    assert torch.equal(out, keep)
    lib.rpa_response(b_novir, eo, e0, f, 4.0, out=out, accumulate=True)
    assert torch.equal(out, keep)
    assert tuple(lib.rpa_response(b, eo, ev, e0, 4.0).shape) == (0, 6, 6)
    b_noaux = torch.zeros((2, 0, 16), dtype=torch.float64, device=dev)
    assert tuple(lib.rpa_response(b_noaux, eo, ev, f, 4.0).shape) == (3, 0, 0)


def test_argument_checks_raise_before_any_launch(dev):
    from dqc_amd import lib
    b, eo, ev = (t.to(dev) for t in _side(2, 5, 6, 2))
    f = _freqs(3).to(dev)
    with pytest.raises(lib.DqcAmdError):
        lib.rpa_response(b[:, :, :5].contiguous(), eo, ev, f)                   # ldv not a multiple of 16
    with pytest.raises(lib.DqcAmdError):
        lib.rpa_response(b, eo[:1], ev, f)                                      # energies that do not match the slabs
    with pytest.raises(lib.DqcAmdError):
        lib.rpa_response(b, eo, torch.cat([ev] * 4), f)                         # more virtual energies than columns
    with pytest.raises(lib.DqcAmdError):
        lib.rpa_response(b, eo, ev, f.reshape(3, 1))                            # a grid that is no vector
    with pytest.raises(lib.DqcAmdError):
        lib.rpa_response(b, eo, ev, f, accumulate=True)                         # nothing to add to
    with pytest.raises(lib.DqcAmdError):
        lib.rpa_response(b, eo, ev, f, out=torch.zeros((3, 6, 5), dtype=torch.float64, device=dev))
    L = lib.load()
    null = [None] * 5
    assert L.dqc_rpa_response(*null, -1, 5, 16, 6, 3, 1.0, 0, None, None) != 0     # the C entry point refuses negative counts itself
    assert L.dqc_rpa_response(*null, 2, 5, 16, 6, -3, 1.0, 0, None, None) != 0
    assert L.dqc_rpa_response(*null, 2, 5, 8, 6, 3, 1.0, 0, None, None) != 0       # ldv no multiple of 16
    assert L.dqc_rpa_response(*null, 2, 17, 16, 6, 3, 1.0, 0, None, None) != 0     # ldv < nv
    assert L.dqc_rpa_response(*null, 2, 5, 16, 6, 3, 1.0, 2, None, None) != 0      # accumulate neither 0 nor 1
    assert L.dqc_rpa_response(*null, 2, 5, 16, 6, 3, 1.0, 0, None, None) != 0      # null output
    q = torch.zeros((3, 6, 6), dtype=torch.float64, device=dev)
    assert L.dqc_rpa_response(q.data_ptr(), None, None, None, None, 2, 5, 16, 6, 3, 1.0, 0, None, None) != 0   # null inputs
    assert float(q.abs().max()) == 0.0
    assert L.dqc_rpa_work_doubles(1, 1, 1, 1) == 0 and L.dqc_rpa_work_doubles(-1, 5, 6, 3) == 0
    assert L.dqc_rpa_work_doubles(2, 16, 16, 4) == 2 * 4 * 16 * 16        # two chunks, one block each: two slots
    assert L.dqc_rpa_work_doubles(2, 33, 130, 685) == 0                   # enough blocks as it is


# ------------------------------------------------------------------------------------------------ 2. end to end
def _host_spins(qc, b):
    """per spin (bov, eps_occ, eps_vir) on the host, from a B tensor and the eigenpairs of the converged Fock matrix (matrices)"""
    eng = qc._engine
    h = eng.hamilton
    focks = (qc._fock[0], qc._fock[1]) if eng.polarized else (qc._fock,)
    nocc = (eng.norb.u, int((eng.orb_weight.d != 0).sum())) if eng.polarized else (eng.norb,)
    spins = []
    for fk, n in zip(focks, nocc):
        e, c = eng._eigpairs(fk)
        c = h._orthozer @ c
        bov = torch.einsum("pmn,mi,na->ipa", b, c[:, :n], c[:, n:])
        spins.append((bov.cpu(), e[:n].cpu(), e[n:].cpu()))
    return spins


def _host_quadrature(spins, r):
    """e_corr on the result's own grid, on the host"""
    from dqc_amd.rpa import energy_from_response, response_reference
    scale = 4.0 if len(spins) == 1 else 2.0
    q = sum(response_reference(bov, eo, ev, r.freqs, scale) for bov, eo, ev in spins)
    return float(energy_from_response(q, r.weights)[0])


def test_fitted_rhf_end_to_end(dev):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.rpa import plasmon_reference
    qc = _run("h2o-rhf-df")
    h = qc._engine.hamilton
    with lib.call_trace() as tr:
        r = dqc_amd.rpa(qc)
    assert any(row[0] == "dqc_rpa_response" for row in tr.rows)
    assert r.df is h.df and r.naux == h.df._b.shape[0] and r.nfreq == 48 and r.frozen == 0
    spins = _host_spins(qc, h.df._b)
    assert spins[0][0].shape[0] * spins[0][2].numel() == 5 * 8
    e_quad = _host_quadrature(spins, r)
    exact = float(plasmon_reference(spins))
    print("RI-dRPA H2O / 3-21G (naux %d, nfreq %d): e_corr %.12f  host quadrature diff %.2e  closed form diff %.2e  quadrature_error %.2e"
          "  e_corr_2nd %.12f  e_dmp2 %.12f" % (r.naux, r.nfreq, float(r.e_corr), float(r.e_corr) - e_quad, float(r.e_corr) - exact,
                                                r.quadrature_error, float(r.e_corr_2nd), float(r.e_dmp2)))
    assert abs(float(r.e_corr) - e_quad) < 1e-10
    assert abs(float(r.e_corr) - exact) < 1e-8 and r.quadrature_error < 1e-8
    assert abs(float(r.e_dmp2) - 2.0 * float(dqc_amd.mp2(qc).e_os)) < 1e-12
    assert abs(float(r.e_exx) - float(qc.energy())) < 1e-12
    assert abs(float(r.e_tot) - (float(r.e_exx) + float(r.e_corr))) < 1e-12
    assert not r.e_tot.requires_grad and tuple(r.integrand.shape) == (48,) and tuple(r.freqs.shape) == (48,)
    assert float(r.e_corr) < 0.0 and abs(float(r.e_corr)) < abs(float(r.e_dmp2))
    with lib.call_trace() as tr:                                      # served from the memo
        again = dqc_amd.rpa(qc)
    assert not any(row[0] == "dqc_rpa_response" for row in tr.rows) and float(again.e_corr) == float(r.e_corr)
    # frozen core, and a grid of another size
    f1 = dqc_amd.rpa(qc, frozen=1)
    exact1 = float(plasmon_reference(spins, frozen=1))
    print("   frozen=1: e_corr %.12f (closed form diff %.2e)" % (float(f1.e_corr), float(f1.e_corr) - exact1))
    assert abs(float(f1.e_corr) - exact1) < 1e-8 and abs(float(f1.e_corr)) < abs(float(r.e_corr))
    r64 = dqc_amd.rpa(qc, nfreq=64)
    print("   nfreq=64: e_corr diff to 48 points %.2e  quadrature_error %.2e" % (float(r64.e_corr) - float(r.e_corr), r64.quadrature_error))
    assert r64.nfreq == 64 and abs(float(r64.e_corr) - exact) < 1e-8
    # coarse grids, where the quadrature error stands far above the round-off of either side: the estimate bounds the true error
    for n in (12, 16, 24):
        rn = dqc_amd.rpa(qc, nfreq=n)
        print("   nfreq=%d: closed form diff %.2e  quadrature_error %.2e" % (n, float(rn.e_corr) - exact, rn.quadrature_error))
        assert rn.quadrature_error > 1e-9 and abs(float(rn.e_corr) - exact) <= 10.0 * rn.quadrature_error


def test_default_grid_within_ten_quadrature_errors_of_the_closed_form(dev):
    """|e_corr - closed form| <= 10 x quadrature_error at the default grid, H2O / 3-21G RHF.  At 48 points the estimate is of the order
    of 1e-15 Ha here (the second-order term is integrated to its last digits), below the 1e-14 Ha the closed form is good to in fp64
    -- it is a difference of sums of 200 Ha -- so the closed form is evaluated in 40-digit arithmetic from the same fp64 inputs; the
    energy meets the bar because its integrand is summed over the eigenvalues of Q (dqc_amd/rpa.py: energy_from_response)"""
    import dqc_amd
    from dqc_amd.rpa import plasmon_reference
    qc = _run("h2o-rhf-df")
    r = dqc_amd.rpa(qc)
    spins = _host_spins(qc, qc._engine.hamilton.df._b)
    exact, exact64 = float(plasmon_reference(spins, digits=40)), float(plasmon_reference(spins))
    print("default grid: closed form (40 digits) diff %.2e  quadrature_error %.2e  fp64 closed form - 40 digits %.2e" % (
        float(r.e_corr) - exact, r.quadrature_error, exact64 - exact))
    assert abs(float(r.e_corr) - exact) <= 10.0 * r.quadrature_error


def test_frequency_batches_give_the_same_energy(dev):
    """Q formed five frequencies at a time (what happens when nfreq naux^2 doubles do not fit): the same integrand and energies to round-off"""
    import importlib
    rpa_mod = importlib.import_module("dqc_amd.rpa")   # the module (the attribute dqc_amd.rpa is the function)
    qc = _run("h2o-rhf-df")
    with torch.no_grad():
        whole = rpa_mod._compute(qc, 0, None, 48, 1.0)
        parts = rpa_mod._compute(qc, 0, None, 48, 1.0, batch=5)
    # (the eigenvalue solver may treat a batch of five differently from one of 48: round-off of the integrand, not bit equality)
    assert float((whole[6] - parts[6]).abs().max()) <= 1e-12 * float(whole[6].abs().max())
    assert abs(float(whole[2]) - float(parts[2])) <= 1e-14   # the second-order term: no solver, another order of the sum over k
    assert abs(float(whole[1]) - float(parts[1])) < 1e-13


def test_uhf_of_a_closed_shell_equals_rhf(dev):
    import dqc_amd
    r, u = dqc_amd.rpa(_run("h2o-rhf-df")), dqc_amd.rpa(_run("h2o-uhf-df"))
    print("UHF - RHF dRPA of H2O: e_corr %.1e  e_dmp2 %.1e  e_tot %.1e" % (float(u.e_corr - r.e_corr), float(u.e_dmp2 - r.e_dmp2),
                                                                         float(u.e_tot - r.e_tot)))
    assert abs(float(u.e_corr - r.e_corr)) < 1e-8 and abs(float(u.e_dmp2 - r.e_dmp2)) < 1e-8 and abs(float(u.e_tot - r.e_tot)) < 1e-8


def test_uhf_open_shell_against_the_spin_orbital_closed_form(dev):
    """the OH radical: five alpha and four beta occupied orbitals, all spin blocks of K"""
    import dqc_amd
    from dqc_amd.rpa import plasmon_reference
    qc = _run("oh-uhf-df")
    assert qc._engine.polarized and (qc._engine.norb.u, qc._engine.norb.d) == (5, 4)
    r = dqc_amd.rpa(qc)
    spins = _host_spins(qc, qc._engine.hamilton.df._b)
    exact = float(plasmon_reference(spins))
    u = dqc_amd.mp2(qc)
    print("RI-dRPA OH / 3-21G UHF: e_corr %.12f (closed form diff %.2e)  quadrature_error %.2e" % (float(r.e_corr), float(r.e_corr) - exact,
                                                                                               r.quadrature_error))
    assert abs(float(r.e_corr) - exact) < 1e-8
    assert r.quadrature_error < 1e-8 and abs(float(r.e_exx) - float(qc.energy())) < 1e-12
    # the alpha-beta part of the second-order term is the opposite-spin MP2 energy; the same-spin parts are not e_ss (no exchange)
    assert float(r.e_dmp2) < float(u.e_os) < 0.0


def test_kohn_sham_reference(dev):
    """RPA@PBE: EXX on the PBE density plus dRPA on the PBE orbitals"""
    import dqc_amd
    qc = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid="sg2").densityfit(auxbasis="etb", exchange=True),
                    xc="gga_x_pbe+gga_c_pbe").run(fwd_options=TIGHT)
    assert qc.accepted
    r = dqc_amd.rpa(qc)
    print("RPA@PBE H2O / 3-21G: E(PBE) %.10f  e_exx %.10f  e_corr %.10f  e_dmp2 %.10f  e_tot %.10f  quadrature_error %.2e" % (
        float(qc.energy()), float(r.e_exx), float(r.e_corr), float(r.e_dmp2), float(r.e_tot), r.quadrature_error))
    assert abs(float(r.e_exx) - float(qc.energy())) > 1e-3
    assert float(r.e_exx) > float(_run("h2o-rhf-df").energy())        # the HF functional on another density: above its minimum
    assert abs(float(r.e_tot) - (float(r.e_exx) + float(r.e_corr))) < 1e-12
    assert float(r.e_corr) < 0.0 and abs(float(r.e_corr)) < abs(float(r.e_dmp2))   # ln(1 + x) - x >= -x^2 / 2 for x >= 0
    assert r.quadrature_error < 1e-8


def test_exact_reference_and_the_ri_error(dev):
    """tile-store RHF, rpa(qc, auxbasis="etb") against the closed form on the dense exact (ov|ov): the difference is the RI error"""
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.rpa import plasmon_reference
    qc = _run("h2o-rhf-exact")
    eng = qc._engine
    h = eng.hamilton
    assert h.df is None
    nao, no = h._nao_ao, eng.norb
    eri = lib.eri_dense(lib.eri_tiles(h._tab, dev), nao)
    e, c = eng._eigpairs(qc._fock)
    c = h._orthozer @ c
    co, cv = c[:, :no], c[:, no:]
    v = torch.einsum("mnls,mi,na,lj,sb->iajb", eri, co, cv, co, cv).cpu()
    exact = float(plasmon_reference([(v, e[:no].cpu(), e[no:].cpu())]))
    r = dqc_amd.rpa(qc, auxbasis="etb")
    err = float(r.e_corr) - exact
    print("exact dRPA H2O / 3-21G: e_corr %.10f;  RI (etb, naux %d): e_corr %.10f  RI error %.3e  quadrature_error %.2e"
          % (exact, r.naux, float(r.e_corr), err, r.quadrature_error))
    assert RI_ERROR_BOUND >= 3.0 * RI_MEASURED and RI_ERROR_BOUND < 1.3e-3
    assert abs(err) < RI_ERROR_BOUND
    assert abs(float(r.e_exx) - float(qc.energy())) < 1e-12          # the exact-integral Hamiltonian forms K itself
    assert r.df is dqc_amd.mp2(qc, auxbasis="etb").df                 # one tensor for both methods
