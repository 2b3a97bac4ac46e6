"""BSE@G0W0 on the GPU: the fused product kernel dqc_bse_exchange and dqc_amd.bse end to end.

Yardsticks:
  * the kernel: `exchange_reference` (dqc_amd/bse.py) on the CPU in fp64 on the same synthetic inputs (noise in the padding columns of
    both slab tensors).  Bar, per element: |out - ref| <= 1e-12 sum |terms|, the standing bar of the fp64 contraction kernels,
    sum |terms| the reference applied to |L|, |X| and |R|; both sides are fp64 sums of the same terms in different orders.  Two
    launches, and noisy against zeroed padding, are bit-equal;
  * end to end: see the header of the second part."""
import pytest
import torch

from tests import molecules as M
from tests.test_gpu_gw import _host_spins
from tests.test_gpu_mp2 import TIGHT, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _inputs(np_, nq, nr, ns, naux, nvec, seed):
    """(l (np, naux, ldr), r (nq, naux, lds), both with NOISE in the padding columns, x (nvec, nr, ns)) on the host"""
    g = torch.Generator().manual_seed(seed)
    ldr, lds = (nr + 15) // 16 * 16, (ns + 15) // 16 * 16
    l = torch.randn((np_, naux, ldr), dtype=torch.float64, generator=g)
    r = torch.randn((nq, naux, lds), dtype=torch.float64, generator=g)
    x = torch.randn((nvec, nr, ns), dtype=torch.float64, generator=g)
    return l, r, x


# (np, nq, nr, ns, naux, nvec).  The kernel's tile constants (csrc/bse.hip): a block owns BSE_NV = 2 vectors, a row panel of 64 rows p
# (four MFMA tiles), a column panel of 64 columns q (one tile per wave); the inner sum runs over tiles of 16 rows r and chunks of 32
# columns s; the sum over P is split into slots = min(ceil(512 / blocks), naux) with blocks = (vector batches) (row panels) (column
# panels), ceil(naux / slots) auxiliary functions per slot.  Each of np, nq, nr, ns at 1, 15, 16, 17; ns below, at and past a chunk
# (31, 32, 33) and in a third chunk (65); nr in a second and a third tile (17, 33); np and nq below, at and past a panel (63, 64, 65)
# and in a third panel (130); nvec 1, 2, one past the batch (3) and a third batch (5).  naux: with nvec 3 and nq 65 the launch has
# 2 x 1 x 2 = 4 blocks, 128 slots: 128 is one function per slot, 129 two per slot with a single one in the last of 65 slots, 130 two in
# every slot; 1 is a single slot of one.  The Wd shape is np = nr small (occupied), nq = ns large (virtual); the Wx shape nr large, ns
# small
CASES = {
    "minimal": (1, 1, 1, 1, 1, 1),
    "below-the-tile-edge": (15, 15, 15, 15, 15, 1),
    "at-the-tile-edge": (16, 16, 16, 16, 16, 2),
    "past-the-tile-edge": (17, 17, 17, 17, 17, 3),
    "s-chunk-edge-31": (5, 20, 7, 31, 9, 1),
    "s-chunk-full": (5, 20, 7, 32, 9, 2),
    "second-s-chunk-of-one": (5, 20, 7, 33, 9, 1),
    "three-s-chunks-65": (3, 9, 4, 65, 5, 2),
    "third-r-tile-of-one": (4, 9, 33, 6, 5, 1),
    "column-panel-edge-63": (4, 63, 5, 9, 6, 1),
    "column-panel-full": (4, 64, 5, 9, 6, 2),
    "second-column-panel-of-one": (4, 65, 5, 9, 6, 1),
    "three-column-panels-130": (3, 130, 5, 6, 4, 1),
    "row-panel-edge-63": (63, 4, 9, 5, 6, 1),
    "row-panel-full": (64, 4, 9, 5, 6, 2),
    "second-row-panel-of-one": (65, 4, 9, 5, 6, 1),
    "three-row-panels-130": (130, 3, 6, 5, 4, 1),
    "three-vector-batches": (6, 7, 6, 7, 8, 5),
    "one-function-per-slot-128": (3, 65, 4, 5, 128, 3),
    "last-slot-of-one-129": (3, 65, 4, 5, 129, 3),
    "two-per-slot-130": (3, 65, 4, 5, 130, 3),
    "one-auxiliary-function": (17, 33, 17, 33, 1, 2),
    "wd-shape": (9, 70, 9, 70, 40, 2),
    "wx-shape": (9, 70, 70, 9, 40, 2),
    "wx-shape-two-panels": (66, 130, 130, 66, 7, 3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_reference(dev, name):
    from dqc_amd import lib
    from dqc_amd.bse import exchange_reference
    np_, nq, nr, ns, naux, nvec = CASES[name]
    l, r, x = _inputs(np_, nq, nr, ns, naux, nvec, 7000 + 1000 * nvec + 100 * np_ + 10 * nq + naux + nr + ns)
    ref, mag = exchange_reference(l, x, r, nr, ns), exchange_reference(l.abs(), x.abs(), r.abs(), nr, ns)
    ld, rd, xd = l.to(dev), r.to(dev), x.to(dev)
    with lib.call_trace() as tr:
        o1 = lib.bse_exchange(ld, rd, xd, nr, ns)
    assert any(row[0] == "dqc_bse_exchange" for row in tr.rows)
    assert tuple(o1.shape) == (nvec, np_, nq)
    assert torch.equal(o1, lib.bse_exchange(ld, rd, xd, nr, ns))             # launched twice: bit-equal
    lz, rz = l.clone(), r.clone()
    lz[:, :, nr:] = 0.0
    rz[:, :, ns:] = 0.0
    assert torch.equal(o1, lib.bse_exchange(lz.to(dev), rz.to(dev), xd, nr, ns))   # the padding columns do not enter, not by a bit
    junk = torch.full_like(o1, 3.0)
    assert lib.bse_exchange(ld, rd, xd, nr, ns, out=junk) is junk and torch.equal(junk, o1)
    ratio = float(((o1.cpu() - ref).abs() / mag).max())
    print("bse kernel %s (np %d, nq %d, nr %d, ns %d, naux %d, nvec %d): worst |out - ref| / sum|terms| %.2e"
          % (name, np_, nq, nr, ns, naux, nvec, ratio))
    assert torch.all((o1.cpu() - ref).abs() <= 1e-12 * mag)


def test_kernel_empty_sides(dev):
    """no vector, no row or no column: an empty output; no auxiliary function or an empty inner sum: zeros"""
    from dqc_amd import lib
    l, r, x = (t.to(dev) for t in _inputs(3, 4, 5, 6, 7, 2, 1))
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    assert tuple(lib.bse_exchange(l, r, x[:0], 5, 6).shape) == (0, 3, 4)
    assert tuple(lib.bse_exchange(l[:0], r, x, 5, 6).shape) == (2, 0, 4)
    assert tuple(lib.bse_exchange(l, r[:0], x, 5, 6).shape) == (2, 3, 0)
    for o in (lib.bse_exchange(z(3, 0, 16), z(4, 0, 16), x, 5, 6, out=torch.full((2, 3, 4), 7.0, dtype=torch.float64, device=dev)),
              lib.bse_exchange(l, r, z(2, 0, 6), 0, 6, out=torch.full((2, 3, 4), 7.0, dtype=torch.float64, device=dev)),
              lib.bse_exchange(l, r, z(2, 5, 0), 5, 0, out=torch.full((2, 3, 4), 7.0, dtype=torch.float64, device=dev))):
        assert tuple(o.shape) == (2, 3, 4) and float(o.abs().max()) == 0.0


def test_argument_checks_raise_before_any_launch(dev):
    from dqc_amd import lib
    l, r, x = (t.to(dev) for t in _inputs(3, 4, 5, 6, 7, 2, 2))
    off = lambda t: torch.zeros(t.numel() + 1, dtype=torch.float64, device=dev)[1:].view(t.shape)  # noqa: E731
    bad = [
        lambda: lib.bse_exchange(l[:, :, :5].contiguous(), r, x, 5, 6),                    # ldr not a multiple of 16
        lambda: lib.bse_exchange(l, r[:, :, :6].contiguous(), x, 5, 6),                    # lds not a multiple of 16
        lambda: lib.bse_exchange(l, r, torch.zeros((2, 17, 6), dtype=torch.float64, device=dev), 17, 6),   # more columns than the slabs hold
        lambda: lib.bse_exchange(l, r, x, 5, -1),
        lambda: lib.bse_exchange(l, r[:, :6].contiguous(), x, 5, 6),                       # another number of auxiliary functions
        lambda: lib.bse_exchange(l, r, x[:, :4].contiguous(), 5, 6),                       # x of another shape
        lambda: lib.bse_exchange(l, r, x[0], 5, 6),                                        # no batch of vectors
        lambda: lib.bse_exchange(l[0], r, x, 5, 6),
        lambda: lib.bse_exchange(l.float(), r, x, 5, 6),                                   # dtype
        lambda: lib.bse_exchange(l, r, x.float(), 5, 6),
        lambda: lib.bse_exchange(l.cpu(), r, x, 5, 6),                                     # device
        lambda: lib.bse_exchange(l, r, x.cpu(), 5, 6),
        lambda: lib.bse_exchange(l, r, x.transpose(1, 2).contiguous().transpose(1, 2), 5, 6),   # strides
        lambda: lib.bse_exchange(l, r, x, 5, 6, out=torch.zeros((2, 3, 5), dtype=torch.float64, device=dev)),
        lambda: lib.bse_exchange(off(l), r, x, 5, 6),                                      # alignment
        lambda: lib.bse_exchange(l, off(r), x, 5, 6),
    ]
    o = torch.zeros((2, 3, 4), dtype=torch.float64, device=dev)
    wk = torch.zeros(int(lib.load().dqc_bse_work_doubles(3, 4, 5, 6, 7, 2)) + 1, dtype=torch.float64, device=dev)
    L = lib.load()
    po, pl, pr, px, pw = (t.data_ptr() for t in (o, l, r, x, wk))
    with lib.call_trace() as tr:
        for f in bad:
            with pytest.raises(lib.DqcAmdError):
                f()
        # the C entry point refuses by itself: (out, l, r, x, np, nq, nr, ns, ldr, lds, naux, nvec, work, stream)
        for k in range(8):
            counts = [3, 4, 5, 6, 16, 16, 7, 2]
            counts[k] = -1
            assert L.dqc_bse_exchange(po, pl, pr, px, *counts, pw, None) != 0              # every count negative in turn
        assert L.dqc_bse_exchange(po, pl, pr, px, 3, 4, 5, 6, 8, 16, 7, 2, pw, None) != 0      # ldr no multiple of 16
        assert L.dqc_bse_exchange(po, pl, pr, px, 3, 4, 5, 6, 16, 24, 7, 2, pw, None) != 0     # lds no multiple of 16
        assert L.dqc_bse_exchange(po, pl, pr, px, 3, 4, 17, 6, 16, 16, 7, 2, pw, None) != 0    # ldr < nr
        assert L.dqc_bse_exchange(po, pl, pr, px, 3, 4, 5, 17, 16, 16, 7, 2, pw, None) != 0    # lds < ns
        assert L.dqc_bse_exchange(None, pl, pr, px, 3, 4, 5, 6, 16, 16, 7, 2, pw, None) != 0   # null output
        assert L.dqc_bse_exchange(po, None, pr, px, 3, 4, 5, 6, 16, 16, 7, 2, pw, None) != 0   # null inputs
        assert L.dqc_bse_exchange(po, pl, None, px, 3, 4, 5, 6, 16, 16, 7, 2, pw, None) != 0
        assert L.dqc_bse_exchange(po, pl, pr, None, 3, 4, 5, 6, 16, 16, 7, 2, pw, None) != 0
        assert L.dqc_bse_exchange(po, pl, pr, px, 3, 4, 5, 6, 16, 16, 7, 2, None, None) != 0   # the sum is split: null work buffer
        assert L.dqc_bse_exchange(po, pl + 8, pr, px, 3, 4, 5, 6, 16, 16, 7, 2, pw, None) != 0   # misaligned
        assert L.dqc_bse_exchange(po, pl, pr + 8, px, 3, 4, 5, 6, 16, 16, 7, 2, pw, None) != 0
        assert L.dqc_bse_exchange(po, pl, pr, px, 1 << 20, 1 << 20, 5, 6, 16, 16, 7, 1 << 20, pw, None) != 0   # too many blocks
        assert b"blocks" in L.dqc_last_error()
        assert L.dqc_bse_exchange(po, pl, pr, px, 1 << 30, 1 << 30, 5, 6, 16, 16, 7, 1 << 30, pw, None) != 0   # past a 64-bit count
        assert L.dqc_bse_exchange(None, None, None, None, 0, 4, 5, 6, 16, 16, 7, 2, None, None) == 0   # an empty output is legal
        assert L.dqc_bse_work_doubles(3, 4, 5, 6, 7, 2) == 7 * 2 * 3 * 4 and L.dqc_bse_work_doubles(-3, 4, 5, 6, 7, 2) == 0
    assert not tr.rows and float(o.abs().max()) == 0.0 and float(wk.abs().max()) == 0.0   # nothing was launched, nothing written


# ------------------------------------------------------------------------------------------------ 2. end to end
# H2O / 3-21G, densityfit(exchange=True) with "etb" (naux 101), SCF converged to TIGHT; the ov space is 5 x 8 = 40.  Yardsticks:
#   * bse(qc, qp=E) against `bse_reference` on the host from the Hamiltonian's tensor, the eigenpairs of the converged Fock matrix, M
#     from `rpa.response_reference` at w = 0 and the same E = eps + a fixed made-up shift pattern (no Pade noise enters): singlet and
#     triplet, TDA and full.  nstates = 5 with tol = 1e-9: 1e-8 Ha (the eigenvalue error is second order in the residual for TDA and
#     first order at worst for the full problem: 10 x tol); nstates = 40, the whole space, where the solvers are exact: 1e-10 Ha, and
#     the oscillator strengths to 1e-8.  The same on a PBE reference (BSE on Kohn-Sham orbitals);
#   * the default path: bse(qc) is bse(qc, qp=quasiparticle_ladder(...)) of gw(qc, orbs=<the window>) bit for bit;
#   * screened=False (RI-TDHF / RI-CIS) on the fitted run against dqc_amd.excitations of the exact-integral run: the RI error of the
#     reference's own integrals, deterministic.  Measured over TDA and full, singlet and triplet, the lowest 5: see RI_TDHF_MEASURED;
#     asserted at 3 x that rounded up to one digit, as RI_HOMO_BOUND of tests/test_gpu_gw.py is made;
#   * exact-integral RHF with bse(qc, auxbasis="etb", qp=E) against the fitted run, E each run's own eps + the shift pattern:
#     RI_BSE_MEASURED, the bound made the same way.
RI_TDHF_MEASURED, RI_TDHF_BOUND = 1.095e-4, 4e-4   # Ha: the second triplet state of the full problem (singlets: 4.1e-5 at most)
RI_BSE_MEASURED, RI_BSE_BOUND = 9.40e-5, 3e-4      # Ha: the lowest singlet state (the five: -9.4e-5 ... -6.1e-5)


def _shifted(eps, nocc, scale=1.0):
    """eps + a fixed made-up correction: occupied down, virtual up, each orbital by its own amount.  scale: 1 on Hartree-Fock
    energies; 8 on PBE ones, whose gap (0.27 Ha) the kernel closes unless it is opened about as far as G0W0 opens it -- with scale 1 the
    lowest TDA energy is -0.016 Ha and A - B is not positive definite, which `bse` and `bse_reference` both refuse"""
    k = torch.arange(eps.numel(), dtype=eps.dtype, device=eps.device)
    return torch.where(k < nocc, eps - scale * (0.020 + 0.003 * k), eps + scale * (0.030 + 0.002 * k))


def _static_m(bov, eps, nocc):
    from dqc_amd.rpa import response_reference
    q0 = response_reference(bov, eps[:nocc], eps[nocc:], torch.zeros(1, dtype=torch.float64), 4.0)[0]
    eye = torch.eye(q0.shape[0], dtype=torch.float64)
    return torch.cholesky_solve(eye, torch.linalg.cholesky(q0 + eye))


_PBE = {}


def _pbe():
    if not _PBE:
        import dqc_amd
        qc = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="3-21G", grid="sg2").densityfit(auxbasis="etb", exchange=True),
                        xc="gga_x_pbe+gga_c_pbe").run(fwd_options=TIGHT)
        assert qc.accepted
        _PBE["qc"] = qc
    return _PBE["qc"]


def _host_side(qc, scale=1.0):
    """(bmo, bov, eps, E, M, r_ia (3, 40)) on the host; scale: that of `_shifted`"""
    from dqc_amd import lib
    from dqc_amd.postscf import orbitals
    bmo, bov, eps = _host_spins(qc, qc._engine.hamilton.df._b)[0]
    co, cv, _, _ = orbitals(qc, 0)[0]
    h = qc.get_system().get_hamiltonian()
    r = torch.matmul(torch.matmul(co.t(), lib.int1e("r0", h._tab, h.device)), cv).reshape(3, -1).cpu()
    return bmo, bov, eps, _shifted(eps, 5, scale), _static_m(bov, eps, 5), r


@pytest.mark.parametrize("ref", ["rhf", "pbe"])
@pytest.mark.parametrize("spin", ["singlet", "triplet"])
@pytest.mark.parametrize("tda", [True, False])
def test_against_the_dense_matrices(dev, ref, spin, tda):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.bse import bse_reference
    qc = _run("h2o-rhf-df") if ref == "rhf" else _pbe()
    bmo, bov, eps, e_qp, m, r = _host_side(qc, 1.0 if ref == "rhf" else 8.0)
    assert bov.shape[0] * bov.shape[2] == 5 * 8
    w, xpy = bse_reference(bmo, e_qp, 5, m, spin, tda)
    f = (2.0 / 3.0) * w * ((2.0 ** 0.5 * (xpy @ r.t())) ** 2).sum(1)
    with lib.call_trace() as tr:
        low = dqc_amd.bse(qc, nstates=5, spin=spin, tda=tda, qp=e_qp, tol=1e-9)
    assert any(row[0] == "dqc_bse_exchange" for row in tr.rows) and not any(row[0] == "dqc_gw_screened_diag" for row in tr.rows)
    full = dqc_amd.bse(qc, nstates=40, spin=spin, tda=tda, qp=e_qp, tol=1e-9)
    e5, e40 = float((low.energies - w[:5]).abs().max()), float((full.energies - w).abs().max())
    ef = float((full.osc_strengths - (f if spin == "singlet" else 0.0 * f)).abs().max())
    print("BSE %s H2O / 3-21G %s %s: lowest %.6f Ha; 5 states: diff %.2e (bar 1e-8, residual %.1e)  40 states: diff %.2e (bar 1e-10)  "
          "osc diff %.2e (bar 1e-8, largest f %.4f)" % (ref, spin, "TDA" if tda else "full", float(w[0]), e5, low.residual, e40, ef,
                                                        float(full.osc_strengths.max())))
    assert low.gw is None and low.window_orbs is None and low.spin == spin and low.tda == tda and low.naux == bmo.shape[1]
    assert low.df is qc._engine.hamilton.df and torch.equal(low.qp_energies, e_qp) and not low.energies.requires_grad
    assert tuple(low.xpy.shape) == (5, 40) and (low.xmy is None) == tda and tuple(full.transition_dipoles.shape) == (40, 3)
    assert low.residual < 1e-9
    assert e5 <= 1e-8
    assert e40 <= 1e-10
    assert ef <= 1e-8
    if spin == "singlet":
        assert float(full.osc_strengths.max()) > 1e-2                  # (there is something to compare)
    else:
        assert float(full.osc_strengths.abs().max()) == 0.0
    if not tda:
        assert float(((full.xpy * full.xmy).sum(1) - 1.0).abs().max()) < 1e-10


def test_tda_singlets_lie_above_triplets(dev):
    """A_singlet - A_triplet = 2 v is positive semidefinite: state by state (Weyl)"""
    import dqc_amd
    qc = _run("h2o-rhf-df")
    e_qp = _host_side(qc)[3]
    s = dqc_amd.bse(qc, nstates=40, spin="singlet", tda=True, qp=e_qp, tol=1e-9).energies
    t = dqc_amd.bse(qc, nstates=40, spin="triplet", tda=True, qp=e_qp, tol=1e-9).energies
    print("BSE TDA H2O: smallest singlet - triplet %.3e Ha" % float((s - t).min()))
    assert bool(torch.all(s >= t - 1e-10))


def test_default_path_is_the_ladder_of_gw(dev):
    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.bse import quasiparticle_ladder
    qc = _run("h2o-rhf-df")
    with lib.call_trace() as tr:
        r = dqc_amd.bse(qc)
    names = {row[0] for row in tr.rows}
    assert "dqc_bse_exchange" in names and "dqc_gw_screened_diag" in names and "dqc_rpa_response" in names
    assert r.window_orbs == list(range(1, 9)) and r.spin == "singlet" and not r.tda and r.screened
    g = dqc_amd.gw(qc, orbs=r.window_orbs)
    assert r.gw.orbs == g.orbs and torch.equal(r.gw.qp_energies, g.qp_energies) and bool(r.gw.converged.all())
    eps = _host_side(qc)[2]
    e_qp = quasiparticle_ladder(eps, 5, g.orbs, g.qp_energies)
    assert torch.equal(r.qp_energies, e_qp)
    shift = e_qp - eps                                                  # the scissor (to the rounding of eps + shift - eps)
    assert abs(float(shift[0] - shift[1])) < 1e-13 and abs(float(shift[12] - shift[8])) < 1e-13 and abs(float(shift[1] - shift[2])) > 1e-6
    r2 = dqc_amd.bse(qc, qp=e_qp)
    assert r2.gw is None and torch.equal(r.energies, r2.energies) and torch.equal(r.osc_strengths, r2.osc_strengths)
    with lib.call_trace() as tr:
        r3 = dqc_amd.bse(qc)                                            # gw from the memo: the same object, the same numbers
    assert r3.gw is r.gw and torch.equal(r3.energies, r.energies) and not any(row[0] == "dqc_gw_screened_diag" for row in tr.rows)
    un = dqc_amd.bse(qc, screened=False)
    print("BSE@G0W0@HF H2O / 3-21G: %s\n   G0W0 gap %.6f (HF %.6f);  RI-TDHF lowest %.6f" % (r, r.gw.gap, float(eps[5] - eps[4]), float(un.energies[0])))
    assert un.gw is None and torch.equal(un.qp_energies, eps) and not un.screened
    assert float(r.energies[0]) > 0.0 and abs(float(r.energies[0] - un.energies[0])) > 1e-4


def test_unscreened_is_tdhf_up_to_the_ri_error(dev):
    """screened=False on the fitted run against dqc_amd.excitations on the exact integrals"""
    import dqc_amd
    fit, exact = _run("h2o-rhf-df"), _run("h2o-rhf-exact")
    worst = 0.0
    for spin in ("singlet", "triplet"):
        for tda in (True, False):
            a = dqc_amd.bse(fit, nstates=5, spin=spin, tda=tda, screened=False, tol=1e-8)
            b = dqc_amd.excitations(exact, nstates=5, spin=spin, tda=tda, tol=1e-8)
            d = (a.energies - b.energies.cpu())
            worst = max(worst, float(d.abs().max()))
            print("RI-TDHF - TDHF H2O / 3-21G %s %s: %s  (lowest %.6f Ha; osc diff %.2e)" % (
                spin, "TDA" if tda else "full", ["%.3e" % float(v) for v in d], float(b.energies[0]),
                float((a.osc_strengths - b.osc_strengths.cpu()).abs().max())))
    print("RI-TDHF - TDHF: largest |difference| %.3e Ha (bound %s)" % (worst, RI_TDHF_BOUND))
    assert RI_TDHF_BOUND >= 3.0 * RI_TDHF_MEASURED and RI_TDHF_BOUND <= 6.0 * RI_TDHF_MEASURED
    assert worst < RI_TDHF_BOUND


def test_exact_reference_with_a_tensor_built_here(dev):
    """tile-store RHF with bse(qc, auxbasis="etb", qp=E): the orbitals from the exact integrals, the kernel from a tensor built here"""
    import dqc_amd
    from dqc_amd.postscf import orbitals
    fit, exact = _run("h2o-rhf-df"), _run("h2o-rhf-exact")
    assert exact._engine.hamilton.df is None
    es = []
    for qc in (exact, fit):
        _, _, eo, ev = orbitals(qc, 0)[0]
        es.append(dqc_amd.bse(qc, auxbasis="etb", qp=_shifted(torch.cat([eo, ev]).cpu(), 5), tol=1e-8))
    d = es[0].energies - es[1].energies
    worst = float(d.abs().max())
    print("exact-integral BSE H2O / 3-21G (naux %d) - fitted run: %s;  largest %.3e Ha (bound %s)"
          % (es[0].naux, ["%.3e" % float(v) for v in d], worst, RI_BSE_BOUND))
    assert es[0].df is dqc_amd.mp2(exact, auxbasis="etb").df and es[1].df is fit._engine.hamilton.df
    assert RI_BSE_BOUND >= 3.0 * RI_BSE_MEASURED and RI_BSE_BOUND <= 6.0 * RI_BSE_MEASURED
    assert worst < RI_BSE_BOUND
