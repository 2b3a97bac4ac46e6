"""The integral-driven particle-particle ladder kernel dqc_cc_ladder (csrc/cc.hip) alone.

Yardstick: `exchange_reference` (dqc_amd/bse.py) on the CPU in fp64 on the same synthetic inputs, noise in every padding column of both
slab tensors -- the same contraction summed vector by vector, the intermediate stored.  Bar, per element: |out - ref| <= 1e-12 sum
|terms|, the standing bar of the fp64 contraction kernels, sum |terms| the reference applied to |L|, |X| and |R|; both sides are fp64
sums of the same terms in different orders.  Two launches, and noisy against zeroed padding, are bit-equal.  The vector-driven kernel
of the parent (dqc_bse_exchange) on the same operands is a second witness, on the GPU, at twice the bar (two kernels' errors)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


def _inputs(np_, nq, nr, ns, naux, nvec, seed, same=False):
    """(l (np, naux, ldr), r (nq, naux, lds), both with NOISE in the padding columns, x (nvec, nr, ns)) on the host; same: r is l"""
    g = torch.Generator().manual_seed(seed)
    ldr, lds = (nr + 15) // 16 * 16, (ns + 15) // 16 * 16
    l = torch.randn((np_, naux, ldr), dtype=torch.float64, generator=g)
    r = l if same else torch.randn((nq, naux, lds), dtype=torch.float64, generator=g)
    x = torch.randn((nvec, nr, ns), dtype=torch.float64, generator=g)
    return l, r, x


def _kernel_x(x):
    """(nvec, nr, ns) -> the kernel's layout (nr, ns, nvec): the vector index last"""
    return x.permute(1, 2, 0).contiguous()


# (np, nq, nr, ns, naux, nvec, L and R one tensor).  The kernel's tile constants (csrc/cc.hip): a block of eight waves owns ONE row p, one
# tile of CC_QW = 16 columns q (two of them built per wave) and a vector panel of at most 8 waves x CC_NVT = 9 tiles x 16 = 1152
# vectors; a launch of more vectors splits them into equal panels of whole tiles.  The inner sum runs over tiles of 16 rows r times
# tiles of 16 columns s; a W tile is summed over P in k-steps of 4, three in flight, the loop advancing by 12.  No sum is split over
# blocks: there are no slots.  So: each of np, nq, nr, ns at 1, 15, 16, 17 (below, at and past the only tile edge there is) and at 33
# (a third tile; for np a 33rd block row); nvec 1, 15 / 16 / 17 (a vector tile), 128 / 129 (one tile per wave / the first wave with
# two), 1152 / 1153 (a full panel / two panels of 37 and 36 tiles, five per wave); naux 1, 3, 4, 5 (the k-step), 8 and 9 (the second
# fetch), 11, 12, 13 (the loop stride), 24 and 25 (two trips and one more k-step).
CASES = {
    "minimal": (1, 1, 1, 1, 1, 1, False),
    "below-the-tile-edge": (15, 15, 15, 15, 3, 15, False),
    "at-the-tile-edge": (16, 16, 16, 16, 4, 16, False),
    "past-the-tile-edge": (17, 17, 17, 17, 5, 17, False),
    "one-tensor-below": (15, 15, 15, 15, 8, 2, True),
    "one-tensor-at": (16, 16, 16, 16, 9, 3, True),
    "one-tensor-past": (17, 17, 17, 17, 11, 2, True),
    "one-tensor-one": (1, 1, 1, 1, 12, 3, True),
    "p-33": (33, 2, 3, 4, 13, 2, False),
    "q-third-tile": (2, 33, 4, 3, 24, 2, False),
    "r-third-tile": (2, 3, 33, 4, 25, 2, False),
    "s-third-tile": (3, 2, 4, 33, 5, 2, False),
    "q-1-r-17-s-15": (3, 1, 17, 15, 7, 3, False),
    "q-15-r-1-s-16": (2, 15, 1, 16, 6, 2, False),
    "q-16-r-15-s-1": (2, 16, 15, 1, 4, 2, False),
    "q-17-r-16-s-17": (1, 17, 16, 17, 3, 2, False),
    "one-tile-per-wave-128": (2, 3, 3, 2, 5, 128, False),
    "first-wave-with-two-129": (2, 3, 3, 2, 5, 129, False),
    "full-panel-1152": (1, 2, 3, 2, 3, 1152, False),
    "two-panels-1153": (2, 3, 3, 2, 3, 1153, False),
    "all-33-nvec-37": (33, 33, 33, 33, 10, 37, False),
    "one-tensor-33-nvec-37": (33, 33, 33, 33, 6, 37, True),
    "ccsd-shape": (19, 19, 19, 19, 40, 15, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_reference(dev, name):
    from dqc_amd import lib
    from dqc_amd.bse import exchange_reference
    np_, nq, nr, ns, naux, nvec, same = CASES[name]
    l, r, x = _inputs(np_, nq, nr, ns, naux, nvec, 9000 + 1000 * nvec + 100 * np_ + 10 * nq + naux + nr + ns, same)
    ref, mag = exchange_reference(l, x, r, nr, ns), exchange_reference(l.abs(), x.abs(), r.abs(), nr, ns)
    ld, xd = l.to(dev), _kernel_x(x).to(dev)
    rd = ld if same else r.to(dev)
    with lib.call_trace() as tr:
        o1 = lib.cc_ladder(ld, rd, xd, nr, ns)
    assert any(row[0] == "dqc_cc_ladder" for row in tr.rows)
    assert tuple(o1.shape) == (nvec, np_, nq)
    assert torch.equal(o1, lib.cc_ladder(ld, rd, xd, nr, ns))                # launched twice: bit-equal
    lz, rz = l.clone(), r.clone()
    lz[:, :, nr:] = 0.0
    rz[:, :, ns:] = 0.0
    assert torch.equal(o1, lib.cc_ladder(lz.to(dev), rz.to(dev), xd, nr, ns))      # the padding columns do not enter, not by a bit
    junk = torch.full_like(o1, 3.0)
    assert lib.cc_ladder(ld, rd, xd, nr, ns, out=junk) is junk and torch.equal(junk, o1)
    ratio = float(((o1.cpu() - ref).abs() / mag).max())
    # the parent's fused kernel on the same operands, in its layout
    ob = lib.bse_exchange(ld, rd, x.to(dev), nr, ns)
    ratio_b = float(((o1 - ob).abs().cpu() / mag).max())
    print("cc ladder %s (np %d, nq %d, nr %d, ns %d, naux %d, nvec %d%s): worst |out - ref| / sum|terms| %.2e;  against dqc_bse_exchange %.2e"
          % (name, np_, nq, nr, ns, naux, nvec, ", one tensor" if same else "", ratio, ratio_b))
    assert torch.all((o1.cpu() - ref).abs() <= 1e-12 * mag)
    assert torch.all((o1 - ob).abs().cpu() <= 2e-12 * mag)


def test_kernel_empty_sides(dev):
    """no vector, no row or no column: an empty output; no auxiliary function or an empty inner sum: zeros, nothing launched"""
    from dqc_amd import lib
    l, r, x = _inputs(3, 4, 5, 6, 7, 2, 1)
    l, r, x = l.to(dev), r.to(dev), _kernel_x(x).to(dev)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    seven = lambda: torch.full((2, 3, 4), 7.0, dtype=torch.float64, device=dev)  # noqa: E731
    assert tuple(lib.cc_ladder(l, r, x[:, :, :0].contiguous(), 5, 6).shape) == (0, 3, 4)
    assert tuple(lib.cc_ladder(l[:0], r, x, 5, 6).shape) == (2, 0, 4)
    assert tuple(lib.cc_ladder(l, r[:0], x, 5, 6).shape) == (2, 3, 0)
    for o in (lib.cc_ladder(z(3, 0, 16), z(4, 0, 16), x, 5, 6, out=seven()),
              lib.cc_ladder(l, r, z(0, 6, 2), 0, 6, out=seven()),
              lib.cc_ladder(l, r, z(5, 0, 2), 5, 0, out=seven())):
        assert tuple(o.shape) == (2, 3, 4) and float(o.abs().max()) == 0.0


def test_argument_checks_raise_before_any_launch(dev):
    from dqc_amd import lib
    l, r, x = _inputs(3, 4, 5, 6, 7, 2, 2)
    l, r, x = l.to(dev), r.to(dev), _kernel_x(x).to(dev)
    bad = [
        lambda: lib.cc_ladder(l[:, :, :5].contiguous(), r, x, 5, 6),                      # ldr not a multiple of 16
        lambda: lib.cc_ladder(l, r[:, :, :6].contiguous(), x, 5, 6),                      # lds not a multiple of 16
        lambda: lib.cc_ladder(l, r, torch.zeros((17, 6, 2), dtype=torch.float64, device=dev), 17, 6),   # more columns than the slabs hold
        lambda: lib.cc_ladder(l, r, x, 5, -1),
        lambda: lib.cc_ladder(l, r[:, :6].contiguous(), x, 5, 6),                         # another number of auxiliary functions
        lambda: lib.cc_ladder(l, r, x[:4].contiguous(), 5, 6),                            # x of another shape
        lambda: lib.cc_ladder(l, r, x.permute(2, 0, 1).contiguous(), 5, 6),               # x in the layout of bse_exchange
        lambda: lib.cc_ladder(l, r, x[:, :, 0], 5, 6),                                    # no batch of vectors
        lambda: lib.cc_ladder(l[0], r, x, 5, 6),
        lambda: lib.cc_ladder(l.float(), r, x, 5, 6),                                     # dtype
        lambda: lib.cc_ladder(l, r, x.float(), 5, 6),
        lambda: lib.cc_ladder(l.cpu(), r, x, 5, 6),                                       # device
        lambda: lib.cc_ladder(l, r, x.cpu(), 5, 6),
        lambda: lib.cc_ladder(l, r, x.transpose(0, 1).contiguous().transpose(0, 1), 5, 6),      # strides
        lambda: lib.cc_ladder(l, r, x, 5, 6, out=torch.zeros((2, 3, 5), dtype=torch.float64, device=dev)),
    ]
    o = torch.zeros((2, 3, 4), dtype=torch.float64, device=dev)
    L = lib.load()
    po, pl, pr, px = (t.data_ptr() for t in (o, l, r, x))
    with lib.call_trace() as tr:
        for f in bad:
            with pytest.raises(lib.DqcAmdError, match="cc_ladder"):
                f()
        # the C entry point refuses by itself: (out, l, r, x, np, nq, nr, ns, ldr, lds, naux, nvec, work, stream)
        for k in range(8):
            counts = [3, 4, 5, 6, 16, 16, 7, 2]
            counts[k] = -1
            assert L.dqc_cc_ladder(po, pl, pr, px, *counts, None, None) != 0                 # every count negative in turn
        assert L.dqc_cc_ladder(po, pl, pr, px, 3, 4, 5, 6, 8, 16, 7, 2, None, None) != 0         # ldr no multiple of 16
        assert L.dqc_cc_ladder(po, pl, pr, px, 3, 4, 5, 6, 16, 24, 7, 2, None, None) != 0        # lds no multiple of 16
        assert L.dqc_cc_ladder(po, pl, pr, px, 3, 4, 17, 6, 16, 16, 7, 2, None, None) != 0       # ldr < nr
        assert L.dqc_cc_ladder(po, pl, pr, px, 3, 4, 5, 17, 16, 16, 7, 2, None, None) != 0       # lds < ns
        assert L.dqc_cc_ladder(None, pl, pr, px, 3, 4, 5, 6, 16, 16, 7, 2, None, None) != 0      # null output
        assert L.dqc_cc_ladder(po, None, pr, px, 3, 4, 5, 6, 16, 16, 7, 2, None, None) != 0      # null inputs
        assert L.dqc_cc_ladder(po, pl, None, px, 3, 4, 5, 6, 16, 16, 7, 2, None, None) != 0
        assert L.dqc_cc_ladder(po, pl, pr, None, 3, 4, 5, 6, 16, 16, 7, 2, None, None) != 0
        assert L.dqc_cc_ladder(po, pl, pr, px, 1 << 20, 1 << 20, 5, 6, 16, 16, 7, 1 << 20, None, None) != 0   # too many blocks
        assert b"blocks" in L.dqc_last_error()
        assert L.dqc_cc_ladder(po, pl, pr, px, 1 << 30, 1 << 30, 5, 6, 16, 16, 7, 1 << 30, None, None) != 0   # past a 64-bit count
        assert L.dqc_cc_ladder(None, None, None, None, 0, 4, 5, 6, 16, 16, 7, 2, None, None) == 0   # an empty output is legal
    assert not tr.rows and float(o.abs().max()) == 0.0        # nothing was launched, nothing written


def test_no_allocation_grows_like_the_four_index_quantity(dev):
    """np = nq = nr = ns = 96: W would be 96^4 doubles = 679 MB.  The work buffer stays below the project's cap of 2^24 doubles (it is
    empty: no sum is split) and a call allocates its output and nothing else"""
    from dqc_amd import lib
    n, naux, nvec = 96, 8, 4
    need = int(lib.load().dqc_cc_ladder_work_doubles(n, n, n, n, naux, nvec))
    assert need < (1 << 24) and need * 1000 < n ** 4
    l, r, x = _inputs(n, n, n, n, naux, nvec, 5)
    l, r, x = l.to(dev), r.to(dev), _kernel_x(x).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = lib.cc_ladder(l, r, x, n, n)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(dev) - before
    print("cc ladder n = 96: work doubles %d; peak device memory of the call %d bytes (output %d, W would be %d)"
          % (need, grown, out.numel() * 8, 8 * n ** 4))
    assert grown <= 2 * out.numel() * 8 + 4096
    from dqc_amd.bse import exchange_reference
    lh, rh, xh = l.cpu(), r.cpu(), x.permute(2, 0, 1).contiguous().cpu()
    ref, mag = exchange_reference(lh, xh, rh, n, n), exchange_reference(lh.abs(), xh.abs(), rh.abs(), n, n)
    assert torch.all((out.cpu() - ref).abs() <= 1e-12 * mag)
