"""The Coulomb stream (j_stream_kernel, csrc/jk.hip) walks its range of the packed tile store tile by tile: block indices, tile
address and stored row count are carried from one tile to the next, the closed forms are used for a range's first tile and for a
new bra pair; a thread's patch is 4 rows x the columns {2l, 2l + 1, 32 + 2l, 33 + 2l}; a store larger than the Infinity Cache is
read with non-temporal loads.  These tests reach every branch of that walk:

    nao   8   one block, the only tile doubly diagonal
    nao   9   last block of width 1
    nao  20   last block of width 4
    nao  24   no truncation
    nao  40   15 bra pairs: a 4-tile range crosses bra pairs and meets packed-row, packed-column and plain tiles
    nao 130   a store of 0.286 GB, past the 256 MiB below which the kernel keeps the default cache policy

J only from dqc_jk_from_tiles against the dense contraction of the same store (bound 1e-12 of max |ref|, the bound
tests/test_streamed_operand_loads_gpu.py holds for this comparison), with a NON-symmetric input density (the prep symmetrises
it), deterministic mode twice with equal bits; slices of the store (dqc_jk_from_tiles_part) cut inside a bra pair, directly before
and directly after a K == L tile, summed, against the whole (1e-13 of max |J|: the partial sums are the same numbers, only the
accumulators' order of arrival differs); and the fused Fock build (fock_combine_kernel reads the accumulators in place) against
the torch form of the same build (1e-11 on the matrix, the bound tests/test_gpu_fock_builds.py holds for it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 1e-12
PART_BOUND = 1e-13
J_NAO = [8, 9, 20, 24, 40]
# (nao, cuts): tile = IJ (IJ + 1) / 2 + KL, KL diagonal (K == L) at 0, 2, 5, 9, 14
#   nao 40: 33 = (IJ 7, KL 5), directly before a K == L tile, inside the pair; 65 = (IJ 10, KL 10), directly after (IJ 10, KL 9)
#   nao 20: 12 = (IJ 4, KL 2), directly before a K == L tile; 13 directly after it
PART_CASES = [(40, (33,)), (40, (33, 65)), (20, (12, 13))]

_STORE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")
    _STORE.clear()


def _tables(nao):
    from oracle import basis as ob
    from dqc_amd import lib
    s1, s2, p1, p2, d1 = (0, [3.1, 0.7], [0.4, 0.7]), (0, [0.25], [1.0]), (1, [1.3, 0.35], [0.5, 0.6]), (1, [0.2], [1.0]), (2, [0.8], [1.0])
    atoms = {8: [[s1, p1], [s1, p1]], 9: [[s1, p1], [s1, s2, p1]], 20: [[s1, s2, p1, d1]] * 2, 24: [[s1, p1, p2, d1]] * 2,
             40: [[s1, s2, p1, d1]] * 4, 130: [[s1, s2, p1, d1]] * 13}[nao]
    # centres on a 3 x 3 x 2 lattice of 1.9 Bohr, pushed off the lattice planes
    pos = np.array([[1.9 * (k % 3) + 0.1 * (k % 2), 1.9 * ((k // 3) % 3) - 0.2 * (k % 3), 1.9 * (k // 9) + 0.3 * (k % 4)] for k in range(13)])
    t = ob.make_tables((([7, 6, 8, 6] * 4)[:len(atoms)], pos[:len(atoms)]), atoms)
    tab = lib.Tables(t.atm, t.bas, t.env)
    assert tab.nao == nao
    return tab


def _store(dev, nao):
    """(tiles, non-symmetric density, dense-contraction reference) of one shape: made once, never written to"""
    from dqc_amd import lib
    if nao not in _STORE:
        tiles = lib.eri_tiles(_tables(nao), dev)
        assert tiles.numel() == lib.eri_store_doubles(nao)
        dense = lib.eri_dense(tiles, nao)
        gen = torch.Generator(device="cpu").manual_seed(7919 + nao)
        d = torch.randn((nao, nao), dtype=torch.float64, generator=gen).to(dev)
        ref = torch.einsum("ij,ijkl->kl", 0.5 * (d + d.T), dense)
        _STORE[nao] = (tiles, d, ref)
    return _STORE[nao]


def _bits(x):
    return x.contiguous().view(torch.int64)


@pytest.mark.parametrize("nao", J_NAO)
def test_coulomb_stream_walk_vs_dense(dev, nao):
    from dqc_amd import lib
    tiles, d, ref = _store(dev, nao)
    assert float((d - d.T).abs().max()) > 0.1  # the input is not symmetric
    work = lib.jk_workspace(nao, dev)
    j, k = lib.jk(tiles, d, work, False)
    prev = lib.set_deterministic(True)
    try:
        j1, j2 = lib.jk(tiles, d, work, False)[0], lib.jk(tiles, d, work, False)[0]
    finally:
        lib.set_deterministic(prev)
    scale = float(ref.abs().max())
    e, e_det = float((j - ref).abs().max()) / scale, float((j1 - ref).abs().max()) / scale
    e_sym = float((j - j.T).abs().max()) / scale
    print("J nao %d (%d tiles): %.2e  deterministic %.2e  asymmetry %.2e" % (nao, int(lib.load().dqc_eri_tile_count(nao)), e, e_det, e_sym))
    assert k is None
    assert e < BOUND and e_det < BOUND, (nao, e, e_det)
    assert e_sym == 0.0, (nao, e_sym)
    assert torch.equal(_bits(j1), _bits(j2)), (nao, "two deterministic calls differ")


def test_coulomb_stream_past_the_caches_vs_dense(dev):
    """a store larger than the Infinity Cache (256 MiB) takes the kernel's non-temporal tile loads: 13 centres, nao 130 (0.286 GB,
    last block of width 2)"""
    from dqc_amd import lib
    nao = 130
    tiles = lib.eri_tiles(_tables(nao), dev)
    n = tiles.numel()
    assert n == lib.eri_store_doubles(nao) and 8 * n > 256 << 20
    gen = torch.Generator(device="cpu").manual_seed(nao)
    d = torch.randn((nao, nao), dtype=torch.float64, generator=gen).to(dev)
    dense = lib.eri_dense(tiles, nao)
    ref = torch.einsum("ij,ijkl->kl", 0.5 * (d + d.T), dense)
    del dense
    work = lib.jk_workspace(nao, dev)
    j = lib.jk(tiles, d, work, False)[0]
    prev = lib.set_deterministic(True)
    try:
        j1, j2 = lib.jk(tiles, d, work, False)[0], lib.jk(tiles, d, work, False)[0]
    finally:
        lib.set_deterministic(prev)
    scale = float(ref.abs().max())
    e, e_det = float((j - ref).abs().max()) / scale, float((j1 - ref).abs().max()) / scale
    print("J nao %d (%.3f GB): %.2e  deterministic %.2e" % (nao, 8e-9 * n, e, e_det))
    assert e < BOUND and e_det < BOUND, (e, e_det)
    assert torch.equal(_bits(j1), _bits(j2)), "two deterministic calls differ"


@pytest.mark.parametrize("nao,cuts", PART_CASES, ids=["nao40-2", "nao40-3", "nao20-3"])
def test_coulomb_stream_slices_add_up_to_the_whole(dev, nao, cuts):
    from dqc_amd import lib
    L = lib.load()
    tiles, d, ref = _store(dev, nao)
    nt = int(L.dqc_eri_tile_count(nao))
    work = lib.jk_workspace(nao, dev)
    whole = lib.jk(tiles, d, work, False)[0]
    edges = [0] + list(cuts) + [nt]
    total = torch.zeros_like(whole)
    for t0, t1 in zip(edges[:-1], edges[1:]):
        o0, o1 = int(L.dqc_eri_tile_offset(nao, t0)), int(L.dqc_eri_tile_offset(nao, t1))
        part = tiles[o0:o1].clone()  # an allocation of its own: the slice ends where the allocation ends
        total += lib.jk_part(part, d, work, False, t0, t1)[0]
    scale = float(whole.abs().max())
    e, e_ref = float((total - whole).abs().max()) / scale, float((total - ref).abs().max()) / float(ref.abs().max())
    print("J nao %d slices %s: sum - whole %.2e  sum - dense %.2e" % (nao, edges, e, e_ref))
    assert e < PART_BOUND, (nao, cuts, e)
    assert e_ref < BOUND, (nao, cuts, e_ref)


def _h_chain(n):
    """n hydrogen atoms on a zigzag chain (cc-pVDZ: 5 functions each)"""
    return [1] * n, [[1.5 * k, 0.6 * (k % 2), 0.25 * (k % 3)] for k in range(n)]


@pytest.mark.parametrize("natom", [4, 8], ids=["nao20", "nao40"])
def test_fused_fock_build_reads_the_stream_accumulators(dev, monkeypatch, natom):
    """one dm2scp of a restricted PBE build, fused (the combine kernel reads the Coulomb accumulators where the stream left them)
    against the torch form around dqc_jk_from_tiles"""
    import dqc_amd
    from tests import molecules as M
    eng = dqc_amd.KS(dqc_amd.Mol(_h_chain(natom), basis="cc-pvdz", grid="sg2"), xc="gga_x_pbe + gga_c_pbe")._engine
    h = eng.hamilton
    assert h._nao_ao == 5 * natom

    def density():
        sx = h._ovlp_ao @ h._orthozer
        dao = torch.as_tensor(M.seeded_dm_ao(h._nao_ao, natom, h._ovlp_ao.cpu().numpy(), 17), device=h.device)
        dd = sx.T @ dao @ sx
        w, v = torch.linalg.eigh((dd + dd.T) * 0.5)
        r = natom // 2
        return h.ao_orb2dm(v[:, -r:].contiguous(), w[-r:].contiguous())

    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("DQC_AMD_FUSED_FOCK", fused)
        out[fused] = eng.dm2scp(density())
    err = float((out["1"] - out["0"]).abs().max())
    print("H%d nao %d: max |F fused - F torch| %.2e  max |F| %.3f" % (natom, h._nao_ao, err, float(out["0"].abs().max())))
    assert err < 1e-11, (natom, err)
