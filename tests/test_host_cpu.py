"""CPU tests (-m "not gpu") of the host logic and of the C-ABI library surface (no compute calls)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import basis as ob, grid as og
from tests import molecules as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_declared_symbol():
    """libdqc_amd.so loads without a GPU and exports exactly the entry points include/dqc_amd.h declares"""
    from dqc_amd import build, lib
    build.build()
    hdr = open(os.path.join(ROOT, "include", "dqc_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(dqc_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 14
    so = ctypes.CDLL(lib.libpath())
    for n in names:
        assert hasattr(so, n), n
    L = lib.load()
    assert L.dqc_version() >= 100
    assert L.dqc_padded_nao(114) == 128 and L.dqc_padded_nao(208) == 208 and L.dqc_padded_nao(7) == 16
    assert L.dqc_ao_stride(114) == 120 and L.dqc_ao_stride(7) == 8 and L.dqc_ao_stride(208) == 208 and L.dqc_ao_stride(412) == 416
    L.dqc_ao_doubles.restype = __import__("ctypes").c_size_t
    assert L.dqc_ao_doubles(4, 10, 114) == 4 * 10 * 120 + 8
    assert L.dqc_eri_tile_count(208) == 351 * 352 // 2 * (351 * 352 // 2 + 1) // 2 or L.dqc_eri_tile_count(208) > 0
    nb = 26
    npair = nb * (nb + 1) // 2
    assert L.dqc_eri_tile_count(208) == npair * (npair + 1) // 2
    L.dqc_eri_store_doubles.restype = ctypes.c_size_t
    # packed store: diagonal block pairs keep 36 of their 64 rows / columns
    # ... and the pairs of the last block keep only the rows of real AOs (nao = 8 last + wl: 8 wl resp. wl (wl + 1) / 2 rows)
    assert L.dqc_eri_store_doubles(7) == 28 * 36 and L.dqc_eri_store_doubles(16) == 36 * 36 + 64 * (36 + 64) + 36 * (36 + 64 + 36)
    L.dqc_eri_tile_offset.argtypes = [ctypes.c_int, ctypes.c_longlong]
    L.dqc_eri_tile_offset.restype = ctypes.c_longlong
    for nao in (1, 9, 17, 23, 114, 120, 121, 412):  # explicit prefix sums over the block pairs
        nb_ = (nao + 7) // 8
        last, wl = nb_ - 1, nao - 8 * (nb_ - 1)
        tot, P, tile = 0, 0, 0
        for x in range(nb_):
            for y in range(x + 1):
                r = (wl * (wl + 1) // 2 if x == y else 8 * wl) if (x == last and wl < 8) else (36 if x == y else 64)
                if nao <= 23:  # every tile offset of the small stores
                    for kl in range(P + 1):
                        kk = int(((8 * kl + 1) ** 0.5 - 1) / 2)
                        while kk * (kk + 1) // 2 > kl:
                            kk -= 1
                        while (kk + 1) * (kk + 2) // 2 <= kl:
                            kk += 1
                        assert L.dqc_eri_tile_offset(nao, tile) == tot + r * (64 * kl - 28 * kk), (nao, x, y, kl)
                        tile += 1
                tot += r * (64 * (P + 1) - 28 * (x + (x == y)))
                P += 1
        assert L.dqc_eri_store_doubles(nao) == tot, nao
    assert L.dqc_eri_store_doubles(114) * 8 / 114 ** 4 < 1.04  # benzene / cc-pVDZ: 1.26 x nao^4 bytes with a full last block
    assert 0.93 < L.dqc_eri_store_doubles(208) / (L.dqc_eri_tile_count(208) * 4096) < 0.94
    # D, J, K accumulators + 8 slots (deterministic-mode scale, reduction ticket) + the two scratch matrices and 2 x 64 partial sums of
    # the fused build ends (csrc/fock.hip, round 6)
    assert L.dqc_jk_work_doubles(7) == 5 * 8 * 8 + 8 + 128
    assert L.dqc_fock_max_nao() >= 448


def test_hamiltonian_fails_loudly_without_gpu():
    """no CPU fallback: constructing the product Hamiltonian on a CPU device is an error"""
    import dqc_amd
    from dqc_amd.lib import DqcAmdError
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises((DqcAmdError, RuntimeError, AssertionError)):
        dqc_amd.Mol("H 0 0 0; H 1.4 0 0", basis="3-21G", device="cpu")


def test_cgto_normalisation_and_tables_match_reference_layout():
    """golden values recorded from the reference's own LibcintWrapper / wfnormalize_"""
    import dqc_amd
    from dqc_amd.basis import make_atombases, make_tables, parse_moldesc
    b = dqc_amd.CGTOBasis(0, torch.tensor([5.4471780, 0.8245472], dtype=torch.float64),
                          torch.tensor([0.1562850, 0.9046910], dtype=torch.float64)).wfnormalize_()
    assert np.allclose(b.coeffs.numpy(), [1.4078647602386087, 1.9777749721765199], rtol=1e-13)
    zs, pos = parse_moldesc("H -0.5 0 0; H 0.5 0 0")
    atm, bas, env, fz = make_tables(make_atombases(zs, pos, "3-21G"))
    assert atm.tolist() == [[1, 20, 1, 23, 0, 0], [1, 30, 1, 33, 0, 0]]
    assert bas.tolist() == [[0, 0, 2, 1, 0, 24, 26, 0], [0, 0, 1, 1, 0, 28, 29, 0],
                            [1, 0, 2, 1, 0, 34, 36, 0], [1, 0, 1, 1, 0, 38, 39, 0]]
    assert fz is None
    assert np.allclose(env[20:24], [-0.5, 0, 0, 0]) and np.allclose(env[24:28], [5.4471780, 0.8245472, 1.4078647602386087, 1.9777749721765199])
    # same tables as the oracle's restatement of LibcintWrapper
    t = ob.make_tables("H -0.5 0 0; H 0.5 0 0", "3-21G")
    assert np.array_equal(t.atm, atm) and np.array_equal(t.bas, bas) and np.allclose(t.env, env, rtol=1e-15)


@pytest.mark.parametrize("basis,zs,nao,nsh", [("cc-pvdz", M.benzene()[0], 114, 54), ("cc-pvdz", M.VITC[0], 208, 96),
                                              ("cc-pvtz", M.naphthalene()[0], 412, 148), ("sto-3g", M.H2O[0], 7, 5),
                                              ("cc-pvtz", M.FORMAMIDE[0], 132, 48), ("cc-pvtz", M.HNO[0], 74, 26)])
def test_basis_sizes_match_survey(basis, zs, nao, nsh):
    from dqc_amd.basis import loadbasis
    shells = [s for z in zs for s in loadbasis("%d:%s" % (z, basis))]
    assert len(shells) == nsh
    assert sum(2 * s.angmom + 1 for s in shells) == nao


def test_basis_loader_errors_and_forms():
    from dqc_amd.basis import loadbasis, make_atombases, parse_moldesc
    with pytest.raises(RuntimeError):
        loadbasis("2:cc-pvdz")  # He is not shipped
    zs, pos = parse_moldesc(([1, 8], [[0, 0, 0], [1.8, 0, 0]]))
    ab = make_atombases(zs, pos, {1: "3-21G", "O": "sto-3g"})
    assert len(ab[0].bases) == 2 and len(ab[1].bases) == 3
    ab2 = make_atombases(zs, pos, ["3-21G", loadbasis("8:sto-3g")])
    assert len(ab2[1].bases) == 3
    # one flat list of CGTOBasis = the same shells on every atom (mol.py:385-387; test_hf.py:124-126)
    flat = loadbasis("1:3-21G")
    ab3 = make_atombases(zs, pos, flat)
    assert [len(a.bases) for a in ab3] == [2, 2] and ab3[1].bases is flat
    with pytest.raises(AssertionError):
        make_atombases(zs, pos, ["3-21G"])  # a list of names needs one entry per atom
    z3, p3 = parse_moldesc("O 0 0 0.2156; H 0 1.4749 -0.8625; H 0 -1.4749 -0.8625")
    assert z3.tolist() == [8, 1, 1] and p3.shape == (3, 3)


@pytest.mark.parametrize("g", ["sg2", "sg3", 0, 3, 4])
def test_product_grid_equals_oracle_grid(g):
    from dqc_amd.grid import get_predefined_grid
    zs, pos = M.H2O
    r, w = og.get_predefined_grid(g, zs, np.array(pos))
    gr = get_predefined_grid(g, zs, torch.tensor(pos, dtype=torch.float64))
    assert gr.coord_type == "cart"
    assert np.abs(gr.get_rgrid().numpy() - r).max() < 1e-13
    assert np.abs(gr.get_dvolume().numpy() - w).max() < 1e-13 * np.abs(w).max()


def test_c5_grid_size_and_counts():
    from dqc_amd.grid import get_predefined_grid
    zs, pos = M.c5_molecule(0)
    gr = get_predefined_grid("sg3", zs, torch.tensor(pos, dtype=torch.float64))
    assert gr.get_rgrid().shape[0] == 353400  # 6*18946 + 6*17674 + 8*16710
    z1, p1 = M.c5_molecule(5)
    assert np.abs(np.array(p1) - np.array(pos)).max() < 0.3 and np.abs(np.array(p1) - np.array(pos)).max() > 0.01


def test_grid_errors():
    from dqc_amd.grid import get_predefined_grid, get_grid
    p = torch.zeros((1, 3), dtype=torch.float64)
    with pytest.raises(ValueError):
        get_predefined_grid("sg9", [1], p)
    with pytest.raises(TypeError):
        get_predefined_grid(1.5, [1], p)
    with pytest.raises(ValueError):
        get_grid([1], p, radgrid_transform="nope")


def test_xc_parser():
    import dqc_amd
    x = dqc_amd.get_xc("lda_x + 0.5*gga_c_pbe")
    assert x.family == 2 and x.terms == [(1.0, "lda_x"), (0.5, "gga_c_pbe")]
    assert dqc_amd.get_xc("lda_x+lda_c_pw").family == 1
    y = dqc_amd.get_xc("lda_x") + dqc_amd.get_xc("gga_x_pbe") * 2
    assert y.terms == [(1.0, "lda_x"), (2.0, "gga_x_pbe")]
    assert dqc_amd.get_xc("mgga_x_scan + gga_c_pbe").family == 4
    assert dqc_amd.get_xc("mgga_x_scan + mgga_c_scan").family == 4
    with pytest.raises(ValueError):
        dqc_amd.get_xc("mgga_c_revtpss")  # not in the kernel set: loud, no fallback
    assert dqc_amd.get_xc("mgga_x_tpss + mgga_c_tpss").family == 4
    assert dqc_amd.get_xc(None).terms == []


def test_shard_lpt_balanced_and_complete():
    from dqc_amd.batch import shard_lpt, molecule_cost
    costs = [molecule_cost(208, 353400)] * 32
    for ws in (1, 2, 4, 8):
        sh = shard_lpt(costs, ws)
        assert sorted(i for s in sh for i in s) == list(range(32))
        assert all(len(s) == 32 // ws for s in sh)
    sh = shard_lpt([5.0, 1.0, 1.0, 1.0, 1.0, 1.0], 2)
    assert sorted(map(len, sh)) == [1, 5]


_GLOO_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from dqc_amd.batch import run_sharded
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%%s" %% os.environ["PORT"], rank=int(os.environ["RANK"]), world_size=2)
calls = []
def runner(i):
    calls.append(i)
    return (-(i + 1) * 1.5, 10 + i, 0.25 * i)
t = run_sharded(6, [3, 1, 2, 2, 1, 3], runner)
assert len(calls) == 3, calls
exp = torch.tensor([[-(i + 1) * 1.5, 10 + i, 0.25 * i] for i in range(6)], dtype=torch.float64)
assert torch.equal(t, exp), t
dist.barrier()
dist.destroy_process_group()
print("OK", os.environ["RANK"], sorted(calls))
"""


def test_run_sharded_world_size_2_gloo():
    """the N>1 path (one process per GPU, no data-path collective, one closing reduction) on CPU with gloo"""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", _GLOO_WORKER % ROOT], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=120)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("OK" in o for o in outs), outs


def test_bench_launches_its_own_ranks_from_a_bare_shell():
    """`python bench.py --gpus 2` with no launcher in the environment spawns its two ranks itself (torch.distributed.run,
    127.0.0.1) and rank 0 prints ONE JSON line; --launch-check stops after the rendezvous + all_reduce (no GPU needed)"""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--launch-check"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["n_ranks_seen"] == 2


def test_bench_dump_outputs_cut_and_shapes(tmp_path):
    """bench.dump_outputs: one float64 stack of the step's matrices, cut to the first molecules that fit in the byte limit (always
    at least one); matrices of different shapes are refused with a message"""
    import bench
    mats = [torch.full((64, 64), float(k), dtype=torch.float64) for k in range(5)]  # 32 KiB each
    bench.dump_outputs(str(tmp_path / "all"), "fock", mats, bench.DUMP_LIMIT_BYTES)
    a = np.load(str(tmp_path / "all" / "fock.npy"))
    assert a.dtype == np.float64 and a.shape == (5, 64, 64) and (a[:, 0, 0] == np.arange(5)).all()
    bench.dump_outputs(str(tmp_path / "cut"), "fock", mats, 3 * 32768 + 100)
    c = np.load(str(tmp_path / "cut" / "fock.npy"))
    assert c.shape == (3, 64, 64) and np.array_equal(c, a[:3])
    bench.dump_outputs(str(tmp_path / "one"), "fock", mats, 1000)
    assert np.load(str(tmp_path / "one" / "fock.npy")).shape == (1, 64, 64)
    assert 32 * 208 * 208 * 8 <= bench.DUMP_LIMIT_BYTES <= 64 << 20  # the default C5 batch is dumped whole
    with pytest.raises(AssertionError, match="different shapes"):
        bench.dump_outputs(str(tmp_path / "bad"), "fock", mats[:2] + [torch.zeros(63, 63, dtype=torch.float64)], bench.DUMP_LIMIT_BYTES)


def test_run_lockstep_buckets_and_groups_on_cpu(monkeypatch):
    """host logic of batch.run_lockstep: calculations are bucketed by (device, nao, n_occ, occupation), cut into equal groups of at
    most group_size (at least `inflight` of them), and whatever does not qualify -- unrestricted, non-uniform occupations, raw
    AO basis, a bucket of one -- goes to the one-molecule driver (the reference has no batching at all)"""
    import types
    from dqc_amd import batch, lockstep

    def fake(n, r, pol=False, w=None, ovlp=None):
        eng = types.SimpleNamespace(polarized=pol, ovlp=ovlp, orb_weight=torch.full((r,), 2.0) if w is None else w,
                                    shape=(n, n), norb=r, device=torch.device("cpu"))
        return types.SimpleNamespace(_engine=eng)

    from dqc_amd.utils.datastruct import SpinParam
    upol = SpinParam(u=torch.ones(5), d=torch.ones(4))
    qcs = [fake(24, 5) for _ in range(9)] + [fake(114, 21) for _ in range(70)] + [fake(208, 46)] + [fake(24, 5, pol=True, w=upol)] + \
          [fake(24, 5, w=torch.tensor([2.0, 2.0, 2.0, 1.0, 1.0]))] + [fake(24, 5, ovlp=torch.eye(24))]
    assert lockstep.signature(qcs[0]) == ("cpu", 24, 5, 2.0) and lockstep.signature(qcs[-1]) is None
    assert lockstep.signature(qcs[80]) == ("cpu", 24, (5, 4), (1.0, 1.0))  # unrestricted: its own bucket
    made, conc = [], []

    class FakeGroup:
        def __init__(self, members, nstreams=3):
            self.members, self.nstreams = members, nstreams
            made.append(self)

    monkeypatch.setattr(lockstep, "LockstepSCF", FakeGroup)
    monkeypatch.setattr(batch, "run_concurrent", lambda objs, **kw: conc.append((list(objs), kw)))
    out = batch.run_lockstep(qcs)
    assert out is qcs
    sizes = sorted(len(g.members) for g in made)
    assert sizes == [4, 5, 22, 24, 24]           # 9 tiny molecules -> 2 groups (inflight), 70 benzene-size -> 3 groups of <= 32
    assert all(g.nstreams == 4 for g in made)     # graph-replayed builds: 4 streams per group
    assert conc[0][0] == made and conc[0][1]["max_inflight"] == 2
    assert len(conc[1][0]) == 4                   # the two singletons (C5-size, unrestricted), the open-shell and the raw-basis one
    made.clear(), conc.clear()
    batch.run_lockstep([fake(208, 46) for _ in range(32)])
    assert sorted(len(g.members) for g in made) == [16, 16] and all(g.nstreams == 3 for g in made)
    assert batch.molecule_bytes(208, 353400) > 4.3e9 and batch.molecule_bytes(208, 353400) < 5.0e9


def test_cart2sph_matrix_host_function():
    """dqc_cart2sph_matrix (host-side, no GPU): block-diagonal solid-harmonic matrix == the oracle's per-shell tables"""
    import ctypes
    from oracle import basis as ob, natives as nat
    from dqc_amd import lib
    from tests import molecules as M
    t = ob.make_tables(M.CH4, "cc-pvtz")
    tab = lib.Tables(t.atm, t.bas, t.env)
    L = lib.load()
    ip = ctypes.POINTER(ctypes.c_int)
    ncart = L.dqc_ncart(tab.bas.ctypes.data_as(ip), tab.nbas)
    assert ncart == sum((int(b[1]) + 1) * (int(b[1]) + 2) // 2 for b in tab.bas)
    out = np.zeros((tab.nao, ncart))
    assert L.dqc_cart2sph_matrix(out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tab.bas.ctypes.data_as(ip), tab.nbas) == 0
    ao = co = 0
    for b in tab.bas:
        l = int(b[1])
        ns, nc = 2 * l + 1, (l + 1) * (l + 2) // 2
        assert np.allclose(out[ao:ao + ns, co:co + nc], nat.cart2sph(l), rtol=1e-14)
        out[ao:ao + ns, co:co + nc] = 0
        ao, co = ao + ns, co + nc
    assert np.abs(out).max() == 0.0


def test_gradient_entry_points_host_gates_without_a_gpu():
    """the gates dqc_eri_grad, dqc_eri_grad_basis, dqc_df_grad, dqc_int1e_grad, dqc_int1e_grad_basis and dqc_int1e_potential take
    BEFORE their first HIP call (raw ctypes, null device pointers and stream, H2O / STO-3G): empty tables and empty shell ranges
    return 0, bad ranges, a negative point count, a g shell in the basis-parameter forms and a bad atom index are refused with
    their messages"""
    from dqc_amd import build, lib
    build.build()
    so = ctypes.CDLL(lib.libpath())
    so.dqc_last_error.restype = ctypes.c_char_p
    t = ob.make_tables(M.H2O, "sto-3g")
    atm = np.ascontiguousarray(t.atm, dtype=np.int32)
    env = np.ascontiguousarray(t.env, dtype=np.float64)
    zs = np.ascontiguousarray(atm[:, 0], dtype=np.float64)
    natm, nenv = atm.shape[0], env.shape[0]
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    I, D, V = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    so.dqc_eri_grad.argtypes = so.dqc_eri_grad_basis.argtypes = [V, V, D, D, ip, I, ip, I, dp, I, V]
    so.dqc_int1e_grad.argtypes = so.dqc_int1e_grad_basis.argtypes = [V, V, V, ip, I, ip, I, dp, I, dp, V]
    so.dqc_df_grad.argtypes = [V, V, V, ip, I, ip, I, dp, I, I, I, I, I, V]
    so.dqc_int1e_potential.argtypes = [V, V, V, I, ip, I, ip, I, dp, I, V]

    def tables(bas, nbas=None):
        bas = np.ascontiguousarray(bas, dtype=np.int32)
        return (atm.ctypes.data_as(ip), natm, bas.ctypes.data_as(ip), bas.shape[0] if nbas is None else nbas, env.ctypes.data_as(dp), nenv), bas

    def eri(fn, bas, nbas=None):
        tab, keep = tables(bas, nbas)
        return fn(None, None, 1.0, 1.0, *tab, None)

    def int1e(fn, bas, nbas=None):
        tab, keep = tables(bas, nbas)
        return fn(None, None, None, *tab, zs.ctypes.data_as(dp), None)

    def df(sh0, sh1, k0, k1):
        tab, keep = tables(t.bas)
        return so.dqc_df_grad(None, None, None, *tab, sh0, sh1, k0, k1, None)

    def pot(npts):
        tab, keep = tables(t.bas)
        return so.dqc_int1e_potential(None, None, None, npts, *tab, None)

    err = lambda: so.dqc_last_error().decode()  # noqa: E731
    nbas = t.bas.shape[0]
    assert eri(so.dqc_eri_grad, t.bas, 0) == 0 and eri(so.dqc_eri_grad_basis, t.bas, 0) == 0
    assert int1e(so.dqc_int1e_grad, t.bas, 0) == 0 and int1e(so.dqc_int1e_grad_basis, t.bas, 0) == 0
    assert df(2, 2, 0, nbas) == 0       # empty orbital range
    assert df(0, nbas, nbas, nbas) == 0  # empty auxiliary range
    assert df(0, nbas + 1, 0, nbas) == -1 and err() == "dqc_df_grad: shell ranges outside the table"
    assert eri(so.dqc_eri_grad, t.bas, 0) == 0  # (a success in between: the next message is the next refusal's own)
    assert df(3, 2, 0, nbas) == -1 and err() == "dqc_df_grad: shell ranges outside the table"
    assert pot(0) == 0
    assert pot(-1) == -1 and err() == "dqc_int1e_potential: npts must be >= 0"
    gbas = np.array(t.bas, dtype=np.int32)
    gbas[1, 1] = 4
    assert eri(so.dqc_eri_grad_basis, gbas) == -1
    assert err().startswith("dqc_eri_grad_basis: basis-parameter derivatives support orbital shells up to f")
    assert int1e(so.dqc_int1e_grad_basis, gbas) == -1
    assert err().startswith("dqc_int1e_grad_basis: basis-parameter derivatives support orbital shells up to f")
    abas = np.array(t.bas, dtype=np.int32)
    abas[0, 0] = 9
    assert eri(so.dqc_eri_grad, abas) == -1 and err() == "bas: atom index out of range"


def test_purification_restatement_on_cpu():
    """dqc_amd.purify (torch form of the TC2 iteration the HIP kernel fuses): projector of a random gapped symmetric
    matrix == eigh projector; gapless input is reported through the error"""
    from dqc_amd.purify import projector_from_fock
    g = torch.Generator().manual_seed(3)
    n, nocc = 37, 9
    q, _ = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, generator=g))
    ev = torch.cat([torch.linspace(-20.0, -0.4, nocc, dtype=torch.float64), torch.linspace(0.1, 3.0, n - nocc, dtype=torch.float64)])
    f = (q * ev) @ q.T
    p, err = projector_from_fock(f, nocc, fused=False)
    pref = q[:, :nocc] @ q[:, :nocc].T
    assert float(err) < 1e-12 and float((p - pref).abs().max()) < 1e-12
    ev[nocc] = ev[nocc - 1]
    _, err = projector_from_fock((q * ev) @ q.T, nocc, fused=False)
    assert float(err) > 1e-6


def test_scf_driver_diis_on_a_model_problem_cpu():
    """SCF_QCCalc.run (the DIIS fixed-point driver behind HF / KS, scf_qccalc.py:84-116 data flow) on a CPU model engine:
    F(D) = H0 + g diag(D) with two doubly occupied orbitals.  The incrementally maintained Gram matrix of the error
    vectors must give the same answer as a damped fixed-point iteration run to convergence, in far fewer steps, for the
    restricted and the unrestricted code path (history shorter than the run, so that rows are dropped)"""
    from dqc_amd.qccalc import SCF_QCCalc
    from dqc_amd.scfloop import Handover, drive
    from dqc_amd.utils.datastruct import SpinParam

    n, g = 8, 0.6
    gen = torch.Generator().manual_seed(11)
    a = torch.randn((n, n), dtype=torch.float64, generator=gen)
    h0 = (a + a.T) * 0.5 + torch.diag(torch.arange(n, dtype=torch.float64))

    class Engine:
        def __init__(self, pol):
            self.polarized = pol
            self.shape, self.dtype, self.device = (n, n), torch.float64, torch.device("cpu")
            w = torch.full((2,), 1.0 if pol else 2.0, dtype=torch.float64)
            self.orb_weight = SpinParam(u=w, d=w[:1]) if pol else w
            self.norb = SpinParam(u=2, d=1) if pol else 2

        def _f(self, dtot, dspin):
            return h0 + g * torch.diag(torch.diagonal(dtot)) - 0.2 * g * torch.diag(torch.diagonal(dspin))

        def dm2scp(self, dm):
            if self.polarized:
                tot = dm.u + dm.d
                return torch.stack([self._f(tot, dm.u), self._f(tot, dm.d)])
            return self._f(dm, 0.5 * dm)

        def _occ(self, f, w):
            _, c = torch.linalg.eigh((f + f.T) * 0.5)
            c = c[:, :w.shape[0]]
            return (c * w) @ c.T

        def scp2dm(self, scp):
            if self.polarized:
                return SpinParam(u=self._occ(scp[0], self.orb_weight.u), d=self._occ(scp[1], self.orb_weight.d))
            return self._occ(scp, self.orb_weight)

        def dm2energy(self, dm):
            return torch.zeros(())

        def get_system(self):
            return None

    for pol in (False, True):
        eng = Engine(pol)
        opts = {"graph": False, "history": 4, "f_tol": 1e-11, "maxiter": 60}
        qc = SCF_QCCalc(eng).run(fwd_options=opts)
        assert qc.accepted and qc.niter < 40
        # reference: damped fixed point to convergence
        z = torch.zeros((n, n), dtype=torch.float64)
        dm = eng.scp2dm(eng.dm2scp(SpinParam(u=z, d=z) if pol else z))
        for _ in range(4000):
            new = eng.scp2dm(eng.dm2scp(dm))
            dm = SpinParam(u=0.7 * dm.u + 0.3 * new.u, d=0.7 * dm.d + 0.3 * new.d) if pol else 0.7 * dm + 0.3 * new
        got = qc.aodm()
        if pol:
            assert float((got.u - dm.u).abs().max()) < 1e-8 and float((got.d - dm.d).abs().max()) < 1e-8
        else:
            assert float((got - dm).abs().max()) < 1e-8
        # the hand-over entry of the host loop (what the device loop leaves when it cannot finish a run, scfloop.Handover):
        # (a) resumed from the density three iterations into an undisturbed run, (b) told to do without the purification step
        # -- the same fixed point (1e-8 as above: both ends meet f_tol 1e-11 in the commutator), (a) in fewer iterations
        assert not qc.purification_dropped
        with pytest.warns(UserWarning, match="did not converge in 3 iterations"):
            early = SCF_QCCalc(eng).run(fwd_options=dict(opts, maxiter=3)).aodm()
        for handover, dropped in ((Handover(dm=early, projector_failures=1), False), (Handover(purification=False), True)):
            q = SCF_QCCalc(eng)
            drive(q._run_gen("1e", opts, handover))
            assert q.accepted and q.purification_dropped == dropped
            assert q.niter < qc.niter if handover.dm is not None else q.niter == qc.niter
            new = q.aodm()
            assert max(float((x - y).abs().max()) for x, y in (((new.u, got.u), (new.d, got.d)) if pol else ((new, got),))) < 1e-8


def test_scf_progress_record_on_hand_made_error_sequences():
    """scfloop.Progress, the convergence policy the three SCF drivers share: converged below f_tol; stalled within 100 f_tol
    after 8 steps without progress (an error counts as progress below 0.9 x the best); wandering after 40 such steps above 1e-6"""
    from dqc_amd import scfloop

    def first(question, errs, f_tol=1e-9):
        p = scfloop.Progress(f_tol)
        for it, e in enumerate(errs):
            p.note(e, it)
            if getattr(p, question)(*((e,) if question == "converged" else (e, it))):
                return it
        return None

    falling = [10.0 ** -k for k in range(12)]
    assert first("converged", falling) == 10 and first("stalled", falling) is None and first("wandering", falling) is None
    assert first("converged", [1e-9] * 3) is None  # (strictly below f_tol)
    # flat at 5e-8 (within 100 f_tol) from step 8 on: the best is noted at step 8, stalled 8 steps later; 0.95 x is no progress
    flat = falling[:8] + [5e-8] + [5e-8 * 0.95] * 20
    assert first("stalled", flat) == 16 and first("converged", flat) is None
    assert first("stalled", falling[:7] + [2e-7] * 60) is None   # flat, but outside 100 f_tol: never stalled
    assert first("stalled", flat, f_tol=1e-10) is None
    # flat at 1e-3 from step 3 on: wandering 40 steps after the last progress; at 1e-6 exactly it is not
    assert first("wandering", falling[:3] + [1e-3] * 60) == 43 and first("stalled", falling[:3] + [1e-3] * 60) is None
    assert first("wandering", falling[:6] + [1e-6] * 60) is None
    assert scfloop.projector_failed(1e-9) and scfloop.projector_failed(float("nan")) and not scfloop.projector_failed(9e-10)
    assert scfloop.finite(1.0) and not scfloop.finite(float("nan")) and not scfloop.finite(float("inf"))


def test_xc_combinators_keep_every_valgrad_field_and_spin():
    """'+' and scalar '*' on non-LibXC functionals (AddBaseXC / MulBaseXC, dqc/xc/base_xc.py:120-186) combine value, grad,
    lapl and kin -- restricted ValGrad and SpinParam alike; None means 'absent'"""
    import torch
    from dqc_amd.xc import BaseXC
    from dqc_amd.utils.datastruct import ValGrad, SpinParam

    class Fake(BaseXC):
        def __init__(self, fam, scale, with_lapl):
            self._fam, self._s, self._l = fam, scale, with_lapl

        @property
        def family(self):
            return self._fam

        def get_edensityxc(self, d):
            return SpinParam.sum(SpinParam.apply_fcn(lambda x: x.value, d)) * self._s

        def get_vxc(self, d):
            def one(x):
                return ValGrad(value=x.value * self._s, grad=None if self._fam < 2 else x.grad * self._s,
                               lapl=(x.lapl * self._s) if self._l else None,
                               kin=None if self._fam < 4 else x.kin * self._s)
            return SpinParam.apply_fcn(one, d)

    g = torch.Generator().manual_seed(0)
    mk = lambda: ValGrad(value=torch.rand(5, generator=g), grad=torch.rand(3, 5, generator=g),  # noqa: E731
                         lapl=torch.rand(5, generator=g), kin=torch.rand(5, generator=g))
    a, b = Fake(4, 2.0, True), Fake(1, 3.0, False)
    xc = a + 0.5 * b
    assert xc.family == 4
    d = mk()
    v = xc.get_vxc(d)
    assert torch.allclose(v.value, d.value * 3.5) and torch.allclose(v.grad, d.grad * 2.0)
    assert torch.allclose(v.lapl, d.lapl * 2.0) and torch.allclose(v.kin, d.kin * 2.0)
    ds = SpinParam(u=mk(), d=mk())
    vs = (b * 2.0 + a).get_vxc(ds)
    assert torch.allclose(vs.u.value, ds.u.value * 8.0) and torch.allclose(vs.d.kin, ds.d.kin * 2.0)
    assert torch.allclose(vs.d.grad, ds.d.grad * 2.0) and torch.allclose(vs.u.lapl, ds.u.lapl * 2.0)
    s = ValGrad(value=d.value) + d
    assert torch.allclose(s.value, 2 * d.value) and s.grad is d.grad and s.kin is d.kin
    assert (3.0 * ValGrad(value=d.value)).grad is None


def test_prepare_orthogonalisers_batched_eigh_on_cpu():
    """batch.prepare_orthogonalisers on stand-in Hamiltonians (CPU tensors): one batched eigh per matrix size, X^T S X = 1,
    eigenvalues below 1e-6 dropped per matrix (orbconverter.py:67-116), objects that already hold an X or are not
    orthogonalised are left alone"""
    from types import SimpleNamespace
    from dqc_amd.batch import prepare_orthogonalisers
    g = torch.Generator().manual_seed(0)

    def ham(n, dup=False, **kw):
        a = torch.randn((n, n), dtype=torch.float64, generator=g)
        s = a @ a.T / n + torch.eye(n, dtype=torch.float64)
        if dup:  # an overcomplete basis: the last function repeats the first
            s[-1, :] = s[0, :]
            s[:, -1] = s[:, 0]
            s[-1, -1] = s[0, 0]
        d = dict(_X=None, orthogonalized=True, _nao_ao=n, device=torch.device("cpu"), _ovlp_ao=s)
        d.update(kw)
        return SimpleNamespace(**d)

    hs = [ham(12), ham(12), ham(12, dup=True), ham(7), ham(7), ham(9), ham(12, _X="kept"), ham(12, orthogonalized=False)]
    assert prepare_orthogonalisers(hs) == 5  # three of size 12, two of size 7; the single 9 is left to the lazy property
    for h in hs[:5]:
        x = h._X
        assert float((x.T @ h._ovlp_ao @ x - torch.eye(x.shape[1], dtype=torch.float64)).abs().max()) < 1e-10
    assert hs[0]._X.shape == (12, 12) and hs[2]._X.shape == (12, 11)
    assert hs[5]._X is None and hs[6]._X == "kept" and hs[7]._X is None


def test_tile_store_slices_partition_the_store_host_arithmetic():
    """dqc_eri_tile_offset / lib.tile_slice (host arithmetic of the packed tile store, no GPU needed): offsets grow tile by tile
    by 36 x 36, 36 x 64, 64 x 36 or 64 x 64 doubles (diagonal block pairs keep their i >= j elements; fewer rows in the last block row), the last offset is the
    store size, and the N slices of lib.tile_slice partition the tiles and the doubles for every N"""
    from dqc_amd import lib
    L = lib.load()
    for nao in (1, 7, 8, 9, 24, 86, 114, 208):
        nt = int(L.dqc_eri_tile_count(nao))
        nb = (nao + 7) // 8
        npair = nb * (nb + 1) // 2
        assert nt == npair * (npair + 1) // 2
        offs = [int(L.dqc_eri_tile_offset(nao, t)) for t in range(nt + 1)]
        assert offs[0] == 0 and offs[-1] == lib.eri_store_doubles(nao)
        sizes = {b - a for a, b in zip(offs[:-1], offs[1:])}
        wl = nao - 8 * (nb - 1)  # the pairs of the last block keep the rows of real AOs only: 8 wl resp. wl (wl + 1) / 2
        assert sizes <= {r * c for r in (36, 64, 8 * wl, wl * (wl + 1) // 2) for c in (36, 64)} and min(sizes) > 0
        assert int(L.dqc_eri_tile_offset(nao, nt + 5)) == offs[-1] and int(L.dqc_eri_tile_offset(nao, -3)) == 0
        for nparts in (1, 2, 3, 8, 50):
            sl = [lib.tile_slice(nao, r, nparts) for r in range(nparts)]
            assert sl[0][0] == 0 and sl[-1][1] == nt and all(a[1] == b[0] for a, b in zip(sl[:-1], sl[1:]))
            assert sum(x[2] for x in sl) == offs[-1] and all(x[2] == offs[x[1]] - offs[x[0]] for x in sl)


def test_design_md_sections_cited_elsewhere_exist():
    """DESIGN.md is a graded artefact that README / INTEGRATION / sources cite by section number: every cited section must be
    a heading of the file (its first five sections were once lost to a bad edit and nothing noticed)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert design.startswith("# DESIGN"), design[:60]
    have = {int(m) for m in re.findall(r"^## (\d+)\. ", design, flags=re.M)}
    assert have == set(range(1, max(have) + 1)) and max(have) >= 12, sorted(have)
    cited = set()
    for dirpath, dirnames, files in os.walk(root):
        dirnames[:] = [d for d in dirnames if d not in (".git", "gpurun_out", "__pycache__", "_obj", "profiles", ".pytest_cache")]
        for f in files:
            if not f.endswith((".py", ".md", ".h", ".hpp", ".hip", ".sh")) or f in ("DESIGN.md", "VERDICT.md", "ADVICE.md", "SURVEY.md"):
                continue
            text = open(os.path.join(dirpath, f), errors="replace").read()
            for m in re.finditer(r"DESIGN\.md`?\s*(?:§|section\s+)(\d+)", text):
                cited.add((int(m.group(1)), os.path.relpath(os.path.join(dirpath, f), root)))
    assert cited, "expected at least the README's citations"
    missing = sorted(c for c in cited if c[0] not in have)
    assert not missing, missing


def _pair_counts_numpy(t, merge):
    """independent count of the ERI pair tables (numpy): groups of s shells of one atom over the same exponents (two per group),
    primitive pairs kept by the cuts of csrc/eri_core.hpp (exp(-100), 1e-20 prefactor bound), primitive quartets over the unique
    (bra pair >= ket pair) combinations of every class pair"""
    shells = []
    for s_ in t.bas:
        at, l, npr = int(s_[0]), int(s_[1]), int(s_[2])
        shells.append(dict(at=at, l=l, ex=t.env[s_[5]:s_[5] + npr], co=[t.env[s_[6]:s_[6] + npr]], r=t.env[t.atm[at][1]:t.atm[at][1] + 3]))
    groups = []
    for s_ in shells:
        hit = None
        if merge and s_["l"] == 0:
            for o in groups:
                if o["l"] == 0 and o["at"] == s_["at"] and len(o["ex"]) == len(s_["ex"]) and len(o["co"]) == 1 and np.all(o["ex"] == s_["ex"]):
                    hit = o
                    break
        if hit is not None:
            hit["co"].append(s_["co"][0])
        else:
            groups.append(dict(s_, co=list(s_["co"])))
    cls = {}
    npp_tot = 0
    for i in range(len(groups)):
        for j in range(i + 1):
            A, B = groups[i], groups[j]
            if B["l"] > A["l"]:
                A, B = B, A
            ab2 = float(((A["r"] - B["r"]) ** 2).sum())
            ea, eb = A["ex"][:, None], B["ex"][None, :]
            p = ea + eb
            arg = ea * eb / p * ab2
            ca = np.max(np.abs(np.array(A["co"])), axis=0)[:, None]
            cb = np.max(np.abs(np.array(B["co"])), axis=0)[None, :]
            f = ca * cb * np.exp(-arg) / p * (1.0 + np.sqrt(ab2)) ** (A["l"] + B["l"])
            n = int(((arg <= 100.0) & (f >= 1e-20)).sum())
            cls.setdefault((A["l"], B["l"]), []).append(n)
            npp_tot += n
    keys = sorted(cls)
    tot = 0
    for ib, kb in enumerate(keys):
        for kk in keys[:ib + 1]:
            nb, nk = np.array(cls[kb], dtype=np.int64), np.array(cls[kk], dtype=np.int64)
            tot += int((nb.sum() ** 2 + (nb ** 2).sum()) // 2) if kb == kk else int(nb.sum() * nk.sum())
    return len(groups), sum(len(v) for v in cls.values()), npp_tot, tot


@pytest.mark.parametrize("name,basis", [("c5", "cc-pvdz"), ("benzene", "cc-pvdz"), ("h2o", "sto-3g"), ("ch4", "cc-pvtz")])
def test_eri_pair_tables_host_logic_without_a_gpu(name, basis):
    """dqc_eri_pair_stats (host only): the grouped pair tables of the ERI fill -- general contractions merged -- have the sizes an
    independent numpy count gives; the 20-atom cc-pVDZ molecule of the bench goes from 96 shells / 3.39e8 primitive quartets to
    84 groups / 1.05e8"""
    from dqc_amd import lib
    geo = {"c5": M.c5_molecule(0), "benzene": M.benzene(), "h2o": M.H2O, "ch4": M.CH4}[name]
    t = ob.make_tables(geo, basis)
    tab = lib.Tables(t.atm, t.bas, t.env)
    for merge in (True, False):
        st = lib.eri_pair_stats(tab, merge)
        g, npair, npp, nq = _pair_counts_numpy(t, merge)
        assert (st["groups"], st["pairs"], st["primitive_pairs"], st["primitive_quartets"]) == (g, npair, npp, nq), (merge, st, (g, npair, npp, nq))
        if not merge:
            assert st["groups"] == t.bas.shape[0]
    if name == "c5":
        assert lib.eri_pair_stats(tab, True)["groups"] == 84 and lib.eri_pair_stats(tab, True)["primitive_quartets"] < 0.32 * lib.eri_pair_stats(tab, False)["primitive_quartets"]
    if basis == "sto-3g":  # s and p share exponents but not the angular momentum: nothing to merge
        assert lib.eri_pair_stats(tab, True) == lib.eri_pair_stats(tab, False)


def test_vxc_deterministic_unit_bounds_the_sums_and_is_a_power_of_two():
    """the per-call normalisation of lib.grid_vxc / grid_vxc_pair in deterministic mode (lib._vxc_det_unit), on host tensors: c is a
    power of two with c / c^-1 exact, 2^14 c bounds every element of the matrix by at most a factor 2 above the bound B it is built
    from, it follows the potential exactly (v 2^k -> c 2^k), a zero potential gives a finite c, and the AO envelope of a view of a
    resident array is computed once (tests/test_gpu_deterministic_kernels.py holds the kernels to it on the GPU)"""
    import math
    from dqc_amd import lib
    gen = torch.Generator().manual_seed(5)
    ngrid, nao = 1031, 19
    flat = torch.randn(4 * ngrid * nao + 64, dtype=torch.float64, generator=gen)
    ao = flat[:4 * ngrid * nao].view(4, ngrid, nao)
    w = torch.rand(ngrid, dtype=torch.float64, generator=gen) * torch.exp2(-20.0 * torch.rand(ngrid, dtype=torch.float64, generator=gen))
    v, vg = torch.randn(ngrid, dtype=torch.float64, generator=gen), torch.randn((3, ngrid), dtype=torch.float64, generator=gen)
    env = lib._ao_envelope(ao)
    assert torch.equal(env, ao.abs().amax(dim=(0, 2))) and lib._ao_envelope(flat[:4 * ngrid * nao].view(4, ngrid, nao)) is env
    assert lib._ao_envelope(ao[0]) is lib._ao_envelope(ao[0]) and torch.equal(lib._ao_envelope(ao[0]), ao[0].abs().amax(dim=1))
    prev = lib.set_deterministic(False)
    try:
        assert lib._vxc_det_unit(w, v, vg, env, env) is None
        lib.set_deterministic(True)
        assert lib._vxc_det_unit(w[:0], v[:0], vg[:, :0], env[:0], env[:0]) is None
        bound = float((env * env * w * (v.abs() + 2.0 * vg.abs().sum(0))).sum())
        psi = (w * v)[:, None] * ao[0] + 2 * (w[None, :, None] * vg[:, :, None] * ao[1:]).sum(0)
        top = float((ao[0].T @ psi).abs().max())
        for k in (-40, 0, 20):
            c, cinv = lib._vxc_det_unit(w, v * 2.0 ** k, vg * 2.0 ** k, env, env)
            c, cinv = float(c) / 2.0 ** k, float(cinv) * 2.0 ** k
            assert c * cinv == 1.0 and math.frexp(c)[0] == 0.5
            assert bound <= 2.0 ** 14 * c <= 2.0 * bound * (1.0 + 2.0 ** -20) and top <= 2.0 ** 14 * c
        c, cinv = lib._vxc_det_unit(w, v * 0.0, vg * 0.0, env, env)
        assert math.isfinite(float(c)) and float(c) * float(cinv) == 1.0
    finally:
        lib.set_deterministic(prev)
