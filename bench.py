"""bench.py -- SCF iterations/sec (Fock build + XC grid) per GPU, cc-pVDZ 20-atom  (BASELINE.json metric).

A "step" is one pass of the hot path over the batch: for every molecule one evaluation of
engine.dm2scp(D) = J (ERI tiles -> Coulomb matrix) + density on the grid + XC functional + Vxc matrix, i.e.
exactly the per-SCF-iteration Fock build of the reference's _KSEngine (dqc/qccalc/ks.py:176-187), float64,
with the one-off setup (ERI fill, AO-on-grid, Becke grid) excluded and reported separately.  Inputs are the
C5 set of SURVEY.md 8(d): vitamin C (the reference's own 20-atom cc-pVDZ benchmark molecule,
dqc/test/benchmark.py:7-26) plus seeded 0.05-Bohr jitters, RKS PBE, grid sg3.

The workload is the north-star's 32-molecule batch: at --gpus 1 all 32 molecules (141 GB resident) run on the one
GPU; at N GPUs the SAME batch is sharded 32/N per rank (strong scaling over a fixed batch, no data-path collective --
only the closing barrier / max-reduce of the timing).  value = molecules x steps / max-over-ranks time.

Usage: python bench.py [--gpus N --steps K --warmup W --molecules M --full --dump-outputs DIR --no-cpu-baseline --profile-mode]
A plain run does only what the headline needs: setup, W warm-up steps, K timed steps (one pass over the batch each, unless
--min-seconds stretches them), the JSON line.  --full adds everything else the line used to carry: per-kernel HIP-event times
and rooflines (with their in-process ceiling probes), the other drivers and density forms, the HF / deterministic / small-batch /
direct / F-row legs, the CPU baselines and, at N > 1, the one-molecule-over-the-ranks leg; --full --profile-mode keeps
only the per-kernel times and rooflines of these (the rocprofv3 passes of tools/profile_bench.sh).  --dump-outputs DIR writes what the
last timed step returned to its caller: DIR/fock.npy, the Fock matrices of the batch (float64; DIR/fock_rank<r>.npy per rank at
N > 1).  The density matrices fed to the timed steps are made in deterministic mode, so the same arguments give the same inputs.
With --gpus N > 1 from a bare shell the script launches its own N ranks (torch.distributed.run, one per GPU, RCCL);
started under a launcher (WORLD_SIZE set) it is one of the ranks.  ONE JSON line on rank 0 either way.
"""
import argparse
import contextlib
import glob
import hashlib
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0    # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
UBENCH_READ_GBS = 6450.0  # asymptotic streaming-read rate (large buffers; profiles/r02a_read_bw_ubench.txt, r06a_hbm_ceiling_bisect.txt)
F64_MFMA_PEAK_TF = 78.6  # MI355X dense fp64 matrix peak (vendor figure; the guide lists no fp64 row)
XC = "gga_x_pbe+gga_c_pbe"


def source_sha16():
    """identity of what a profile was taken with: the kernel sources and this file"""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "dqc_amd", "csrc", "*.h*")) + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if f.endswith("rys_tables.inc"):
            continue
        h.update(open(f, "rb").read())
    return {"csrc_sha16": h.hexdigest()[:16],
            "bench_py_sha16": hashlib.sha256(open(os.path.abspath(__file__), "rb").read()).hexdigest()[:16]}


DEFAULT_J_CUS = 0  # compute units per XCD for a Coulomb-stream partition: OFF -- measured no better than ordinary streams
                   # (profiles/r06a_cu_partition_curves.txt, r06b_vxc_cus_streams_partition_sweep.txt: 714 against 726-738 it/s)
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs, all ranks together


def dump_outputs(path, name, mats, limit):
    """path/<name>.npy: the (molecules, n, n) float64 stack of the matrices one step returned, cut to the first molecules of the
    batch (whose order the arguments fix) that fit in `limit` bytes"""
    assert all(m.shape == mats[0].shape for m in mats), "--dump-outputs: Fock matrices of different shapes %s" % sorted(
        {tuple(m.shape) for m in mats})
    os.makedirs(path, exist_ok=True)
    keep = max(1, min(len(mats), limit // (mats[0].numel() * 8)))
    np.save(os.path.join(path, name + ".npy"), torch.stack(mats[:keep]).to("cpu", torch.float64).numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--molecules", type=int, default=32, help="size of the batch (whole job; sharded over the ranks)")
    ap.add_argument("--min-seconds", type=float, default=0.0,
                    help="> 0: a step is repeated `repeats` times so that the timed region of K steps lasts at least this long "
                         "(default 0: a step is one pass over the batch)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: per-kernel times and rooflines, the extra legs, the CPU baselines")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the Fock matrices the last timed step returned to DIR/fock.npy (float64)")
    ap.add_argument("--streams", type=int, default=8,
                    help="HIP streams the batch's Fock builds are dealt to (molecule k -> stream k %% S): independent molecules, so "
                         "the tail of one molecule's kernels overlaps the head of the next one's (SURVEY 8e: each rank, own streams)")
    ap.add_argument("--j-cus", type=int, default=-1,
                    help="compute units PER XCD given to the Coulomb tile stream (dqc_amd.batch.CuPartition): the grid pass of every "
                         "build runs on the other 32 - k of each XCD, the HBM-bound tile stream of the same molecule beside it; 0: no "
                         "partition (--streams ordinary streams, the rounds 2-5 form); -1: DQC_AMD_J_CUS or the shipped default")
    ap.add_argument("--grid-streams", type=int, default=2, help="with --j-cus > 0: streams (all on the grid partition) the builds are dealt to")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-one-molecule-leg", action="store_true",
                    help="N > 1: skip the leg that spreads ONE C4 molecule over the ranks (HamiltonMI355.shard_over)")
    ap.add_argument("--cpu-steps", type=int, default=5)
    ap.add_argument("--profile-mode", action="store_true",
                    help="with --full: no extra legs and no CPU work beside the per-kernel times (a plain run is leaner still)")
    ap.add_argument("--df", default=None, metavar="AUXBASIS",
                    help="density-fitted Coulomb operator (Mol.densityfit, e.g. --df etb) instead of the exact-J tile stream; "
                         "a different formulation, labelled as such in config")
    ap.add_argument("--dense-dm", action="store_true",
                    help="feed dm2scp an anonymous full density matrix (no ao_orb2dm factor): full-matrix density kernel")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL); gloo for self-tests")
    ap.add_argument("--all-ranks-on-gpu0", action="store_true",
                    help="self-test only: map every rank to cuda:0 (exercise the N>1 code path on a 1-GPU box)")
    ap.add_argument("--launch-check", action="store_true",
                    help="self-test of the N-rank launch path only (rendezvous + one all_reduce, no GPU work)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.profile_mode and not args.full:
        ap.error("--profile-mode trims a --full run: give both (a plain run already has no extra legs)")

    if args.gpus > 1 and not (args.all_ranks_on_gpu0 or args.launch_check) and torch.cuda.device_count() < args.gpus:
        # fewer devices than ranks: ONE JSON line saying so (before any rendezvous: nothing can hang) and a non-zero exit
        if int(os.environ.get("RANK", "0")) == 0:
            print(json.dumps({"error": "--gpus %d but %d device(s) visible" % (args.gpus, torch.cuda.device_count()),
                              "n_gpus": args.gpus, "devices_visible": torch.cuda.device_count()}), flush=True)
        raise SystemExit(2)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started from a bare shell (`python bench.py --gpus N`): become the launcher -- one rank per GPU under
        # torch.distributed.run, rendezvous on 127.0.0.1; rank 0 of the children prints the ONE JSON line
        raise SystemExit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (one rank per GPU)" % (args.gpus, world))
    import torch.distributed as dist
    if args.all_ranks_on_gpu0:
        local_rank = 0
    dev = None
    if not args.launch_check:
        if not args.all_ranks_on_gpu0 and torch.cuda.device_count() < world:
            raise SystemExit("bench.py: --gpus %d but only %d device(s) visible" % (world, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    n_ranks_seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
        # every rank contributes a one: the sum is the number of ranks that really joined the collective (RCCL over xGMI
        # with the nccl backend); reported in the JSON line
        ones = torch.ones(1, dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(ones)
        n_ranks_seen = int(ones.item())
    if args.launch_check:  # launcher self-test (runs without a GPU): rendezvous + collective only
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "n_ranks_seen": n_ranks_seen, "backend": args.backend}), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    import dqc_amd
    from dqc_amd import lib
    from dqc_amd.batch import shard_lpt, molecule_cost
    from tests import molecules as M

    nmol = args.molecules
    costs = [molecule_cost(208, 353400)] * nmol
    mine = shard_lpt(costs, world)[rank]
    extras = args.full and not args.profile_mode

    # ---------------- one-off setup (not timed as part of the metric) ----------------
    t0 = time.perf_counter()
    qcs, engines, dms, orbs = [], [], [], []
    brk = {}

    def lap(name, t):  # stage clock of the setup (each stage closed by a device synchronise)
        torch.cuda.synchronize()
        now = time.perf_counter()
        brk[name] = brk.get(name, 0.0) + now - t
        return now

    from dqc_amd.xc import get_xc
    from dqc_amd.batch import molecule_bytes, reserve_device_memory
    # the batch's device memory in one request (the driver clears fresh VRAM at ~35 GB/s: its own line of the breakdown)
    brk["device_memory_reserve"] = reserve_device_memory(len(mine) * molecule_bytes(208, 353400) + (4 << 30), dev)
    from dqc_amd.batch import prepare_orthogonalisers
    # once per PROCESS, like the reserve: the first call of every rocSOLVER / rocBLAS routine and the first launch of every kernel
    # family of libdqc_amd.so load their code objects (tools/gpu_cold_start.py: first eigh 0.07-0.14 s, first Cholesky 0.15-0.25 s,
    # first 20-atom molecule 0.16-0.54 s against 0.021 s for the second) -- paid here on a water molecule, its own line of the
    # breakdown.  (Running it in a thread underneath the reserve gains nothing: the allocation holds the allocator / driver lock,
    # 3.93 s serial against 3.96 s overlapped.)
    t = time.perf_counter()
    wq = dqc_amd.KS(dqc_amd.Mol(M.H2O, basis="cc-pvdz", grid="sg3", device=dev), xc=XC)
    we = wq._engine
    wz = torch.zeros(we.shape[-2:], dtype=torch.float64, device=dev)
    we.dm2scp(we.scp2dm(we.dm2scp(wz)))  # (integrals, grid, AO, eigh, one Fock build with the grid pass)
    wa = we.hamilton._ovlp_ao
    torch.linalg.eigh(torch.stack([wa, wa]))
    torch.linalg.cholesky(wa)
    del wq, we, wz, wa
    t = lap("process_warmup", t)
    mols = []
    for i in mine:
        zs, pos = M.c5_molecule(i)
        mol = dqc_amd.Mol((zs, pos), basis="cc-pvdz", grid="sg3", device=dev)
        if args.df:
            mol.densityfit(method="coulomb", auxbasis=args.df)
        mol.get_hamiltonian()  # tables on the device, overlap matrix enqueued
        mols.append(mol)
    # the orthogonalisers of the whole batch from one batched eigh (one rocSOLVER call per molecule made the host wait 11 ms each)
    prepare_orthogonalisers([m.get_hamiltonian() for m in mols])
    t = lap("tables_overlap_orthogonalisers", t)
    for mol in mols:
        qc = dqc_amd.KS(mol, xc=XC)
        qcs.append(qc)
        engines.append(qc._engine)
    # (per molecule: ERI tile fill on a side stream underneath T, V, the Becke grid and the AO evaluation; no device
    # synchronisation between molecules, so the next molecule's host work overlaps this one's fill -- stage clocks inside would
    # serialise what the build overlaps: tools/gpu_setup_breakdown.py has them one by one)
    t = lap("integrals_grid_ao", t)
    del mols
    # density of the core-Hamiltonian guess ("1e", reference scf_qccalc.py:88-91) after one SCF update, for every molecule:
    # the occupied spaces come from the batched purification of the lockstep driver (no eigensolver)
    # in deterministic mode (fixed-point cross-block sums): these densities are the timed steps' inputs, and with the same
    # arguments they must be the same bits from run to run (--dump-outputs compares builds output for output)
    t = time.perf_counter()
    det_prev = lib.set_deterministic(True)
    from dqc_amd.lockstep import LockstepSCF
    ls = LockstepSCF(qcs)
    n = engines[0].shape[-1]
    z0 = torch.zeros((n, n), dtype=torch.float64, device=dev)
    q0 = ls.occupied_orbitals(torch.stack([e.dm2scp(z0) for e in engines]))
    f1 = torch.stack([e.dm2scp(e.hamilton.ao_orb2dm(q0[k], e.orb_weight)) for k, e in enumerate(engines)])
    q1 = ls.occupied_orbitals(f1)
    for k, eng in enumerate(engines):
        orbs.append(q1[k].contiguous())
        dms.append(eng.hamilton.ao_orb2dm(orbs[k], eng.orb_weight))
    del ls, q0, f1
    lap("two_fock_builds_and_projectors", t)
    lib.set_deterministic(det_prev)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    brk = {k: round(v, 4) for k, v in brk.items()}
    h0 = engines[0].hamilton
    nao, ngrid, ld = h0._nao_ao, h0.rgrid.shape[0], h0._ld

    from dqc_amd.batch import CuPartition
    j_cus = args.j_cus if args.j_cus >= 0 else int(os.environ.get("DQC_AMD_J_CUS", str(DEFAULT_J_CUS)))
    if args.df or args.dense_dm:
        j_cus = 0 if args.df else j_cus
    partition = None
    if j_cus > 0:
        # round 6: the chip split in two -- grid pass (matrix-core-bound) on 32 - k CUs of every XCD, the Coulomb tile stream
        # (HBM-bound) of the same molecule on the other k; builds dealt to --grid-streams streams of the grid partition
        partition = CuPartition(dev, j_cus, max(1, args.grid_streams))
        streams = partition.grid_streams
        nstreams = len(streams)
    else:
        nstreams = max(1, min(args.streams, len(engines)))
        streams = [torch.cuda.Stream(device=dev) for _ in range(nstreams)] if nstreams > 1 else [torch.cuda.current_stream(dev)]
    torch.cuda.synchronize()

    def step(record=None, dense_dm=False, sel=None):
        scps = []  # what the callers of dm2scp receive: the Fock matrices
        for k, (eng, dm, orb) in enumerate(zip(engines, dms, orbs)):
            if sel is not None and k >= sel:
                break
            # a fresh density-matrix tensor every step (defeats the J/K memoisation: everything is recomputed).
            # Default: D = ao_orb2dm(C_occ, n) exactly as scp2dm produces it in every SCF iteration (hf.py:105-113), so
            # the Hamiltonian knows its rank-n_occ factor; --dense-dm hands over an anonymous full matrix instead.
            if record is None:
                with torch.cuda.stream(streams[k % nstreams]) if (nstreams > 1 or partition is not None) else contextlib.nullcontext():  # independent molecules: dealt round-robin to the streams
                    d = dm.clone() if dense_dm else eng.hamilton.ao_orb2dm(orb, eng.orb_weight)
                    scps.append(eng.dm2scp(d))
            else:  # per-kernel events: one molecule at a time on the current stream
                d = dm.clone() if dense_dm else eng.hamilton.ao_orb2dm(orb, eng.orb_weight)
                record.append(eng.hamilton.timed_fock_kernels(d, eng.knvext.fullmatrix()))
        return scps

    dense = args.dense_dm
    for _ in range(args.warmup):
        step(dense_dm=dense)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # --min-seconds > 0: a step is repeated so that the timed region is long enough for the driver's samplers
    repeats = 1
    if args.min_seconds > 0:
        barrier()
        t0 = time.perf_counter()
        step(dense_dm=dense)
        barrier()
        est = time.perf_counter() - t0
        repeats = max(1, int(math.ceil(args.min_seconds / max(est * args.steps, 1e-9))))
        if world > 1:
            tr = torch.tensor([repeats], dtype=torch.int64, device=dev)
            dist.all_reduce(tr, op=dist.ReduceOp.MAX)
            repeats = int(tr)

    # ---------------- timed region: exactly K steps (each = `repeats` passes over the batch) ----------------
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        for _ in range(repeats):
            last = step(dense_dm=dense)
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, "fock" if world == 1 else "fock_rank%d" % rank, last, DUMP_LIMIT_BYTES // world)
    del last
    per_rank = {"setup_s": [setup_s], "timed_s": [elapsed]}
    if world > 1:
        # one row per rank (owned by it, zero elsewhere): a sum is a gather
        tab_r = torch.zeros((world, 2), dtype=torch.float64, device=dev)
        tab_r[rank, 0], tab_r[rank, 1] = setup_s, elapsed
        dist.all_reduce(tab_r)
        per_rank = {"setup_s": tab_r[:, 0].tolist(), "timed_s": tab_r[:, 1].tolist()}
        elapsed = float(tab_r[:, 1].max())
    passes = args.steps * repeats

    # ---------------- --full: per-kernel HIP-event timing (same stream as the launches), first 4 local molecules ----------------
    nsel = min(4, len(engines))
    ktime = {}
    if args.full:
        rec = []
        for _ in range(max(3, min(args.steps, 10))):
            step(rec, dense_dm=dense, sel=nsel)
        torch.cuda.synchronize()
        names = rec[0][0]
        ktime = {nm: sum(e[1][i].elapsed_time(e[1][i + 1]) for e in rec) / len(rec) for i, nm in enumerate(names)}  # ms / launch

    out_extra = {}
    if extras:
        K = max(3, min(args.steps, 10))
        # the same steps with an anonymous full density matrix (no factor): the rate a caller that bypasses ao_orb2dm gets
        if not dense:
            step(dense_dm=True, sel=nsel)
            barrier()
            t0 = time.perf_counter()
            for _ in range(K):
                step(dense_dm=True, sel=nsel)
            barrier()
            out_extra["value_full_matrix_dm_per_gpu"] = nsel * K / (time.perf_counter() - t0)
        # SURVEY.md 8(d) metric (ii): the full SCF iteration F -> eigh -> ao_orb2dm -> dm2scp (scp2scp)
        focks = [eng.dm2scp(eng.hamilton.ao_orb2dm(orb, eng.orb_weight)) for eng, orb in zip(engines[:nsel], orbs)]
        for eng, f in zip(engines, focks):
            eng.scp2scp(f)
        barrier()
        t0 = time.perf_counter()
        for _ in range(K):
            for eng, f in zip(engines, focks):
                eng.scp2scp(f)
        barrier()
        out_extra["full_scf_iterations_per_s_eigh_per_gpu"] = nsel * K / (time.perf_counter() - t0)
        # the same with the eigensolver-free step: purification + Fock build replayed as one hipGraph (dqc_amd/graph.py)
        from dqc_amd.graph import GraphedSCFStep
        steps_g = [GraphedSCFStep(eng) for eng in engines[:nsel]]
        for st, f in zip(steps_g, focks):
            st(f)
        barrier()
        t0 = time.perf_counter()
        for _ in range(K):
            for st, f in zip(steps_g, focks):
                st(f)
        barrier()
        one_mol_graph_rate = nsel * K / (time.perf_counter() - t0)
        del steps_g
        # the Hartree-Fock flavour of the J/K pass (get_elrep + get_exchange, hf.py:198-199): one fused J + K launch
        if h0.df is None:
            dao0 = h0._unconvert_dm(dms[0]).contiguous()
            lib.jk(h0._tiles, dao0, h0._jkwork, True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                lib.jk(h0._tiles, dao0, h0._jkwork, True)
            e1.record()
            torch.cuda.synchronize()
            out_extra["jk_with_exchange_ms"] = e0.elapsed_time(e1) / K
            # unrestricted Hartree-Fock trio J[D_u + D_d], K[2 D_u], K[2 D_d] in ONE tile pass (dqc_jk_from_tiles_multi)
            du = torch.stack([dao0 * 0.6, dao0 * 0.4])
            lib.jk_multi(h0._tiles, dao0.unsqueeze(0), du)
            e0.record()
            for _ in range(K):
                lib.jk_multi(h0._tiles, dao0.unsqueeze(0), du)
            e1.record()
            torch.cuda.synchronize()
            out_extra["jk_unrestricted_j_2k_one_pass_ms"] = e0.elapsed_time(e1) / K
            lib.jk_multi(h0._tiles, dao0.unsqueeze(0), None)
            e0.record()
            for _ in range(K):
                lib.jk_multi(h0._tiles, dao0.unsqueeze(0), None)
            e1.record()
            torch.cuda.synchronize()
            out_extra["jk_multi_j_only_ms"] = e0.elapsed_time(e1) / K
            out_extra["eri_fill"] = eri_fill_stats(h0, dev)
        # deterministic mode (fixed-point integer atomics instead of fp64 atomics in the cross-block sums): cost and proof
        def _rate(k):
            torch.cuda.synchronize()
            t0_ = time.perf_counter()
            for _ in range(k):
                engines[0].dm2scp(engines[0].hamilton.ao_orb2dm(orbs[0], engines[0].orb_weight))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0_) / k
        _rate(3)
        t_at = _rate(20)
        lib.set_deterministic(True)
        _rate(3)
        t_det = _rate(20)
        fdet = [engines[0].dm2scp(dms[0].clone()) for _ in range(3)]
        lib.set_deterministic(False)
        fat = engines[0].dm2scp(dms[0].clone())
        out_extra["deterministic_mode"] = {"fock_build_ms_fp64_atomics": 1e3 * t_at, "fock_build_ms_deterministic": 1e3 * t_det,
                                           "cost_percent": 100.0 * (t_det / t_at - 1.0),
                                           "repeated_builds_bit_identical": bool(all(torch.equal(f, fdet[0]) for f in fdet[1:])),
                                           "max_abs_fock_diff_vs_fp64_atomics": float((fdet[0] - fat).abs().max()),
                                           "note": "dqc_set_deterministic(1): J accumulators, split-K Vxc and the purification trace summed as "
                                                   "fixed-point 64-bit integers (associative); one molecule, one stream"}
        # SURVEY.md 8(d) metric (iv): time to the converged energies of the batch -- KS(...).energy() of every molecule of this
        # rank from the core guess (setup above excluded, reported beside it).  (a) the batch driver: lockstep SCF
        # (dqc_amd/lockstep.py: DIIS, purification and the Cholesky-QR batched over the molecules, one host read per iteration
        # for the batch); (b) the one-molecule drivers of round 2, 8 in flight on their own streams, as the cross-check
        from dqc_amd.batch import run_concurrent, run_lockstep
        barrier()
        t0 = time.perf_counter()
        run_lockstep(qcs)
        es = [float(qc.energy()) for qc in qcs]
        barrier()
        scf_s = time.perf_counter() - t0
        nits = [int(qc.niter) for qc in qcs]
        nit, nconv = sum(nits), sum(int(qc.converged) for qc in qcs)
        nstall, nfb = sum(int(qc.stalled) for qc in qcs), sum(int(getattr(qc, "eigh_fallbacks", 0)) for qc in qcs)
        errmax = max(float(qc.scf_error) for qc in qcs)
        hist = {}
        for k in nits:
            hist[k] = hist.get(k, 0) + 1
        barrier()
        t0 = time.perf_counter()
        run_concurrent(qcs, max_inflight=8)
        es_conc = [float(qc.energy()) for qc in qcs]
        nit_conc = sum(qc.niter for qc in qcs)
        barrier()
        scf_conc_s = time.perf_counter() - t0
        de_max = max(abs(a - b) for a, b in zip(es, es_conc))
        tab = torch.tensor([scf_s, float(nit), float(nconv), float(len(qcs)), setup_s, float(nstall), float(nfb), scf_conc_s,
                            float(nit_conc)], dtype=torch.float64, device=dev)
        if world > 1:
            tmx = tab.clone()
            dist.all_reduce(tmx, op=dist.ReduceOp.MAX)
            dist.all_reduce(tab, op=dist.ReduceOp.SUM)
            tab[0], tab[4], tab[7] = tmx[0], tmx[4], tmx[7]
        out_extra["batch_scf"] = {"time_to_converged_energy_s": float(tab[0]), "scf_iterations_total": int(tab[1]),
                                  "molecules": int(tab[3]), "converged": int(tab[2]), "stalled": int(tab[5]),
                                  "eigh_fallbacks": int(tab[6]), "max_scf_error_rank0": errmax,
                                  "iterations_histogram_rank0": {str(k): v for k, v in sorted(hist.items())},
                                  "time_one_molecule_drivers_8_in_flight_s": float(tab[7]),
                                  "scf_iterations_one_molecule_drivers": int(tab[8]),
                                  "max_abs_energy_diff_lockstep_vs_one_molecule_ha": de_max, "setup_s_max_rank": float(tab[4]),
                                  "energy_molecule0_ha": es[0] if rank == 0 else None,
                                  "note": "KS(mol, xc) energies of every molecule from the core guess, f_tol 1e-9 on max|[F,D]|: "
                                          "lockstep batch driver (batch.run_lockstep); the one-molecule DIIS + purification-graph "
                                          "drivers (batch.run_concurrent, 8 in flight) beside it; one-off setup (ERI fill, AO on "
                                          "grid) listed separately"}
        # SURVEY.md 8(d) metric (ii) for the batch: whole SCF iterations (DIIS + projector + Fock build) per second
        out_extra["full_scf_iterations_per_s_per_gpu"] = nit / scf_s
        out_extra["full_scf_iterations_per_s_one_molecule_graph_per_gpu"] = one_mol_graph_rate

    if extras and world == 1:
        out_extra["small_batch"] = small_batch_leg(dev)
        out_extra["direct_scf"] = direct_scf_leg(dev)

    if extras and world == 1:
        out_extra["f_rows"] = f_row_legs(dev)

    # N > 1 only, after everything that is timed for the headline: ONE molecule (C4) spread over the N ranks -- the path with a
    # data-path collective (last row).  Run under a watchdog: a wedged collective must not cost the line above.
    one_mol = None
    if world > 1 and extras and not args.no_one_molecule_leg:
        one_mol = one_molecule_sharded_leg(dev, rank, world, timeout_s=150.0)
        if one_mol is not None:
            out_extra["one_molecule_sharded"] = one_mol

    if rank == 0:
        c = 4  # GGA: phi + 3 gradient components
        norb_pad = 0 if dense else lib.padded_norb(orbs[0].shape[1])
        fused = "grid_fused" in ktime
        alg_bytes = {
            # AO read once per pass + per-point in/outs + the (n,n) matrix; see DESIGN.md
            "grid_density": 8.0 * c * ngrid * nao + 8.0 * ngrid * 4 + 8.0 * nao * nao,
            "grid_vxc": 8.0 * c * ngrid * nao + 8.0 * ngrid * 5 + 8.0 * nao * nao,
            "grid_fused": 8.0 * c * ngrid * nao + 8.0 * ngrid * 2 + 2 * 8.0 * nao * nao,
            "jk_tiles": float(nao) ** 4 + 3 * 8.0 * nao * nao,
        }
        if args.df:  # two passes over the i >= j rows of j3c (dqc_df_coulomb) + inv_j2c
            naux = int(h0.df.j2c.shape[0])
            alg_bytes["jk_tiles"] = 2 * 4.0 * nao * (nao + 1) * naux + 8.0 * naux * naux + 2 * 8.0 * nao * nao
        f_den = (2.0 * ngrid * nao * nao if dense else 4.0 * ngrid * nao * norb_pad) + 2.0 * c * ngrid * nao  # (algorithmic: nao, not the padded widths)
        f_vxc = 2.0 * ngrid * nao * nao + 2.0 * c * ngrid * nao
        alg_flops = {
            # 2 G n^2 per GEMM pass (+ the row dots / Psi combination); J: 2 n^4 dense-equivalent
            # density: Phi . D (full matrix) or the two chained rank-n_occ GEMMs Phi . L, (Phi L) . L^T (factor form)
            "grid_density": f_den, "grid_vxc": f_vxc, "grid_fused": f_den + f_vxc, "jk_tiles": 2.0 * float(nao) ** 4,
        }
        alg_bytes = {k: v for k, v in alg_bytes.items() if k in ktime}
        roofs = {}
        if args.full:
            # HBM bytes per launch from the committed rocprofv3 PMC pass of this same command (bench.py cannot sample
            # counters itself): only reported when that pass was taken with these very sources (kernel code + this file)
            traffic, traffic_note = {}, None
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
                sha = source_sha16()
                if tj.get("csrc_sha16") != sha["csrc_sha16"] or tj.get("bench_py_sha16") != sha["bench_py_sha16"]:
                    traffic_note = "profiles/pmc_traffic.json was taken with other sources (%s / %s): not reported" % (
                        tj.get("csrc_sha16"), tj.get("bench_py_sha16"))
                elif tj["workload"] == {"nao": nao, "ngrid": ngrid, "xc": "gga"}:
                    traffic = dict(tj["hbm_read_bytes_per_launch"])
            except Exception as e:  # noqa: BLE001
                traffic_note = "no usable profiles/pmc_traffic.json (%s)" % type(e).__name__
            mfma_ceiling = lib.probe_mfma_f64_tflops(dev)
            hbm_ceiling = lib.probe_hbm_read_gbs(dev)

            def roof(k):
                t = ktime[k] * 1e-3
                gbs, tfs = alg_bytes[k] / t / 1e9, alg_flops[k] / t / 1e12
                # the binding roof is the one the kernel sits closer to
                if k != "jk_tiles" and tfs / F64_MFMA_PEAK_TF > gbs / HBM_PEAK_GBS:
                    return {"bound": "mfma", "kernel": k, "achieved": tfs, "peak": F64_MFMA_PEAK_TF, "unit": "TFLOP/s",
                            "frac": tfs / F64_MFMA_PEAK_TF, "traffic": traffic.get(k), "algorithmic_flops_per_launch": alg_flops[k],
                            "algorithmic_bytes_per_launch": alg_bytes[k], "hbm_gbs": gbs, "hbm_frac": gbs / HBM_PEAK_GBS,
                            "measured_mfma_f64_ceiling_tflops": mfma_ceiling, "frac_of_measured_ceiling": tfs / mfma_ceiling,
                            "avg_launch_ms": ktime[k]}
                return {"bound": "hbm", "kernel": k, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": gbs / HBM_PEAK_GBS, "traffic": traffic.get(k), "algorithmic_bytes_per_launch": alg_bytes[k],
                        "measured_hbm_read_ceiling_gbs": hbm_ceiling, "frac_of_measured_ceiling": gbs / hbm_ceiling,
                        "standalone_read_ceiling_gbs": UBENCH_READ_GBS, "frac_of_standalone_ceiling": gbs / UBENCH_READ_GBS,
                        "avg_launch_ms": ktime[k]}

            dom = max(alg_bytes, key=lambda k: ktime[k])
            # the whole molecule-iteration against the HBM roof: algorithmic bytes of ALL its kernels x the rate the timed region achieved
            # (with several streams the kernels of different molecules share the chip and each one's own duration stretches: this entry
            # is the figure that does not depend on how the launches overlap)
            it_bytes = sum(alg_bytes.values())
            it_rate = nmol * passes / elapsed / world
            whole_iteration = {"bound": "hbm", "kernel": "whole_iteration", "achieved": it_bytes * it_rate / 1e9, "peak": HBM_PEAK_GBS,
                               "unit": "GB/s", "frac": it_bytes * it_rate / 1e9 / HBM_PEAK_GBS, "traffic": None,
                               "algorithmic_bytes_per_molecule_iteration": it_bytes, "iterations_per_s_per_gpu": it_rate,
                               "measured_hbm_read_ceiling_gbs": hbm_ceiling, "frac_of_measured_ceiling": it_bytes * it_rate / 1e9 / hbm_ceiling,
                               "standalone_read_ceiling_gbs": UBENCH_READ_GBS, "frac_of_standalone_ceiling": it_bytes * it_rate / 1e9 / UBENCH_READ_GBS,
                               "streams_per_gpu": nstreams,
                               "note": "sum of the kernels' algorithmic bytes per molecule-iteration x the timed region's rate; the per-kernel "
                                       "entries are HIP-event durations of one molecule at a time on one stream"}
            roofs = {
                "kernel_ms_per_molecule": ktime,
                "roofline": roof(dom),
                "roofline_other_kernels": [roof(k) for k in alg_bytes if k != dom] + [whole_iteration],
                "measured_ceilings_note": "measured_hbm_read_ceiling_gbs = dqc_probe_stream_read on a 2 GB buffer (contiguous 32 KB tiles per block, "
                                          "16-byte non-temporal loads, four tiles in flight, two blocks per CU).  Until round 6 the probe ended in 16384 "
                                          "fp64 atomicAdds of its checksum on one address (~75 us per launch) and read 5.2-5.3 TB/s on 2 GB -- the "
                                          "'in-process ceiling' of rounds 2-5, which profiles/r06a_hbm_ceiling_bisect.txt showed to be independent of "
                                          "the process state and profiles/r06c_read_shape.txt traced to those atomics; with one atomic per block it "
                                          "reads 6.15-6.25 TB/s, like plain read kernels in any access shape the grid kernels use.  "
                                          "standalone_read_ceiling_gbs = 6450 is the large-buffer asymptote (tools/ubench/read_bw.hip)",
                "traffic_note": traffic_note,
            }
        out = {
            "metric": "SCF iterations/sec (Fock build + XC grid) per GPU, cc-pVDZ 20-atom",
            "value": nmol * passes / elapsed,
            "unit": "SCF Fock-build iterations/s (whole job)",
            "n_gpus": world, "n_ranks_seen": n_ranks_seen, "per_rank": per_rank, "steps": args.steps, "warmup": args.warmup, "repeats": repeats,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "timed_region_s": elapsed,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "C5: batch of %d x 20-atom vitamin-C-like organics (nao 208, 353400 grid pts of which %d carry "
                                   "non-zero weight and are resident) RKS PBE/cc-pVDZ sg3, %d per GPU; a step = %d pass(es) over the batch"
                                   % (nmol, ngrid, len(mine), repeats),
                       "ngrid_full": int(h0.ngrid_full), "ngrid_resident_molecule0": ngrid,
                       "coulomb": ("density-fitted J, auxbasis %s (naux %d)" % (args.df, int(h0.df.j2c.shape[0]))) if args.df
                                  else "exact J from stored ERI tiles",
                       "molecules_per_gpu": len(mine), "global_batch": nmol, "nao": nao, "ngrid": ngrid, "streams_per_gpu": nstreams,
                       "parallelism": "molecule-sharded x%d, no data-path collective" % world},
            "per_gpu_value": nmol * passes / elapsed / world,
            "density_matrix_input": "full matrix (no factor)" if dense else
                                    "ao_orb2dm(C_occ, n): rank-%d factor known to the Hamiltonian" % norb_pad,
            "setup_s_per_rank": setup_s,
            "setup_breakdown_s_rank0": brk,
            "setup_s_excluding_memory_reserve_rank0": setup_s - brk.get("device_memory_reserve", 0.0),
            "setup_s_batch_only_rank0": setup_s - brk.get("device_memory_reserve", 0.0) - brk.get("process_warmup", 0.0),
            "setup_note": "device_memory_reserve = ONE request for the batch's device memory: the kernel driver clears VRAM that a "
                          "previous process released at ~35 GB/s before handing it out again (instant on a box that has been idle "
                          "for seconds; tools/gpu_alloc_cost3.py) -- a property of the box state, paid once per process; "
                          "process_warmup = first-use loading of the vendor libraries' and this library's code objects, on a water "
                          "molecule, also once per process; setup_s_batch_only_rank0 = the batch's own setup (tables, orthogonalisers, "
                          "ERI fill, grid, AO, two Fock builds) without those two",
            "sources": source_sha16(),
        }
        if args.full:  # (named from the per-kernel pass)
            out["config"]["grid_pass"] = "fused density+XC+Vxc kernel" if fused else "density, XC, Vxc kernels"
        out.update(roofs)
        out.update(out_extra)
        if world == 1 and extras and not args.no_cpu_baseline:
            out["cpu_baseline"], par = cpu_baseline(args.cpu_steps, engines[0], dms[0])
            out.update(par)
            out["cpu_baseline_reference_shape"] = cpu_baseline_dense_benzene(dev)
        print(json.dumps(out), flush=True)
    if world > 1:
        if one_mol is not None and (one_mol.get("hung") or one_mol.get("error")):
            # a collective of the one-molecule leg did not return on some rank (or a rank left the leg early): the line is out;
            # leave without touching the process group again -- a rank stuck in its watchdog follows when that expires
            sys.stdout.flush()
            os._exit(0)
        if one_mol is not None:  # (the closing barrier under the same kind of watchdog)
            import threading
            th = threading.Thread(target=lambda: (dist.barrier(), dist.destroy_process_group()), daemon=True)
            th.start()
            th.join(120.0)
            if th.is_alive():
                sys.stdout.flush()
                os._exit(0)
            return
        dist.barrier()
        dist.destroy_process_group()


def one_molecule_sharded_leg(dev, rank, world, timeout_s):
    """ONE C4 molecule (naphthalene / cc-pVTZ, RKS PBE, sg3) spread over the ranks of this run: HamiltonMI355.shard_over(eri="tiles")
    -- every rank fills and streams its slice of the 30 GB tile store and its slab of the grid; the partial J + Vxc + E_xc of a
    Fock build travel in one all_reduce (RCCL over xGMI).  Timed: Fock builds of the core-guess density, barrier-bracketed.  The
    work runs in a watchdog thread: on a timeout (a wedged collective) the leg reports `hung` and the caller leaves without
    touching the process group again.  `fock_build_ms_one_gpu_unsharded` is in the N = 1 line (direct_scf leg) for comparison."""
    import threading
    import torch.distributed as dist
    res = {}

    def work():
        try:
            import dqc_amd
            from tests import molecules as M
            torch.cuda.set_device(dev)
            t0 = time.perf_counter()
            mol = dqc_amd.Mol(M.naphthalene(), basis="cc-pvtz", grid="sg3", device=dev)
            h = mol.get_hamiltonian().shard_over(eri="tiles")
            eng = dqc_amd.KS(mol, xc=XC)._engine
            n = eng.shape[-1]
            dm = eng.scp2dm(eng.dm2scp(torch.zeros((n, n), dtype=torch.float64, device=dev)))
            torch.cuda.synchronize(dev)
            dist.barrier()
            res["setup_s"] = time.perf_counter() - t0
            for _ in range(3):
                eng.dm2scp(dm)
            torch.cuda.synchronize(dev)
            dist.barrier()
            k = 40
            t1 = time.perf_counter()
            for _ in range(k):
                f = eng.dm2scp(dm)
            torch.cuda.synchronize(dev)
            dist.barrier()
            res["fock_build_ms"] = 1e3 * (time.perf_counter() - t1) / k
            chk = torch.stack([f.abs().sum(), -f.abs().sum()])
            dist.all_reduce(chk, op=dist.ReduceOp.MAX)  # max and -min of the ranks' Fock checksums
            res["fock_checksum"] = float(chk[0])
            res["fock_checksum_spread_over_ranks"] = float(chk[0] + chk[1])
            res.update({"ranks": world, "nao": int(h._nao_ao), "tile_store_gb_per_rank": h._tiles.numel() * 8 / 1e9,
                        "grid_points_per_rank": int(h.rgrid.shape[0]), "collectives_per_build": 1,
                        "all_reduce_bytes_per_build": int(8 * (h._nao_ao ** 2 + h._ld ** 2 + 1)),
                        "note": "C4 naphthalene RKS PBE / cc-pVTZ sg3, one molecule on all ranks: tile store and grid sliced over "
                                "the ranks, partial J + Vxc + E_xc summed with one all_reduce per Fock build"})
            del eng, mol, h
        except Exception as e:  # noqa: BLE001
            res["error"] = repr(e)[:400]

    th = threading.Thread(target=work, daemon=True)
    th.start()
    th.join(timeout_s)
    if th.is_alive():
        return {"error": "timed out after %.0f s (a collective did not return)" % timeout_s, "hung": True, "ranks": world}
    return res


def direct_scf_leg(dev):
    """the path above the tile store's reach (nao > ~740: dqc_direct_*, Schwarz-screened, incremental builds), timed where both
    forms exist: C4 (naphthalene / cc-pVTZ, nao 412) once from the stored tiles and once direct, same energy"""
    import dqc_amd
    from tests import molecules as M
    out = {}
    old = os.environ.get("DQC_AMD_ERI")
    try:
        for mode in ("tiles", "direct"):
            os.environ["DQC_AMD_ERI"] = mode
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            mol = dqc_amd.Mol(M.naphthalene(), basis="cc-pvtz", grid="sg3", device=dev)
            qc = dqc_amd.KS(mol, xc="gga_x_pbe+gga_c_pbe")
            mol.get_hamiltonian()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            qc.run()
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            h = mol.get_hamiltonian()
            out[mode] = {"setup_s": t1 - t0, "scf_s": t2 - t1, "iterations": int(qc.niter), "energy_ha": float(qc.energy()),
                         "converged": bool(qc.converged)}
            if mode == "tiles":  # one Fock build of this molecule on one GPU: the reference point of the N > 1 one-molecule leg
                eng = qc._engine
                n = eng.shape[-1]
                dm = eng.scp2dm(eng.dm2scp(torch.zeros((n, n), dtype=torch.float64, device=dev)))
                for _ in range(3):
                    eng.dm2scp(dm)
                torch.cuda.synchronize(dev)
                t3 = time.perf_counter()
                for _ in range(20):
                    eng.dm2scp(dm)
                torch.cuda.synchronize(dev)
                out["fock_build_ms_one_gpu_unsharded"] = 1e3 * (time.perf_counter() - t3) / 20
                del eng, dm
            if mode == "direct":
                tot, lau, dmax = h._direct_stats
                out[mode].update({"unique_shell_quartets": int(tot), "launched_share_last_build": lau / max(tot, 1),
                                  "max_abs_density_difference_last_build": dmax, "tau": h._DIRECT_TAU})
            del qc, mol, h
            torch.cuda.empty_cache()
    finally:
        if old is None:
            os.environ.pop("DQC_AMD_ERI", None)
        else:
            os.environ["DQC_AMD_ERI"] = old
    out["energy_diff_ha"] = out["direct"]["energy_ha"] - out["tiles"]["energy_ha"]
    out["note"] = ("C4 naphthalene RKS PBE / cc-pVTZ sg3 from the core guess: stored 8-fold-unique tiles (30 GB) vs direct SCF "
                   "(no store: Schwarz-screened shell quartets re-evaluated per build, G[D] = G[D_prev] + G[D - D_prev])")
    return out


def small_batch_leg(dev):
    """batches of SMALL molecules (the sizes of configs C1-C3), where one molecule's kernels fill a fraction
    of the chip and the one-molecule driver is launch-bound: the lockstep batch driver (one set of DIIS / purification launches
    for the batch, per-molecule Fock builds replayed as hipGraphs on a few streams) against the one-molecule drivers run
    concurrently.  Whole SCF runs from the core guess; rate = SCF iterations of all molecules / wall time."""
    import dqc_amd
    from dqc_amd.batch import run_concurrent, run_lockstep
    from tests import molecules as M
    out = {}
    for name, base, nmol, xc, grid, sig in (("h2o_ccpvdz_pbe", M.H2O, 256, XC, "sg2", 0.05),
                                            ("benzene_ccpvdz_lda", M.benzene(), 128, "lda_x+lda_c_pw", "sg3", 0.03)):
        zs, pos0 = base
        mols = []
        for i in range(nmol):
            pos = np.array(pos0) + np.random.default_rng(100 + i).normal(0.0, sig, (len(zs), 3))
            mols.append(dqc_amd.Mol((zs, pos.tolist()), basis="cc-pvdz", grid=grid, device=dev))
        res = {}
        for label, runner in (("lockstep", lambda q: run_lockstep(q)),
                              ("one_molecule_drivers", lambda q: run_concurrent(q, max_inflight=16))):
            qcs = [dqc_amd.KS(m, xc=xc) for m in mols]
            if label == "lockstep":
                runner(qcs[:4])  # (kernel / graph warm-up outside the clock)
                qcs[:4] = [dqc_amd.KS(m, xc=xc) for m in mols[:4]]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner(qcs)
            es = [float(q.energy()) for q in qcs]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[label] = (sum(int(q.niter) for q in qcs) / dt, es, sum(int(q.converged) for q in qcs), dt)
        out[name] = {"molecules": nmol, "xc": xc, "grid": grid,
                     "molecule_iterations_per_s_lockstep": res["lockstep"][0],
                     "molecule_iterations_per_s_one_molecule_drivers": res["one_molecule_drivers"][0],
                     "converged_lockstep": res["lockstep"][2], "wall_s_lockstep": res["lockstep"][3],
                     "max_abs_energy_diff_ha": max(abs(a - b) for a, b in zip(res["lockstep"][1], res["one_molecule_drivers"][1]))}
        del mols, qcs
        torch.cuda.empty_cache()
    return out


def _entry_rooflines(tr_ms, nbuild, shape):
    """per-entry-point rows from a lib.call_trace of `nbuild` Fock builds: calls per build, ms per call, algorithmic bytes / flops
    (SURVEY.md 8d models: AO read once per pass, 2 G n^2 per GEMM pass, n^4 bytes of tiles, two passes over the i >= j rows of
    j3c) and the fraction of the roof the call sits closer to.  An entry point may be several launches (prep / finish kernels)."""
    n, G, r, naux = shape["nao"], shape["ngrid"], shape.get("norb_pad", 0), shape.get("naux", 0)
    def model(name):
        if name == "dqc_grid_density_lr":                 # two chained rank-r GEMMs, four AO components read
            return 8.0 * 4 * G * n, 4.0 * G * n * r + 2.0 * 4 * G * n
        if name == "dqc_grid_density_lr_tau":             # four rank-r GEMMs, four AO components read once
            return 8.0 * 4 * G * n, 8.0 * G * n * r
        if name == "dqc_grid_density_lr[value only]":     # phase 1 only, one component
            return 8.0 * G * n, 2.0 * G * n * r
        if name == "dqc_grid_density":
            return 8.0 * 4 * G * n, 2.0 * G * n * n + 2.0 * 4 * G * n
        if name == "dqc_grid_density[value only]":
            return 8.0 * G * n, 2.0 * G * n * n
        if name == "dqc_grid_density_pair":
            return 8.0 * G * n, 2.0 * G * n * n
        if name == "dqc_grid_vxc":
            return 8.0 * 4 * G * n, 2.0 * G * n * n + 4.0 * 4 * G * n
        if name in ("dqc_grid_vxc[no gradient term]", "dqc_grid_vxc_pair"):  # one operand: symmetric, the upper triangle only
            return 8.0 * G * n, 1.0 * G * n * n
        if name == "dqc_grid_vxc_pair[three gradient components]":  # the tau term: one symmetric update over 3 G stacked rows
            return 8.0 * 3 * G * n, 3.0 * G * n * n
        if name.startswith("dqc_xc_eval"):
            return 8.0 * G * 9, 0.0
        if name in ("dqc_jk_from_tiles", "dqc_jk_from_tiles_part", "dqc_jk_from_tiles_multi"):
            return float(n) ** 4, 2.0 * float(n) ** 4
        if name == "dqc_df_coulomb":
            return 2 * 4.0 * n * (n + 1) * naux + 8.0 * naux * naux, 2 * 2.0 * n * (n + 1) / 2 * naux
        return None

    rows = []
    for name, (calls, ms) in sorted(tr_ms.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
        row = {"entry": name, "calls_per_build": calls / nbuild, "ms_per_call": ms}
        m = model(name)
        if m is not None and ms > 0:
            gbs, tfs = m[0] / ms / 1e6, m[1] / ms / 1e9
            mf = tfs / F64_MFMA_PEAK_TF > gbs / HBM_PEAK_GBS
            row.update({"algorithmic_bytes": m[0], "algorithmic_flops": m[1], "bound": "mfma" if mf else "hbm",
                        "achieved": tfs if mf else gbs, "unit": "TFLOP/s" if mf else "GB/s",
                        "frac": tfs / F64_MFMA_PEAK_TF if mf else gbs / HBM_PEAK_GBS})
        rows.append(row)
    return rows


def f_row_legs(dev, K=10):
    """SURVEY.md 8 'next' rows on the clock, ONE C5 molecule each, steady-state Fock builds dm2scp(ao_orb2dm(C))
    timed with HIP events + a lib.call_trace pass for the per-entry rooflines:
       uks_pbe   unrestricted KS, two-spin grid pass (hcgto.py:260-269 polarised branch, hf.py:93-103)
       scan      meta-GGA: rho, grad rho and tau from one factor-form pass, the tau Vxc term as one one-operand update over the stacked gradient components (hcgto.py:420-438, 473-489)
       df_lda    the reference's own 20-atom benchmark call (dqc/test/benchmark.py:40-42): Mol(...).densityfit() + lda_x+lda_c_pw,
                 with the energy error of the generated auxiliary set against exact J
       anonymous_dm  the same PBE build from a density matrix without a known orbital factor (dense density kernel, hcgto.py:407-418)
       gradient  nuclear gradient of the converged RKS PBE energy (scf_qccalc.py:63-67 by autograd there)"""
    import warnings
    import dqc_amd
    from dqc_amd import lib
    from tests import molecules as M
    geo = M.c5_molecule(0)
    out = {}

    def steady(qc, pol):
        eng, h = qc._engine, qc._engine.hamilton
        n = eng.shape[-1]
        z = torch.zeros((n, n), dtype=torch.float64, device=dev)
        from dqc_amd.utils.datastruct import SpinParam
        dm = eng.scp2dm(eng.dm2scp(SpinParam(u=z, d=z) if pol else z))
        f = eng.dm2scp(dm)
        if pol:  # (F_u, F_d) stacked: each spin channel's own lowest orbitals (hf.py:105-113)
            orbs = [eng._eigvecs(f[0])[..., :eng.norb.u].contiguous(), eng._eigvecs(f[1])[..., :eng.norb.d].contiguous()]
        else:
            orbs = eng.scp2orb(f).contiguous()

        def build():
            if pol:
                d = SpinParam(u=h.ao_orb2dm(orbs[0], eng.orb_weight.u), d=h.ao_orb2dm(orbs[1], eng.orb_weight.d))
            else:
                d = h.ao_orb2dm(orbs, eng.orb_weight)
            return eng.dm2scp(d)

        for _ in range(3):
            build()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(K):
            build()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / K
        with lib.call_trace() as tr:
            for _ in range(3):
                build()
        shape = {"nao": h._nao_ao, "ngrid": int(h.rgrid.shape[0]), "ncomp": 1 if h.xcfamily == 1 else 4,
                 "norb_pad": lib.padded_norb(int((orbs[0] if pol else orbs).shape[1])),
                 "naux": int(h.df.j2c.shape[0]) if h.df is not None else 0}
        return ms, _entry_rooflines(tr.ms(), 3, shape), shape

    try:
        qc = dqc_amd.KS(dqc_amd.Mol(geo, basis="cc-pvdz", grid="sg3", device=dev), xc=XC, restricted=False)
        ms, rows, shape = steady(qc, True)
        out["uks_pbe"] = {"fock_build_ms": ms, "fock_builds_per_s": 1e3 / ms, "entries": rows, "shape": shape,
                          "what": "C5 molecule 0, unrestricted KS PBE: J[D_u + D_d], two factor-form densities, spin-polarised functional, two Vxc matrices"}
        del qc
        qc = dqc_amd.KS(dqc_amd.Mol(geo, basis="cc-pvdz", grid="sg3", device=dev), xc="mgga_x_scan+mgga_c_scan")
        ms, rows, shape = steady(qc, False)
        out["scan"] = {"fock_build_ms": ms, "fock_builds_per_s": 1e3 / ms, "entries": rows, "shape": shape,
                       "what": "C5 molecule 0, RKS SCAN (meta-GGA): density + gradient + tau from the factor in one pass, Vxc + the tau term"}
        del qc
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mdf = dqc_amd.Mol(geo, basis="cc-pvdz", device=dev).densityfit()
        qdf = dqc_amd.KS(mdf, xc="lda_x+lda_c_pw")
        ms, rows, shape = steady(qdf, False)
        def timed_runs(q):  # first run(): captures the iteration graph; second: the SCF loop alone
            ts = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                q.run()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return ts

        t_df1, t_df = timed_runs(qdf)
        e_df = float(qdf.energy())
        qex = dqc_amd.KS(dqc_amd.Mol(geo, basis="cc-pvdz", device=dev), xc="lda_x+lda_c_pw")
        t_ex1, t_ex = timed_runs(qex)
        e_ex = float(qex.energy())
        out["df_lda"] = {"fock_build_ms": ms, "fock_builds_per_s": 1e3 / ms, "entries": rows, "shape": shape,
                         "auxbasis": "autoaux (generated from cc-pVDZ: the reference's default cc-pvtz-jkfit is external data)",
                         "scf_s": t_df, "first_run_s": t_df1, "scf_iterations": qdf.niter, "energy_ha": e_df, "exact_j_energy_ha": e_ex,
                         "energy_error_vs_exact_j_ha": e_df - e_ex, "exact_j_scf_s": t_ex, "exact_j_first_run_s": t_ex1,
                         "exact_j_scf_iterations": qex.niter, "scf_driver": getattr(qdf, "driver_used", None),
                         "what": "the reference's own 20-atom benchmark call (dqc/test/benchmark.py:40-42): "
                                 "KS(Mol(vitamin C, 'cc-pvdz').densityfit(), 'lda_x+lda_c_pw')"}
        del qdf, qex, mdf
        # an ANONYMOUS density matrix (a user's dm0, a density from elsewhere: no orbital factor known) -- the full-matrix
        # density kernel Phi . D (hcgto.py:407-418) instead of the two thin GEMMs
        qa = dqc_amd.KS(dqc_amd.Mol(geo, basis="cc-pvdz", grid="sg3", device=dev), xc=XC)
        ea, ha = qa._engine, qa._engine.hamilton
        na = ea.shape[-1]
        za = torch.zeros((na, na), dtype=torch.float64, device=dev)
        dm_a = ea.scp2dm(ea.dm2scp(za)).clone()  # (a copy: the Hamiltonian does not know its factor)
        before = dict(ha.grid_path_counts)
        for _ in range(3):
            ea.dm2scp(dm_a.clone())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(K):
            ea.dm2scp(dm_a.clone())
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / K
        with lib.call_trace() as tr:
            for _ in range(3):
                ea.dm2scp(dm_a.clone())
        shape = {"nao": ha._nao_ao, "ngrid": int(ha.rgrid.shape[0]), "ncomp": 4, "norb_pad": 0, "naux": 0}
        out["anonymous_dm"] = {"fock_build_ms": ms, "fock_builds_per_s": 1e3 / ms, "entries": _entry_rooflines(tr.ms(), 3, shape), "shape": shape,
                               "dense_density_passes": ha.grid_path_counts["dense"] - before.get("dense", 0),
                               "what": "C5 molecule 0, RKS PBE Fock build of a density matrix whose orbital factor is not known: dense Phi . D density kernel"}
        del qa, dm_a
        qg = dqc_amd.KS(dqc_amd.Mol(geo, basis="cc-pvdz", grid="sg3", device=dev), xc=XC).run()
        qg.nuclear_gradient()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = qg.nuclear_gradient()
        torch.cuda.synchronize()
        out["gradient"] = {"seconds": time.perf_counter() - t0, "sum_of_forces_abs_max": float(g.sum(0).abs().max()),
                           "what": "C5 molecule 0, analytic nuclear gradient of the converged RKS PBE energy (derivative ERIs, int1e, XC terms)"}
        # its parts, each timed on its own (HIP events on the launch stream), with the roof that bounds the XC grid pass
        from dqc_amd import gradient as G
        eg, hg = qg._engine, qg._engine.hamilton
        Xg = hg._orthozer
        dg = Xg @ qg._dm @ Xg.T
        dg = (dg + dg.T) * 0.5
        Tg = lib.cart2sph_matrix(hg._tab, dev)
        dcg = (Tg.T @ dg @ Tg).contiguous()
        gacc = torch.zeros((len(geo[0]), 3), dtype=torch.float64, device=dev)

        def ev_ms(fn, k=3):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / k
        parts = {"eri_grad_ms": ev_ms(lambda: lib.eri_grad(gacc, dcg, 0.0, hg._tab)),
                 "int1e_grad_ms": ev_ms(lambda: lib.int1e_grad(gacc, dcg, dcg, hg._tab, hg._zs)),
                 "xc_gradient_ms": ev_ms(lambda: G._xc_gradient(eg, [dg]))}
        ao3 = lib.eval_gto(hg._tab, hg.rgrid, 3)
        dpg = lib.pad_matrix(dg, hg._ld)
        ldg = ao3.shape[-1]
        bg = ao3[0] @ dpg[:ldg, :ldg]
        cg = [ao3[1 + i] @ dpg[:ldg, :ldg] for i in range(3)]
        rg, grg = lib.grid_density(ao3[:4], hg._nao_ao, dpg, True)
        from dqc_amd.utils.datastruct import ValGrad
        pg = hg.xc.get_vxc(ValGrad(value=rg, grad=grg))
        tk = ev_ms(lambda: lib.grid_xc_gradient_terms(ao3, hg._nao_ao, bg, cg, hg.dvolume, pg.value, pg.grad, grg))
        kb = 8.0 * hg.rgrid.shape[0] * (9 * hg._nao_ao + 4 * hg._nao_ao + 12)  # nine derivative arrays + b, c0..2 + per-point in/out
        parts["xc_terms_kernel"] = {"ms": tk, "algorithmic_bytes": kb, "bound": "hbm", "achieved": kb / (tk * 1e-3) / 1e9, "unit": "GB/s",
                                    "peak": HBM_PEAK_GBS, "frac": kb / (tk * 1e-3) / 1e9 / HBM_PEAK_GBS}
        parts["note"] = ("eri_grad: derivative shell quartets (one launch per class, up / down companions of every bra shell: a "
                         "VALU / LDS recurrence kernel like the fill, no stream roof -- ~8x the fill's quartets at one unit of angular "
                         "momentum more); xc_gradient: deriv-3 AO evaluation, Phi D and d Phi D GEMMs, the fused grid-sum kernel "
                         "(xc_terms_kernel) and the analytic Becke-weight derivative")
        out["gradient"]["parts"] = parts
        del qg, ao3, bg, cg
    except Exception as e:  # noqa: BLE001
        import traceback
        out["error"] = repr(e)[:300] + " | " + traceback.format_exc()[-600:]
    torch.cuda.empty_cache()
    return out


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-run this very command line as N ranks under torch.distributed.run
    (one process per GPU, rendezvous on 127.0.0.1 at a free port) and hand its exit code back"""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def eri_fill_stats(h, dev):
    """the one-off ERI fill of one C5 molecule, warm (second call), into a scratch tile store"""
    from dqc_amd import lib
    tab = h._tab
    lib.eri_tiles(tab, dev)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tiles = lib.eri_tiles(tab, dev)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    nbytes = tiles.numel() * 8
    del tiles
    # shell-pair classes i >= j; quartets (ij|kl) with ij >= kl: what the kernel evaluates (8-fold symmetry)
    ls, npr = tab.bas[:, 1].astype(np.int64), tab.bas[:, 2].astype(np.int64)
    ii, jj = np.tril_indices(tab.nbas)
    pl = np.stack([ls[ii], ls[jj]], 1)
    pp = npr[ii] * npr[jj]
    npair = len(ii)
    nquart = npair * (npair + 1) // 2
    nprimq = (float(pp.sum()) ** 2 + float((pp.astype(np.float64) ** 2).sum())) / 2
    # flop MODEL (not a counter): per primitive quartet and Rys root ~ 3 (la+lb+1)(lc+ld+1) * 8 for the 2D recurrences,
    # + 3 flops per Cartesian integral and root for the assembly; roots = L/2 + 1
    ncart = lambda l: (l + 1) * (l + 2) // 2  # noqa: E731
    lb_, cb_ = pl.sum(1), ncart(pl[:, 0]) * ncart(pl[:, 1])
    flops = 0.0
    # class-pair sums without forming the npair^2 table: group pairs by (la, lb)
    keys = {}
    for k in range(npair):
        key = (int(pl[k, 0]), int(pl[k, 1]))
        keys[key] = keys.get(key, 0.0) + float(pp[k])
    items = list(keys.items())
    for (a, wa) in items:
        for (b, wb) in items:
            L = sum(a) + sum(b)
            roots = L // 2 + 1
            per = roots * (24.0 * (sum(a) + 1) * (sum(b) + 1) + 3.0 * ncart(a[0]) * ncart(a[1]) * ncart(b[0]) * ncart(b[1]))
            flops += 0.5 * wa * wb * per
    # what the kernels really walk: pair tables after the negligible-primitive cut, general contractions merged (round 5)
    try:
        stg, stu = lib.eri_pair_stats(tab, True), lib.eri_pair_stats(tab, False)
        actual = {"groups": stg["groups"], "shells": stu["groups"], "primitive_quartets_evaluated": stg["primitive_quartets"],
                  "primitive_quartets_one_shell_per_contraction": stu["primitive_quartets"],
                  "primitive_quartets_evaluated_per_s": stg["primitive_quartets"] / (ms * 1e-3)}
    except Exception as e:  # noqa: BLE001
        actual = {"error": repr(e)[:200]}
    return {"ms": ms, "shell_quartets": int(nquart), "shell_quartets_per_s": nquart / (ms * 1e-3),
            "primitive_quartets_nominal_per_s": nprimq / (ms * 1e-3), "pair_tables": actual, "tile_bytes": nbytes,
            "tile_write_gbs": nbytes / (ms * 1e-3) / 1e9, "fp64_gflops_model": flops / (ms * 1e-3) / 1e9,
            "flop_model": "NOMINAL primitive quartets (nprim products of all shell pairs, no cut, one shell per contraction) x, per "
                          "Rys root, 24 (la+lb+1)(lc+ld+1) for the 2D recurrences + 3 per Cartesian integral; an estimate, not a "
                          "hardware counter -- the kernels evaluate pair_tables.primitive_quartets_evaluated of them"}


def _calibrated_threads(fn):
    """torch's intra-op pool collapses when oversubscribed (256 threads: 70 s per call on the 64-core EPYC box), so the
    thread count is calibrated: one call each at 16/32/64 threads (capped by the core count), best kept"""
    best = None
    for nt in sorted({min(c, os.cpu_count() or 1) for c in (16, 32, 64)}):
        torch.set_num_threads(nt)
        fn()
        t0 = time.perf_counter()
        fn()
        dt1 = time.perf_counter() - t0
        if best is None or dt1 < best[0]:
            best = (dt1, nt)
    torch.set_num_threads(best[1])
    return best[1]


def cpu_baseline(nsteps, gpu_eng, gpu_dm):
    """the oracle (CPU restatement of DQC's algorithm, kind = "port") timed on this box's host cores on a bounded
    sample of the same workload: molecule 0 of the C5 set, `nsteps` dm2scp evaluations after one warm-up.  The Fock
    matrix and energy the oracle produces for the GPU's own density of that molecule are compared with the GPU's
    (parity_* fields): the checker checks, it is never the thing measured as the product."""
    from oracle import basis as ob, hamilton as oh
    from tests import molecules as M
    t = ob.make_tables(M.c5_molecule(0), "cc-pvdz")
    t0 = time.perf_counter()
    eng = oh.Engine(t, xc=XC, grid="sg3", eri_mode="s4")
    setup = time.perf_counter() - t0
    # the GPU's density of molecule 0, carried over through the AO basis: D_ao = X_g D X_g^T = X_o D_o X_o^T
    hg = gpu_eng.hamilton
    S = hg._ovlp_ao.cpu()
    Dao = (hg._orthozer @ gpu_dm @ hg._orthozer.T).cpu()
    Xo = eng.h.X
    Xinv = Xo.T @ S
    dm = Xinv @ Dao @ Xinv.T
    dm = (dm + dm.T) * 0.5
    nt = _calibrated_threads(lambda: eng.dm2scp(dm))
    t0 = time.perf_counter()
    for _ in range(nsteps):
        F_o = eng.dm2scp(dm)
    dt = time.perf_counter() - t0
    SXo = S @ Xo
    F_cpu = SXo @ F_o @ SXo.T
    SXg = hg._ovlp_ao @ hg._orthozer
    F_gpu = (SXg @ gpu_eng.dm2scp(gpu_dm) @ SXg.T).cpu()
    e_cpu, e_gpu = float(eng.dm2energy(dm)), float(gpu_eng.dm2energy(gpu_dm))
    par = {"parity_max_abs_fock": float((F_gpu - F_cpu).abs().max()), "parity_energy_diff_ha": e_gpu - e_cpu,
           "parity_note": "C5 molecule 0: Fock matrix (AO representation S X F X^T S) and total energy of the GPU's own "
                          "second-iterate density, GPU dm2scp / dm2energy vs the oracle engine timed as cpu_baseline",
           "functional_pins": "the bench functional gga_x_pbe+gga_c_pbe: exchange pinned by a closed form and RKS energies the "
                              "reference's tests hold (test_xc.py:422-428, test_ks.py:49-55); gga_c_pbe has no reference-held "
                              "literal (PBE paper + libxc constants: parity against an executed libxc unpinned).  Of the 24 "
                              "functionals only lda_x, lda_c_pw, gga_x_pbe, mgga_x_scan have reference-held pins "
                              "(DESIGN.md 5, pin table)"}
    return ({"value": nsteps / dt, "unit": "SCF Fock-build iterations/s", "cores": nt,
             "kind": "port", "setup_s": setup,
             "sample": "molecule 0 of the C5 set, %d dm2scp calls after 1 warm-up; J from the packed-s4 ERI matrix "
                       "(3.8 GB) instead of the reference's dense 15 GB einsum (faster than the reference shape), "
                       "density/Vxc passes chunked at 16 MiB like the reference" % nsteps}, par)


def cpu_baseline_dense_benzene(dev):
    """second CPU leg in the reference's EXACT shape -- dense (nao,)^4 ERI tensor and the einsum of hcgto.py:204-214 -- on
    the largest BASELINE config whose dense tensor fits comfortably: benzene RKS PBE/cc-pVDZ sg3 (nao 114, 1.35 GB), with
    the GPU rate on that same molecule beside it"""
    import dqc_amd
    from oracle import basis as ob, hamilton as oh
    from tests import molecules as M
    mol = M.benzene()
    t = ob.make_tables(mol, "cc-pvdz")
    eng = oh.Engine(t, xc=XC, grid="sg3", eri_mode="dense")
    n = eng.h.nao
    dm = eng.scp2dm(eng.dm2scp(torch.zeros((n, n), dtype=torch.float64)))
    nt = _calibrated_threads(lambda: eng.dm2scp(dm))
    t0 = time.perf_counter()
    k = 0
    while k < 3 or time.perf_counter() - t0 < 5.0:
        eng.dm2scp(dm)
        k += 1
    cpu_rate = k / (time.perf_counter() - t0)
    g = dqc_amd.KS(dqc_amd.Mol(mol, basis="cc-pvdz", grid="sg3", device=dev), xc=XC)._engine
    gn = g.shape[-1]
    gd = g.scp2dm(g.dm2scp(torch.zeros((gn, gn), dtype=torch.float64, device=dev)))
    orb = g.scp2orb(g.dm2scp(gd)).contiguous()
    for _ in range(3):
        g.dm2scp(g.hamilton.ao_orb2dm(orb, g.orb_weight))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        g.dm2scp(g.hamilton.ao_orb2dm(orb, g.orb_weight))
    torch.cuda.synchronize()
    gpu_rate = 200 / (time.perf_counter() - t0)
    return {"value": cpu_rate, "unit": "SCF Fock-build iterations/s", "cores": nt, "kind": "port",
            "sample": "benzene RKS PBE/cc-pVDZ sg3 (nao %d, %d grid points), %d dm2scp calls: dense (nao,)^4 ERI tensor + "
                      "torch.einsum exactly as the reference's get_elrep (hcgto.py:204-214), 16 MiB grid chunks" % (
                          n, eng.h.basis.shape[0], k),
            "gpu_value_same_workload": gpu_rate}


if __name__ == "__main__":
    main()
