"""Density-fitted exchange on one molecule of the headline batch (vitamin C, 20 atoms, cc-pVDZ): what a K build costs and what
bounds it.  Device events, warm-up, at least 0.5 s of timed work per variant, the variants alternated in rounds inside one
process (the median round is reported).  Byte and flop counts come from the shapes, not from counters.

  1. dqc_df_exchange per build (both stages); stage 2 alone (dqc_grid_vxc on an array of the half-transformed tensor's shape);
     stage 1 = the difference
  2. the torch / rocBLAS form of the same contraction: Y = B L as one tall-skinny GEMM and K = Y^T Y, and the dense-density form
     sum_P B_P D B_P (DFMI355.exchange_ao without a factor)
  3. the exact J + K pass over the ERI tile store of the same molecule (lib.jk(..., with_k=True))
  4. a whole RI-PBE0 Fock build against a whole exact PBE0 build (eng.dm2scp)

usage: python tools/bench_dfk.py [--auxbasis etb] [--seconds 0.5]   -> one JSON line on stdout, a table on stderr"""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dqc_amd  # noqa: E402
from dqc_amd import lib  # noqa: E402
from tests import molecules as M  # noqa: E402

HBM, MFMA64 = 8.0e12, 78.0e12  # bytes/s of the HBM, fp64 matrix FLOP/s (the measured chip-wide rate of v_mfma_f64_16x16x4: grid_vxc.hip)
ROUNDS = 5


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def measure(variants, seconds):
    """{name: median seconds per call}: every variant warmed up and sized to seconds / ROUNDS per round, then ROUNDS alternating rounds"""
    reps = {}
    for name, fn in variants.items():
        timed(fn, 3)
        reps[name] = max(3, int(seconds / ROUNDS / max(timed(fn, 5), 1e-7)) + 1)
    rows = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            rows[name].append(timed(fn, reps[name]))
    return {name: statistics.median(v) for name, v in rows.items()}, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--auxbasis", default=None, help="auxiliary set of the fit (default: Mol.densityfit's own default)")
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda")
    mol = M.c5_molecule(0)
    mdf = dqc_amd.Mol(mol, basis="cc-pvdz", grid="sg3").densityfit(auxbasis=args.auxbasis, exchange=True)
    mex = dqc_amd.Mol(mol, basis="cc-pvdz", grid="sg3")
    edf, eex = dqc_amd.KS(mdf, xc="pbe0")._engine, dqc_amd.KS(mex, xc="pbe0")._engine
    hdf, hex_ = edf.hamilton, eex.hamilton
    df = hdf.df
    nao, naux = hdf._nao_ao, int(df.j2c.shape[0])
    # a converged-looking density: the occupied orbitals of the core guess
    nocc = int(sum(mol[0])) // 2
    _, c = torch.linalg.eigh(edf._core_matrix())
    orb, w = c[:, :nocc].contiguous(), torch.full((nocc,), 2.0, dtype=torch.float64, device=dev)
    dm_df, dm_ex = hdf.ao_orb2dm(orb, w), hex_.ao_orb2dm(orb, w)
    fac = hdf._factor_of(dm_df)
    assert fac is not None and len(fac) == 1
    pair = fac[0]
    rp, ld, lda = int(pair[0].shape[1]), hdf._ld, lib.ao_stride(nao)
    dao = hdf._unconvert_dm(dm_df).contiguous()
    work = lib.df_exchange_work(nao, naux, rp, dev)
    # stage 2 alone: the Vxc rank update on an array of Yt's shape
    yt = lib.ao_from(torch.randn(naux * rp, nao, dtype=torch.float64, device=dev))
    ones = torch.ones(naux * rp, dtype=torch.float64, device=dev)
    b2 = df._b.reshape(naux * nao, nao)
    lf = pair[0][:nao].contiguous()  # (nao, rp)
    ybuf = torch.empty((naux * nao, rp), dtype=torch.float64, device=dev)

    def torch_half():
        torch.matmul(b2, lf, out=ybuf)

    def torch_rank():
        y = ybuf.reshape(naux, nao, rp).transpose(0, 1).reshape(nao, naux * rp)  # (a copy: rocBLAS wants a matrix)
        return y @ y.t()

    jkwork = lib.jk_workspace(nao, dev)
    tiles = hex_._tiles
    variants = {
        "dqc_df_exchange": lambda: lib.df_exchange(df._b, pair, work),
        "stage2_grid_vxc": lambda: lib.grid_vxc(yt, nao, ones, ones, None),
        "torch_half_transform": torch_half,
        "torch_rank_update": torch_rank,
        "torch_dense_density": lambda: df.exchange_ao(dao, None),
        "exact_jk_tiles": lambda: lib.jk(tiles, dao, jkwork, True),
        "ri_pbe0_build": lambda: edf.dm2scp(dm_df),
        "exact_pbe0_build": lambda: eex.dm2scp(dm_ex),
    }
    # the kernel and the torch forms compute the same matrix
    k_kernel = lib.df_exchange(df._b, pair, work)
    torch_half()
    dk = float((k_kernel - torch_rank()).abs().max()), float((k_kernel - df.exchange_ao(dao, None)).abs().max())
    t, reps = measure(variants, args.seconds)
    t["stage1_half_transform"] = t["dqc_df_exchange"] - t["stage2_grid_vxc"]
    # counts from the shapes (rp: the padded factor width the kernels really work on; r: the occupied orbitals)
    b_bytes, y_bytes = 8.0 * nao * nao * naux, 8.0 * lda * rp * naux
    fl1 = 2.0 * naux * nao * nao * rp                       # Y = B L
    fl2_full, fl2_sym = 2.0 * naux * rp * nao * nao, 1.0 * naux * rp * nao * (nao + 16)   # K = Y^T Y: all tiles / the upper triangle
    sym = ld // 16 <= 15
    counts = {
        "dqc_df_exchange": (b_bytes + 2 * y_bytes, fl1 + (fl2_sym if sym else fl2_full)),
        "stage1_half_transform": (b_bytes + y_bytes, fl1),
        "stage2_grid_vxc": (y_bytes, fl2_sym if sym else fl2_full),
        "torch_half_transform": (b_bytes + 8.0 * nao * rp * naux, fl1),
        "torch_rank_update": (3 * 8.0 * nao * rp * naux, fl2_full),
        "torch_dense_density": (3 * b_bytes, 4.0 * naux * nao ** 3),
        "exact_jk_tiles": (8.0 * lib.eri_store_doubles(nao), None),
    }
    out = {"molecule": "vitamin C / cc-pVDZ", "nao": nao, "naux": naux, "r": nocc, "rp": rp, "auxbasis": getattr(mdf, "auxbasis_used", None),
           "max_abs_diff_kernel_vs_torch_factor_form": dk[0], "max_abs_diff_kernel_vs_torch_dense_form": dk[1], "variants": {}}
    print("nao %d  naux %d  r %d (padded %d)   B %.3f GB  Yt %.1f MB   |K_kernel - K_torch| %.1e / %.1e"
          % (nao, naux, nocc, rp, b_bytes / 1e9, y_bytes / 1e6, dk[0], dk[1]), file=sys.stderr)
    for name in ["dqc_df_exchange", "stage1_half_transform", "stage2_grid_vxc", "torch_half_transform", "torch_rank_update",
                 "torch_dense_density", "exact_jk_tiles", "ri_pbe0_build", "exact_pbe0_build"]:
        row = {"ms": t[name] * 1e3, "calls_per_round": reps.get(name)}
        by, fl = counts.get(name, (None, None))
        if by is not None:
            row.update(bytes=by, bytes_per_s=by / t[name], hbm_fraction=by / t[name] / HBM)
        if fl is not None:
            row.update(flop=fl, flop_per_s=fl / t[name], mfma_f64_fraction=fl / t[name] / MFMA64)
            row["bound"] = "fp64 matrix" if fl / MFMA64 > (by or 0.0) / HBM else "HBM"
        out["variants"][name] = row
        print("%-24s %8.4f ms  %s  %s" % (name, row["ms"], "%6.2f TB/s (%.2f of HBM)" % (row["bytes_per_s"] / 1e12, row["hbm_fraction"]) if by else " " * 26,
                                           "%6.2f TFLOP/s (%.2f of fp64 MFMA)  nearer bound: %s" % (row["flop_per_s"] / 1e12, row["mfma_f64_fraction"], row["bound"]) if fl else ""),
              file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
