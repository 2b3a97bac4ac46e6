"""Time the integral-driven ladder kernel (dqc_cc_ladder) against the vector-driven fused kernel (dqc_bse_exchange) and the library
route with W stored, and run dqc_amd.ccsd end to end.

usage: python tools/gpu_ccsd_time.py [out.json] [--small] [--no-ccsd]

The particle-particle ladder of one CCSD iteration, out[v, a, b] = sum_cd W[a, b, c, d] X[v, c, d], W = sum_P B[a, P, c] B[b, P, d], v
the pairs i <= j, on random slabs (the time does not depend on the values) at two sets of extents:
  * the 20-atom molecule of tests/molecules.py (C5 molecule 0) in cc-pVDZ: nvir 162, naux 1156, nocc 46 -> nvec 1081;
  * naphthalene / cc-pVTZ: nvir 378, naux 1440, nocc 34 -> nvec 595.
After a warm-up of each, repetitions of
  (a) ladder   lib.cc_ladder                        (timed through lib.call_trace: HIP events around the entry point)
  (b) vector   lib.bse_exchange on the same operands, x permuted to its layout (the parent's fused route, 4 n^3 naux flops per vector)
  (c) library  W = matmul(B as (n n, naux) ...) STORED (8 n^4 bytes), then one GEMM with the vectors -- only where 3 x 8 n^4 bytes are free
and: the counted flops of (a), 2 n^4 (panels naux + nvec) as launched and 2 n^4 (naux + nvec) as the contraction needs, its rate on the
latter against lib.probe_mfma_f64_tflops(), and the largest difference between the results relative to the largest element.
Then dqc_amd.ccsd on the first molecule (Hartree-Fock with densityfit(exchange=True)): wall time, iterations, and the time inside
dqc_cc_ladder (call_trace) against the rest.  --small: toy extents and H2O / 3-21G, to rehearse the script."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dqc_amd  # noqa: E402
from dqc_amd import lib  # noqa: E402
from tests import molecules as M  # noqa: E402


def timed(fcn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fcn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_row(label, n, naux, nvec, peak, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3)
    ld = (n + 15) // 16 * 16
    b = torch.randn((n, naux, ld), dtype=torch.float64, device=dev, generator=g)
    x = torch.randn((n, n, nvec), dtype=torch.float64, device=dev, generator=g)       # the ladder's layout: the vector index last
    xv = x.permute(2, 0, 1).contiguous()                                               # (nvec, n, n): bse_exchange's
    o_a = torch.empty((nvec, n, n), dtype=torch.float64, device=dev)
    o_b = torch.empty_like(o_a)
    need = int(lib.load().dqc_bse_work_doubles(n, n, n, n, naux, nvec))
    work = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    res = {}

    def ladder():
        with lib.call_trace() as tr:
            lib.cc_ladder(b, b, x, n, n, out=o_a)
        return tr.ms()["dqc_cc_ladder"][1]

    def vector():
        with lib.call_trace() as tr:
            lib.bse_exchange(b, b, xv, n, n, out=o_b, work=work)
        return tr.ms()["dqc_bse_exchange"][1]

    store_w = 3 * 8 * n ** 4 < torch.cuda.mem_get_info(dev)[0]
    if store_w:
        bm = b[:, :, :n].permute(0, 2, 1).reshape(n * n, naux).contiguous()             # [(a, c), P]
        xm = x.reshape(n * n, nvec)

        def library():
            w = torch.matmul(bm, bm.t()).view(n, n, n, n).permute(0, 2, 1, 3).reshape(n * n, n * n)   # [(a, b), (c, d)]: stored, and moved once
            res["out"] = torch.matmul(w, xm).t().reshape(nvec, n, n)

    t_a, t_b, t_c = [ladder()], [vector()], ([timed(library)] if store_w else [])
    diff_b = float((o_a - o_b).abs().max() / o_b.abs().max())
    diff_c = float((o_a - res["out"]).abs().max() / o_a.abs().max()) if store_w else None
    t_a, t_b, t_c = [], [], []
    for _ in range(reps):
        t_a.append(ladder())
        t_b.append(vector())
        if store_w:
            t_c.append(timed(library))
    panels = -(-nvec // 1152)
    flops, launched = 2.0 * n ** 4 * (naux + nvec), 2.0 * n ** 4 * (panels * naux + nvec)
    row = {"shape": label, "n": n, "naux": naux, "nvec": nvec, "ladder_ms": t_a, "vector_driven_ms": t_b, "library_w_stored_ms": t_c,
           "vector_over_ladder_best": min(t_b) / min(t_a), "flops_counted": flops, "flops_launched": launched, "vector_panels": panels,
           "vector_driven_flops": 4.0 * n ** 3 * naux * nvec, "ladder_tflops_best": flops / (min(t_a) * 1e-3) / 1e12,
           "ladder_share_of_mfma_probe": flops / (min(t_a) * 1e-3) / 1e12 / peak,
           "vector_driven_tflops_best": 4.0 * n ** 3 * naux * nvec / (min(t_b) * 1e-3) / 1e12,
           "w_bytes": 8 * n ** 4, "max_diff_vector_over_max_abs": diff_b, "max_diff_library_over_max_abs": diff_c}
    if store_w:
        row["library_over_ladder_best"] = min(t_c) / min(t_a)
    return row


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    lib.load()
    peak = max(lib.probe_mfma_f64_tflops(dev), lib.probe_mfma_f64_tflops(dev))
    shapes = [("toy", 19, 40, 15, 2), ("toy two panels", 33, 12, 1200, 2)] if small else \
        [("C5 molecule 0 / cc-pVDZ extents", 162, 1156, 1081, 3), ("naphthalene / cc-pVTZ extents", 378, 1440, 595, 2)]
    row = {"mfma_f64_probe_tflops": peak, "device": torch.cuda.get_device_name(0), "kernel": []}
    for label, n, naux, nvec, reps in shapes:
        row["kernel"].append(kernel_row(label, n, naux, nvec, peak, reps))
        print(json.dumps(row["kernel"][-1]), flush=True)
        torch.cuda.empty_cache()
    if "--no-ccsd" not in sys.argv:
        m = dqc_amd.Mol(M.H2O if small else M.c5_molecule(0), basis="3-21G" if small else "cc-pvdz")
        m = m.densityfit(auxbasis="etb", exchange=True) if small else m.densityfit(exchange=True)
        t0 = time.time()
        qc = dqc_amd.HF(m).run()
        t_scf = time.time() - t0
        torch.cuda.synchronize()
        t0 = time.time()
        with lib.call_trace() as tr:
            r = dqc_amd.ccsd(qc)
        torch.cuda.synchronize()
        wall = time.time() - t0
        ms = tr.ms()
        calls, mean = ms["dqc_cc_ladder"]
        row["ccsd"] = {"molecule": "H2O / 3-21G" if small else "C5 molecule 0 (20 atoms) / cc-pVDZ", "scf_seconds": t_scf, "ccsd_seconds": wall,
                       "ladder_calls": calls, "ladder_seconds": calls * mean * 1e-3, "rest_seconds": wall - calls * mean * 1e-3,
                       "niter": r.niter, "converged": r.converged, "residual": r.residual, "e_scf": float(qc.energy()),
                       "e_corr": float(r.e_corr), "e_mp2": float(r.e_mp2), "t1_diagnostic": r.t1_diagnostic, "naux": r.naux,
                       "nocc": int(r.t1.shape[0]), "nvir": int(r.t1.shape[1])}
    print(json.dumps(row), flush=True)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(row, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
