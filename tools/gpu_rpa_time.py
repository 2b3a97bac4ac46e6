"""Time the fused RI-dRPA response kernel (dqc_rpa_response) against the library route on the tensor of a real molecule.

usage: python tools/gpu_rpa_time.py [out.json] [--small]

The 20-atom molecule of tests/molecules.py (VITC) in cc-pVDZ, Hartree-Fock with densityfit(exchange=True): Bov from the Hamiltonian's
own fitted tensor and the converged orbitals (nocc 46, nvir 162), the default grid of dqc_amd.rpa (nfreq 48).  After a warm-up of
both sides, three ALTERNATING repetitions of
  fused    lib.rpa_response on the whole grid                      (timed through lib.call_trace: HIP events around the entry point)
  library  per frequency one elementwise scaled copy of the tensor and one torch.matmul against the unscaled one (both triangles);
           the (naux, nocc ldv) layout the GEMM wants is made once, outside the timed part
and: the fused kernel's share of lib.probe_mfma_f64_tflops() on the MFMAs it issues (lower-triangle tiles of 16 x 16, padded virtual
chunks: 2 * 256 * nt (nt + 1) / 2 * nocc * 16 ceil(nv / 16) * nfreq flops), the largest difference of the two results relative to the
largest element (they must agree: faster and different is not faster), and dqc_amd.rpa end to end on the same calculation
(wall time, e_corr, quadrature_error).  --small: H2O / 3-21G, to rehearse the script."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dqc_amd  # noqa: E402
from dqc_amd import lib  # noqa: E402
from dqc_amd.postscf import orbitals, transform_ov  # noqa: E402
from dqc_amd.rpa import frequency_grid  # noqa: E402
from tests import molecules as M  # noqa: E402


def library_route(bflat, gflat, out):
    """Q[k] = (bflat * g_k) bflat^T, one scaled copy and one GEMM per frequency; bflat (naux, nocc ldv), gflat (nfreq, nocc ldv) with
    the scale folded in and zeros in the padding"""
    bt = bflat.t()
    for k in range(gflat.shape[0]):
        torch.matmul(bflat * gflat[k], bt, out=out[k])
    return out


def timed(fcn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fcn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    lib.load()
    peak = max(lib.probe_mfma_f64_tflops(dev), lib.probe_mfma_f64_tflops(dev))
    mol = dqc_amd.Mol(M.H2O if small else M.VITC, basis="3-21G" if small else "cc-pvdz")
    mol = mol.densityfit(auxbasis="etb", exchange=True) if small else mol.densityfit(exchange=True)
    t0 = time.time()
    qc = dqc_amd.HF(mol).run()
    t_scf = time.time() - t0
    h = qc._engine.hamilton
    co, cv, eo, ev = orbitals(qc, 0)[0]
    bov = transform_ov(h.df._b, co, cv)
    no, naux, ldv = (int(x) for x in bov.shape)
    nv, nfreq = int(ev.numel()), 48
    freqs, _ = frequency_grid(nfreq, 1.0)
    fd = freqs.to(dev)
    work_doubles = int(lib.load().dqc_rpa_work_doubles(no, nv, naux, nfreq))
    work = torch.empty(max(work_doubles, 1), dtype=torch.float64, device=dev)
    q_f = torch.empty((nfreq, naux, naux), dtype=torch.float64, device=dev)
    q_l = torch.empty_like(q_f)
    d = torch.zeros((no, ldv), dtype=torch.float64, device=dev)
    d[:, :nv] = ev[None, :] - eo[:, None]
    gflat = 4.0 * d[None] / (d[None] ** 2 + fd[:, None, None] ** 2)
    gflat[:, :, nv:] = 0.0
    gflat = gflat.reshape(nfreq, no * ldv).contiguous()
    bflat = bov.transpose(0, 1).reshape(naux, no * ldv).contiguous()

    def fused():
        with lib.call_trace() as tr:
            lib.rpa_response(bov, eo, ev, fd, 4.0, out=q_f, work=work)
        return tr.ms()["dqc_rpa_response"][1]

    fused(), timed(lambda: library_route(bflat, gflat, q_l))
    diff = float((q_f - q_l).abs().max() / q_l.abs().max())
    sym = bool(torch.equal(q_f, q_f.transpose(1, 2)))
    t_f, t_l = [], []
    for _ in range(3):
        t_f.append(fused())
        t_l.append(timed(lambda: library_route(bflat, gflat, q_l)))
    nt, nca = (naux + 15) // 16, (nv + 15) // 16
    flops = 2.0 * 256 * (nt * (nt + 1) / 2) * no * 16 * nca * nfreq
    best = min(t_f)
    del q_l, bflat, gflat
    t0 = time.time()
    r = dqc_amd.rpa(qc)
    torch.cuda.synchronize()
    t_rpa = time.time() - t0
    row = {"molecule": "H2O / 3-21G" if small else "VITC (20 atoms) / cc-pVDZ", "nocc": no, "nvir": nv, "ldv": ldv, "naux": naux,
           "auxbasis": mol.auxbasis_used, "nfreq": nfreq, "bov_bytes": bov.numel() * 8, "q_bytes": q_f.numel() * 8, "work_doubles": work_doubles,
           "mfma_f64_probe_tflops": peak, "device": torch.cuda.get_device_name(0),
           "fused_ms": t_f, "library_ms": t_l, "library_over_fused_best": min(t_l) / best,
           "library_beats_fused_in_any_pair_of_runs": min(t_l) < max(t_f),
           "flops_issued": flops, "fused_tflops_best": flops / (best * 1e-3) / 1e12,
           "fused_share_of_mfma_probe": flops / (best * 1e-3) / 1e12 / peak,
           "max_diff_over_max_abs": diff, "fused_bit_symmetric": sym,
           "scf_seconds": t_scf, "rpa_seconds_end_to_end": t_rpa, "e_hf": float(qc.energy()), "e_corr": float(r.e_corr),
           "e_dmp2": float(r.e_dmp2), "e_corr_2nd": float(r.e_corr_2nd), "quadrature_error": r.quadrature_error, "e_tot": float(r.e_tot)}
    print(json.dumps(row), flush=True)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(row, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
