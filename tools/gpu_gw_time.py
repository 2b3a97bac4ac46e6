"""Time the fused G0W0 screening kernel (dqc_gw_screened_diag) against the library route on the tensor of a real molecule, and run
dqc_amd.gw end to end on Hartree-Fock and PBE references.

usage: python tools/gpu_gw_time.py [out.json] [--small]

The 20-atom molecule of tests/molecules.py (VITC) in cc-pVDZ, Hartree-Fock with densityfit(exchange=True): Q on the default grid of
dqc_amd.gw (nfreq 100) from the Hamiltonian's own fitted tensor, Wc = -(1 + Q)^-1 Q, and for two target sets -- HOMO-4 ... LUMO+4 and
every orbital -- after a warm-up of both sides three ALTERNATING repetitions of
  fused    lib.gw_screened_diag on the whole grid                      (timed through lib.call_trace: HIP events around the entry point)
  library  per frequency Y = torch.matmul(Wc[k], B) (both triangles), then W[k] = sum_P B * Y; the (naux, ntarget ldm) layout the
           GEMM wants is made once, outside the timed part
and: the flops of each side on its own count (fused: the lower triangle and the row dot, nfreq ntarget nmo (naux (naux + 1) + 2 naux);
library: 2 nfreq ntarget nmo naux^2 + the reduction), the fused kernel's share of lib.probe_mfma_f64_tflops(), the largest difference of the
two results relative to the largest element (they must agree: faster and different is not faster), and dqc_amd.gw end to end (wall
time; HOMO, LUMO, gap) on the HF calculation and on a PBE one of the same molecule.  --small: H2O / 3-21G with "etb", to rehearse the
script (and for the H2O rows of the log)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dqc_amd  # noqa: E402
from dqc_amd import lib  # noqa: E402
from dqc_amd.gw import correlation_part  # noqa: E402
from dqc_amd.postscf import orbitals, transform_ov  # noqa: E402
from dqc_amd.rpa import frequency_grid  # noqa: E402
from tests import molecules as M  # noqa: E402


def library_route(wc, bflat, ntarget, ldm, out):
    """W[k, n, m] = sum_P B[P, (n, m)] (Wc[k] B)[P, (n, m)], one GEMM and one multiply-and-reduce per frequency; bflat (naux, ntarget ldm)"""
    for k in range(wc.shape[0]):
        out[k] = (bflat * torch.matmul(wc[k], bflat)).sum(0).view(ntarget, ldm)
    return out


def timed(fcn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fcn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def end_to_end(qc, t_scf):
    t0 = time.time()
    g = dqc_amd.gw(qc)
    torch.cuda.synchronize()
    t_gw = time.time() - t0
    no = int((qc._engine.orb_weight != 0).sum())
    e = g.mo_energies
    return {"scf_seconds": t_scf, "gw_seconds_end_to_end": t_gw, "e_scf": float(qc.energy()), "mo_homo": float(e[no - 1]), "mo_lumo": float(e[no]),
            "homo": g.homo, "lumo": g.lumo, "gap": g.gap, "z_homo": float(g.z[no - 1]), "z_lumo": float(g.z[no]),
            "converged_frontier": bool(g.converged[no - 1]) and bool(g.converged[no]), "converged_all": int(g.converged.sum()),
            "sigma_points": int(g.sigma_points.numel()), "naux": g.naux}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    lib.load()
    peak = max(lib.probe_mfma_f64_tflops(dev), lib.probe_mfma_f64_tflops(dev))

    def mol(**kw):
        m = dqc_amd.Mol(M.H2O if small else M.VITC, basis="3-21G" if small else "cc-pvdz", **kw)
        return m.densityfit(auxbasis="etb", exchange=True) if small else m.densityfit(exchange=True)

    t0 = time.time()
    qc = dqc_amd.HF(mol()).run()
    t_scf = time.time() - t0
    h = qc._engine.hamilton
    b = h.df._b
    co, cv, eo, ev = orbitals(qc, 0)[0]
    c_all = torch.cat([co, cv], dim=1)
    no, nmo, naux, nfreq = int(co.shape[1]), int(c_all.shape[1]), int(b.shape[0]), 100
    freqs, _ = frequency_grid(nfreq, 1.0)
    q = lib.rpa_response(transform_ov(b, co, cv), eo, ev, freqs.to(dev), 4.0)
    wc = correlation_part(q).contiguous()
    del q
    rows = []
    for label, orbs in (("HOMO-4 ... LUMO+4", list(range(max(no - 5, 0), min(no + 5, nmo)))), ("all orbitals", list(range(nmo)))):
        bn = transform_ov(b, c_all[:, orbs].contiguous(), c_all)
        ntarget, ldm = int(bn.shape[0]), int(bn.shape[2])
        bflat = bn.transpose(0, 1).reshape(naux, ntarget * ldm).contiguous()
        w_f = torch.empty((nfreq, ntarget, nmo), dtype=torch.float64, device=dev)
        w_l = torch.empty((nfreq, ntarget, ldm), dtype=torch.float64, device=dev)

        def fused():
            with lib.call_trace() as tr:
                lib.gw_screened_diag(wc, bn, nmo, out=w_f)
            return tr.ms()["dqc_gw_screened_diag"][1]

        fused(), timed(lambda: library_route(wc, bflat, ntarget, ldm, w_l))
        diff = float((w_f - w_l[:, :, :nmo]).abs().max() / w_l[:, :, :nmo].abs().max())
        t_f, t_l = [], []
        for _ in range(3):
            t_f.append(fused())
            t_l.append(timed(lambda: library_route(wc, bflat, ntarget, ldm, w_l)))
        flops_f = float(nfreq) * ntarget * nmo * (naux * (naux + 1.0) + 2.0 * naux)
        flops_l = float(nfreq) * ntarget * ldm * (2.0 * naux * naux + 2.0 * naux)
        rows.append({"targets": label, "ntarget": ntarget, "bn_bytes": bn.numel() * 8, "fused_ms": t_f, "library_ms": t_l,
                     "library_over_fused_best": min(t_l) / min(t_f), "library_beats_fused_in_any_pair_of_runs": min(t_l) < max(t_f),
                     "fused_flops": flops_f, "fused_tflops_best": flops_f / (min(t_f) * 1e-3) / 1e12,
                     "fused_share_of_mfma_probe": flops_f / (min(t_f) * 1e-3) / 1e12 / peak,
                     "library_flops": flops_l, "library_tflops_best": flops_l / (min(t_l) * 1e-3) / 1e12, "max_diff_over_max_abs": diff})
        del bn, bflat, w_f, w_l
    del wc
    hf = end_to_end(qc, t_scf)
    t0 = time.time()
    ks = dqc_amd.KS(mol(grid="sg2"), xc="gga_x_pbe+gga_c_pbe").run()
    pbe = end_to_end(ks, time.time() - t0)
    row = {"molecule": "H2O / 3-21G" if small else "VITC (20 atoms) / cc-pVDZ", "nocc": no, "nmo": nmo, "naux": naux, "nfreq": nfreq,
           "wc_bytes": nfreq * naux * naux * 8, "mfma_f64_probe_tflops": peak, "device": torch.cuda.get_device_name(0),
           "kernel": rows, "g0w0_hf": hf, "g0w0_pbe": pbe}
    print(json.dumps(row), flush=True)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(row, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
