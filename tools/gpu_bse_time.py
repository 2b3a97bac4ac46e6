"""Time the fused BSE product kernel (dqc_bse_exchange) against the library route, and run dqc_amd.bse end to end.

usage: python tools/gpu_bse_time.py [out.json] [--small]

The direct product Wd X of eight trial vectors, out[v, i, a] = sum_P sum_jb L[i, P, j] X[v, j, b] R[a, P, b], on two shapes:
  * the 20-atom molecule of tests/molecules.py (VITC) in cc-pVDZ, Hartree-Fock with densityfit(exchange=True): L = (1 + Q(0))^-1 Boo
    and R = Bvv from the Hamiltonian's own fitted tensor, as dqc_amd.bse makes them;
  * the extents of naphthalene / cc-pVTZ (nocc 34, nvir 378, naux 1440: tools/gpu_mp2_density_time.py), random tensors -- the time
    does not depend on the values.
After a warm-up of both sides three ALTERNATING repetitions of
  fused    lib.bse_exchange                                       (timed through lib.call_trace: HIP events around the entry point,
           the slot sum included)
  library  two torch.matmul with the STORED intermediate of nvec naux nocc nvir doubles, in both orders of the chain: "L first",
           T = matmul(L as (nocc naux, nocc), X), then matmul(T as (nvec nocc, naux nvir), R as (naux nvir, nvir)) -- the order of the
           formula, but its first product has an inner extent of nocc only -- and "R first", Z = matmul(X as (nvec nocc, nvir),
           R as (nvir, naux nvir)), then matmul(L as (nocc, nocc naux), Z as (nvec, nocc naux, nvir)); the unpadded layouts the GEMMs
           want are made once, outside the timed part.  The ratio is taken against the FASTER of the two
and: the flops (the same on both sides: 2 nvec naux nocc nvir (nocc + nvir)), the fused kernel's share of
lib.probe_mfma_f64_tflops(), the bytes of the stored intermediate, the largest difference of the two results relative to the largest
element (they must agree: faster and different is not faster), and dqc_amd.bse end to end on the VITC calculation (wall time of the
first call: tensors, Q(0), G0W0 for the window, Davidson; and of a second spin channel from the memo).  --small: H2O / 3-21G with
"etb" and a toy second shape, to rehearse the script."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dqc_amd  # noqa: E402
from dqc_amd import lib  # noqa: E402
from dqc_amd.bse import _tensors  # noqa: E402
from tests import molecules as M  # noqa: E402

NVEC = 8


def timed(fcn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fcn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_row(label, l, r, no, nv, peak):
    """fused against library on L (no, naux, ldo), R (nv, naux, ldv)"""
    dev, naux = l.device, int(l.shape[1])
    x = torch.randn((NVEC, no, nv), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    lmat = l[:, :, :no].reshape(no * naux, no).contiguous()
    rmat = r[:, :, :nv].reshape(nv, naux * nv).t().contiguous()
    lmat2 = l[:, :, :no].permute(0, 2, 1).reshape(no, no * naux).contiguous()           # [i, (j, P)]
    rmat2 = r[:, :, :nv].permute(2, 1, 0).reshape(nv, naux * nv).contiguous()           # [b, (P, a)]
    need = int(lib.load().dqc_bse_work_doubles(no, nv, no, nv, naux, NVEC))
    work = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    o_f = torch.empty((NVEC, no, nv), dtype=torch.float64, device=dev)
    res = {}

    def fused():
        with lib.call_trace() as tr:
            lib.bse_exchange(l, r, x, no, nv, out=o_f, work=work)
        return tr.ms()["dqc_bse_exchange"][1]

    def library():
        t = torch.matmul(lmat, x)                                              # (nvec, no naux, nv): stored
        res["out"] = torch.matmul(t.view(NVEC * no, naux * nv), rmat).view(NVEC, no, nv)

    def library_r_first():
        z = torch.matmul(x.view(NVEC * no, nv), rmat2)                         # (nvec no, naux nv) = [v, j, P, a]: stored
        res["out2"] = torch.matmul(lmat2, z.view(NVEC, no * naux, nv))

    fused(), timed(library), timed(library_r_first)
    diff = float((o_f - res["out"]).abs().max() / res["out"].abs().max())
    diff2 = float((o_f - res["out2"]).abs().max() / res["out2"].abs().max())
    t_f, t_l, t_l2 = [], [], []
    for _ in range(3):
        t_f.append(fused())
        t_l.append(timed(library))
        t_l2.append(timed(library_r_first))
    best_l = min(min(t_l), min(t_l2))
    flops = 2.0 * NVEC * naux * no * nv * (no + nv)
    return {"shape": label, "nocc": no, "nvir": nv, "naux": naux, "nvec": NVEC, "fused_ms": t_f, "library_l_first_ms": t_l,
            "library_r_first_ms": t_l2, "library_over_fused_best": best_l / min(t_f), "library_beats_fused_in_any_pair_of_runs": best_l < max(t_f),
            "flops": flops, "fused_tflops_best": flops / (min(t_f) * 1e-3) / 1e12,
            "fused_share_of_mfma_probe": flops / (min(t_f) * 1e-3) / 1e12 / peak, "library_tflops_best": flops / (best_l * 1e-3) / 1e12,
            "intermediate_bytes": NVEC * naux * no * nv * 8, "work_bytes": need * 8, "max_diff_over_max_abs": max(diff, diff2)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    lib.load()
    peak = max(lib.probe_mfma_f64_tflops(dev), lib.probe_mfma_f64_tflops(dev))
    m = dqc_amd.Mol(M.H2O if small else M.VITC, basis="3-21G" if small else "cc-pvdz")
    m = m.densityfit(auxbasis="etb", exchange=True) if small else m.densityfit(exchange=True)
    t0 = time.time()
    qc = dqc_amd.HF(m).run()
    t_scf = time.time() - t0
    with torch.no_grad():
        t = _tensors(qc, None, True)
    rows = [kernel_row("H2O / 3-21G" if small else "VITC (20 atoms) / cc-pVDZ", t["mboo"], t["bvv"], t["no"], t["nv"], peak)]
    del t
    no, nv, naux = (3, 33, 41) if small else (34, 378, 1440)
    g = torch.Generator(device=dev).manual_seed(2)
    l = torch.randn((no, naux, (no + 15) // 16 * 16), dtype=torch.float64, device=dev, generator=g)
    r = torch.randn((nv, naux, (nv + 15) // 16 * 16), dtype=torch.float64, device=dev, generator=g)
    rows.append(kernel_row("toy" if small else "naphthalene / cc-pVTZ extents, random tensors", l, r, no, nv, peak))
    del l, r
    torch.cuda.synchronize()
    t0 = time.time()
    s = dqc_amd.bse(qc)
    torch.cuda.synchronize()
    t_first = time.time() - t0
    t0 = time.time()
    tr = dqc_amd.bse(qc, spin="triplet")
    torch.cuda.synchronize()
    t_second = time.time() - t0
    e2e = {"scf_seconds": t_scf, "bse_seconds_first_call": t_first, "bse_seconds_triplet_from_memo": t_second, "e_scf": float(qc.energy()),
           "window_orbs": s.window_orbs, "gw_gap": s.gw.gap, "singlet_energies": s.energies.tolist(), "osc_strengths": s.osc_strengths.tolist(),
           "triplet_energies": tr.energies.tolist(), "residual": s.residual, "naux": s.naux}
    row = {"molecule": "H2O / 3-21G" if small else "VITC (20 atoms) / cc-pVDZ", "mfma_f64_probe_tflops": peak,
           "device": torch.cuda.get_device_name(0), "kernel": rows, "bse_g0w0_hf": e2e}
    print(json.dumps(row), flush=True)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(row, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
