"""Time the fused RI-MP2 pair kernel (dqc_mp2_pair_energies, same mode) against the library-GEMM form on synthetic Bov tensors.

usage: python tools/gpu_mp2_time.py [out.json] [--small]

Two shapes: the benchmark molecule (C5 / cc-pVDZ: nocc 46, nvir 162) and naphthalene / cc-pVTZ (nocc 34, nvir 378), naux of the
auxiliary set Mol.densityfit() generates for each (counted on the host from the shell tables; no integrals are computed).
Per shape, after a warm-up of both sides, three ALTERNATING repetitions of
  fused   lib.mp2_pair_energies                                    (device events around `inner` back-to-back calls)
  torch   mp2.pair_energies_reference restricted to i <= j         (batched matmul per i + elementwise torch: the same flops)
and: the fused kernel's share of lib.probe_mfma_f64_tflops() on its 2 * 2 * (o (o + 1) / 2) * (v_pad (v_pad + 16) / 2) * naux flops,
the peak device memory each form allocates beyond its inputs, and the largest difference of the two results relative to
sum |pair energy| (they must agree: faster and different is not faster).  --small: toy shapes, to rehearse the script."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dqc_amd import lib  # noqa: E402
from dqc_amd.mp2 import pair_energies_reference  # noqa: E402
from tests import molecules as M  # noqa: E402


def generated_naux(moldesc, basis):
    """auxiliary functions of the set Mol.densityfit() resolves its default to, for this molecule and orbital basis"""
    import warnings
    from dqc_amd.basis import make_atombases, make_aux_atombases, parse_moldesc
    zs, pos = parse_moldesc(moldesc, dtype=torch.float64)
    orb = make_atombases(zs, pos, basis)
    info = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        aux = make_aux_atombases(zs, pos, "cc-pvtz-jkfit", orb, info)
    return sum((2 * sh.angmom + 1) for ab in aux for sh in ab.bases), info["auxbasis_used"]


def torch_form(b, eo, ev):
    """pair energies of i <= j through the reference: row i against the slabs j >= i"""
    no = b.shape[0]
    pos = torch.zeros((no, no), dtype=b.dtype, device=b.device)
    pss = torch.zeros_like(pos)
    for i in range(no):
        o, s = pair_energies_reference(b[i:i + 1], b[i:], eo[i:i + 1], eo[i:], ev, ev, True)
        pos[i, i:], pss[i, i:] = o[0], s[0]
    return pos, pss


def timed(fcn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fcn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def peak_extra(fcn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fcn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def one_shape(name, no, nv, naux, dev, peak_tflops, inner_fused, inner_torch):
    ldv = (nv + 15) // 16 * 16
    g = torch.Generator(device="cpu").manual_seed(no * 1000 + nv)
    b = torch.zeros((no, naux, ldv), dtype=torch.float64)
    b[:, :, :nv] = torch.randn((no, naux, nv), dtype=torch.float64, generator=g) / naux ** 0.5
    b = b.to(dev)
    eo = torch.linspace(-11.0, -0.3, no, dtype=torch.float64, device=dev)
    ev = torch.linspace(0.1, 4.0, nv, dtype=torch.float64, device=dev)
    need = int(lib.load().dqc_mp2_work_doubles(no, no, nv, nv, 1))
    work = torch.empty(need, dtype=torch.float64, device=dev)
    fused = lambda: lib.mp2_pair_energies(b, b, eo, eo, ev, ev, True, work)  # noqa: E731
    torchf = lambda: torch_form(b, eo, ev)  # noqa: E731
    fo, fs = fused()
    to, ts = torchf()
    tri = torch.triu(torch.ones((no, no), dtype=torch.bool, device=dev))
    diff = max(float(((fo - to) * tri).abs().max() / to.abs().sum()), float(((fs - ts) * tri).abs().max() / ts.abs().sum()))
    for _ in range(2):
        timed(fused, inner_fused), timed(torchf, inner_torch)
    t_f, t_t = [], []
    for _ in range(3):
        t_f.append(timed(fused, inner_fused))
        t_t.append(timed(torchf, inner_torch))
    flops = 2.0 * 2.0 * (no * (no + 1) / 2) * (ldv * (ldv + 16) / 2) * naux
    best = min(t_f)
    row = {"shape": name, "nocc": no, "nvir": nv, "ldv": ldv, "naux": naux, "bov_bytes": b.numel() * 8,
           "fused_ms": t_f, "torch_ms": t_t, "inner_calls": [inner_fused, inner_torch], "flops": flops,
           "fused_tflops_best": flops / (best * 1e-3) / 1e12, "fused_share_of_mfma_probe": flops / (best * 1e-3) / 1e12 / peak_tflops,
           "torch_beats_fused_in_any_pair_of_runs": min(t_t) < max(t_f),
           "max_diff_over_sum_abs_pair_energies": diff,
           "peak_extra_bytes_fused": peak_extra(fused), "peak_extra_bytes_torch": peak_extra(torchf)}
    print(json.dumps(row), flush=True)
    return row


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    lib.load()
    peak = lib.probe_mfma_f64_tflops(dev)
    peak = max(peak, lib.probe_mfma_f64_tflops(dev))
    out = {"mfma_f64_probe_tflops": peak, "device": torch.cuda.get_device_name(0), "shapes": []}
    print(json.dumps({"mfma_f64_probe_tflops": peak}), flush=True)
    if small:
        shapes = [("toy", 3, 33, 41, "none")]
    else:
        n1, used1 = generated_naux(M.c5_molecule(0), "cc-pvdz")
        n2, used2 = generated_naux(M.naphthalene(), "cc-pvtz")
        shapes = [("c5-ccpvdz (benchmark molecule)", 46, 162, n1, used1), ("naphthalene-ccpvtz", 34, 378, n2, used2)]
    for name, no, nv, naux, used in shapes:
        row = one_shape(name, no, nv, naux, dev, peak, 2 if small else 20, 1 if small else 2)
        row["auxbasis"] = used
        out["shapes"].append(row)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(out, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
