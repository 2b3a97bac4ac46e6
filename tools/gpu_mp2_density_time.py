"""Time the RI-MP2 amplitude kernel (dqc_mp2_amplitudes) and the unrelaxed density build around it against an all-torch form, on
synthetic Bov tensors.

usage: python tools/gpu_mp2_density_time.py [out.json] [--small]

The two shapes of tools/gpu_mp2_time.py: the benchmark molecule (C5 / cc-pVDZ: nocc 46, nvir 162, naux 1156) and naphthalene / cc-pVTZ
(nocc 34, nvir 378, naux 1440).  Per shape, after two warm-up rounds of every side, three ALTERNATING repetitions, device events:
  kernel    lib.mp2_amplitudes for all occupied orbitals in one block, into preallocated buffers   (`inner` back-to-back calls)
  build     mp2.unrelaxed_blocks: kernel + the three library contractions (P_vv, P_oo, Gamma)
  torch     the same build with all-torch amplitudes: V by a batched matmul, T = V / D and Tt elementwise, the same contractions
All occupied orbitals form one block on both sides (both shapes fit: 1.05 and 2.7 GB of amplitudes).  Reported too: the kernel's store
bandwidth (its two outputs, 16 B per (a, b)) and flop rate (two accumulators over the tile pairs A <= B) with the share of
lib.probe_mfma_f64_tflops(), the peak device memory each build allocates beyond Bov, and the largest difference between the two
builds' results relative to the largest element (they must agree).  --small: toy shapes, to rehearse the script."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dqc_amd import lib  # noqa: E402
from dqc_amd.mp2 import unrelaxed_blocks  # noqa: E402


def torch_amplitudes(bov, eo, ev, i0, ni, c_os=1.0, c_ss=1.0, out=None):
    """lib.mp2_amplitudes in plain torch (out is not used: the temporaries are the point of the comparison)"""
    ldv = bov.shape[2]
    evp = torch.full((ldv,), float("inf"), dtype=bov.dtype, device=bov.device)   # padded virtuals: D = -inf, T = 0
    evp[:ev.numel()] = ev
    v = torch.matmul(bov[i0:i0 + ni].transpose(1, 2)[:, None], bov[None])        # (ni, no, ldv, ldv)
    d = eo[i0:i0 + ni, None, None, None] + eo[None, :, None, None] - evp[None, None, :, None] - evp[None, None, None, :]
    t = v.div_(d)
    tt = (c_os + c_ss) * t - c_ss * t.transpose(2, 3)
    return t, tt


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


def one_shape(name, no, nv, naux, dev, peak_tflops, inner):
    ldv = (nv + 15) // 16 * 16
    g = torch.Generator(device="cpu").manual_seed(no * 1000 + nv)
    b = torch.zeros((no, naux, ldv), dtype=torch.float64)
    b[:, :, :nv] = torch.randn((no, naux, nv), dtype=torch.float64, generator=g) / naux ** 0.5
    b = b.to(dev)
    eo = torch.linspace(-11.0, -0.3, no, dtype=torch.float64, device=dev)
    ev = torch.linspace(0.1, 4.0, nv, dtype=torch.float64, device=dev)
    out = tuple(torch.empty(no * no * ldv * ldv, dtype=torch.float64, device=dev) for _ in range(2))
    kernel = lambda: lib.mp2_amplitudes(b, eo, ev, 0, no, out=out)  # noqa: E731
    build = lambda: unrelaxed_blocks(b, eo, ev, block=no)  # noqa: E731
    torchf = lambda: unrelaxed_blocks(b, eo, ev, block=no, amplitudes=torch_amplitudes)  # noqa: E731
    r_k, r_t = build(), torchf()
    diff = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(r_k[:3], r_t[:3]))
    del r_k, r_t
    for _ in range(2):
        timed(kernel, inner), timed(build, 1), timed(torchf, 1)
    t_k, t_b, t_t = [], [], []
    for _ in range(3):
        t_k.append(timed(kernel, inner))
        t_b.append(timed(build, 1))
        t_t.append(timed(torchf, 1))
    nt = ldv // 16
    flops = 2.0 * 2.0 * no * no * (nt * (nt + 1) / 2) * 256 * naux
    stored = 2.0 * 8.0 * no * no * ldv * ldv
    best = min(t_k)
    row = {"shape": name, "nocc": no, "nvir": nv, "ldv": ldv, "naux": naux, "bov_bytes": b.numel() * 8, "inner_kernel_calls": inner,
           "kernel_ms": t_k, "build_ms": t_b, "torch_build_ms": t_t,
           "kernel_stored_bytes": stored, "kernel_store_gbs_best": stored / (best * 1e-3) / 1e9,
           "kernel_flops": flops, "kernel_tflops_best": flops / (best * 1e-3) / 1e12,
           "kernel_share_of_mfma_probe": flops / (best * 1e-3) / 1e12 / peak_tflops,
           "torch_beats_build_in_any_pair_of_runs": min(t_t) < max(t_b),
           "max_diff_over_max_abs": diff}
    del out
    row["peak_extra_bytes_build"] = peak_extra(build)
    row["peak_extra_bytes_torch_build"] = peak_extra(torchf)
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
    shapes = [("toy", 3, 33, 41)] if small else [("c5-ccpvdz (benchmark molecule)", 46, 162, 1156), ("naphthalene-ccpvtz", 34, 378, 1440)]
    for name, no, nv, naux in shapes:
        out["shapes"].append(one_shape(name, no, nv, naux, dev, peak, 2 if small else 10))
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(out, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
