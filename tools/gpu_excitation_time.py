"""Cost of the paired linear-response product OrbitalHessian.mm_pair ((A+B) k and (A-B) k from one jk_multi call) against the
Hessian-vector product OrbitalHessian.mm on the same 4 trial vectors: benzene / cc-pVDZ, RHF and PBE0 (and PBE, where A-B is the
diagonal).  Prints one line per method: ms per call (median of 5 after 2 warm-up calls) and the number of kernel launches of one call
(torch profiler, when available).
usage: python tools/gpu_excitation_time.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import dqc_amd  # noqa: E402
from dqc_amd.response import OrbitalHessian  # noqa: E402
from tests import molecules as M  # noqa: E402


def timed(fn, reps=5):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def launches(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # the profiler is a convenience here, the times are the result
        return "n/a (%s)" % type(exc).__name__


if __name__ == "__main__":
    for label, make in (("RHF", lambda m: dqc_amd.HF(m)), ("PBE0", lambda m: dqc_amd.KS(m, xc="pbe0")),
                        ("PBE", lambda m: dqc_amd.KS(m, xc="gga_x_pbe+gga_c_pbe"))):
        qc = make(dqc_amd.Mol(M.benzene(), basis="cc-pvdz", grid="sg2")).run()
        H = OrbitalHessian(qc)
        g = torch.Generator().manual_seed(1)
        k = torch.randn((4, H.n), generator=g, dtype=torch.float64).to("cuda")
        t_mm, t_pair, t_minus = timed(lambda: H.mm(k)), timed(lambda: H.mm_pair(k)), timed(lambda: H.mm_minus(k))
        print("benzene/cc-pVDZ %-5s n %5d  4 vectors: mm %.3f ms  mm_pair %.3f ms (%.2f x)  mm_minus %.3f ms  launches mm %s  mm_pair %s" % (
            label, H.n, t_mm, t_pair, t_pair / t_mm, t_minus, launches(lambda: H.mm(k)), launches(lambda: H.mm_pair(k))), flush=True)
