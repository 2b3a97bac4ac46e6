"""Time the bilinear derivative pass (dqc_eri_grad2) against the quadratic pass (dqc_eri_grad) on the same tables, and the stages of
dqc_amd.excited_gradient, on the 20-atom benchmark molecule (C5 / cc-pVDZ).

usage: python tools/gpu_excited_gradient_time.py [out.json] [--small]

  kernel    lib.eri_grad(D) against lib.eri_grad2(D, P) and against the three quadratic calls Q(D + P), Q(D), Q(P) that give the same
            polarisation term: after one warm-up of every side, three ALTERNATING repetitions, wall time around the call (all entry
            points end with a stream synchronise; their host work -- pair lists, uploads, the fold -- is the same and is inside every
            figure).  D is the converged SCF density, P a seeded symmetric matrix of its magnitude; the largest difference between
            2 eri_grad2(D, P) and the three-call result over the largest component is reported too.  The antisymmetric pair (jscale 0:
            no Coulomb loads) is timed beside them.
  stages    excited_gradient (CIS singlet, state 0) on the converged RHF calculation, twice, the second run warm with the excitation
            memo cleared: the excitations, the right-hand side with the Z-vector solve, `passes` = the three dqc_eri_grad2 passes with the
            one-electron call of the relaxed density (dqc_int1e_grad), the whole call.
--small: H2O / 3-21G, to rehearse the script."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dqc_amd  # noqa: E402
from dqc_amd import lib  # noqa: E402
from dqc_amd.excited import _gradient  # noqa: E402
from dqc_amd.gradient import _pulay_densities  # noqa: E402
from dqc_amd.response import state_memo  # noqa: E402
from tests import molecules as M  # noqa: E402


def wall(fcn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fcn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    mol = dqc_amd.Mol(M.H2O if small else M.c5_molecule(0), basis="3-21G" if small else "cc-pvdz", device=dev)
    qc = dqc_amd.HF(mol).run()
    out = {"device": torch.cuda.get_device_name(0), "molecule": "h2o-321g" if small else "c5-ccpvdz (benchmark molecule)"}
    h = qc._engine.hamilton
    tab = h._tab
    T = lib.cart2sph_matrix(tab, dev)
    ncart = int(T.shape[1])
    out.update(natm=int(tab.natm), ncart=ncart)
    d = T.T @ _pulay_densities(qc)[1].detach() @ T
    d = (0.5 * (d + d.T)).contiguous()
    g = torch.Generator(device="cpu").manual_seed(5)
    r = torch.randn((ncart, ncart), dtype=torch.float64, generator=g).to(dev)
    p = ((r + r.T) * (d.abs().max() / (r + r.T).abs().max())).contiguous()
    n = ((r - r.T) * (d.abs().max() / (r - r.T).abs().max())).contiguous()
    dp = (d + p).contiguous()
    res = {}

    def run(name, fcn):
        res[name] = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
        return wall(lambda: fcn(res[name]))

    def three(o):
        lib.eri_grad(o, dp, 1.0, tab)
        sub = torch.zeros_like(o)
        lib.eri_grad(sub, d, 1.0, tab)
        lib.eri_grad(sub, p, 1.0, tab)
        o -= sub

    sides = {"eri_grad(D)": lambda o: lib.eri_grad(o, d, 1.0, tab),
             "eri_grad2(D, P)": lambda o: lib.eri_grad2(o, d, p, 1.0, 1.0, tab),
             "three quadratic calls": three,
             "eri_grad2(N, N, 0, 1)": lambda o: lib.eri_grad2(o, n, n, 0.0, 1.0, tab)}
    for name, fcn in sides.items():
        run(name, fcn)
    times = {name: [] for name in sides}
    for _ in range(3):
        for name, fcn in sides.items():
            times[name].append(run(name, fcn))
    out["kernel_ms"] = times
    out["eri_grad2_over_eri_grad_best"] = min(times["eri_grad2(D, P)"]) / min(times["eri_grad(D)"])
    out["three_calls_over_eri_grad2_best"] = min(times["three quadratic calls"]) / min(times["eri_grad2(D, P)"])
    out["max_diff_over_max_abs"] = float((2.0 * res["eri_grad2(D, P)"] - res["three quadratic calls"]).abs().max()
                                         / res["three quadratic calls"].abs().max())
    print(json.dumps({k: out[k] for k in ("kernel_ms", "eri_grad2_over_eri_grad_best", "three_calls_over_eri_grad2_best",
                                          "max_diff_over_max_abs")}), flush=True)
    # the stages of excited_gradient (not through its memo: timed twice, the second run warm)
    qc.nuclear_gradient()
    stages = []
    for _ in range(2):
        memo = state_memo(qc)
        for key in [k for k in memo if isinstance(k, tuple) and k and k[0] == "excitations"]:
            del memo[key]
        t = {}
        with torch.no_grad():
            t["total"] = wall(lambda: _gradient(qc, 0, "singlet", True, None, 1e-8, 1e-9, times=t)) * 1e-3
        t["rest"] = t["total"] - t["excitations"] - t["z_vector"] - t["passes"]
        stages.append(t)
        print(json.dumps(t), flush=True)
    out["excited_gradient_seconds"] = stages
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(out, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
