"""Time the third-order functional kernel (dqc_xc_eval_kxc) against the second-order one (dqc_xc_eval_fxc, nvec = 1) on the same grid,
and the stages of dqc_amd.tddft_gradient, on the 20-atom benchmark molecule (C5 / cc-pVDZ) with PBE and PBE0.

usage: python tools/gpu_tddft_gradient_time.py [out.json] [--small]

  kernel    lib.xc_eval_fxc(terms, rho, grho, d rho) against lib.xc_eval_kxc(terms, rho, grho, d rho, d rho) with the ground-state density
            of the converged calculation and one response density on its grid: after one warm-up of either side, five ALTERNATING
            repetitions, HIP events around the call (lib.call_trace).
  stages    tddft_gradient (TDA singlet, state 0), twice, the second run warm with the excitation memo cleared: the excitations, the
            right-hand side with the Z-vector solve, the dqc_eri_grad2 passes (with dqc_int1e_grad), the three grid passes (AO evaluation and the potentials
            on the grid included), the weight term, the whole call.
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
from dqc_amd.response import orbital_hessian, state_memo  # noqa: E402
from tests import molecules as M  # noqa: E402


def wall(fcn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fcn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "molecule": "h2o-321g" if small else "c5-ccpvdz (benchmark molecule)"}
    for label, xc in (("pbe", "gga_x_pbe+gga_c_pbe"), ("pbe0", "pbe0")):
        mol = dqc_amd.Mol(M.H2O if small else M.c5_molecule(0), basis="3-21G" if small else "cc-pvdz", grid="sg2", device=dev)
        qc = dqc_amd.KS(mol, xc=xc).run()
        op = orbital_hessian(qc)
        h = qc._engine.hamilton
        rho, grho = op._rho[0]
        sp = op.spins[0]
        s = sp.co[:, -1:] @ sp.cv[:, :1].T      # the HOMO -> LUMO transition density
        dr, dg = lib.grid_density(h._ao, op.nao, lib.pad_matrix(0.5 * (s + s.T), h._ld), True)
        dr, dg = dr.unsqueeze(0), dg.unsqueeze(0)
        sides = {"dqc_xc_eval_fxc": lambda: lib.xc_eval_fxc(op.terms, rho, grho, dr, dg),
                 "dqc_xc_eval_kxc": lambda: lib.xc_eval_kxc(op.terms, rho, grho, dr, dg, dr, dg)}
        for f in sides.values():
            f()
        ms = {k: [] for k in sides}
        for _ in range(5):
            for k, f in sides.items():
                with lib.call_trace() as tr:
                    f()
                ms[k].append(tr.ms()[k][1])
        res = {"ngrid": int(rho.shape[0]), "nao": int(op.nao), "kernel_ms": ms,
               "kxc_over_fxc_best": min(ms["dqc_xc_eval_kxc"]) / min(ms["dqc_xc_eval_fxc"])}
        print(label, json.dumps(res), flush=True)
        qc.nuclear_gradient()
        stages = []
        for _ in range(2):
            memo = state_memo(qc)
            for key in [k for k in memo if isinstance(k, tuple) and k and k[0] == "excitations"]:
                del memo[key]
            t = {}
            with torch.no_grad():
                t["total"] = wall(lambda: _gradient(qc, 0, "singlet", True, None, 1e-8, 1e-9, times=t, who="tddft_gradient"))
            t["rest"] = t["total"] - sum(t[k] for k in ("excitations", "z_vector", "passes", "grid_passes", "weight_term"))
            stages.append(t)
            print(label, json.dumps(t), flush=True)
        res["tddft_gradient_seconds"] = stages
        out[label] = res
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(out, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
