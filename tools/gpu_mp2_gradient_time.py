"""Time the three-index-density derivative pass (dqc_df_grad3) against the rank-one pass (dqc_df_grad) on the same tables, and the
stages of dqc_amd.mp2_gradient, on the 20-atom benchmark molecule (C5 / cc-pVDZ, auxbasis "etb").

usage: python tools/gpu_mp2_gradient_time.py [out.json] [--small]

  kernel    lib.df_grad(D, c) against lib.df_grad3(Z = D (x) c, G = c c^T) in ONE call over the whole auxiliary range, and lib.df_grad3
            with Z alone and with G alone: after one warm-up of every side, three ALTERNATING repetitions, wall time around the call
            (both entry points end with a stream synchronise; their host work -- pair lists, uploads, the fold -- is the same and is
            inside both figures).  The largest difference of the two results over the largest component is reported too.
  stages    mp2_gradient on the converged RHF calculation: the relaxed density with its Z-vector solve, `separable` = the one-electron
            call and the one bilinear eri_grad2 pass of the relaxed density, the formation of Z and G (triangular solves, back-transformation, Cartesian transform), the dqc_df_grad3 passes, and
            the whole call; the number of auxiliary-shell blocks Z was walked in.
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
from dqc_amd.mp2 import _gradient  # noqa: E402
from dqc_amd.postscf import b_tensor  # noqa: E402
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
    df = b_tensor(qc, "etb")
    tab, orb, aux = df._tab, df._orb_range, df._aux_range
    ncart = lambda r: sum((int(l) + 1) * (int(l) + 2) // 2 for l in tab.bas[r[0]:r[1], 1])  # noqa: E731
    no, nk = ncart(orb), ncart(aux)
    out.update(natm=int(tab.natm) // 2, ncart_orbital=no, ncart_auxiliary=nk, z_bytes=8 * no * no * nk)
    g = torch.Generator(device="cpu").manual_seed(5)
    d = torch.randn((no, no), dtype=torch.float64, generator=g) / no
    d = (d + d.t()).to(dev)
    c = (0.1 * torch.randn(nk, dtype=torch.float64, generator=g)).to(dev)
    dbig = torch.zeros((no + nk, no + nk), dtype=torch.float64, device=dev)
    dbig[:no, :no] = d
    cbig = torch.zeros(no + nk, dtype=torch.float64, device=dev)
    cbig[no:] = c
    z = (d[:, :, None] * c[None, None, :]).contiguous()
    gm = torch.outer(c, c).contiguous()
    res = {}

    def run(name, fcn):
        res[name] = torch.zeros((tab.natm, 3), dtype=torch.float64, device=dev)
        return wall(lambda: fcn(res[name]))

    sides = {"df_grad": lambda o: lib.df_grad(o, dbig, cbig, tab, orb, aux),
             "df_grad3": lambda o: lib.df_grad3(o, z, gm, tab, orb, aux),
             "df_grad3_z_alone": lambda o: lib.df_grad3(o, z, None, tab, orb, aux),
             "df_grad3_g_alone": lambda o: lib.df_grad3(o, None, gm, tab, orb, aux)}
    for name, fcn in sides.items():
        run(name, fcn)
    times = {name: [] for name in sides}
    for _ in range(3):
        for name, fcn in sides.items():
            times[name].append(run(name, fcn))
    out["kernel_ms"] = times
    out["df_grad3_over_df_grad_best"] = min(times["df_grad3"]) / min(times["df_grad"])
    out["max_diff_over_max_abs"] = float((res["df_grad3"] - res["df_grad"]).abs().max() / res["df_grad"].abs().max())
    print(json.dumps({k: out[k] for k in ("kernel_ms", "df_grad3_over_df_grad_best", "max_diff_over_max_abs")}), flush=True)
    del z, dbig
    # the stages of mp2_gradient (not through the memo: timed twice, the second run warm)
    qc.nuclear_gradient()
    stages = []
    for _ in range(2):
        t = {}
        with torch.no_grad():
            t["total"] = wall(lambda: _gradient(qc, "etb", 1.0, 1.0, 1e-9, None, times=t)) * 1e-3
        stages.append(t)
        print(json.dumps(t), flush=True)
    out["mp2_gradient_seconds"] = stages
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        json.dump(out, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
