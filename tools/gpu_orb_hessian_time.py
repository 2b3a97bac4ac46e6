"""Timings of the orbital-Hessian product (dqc_amd/response.py) against one ordinary Fock build of the same molecule on the same
commit: benzene / cc-pVDZ and molecule 0 of the C5 batch (vitamin C / cc-pVDZ), RKS PBE on sg2.

    fock      one Fock build of the converged density (eng.dm2scp), the yardstick; every call gets a fresh copy of the density, as
              an SCF iteration does, so that the per-density memos of the Hamiltonian are not hit
    mm1, mm8  one H.mm with 1 and with 8 trial vectors
    fxc1/8    the second-order functional kernel alone on the molecule's grid (dqc_xc_eval_fxc), 1 and 8 vectors
    is_orb_min  the whole stability check (block Davidson, memo cleared)

Every shape is warmed up first; a figure is the median over `--repeats` windows of (device time between two events recorded on
the stream) / (calls in the window).  The windows of the millisecond-scale functional kernel hold `--inner` calls, so that launch
and event overhead do not carry the figure; `is_orb_min` synchronises with the host by itself and is one call per window.
Expectation (derived): mm1 ~ one Fock build (one tile pass, one density pass, one Vxc GEMM), mm8 well under 8 x mm1 (the tile
stream is read once).  Prints one JSON line per molecule.      usage: python tools/gpu_orb_hessian_time.py [--repeats 9] [--inner 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import dqc_amd  # noqa: E402
from dqc_amd import lib  # noqa: E402
from dqc_amd.response import OrbitalHessian  # noqa: E402
from tests import molecules as M  # noqa: E402


def timed(fn, repeats, inner=1, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def one(name, mol, repeats, inner):
    m = dqc_amd.Mol(mol, basis="cc-pvdz", grid="sg2")
    qc = dqc_amd.KS(m, xc="gga_x_pbe+gga_c_pbe").run()
    eng = qc._engine
    dm = qc.aodm()
    H = OrbitalHessian(qc)
    g = torch.Generator(device="cpu").manual_seed(1)
    k8 = torch.randn((8, H.n), generator=g, dtype=torch.float64).to(eng.device)
    rho, grho = H._rho[0]
    drho, dgrho = torch.stack([rho * 0.1] * 8), torch.stack([grho * 0.1] * 8)
    out = {"molecule": name, "nao": H.nao, "ngrid": int(rho.shape[0]), "nparam": H.n, "ms": {}}

    def stability():
        qc.__dict__.pop("_response_memo", None)
        return dqc_amd.is_orb_min(qc)
    for key, fn, n_in in (("fock", lambda: eng.dm2scp(dm.clone()), 1), ("mm1", lambda: H.mm(k8[:1]), 1), ("mm8", lambda: H.mm(k8), 1),
                          ("fxc1", lambda: lib.xc_eval_fxc(H.terms, rho, grho, drho[:1], dgrho[:1]), inner),
                          ("fxc8", lambda: lib.xc_eval_fxc(H.terms, rho, grho, drho, dgrho), inner), ("is_orb_min", stability, 1)):
        med, lo, hi = timed(fn, repeats if key != "is_orb_min" else max(3, repeats // 2), n_in, warm=3 if key != "is_orb_min" else 1)
        out["ms"][key] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
    f = out["ms"]["fock"]["median"]
    out["ratio_mm1_to_fock"] = round(out["ms"]["mm1"]["median"] / f, 3)
    out["ratio_mm8_to_mm1"] = round(out["ms"]["mm8"]["median"] / out["ms"]["mm1"]["median"], 3)
    out["ratio_fxc1_to_fock"] = round(out["ms"]["fxc1"]["median"] / f, 4)
    out["ratio_is_orb_min_to_fock"] = round(out["ms"]["is_orb_min"]["median"] / f, 2)
    out["stable"] = bool(stability())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    one("benzene", M.benzene(), a.repeats, a.inner)
    one("c5[0] vitamin C", M.c5_molecule(0), a.repeats, a.inner)
