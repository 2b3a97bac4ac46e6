"""Time of ONE restricted Fock build on the C5 molecule (vitamin C, cc-pVDZ, nao 208, sg3 grid): pure Kohn-Sham PBE, restricted
Hartree-Fock (the J + K tile stream) and, where this tree has hybrids, PBE0 -- the yardstick of docs/LOG_r08.md: a hybrid build
should cost about the pure-KS build plus the difference between the J + K and the J-only tile streams.

Each build is `ao_orb2dm(C_occ) -> dm2scp(D)` as the SCF drivers issue it, eagerly on one stream, timed with device events over
`--reps` builds after `--warmup`; the legs alternate for `--rounds` rounds so that clock drift and neighbours hit them alike.
Prints one JSON line.  usage: python tools/gpu_hybrid_build_time.py [--rounds 5] [--reps 50] [--warmup 10] [--tag NAME]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: no timing is taken without one")
    import dqc_amd
    from tests import molecules as M
    mol = lambda: dqc_amd.Mol(M.c5_molecule(0), basis="cc-pvdz", grid="sg3")  # noqa: E731
    legs = {"ks_pbe": dqc_amd.KS(mol(), xc="gga_x_pbe+gga_c_pbe"), "rhf": dqc_amd.HF(mol())}
    try:
        legs["ks_pbe0"] = dqc_amd.KS(mol(), xc="pbe0")
    except ValueError:  # a tree without hybrid functionals: the two yardsticks alone
        pass
    states = {}
    for name, qc in legs.items():
        eng = qc._engine
        dm = eng.scp2dm(eng.dm2scp(torch.zeros(eng.shape, dtype=eng.dtype, device=eng.device)))
        orb = eng.scp2orb(eng.dm2scp(dm)).contiguous()  # occupied orbitals of a sensible density
        states[name] = (eng, orb)

    def build(name):
        eng, orb = states[name]
        return eng.dm2scp(eng.hamilton.ao_orb2dm(orb, eng.orb_weight))

    for name in states:
        for _ in range(a.warmup):
            build(name)
    torch.cuda.synchronize()
    out = {name: [] for name in states}
    for _ in range(a.rounds):
        for name in states:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                build(name)
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / a.reps)
    res = {"tag": a.tag, "molecule": "c5_molecule(0) / cc-pVDZ / sg3", "nao": int(states["rhf"][0].shape[-1]), "reps": a.reps,
           "ms_per_build": {k: [round(x, 4) for x in v] for k, v in out.items()},
           "median_ms": {k: round(sorted(v)[len(v) // 2], 4) for k, v in out.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
