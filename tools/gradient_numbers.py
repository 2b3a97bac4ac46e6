"""The numbers of every gradient entry point on one small molecule, as JSON, and the comparison of such files between two commits.

usage: python tools/gradient_numbers.py out.json [--fd]
       python tools/gradient_numbers.py --compare base_a.json base_b.json head.json

First form (GPU): distorted H2O / 3-21G (the geometry of the gradient tests; grid "sg2" for Kohn-Sham), tight SCF.  Written to out.json:
nuclear_gradient for RHF, RKS LDA, RKS PBE, RKS SCAN and UKS PBE (the triplet); basis_gradient for RKS PBE; mp2_gradient(auxbasis="etb");
excited_gradient for a TDA singlet and a TDHF triplet; tddft_gradient for PBE and PBE0 (TDA singlets); the dipoles of the SCF density
(edipole), of the relaxed MP2 density and of the relaxed excited state, in atomic units.  Public entry points only, so that the script
runs unchanged on an older commit.  --fd adds the Richardson-extrapolated central difference (h = 1e-3 and 2e-3 Bohr) of the RI-MP2 total
energy for the four components of tests/test_gpu_mp2_gradient.py.

Second form (no GPU): base_a and base_b are two runs of the base commit, each in a fresh process; the largest difference between them is
the noise floor of a quantity (atomics: two runs differ in the last digits).  For every quantity but mp2_gradient the head must stay
within ten floors of base_a (a zero floor counts as 1e-13 of the largest element); for mp2_gradient, whose separable term changed from
a difference of two quadratic passes to one bilinear pass, the distance of either commit from the finite difference is printed and the
head must not be farther from it than the base (by more than ten floors: below that the two are the same number).  Exit status 1 when a
quantity misses."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ZS = [8, 1, 1]
POS = [[0.0, 0.0, 0.2217], [0.0, 1.4309, -0.8867], [0.1, -1.4309, -0.8867]]
TIGHT = {"maxiter": 300, "f_tol": 1e-11}
FD_COMPONENTS = [(0, 2), (1, 1), (2, 0), (2, 2)]


def numbers(fd):
    import torch
    import dqc_amd
    assert torch.cuda.is_available(), "the numbers are those of the GPU"
    lst = lambda t: t.detach().cpu().tolist()  # noqa: E731

    def mol(pos=POS, **kw):
        return dqc_amd.Mol((ZS, pos), basis="3-21G", **kw)

    def ks(xc, restricted=None, **kw):
        return dqc_amd.KS(mol(grid="sg2", **kw), xc=xc, restricted=restricted).run(fwd_options=TIGHT)

    out = {}
    hf = dqc_amd.HF(mol()).run(fwd_options=TIGHT)
    pbe = ks("gga_x_pbe+gga_c_pbe")
    pbe0 = ks("pbe0")
    out["nuclear_gradient rhf"] = lst(hf.nuclear_gradient())
    out["nuclear_gradient rks lda"] = lst(ks("lda_x+lda_c_pw").nuclear_gradient())
    out["nuclear_gradient rks pbe"] = lst(pbe.nuclear_gradient())
    out["nuclear_gradient rks scan"] = lst(ks("mgga_x_scan").nuclear_gradient())
    out["nuclear_gradient uks pbe"] = lst(ks("gga_x_pbe+gga_c_pbe", spin=2, restricted=False).nuclear_gradient())
    out["basis_gradient rks pbe"] = lst(pbe.basis_gradient())
    g = dqc_amd.mp2_gradient(hf, auxbasis="etb")
    out["mp2_gradient"] = lst(g.gradient)
    out["dipole mp2 relaxed"] = lst(g.density.dipole(unit=None))
    out["dipole scf rhf"] = lst(dqc_amd.edipole(hf, unit=None))
    e = dqc_amd.excited_gradient(hf, state=0, spin="singlet", tda=True)
    out["excited_gradient tda singlet"] = lst(e.gradient)
    out["dipole excited tda singlet"] = lst(e.density.dipole(unit=None))
    out["excited_gradient tdhf triplet"] = lst(dqc_amd.excited_gradient(hf, state=0, spin="triplet", tda=False).gradient)
    out["tddft_gradient pbe"] = lst(dqc_amd.tddft_gradient(pbe, state=0, tda=True).gradient)
    out["tddft_gradient pbe0"] = lst(dqc_amd.tddft_gradient(pbe0, state=0, tda=True).gradient)
    if fd:
        rich = {}
        for atom, d in FD_COMPONENTS:
            e = {}
            for m in (1, -1, 2, -2):
                pos = [list(p) for p in POS]
                pos[atom][d] += m * 1e-3
                e[m] = float(dqc_amd.mp2(dqc_amd.HF(mol(pos)).run(fwd_options=TIGHT), auxbasis="etb").e_tot)
            f1, f2 = (e[1] - e[-1]) / 2e-3, (e[2] - e[-2]) / 4e-3
            rich["%d,%d" % (atom, d)] = [(4.0 * f1 - f2) / 3.0, abs(f1 - f2)]
        out["mp2 richardson"] = rich
    return out


def compare(a, b, head):
    import numpy as np
    ok = True
    for key in a:
        if key == "mp2 richardson":
            continue
        x, y, z = (np.asarray(m[key], dtype=float) for m in (a, b, head))
        floor, diff, scale = float(np.abs(x - y).max()), float(np.abs(z - x).max()), float(np.abs(x).max())
        if key == "mp2_gradient":
            print("%-32s base runs apart %.2e   head - base %.2e   max |x| %.3e" % (key, floor, diff, scale))
            rich = head.get("mp2 richardson") or a.get("mp2 richardson") or b.get("mp2 richardson")
            assert rich, "one of the files must come from a run with --fd"
            for comp, (fr, spread) in sorted(rich.items()):
                i, j = (int(s) for s in comp.split(","))
                db, dh = abs(x[i, j] - fr), abs(z[i, j] - fr)
                noise = 10.0 * max(floor, 1e-13 * scale)   # (what two runs of the base differ by says nothing about either)
                verdict = "head is closer" if dh <= db else "equal within the noise of the base" if dh - db <= noise else "HEAD IS FARTHER"
                ok &= dh - db <= noise
                print("    (%s)  Richardson % .10f (|FD(h) - FD(2h)| %.1e)   |base - FD| %.3e   |head - FD| %.3e   %s"
                      % (comp, fr, spread, db, dh, verdict))
            continue
        bound = 10.0 * floor if floor > 0.0 else 1e-13 * scale
        good = diff <= bound
        ok &= good
        print("%-32s base runs apart %.2e   head - base %.2e   bound %.2e   max |x| %.3e   %s"
              % (key, floor, diff, bound, scale, "ok" if good else "MISSES"))
    return ok


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--compare" in sys.argv:
        a, b, head = (json.load(open(p)) for p in args)
        sys.exit(0 if compare(a, b, head) else 1)
    out = numbers("--fd" in sys.argv)
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    json.dump(out, open(args[0], "w"), indent=1)
    print("wrote %d quantities to %s" % (len(out), args[0]))


if __name__ == "__main__":
    main()
