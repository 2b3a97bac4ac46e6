"""Fixtures for the hybrid functionals (exact-exchange fraction a): a CPU hybrid SCF COMPOSED from the oracle's own, separately
pinned operators -- F = h + J[D] + a get_exchange(D) + Vxc[f_a](D), get_exchange = -K / 2 (oracle/hamilton.py; per spin
get_exchange(2 D_s)), f_a the grid part of the functional -- iterated with the oracle engines' own DIIS loops to 1e-11.
The reference has no hybrid functionals, so there is no reference literal; every operator used here is one the parity suite
already pins.  Imports `oracle` only, never dqc_amd.  Writes

    tests/golden/oracle_hybrid.json        converged energies, energy parts, AO Fock / density matrices, finite-difference
                                           gradients (h = 1e-3 Bohr, Becke cut off as in tools/make_grad_golden.py)
    tests/golden/oracle_hybrid_builds.npz  single Fock builds of seeded densities (tests.molecules.seeded_dm_ao)

usage: python tools/make_hybrid_golden.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import hamilton as oh, grid as og, basis as ob  # noqa: E402
from tests import molecules as M  # noqa: E402

# name -> (grid part in the oracle's spelling, exact-exchange fraction)
FUNCTIONALS = {
    "pbe0": ("0.75 * gga_x_pbe + gga_c_pbe", 0.25),
    "b3lyp5": ("0.08 * lda_x + 0.72 * gga_x_b88 + 0.19 * lda_c_vwn + 0.81 * gga_c_lyp", 0.20),
    "hf37pbe": ("0.63 * gga_x_pbe + gga_c_pbe", 0.37),
    "hf": (None, 1.0),
}
H2O_D = ([8, 1, 1], [[0, 0, 0.2217], [0, 1.4309, -0.8867], [0.1, -1.4309, -0.8867]])
LIH = ([3, 1], [[0, 0.1, -1.5], [0, 0, 1.5]])
CH3 = ([6, 1, 1, 1], [[0, 0, 0.05], [2.039, 0, 0], [-1.0195, 1.7658, 0], [-1.0195, -1.7658, 0.1]])


class HybridRKS(oh.Engine):
    """restricted: the oracle's engine and SCF loop with F = h + J + a get_exchange + Vxc[f_a]"""

    def __init__(self, tables, gridxc, a, grid):
        super().__init__(tables, xc=gridxc, grid=grid)  # (gridxc None: no grid is set up)
        self.a, self.has_grid = float(a), gridxc is not None

    def dm2scp(self, dm):
        F = self.h.kinnucl_mat + self.h.get_elrep(dm) + self.a * self.h.get_exchange(dm)
        return F + self.h.get_vxc(dm) if self.has_grid else F

    def energy_parts(self, dm):
        p = {"e_core": float(self.h.get_e_hcore(dm)), "e_elrep": float(self.h.get_e_elrep(dm)), "e_nuc": self.enuc,
             "e_exch": self.a * float(self.h.get_e_exchange(dm)), "e_xc": float(self.h.get_e_xc(dm)) if self.has_grid else 0.0}
        p["e_tot"] = sum(p.values())
        return p

    def dm2energy(self, dm):
        return self.energy_parts(dm)["e_tot"]


class HybridUKS(oh.EnginePol):
    """unrestricted: J from the total density, a get_exchange(2 D_s) = -a K[D_s] and Vxc_s per spin"""

    def __init__(self, tables, spin, gridxc, a, grid):
        super().__init__(tables, spin, xc=gridxc, grid=grid)
        self.a = float(a)

    def dm2scp(self, dm):
        dmu, dmd = dm
        core = self.h.kinnucl_mat + self.h.get_elrep(dmu + dmd)
        vu, vd, _ = self._vxc(dmu, dmd)
        return torch.stack([core + vu + self.a * self.h.get_exchange(2 * dmu), core + vd + self.a * self.h.get_exchange(2 * dmd)])

    def energy_parts(self, dm):
        dmu, dmd = dm
        tot = dmu + dmd
        ex = 0.5 * torch.sum(self.h.get_exchange(2 * dmu) * dmu) + 0.5 * torch.sum(self.h.get_exchange(2 * dmd) * dmd)
        p = {"e_core": float(self.h.get_e_hcore(tot)), "e_elrep": float(self.h.get_e_elrep(tot)), "e_nuc": self.enuc,
             "e_exch": self.a * float(ex), "e_xc": self._vxc(dmu, dmd)[2]}
        p["e_tot"] = sum(p.values())
        return p

    def dm2energy(self, dm):
        return self.energy_parts(dm)["e_tot"]


def _ao(h, t, m):
    """orthogonal-basis operator -> AO basis, S X m X^T S (independent of the choice of X)"""
    S = torch.as_tensor(oh.natives.int1e("ovlp", t))
    SX = S @ h.X
    return (SX @ m @ SX.T).numpy()


def scf(mol, basis, fn, grid, spin=None):
    gridxc, a = FUNCTIONALS[fn]
    t = ob.make_tables(mol, basis)
    if spin is None:
        eng = HybridRKS(t, gridxc, a, grid)
        eng.run(maxiter=300, tol=1e-11)
        dm = eng.dm
        fock = eng.dm2scp(dm)
        comm = float((fock @ dm - dm @ fock).abs().max())
        out = {"fock_ao": _ao(eng.h, t, fock).tolist(), "dm_ao": eng.h.unconvert_dm(dm).numpy().tolist()}
    else:
        eng = HybridUKS(t, spin, gridxc, a, grid)
        eng.run(maxiter=300, tol=1e-11)
        dm = eng.dm
        fock = eng.dm2scp(dm)
        comm = max(float((fock[s] @ dm[s] - dm[s] @ fock[s]).abs().max()) for s in range(2))
        out = {"fock_ao": [_ao(eng.h, t, fock[s]).tolist() for s in range(2)],
               "dm_ao": [eng.h.unconvert_dm(dm[s]).numpy().tolist() for s in range(2)]}
    out.update(eng.energy_parts(dm))
    out["commutator"] = comm
    return out


def fd_gradient(mol, basis, fn, grid, spin, h=1e-3):
    zs, pos = mol[0], np.array(mol[1], dtype=np.float64)
    g = np.zeros_like(pos)
    for i in range(len(zs)):
        for d in range(3):
            e = []
            for sgn in (1, -1):
                p = pos.copy()
                p[i, d] += sgn * h
                e.append(scf((zs, p.tolist()), basis, fn, grid, spin)["e_tot"])
            g[i, d] = (e[0] - e[1]) / (2 * h)
    return g


def single_builds():
    """F (AO basis) and the energy parts of seeded densities: H2O and benzene / cc-pVDZ, restricted; H2O unrestricted"""
    out = {}
    for name, mol, seed in (("h2o", M.H2O, 11), ("benzene", M.benzene(), 12)):
        t = ob.make_tables(mol, "cc-pvdz")
        nel = int(sum(mol[0]))
        for fn in ("pbe0", "b3lyp5", "hf37pbe"):
            gridxc, a = FUNCTIONALS[fn]
            eng = HybridRKS(t, gridxc, a, "sg2")
            S = torch.as_tensor(oh.natives.int1e("ovlp", t))
            SX = S @ eng.h.X
            dm = SX.T @ torch.as_tensor(M.seeded_dm_ao(t.nao, nel, S.numpy(), seed)) @ SX
            p = eng.energy_parts(dm)
            key = "%s_%s_" % (name, fn)
            out[key + "fock_ao"] = _ao(eng.h, t, eng.dm2scp(dm))
            out[key + "parts"] = np.array([p["e_core"], p["e_elrep"], p["e_exch"], p["e_xc"]])
            if name == "h2o":  # unrestricted: two different seeded spin densities
                ep = HybridUKS(t, 0, gridxc, a, "sg2")
                du = SX.T @ torch.as_tensor(M.seeded_dm_ao(t.nao, nel, S.numpy(), seed + 100)) @ SX * 0.5
                dd = SX.T @ torch.as_tensor(M.seeded_dm_ao(t.nao, nel - 2, S.numpy(), seed + 200)) @ SX * 0.5
                f = ep.dm2scp((du, dd))
                p = ep.energy_parts((du, dd))
                out[key + "ufock_ao"] = np.stack([_ao(ep.h, t, f[0]), _ao(ep.h, t, f[1])])
                out[key + "uparts"] = np.array([p["e_core"], p["e_elrep"], p["e_exch"], p["e_xc"]])
            print("build %-22s done" % key, flush=True)
    return out


CONVERGED = {
    # name: (mol, basis, functional, grid, spin)
    "h2o-321g-pbe0": (H2O_D, "3-21G", "pbe0", 3, None),
    "h2o-321g-b3lyp5": (H2O_D, "3-21G", "b3lyp5", 3, None),
    "lih-321g-pbe0": (LIH, "3-21G", "pbe0", "sg2", None),
    "lih-321g-b3lyp5": (LIH, "3-21G", "b3lyp5", "sg2", None),
    "h2o-ccpvdz-pbe0": (M.H2O, "cc-pvdz", "pbe0", "sg2", None),
    "ch3-321g-upbe0": (CH3, "3-21G", "pbe0", 3, 1),
    "ch3-321g-ub3lyp5": (CH3, "3-21G", "b3lyp5", 3, 1),
    "h2o-321g-upbe0-closed": (H2O_D, "3-21G", "pbe0", 3, 0),
}
GRADIENTS = {"h2o-321g-pbe0": (H2O_D, "3-21G", "pbe0", 3, None), "ch3-321g-upbe0": (CH3, "3-21G", "pbe0", 3, 1)}


if __name__ == "__main__":
    out = {"_how": __doc__, "h": 1e-3, "functionals": {k: {"grid_part": v[0], "exx_fraction": v[1]} for k, v in FUNCTIONALS.items()},
           "converged": {}, "gradients": {}}
    # the golden file's own consistency: a = 1 and no grid term on the geometry of the committed RHF fixture
    ref = np.load(os.path.join(ROOT, "tests", "golden", "ref_h2o_sto3g_rhf.npz"))
    mol = ([int(z) for z in ref["atomzs"]], ref["atompos"].tolist())
    r = scf(mol, "sto-3g", "hf", 3)
    out["converged"]["h2o-sto3g-hf"] = dict(r, atomzs=mol[0], atompos=mol[1], basis="sto-3g", functional="hf", grid=None, spin=None)
    print("h2o-sto3g-hf  e_tot %.12f  fixture %.12f" % (r["e_tot"], float(ref["e_tot"])), flush=True)
    for name, (mol, basis, fn, grid, spin) in CONVERGED.items():
        t0 = time.time()
        r = scf(mol, basis, fn, grid, spin)
        out["converged"][name] = dict(r, atomzs=mol[0], atompos=mol[1], basis=basis, functional=fn, grid=grid, spin=spin)
        print("%-24s %.1f s  e_tot %.10f  |[F,D]| %.1e" % (name, time.time() - t0, r["e_tot"], r["commutator"]), flush=True)
    og.BECKE_CUT = 2.0
    for name, (mol, basis, fn, grid, spin) in GRADIENTS.items():
        t0 = time.time()
        g = fd_gradient(mol, basis, fn, grid, spin)
        out["gradients"][name] = {"atomzs": mol[0], "atompos": mol[1], "basis": basis, "functional": fn, "grid": grid, "spin": spin,
                                  "becke_cut": "off", "gradient": g.tolist()}
        print("%-24s %.1f s  max|g| %.5f  sum %.1e" % (name, time.time() - t0, np.abs(g).max(), np.abs(g.sum(0)).max()), flush=True)
    og.BECKE_CUT = 0.74
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "oracle_hybrid.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "oracle_hybrid_builds.npz"), **single_builds())
