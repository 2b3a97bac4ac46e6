"""Fixtures for density-fitted exchange (RI-K, Mol.densityfit(exchange=True)): a CPU SCF COMPOSED from the oracle's own operators --
F = h + J_df[D] + a (-K_df[D] / 2) (+ Vxc[f_a](D)), per spin -a K_df[D_s] -- iterated with the oracle engines' own DIIS loops to
1e-11.  J_df is the oracle's fitted Coulomb operator (oracle/hamilton.py, pinned against the reference's DFMol); K_df is formed
here in numpy from the oracle's j2c / j3c,

    K_df[mu, nu] = sum_{lam, sig, Q} (mu lam|Q) [j2c^-1 (nu sig|.)]_Q D[lam, sig],      np.linalg.solve, no explicit inverse

and the grid part is the oracle's Vxc.  The reference has no fitted exchange, so there is no reference literal.  Imports `oracle`
only, never dqc_amd.  Writes tests/golden/oracle_dfk.json: converged energies and energy parts.

usage: python tools/make_dfk_golden.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import hamilton as oh, basis as ob  # noqa: E402
from tests import molecules as M  # noqa: E402

# name -> (grid part in the oracle's spelling, exact-exchange fraction)
FUNCTIONALS = {"pbe0": ("0.75 * gga_x_pbe + gga_c_pbe", 0.25), "hf": (None, 1.0)}
CH3 = ([6, 1, 1, 1], [[0, 0, 0.05], [2.039, 0, 0], [-1.0195, 1.7658, 0], [-1.0195, -1.7658, 0.1]])


class FittedK:
    """K_df of an orthogonal-basis density from a density-fitted oracle Hamiltonian's j2c / j3c"""

    def __init__(self, hdf):
        self.h = hdf
        j3c, j2c = hdf.j3c.numpy(), hdf.j2c.numpy()
        self.nao, self.naux = j3c.shape[0], j3c.shape[2]
        self.j3c = j3c
        self.cfit = np.linalg.solve(j2c, j3c.reshape(-1, self.naux).T).reshape(self.naux, self.nao, self.nao)  # [Q, nu, sig]

    def __call__(self, dm):
        dao = self.h.unconvert_dm(dm).numpy()
        dao = (dao + dao.T) * 0.5
        t = np.einsum("mlq,ls->msq", self.j3c, dao)
        k = np.einsum("msq,qns->mn", t, self.cfit)
        return self.h.convert2(torch.as_tensor((k + k.T) * 0.5))


class FittedRKS(oh.Engine):
    """restricted: F = h + J_df + a (-K_df / 2) + Vxc[f_a]"""

    def __init__(self, tables, df, gridxc, a, grid):
        super().__init__(tables, xc=gridxc, grid=grid, df=df)  # (gridxc None: no grid is set up)
        self.a, self.has_grid, self.kdf = float(a), gridxc is not None, FittedK(self.h)

    def dm2scp(self, dm):
        F = self.h.kinnucl_mat + self.h.get_elrep(dm) - 0.5 * self.a * self.kdf(dm)
        return F + self.h.get_vxc(dm) if self.has_grid else F

    def energy_parts(self, dm):
        p = {"e_core": float(self.h.get_e_hcore(dm)), "e_elrep": float(self.h.get_e_elrep(dm)), "e_nuc": self.enuc,
             "e_exch": -0.25 * self.a * float(torch.sum(self.kdf(dm) * dm)), "e_xc": float(self.h.get_e_xc(dm)) if self.has_grid else 0.0}
        p["e_tot"] = sum(p.values())
        return p

    def dm2energy(self, dm):
        return self.energy_parts(dm)["e_tot"]


class FittedUKS(oh.EnginePol):
    """unrestricted: J_df from the total density, -a K_df[D_s] and Vxc_s per spin (the grid lives on the engine's own Hamiltonian,
    J_df and K_df come from a second, density-fitted one over the same orbital tables)"""

    def __init__(self, tables, df, spin, gridxc, a, grid):
        super().__init__(tables, spin, xc=gridxc, grid=grid)
        self.a, self.has_grid = float(a), gridxc is not None
        self.hdf = oh.Hamilton(tables, df=df).build()
        self.kdf = FittedK(self.hdf)

    def dm2scp(self, dm):
        dmu, dmd = dm
        core = self.h.kinnucl_mat + self.hdf.get_elrep(dmu + dmd)
        vu, vd = self._vxc(dmu, dmd)[:2] if self.has_grid else (0.0, 0.0)
        return torch.stack([core + vu - self.a * self.kdf(dmu), core + vd - self.a * self.kdf(dmd)])

    def energy_parts(self, dm):
        dmu, dmd = dm
        tot = dmu + dmd
        ex = -0.5 * (torch.sum(self.kdf(dmu) * dmu) + torch.sum(self.kdf(dmd) * dmd))
        p = {"e_core": float(self.h.get_e_hcore(tot)), "e_elrep": float(self.hdf.get_e_elrep(tot)), "e_nuc": self.enuc,
             "e_exch": self.a * float(ex), "e_xc": self._vxc(dmu, dmd)[2] if self.has_grid else 0.0}
        p["e_tot"] = sum(p.values())
        return p

    def dm2energy(self, dm):
        return self.energy_parts(dm)["e_tot"]


def scf(mol, basis, fn, grid, spin=None):
    gridxc, a = FUNCTIONALS[fn]
    t = ob.make_tables(mol, basis)
    df = ob.make_tables_df(mol, basis, "etb")
    if spin is None:
        eng = FittedRKS(t, df, gridxc, a, grid)
        eng.run(maxiter=300, tol=1e-11)
        dm = eng.dm
        fock = eng.dm2scp(dm)
        comm = float((fock @ dm - dm @ fock).abs().max())
    else:
        eng = FittedUKS(t, df, spin, gridxc, a, grid)
        eng.run(maxiter=300, tol=1e-11)
        dm = eng.dm
        fock = eng.dm2scp(dm)
        comm = max(float((fock[s] @ dm[s] - dm[s] @ fock[s]).abs().max()) for s in range(2))
    out = dict(eng.energy_parts(dm))
    out["commutator"] = comm
    out["naux"] = int(eng.kdf.naux)
    return out


CONVERGED = {
    # name: (mol, basis, functional, grid, spin)
    "h2o-ccpvdz-rihf": (M.H2O, "cc-pvdz", "hf", "sg2", None),
    "h2o-ccpvdz-ripbe0": (M.H2O, "cc-pvdz", "pbe0", "sg2", None),
    "ch3-321g-riuhf": (CH3, "3-21G", "hf", "sg2", 1),
    "ch3-321g-riupbe0": (CH3, "3-21G", "pbe0", "sg2", 1),
}


if __name__ == "__main__":
    out = {"_how": __doc__, "auxbasis": "etb", "functionals": {k: {"grid_part": v[0], "exx_fraction": v[1]} for k, v in FUNCTIONALS.items()},
           "converged": {}}
    for name, (mol, basis, fn, grid, spin) in CONVERGED.items():
        t0 = time.time()
        r = scf(mol, basis, fn, grid, spin)
        out["converged"][name] = dict(r, atomzs=[int(z) for z in mol[0]], atompos=[list(map(float, p)) for p in mol[1]], basis=basis,
                                      functional=fn, grid=grid, spin=spin)
        print("%-20s %.1f s  e_tot %.10f  |[F,D]| %.1e" % (name, time.time() - t0, r["e_tot"], r["commutator"]), flush=True)
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "oracle_dfk.json"), "w"), indent=1)
