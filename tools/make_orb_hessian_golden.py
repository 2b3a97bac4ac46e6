"""Fixtures for the orbital Hessian (dqc_amd/response.py): the DENSE Hessian d2E / dkappa2 of small oracle SCF solutions, built
column by column from central differences of the oracle's own Fock matrix.

For each case the oracle SCF is converged to 1e-11, C and eps are the eigenvectors / eigenvalues of the oracle's Fock matrix, and
for every rotation (a, i) [of every spin] the response Fock matrix is

    G[dD] ~ (F[D + h dD] - F[D - h dD]) / 2 h,      dD = occ (c_a c_i^T + c_i c_a^T)    (occ = 2 restricted, 1 per spin),

J and K are linear in D, so only Vxc carries a stencil error: two steps (h, h / 2) and Richardson extrapolation (4 G(h/2) - G(h)) / 3;
`fd_stencil` = max |Richardson - (h / 2 value)| over the Hessian.  The differences also carry the round-off of the Fock matrices
divided by h, which that estimate does not see: `fd_roundoff` = 3 pref eps max|F| max|c_a|_1 max|c_i|_1 / h (derived in `hessian`).
`fd_error` = max(fd_stencil, fd_roundoff) is the recorded error of a Hessian element.  Column (a, i) of the Hessian is  pref [ (eps_a - eps_i) e_ai +
C_v^T G C_o ]  with pref = 4 (restricted) or 2 (unrestricted, alpha block then beta block) -- the prefactors of dqc_amd/response.py.

Recorded per case: the Hessian, its three lowest eigenvalues, H kappa of a seeded kappa, the orbitals (AO basis) and densities the
GPU tests start from, and for the stable cases the static polarizability alpha[e, d] = d mu_e / d F_d by finite fields: oracle SCF
runs at +-F and +-F/2 per direction, Richardson, `alpha_error` = max |Richardson - (F / 2 value)|.

Cases (all 3-21G, Kohn-Sham on the sg2 grid): H2O RHF / LDA / PBE / BLYP / PBE0; CH3 (spin 1) UHF / UKS PBE; H2 at 1.4 Bohr
unrestricted HF / LDA (stable); H2 at 4.0 Bohr unrestricted, spin 0, HF / LDA on the SYMMETRIC solution: the textbook RHF -> UHF
instability -- asserted here (lowest eigenvalue far below -1e-3, and the oracle SCF must not have broken the symmetry by itself).

Imports `oracle` and `tests.molecules` only, never dqc_amd.  Writes tests/golden/oracle_orb_hessian.npz.
usage: python tools/make_orb_hessian_golden.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import hamilton as oh, basis as ob, natives  # noqa: E402
from tests import molecules as M  # noqa: E402

CH3 = ([6, 1, 1, 1], [[0, 0, 0.05], [2.039, 0, 0], [-1.0195, 1.7658, 0], [-1.0195, -1.7658, 0.1]])
H2_14 = ([1, 1], [[0, 0, -0.7], [0, 0, 0.7]])
H2_40 = ([1, 1], [[0, 0, -2.0], [0, 0, 2.0]])
LDA, PBE, BLYP = "lda_x + lda_c_pw", "gga_x_pbe + gga_c_pbe", "gga_x_b88 + gga_c_lyp"
# name: (molecule, spin or None for restricted, xc string given to dqc_amd (None: HF), grid part for the oracle, exchange fraction, stable)
CASES = {
    "h2o_rhf": (M.H2O, None, None, None, 1.0, True),
    "h2o_lda": (M.H2O, None, LDA, LDA, 0.0, True),
    "h2o_pbe": (M.H2O, None, PBE, PBE, 0.0, True),
    "h2o_blyp": (M.H2O, None, BLYP, BLYP, 0.0, True),
    "h2o_pbe0": (M.H2O, None, "pbe0", "0.75 * gga_x_pbe + gga_c_pbe", 0.25, True),
    "ch3_uhf": (CH3, 1, None, None, 1.0, True),
    "ch3_upbe": (CH3, 1, PBE, PBE, 0.0, True),
    "h2_14_uhf": (H2_14, 0, None, None, 1.0, True),
    "h2_14_ulda": (H2_14, 0, LDA, LDA, 0.0, True),
    "h2_40_uhf": (H2_40, 0, None, None, 1.0, False),
    "h2_40_ulda": (H2_40, 0, LDA, LDA, 0.0, False),
}
BASIS, GRID, H_STEP, F_STEP = "3-21G", "sg2", 4e-4, 2e-3


class Restricted(oh.Engine):
    """F = h + J + a get_exchange + Vxc[grid part] (get_exchange = -K / 2)"""

    def __init__(self, tables, gridxc, a):
        super().__init__(tables, xc=gridxc, grid=GRID)
        self.a, self.has_grid = float(a), gridxc is not None

    def dm2scp(self, dm):
        F = self.h.kinnucl_mat + self.h.get_elrep(dm)
        if self.a != 0.0:
            F = F + self.a * self.h.get_exchange(dm)
        return F + self.h.get_vxc(dm) if self.has_grid else F

    def focks(self, dms):
        return [self.dm2scp(dms[0])]

    def dms(self):
        return [self.dm]


class Unrestricted(oh.EnginePol):
    def __init__(self, tables, spin, gridxc, a):
        super().__init__(tables, spin, xc=gridxc, grid=GRID)
        self.a, self.has_grid = float(a), gridxc is not None

    def dm2scp(self, dm):
        dmu, dmd = dm
        core = self.h.kinnucl_mat + self.h.get_elrep(dmu + dmd)
        fu, fd = core, core
        if self.a != 0.0:
            fu, fd = fu + self.a * self.h.get_exchange(2 * dmu), fd + self.a * self.h.get_exchange(2 * dmd)
        if self.has_grid:
            vu, vd, _ = self._vxc(dmu, dmd)
            fu, fd = fu + vu, fd + vd
        return torch.stack([fu, fd])

    def focks(self, dms):
        return list(self.dm2scp(tuple(dms)))

    def dms(self):
        return list(self.dm)


def make(case):
    mol, spin, _, gridxc, a, _ = CASES[case]
    t = ob.make_tables(mol, BASIS)
    eng = Restricted(t, gridxc, a) if spin is None else Unrestricted(t, spin, gridxc, a)
    return t, eng


def hessian(eng, step):
    dms = eng.dms()
    nspin = len(dms)
    occ, pref = (2.0, 4.0) if nspin == 1 else (1.0, 2.0)
    nocc = [eng.norb] if nspin == 1 else [eng.nup, eng.ndn]
    F0 = eng.focks(dms)
    orbs = []
    for f, no in zip(F0, nocc):
        e, c = torch.linalg.eigh((f + f.T) * 0.5)
        orbs.append((e, c, no))
    sizes = [(c.shape[1] - no) * no for _, c, no in orbs]
    n = sum(sizes)

    def build(h):
        H = torch.zeros((n, n), dtype=torch.float64)
        col = 0
        for s, (e, c, no) in enumerate(orbs):
            for a_ in range(no, c.shape[1]):
                for i in range(no):
                    dd = occ * (torch.outer(c[:, a_], c[:, i]) + torch.outer(c[:, i], c[:, a_]))
                    plus = [d + h * dd if k == s else d for k, d in enumerate(dms)]
                    minus = [d - h * dd if k == s else d for k, d in enumerate(dms)]
                    G = [(fp - fm) / (2 * h) for fp, fm in zip(eng.focks(plus), eng.focks(minus))]
                    H[:, col] = torch.cat([pref * (c2[:, no2:].T @ g @ c2[:, :no2]).reshape(-1) for g, (_, c2, no2) in zip(G, orbs)])
                    H[col, col] += pref * (e[a_] - e[i])
                    col += 1
        return H
    h1, h2 = build(step), build(step / 2)
    rich = (4 * h2 - h1) / 3
    # round-off of the differenced Fock matrices, which the stencil estimate does not see (it is all there is for Hartree-Fock):
    # an element of F carries at least eps max|F|; (F+ - F-) / 2h at the steps h and h / 2 then eps max|F| / h and twice that, the
    # Richardson value (4 * 2 + 1) / 3 = 3 times it; the projection sum_pq c_pa G_pq c_qi multiplies by at most |c_a|_1 |c_i|_1
    eps = float(torch.finfo(torch.float64).eps)
    fmax = max(float(f.abs().max()) for f in F0)
    cnorm = max(float(c[:, no:].abs().sum(0).max() * c[:, :no].abs().sum(0).max()) for _, c, no in orbs)
    roundoff = 3.0 * pref * eps * fmax * cnorm / step
    return rich, float((rich - h2).abs().max()), roundoff, orbs


def polarizability(eng, step):
    r = torch.as_tensor(natives.int1e("r0", eng.t))
    r_orth = torch.stack([eng.h.convert2(x) for x in r])
    base = eng.h.kinnucl_mat.clone()

    def dipole(f):
        eng.h.kinnucl_mat = base + torch.einsum("dab,d->ab", r_orth, torch.as_tensor(f))
        eng.run(maxiter=300, tol=1e-11)
        tot = sum(eng.dms())
        return -torch.einsum("dab,ba->d", r_orth, tot)

    def fd(s):
        cols = []
        for d in range(3):
            f = np.zeros(3)
            f[d] = s
            cols.append((dipole(f) - dipole(-f)) / (2 * s))
        return torch.stack(cols, dim=-1)
    a1, a2 = fd(step), fd(step / 2)
    eng.h.kinnucl_mat = base
    rich = (4 * a2 - a1) / 3
    return rich, float((rich - a2).abs().max())


if __name__ == "__main__":
    out = {"_how": np.array(__doc__)}
    meta = {}
    for case, (mol, spin, xc, gridxc, a, stable) in CASES.items():
        t0 = time.time()
        t, eng = make(case)
        eng.run(maxiter=300, tol=1e-11)
        if spin == 0:  # the symmetric solution: the oracle SCF must not have broken the spin symmetry by itself
            assert float((eng.dm[0] - eng.dm[1]).abs().max()) < 1e-9, "%s: the oracle SCF broke the spin symmetry" % case
        H, fd_stencil, fd_roundoff, orbs = hessian(eng, H_STEP)
        fd_error = max(fd_stencil, fd_roundoff)
        Hs = (H + H.T) * 0.5
        ev = torch.linalg.eigvalsh(Hs)
        if stable:
            assert ev[0] > -1e-3, (case, float(ev[0]))
        else:
            assert ev[0] < -1e-2, "%s: expected the RHF -> UHF instability, lowest eigenvalue %g" % (case, float(ev[0]))
        kappa = torch.as_tensor(np.random.default_rng(20260910 + len(meta)).normal(size=H.shape[0]))
        X = eng.h.X
        out[case + "_hessian"] = H.numpy()
        out[case + "_fd_error"] = np.array(fd_error)
        out[case + "_fd_stencil"], out[case + "_fd_roundoff"] = np.array(fd_stencil), np.array(fd_roundoff)
        out[case + "_eig3"] = ev[:3].numpy()
        out[case + "_kappa"] = kappa.numpy()
        out[case + "_hkappa"] = (H @ kappa).numpy()
        for s, (e, c, no) in enumerate(orbs):
            out["%s_c_ao_%d" % (case, s)] = (X @ c).numpy()
            out["%s_eps_%d" % (case, s)] = e.numpy()
            out["%s_dm_ao_%d" % (case, s)] = eng.h.unconvert_dm(eng.dms()[s]).numpy()
        if stable:
            alpha, alpha_error = polarizability(eng, F_STEP)
            out[case + "_alpha"], out[case + "_alpha_error"] = alpha.numpy(), np.array(alpha_error)
        meta[case] = {"atomzs": mol[0], "atompos": mol[1], "spin": spin, "xc": xc, "oracle_grid_part": gridxc, "exx_fraction": a,
                      "stable": stable, "basis": BASIS, "grid": GRID, "nocc": [o[2] for o in orbs], "n": int(H.shape[0])}
        print("%-12s n %3d  %.0f s  fd_error %.1e (stencil %.1e, round-off %.1e)  asym %.1e  lowest %s%s" % (
            case, H.shape[0], time.time() - t0, fd_error, fd_stencil, fd_roundoff, float((H - H.T).abs().max()), ev[:3].numpy(),
            "  alpha_error %.1e" % out[case + "_alpha_error"] if stable else ""), flush=True)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "oracle_orb_hessian.npz"), **out)
