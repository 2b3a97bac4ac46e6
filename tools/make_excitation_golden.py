"""Fixtures for the linear-response excited states (dqc_amd.excitations): DENSE A + B and A - B of small oracle SCF solutions and
the spectra that follow from them by dense eigh.

Definitions (real orbitals, variables kappa_ai of dqc_amd/response.py; a = exact-exchange fraction, K[D]_pq = (pr|qs) D_rs):

    restricted   (A+B)^S = H / 4       H: the orbital Hessian of tools/make_orb_hessian_golden.py (Richardson central differences of
                                       the oracle's Fock matrix, `fd_error` per element of H)
                 (A-B)   column (a, i) = (eps_a - eps_i) e_ai - (a / 2) C_v^T K[2 (c_a c_i^T - c_i c_a^T)] C_o
                 (A+B)^T column (a, i) = (eps_a - eps_i) e_ai + C_v^T G_u C_o,  G_u = (F_u[D/2 + h d, D/2 - h d] - F_u[D/2 - h d, D/2 + h d]) / 2h,
                                       d = c_a c_i^T + c_i c_a^T: the SAME Richardson differences, of the oracle's polarised Fock pair
                                       under dD_u = -dD_d (no Coulomb term; exchange -(a / 2) K[2 d]; the spin-flip functional kernel)
    unrestricted (A+B) = H / 2,  (A-B)_s column (a, i) = (eps_a - eps_i) e_ai - a C_vs^T K[c_a c_i^T - c_i c_a^T] C_os, no coupling of the spins

A - B is exact: K is the oracle's own exchange contraction  einsum("il,ijkl->ijk", dm, el_mat).sum(-3)  (oracle/hamilton.py:
get_exchange), which is linear and takes any matrix.  get_exchange itself symmetrises what that einsum returns -- the exchange of
an antisymmetric matrix is antisymmetric, it would come back as zero -- so the einsum is restated here (`exchange`), checked
against get_exchange on a symmetric matrix and against the plain four-index sum on a random antisymmetric one.

Spectra: full response (A-B)^(1/2) (A+B) (A-B)^(1/2) Z = w^2 Z, X+Y = (A-B)^(1/2) Z / sqrt(w), X-Y = sqrt(w) (A-B)^(-1/2) Z, so that
(X+Y)^T (X-Y) = 1; TDA: A = ((A+B) + (A-B)) / 2, A X = w X, X^T X = 1.  Transition dipoles mu = sqrt(2) sum_ai r_ai (X+Y)_ai
(restricted singlet), sum_s sum_ai r^s_ai (X+Y)^s_ai (unrestricted), zero (triplet); f = (2 / 3) w |mu|^2.

Errors.  Only A+B with a grid functional carries a stencil error; an element of A+B carries e = fd_error / pref (pref 4 / 2), and
e_T for the triplet from its own differences.  A symmetric perturbation with elements <= e has a 2-norm <= n e, so
    TDA            |dw| <= n e / 2                        (A = (A+B)/2 + (A-B)/2, Weyl)
    full response  |d(w^2)| <= |A-B|_2 n e   (the matrix is (A-B)^(1/2) (A+B) (A-B)^(1/2)),   |dw| = |d(w^2)| / 2w
recorded per state as `*_omega_error_*`.  The triplet of an unstable closed-shell state (H2 at 4 Bohr: (A+B)^T has a negative
eigenvalue -- the RHF -> UHF instability) has no real spectrum: only its matrices and lowest eigenvalue are recorded.

Cases (3-21G, sg2; the table of tools/make_orb_hessian_golden.py): h2o_rhf, h2o_lda, h2o_pbe, h2o_pbe0 (n = 40), ch3_uhf, ch3_upbe,
h2_14_uhf, and RESTRICTED H2 at 4.0 Bohr (h2_40_rhf, h2_40_rlda) and 1.4 Bohr (h2_14_rhf, h2_14_rlda) for the triplet stability.

Imports `oracle`, `tests.molecules` and the helpers of tools/make_orb_hessian_golden.py, never dqc_amd.  Writes
tests/golden/oracle_excitations.npz.
usage: python tools/make_excitation_golden.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import make_orb_hessian_golden as moh  # noqa: E402
from oracle import natives  # noqa: E402

CASES = {k: moh.CASES[k] for k in ("h2o_rhf", "h2o_lda", "h2o_pbe", "h2o_pbe0", "ch3_uhf", "ch3_upbe", "h2_14_uhf")}
CASES.update({
    "h2_14_rhf": (moh.H2_14, None, None, None, 1.0, True),
    "h2_14_rlda": (moh.H2_14, None, moh.LDA, moh.LDA, 0.0, True),
    "h2_40_rhf": (moh.H2_40, None, None, None, 1.0, True),   # (stable in the singlet space: what `hessian` asserts nothing about)
    "h2_40_rlda": (moh.H2_40, None, moh.LDA, moh.LDA, 0.0, True),
})


def exchange(el_mat, dm):
    """K[D]_pq = (pr|qs) D_rs: the einsum of oracle get_exchange, without its factor -1/2 and its symmetrisation"""
    return torch.einsum("il,ijkl->ijk", dm, el_mat).sum(dim=-3)


def check_exchange(h):
    n = h.nao
    g = torch.Generator().manual_seed(7)
    s = torch.randn((n, n), generator=g, dtype=torch.float64)
    sym, anti = s + s.T, s - s.T
    assert float((-0.5 * exchange(h.el_mat, sym) - h.get_exchange(sym)).abs().max()) < 1e-12
    k = exchange(h.el_mat, anti)
    ref = torch.einsum("prqs,rs->pq", h.el_mat, anti)
    assert float((k - ref).abs().max()) < 1e-12 * float(ref.abs().max()) and float((k + k.T).abs().max()) < 1e-12 * float(ref.abs().max())
    assert float(h.get_exchange(anti).abs().max()) < 1e-12  # (why get_exchange itself cannot be used)


def a_minus_b(eng, orbs, a):
    nspin = len(orbs)
    sizes = [(c.shape[1] - no) * no for _, c, no in orbs]
    M = torch.zeros((sum(sizes), sum(sizes)), dtype=torch.float64)
    off = 0
    for (e, c, no), size in zip(orbs, sizes):
        col = off
        for a_ in range(no, c.shape[1]):
            for i in range(no):
                M[col, col] = e[a_] - e[i]
                if a != 0.0:
                    d = torch.outer(c[:, a_], c[:, i]) - torch.outer(c[:, i], c[:, a_])
                    k = exchange(eng.h.el_mat, (2.0 if nspin == 1 else 1.0) * d)
                    M[off:off + size, col] -= (0.5 * a if nspin == 1 else a) * (c[:, no:].T @ k @ c[:, :no]).reshape(-1)
                col += 1
        off += size
    return M


def triplet_a_plus_b(case, eng, orbs, step):
    """(A+B)^T of a restricted solution by central differences of the oracle's polarised Fock pair; -> matrix, element error"""
    mol, _, _, gridxc, a, _ = CASES[case]
    pol = moh.Unrestricted(eng.t, 0, gridxc, a)
    (e, c, no), = orbs
    half = eng.dm * 0.5
    n = (c.shape[1] - no) * no

    def build(h):
        M = torch.zeros((n, n), dtype=torch.float64)
        col = 0
        for a_ in range(no, c.shape[1]):
            for i in range(no):
                d = torch.outer(c[:, a_], c[:, i]) + torch.outer(c[:, i], c[:, a_])
                fp = pol.focks([half + h * d, half - h * d])[0]
                fm = pol.focks([half - h * d, half + h * d])[0]
                M[:, col] = (c[:, no:].T @ ((fp - fm) / (2 * h)) @ c[:, :no]).reshape(-1)
                M[col, col] += e[a_] - e[i]
                col += 1
        return M
    h1, h2 = build(step), build(step / 2)
    rich = (4 * h2 - h1) / 3
    eps = float(torch.finfo(torch.float64).eps)  # round-off of the differenced Fock matrices: as in make_orb_hessian_golden.hessian, pref 1
    fmax = float(pol.focks([half, half])[0].abs().max())
    roundoff = 3.0 * eps * fmax * float(c[:, no:].abs().sum(0).max() * c[:, :no].abs().sum(0).max()) / step
    return rich, max(float((rich - h2).abs().max()), roundoff)


def spectra(apb, amb, e_apb):
    """-> dict: w / xpy / xmy (full response), w_tda / x_tda, their error bounds; None when A+B or A-B is not positive definite"""
    n = apb.shape[0]
    apb, amb = (apb + apb.T) * 0.5, (amb + amb.T) * 0.5
    if float(torch.linalg.eigvalsh(apb)[0]) <= 0 or float(torch.linalg.eigvalsh(amb)[0]) <= 0:
        return None
    d, u = torch.linalg.eigh(amb)
    rt, irt = (u * d.sqrt()) @ u.T, (u / d.sqrt()) @ u.T
    w2, z = torch.linalg.eigh(rt @ apb @ rt)
    w = w2.sqrt()
    xpy, xmy = (rt @ z / w.sqrt()).T, (irt @ z * w.sqrt()).T
    assert float(((xpy * xmy).sum(1) - 1).abs().max()) < 1e-10
    # the non-Hermitian form, as a check of the reduction: eigenvalues of (A-B)(A+B)
    w2_ns = np.sort(np.linalg.eigvals((amb @ apb).numpy()).real)
    assert np.abs(w2_ns - w2.numpy()).max() < 1e-9 * max(1.0, float(w2[-1]))
    wt, xt = torch.linalg.eigh((apb + amb) * 0.5)
    return {"w": w, "xpy": xpy, "xmy": xmy, "w_tda": wt, "x_tda": xt.T,
            "err": float(d[-1]) * n * e_apb / (2 * w), "err_tda": torch.full_like(wt, 0.5 * n * e_apb)}


def dipoles(r_blocks, vecs, restricted):
    """r_blocks: per spin (3, nv no); vecs (nstate, n) -> (nstate, 3)"""
    r = torch.cat(r_blocks, dim=1)
    return (np.sqrt(2.0) if restricted else 1.0) * vecs @ r.T


if __name__ == "__main__":
    gold = np.load(os.path.join(ROOT, "tests", "golden", "oracle_orb_hessian.npz"))
    out = {"_how": np.array(__doc__)}
    meta = {}
    for case, (mol, spin, xc, gridxc, a, _) in CASES.items():
        t0 = time.time()
        t = moh.ob.make_tables(mol, moh.BASIS)
        eng = moh.Restricted(t, gridxc, a) if spin is None else moh.Unrestricted(t, spin, gridxc, a)
        eng.run(maxiter=300, tol=1e-11)
        check_exchange(eng.h)
        if spin == 0:
            assert float((eng.dm[0] - eng.dm[1]).abs().max()) < 1e-9
        H, fd_stencil, fd_roundoff, orbs = moh.hessian(eng, moh.H_STEP)
        restricted = spin is None
        pref = 4.0 if restricted else 2.0
        if case + "_hessian" in gold.files:  # the same construction as the existing fixture: the same spectrum (the signs of the
            # orbitals, hence of rows and columns, are the eigensolver's choice and may differ between two runs)
            ev_new, ev_old = np.linalg.eigvalsh((H.numpy() + H.numpy().T) * 0.5), np.linalg.eigvalsh((gold[case + "_hessian"] + gold[case + "_hessian"].T) * 0.5)
            assert np.abs(ev_new - ev_old).max() < H.shape[0] * 10 * float(gold[case + "_fd_error"]) + 1e-9, (case, np.abs(ev_new - ev_old).max())
        apb, e_apb = H / pref, max(fd_stencil, fd_roundoff) / pref
        amb = a_minus_b(eng, orbs, a)
        assert float((amb - amb.T).abs().max()) < 1e-11
        if a == 0.0:
            assert float((amb - torch.diag(torch.diag(amb))).abs().max()) == 0.0
        X = eng.h.X
        r_ao = torch.as_tensor(natives.int1e("r0", t))
        r_blocks = [torch.stack([((X @ c)[:, no:].T @ x @ (X @ c)[:, :no]).reshape(-1) for x in r_ao]) for _, c, no in orbs]
        n = apb.shape[0]
        out[case + "_apb"], out[case + "_amb"], out[case + "_fd_error"] = apb.numpy(), amb.numpy(), np.array(e_apb)
        kappa = torch.as_tensor(np.random.default_rng(20261017 + len(meta)).normal(size=(2, n)))
        out[case + "_kappa"] = kappa.numpy()
        sp = spectra(apb, amb, e_apb)
        assert sp is not None, case
        for key, vec in (("rpa", sp["xpy"]), ("tda", sp["x_tda"])):
            w = sp["w"] if key == "rpa" else sp["w_tda"]
            mu = dipoles(r_blocks, vec, restricted)
            out["%s_w_%s" % (case, key)], out["%s_mu_%s" % (case, key)] = w.numpy(), mu.numpy()
            out["%s_f_%s" % (case, key)] = (2.0 / 3.0 * w * (mu * mu).sum(1)).numpy()
            out["%s_omega_error_%s" % (case, key)] = (sp["err"] if key == "rpa" else sp["err_tda"]).numpy()
        out[case + "_xpy"], out[case + "_xmy"] = sp["xpy"].numpy(), sp["xmy"].numpy()
        note = ""
        if case + "_alpha" in gold.files:  # sum rule against the finite-field polarizability of the existing fixture
            mu = torch.as_tensor(out[case + "_mu_rpa"])
            alpha = 2.0 * torch.einsum("ne,nd,n->ed", mu, mu, 1.0 / sp["w"])
            note = "  sum rule - finite-field alpha %.1e" % float((alpha - torch.as_tensor(gold[case + "_alpha"])).abs().max())
        if restricted:
            apb_t, e_t = triplet_a_plus_b(case, eng, orbs, moh.H_STEP)
            out[case + "_apb_t"], out[case + "_fd_error_t"] = apb_t.numpy(), np.array(e_t)
            low_t = float(torch.linalg.eigvalsh((apb_t + apb_t.T) * 0.5)[0])
            out[case + "_apb_t_lowest"] = np.array(low_t)
            spt = spectra(apb_t, amb, e_t)
            if case.startswith("h2_40"):
                assert spt is None and low_t < -1e-2 / 4, "%s: expected the RHF -> UHF (triplet) instability, lowest %g" % (case, low_t)
            else:
                assert spt is not None, case
                out[case + "_w_rpa_t"], out[case + "_w_tda_t"] = spt["w"].numpy(), spt["w_tda"].numpy()
                out[case + "_omega_error_rpa_t"], out[case + "_omega_error_tda_t"] = spt["err"].numpy(), spt["err_tda"].numpy()
            note += "  triplet: fd_error %.1e lowest (A+B)^T %.6f" % (e_t, low_t)
        for s, (e, c, no) in enumerate(orbs):
            out["%s_c_ao_%d" % (case, s)] = (X @ c).numpy()
            out["%s_eps_%d" % (case, s)] = e.numpy()
            out["%s_dm_ao_%d" % (case, s)] = eng.h.unconvert_dm(eng.dms()[s]).numpy()
        meta[case] = {"atomzs": mol[0], "atompos": mol[1], "spin": spin, "xc": xc, "oracle_grid_part": gridxc, "exx_fraction": a,
                      "basis": moh.BASIS, "grid": moh.GRID, "nocc": [o[2] for o in orbs], "n": int(n),
                      "triplet_stable": (not case.startswith("h2_40")) if restricted else None}
        print("%-11s n %3d  %.0f s  fd_error(A+B) %.1e  asym(A+B) %.1e  w[:3] %s  f[:3] %s  max omega_error %.1e%s" % (
            case, n, time.time() - t0, e_apb, float((apb - apb.T).abs().max()), out[case + "_w_rpa"][:3], out[case + "_f_rpa"][:3],
            float(sp["err"].max()), note), flush=True)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "oracle_excitations.npz"), **out)
