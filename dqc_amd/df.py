"""Density-fitted Coulomb operator: the MI355X counterpart of the reference's DFMol (dqc/df/dfmol.py:12-101).

    build():      j2c = (k|l)  [dqc_int2c2e],  j3c = (ij|k)  [dqc_int3c2e]  over the concatenated orbital + auxiliary
                  shell tables (LibcintWrapper.concatenate, lcintwrap.py:299-370); Cholesky factor of j2c
    get_elrep():  c = j2c^-1 (j3c^T vec D_ao),  J_ao = j3c c,  J = X^T J_ao X      (dfmol.py:60-79)

The reference precomputes inv(j2c) and el_mat = j3c inv(j2c) (a second (nao, nao, naux) tensor); here only inv(j2c)
is kept (its "low memory" branch, dfmol.py:71-73) -- the same numbers without the extra tensor.  The two contractions are matrix-vector products over j3c viewed as (nao^2, naux) -- plain library GEMV
(rocBLAS through torch), HBM-bound at 2 x 8 nao^2 naux bytes per Fock build (0.76 GB for a 20-atom cc-pVDZ molecule
with ~1100 auxiliary functions, against 2.0 GB for the exact-J tile stream).  `method="overlap"` is not implemented in
the reference either (dfmol.py:41-45).

Fitted exchange (RI-K, `DensityFitInfo.exchange`; not in the reference) with the same auxiliary set and metric:

    build():        j2c = C C^T (Cholesky),  B[P, mu, nu] = sum_Q (C^-1)[P, Q] (mu nu|Q)   -- a triangular solve, no inverse
    exchange_ao():  K[mu, nu] = sum_P sum_lam,sig B[P, mu, lam] D[lam, sig] B[P, nu, sig]
                    D = L L^T known (ao_orb2dm):  Y_P = B_P L,  K = sum_P Y_P Y_P^T           [dqc_df_exchange]
                    anonymous D:                  sum_P B_P D B_P as batched matmul over chunks of P

B is a second 8 nao^2 naux-byte tensor, auxiliary index first: one auxiliary function is one contiguous nao x nao slab.
"""
from typing import List

import torch

from . import lib
from .basis import make_tables
from .linop import LinearOperator
from .utils.datastruct import AtomCGTOBasis, DensityFitInfo


class DFMI355:
    def __init__(self, dfinfo: DensityFitInfo, atombases: List[AtomCGTOBasis], orthozer: torch.Tensor, device):
        self.dfinfo = dfinfo
        self._atombases = atombases
        self._orthozer = orthozer
        self.device = device
        self._is_built = False
        if dfinfo.method not in ("coulomb", "overlap"):
            raise RuntimeError("Unknown density fitting method: %s" % dfinfo.method)

    def build(self):
        if self.dfinfo.method == "overlap":  # dfmol.py:41-45
            raise NotImplementedError("Density fitting with overlap minimization is not implemented")
        # concatenated tables: atoms of the orbital parent, then of the auxiliary parent; shells likewise
        atm, bas, env, _ = make_tables(list(self._atombases) + list(self.dfinfo.auxbases))
        tab = lib.Tables(atm, bas, env)
        nsh_orb = sum(len(ab.bases) for ab in self._atombases)
        orb_range, aux_range = (0, nsh_orb), (nsh_orb, tab.nbas)
        self._tab, self._orb_range, self._aux_range = tab, orb_range, aux_range  # kept for the nuclear gradient
        self._j2c = lib.int2c2e(tab, aux_range, self.device)             # (nxao, nxao)
        self._j3c = lib.int3c2e(tab, orb_range, aux_range, self.device)  # (nao, nao, nxao)
        # inverse of the SPD metric through its Cholesky factor (the reference: torch.inverse(j2c), dfmol.py:49); a
        # plain matrix, so that the per-iteration path is two GEMVs and one small GEMV -- all hipGraph-capturable
        self._inv_j2c = torch.cholesky_inverse(torch.linalg.cholesky(self._j2c)).contiguous()
        self._work = torch.empty(2 * self._j2c.shape[0], dtype=torch.float64, device=self.device)
        if self.dfinfo.exchange:
            self._build_exchange()
        self._is_built = True
        return self

    def _build_exchange(self):
        """the Cholesky factor C of j2c and B = C^-1 j3c, auxiliary index first"""
        nao, naux = self._j3c.shape[0], self._j3c.shape[2]
        # B is as large as j3c, and the solve needs a transposed copy of the columns it works on: chunks of nao^2 / 8 columns
        step = max(1, (nao * nao + 7) // 8)
        need = 8 * nao * nao * naux + 2 * 8 * step * naux
        free, _total = torch.cuda.mem_get_info(self.device)
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)  # (cached blocks are reusable)
        if need > free:
            raise lib.DqcAmdError(
                "the fitted-exchange tensor B (nao = %d, naux = %d) needs %.2f GB beside the %.2f GB of j3c but only %.2f GB of "
                "device memory are free: use a smaller auxiliary basis, or densityfit(exchange=False) with a pure functional"
                % (nao, naux, need / 1e9, 8 * nao * nao * naux / 1e9, free / 1e9))
        self._chol_j2c = torch.linalg.cholesky(self._j2c)
        b = torch.empty((naux, nao * nao), dtype=torch.float64, device=self.device)
        j3 = self._j3c.reshape(nao * nao, naux)
        for c0 in range(0, nao * nao, step):
            b[:, c0:c0 + step] = torch.linalg.solve_triangular(self._chol_j2c, j3[c0:c0 + step].t(), upper=False)
        self._b = b.reshape(naux, nao, nao)
        self._kwork, self._kwork_rp = None, 0

    @property
    def exchange(self) -> bool:
        """the exchange operator is fitted too (DensityFitInfo.exchange)"""
        return bool(self.dfinfo.exchange)

    def exchange_ao(self, dao: torch.Tensor, factors=None) -> torch.Tensor:
        """AO-basis K of an AO-basis density matrix.  `factors`: the padded factor pairs of D = sum_p L_p L_p^T (the panels of
        HamiltonMI355._factor_of) -- the kernel, one call per panel; None (an anonymous density, negative occupations): the torch
        form sum_P B_P D B_P, which the kernel is tested against"""
        if not self.dfinfo.exchange:
            raise RuntimeError("Exact exchange cannot be computed with density fitting")  # hcgto.py:229-230
        if not self._is_built:
            raise RuntimeError("Please call `build()` before `exchange_ao`")
        naux, nao = self._b.shape[0], self._b.shape[1]
        if factors is not None:
            rp = max(f[0].shape[1] for f in factors)
            if self._kwork is None or self._kwork_rp < rp:
                self._kwork, self._kwork_rp = lib.df_exchange_work(nao, naux, rp, self.device), rp
            k = lib.df_exchange(self._b, factors[0], self._kwork)
            for f in factors[1:]:
                k = k + lib.df_exchange(self._b, f, self._kwork)
            return k
        d = (dao + dao.transpose(-2, -1)) * 0.5
        k = torch.zeros((nao, nao), dtype=torch.float64, device=self.device)
        step = max(1, min(naux, (1 << 24) // (nao * nao)))  # 128 MB of B_P D per chunk
        for p0 in range(0, naux, step):
            bp = self._b[p0:p0 + step]
            t = torch.matmul(bp, d).transpose(0, 1).reshape(nao, -1)          # [mu, (P, sig)]
            k = k + t @ bp.transpose(0, 1).reshape(nao, -1).t()               # sum_(P, sig) T[mu, (P, sig)] B[P, nu, sig]
        return (k + k.t()) * 0.5

    def get_elrep(self, dm: torch.Tensor) -> LinearOperator:
        if not self._is_built:
            raise RuntimeError("Please call `build()` before `get_elrep`")
        X = self._orthozer

        def one(d):
            dao = (X @ d @ X.transpose(-2, -1)).contiguous()
            mat = lib.df_coulomb(self._j3c, self._inv_j2c, dao, self._work)   # dfmol.py:66-75, one fused pass pair
            mat = (mat + mat.transpose(-2, -1)) * 0.5
            return X.transpose(-2, -1) @ mat @ X

        if dm.dim() == 2:
            mat = one(dm)
        else:
            bshape = dm.shape[:-2]
            mat = torch.stack([one(d) for d in dm.reshape(-1, *dm.shape[-2:])]).reshape(*bshape, X.shape[-1], X.shape[-1])
        return LinearOperator.m(mat, is_hermitian=True)

    def coulomb_ao(self, dao: torch.Tensor) -> torch.Tensor:
        """AO-basis J of an AO-basis density matrix (the kernel call of get_elrep without the basis conversions)"""
        mat = lib.df_coulomb(self._j3c, self._inv_j2c, dao.contiguous(), self._work)
        return (mat + mat.transpose(-2, -1)) * 0.5

    @property
    def j2c(self) -> torch.Tensor:
        return self._j2c

    @property
    def j3c(self) -> torch.Tensor:
        return self._j3c

    def getparamnames(self, methodname: str, prefix: str = "") -> List[str]:
        if methodname == "get_elrep":
            return [prefix + "_inv_j2c", prefix + "_j3c", prefix + "_orthozer"]
        if methodname == "exchange_ao" and self.dfinfo.exchange:
            return [prefix + "_b"]
        raise KeyError("getparamnames has no %s method" % methodname)
