"""Mol: thin equivalent of the reference's dqc/system/mol.py (constructor :77-121, get_nuclei_energy :252-260,
setup_grid :262-267, occupations :421-443) that owns a HamiltonMI355 and a device grid."""
from typing import Optional

import torch

from .basis import parse_moldesc, make_atombases
from .grid import get_predefined_grid
from .hamilton import HamiltonMI355


class Mol:
    def __init__(self, moldesc, basis, *, grid="sg3", spin: Optional[int] = None, charge: int = 0, orb_weights=None,
                 orthogonalize_basis: bool = True, ao_parameterizer: str = "qr", efield=None, vext=None,
                 dtype=torch.float64, device="cuda"):
        if dtype != torch.float64:
            raise NotImplementedError("the MI355X path computes in float64 like the reference default (mol.py:90)")
        self._dtype = dtype
        self._device = torch.device(device)
        self._grid_inp = grid
        self._basis_inp = basis
        self._grid = None
        atomzs, atompos = parse_moldesc(moldesc, dtype=dtype)
        # the caller's tensors are kept for the energy's autograd node (dqc_amd/autograd.py); everything handed down to the
        # Hamiltonian, the grid and the basis is detached, so the SCF runs on plain values (no graph, no grid autograd path)
        self._grad_leaves = {"atompos": atompos}
        if atomzs.is_floating_point():
            self._grad_leaves["atomzs"] = atomzs
        atomzs, atompos = atomzs.detach(), atompos.detach()
        self._atomzs, self._atompos = atomzs, atompos
        self._atombases = make_atombases(atomzs, atompos, basis)
        # the caller's exponents / coefficients of every shell in table order, before make_tables normalises the shells in place
        # (a CGTOBasis an earlier Mol normalised still carries the tensor it was given)
        self._basis_shells = [(sh.angmom, sh.alphas, getattr(sh, "_raw_coeffs", sh.coeffs), sh.normalized and not hasattr(sh, "_raw_coeffs"))
                              for ab in self._atombases for sh in ab.bases]
        bleaves = {id(t): t for _, a, c, _ in self._basis_shells for t in (a, c) if t.requires_grad}
        if bleaves:
            self._grad_leaves["basis"] = tuple(bleaves.values())
        self._user_weights = None
        if orb_weights is not None:
            # mol.py:143-167: explicit occupations (SpinParam of equally long 1-D tensors); electron count, spin and charge
            # follow from them
            from .utils.datastruct import SpinParam
            if not isinstance(orb_weights, SpinParam):
                raise TypeError("Specifying orb_weights must be in SpinParam type")
            assert orb_weights.u.ndim == 1 and orb_weights.d.ndim == 1 and len(orb_weights.u) == len(orb_weights.d)
            wu, wd = orb_weights.u.to(dtype), orb_weights.d.to(dtype)
            self._grad_leaves["orb_weights"] = (wu, wd)
            wu, wd = wu.detach(), wd.detach()
            if not (bool(torch.all(wu[:-1] - wu[1:] > -1e-4)) and bool(torch.all(wd[:-1] - wd[1:] > -1e-4))):
                import warnings
                warnings.warn("The orbitals should be ordered in a non-increasing manner. "
                              "Otherwise, some calculations might be wrong.")
            self._user_weights = SpinParam(u=wu.to(self._device), d=wd.to(self._device))
            spin = float(wu.sum() - wd.sum())
            charge = float(torch.sum(atomzs.to(torch.float64))) - float(wu.sum() + wd.sum())
            if abs(spin - round(spin)) < 1e-12 and abs(charge - round(charge)) < 1e-12 and not atomzs.is_floating_point():
                spin, charge = int(round(spin)), int(round(charge))
        nelecs = float(torch.sum(atomzs.to(torch.float64))) - charge
        assert nelecs >= 0, "Only %f electrons, but needs %f charge" % (nelecs + charge, charge)
        # mol.py:402-419: a floating-point atomz / charge / spin switches to FRACTIONAL mode -- the electron count need not be
        # an integer, the spin must then be given, and the last orbital of each spin channel is partially occupied
        # (safeops.occnumber); integer input keeps the integer bookkeeping and the spin / electron-count parity check
        def _isfloat(x):
            return isinstance(x, float) or (isinstance(x, torch.Tensor) and x.is_floating_point())
        self._frac_mode = bool(atomzs.is_floating_point() or _isfloat(charge) or (spin is not None and _isfloat(spin)))
        if self._user_weights is not None:
            pass  # spin / charge were derived from the weights: nothing to validate
        elif spin is None:
            assert not self._frac_mode, "Fraction case requires the spin argument to be specified"
            spin = int(round(nelecs)) % 2
        else:
            assert spin >= 0, "inconsistent spin %g" % spin
            if not self._frac_mode:
                assert (int(round(nelecs)) - spin) % 2 == 0, "Spin %d is not suited for %d electrons" % (spin, round(nelecs))
        self._spin, self._charge = spin, charge
        self._nelecs = nelecs
        if self._frac_mode or self._user_weights is not None:
            self._ndn = (nelecs - float(spin)) * 0.5
            self._nup = self._ndn + float(spin)
            assert self._ndn >= -1e-12, "spin %g needs more than %g electrons" % (spin, nelecs)
        else:
            self._nup = (int(round(nelecs)) + spin) // 2
            self._ndn = (int(round(nelecs)) - spin) // 2
        if vext is not None:
            vext = vext.to(device=self._device, dtype=dtype)
            self._grad_leaves["vext"] = vext
            vext = vext.detach()
        # mol.py:445-474: a tensor -> 1-tuple; every element flattened ((3,), (3, 3) -> (9,), ...)
        if isinstance(efield, torch.Tensor):
            efield = (efield,)
        if efield is not None:
            for i, ef in enumerate(efield):
                assert ef.numel() == 3 ** (i + 1), "The %d-th tuple element of efield must have %d elements" % (i, 3 ** (i + 1))
            # the SCF sees detached, flattened copies; the caller's tensors (their own shapes) are the energy's autograd inputs
            self._grad_leaves["efield"] = tuple(efield)
            efield = tuple(ef.detach().reshape(-1) for ef in efield)
        self._efield, self._vext = efield, vext
        self._orthogonalize_basis, self._aoparamzer = orthogonalize_basis, ao_parameterizer
        self._hamilton = HamiltonMI355(self._atombases, spherical=True, efield=efield, vext=vext,
                                       orthozer=orthogonalize_basis, aoparamzer=ao_parameterizer,
                                       device=self._device)

    # ---- accessors with the reference's names (dqc/system/base_system.py:10-139) ----
    @property
    def atompos(self):
        return self._atompos

    @property
    def atomzs(self):
        return self._atomzs

    @property
    def spin(self):
        return self._spin

    @property
    def charge(self):
        return self._charge

    @property
    def numel(self):
        return self._nelecs

    @property
    def efield(self):
        return self._efield

    # isotope-averaged atomic masses in a.m.u. (IUPAC abridged standard atomic weights, Z = 1 .. 18) -> atomic units of mass
    _AMU = {1: 1.00797, 2: 4.00260, 3: 6.941, 4: 9.01218, 5: 10.81, 6: 12.011, 7: 14.0067, 8: 15.9994, 9: 18.998403,
            10: 20.179, 11: 22.98977, 12: 24.305, 13: 26.98154, 14: 28.0855, 15: 30.97376, 16: 32.06, 17: 35.453, 18: 39.948}

    @property
    def atommasses(self):
        """atomic masses in atomic units (mol.py:336-342; electron masses per a.m.u.: 1822.888486209)"""
        if self._atomzs.is_floating_point():
            raise RuntimeError("Atom masses are not available for floating point Z")
        heavy = [int(z) for z in self._atomzs if int(z) not in self._AMU]
        if heavy:
            raise RuntimeError("atommasses: no mass table entry for Z = %s (dqc_amd ships Z = 1 .. 18)" % sorted(set(heavy)))
        return torch.tensor([self._AMU[int(z)] * 1822.888486209 for z in self._atomzs], dtype=self._dtype, device=self._device)

    def densityfit(self, method=None, auxbasis=None, exchange=False):
        """dqc/system/mol.py:170-204: switch the Hamiltonian to the density-fitted Coulomb operator.
        exchange=True (not in the reference): the exchange operator is fitted too (RI-K: same auxiliary set, same Coulomb metric), so
        that HF and hybrid functionals run without the ~nao^4-byte ERI tile store; False: J only, exchange and hybrids are refused.
        auxbasis: list (per atom) of lists of CGTOBasis, a basis name shipped under dqc_amd/data/basis, or "etb[:beta]"
        (the built-in even-tempered set, dqc_amd.basis.even_tempered_aux) or "autoaux[:beta]" (generated from the orbital basis,
        dqc_amd.basis.product_etb_aux).  The reference's default "cc-pvtz-jkfit" and the other named JK-fit sets are external
        data (basis_set_exchange): their Gaussian94 tables are read from $DQC_AMD_BASIS_PATH when present; without them the call
        warns and uses "autoaux", so that `Mol(...).densityfit()` (dqc/test/benchmark.py:40-42) runs as written."""
        from .basis import make_aux_atombases
        from .utils.datastruct import DensityFitInfo
        if method is None:
            method = "coulomb"
        if auxbasis is None:
            auxbasis = "cc-pvtz-jkfit"
        info = {}
        auxbases = make_aux_atombases(self._atomzs, self._atompos, auxbasis, self._atombases, info)
        self.auxbasis_used = info["auxbasis_used"]  # (what the fit really uses: "autoaux (generated ...)" when the named set has no tables)
        df = DensityFitInfo(method=method, auxbases=auxbases, exchange=bool(exchange))
        self._hamilton = HamiltonMI355(self._atombases, spherical=True, df=df, efield=self._efield, vext=self._vext,
                                       orthozer=self._orthogonalize_basis, aoparamzer=self._aoparamzer,
                                       device=self._device)
        self._hamilton.auxbasis_used = self.auxbasis_used
        return self

    def get_hamiltonian(self):
        return self._hamilton

    def getparamnames(self, methodname: str, prefix: str = ""):
        """mol.py:289-296"""
        if methodname == "get_nuclei_energy":
            return [prefix + "_atompos"] + ([prefix + "_atomzs"] if self._atomzs.is_floating_point() else [])
        raise KeyError("Unknown methodname: %s" % methodname)

    def set_cache(self, fname, paramnames=None):
        """mol.py:217-250 writes the integral tensors to an h5 file; the MI355X path keeps them in HBM and refills them in
        milliseconds -- the file cache (out of scope) is not provided"""
        raise NotImplementedError("set_cache: the h5 parameter cache of the reference is not part of dqc_amd")

    def make_copy(self, **kwargs):
        """a new Mol identical to this one except for the constructor arguments given (mol.py:298-326)"""
        parameters = {"moldesc": (self._atomzs, self._atompos), "basis": self._basis_inp,
                      "orthogonalize_basis": self._orthogonalize_basis, "ao_parameterizer": self._aoparamzer,
                      "grid": self._grid_inp, "spin": self._spin, "charge": self._charge,
                      "orb_weights": self._user_weights, "efield": self._efield, "vext": self._vext,
                      "dtype": self._dtype, "device": self._device}
        parameters.update(kwargs)
        if parameters["orb_weights"] is not None:  # spin / charge follow from the weights
            parameters.pop("spin"), parameters.pop("charge")
        return Mol(**parameters)

    def requires_grid(self):
        """mol.py:285-286: only an external potential needs the grid outside KS"""
        return self._vext is not None

    def setup_grid(self):
        if self._grid is None:
            # element-wise grid presets and Becke radii by the nearest element (mol.py:262-267: atomzs_int)
            self._grid = get_predefined_grid(self._grid_inp, [int(round(float(z))) for z in self._atomzs],
                                             self._atompos.to(self._device),
                                             dtype=self._dtype, device=self._device)

    def get_grid(self):
        if self._grid is None:
            raise RuntimeError("Please run mol.setup_grid() first before calling get_grid()")
        return self._grid

    def get_nuclei_energy(self):
        """E_nn of the caller's positions and charges (differentiable through them, as the reference's mol.py:252-260); the
        SCF engine adds the detached value"""
        pos = self._grad_leaves["atompos"]
        z = self._grad_leaves.get("atomzs", self._atomzs).to(self._dtype)
        r = torch.cdist(pos, pos) + torch.eye(len(z), dtype=self._dtype)
        q = (z.unsqueeze(0) * z.unsqueeze(1)) / r
        return (torch.sum(q) - torch.sum(torch.diagonal(q))) * 0.5

    def _occnumber(self, a, n=None):
        """occupations (at most 1 each) of the lowest orbitals summing to `a`: floor(a) ones, then the fractional rest
        (dqc/utils/safeops.py:21-60); `n` pads with empty orbitals"""
        import math
        lo, hi = int(math.floor(a + 1e-12)), int(math.ceil(a - 1e-12))
        w = torch.zeros(max(hi, n or 0), dtype=self._dtype, device=self._device)
        w[:lo] = 1.0
        if hi > lo:
            w[hi - 1] = a - lo
        return w

    def get_orbweight(self, polarized: bool = False):
        """occupation numbers of the lowest orbitals (mol.py:421-443, safeops.occnumber), or the user's `orb_weights`"""
        if self._user_weights is not None:
            w = self._user_weights
            return w if polarized else w.u + w.d
        wu = self._occnumber(self._nup)
        if polarized:
            from .utils.datastruct import SpinParam
            # mol.py:437-441: an empty spin-down channel keeps one (empty) orbital
            wd = self._occnumber(self._ndn) if self._ndn > 0 else self._occnumber(0, n=1)
            return SpinParam(u=wu, d=wd)
        return wu + self._occnumber(self._ndn, n=wu.numel())
