"""Basis-set and geometry input, mirroring the reference's dqc/api/loadbasis.py (Gaussian94 parser,
one CGTOBasis per contraction column :54-83; file naming :89-122) and dqc/api/parser.py:8-62.
The tables ship with the package (dqc_amd/data/basis/<normalised name>/<ZZ>.gaussian94) because there
is no network; the reference downloads the same files from basis_set_exchange (loadbasis.py:124-128)."""
import os
from typing import List

import numpy as np
import torch

from .utils.datastruct import CGTOBasis, AtomCGTOBasis

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "basis")
periodic_table_atomz = {s: i for i, s in enumerate(
    ["X", "H", "He", "Li", "Be", "B", "C", "N", "O", "F", "Ne", "Na", "Mg", "Al", "Si", "P", "S", "Cl", "Ar"])}
_SPDF = {"s": 0, "p": 1, "d": 2, "f": 3, "g": 4, "h": 5, "i": 6}


def get_atomz(elmt):
    if isinstance(elmt, str):
        return periodic_table_atomz[elmt]
    if isinstance(elmt, torch.Tensor):
        return elmt.item()
    return elmt


def _normalize_basisname(name):
    b = name.lower()
    for a, r in (("+", "p"), ("*", "s"), ("(", "_"), (")", "_"), (",", "_")):
        b = b.replace(a, r)
    return b


_BASIS_CACHE = {}


def loadbasis(cmd: str, dtype=torch.float64, device=torch.device("cpu"), requires_grad=False) -> List[CGTOBasis]:
    """cmd = "<atomz>:<basis name>", e.g. "8:cc-pVDZ" -> list of normalised CGTOBasis (loadbasis.py:11-83).  Parsed and normalised
    once per (element, basis): later calls get fresh CGTOBasis objects over the same (read-only) tensors."""
    import dataclasses
    key = (cmd.strip().lower(), dtype, str(device))
    if key not in _BASIS_CACHE:
        _BASIS_CACHE[key] = _loadbasis(cmd, dtype, device)
    return [dataclasses.replace(b) for b in _BASIS_CACHE[key]]


def _basis_file(name: str, atomz: int):
    """the Gaussian94 table of (basis, element): dqc_amd/data/basis/<normalised name>/<ZZ>.gaussian94, then the same layout under
    every directory of $DQC_AMD_BASIS_PATH (os.pathsep-separated) -- where tables from basis_set_exchange can be dropped in, the
    file naming of the reference's own cache (loadbasis.py:89-122); None when there is none"""
    sub = os.path.join(_normalize_basisname(name.strip()), "%02d.gaussian94" % atomz)
    for root in [_DATA] + [d for d in os.environ.get("DQC_AMD_BASIS_PATH", "").split(os.pathsep) if d]:
        f = os.path.join(root, sub)
        if os.path.exists(f):
            return f
    return None


def _loadbasis(cmd: str, dtype, device) -> List[CGTOBasis]:
    atomz_str, raw = cmd.split(":")
    atomz = int(atomz_str)
    fpath = _basis_file(raw, atomz)
    if fpath is None:
        raise RuntimeError("The %s basis for atomz %d is not shipped with dqc_amd (%s) and cannot be downloaded here; "
                           "Gaussian94 tables from basis_set_exchange can be put under $DQC_AMD_BASIS_PATH/<name>/<ZZ>.gaussian94"
                           % (raw, atomz, os.path.join(_DATA, _normalize_basisname(raw.strip()), "%02d.gaussian94" % atomz)))
    with open(fpath) as f:
        lines = f.read().split("\n")
    while True:
        line = lines.pop(0)
        if line == "" or line.startswith("!"):
            continue
        break
    res = []
    while lines:
        line = lines.pop(0)
        if line.startswith("**"):
            break
        desc = line.split()
        nlines = int(desc[1])
        if nlines == 0:
            raise RuntimeError("Zero line on basis %s" % fpath)
        alphas, coeffsT = [], []
        for _ in range(nlines):
            ac = [float(x.replace("D", "E")) for x in lines.pop(0).split()]
            alphas.append(ac[0])
            coeffsT.append(ac[1:])
        coeffs = list(zip(*coeffsT))
        s = desc[0]
        if len(s) != len(coeffs):
            if len(coeffs) % len(s) != 0:
                raise RuntimeError("Do not know how to read orbital %s with %d coefficient columns" % (s, len(coeffs)))
            s = s * (len(coeffs) // len(s))
        alpha = torch.tensor(alphas, dtype=dtype, device=device)
        for c, ch in zip(coeffs, s.lower()):
            b = CGTOBasis(angmom=_SPDF[ch], alphas=alpha, coeffs=torch.tensor(c, dtype=dtype, device=device))
            b.wfnormalize_()
            res.append(b)
    return res


def parse_moldesc(moldesc, dtype=torch.float64, device=torch.device("cpu")):
    """'H 1 0 0; H -1 0 0' (Bohr) or (atomzs, atompos) -> (atomzs tensor, atompos (natm,3) tensor)"""
    if isinstance(moldesc, str):
        elmts = [[get_atomz(c.strip()) if i == 0 else float(c.strip()) for i, c in enumerate(line.split())]
                 for line in moldesc.split(";") if line.strip()]
        atomzs = torch.tensor([line[0] for line in elmts], device=device)
        atompos = torch.tensor([line[1:] for line in elmts], dtype=dtype, device=device)
    else:
        atomzs_raw, atompos_raw = moldesc
        assert len(atomzs_raw) == len(atompos_raw), "Mismatch length of atomz and atompos"
        assert len(atomzs_raw) > 0, "Empty atom list"
        if not isinstance(atomzs_raw, torch.Tensor):
            zl = [get_atomz(at) for at in atomzs_raw]
            # fractional charges straight to the working precision (torch.tensor of Python floats would be float32)
            atomzs = torch.tensor(zl, dtype=dtype if any(isinstance(z, float) for z in zl) else None, device=device)
        else:
            atomzs = atomzs_raw.to(device)
        atompos = torch.as_tensor(np.asarray(atompos_raw) if not isinstance(atompos_raw, torch.Tensor)
                                  else atompos_raw, dtype=dtype).to(device)
    if atomzs.is_floating_point():
        atomzs = atomzs.to(dtype)
    return atomzs, atompos


def make_atombases(atomzs, atompos, basis) -> List[AtomCGTOBasis]:
    """basis: str | list of str | list of CGTOBasis | list of list of CGTOBasis | dict keyed by element symbol or atomic
    number (the forms of dqc/system/mol.py:357-400)"""
    natm = len(atomzs)
    out = []
    for i in range(natm):
        z = atomzs[i].item() if isinstance(atomzs[i], torch.Tensor) else atomzs[i]
        zi = int(round(z))  # a fractional charge takes the basis of the NEAREST element (mol.py:112-113: torch.round)
        if isinstance(basis, str):
            b = loadbasis("%d:%s" % (zi, basis))
        elif isinstance(basis, dict):
            bi = basis[zi] if zi in basis else basis[[k for k, v in periodic_table_atomz.items() if v == zi][0]]
            b = loadbasis("%d:%s" % (zi, bi)) if isinstance(bi, str) else bi
        elif len(basis) > 0 and isinstance(basis[0], CGTOBasis):
            b = basis  # one flat list of CGTOBasis: the same shells on every atom (mol.py:385-387)
        else:
            assert len(basis) == natm, "a basis list needs one entry per atom"
            bi = basis[i]
            b = loadbasis("%d:%s" % (zi, bi)) if isinstance(bi, str) else bi
        out.append(AtomCGTOBasis(atomz=z, bases=b, pos=atompos[i]))
    return out


def even_tempered_aux(atomz: int, beta: float = 2.5, dtype=torch.float64) -> List[CGTOBasis]:
    """Built-in even-tempered auxiliary basis, auxbasis="etb[:beta]": uncontracted shells with exponents a0 beta^k
        Z <= 2 :  s x 6 (a0 0.15), p x 3 (0.4), d x 1 (0.9)
        Z  > 2 :  s x 9 (a0 0.15), p x 6 (0.25), d x 4 (0.35), f x 2 (0.6)
    DFMol takes any list of CGTOBasis (dqc/system/mol.py:193-198); this one needs no external data."""
    spec = [(0, 6, 0.15), (1, 3, 0.4), (2, 1, 0.9)] if atomz <= 2 else [(0, 9, 0.15), (1, 6, 0.25), (2, 4, 0.35), (3, 2, 0.6)]
    out = []
    for l, n, a0 in spec:
        for k in range(n):
            b = CGTOBasis(angmom=l, alphas=torch.tensor([a0 * beta ** k], dtype=dtype), coeffs=torch.tensor([1.0], dtype=dtype))
            b.wfnormalize_()
            out.append(b)
    return out


def product_etb_aux(atomz: int, orb_bases: List[CGTOBasis], beta: float = 2.0, dtype=torch.float64) -> List[CGTOBasis]:
    """Auxiliary (Coulomb-fitting) basis GENERATED from the atom's orbital basis, auxbasis="autoaux[:beta]" -- the stand-in for
    the named JK-fit sets, which are external data that cannot be fetched here.  Products of two orbital functions on one
    centre carry exponents a1 + a2 and angular momenta |l1 - l2| ... l1 + l2 (step 2), so for every auxiliary l up to
        l_aux = min(max(2 l_occ, l_basis) + 1, 4)          (l_occ: highest occupied atomic shell, l_basis: highest orbital shell)
    an even-tempered, uncontracted row  a_k = lo beta^k  spans [lo, hi]:
        lo = the smallest a1 + a2 over the pairs that reach l,
        hi = the largest a1 + a2 over those pairs, capped at  2 a_s,max / (c 8^l)  (c = 15 behind a 1s core; H / He: 2 and a
             factor 3 per l): the optimised fitting sets stop one to two decades below the tightest orbital products
             -- core-core products that barely move valence energies -- and so does this one.
    Accuracy against the exact Coulomb operator is measured in tests / bench (`df` leg); the round-1 "etb" set stays available."""
    import math
    emin, emax = {}, {}
    for b in orb_bases:
        a = b.alphas.detach().cpu()
        l = int(b.angmom)
        emin[l] = min(emin.get(l, float("inf")), float(a.min()))
        emax[l] = max(emax.get(l, 0.0), float(a.max()))
    ls = sorted(emin)
    l_occ = 0 if atomz <= 4 else 1
    l_aux = min(max(2 * l_occ, ls[-1]) + 1, 4)
    light = atomz <= 2
    out = []
    for l in range(l_aux + 1):
        pairs = [(a, b) for a in ls for b in ls if a <= b and abs(a - b) <= l <= a + b and (a + b - l) % 2 == 0]
        if not pairs:
            pairs = [(a, b) for a in ls for b in ls if a <= b and a + b >= l]
        if not pairs:
            continue
        lo = min(emin[a] + emin[b] for a, b in pairs)
        hi = max(emax[a] + emax[b] for a, b in pairs)
        hi = min(hi, 2.0 * emax[0] / ((2.0 if light else 15.0) * (3.0 if light else 8.0) ** l))
        if hi < lo:
            hi = lo
        n = int(math.floor(math.log(hi / lo) / math.log(beta) + 1e-9)) + 1
        for k in range(n):
            sh = CGTOBasis(angmom=l, alphas=torch.tensor([lo * beta ** k], dtype=dtype), coeffs=torch.tensor([1.0], dtype=dtype))
            sh.wfnormalize_()
            out.append(sh)
    return out


_FIT_NAMES = ("jkfit", "jfit", "rifit", "ri", "autoaux")


def make_aux_atombases(atomzs, atompos, auxbasis, orb_atombases=None, info=None) -> List[AtomCGTOBasis]:
    """auxbasis: per-atom lists of CGTOBasis, a basis name with Gaussian94 tables under dqc_amd/data/basis or $DQC_AMD_BASIS_PATH,
    "etb[:beta]" (fixed even-tempered rows) or "autoaux[:beta]" (generated from the orbital basis, product_etb_aux).  A NAMED
    fitting set ("cc-pvtz-jkfit", the reference's default, mol.py:190-193; "def2-universal-jkfit", ...) whose tables are not
    there falls back to "autoaux" with a warning -- the reference would download it from basis_set_exchange."""
    # info (a dict, optional) receives "auxbasis_used": the set the shells really come from -- a named fitting set without tables is
    # replaced by the generated one, and a benchmark or test has to be able to assert on that
    if info is not None:
        info["auxbasis_used"] = auxbasis if isinstance(auxbasis, str) else "explicit shells"
    if isinstance(auxbasis, str):
        name = auxbasis.lower()
        if name.startswith("etb"):
            beta = float(auxbasis.split(":")[1]) if ":" in auxbasis else 2.5
            auxbasis = [even_tempered_aux(int(z), beta) for z in atomzs]
        else:
            gen = name.startswith("autoaux")
            if not gen and any(t in name for t in _FIT_NAMES):
                missing = [int(z) for z in atomzs if _basis_file(auxbasis, int(round(float(z)))) is None]
                if missing:
                    import warnings
                    warnings.warn("auxiliary basis %r: no table for Z = %s under dqc_amd/data/basis or $DQC_AMD_BASIS_PATH (the named "
                                  "fitting sets are external data, not shipped); using the generated set auxbasis='autoaux' instead"
                                  % (auxbasis, sorted(set(missing))))
                    gen = True
                    if info is not None:
                        info["auxbasis_used"] = "autoaux (generated: no tables for %r)" % auxbasis
            if gen:
                if orb_atombases is None:
                    raise RuntimeError("auxbasis='autoaux' is generated from the orbital basis: pass the orbital atom bases")
                beta = float(auxbasis.split(":")[1]) if (name.startswith("autoaux") and ":" in auxbasis) else 2.0
                auxbasis = [product_etb_aux(int(round(float(z))), ob.bases, beta) for z, ob in zip(atomzs, orb_atombases)]
    return make_atombases(atomzs, atompos, auxbasis)


def make_tables(atombases: List[AtomCGTOBasis]):
    """libcint-style (atm, bas, env) numpy tables, the layout of LibcintWrapper
    (dqc/hamilton/intor/lcintwrap.py:37-86): 20 pad doubles, then per atom xyz+0 followed by that atom's
    shells' exponents and (normalised) coefficients."""
    ptr = 20
    atm, bas, env = [], [], [0.0] * ptr
    fracz = False
    zs = []
    for ia, ab in enumerate(atombases):
        z = ab.atomz.item() if isinstance(ab.atomz, torch.Tensor) else ab.atomz
        zs.append(float(z))
        fracz = fracz or (float(z) != int(z))
        atm.append([int(z), ptr, 1, ptr + 3, 0, 0])
        env.extend([float(x) for x in ab.pos.detach().cpu()])
        env.append(0.0)
        ptr += 4
        for sh in ab.bases:
            assert sh.alphas.shape == sh.coeffs.shape and sh.alphas.ndim == 1
            sh.wfnormalize_()
            ng = len(sh.alphas)
            bas.append([ia, sh.angmom, ng, 1, 0, ptr, ptr + ng, 0])
            env.extend([float(x) for x in sh.alphas.detach().cpu()])
            env.extend([float(x) for x in sh.coeffs.detach().cpu()])
            ptr += 2 * ng
    return (np.array(atm, dtype=np.int32).reshape(-1, 6), np.array(bas, dtype=np.int32).reshape(-1, 8),
            np.array(env, dtype=np.float64), (np.array(zs) if fracz else None))


def primitive_rows(bas):
    """(prim_shell (nprim_total,), shell_off (nsh + 1,)) of a `bas` table: the shell of every primitive row and the first row of
    every shell -- the rows of dqc_amd.gradient.basis_gradient are the primitives in table order, shell by shell"""
    bas = np.asarray(bas).reshape(-1, 8)
    ng = bas[:, 2].astype(np.int64)
    shell_off = np.concatenate([[0], np.cumsum(ng)])
    return np.repeat(np.arange(bas.shape[0]), ng), shell_off


def companion_tables(atm, bas, env):
    """The per-primitive companion shells of the basis-parameter derivative (the layout dqc_eri_grad_basis builds on the host), as
    (atm, bas, env) tables with 2 * nprim_total UNCONTRACTED shells in primitive-row order:
        [0, nprim)          the primitive itself: l, exponent alpha_p, coefficient 1             d a / d c_p     = g_p
        [nprim, 2 nprim)    its r_A^2 multiple:   l + 2, exponent alpha_p, coefficient -c_p      d a / d alpha_p = -c_p r_A^2 g_p
    (Cartesian components: the l + 2 shell stands for the sum of the three components with one power raised by 2.)"""
    bas = np.asarray(bas, dtype=np.int32).reshape(-1, 8)
    env = list(np.asarray(env, dtype=np.float64))
    rows = []
    for up in (0, 1):
        for sh in bas:
            for k in range(int(sh[2])):
                a, c = env[sh[5] + k], env[sh[6] + k]
                rows.append([sh[0], sh[1] + 2 * up, 1, 1, 0, len(env), len(env) + 1, 0])
                env.extend([a, -c if up else 1.0])
    return np.asarray(atm, dtype=np.int32), np.array(rows, dtype=np.int32).reshape(-1, 8), np.array(env, dtype=np.float64)


def table_parameters(shells):
    """shells: [(angmom, alphas, coeffs, normalized)] in table order, the caller's tensors as handed to Mol.  Returns
    (alphas (nprim_total,), coeffs (nprim_total,)): the exponents and NORMALISED coefficients of make_tables' rows as torch
    functions of those tensors (CGTOBasis.wfnormalize_ is plain torch), for the chain from dE/d(table rows) to the caller's leaves"""
    al, co = [], []
    for l, a, c, normalized in shells:
        sh = CGTOBasis(angmom=l, alphas=a, coeffs=c, normalized=normalized).wfnormalize_()
        al.append(sh.alphas.to(torch.float64).cpu())
        co.append(sh.coeffs.to(torch.float64).cpu())
    return torch.cat(al), torch.cat(co)
