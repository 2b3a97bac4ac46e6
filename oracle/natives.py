"""oracle/natives.py -- TEST INFRASTRUCTURE ONLY.

ctypes binding of oracle/liboracle_cint.so (the C restatement of the libcint /
libcgto arithmetic the reference reaches through dqclibs:
dqc/hamilton/intor/molintor.py:590-708, dqc/hamilton/intor/gtoeval.py:196-239).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "liboracle_cint.so")
        src = os.path.join(_HERE, "cint_oracle.c")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            build()
        _LIB = ctypes.CDLL(so)
    return _LIB


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _tab(t):
    return (_p(t.atm, ctypes.c_int), ctypes.c_int(t.natm), _p(t.bas, ctypes.c_int),
            ctypes.c_int(t.nbas), _p(t.env))


def int1e(which, t, zs=None):
    """which: 'ovlp' | 'kin' | 'nuc' -> (nao, nao); 'r0' -> (3, nao, nao), 'r0r0' -> (9, nao, nao): multipole moments about
    the origin (intor.int1e("r0" * n), hcgto.py:117-125)"""
    if which in ("r0", "r0r0"):
        codes = range(3, 6) if which == "r0" else range(6, 15)
        return np.stack([int1e(c, t) for c in codes])
    code = which if isinstance(which, int) else {"ovlp": 0, "kin": 1, "nuc": 2}[which]
    out = np.zeros((t.nao, t.nao))
    zp = None
    if zs is not None:
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        zp = _p(zs)
    lib().orc_int1e(ctypes.c_int(code), _p(out), *_tab(t), zp)
    return out


def int2e_s4(t):
    """packed (npair, npair), pair index i(i+1)/2+j"""
    npair = t.nao * (t.nao + 1) // 2
    out = np.zeros((npair, npair))
    lib().orc_int2e_s4(_p(out), *_tab(t))
    return out


def int2e_s8(t):
    """packed lower triangle of the s4 matrix: out[P (P + 1) / 2 + Q], P >= Q AO-pair indices (29 GB for nao 412)"""
    npair = t.nao * (t.nao + 1) // 2
    out = np.zeros(npair * (npair + 1) // 2)
    lib().orc_int2e_s8(_p(out), *_tab(t))
    return out


def symv_s8(packed, x):
    """y = M x with M the symmetric matrix held as the packed lower triangle of int2e_s8"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    lib().orc_symv_s8(_p(y), _p(packed), _p(x), ctypes.c_longlong(x.size))
    return y


def fills4(packed, nao):
    out = np.empty((nao, nao, nao, nao))
    lib().orc_fills4(_p(out), _p(np.ascontiguousarray(packed)), ctypes.c_int(nao))
    return out


def int2e(t):
    """dense (nao,)*4 like molintor.elrep after S4Symmetry expansion"""
    return fills4(int2e_s4(t), t.nao)


def int2e_quartets(t, quartets):
    """spherical blocks (sa, sb, sc, sd) of the listed shell quartets (nq, 4) -- for bases whose packed matrix
    does not fit the host (the numbers are those int2e_s4 would scatter)"""
    q = np.ascontiguousarray(quartets, dtype=np.int32).reshape(-1, 4)
    dims = 2 * t.bas[q, 1] + 1                      # (nq, 4)
    sizes = np.prod(dims, axis=1).astype(np.int64)
    offs = np.zeros(len(q) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offs[1:])
    out = np.zeros(int(offs[-1]))
    lib().orc_int2e_quartets(_p(out), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), _p(q, ctypes.c_int),
                             ctypes.c_int(len(q)), *_tab(t))
    return [out[offs[i]:offs[i + 1]].reshape(tuple(int(d) for d in dims[i])) for i in range(len(q))]


def int3c2e(tc, orb_range, aux_range):
    """(ij|k) over the concatenated tables `tc`: orbital shells [s0, s1), auxiliary shells [k0, k1) -> (nao, nao, naux)"""
    (s0, s1), (k0, k1) = orb_range, aux_range
    nao = int(tc.ao_loc[s1] - tc.ao_loc[s0])
    naux = int(tc.ao_loc[k1] - tc.ao_loc[k0])
    out = np.zeros((nao, nao, naux))
    lib().orc_int3c2e(_p(out), *_tab(tc), *(ctypes.c_int(int(v)) for v in (s0, s1, k0, k1)))
    return out


def int2c2e(tc, aux_range):
    """(k|l) over auxiliary shells [k0, k1) of the concatenated tables -> (naux, naux)"""
    k0, k1 = aux_range
    naux = int(tc.ao_loc[k1] - tc.ao_loc[k0])
    out = np.zeros((naux, naux))
    lib().orc_int2c2e(_p(out), *_tab(tc), ctypes.c_int(int(k0)), ctypes.c_int(int(k1)))
    return out


def eval_gto(t, rgrid, deriv=0):
    """deriv 0: (nao, ngrid); 1: (3, nao, ngrid); 2: laplacian (nao, ngrid)"""
    rgrid = np.ascontiguousarray(rgrid, dtype=np.float64)
    ng = rgrid.shape[0]
    shape = (3, t.nao, ng) if deriv == 1 else (t.nao, ng)
    out = np.zeros(shape)
    lib().orc_eval_gto(ctypes.c_int(deriv), _p(out), _p(rgrid), ctypes.c_int(ng), *_tab(t))
    return out


def cart2sph(l):
    nc = (l + 1) * (l + 2) // 2
    out = np.zeros((2 * l + 1, nc))
    lib().orc_cart2sph(ctypes.c_int(l), _p(out))
    return out


def boys(mmax, T):
    out = np.zeros(mmax + 1)
    lib().orc_boys(ctypes.c_int(mmax), ctypes.c_double(T), _p(out))
    return out


def num_threads():
    return lib().orc_num_threads()


# ------------------------------------------------------------------------------------------------
# derivative integrals (gradient checks): d/dA with A the centre of the FIRST function, raw Cartesian
# monomials (cart=True) or solid harmonics; see orc_int1e_ip / orc_int2e_ip_quartets / orc_df_ip
# ------------------------------------------------------------------------------------------------
def _ncart(l):
    return (l + 1) * (l + 2) // 2


def ao_count(t, cart=False, shells=None):
    ls = t.bas[:, 1] if shells is None else t.bas[shells[0]:shells[1], 1]
    return int(sum(_ncart(int(l)) if cart else 2 * int(l) + 1 for l in ls))


def ao_atom(t, cart=False):
    """owning atom of every AO (spherical or Cartesian)"""
    return np.concatenate([[int(b[0])] * (_ncart(int(b[1])) if cart else 2 * int(b[1]) + 1) for b in t.bas]).astype(np.int64)


def int1e_ip(which, t, zs=None, cart=False):
    """which 'ovlp' | 'kin' | 'nuc' -> (3, n, n): out[d, i, j] = d/dA_d <i|O|j>, A the centre of i (for 'nuc' the basis-centre
    term only, V = all nuclei); 'nuc_op' -> (natm, 3, n, n): d/dC_d <i|-Z_C/|r - C||j> (the operator term of nucleus C)"""
    code = {"ovlp": 0, "kin": 1, "nuc": 2, "nuc_op": 3}[which]
    n = ao_count(t, cart)
    out = np.zeros(((t.natm,) if code == 3 else ()) + (3, n, n))
    zp = None
    if zs is not None:
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        zp = _p(zs)
    lib().orc_int1e_ip(ctypes.c_int(code), ctypes.c_int(int(cart)), _p(out), *_tab(t), zp)
    return out


def int2e_ip_quartets(t, quartets, cart=False):
    """(d/dA a b|c d) of the listed shell quartets (nq, 4): blocks (3, da, db, dc, dd), A the centre of the first shell"""
    q = np.ascontiguousarray(quartets, dtype=np.int32).reshape(-1, 4)
    ls = t.bas[q, 1]
    dims = (ls + 1) * (ls + 2) // 2 if cart else 2 * ls + 1
    sizes = 3 * np.prod(dims, axis=1).astype(np.int64)
    offs = np.zeros(len(q) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offs[1:])
    out = np.zeros(int(offs[-1]))
    lib().orc_int2e_ip_quartets(ctypes.c_int(int(cart)), _p(out), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                _p(q, ctypes.c_int), ctypes.c_int(len(q)), *_tab(t))
    return [out[offs[i]:offs[i + 1]].reshape((3,) + tuple(int(d) for d in dims[i])) for i in range(len(q))]


def eri_grad(t, dm, jscale=1.0, kscale=1.0, cart=False):
    """(natm, 3): sum_{a in A} sum_bcd (d_A a b|c d) [2 jscale D_ab D_cd - kscale D_ac D_bd], D symmetric (n, n)"""
    dm = np.ascontiguousarray(dm, dtype=np.float64)
    assert dm.shape == (ao_count(t, cart),) * 2
    g = np.zeros((t.natm, 3))
    lib().orc_eri_grad(ctypes.c_int(int(cart)), _p(g), _p(dm), ctypes.c_double(jscale), ctypes.c_double(kscale), *_tab(t))
    return g


def df_ip(which, tc, orb_range, aux_range, cart=False):
    """concatenated tables: 'ij|k' -> (3, n, n, naux) = (d/dA_i i j|k); 'k' -> (3, n, n, naux) = (i j|d/dC k);
    '2c' -> (3, naux, naux) = (d/dC k|l)"""
    code = {"ij|k": 0, "k": 1, "2c": 2}[which]
    (s0, s1), (k0, k1) = orb_range, aux_range
    n, naux = ao_count(tc, cart, (s0, s1)), ao_count(tc, cart, (k0, k1))
    out = np.zeros((3, naux, naux) if code == 2 else (3, n, n, naux))
    lib().orc_df_ip(ctypes.c_int(code), ctypes.c_int(int(cart)), _p(out), *_tab(tc),
                    *(ctypes.c_int(int(v)) for v in (s0, s1, k0, k1)))
    return out


def int1e_grad(t, dm, wm, zs=None, cart=False):
    """(natm, 3): 2 sum_{a in A} sum_b [D_ab <d_A a|T + V|b> - W_ab <d_A a|b>] + sum_ab D_ab d/dC <a|V_C|b> -- the contraction
    dqc_int1e_grad performs (D, W symmetric), the operator term from its own integrals (no translational invariance)"""
    at = ao_atom(t, cart)
    g = np.zeros((t.natm, 3))
    h = int1e_ip("kin", t, cart=cart) + int1e_ip("nuc", t, zs, cart=cart)
    s = int1e_ip("ovlp", t, cart=cart)
    per_ao = 2.0 * (np.einsum("dij,ij->id", h, dm) - np.einsum("dij,ij->id", s, wm))
    np.add.at(g, at, per_ao)
    g += np.einsum("cdij,ij->cd", int1e_ip("nuc_op", t, zs, cart=cart), dm)
    return g


def df_grad(tc, orb_range, aux_range, dm, coef, cart=False):
    """(natm_tc, 3) over the concatenated tables: sum D_ij c_k d(ij|k) - 1/2 c^T dM c (what dqc_df_grad adds), D symmetric"""
    (s0, s1), (k0, k1) = orb_range, aux_range
    at = ao_atom(tc, cart)
    n = ao_count(tc, cart, (s0, s1))
    ao0 = ao_count(tc, cart, (0, s0))
    ax0 = ao_count(tc, cart, (0, k0))
    orb_at, aux_at = at[ao0:ao0 + n], at[ax0:ax0 + len(coef)]
    g = np.zeros((tc.natm, 3))
    np.add.at(g, orb_at, 2.0 * np.einsum("dijk,ij,k->id", df_ip("ij|k", tc, orb_range, aux_range, cart), dm, coef))
    np.add.at(g, aux_at, np.einsum("dijk,ij,k->kd", df_ip("k", tc, orb_range, aux_range, cart), dm, coef))
    np.add.at(g, aux_at, -np.einsum("dkl,k,l->kd", df_ip("2c", tc, orb_range, aux_range, cart), coef, coef))
    return g
