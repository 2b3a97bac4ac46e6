"""Host arithmetic behind contractions deeper than the 8 primitives of the bundled basis sets (no GPU): the integral kernels pick
their launch map and their primitive loop by contraction depth -- screen_bin / eri_split_lanes / the float-reciprocal index split of
csrc/eri_core.hpp, the 1 ... 45 primitive gate of csrc/host.hip -- and tests/test_gpu_deep_contractions.py runs them on the basis
defined here.  This file holds what can be said without a device:

  * the index split ipb = (int)(((float)iq + 0.5f) * (1.0f / (float)nkp)), restated in numpy float32, equals iq // nkp wherever a
    shell of at most 45 primitives can take it -- and the gate of host.hip is that 45;
  * 45 primitives pass the gate, 46 are refused with its message;
  * the deep dimer of the GPU tests occupies every contraction-depth bin, bin 0 with same-centre and cross-centre pairs (the two
    cut rules of build_pairs and screen_bin restated in numpy, tied to dqc_eri_pair_stats);
  * the 4-centre oracle itself, never run past 8 primitives either, against a 40-digit closed form on 12-primitive (ss|ss) quartets."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------
# the deep dimer (shared with tests/test_gpu_deep_contractions.py)
# ------------------------------------------------------------------------------------------------
ORIGIN = np.array([0.1, -0.2, 0.3])
SKEW = np.array([0.36, -0.48, 0.8])  # a unit vector with no zero component (tests/test_gpu_rys_range.py)
ZS = [7, 6]
GEOS = [1.4, 4.0, 9.0]
_K12, _K9 = np.arange(12.0), np.arange(9.0)
S_EXP = (6000.0 * 3.0 ** -_K12).tolist()  # 6000 ... 0.0339
S_C1 = np.exp(-((_K12 - 4) / 2.5) ** 2).tolist()
S_C2 = (-0.3 * np.exp(-((_K12 - 4) / 2.5) ** 2) + np.exp(-((_K12 - 9) / 1.5) ** 2)).tolist()  # changes sign
P_EXP = (150.0 * 2.5 ** -_K9).tolist()
P_C = np.exp(-((_K9 - 4) / 2) ** 2).tolist()
# per centre: two 12-primitive s contractions over ONE exponent set (the merged general-contraction tables), a diffuse s, a
# 9-primitive p, a 3-primitive d, an f and a two-primitive s (it fills the depth bins 4 and 6, see the coverage test)
SHELLS = [(0, S_EXP, S_C1), (0, S_EXP, S_C2), (0, [0.09], [1.0]), (1, P_EXP, P_C), (2, [2.2, 0.7, 0.25], [0.3, 0.6, 0.4]),
          (3, [0.9], [1.0]), (0, [1.1, 0.3], [0.5, 0.6])]
NSH = len(SHELLS)
NAO = 2 * sum(2 * l + 1 for l, _, _ in SHELLS)  # 38 (36 of the six shells of the table + the two-primitive s)
# the derivative tests drop the f shell and the second s contraction (the gradient kernels do not use the merged tables)
SHELLS_GRAD = [SHELLS[0], SHELLS[2], SHELLS[3], SHELLS[4], SHELLS[6]]
MAX_PRIM = 45  # csrc/host.hip: parse_basis


def deep_mol(R):
    return (ZS, np.stack([ORIGIN, ORIGIN + R * SKEW]))


def deep_tables(R, shells=None):
    from oracle import basis as ob
    shells = SHELLS if shells is None else shells
    return ob.make_tables(deep_mol(R), [shells, shells])


def limit_shells():
    """the 45-primitive centre (s and p, exponents 2e4 1.3^-k: 2e4 ... 0.19, smooth positive coefficients) and its
    single-primitive partner"""
    k = np.arange(float(MAX_PRIM))
    ex = (2.0e4 * 1.3 ** -k).tolist()
    co = (0.2 + np.exp(-((k - 30) / 9.0) ** 2)).tolist()
    return [[(0, ex, co), (1, ex, co)], [(0, [0.8], [1.0]), (1, [0.6], [1.0])]]


@pytest.fixture(scope="module")
def lib():
    from dqc_amd import build, lib as L
    build.build()
    L.load()
    return L


# ------------------------------------------------------------------------------------------------
# the index split
# ------------------------------------------------------------------------------------------------
def _split(iq, nkp, half=np.float32(0.5)):
    """eri_core.hpp: ipb = (int)(((float)iq + 0.5f) * inv_nkp), inv_nkp = 1.0f / (float)nkp -- every step rounded to float32"""
    inv = np.float32(1.0) / np.float32(nkp)
    return ((iq.astype(np.float32) + half) * inv).astype(np.int64)


def test_index_split_is_exact_up_to_the_primitive_limit():
    """for every ket depth nkp = 1 ... 45^2 and every bra depth up to 45^2: the split is exact on both sides of every multiple of
    nkp (iq = m nkp - 1 and m nkp, where a rounding error flips the quotient first) below min(2^22, 2025 nkp); the gate of
    host.hip is the 45 this range stands for, and 46 would leave the range the comment of eri_core.hpp claims"""
    src = open(os.path.join(ROOT, "dqc_amd", "csrc", "host.hip")).read()
    gate = re.search(r"h\.nprim < 1 \|\| h\.nprim > (\d+)", src)
    assert gate and int(gate.group(1)) == MAX_PRIM, "the primitive gate of parse_basis moved: this test covers 1 ... 45 only"
    assert "1 ... %d primitives" % MAX_PRIM in src
    assert MAX_PRIM ** 4 < 2 ** 22 <= (MAX_PRIM + 1) ** 4
    core = open(os.path.join(ROOT, "dqc_amd", "csrc", "eri_core.hpp")).read()
    assert "(int)(((float)iq + 0.5f) * inv_nkp)" in core and "inv_nkp = 1.0f / (float)(nkp > 0 ? nkp : 1)" in core
    npp = MAX_PRIM ** 2
    margin = 1.0
    for nkp in range(1, npp + 1):
        m = np.arange(1, min(2 ** 22 // nkp, npp) + 1, dtype=np.int64)
        hi = m * nkp  # first index of bra primitive pair m
        hi = hi[hi < min(2 ** 22, npp * nkp)]
        lo = m * nkp - 1  # last index of bra primitive pair m - 1
        assert lo.max() < min(2 ** 22, npp * nkp)
        assert np.array_equal(_split(lo, nkp), lo // nkp), nkp
        assert np.array_equal(_split(hi, nkp), hi // nkp), nkp
        # distance of the float32 quotient from the integer it must not cross, in units of the ideal 1 / (2 nkp)
        inv = np.float32(1.0) / np.float32(nkp)
        ql = ((lo.astype(np.float32) + np.float32(0.5)) * inv).astype(np.float64)
        margin = min(margin, float(((m - ql) * 2 * nkp).min()))
        if hi.size:
            qh = ((hi.astype(np.float32) + np.float32(0.5)) * inv).astype(np.float64)
            margin = min(margin, float(((qh - hi // nkp) * 2 * nkp).min()))
    print("index split: smallest distance from the next integer %.3f of 1 / (2 nkp)" % margin)
    assert margin > 0.0
    # the half is what makes it exact: without it the quotient of a multiple of nkp falls below its integer
    bad = [nkp for nkp in range(1, npp + 1)
           if not np.array_equal(_split(np.arange(1, 46, dtype=np.int64) * nkp, nkp, np.float32(0.0)), np.arange(1, 46))]
    assert bad, "the split without + 0.5f should fail somewhere"


# ------------------------------------------------------------------------------------------------
# the limit
# ------------------------------------------------------------------------------------------------
def _one_deep_shell(l, n):
    from oracle import basis as ob
    ex = (2.0e4 * 1.3 ** -np.arange(float(n))).tolist()
    return ob.make_tables(([3, 1], [[0.0, 0.0, 0.0], [0.0, 0.3, 2.0]]), [[(l, ex, [1.0] * n)], [(0, [0.8], [1.0])]])


@pytest.mark.parametrize("l", [0, 1, 3])
def test_45_primitives_pass_the_gate_and_46_are_refused(lib, l):
    t = _one_deep_shell(l, MAX_PRIM)
    st = lib.eri_pair_stats(lib.Tables(t.atm, t.bas, t.env), merge=False)
    assert st["groups"] == 2 and st["pairs"] == 3
    # (every pair of the deep shell with itself survives the cuts: one centre, arg = 0)
    assert MAX_PRIM ** 2 + 1 <= st["primitive_pairs"] <= MAX_PRIM ** 2 + MAX_PRIM + 1
    assert lib.eri_pair_stats(lib.Tables(t.atm, t.bas, t.env), merge=True)["primitive_pairs"] == st["primitive_pairs"]
    t = _one_deep_shell(l, MAX_PRIM + 1)
    for merge in (False, True):
        with pytest.raises(lib.DqcAmdError, match=r"1 \.\.\. 45 primitives"):
            lib.eri_pair_stats(lib.Tables(t.atm, t.bas, t.env), merge=merge)
    t = _one_deep_shell(l, 1)
    t.bas[0, 2] = 0
    with pytest.raises(lib.DqcAmdError, match=r"1 \.\.\. 45 primitives"):
        lib.eri_pair_stats(lib.Tables(t.atm, t.bas, t.env), merge=False)


# ------------------------------------------------------------------------------------------------
# coverage of the test basis
# ------------------------------------------------------------------------------------------------
def screen_bin(npp):
    """eri_core.hpp: 0 = deepest (> 64 primitive pairs) ... 7 = one primitive pair (or none)"""
    for b, edge in enumerate((64, 32, 16, 8, 4, 2, 1)):
        if npp > edge:
            return b
    return 7


def pair_depths(t):
    """[(shell a, shell b, same centre, primitive pairs kept)] for the shell pairs a >= b of the (unmerged) tables: the two cut
    rules of build_pairs, arg = ea eb / p |AB|^2 > 100 and |c_a c_b K / p| (1 + |AB|)^(la + lb) < 1e-20"""
    out = []
    sh = []
    for s_ in t.bas:
        at, l, npr = int(s_[0]), int(s_[1]), int(s_[2])
        sh.append((at, l, t.env[s_[5]:s_[5] + npr], t.env[s_[6]:s_[6] + npr], t.env[t.atm[at][1]:t.atm[at][1] + 3]))
    for i in range(len(sh)):
        for j in range(i + 1):
            (ata, la, ea, ca, ra), (atb, lb, eb, cb, rb) = sh[i], sh[j]
            ab2 = float(((ra - rb) ** 2).sum())
            p = ea[:, None] + eb[None, :]
            arg = ea[:, None] * eb[None, :] / p * ab2
            f = np.abs(ca[:, None] * cb[None, :] * np.exp(-arg) / p)
            for _ in range(la + lb):
                f = f * (1.0 + np.sqrt(ab2))
            out.append((i, j, ata == atb, int(((arg <= 100.0) & (f >= 1e-20)).sum())))
    return out


def test_screen_bin_restatement_matches_the_source():
    core = open(os.path.join(ROOT, "dqc_amd", "csrc", "eri_core.hpp")).read()
    assert "constexpr int SCREEN_NBIN = 8;" in core
    assert ("return npp > 64 ? 0 : (npp > 32 ? 1 : (npp > 16 ? 2 : (npp > 8 ? 3 : (npp > 4 ? 4 : (npp > 2 ? 5 : (npp > 1 ? 6 : 7))))));"
            in core)
    assert [screen_bin(n) for n in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 144, 2025)] == \
        [7, 7, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0]


# bin-0 pairs (same centre, cross centre) and the pairs of every bin per geometry: what the basis above gives under the two rules
_BIN0 = {1.4: (12, 9), 4.0: (12, 8), 9.0: (12, 0)}


def test_deep_dimer_occupies_every_depth_bin(lib):
    """every bin 0 ... 7 holds a pair in at least one geometry, bin 0 same-centre and cross-centre pairs at R = 1.4 and 4.0, and
    the restatement keeps as many primitive pairs as the library's own pair tables"""
    assert abs(float(SKEW @ SKEW) - 1.0) < 1e-15 and min(S_EXP + P_EXP) > 0.03 and max(S_EXP + P_EXP) <= 6000.0
    seen = set()
    for R in GEOS:
        t = deep_tables(R)
        assert t.nao == NAO and t.nbas == 2 * NSH
        pairs = pair_depths(t)
        assert len(pairs) == t.nbas * (t.nbas + 1) // 2
        hist = np.bincount([screen_bin(n) for _, _, _, n in pairs], minlength=8)
        same0 = sum(1 for _, _, same, n in pairs if same and screen_bin(n) == 0)
        cross0 = sum(1 for _, _, same, n in pairs if not same and screen_bin(n) == 0)
        print("R = %.1f: pairs per bin %s, bin 0 same-centre %d cross-centre %d, deepest %d" % (R, hist.tolist(), same0, cross0,
                                                                                             max(n for _, _, _, n in pairs)))
        seen |= {b for b in range(8) if hist[b]}
        assert (same0, cross0) == _BIN0[R], (R, same0, cross0)
        if R < 9.0:
            assert same0 > 0 and cross0 > 0
        assert max(n for _, _, _, n in pairs) == 144
        st = lib.eri_pair_stats(lib.Tables(t.atm, t.bas, t.env), merge=False)
        assert st["pairs"] == len(pairs) and st["groups"] == t.nbas
        assert st["primitive_pairs"] == sum(n for _, _, _, n in pairs), R
        # merged: the two contractions of a centre become one group of two members
        assert lib.eri_pair_stats(lib.Tables(t.atm, t.bas, t.env), merge=True)["groups"] == t.nbas - 2
    assert seen == set(range(8)), sorted(seen)


def test_limit_basis_reaches_the_end_of_the_index_range(lib):
    """the basis of the on-device limit test: 45-primitive s and p on one centre, all 2025 primitive pairs of (ss), (ps), (pp) kept,
    so that the general path walks iq up to 45^4 - 1 = 4 100 624 < 2^22"""
    from oracle import basis as ob
    t = ob.make_tables(([5, 1], np.stack([ORIGIN, ORIGIN + 2.0 * SKEW])), limit_shells())
    depth = {(i, j): n for i, j, _, n in pair_depths(t)}
    assert depth[(0, 0)] == depth[(1, 0)] == depth[(1, 1)] == MAX_PRIM ** 2
    assert depth[(1, 1)] ** 2 - 1 == 4100624 < 2 ** 22
    assert 0 < depth[(2, 0)] <= MAX_PRIM and 0 < depth[(3, 1)] <= MAX_PRIM
    st = lib.eri_pair_stats(lib.Tables(t.atm, t.bas, t.env), merge=False)
    assert st["primitive_pairs"] == sum(depth.values())


# ------------------------------------------------------------------------------------------------
# the oracle at depth
# ------------------------------------------------------------------------------------------------
# (R, shell quartet): shells 0, 1 = the two 12-primitive contractions of centre 0; NSH, NSH + 1 = those of centre 1
_QUARTETS = [(1.4, (0, 0, 0, 0)), (4.0, (1, 0, 1, 1)), (1.4, (0, NSH, 0, NSH)), (4.0, (1, NSH + 1, 0, NSH)), (9.0, (0, 0, NSH + 1, NSH + 1))]


def _ssss_mpmath(t, quartet):
    """sum over the primitive quartets of 2 pi^(5/2) K_ab K_cd F_0(X) / (p q sqrt(p + q)) c_a c_b c_c c_d / (4 pi)^2 at 40 digits;
    returns (value, sum |terms| / |value|)"""
    import mpmath as mp
    mp.mp.dps = 40

    def prims(s):
        s_ = t.bas[s]
        n = int(s_[2])
        r = [mp.mpf(float(x)) for x in t.env[t.atm[int(s_[0])][1]:t.atm[int(s_[0])][1] + 3]]
        return [(mp.mpf(float(t.env[s_[5] + k])), mp.mpf(float(t.env[s_[6] + k])), r) for k in range(n)]

    def pairs(sa, sb):
        out = []
        for ea, ca, ra in prims(sa):
            for eb, cb, rb in prims(sb):
                p = ea + eb
                ab2 = sum((x - y) ** 2 for x, y in zip(ra, rb))
                out.append((p, [(ea * x + eb * y) / p for x, y in zip(ra, rb)], ca * cb * mp.exp(-ea * eb / p * ab2) / p))
        return out

    def f0(x):
        return mp.mpf(1) if x == 0 else mp.sqrt(mp.pi / x) * mp.erf(mp.sqrt(x)) / 2

    tot, tabs = mp.mpf(0), mp.mpf(0)
    ket = pairs(quartet[2], quartet[3])
    for p, P, kp in pairs(quartet[0], quartet[1]):
        for q, Q, kq in ket:
            x = p * q / (p + q) * sum((a - b) ** 2 for a, b in zip(P, Q))
            term = kp * kq * f0(x) / mp.sqrt(p + q)
            tot += term
            tabs += abs(term)
    scale = 2 * mp.pi ** mp.mpf("2.5") / (4 * mp.pi) ** 2
    return float(tot * scale), float(tabs / abs(tot))


@pytest.mark.parametrize("R,quartet", _QUARTETS, ids=["-".join(map(str, q)) + "@%g" % R for R, q in _QUARTETS])
def test_oracle_ssss_of_12_primitive_contractions_vs_40_digit_closed_form(R, quartet):
    """oracle.natives.int2e_quartets on (ss|ss) quartets of 20 736 primitive quartets each, two on one centre and three mixing
    the centres: 1e-13 relative (measured at most 2e-14; sum |terms| / |value| stays below 7: no heavy cancellation)"""
    from oracle import natives as nat
    t = deep_tables(R)
    assert [int(t.bas[s, 2]) for s in quartet] == [12] * 4 and [int(t.bas[s, 1]) for s in quartet] == [0] * 4
    got = float(nat.int2e_quartets(t, [quartet])[0].reshape(()))
    ref, cancel = _ssss_mpmath(t, quartet)
    err = abs(got - ref) / abs(ref)
    print("oracle (%s) at R = %g: %.16e, relative deviation %.2e, sum|terms| / |value| %.2f" % (quartet, R, got, err, cancel))
    assert cancel < 10.0
    assert err <= 1e-13, (got, ref)
