"""Exact-arithmetic cases for the tile kernels of dqc_amd/csrc/fock.hip (tests/test_gpu_fock_tiles.py, tests/test_fock_tile_cases_cpu.py).

Every input is a small dyadic rational: a non-zero integer of a few bits times a fixed power of two.  Under the BUDGET below every
product and every partial sum of the chains computed here is exactly representable in fp64 in ANY order of summation, so the fp64
MFMA, the four-wave split of K and the LDS reduction of `ft_tile` round nowhere and a kernel has to return the host result bit for
bit.  No element is zero: dropping or doubling any single term, or reading a clamped element without zeroing it, changes the result.

BUDGET.  The unit of an array is the largest power of two all its elements are integer multiples of.  A product A @ B is inside
the budget when max(|A| @ |B|) < 2^53 unit(A) unit(B): every term is a multiple of the product unit and every partial sum, in
whatever order, stays below 2^53 units.  Sums and elementwise products are held to the same rule.  `mm`, `add`, `sub`, `mul`,
`dot` check it on every call and raise BudgetError: a case that breaks the budget is an error of the generator, never skipped.

The formulas (`*_chain`) are written once, over `mm` / `add` / `sub` / `mul` / `tr` / `dot`, and run on float64 arrays (the
reference the GPU tests compare with) and on `Fx` -- int64 mantissas with a common binary exponent -- for the integer cross-check
of the CPU test (`to_fx`, `same`).  This module needs no GPU and imports neither torch nor the library."""
import functools
import math

import numpy as np

LIM53 = 2.0 ** 53
LIM62 = 2.0 ** 62


class BudgetError(ValueError):
    pass


def unit_exp(a):
    """e with: every element of the float64 array `a` is an integer multiple of 2^e, e as large as possible (0 for all zeros)"""
    a = np.asarray(a, dtype=np.float64)
    nz = a[a != 0]
    if nz.size == 0:
        return 0
    m, e = np.frexp(nz)
    n = np.abs(np.ldexp(m, 53)).astype(np.int64)  # the 53-bit mantissa as an integer
    tz = np.round(np.log2((n & -n).astype(np.float64))).astype(np.int64)
    return int((e.astype(np.int64) - 53 + tz).min())


def _fits(bound, ue, what):
    top = float(np.max(bound)) if np.size(bound) else 0.0
    if not top < math.ldexp(LIM53, ue):
        raise BudgetError("%s: magnitude bound %.3g is not below 2^53 units of 2^%d" % (what, top, ue))


class Fx:
    """n 2^e with n an int64 array: the integer arithmetic the float64 reference is checked against (every |n| < 2^62, asserted)"""

    def __init__(self, n, e):
        self.n = np.asarray(n, dtype=np.int64)
        self.e = int(e)
        assert self.n.size == 0 or float(np.abs(self.n.astype(np.float64)).max()) < LIM62

    @staticmethod
    def of(a):
        if isinstance(a, Fx):
            return a
        a = np.asarray(a, dtype=np.float64)
        e = unit_exp(a)
        n = np.ldexp(a, -e)
        assert np.all(n == np.round(n)) and (n.size == 0 or np.abs(n).max() < LIM53)
        return Fx(n.astype(np.int64), e)

    def to_float(self):
        assert self.n.size == 0 or np.abs(self.n).max() < 2 ** 53, "the integer result does not fit an fp64 mantissa"
        return np.ldexp(self.n.astype(np.float64), self.e)

    @property
    def shape(self):
        return self.n.shape

    def __getitem__(self, idx):
        return Fx(self.n[idx], self.e)

    def tr(self):
        return Fx(np.swapaxes(self.n, -1, -2), self.e)

    def _aligned(self, o):
        e = min(self.e, o.e)
        sa, sb = self.e - e, o.e - e
        assert sa < 62 and sb < 62
        for n, s in ((self.n, sa), (o.n, sb)):
            assert n.size == 0 or float(np.abs(n.astype(np.float64)).max()) * 2.0 ** s < LIM62 / 2
        return self.n << sa, o.n << sb, e

    def add(self, o):
        a, b, e = self._aligned(o)
        return Fx(a + b, e)

    def sub(self, o):
        a, b, e = self._aligned(o)
        return Fx(a - b, e)

    def mul(self, o):
        a, b = np.abs(self.n.astype(np.float64)), np.abs(o.n.astype(np.float64))
        assert float(np.max(a * b)) < LIM62
        return Fx(self.n * o.n, self.e + o.e)

    def mm(self, o):
        a, b = np.abs(self.n.astype(np.float64)), np.abs(o.n.astype(np.float64))
        assert float(np.max(a @ b)) < LIM62, "integer product beyond 2^62"
        return Fx(self.n @ o.n, self.e + o.e)

    def dot(self, o):
        a, b = np.abs(self.n.astype(np.float64)), np.abs(o.n.astype(np.float64))
        assert float(np.sum(a * b)) < LIM62
        return Fx(np.sum(self.n * o.n), self.e + o.e)


def _is_fx(*xs):
    return any(isinstance(x, Fx) for x in xs)


def _is_ld(*xs):
    """longdouble operands: the reference of the general-input tests, no budget to keep"""
    return any(getattr(x, "dtype", None) == np.longdouble for x in xs)


def mm(a, b, what="product"):
    if _is_ld(a, b):
        return a @ b
    if _is_fx(a, b):
        return Fx.of(a).mm(Fx.of(b))
    _fits(np.abs(a) @ np.abs(b), unit_exp(a) + unit_exp(b), what)
    return a @ b


def mul(a, b, what="elementwise product"):
    if _is_ld(a, b):
        return a * b
    if _is_fx(a, b):
        return Fx.of(a).mul(Fx.of(b))
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    r = a * b
    _fits(np.abs(r), unit_exp(a) + unit_exp(b), what)
    return r


def add(a, b, what="sum"):
    if _is_ld(a, b):
        return a + b
    if _is_fx(a, b):
        return Fx.of(a).add(Fx.of(b))
    _fits(np.abs(a) + np.abs(b), min(unit_exp(a), unit_exp(b)), what)
    return a + b


def sub(a, b, what="difference"):
    if _is_ld(a, b):
        return a - b
    if _is_fx(a, b):
        return Fx.of(a).sub(Fx.of(b))
    _fits(np.abs(a) + np.abs(b), min(unit_exp(a), unit_exp(b)), what)
    return a - b


def dot(a, b, what="trace"):
    """sum_ij a_ij b_ij"""
    if _is_ld(a, b):
        return np.sum(a * b)
    if _is_fx(a, b):
        return Fx.of(a).dot(Fx.of(b))
    _fits(np.sum(np.abs(a) * np.abs(b)), unit_exp(a) + unit_exp(b), what)
    return np.float64(np.sum(a * b))


def tr(a):
    return a.tr() if isinstance(a, Fx) else np.swapaxes(a, -1, -2)


def to_fx(inputs):
    """the inputs of a chain as integers (arrays -> Fx; scalars, flags and None stay)"""
    return {k: Fx.of(v) if isinstance(v, np.ndarray) else v for k, v in inputs.items()}


def same(ref, fx):
    """is the float64 result the integer one, element for element"""
    if ref is None or fx is None:
        return ref is None and fx is None
    return bool(np.array_equal(np.asarray(ref, dtype=np.float64), Fx.of(fx).to_float()))


def dyadic(rng, shape, bits, exp):
    """non-zero integers of at most `bits` bits, either sign, times 2^exp"""
    mag = rng.integers(1, 2 ** bits, size=shape)
    sgn = rng.choice(np.array([-1, 1]), size=shape)
    return np.ldexp((mag * sgn).astype(np.float64), exp)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


# ---------------------------------------------------------------------------------------------------------------------
# dqc_resp_gemm:  C[v] = alpha (op(A[v]) B[v] + (ea[m] - eb[n]) X[v][m][n])
# ---------------------------------------------------------------------------------------------------------------------
# (M, N, K, transa, nbatch, lda slack, ldb slack, ldc slack, sc slack, shared A, shared B, epilogue, alpha)
# every edge value of K {1 3 4 5 127 128 129 131 260} and of M, N {1 15 16 17 33} appears; K = 3, 5: a partial k-quad; K = 128: one
# full trip of ft_tile; 129, 131, 260: the second trip (its first step / ragged); slack 0 and > 0 on every leading dimension and
# on the batch stride of C; a zero batch stride on each operand; nbatch 1, 3, 17; both transa; with and without the epilogue
GEMM_CASES = [
    (1, 1, 1, 0, 1, 0, 0, 0, 0, False, False, False, 1.0),
    (15, 17, 3, 1, 3, 2, 1, 3, 5, False, False, True, 0.5),
    (16, 16, 4, 0, 1, 0, 0, 0, 0, False, False, True, -2.0),
    (17, 15, 5, 0, 3, 3, 0, 1, 0, True, False, True, 0.25),
    (33, 1, 127, 1, 3, 0, 4, 2, 7, False, True, False, 0.5),
    (1, 33, 128, 0, 17, 1, 0, 0, 3, False, False, False, 1.0),
    (17, 17, 129, 1, 3, 5, 3, 2, 9, False, False, True, -2.0),
    (15, 16, 131, 0, 3, 0, 0, 0, 0, True, False, False, 0.25),
    (16, 33, 260, 1, 3, 1, 2, 0, 0, False, True, True, 0.5),
    (33, 15, 129, 0, 3, 7, 1, 4, 11, False, False, False, -2.0),
    (1, 17, 260, 1, 1, 2, 0, 1, 0, False, False, True, 1.0),
    (33, 33, 128, 0, 17, 0, 2, 0, 1, True, False, True, 0.5),
    (17, 1, 131, 1, 17, 3, 0, 5, 2, False, True, False, 0.25),
]


def gemm_chain(a, b, transa, alpha, ea=None, eb=None, x=None):
    t = mm(tr(a) if transa else a, b, "op(A) B")
    if x is not None:
        t = add(t, mul(sub(ea[:, None], eb[None, :]), x, "(ea - eb) X"), "product + diagonal term")
    return mul(alpha, t, "alpha C")


def gemm_inputs(spec, general=False):
    """a (nbatch or 1, rows, cols) and b (nbatch or 1, K, N) WITHOUT slack, ea (M,), eb (N,), x (nbatch, M, N) or None"""
    M, N, K, transa, nb, _, _, _, _, a0, b0, epi, alpha = spec
    rng = _rng(11, *spec[:9], general)
    draw = (lambda shape, bits, exp: general_values(rng, shape)) if general else (lambda shape, bits, exp: dyadic(rng, shape, bits, exp))
    ashape = (1 if a0 else nb, K, M) if transa else (1 if a0 else nb, M, K)
    out = {"a": draw(ashape, 4, -2), "b": draw((1 if b0 else nb, K, N), 4, -1), "transa": transa, "alpha": alpha}
    if epi:
        out.update(ea=draw((M,), 3, -1), eb=draw((N,), 3, 0), x=draw((nb, M, N), 4, -3))
    return out


@functools.lru_cache(maxsize=None)
def gemm_case(spec):
    inp = gemm_inputs(spec)
    return inp, np.broadcast_to(gemm_chain(**inp), (spec[4], spec[0], spec[1])).copy()


# ---------------------------------------------------------------------------------------------------------------------
# resp_kappa2dm(_pm), resp_project
# ---------------------------------------------------------------------------------------------------------------------
# (nao, no, nv, nvec): K = nv {1, 19, 129} in the half transformation, K = 2 no {2, 10, 34, 66, 130} in resp_dm_kernel (2 no
# crosses 128 once, no = 65), K = nao {5, 17, 131} in both products of the projection; no = 17, 33, 65: more than one tile of
# occupied columns; M = nv = 1 and 129 in the projection
RESP_CASES = [
    (5, 1, 1, 1),
    (5, 5, 19, 4),
    (5, 33, 1, 4),
    (17, 5, 19, 4),
    (17, 17, 1, 1),
    (17, 33, 129, 1),
    (17, 1, 129, 4),
    (131, 1, 129, 4),
    (131, 5, 1, 1),
    (131, 17, 19, 1),
    (131, 33, 129, 4),
    (131, 65, 19, 1),
]


def kappa2dm_chain(kappa, cv, co, scale, sign):
    """scale (C_v kappa C_o^T + sign transpose)"""
    p = mm(mm(cv, kappa, "C_v kappa"), tr(co), "T C_o^T")
    # (the kernel sums T C_o^T and sign C_o T^T as ONE product over K = 2 no: the bound of that sum is the bound of this one)
    return mul(scale, add(p, mul(sign, tr(p))), "scale dD")


def project_chain(g, cv, co, alpha, ev=None, eo=None, kappa=None):
    return gemm_chain(cv, mm(g, co, "G C_o"), 1, alpha, ev, eo, kappa)


def resp_inputs(shape, general=False):
    nao, no, nv, nvec = shape
    rng = _rng(12, *shape, general)
    draw = (lambda s, bits, exp: general_values(rng, s)) if general else (lambda s, bits, exp: dyadic(rng, s, bits, exp))
    return {"kappa": draw((nvec, nv, no), 3, -2), "cv": draw((nao, nv), 3, -1), "co": draw((nao, no), 3, -1),
            "g": draw((nvec, nao, nao), 4, -2), "ev": draw((nv,), 3, 0), "eo": draw((no,), 3, -1),
            "scale": 0.5, "alpha": -2.0}


@functools.lru_cache(maxsize=None)
def resp_case(shape):
    i = resp_inputs(shape)
    return i, resp_chains(i)


def resp_chains(i):
    return {"plus": kappa2dm_chain(i["kappa"], i["cv"], i["co"], i["scale"], 1.0),
            "minus": kappa2dm_chain(i["kappa"], i["cv"], i["co"], i["scale"], -1.0),
            "proj": project_chain(i["g"], i["cv"], i["co"], i["alpha"]),
            "proj_diag": project_chain(i["g"], i["cv"], i["co"], i["alpha"], i["ev"], i["eo"], i["kappa"])}


# ---------------------------------------------------------------------------------------------------------------------
# fock_factor, fock_orb2dm, fock_prep
# ---------------------------------------------------------------------------------------------------------------------
# (nao, north, r): K = north in the factor {7, 14, 33, 129, 127, 257}, K = r in C diag(w) C^T {1, 16, 17, 33, 96, 128}, K = rp
# (padded r) or K = north in the AO density; north < nao three times
FACTOR_CASES = [(7, 7, 1), (17, 14, 16), (33, 33, 17), (129, 129, 33), (131, 127, 96), (260, 257, 128)]
FACTOR_MAX = (1024, 1024, 128)  # the documented maximum of the library
SQRT_W = np.array([0.5, 1.0, 2.0, 1.5, 0.25, 3.0])  # w = 1/4, 1, 4, 9/4, 1/16, 9: exact squares of dyadics


def factor_chain(x, c, sw, dm_in):
    """L = X (C sqrt(w)); D = C diag(w) C^T; the AO density from the factor, L L^T, and from a general orthogonal-basis matrix,
    X ((dm + dm^T) / 2) X^T"""
    lfac = mm(x, mul(c, sw[None, :], "C sqrt(w)"), "X (C sqrt(w))")
    w = mul(sw, sw)
    dm = mm(mul(c, w[None, :], "C w"), tr(c), "C w C^T")
    dao = mm(lfac, tr(lfac), "L L^T")
    ds = mul(0.5, add(dm_in, tr(dm_in)), "(dm + dm^T) / 2")
    dao_dm = mm(mm(x, ds, "X Ds"), tr(x), "(X Ds) X^T")
    return {"w": w, "factor": lfac, "dm": dm, "dao": dao, "dao_dm": dao_dm}


def factor_inputs(shape, general=False):
    nao, north, r = shape
    rng = _rng(13, *shape, general)
    if general:
        return {"x": general_values(rng, (nao, north)), "c": general_values(rng, (north, r)),
                "w": np.abs(general_values(rng, (r,))), "dm_in": general_values(rng, (north, north))}
    return {"x": dyadic(rng, (nao, north), 2, -1), "c": dyadic(rng, (north, r), 2, -1),
            "sw": SQRT_W[rng.integers(0, len(SQRT_W), size=r)], "dm_in": dyadic(rng, (north, north), 3, -2)}


@functools.lru_cache(maxsize=None)
def factor_case(shape):
    i = factor_inputs(shape)
    return i, factor_chain(**i)


# ---------------------------------------------------------------------------------------------------------------------
# fock_finish
# ---------------------------------------------------------------------------------------------------------------------
# (nao, north); (260, 257): nao^2 = 67600 > 65536, the second sweep of fock_combine_kernel
FINISH_SHAPES = [(7, 7), (17, 14), (131, 127), (260, 257)]
FINISH_R = 3  # columns of the factor the density of these cases is made from

# name -> (with_k, V: None | "sym" | "raw", kfrac or None, exc given, core given, want_j): the seven forms of fock_combine_kernel
# (WITH_K x HAS_V as the library reaches them), core given and omitted, J_ao wherever fock_finish hands it out
FINISH_FORMS = {
    "j": (False, None, None, False, True, True),
    "j_nocore": (False, None, None, False, False, False),
    "jk": (True, None, None, False, False, True),
    "jk_v": (True, "sym", None, False, True, False),
    "j_v": (False, "sym", None, False, True, True),
    "vraw": (False, "raw", None, False, True, False),
    "hybrid_v": (True, "sym", 0.25, True, True, False),
    "hybrid_vraw": (True, "raw", 0.5, True, False, False),
    "hybrid_v_noexc": (True, "sym", -2.0, False, True, False),
}
DET_SCALE = 2.0 ** 20   # of the J / K accumulators in deterministic mode (slot 0 of the eight-slot area)
DET_VSCALE = 2.0 ** 12  # of the raw Vxc sums


def finish_chain(dao, wj, wk, v, vraw, x, core, kfrac, with_k, hybrid):
    """F = sym(X^T (J - kfrac K / 2 + V) X) + core with J = Wj + Wj^T, K = Wk + Wk^T, V symmetric or (Vraw + Vraw^T) / 2;
    J; en = [sum D Wj, -kfrac / 2 sum D Wk] (= [tr D J / 2, -kfrac tr D K / 4]: D is symmetric)"""
    j = add(wj, tr(wj), "Wj + Wj^T")
    m = j
    k_scale = kfrac if hybrid else 1.0
    if with_k:
        m = sub(m, mul(0.5 * k_scale, add(wk, tr(wk), "Wk + Wk^T")), "J - a K / 2")
    if v is not None:
        m = add(m, mul(0.5, add(v, tr(v), "V + V^T")) if vraw else v, "M + V")
    f0 = mm(mm(tr(x), m, "X^T M"), x, "(X^T M) X")
    f = f0 if core is None else add(f0, core, "F + core")
    e_j = dot(dao, wj, "sum D Wj")
    e_k = mul(-0.5 * k_scale, dot(dao, wk, "sum D Wk")) if with_k else None
    return {"fock": f, "f0": f0, "j": j, "e_j": e_j, "e_k": e_k}


def finish_inputs(shape, general=False):
    nao, north = shape
    rng = _rng(14, *shape, general)
    if general:
        x, c, sw = general_values(rng, (nao, north)), general_values(rng, (north, FINISH_R)), np.ones(FINISH_R)
        vsym = general_values(rng, (nao, nao))
        return {"x": x, "c": c, "sw": sw, "wj": general_values(rng, (nao, nao)), "wk": general_values(rng, (nao, nao)),
                "vsym": vsym + vsym.T, "vraw": general_values(rng, (nao, nao)), "core": general_values(rng, (north, north)), "exc": -1.75}
    half = dyadic(rng, (nao, nao), 3, -3)
    return {"x": dyadic(rng, (nao, north), 2, -1), "c": dyadic(rng, (north, FINISH_R), 2, -1),
            "sw": SQRT_W[rng.integers(0, 3, size=FINISH_R)],
            "wj": dyadic(rng, (nao, nao), 3, -2), "wk": dyadic(rng, (nao, nao), 3, -3),  # asymmetric accumulators
            "vsym": half + half.T + np.diag(np.full(nao, 0.125)), "vraw": dyadic(rng, (nao, nao), 3, -4),
            "core": dyadic(rng, (north, north), 4, -2), "exc": -1.75}  # (core asymmetric: the kernel reads both triangles)


def finish_form_chain(i, dao, form):
    with_k, vkind, kfrac, _, has_core, _ = FINISH_FORMS[form]
    v = None if vkind is None else i["vsym" if vkind == "sym" else "vraw"]
    return finish_chain(dao, i["wj"], i["wk"], v, vkind == "raw", i["x"], i["core"] if has_core else None, kfrac, with_k,
                        kfrac is not None)


def finish_density(i):
    lfac = mm(i["x"], mul(i["c"], i["sw"][None, :]), "X (C sqrt(w))")
    return mm(lfac, tr(lfac), "L L^T")


@functools.lru_cache(maxsize=None)
def finish_case(shape):
    """inputs, the AO density and {form: expected outputs}"""
    i = finish_inputs(shape)
    dao = finish_density(i)
    return i, dao, {form: finish_form_chain(i, dao, form) for form in FINISH_FORMS}


# ---------------------------------------------------------------------------------------------------------------------
# general inputs: normal deviates times 10^u, u uniform in [-3, 3] per element, against a longdouble reference
# ---------------------------------------------------------------------------------------------------------------------
GENERAL_GEMM = [GEMM_CASES[6], GEMM_CASES[8]]
GENERAL_RESP = [(17, 5, 19, 4), (131, 33, 129, 4)]
GENERAL_FACTOR = [(17, 14, 16), (131, 127, 96)]
GENERAL_FINISH = [(17, 14), (131, 127)]
GENERAL_FORMS = ["jk_v", "hybrid_vraw"]


def general_values(rng, shape):
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def gamma(k):
    """2 (k + 8) 2^-53: the dot-product bound of a sum of k terms in any order, per unit of |A| @ |B|.  The factor 2 covers the
    second-order terms and the rounding of the longdouble reference, the 8 the handful of elementwise roundings around a product"""
    return 2.0 * (k + 8) * 2.0 ** -53


def ld(a):
    return None if a is None else np.asarray(a, dtype=np.longdouble)


# Bounds of |kernel - reference| for general inputs, element by element: gamma(K) |A| @ |B| per product, and for a chain the
# first-order composite: the sum of the stages' gamma on the product of the absolute matrices.  Derived, not measured.
def gemm_bound(a, b, transa, alpha, ea=None, eb=None, x=None):
    a, b = np.abs(a), np.abs(b)
    t = (tr(a) if transa else a) @ b
    if x is not None:
        t = t + (np.abs(ea)[:, None] + np.abs(eb)[None, :]) * np.abs(x)
    return gamma(b.shape[-2]) * abs(alpha) * t


def kappa2dm_bound(kappa, cv, co, scale):
    p = np.abs(cv) @ np.abs(kappa) @ np.abs(co).T
    return (gamma(cv.shape[1]) + gamma(2 * co.shape[1])) * abs(scale) * (p + tr(p))


def project_bound(g, cv, co, alpha, ev=None, eo=None, kappa=None):
    t = np.abs(cv).T @ (np.abs(g) @ np.abs(co))
    if kappa is not None:
        t = t + (np.abs(ev)[:, None] + np.abs(eo)[None, :]) * np.abs(kappa)
    return 2.0 * gamma(cv.shape[0]) * abs(alpha) * t


def factor_bounds(x, c, w, dm_in, rp):
    north, r = c.shape
    x, c, sw = np.abs(x), np.abs(c), np.sqrt(w)
    labs = x @ (c * sw[None, :])
    ds = 0.5 * (np.abs(dm_in) + np.abs(dm_in).T)
    return {"factor": gamma(north) * labs, "dm": gamma(r) * ((c * w[None, :]) @ c.T),
            "dao": (2.0 * gamma(north) + gamma(rp)) * (labs @ labs.T), "dao_dm": 2.0 * gamma(north) * (x @ ds @ x.T)}


def finish_bounds(i, form, rp):
    with_k, vkind, kfrac, _, has_core, _ = FINISH_FORMS[form]
    nao, north = i["x"].shape
    x, wj, wk = np.abs(i["x"]), np.abs(i["wj"]), np.abs(i["wk"])
    ks = abs(kfrac) if kfrac is not None else 1.0
    jabs = wj + wj.T
    mabs = jabs + (0.5 * ks * (wk + wk.T) if with_k else 0.0)
    if vkind == "sym":
        mabs = mabs + np.abs(i["vsym"])
    if vkind == "raw":
        mabs = mabs + 0.5 * (np.abs(i["vraw"]) + np.abs(i["vraw"]).T)
    labs = x @ (np.abs(i["c"]) * i["sw"][None, :])
    dabs = labs @ labs.T
    g_d = 2.0 * gamma(north) + gamma(rp) + gamma(nao * nao)
    return {"fock": 2.0 * gamma(nao) * (x.T @ mabs @ x) + (gamma(0) * np.abs(i["core"]) if has_core else 0.0),
            "j": gamma(0) * jabs, "e_j": g_d * np.sum(dabs * wj), "e_k": g_d * 0.5 * ks * np.sum(dabs * wk)}
