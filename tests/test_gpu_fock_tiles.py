"""The tile kernels of dqc_amd/csrc/fock.hip -- the Fock ends (factor, orb2dm, the AO density, combine, finish) and the response ends
(resp_gemm, resp_dm) -- bit for bit against exact host arithmetic at ragged shapes, and within a derived bound on general inputs.

Part 1 (bitwise).  The inputs of tests/fock_tile_cases.py are small dyadic rationals inside a budget that makes every product and
every partial sum exact in fp64 in any order (tests/test_fock_tile_cases_cpu.py proves it case by case against int64), so the
kernels must return the float64 host result exactly: `torch.equal`, no tolerance.  The shapes are the edges of `ft_tile`: K = 1, a
partial k-quad (3, 5), one full trip (128), the first step of the second trip (129), a ragged second trip (131, 260), M / N = 1,
15, 16, 17, 33, north < nao, ldc > r, zero batch strides, both transa, sign = -1, nao^2 > 65536 (the second sweep of
fock_combine_kernel), every form of the finish in both modes, and nao = 1024, the library's maximum.

Part 2 (general inputs: normal deviates times 10^u, u uniform in [-3, 3] per element) catches what dyadics cannot, an operand
path narrower than fp64: |kernel - longdouble reference| <= 2 (K + 8) 2^-53 (|A| @ |B|) element by element for one product -- the
dot-product bound, valid for any summation order -- and its first-order composite for a chain (fock_tile_cases.*_bound).  The worst
ratio of error to bound is printed per case.

The tests are built to catch structural errors that change a value by however little: a k-step dropped or doubled at a tile
edge, a clamped element read without being zeroed, a mis-indexed second loop trip or second combine sweep, a store outside the
guarded range, a ticket left unreset."""
import numpy as np
import pytest
import torch

from tests import fock_tile_cases as ftc

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
JUNK = 3.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from dqc_amd import lib
    lib.load()
    yield torch.device("cuda")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _eq(got, want):
    """bitwise as values: every element of the device tensor equals the host array"""
    want = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float64))
    got = got.detach().cpu()
    return got.shape == want.shape and torch.equal(got, want)


TICKET_JUNK = 0x5A5A


def _dirty(work, npad):
    """every double of the work buffer non-zero, and the 32-bit ticket word of fock_combine_kernel too (the low word of 7.0 is 0)"""
    work.fill_(7.0)
    _ticket(work, npad)[0] = TICKET_JUNK


def _ticket(work, npad):
    n2 = npad * npad
    return work[3 * n2 + 1:3 * n2 + 2].view(torch.int32)


def _plus_zero(t):
    return bool((t.contiguous().view(torch.int64) == 0).all())


def _ratio(got, ref, bound):
    """worst |got - ref| / bound (ref longdouble, bound > 0 wherever anything is summed)"""
    err = np.abs(np.asarray(got.detach().cpu().numpy(), dtype=np.longdouble) - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    assert np.all(np.isfinite(err.astype(np.float64))) and np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def _ld_inputs(inp):
    return {k: ftc.ld(v) if isinstance(v, np.ndarray) else v for k, v in inp.items()}


# ---------------------------------------------------------------------------------------------------------------------
# a. dqc_resp_gemm, called directly
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_call(c, a, b, M, N, K, lda, ldb, ldc, sa, sb, sc, transa, nbatch, alpha, ea=None, eb=None, x=None):
    from dqc_amd import lib
    with lib._on(c.device) as st_:
        lib._check(lib.load().dqc_resp_gemm(lib._ptr(c), lib._ptr(a), lib._ptr(b), M, N, K, lda, ldb, ldc, sa, sb, sc, transa, nbatch,
                                            float(alpha), lib._ptr(ea), lib._ptr(eb), lib._ptr(x), st_), "dqc_resp_gemm")


def _slacked(a, slack, dev):
    """(nb, rows, cols) -> device buffer (nb, rows, cols + slack), the slack columns filled with junk"""
    buf = np.full(a.shape[:2] + (a.shape[2] + slack,), JUNK)
    buf[:, :, :a.shape[2]] = a
    return _t(buf, dev)


def _run_gemm(dev, spec, inp):
    """-> (the whole C buffer (nbatch, sc), sc, ldc): the kernel's writes and the sentinel everywhere else"""
    M, N, K, transa, nb, sl_a, sl_b, sl_c, sl_sc, a0, b0, epi, alpha = spec
    a, b = _slacked(inp["a"], sl_a, dev), _slacked(inp["b"], sl_b, dev)
    lda, ldb, ldc = a.shape[2], b.shape[2], N + sl_c
    sc = M * ldc + sl_sc
    c = torch.full((nb, sc), SENTINEL, dtype=torch.float64, device=dev)
    sa, sb = (0 if a0 else a.shape[1] * lda), (0 if b0 else K * ldb)
    ea, eb, x = (_t(inp[k], dev) for k in ("ea", "eb", "x")) if epi else (None, None, None)
    _gemm_call(c, a, b, M, N, K, lda, ldb, ldc, sa, sb, sc, transa, nb, alpha, ea, eb, x)
    torch.cuda.synchronize()
    return c, sc, ldc


def _c_body(c, M, N, ldc):
    return c[:, :M * ldc].view(c.shape[0], M, ldc)[:, :, :N]


@pytest.mark.parametrize("spec", ftc.GEMM_CASES, ids=lambda s: "M%d-N%d-K%d-t%d-b%d" % s[:5])
def test_resp_gemm_bitwise(dev, spec):
    M, N = spec[:2]
    inp, ref = ftc.gemm_case(spec)
    c, sc, ldc = _run_gemm(dev, spec, inp)
    want = np.full((spec[4], sc), SENTINEL)
    for v in range(spec[4]):
        want[v, :M * ldc].reshape(M, ldc)[:, :N] = ref[v]
    assert _eq(_c_body(c, M, N, ldc), ref), "the product"
    assert _eq(c, want), "the slack of C (row slack, batch slack) was written"


def test_resp_gemm_refuses_without_launching(dev):
    from dqc_amd import lib
    M, N, K = 5, 6, 7
    a = torch.ones((2, M, K), dtype=torch.float64, device=dev)
    b = torch.ones((2, K, N), dtype=torch.float64, device=dev)
    e = torch.ones(8, dtype=torch.float64, device=dev)
    c = torch.full((2, M * N), SENTINEL, dtype=torch.float64, device=dev)
    ok = dict(M=M, N=N, K=K, lda=K, ldb=N, ldc=N, sa=M * K, sb=K * N, sc=M * N, transa=0, nbatch=2, alpha=1.0)
    for change, extra in (({"K": 0}, {}), ({"lda": K - 1}, {}), ({"transa": 1, "lda": M - 1}, {}), ({}, {"x": c.clone(), "eb": e}),
                          ({"nbatch": 65536}, {}), ({"ldc": N - 1}, {}), ({"sc": M * N - 1}, {})):
        with pytest.raises(lib.DqcAmdError):
            _gemm_call(c, a, b, **dict(ok, **change), **extra)
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all())
    _gemm_call(c, a, b, **ok)  # (the unchanged arguments are accepted)
    assert bool((c == float(K)).all())


@pytest.mark.parametrize("spec", ftc.GENERAL_GEMM, ids=lambda s: "M%d-N%d-K%d-t%d-b%d" % s[:5])
def test_resp_gemm_general_inputs_within_the_dot_product_bound(dev, spec):
    inp = ftc.gemm_inputs(spec, general=True)
    c, sc, ldc = _run_gemm(dev, spec, inp)
    ref = ftc.gemm_chain(**_ld_inputs(inp))
    worst = _ratio(_c_body(c, spec[0], spec[1], ldc), ref, ftc.gemm_bound(**inp))
    print("resp_gemm %s: worst error / bound %.3g" % (spec[:5], worst))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# b. resp_project, resp_kappa2dm, resp_kappa2dm_pm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ftc.RESP_CASES, ids=lambda s: "nao%d-no%d-nv%d-nvec%d" % s)
def test_response_ends_bitwise(dev, shape):
    from dqc_amd import lib
    inp, ref = ftc.resp_case(shape)
    kappa, cv, co, g, ev, eo = (_t(inp[k], dev) for k in ("kappa", "cv", "co", "g", "ev", "eo"))
    plus = lib.resp_kappa2dm(kappa, cv, co, inp["scale"])
    assert _eq(plus, ref["plus"])
    p2, m2 = lib.resp_kappa2dm_pm(kappa, cv, co, inp["scale"])
    p1, none = lib.resp_kappa2dm_pm(kappa, cv, co, inp["scale"], minus=False)
    none2, m1 = lib.resp_kappa2dm_pm(kappa, cv, co, inp["scale"], plus=False)
    assert none is None and none2 is None
    assert torch.equal(p2, plus) and torch.equal(p1, plus), "dD+ of _pm is the one of resp_kappa2dm"
    assert _eq(m2, ref["minus"]) and torch.equal(m1, m2)
    assert torch.equal(plus, plus.transpose(1, 2)), "dD+ is bitwise symmetric"
    assert torch.equal(m2, -m2.transpose(1, 2)), "dD- is bitwise antisymmetric"
    assert bool((torch.diagonal(m2, dim1=1, dim2=2) == 0).all()), "the diagonal of dD- is exactly zero"
    assert _eq(lib.resp_project(g, cv, co, inp["alpha"]), ref["proj"])
    assert _eq(lib.resp_project(g, cv, co, inp["alpha"], ev, eo, kappa), ref["proj_diag"])


@pytest.mark.parametrize("shape", ftc.GENERAL_RESP, ids=lambda s: "nao%d-no%d-nv%d-nvec%d" % s)
def test_response_ends_general_inputs_within_the_composite_bound(dev, shape):
    from dqc_amd import lib
    inp = ftc.resp_inputs(shape, general=True)
    ref = ftc.resp_chains(_ld_inputs(inp))
    kappa, cv, co, g, ev, eo = (_t(inp[k], dev) for k in ("kappa", "cv", "co", "g", "ev", "eo"))
    plus, minus = lib.resp_kappa2dm_pm(kappa, cv, co, inp["scale"])
    bdm = ftc.kappa2dm_bound(inp["kappa"], inp["cv"], inp["co"], inp["scale"])
    args = (inp["g"], inp["cv"], inp["co"], inp["alpha"])
    worst = {"plus": _ratio(plus, ref["plus"], bdm), "minus": _ratio(minus, ref["minus"], bdm),
             "kappa2dm": _ratio(lib.resp_kappa2dm(kappa, cv, co, inp["scale"]), ref["plus"], bdm),
             "proj": _ratio(lib.resp_project(g, cv, co, inp["alpha"]), ref["proj"], ftc.project_bound(*args)),
             "proj_diag": _ratio(lib.resp_project(g, cv, co, inp["alpha"], ev, eo, kappa), ref["proj_diag"],
                                 ftc.project_bound(*args, inp["ev"], inp["eo"], inp["kappa"]))}
    print("response ends %s: worst error / bound %s" % (shape, {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# c. fock_factor, fock_orb2dm, fock_prep
# ---------------------------------------------------------------------------------------------------------------------
def _strided_c(c, dev):
    """c as a view with row stride r + 3 into a junk-filled buffer"""
    buf = torch.full((c.shape[0], c.shape[1] + 3), JUNK, dtype=torch.float64, device=dev)
    buf[:, :c.shape[1]] = _t(c, dev)
    return buf[:, :c.shape[1]]


def _check_factor(pair, lfac, nao, r):
    orb, orbt = pair
    assert _eq(orb[:nao, :r], lfac), "the factor"
    assert _plus_zero(orb[nao:, :]) and _plus_zero(orb[:, r:]), "the padding of the factor is +0.0"
    assert torch.equal(orbt, orb.t()), "orbt is the transpose"


def _prep_and_check(lib, work, x, nao, npad, want, **src):
    n2 = npad * npad
    for with_k in (False, True):
        _dirty(work, npad)
        assert int(_ticket(work, npad)[0]) == TICKET_JUNK
        lib.fock_prep(work, x, nao, with_k, **src)
        d = work[:n2].view(npad, npad)
        assert _eq(d[:nao, :nao], want), "the AO density"
        assert _plus_zero(d[nao:, :]) and _plus_zero(d[:, nao:]), "the padding of the AO density is +0.0"
        assert _plus_zero(work[n2:(3 if with_k else 2) * n2]), "the accumulators are zeroed"
        assert int(_ticket(work, npad)[0]) == 0, "the ticket word is reset"


@pytest.mark.parametrize("shape", ftc.FACTOR_CASES + [ftc.FACTOR_MAX], ids=lambda s: "nao%d-north%d-r%d" % s)
def test_factor_orb2dm_and_prep_bitwise(dev, shape):
    from dqc_amd import lib
    nao, north, r = shape
    inp, ref = ftc.factor_case(shape)
    x, w, c = _t(inp["x"], dev), _t(ref["w"], dev), _strided_c(inp["c"], dev)
    assert c.stride(0) > r
    ld, npad = lib.padded_nao(nao), (nao + 7) // 8 * 8
    _check_factor(lib.fock_factor(x, c, w, nao, ld), ref["factor"], nao, r)
    dm, pair = lib.fock_orb2dm(x, c, w, nao, ld)
    _check_factor(pair, ref["factor"], nao, r)
    assert _eq(dm, ref["dm"]), "D = C diag(w) C^T"
    work = lib.jk_workspace(nao, dev)
    assert work.numel() >= 5 * npad * npad + 8 + 128
    _prep_and_check(lib, work, x, nao, npad, ref["dao"], orb=pair[0])
    _prep_and_check(lib, work, x, nao, npad, ref["dao_dm"], dm=_t(inp["dm_in"], dev))  # asymmetric: the (D + D^T) / 2 of fock_xd_kernel


def test_fock_ends_refuse_more_than_1024_aos(dev):
    from dqc_amd import lib
    assert lib.fock_max_nao() == 1024
    nao = 1025
    x = torch.ones((nao, nao), dtype=torch.float64, device=dev)
    c = torch.ones((nao, 4), dtype=torch.float64, device=dev)
    w = torch.ones(4, dtype=torch.float64, device=dev)
    work = lib.jk_workspace(nao, dev)
    with pytest.raises(lib.DqcAmdError):
        lib.fock_factor(x, c, w, nao, lib.padded_nao(nao))
    with pytest.raises(lib.DqcAmdError):
        lib.fock_orb2dm(x, c, w, nao, lib.padded_nao(nao))
    with pytest.raises(lib.DqcAmdError):
        lib.fock_prep(work, x, nao, True, dm=x)
    with pytest.raises(lib.DqcAmdError):
        lib.fock_finish(work, x, nao, True)


@pytest.mark.parametrize("shape", ftc.GENERAL_FACTOR, ids=lambda s: "nao%d-north%d-r%d" % s)
def test_factor_orb2dm_and_prep_general_inputs_within_the_composite_bound(dev, shape):
    from dqc_amd import lib
    nao, north, r = shape
    inp = ftc.factor_inputs(shape, general=True)
    ref = ftc.factor_chain(ftc.ld(inp["x"]), ftc.ld(inp["c"]), np.sqrt(ftc.ld(inp["w"])), ftc.ld(inp["dm_in"]))
    x, w, c = _t(inp["x"], dev), _t(inp["w"], dev), _strided_c(inp["c"], dev)
    ld, npad = lib.padded_nao(nao), (nao + 7) // 8 * 8
    dm, (orb, orbt) = lib.fock_orb2dm(x, c, w, nao, ld)
    bounds = ftc.factor_bounds(inp["x"], inp["c"], inp["w"], inp["dm_in"], orb.shape[1])
    worst = {"factor": _ratio(orb[:nao, :r], ref["factor"], bounds["factor"]), "dm": _ratio(dm, ref["dm"], bounds["dm"]),
             "factor alone": _ratio(lib.fock_factor(x, c, w, nao, ld)[0][:nao, :r], ref["factor"], bounds["factor"])}
    work = lib.jk_workspace(nao, dev)
    lib.fock_prep(work, x, nao, True, orb=orb)
    worst["dao"] = _ratio(work[:npad * npad].view(npad, npad)[:nao, :nao], ref["dao"], bounds["dao"])
    lib.fock_prep(work, x, nao, True, dm=_t(inp["dm_in"], dev))
    worst["dao_dm"] = _ratio(work[:npad * npad].view(npad, npad)[:nao, :nao], ref["dao_dm"], bounds["dao_dm"])
    print("factor / density %s: worst error / bound %s" % (shape, {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# d. fock_finish, stand-alone: fock_prep, synthetic J / K accumulators written into the work buffer, fock_finish
# ---------------------------------------------------------------------------------------------------------------------
def _put(work, lo, npad, nao, values, det_scale):
    """values (nao, nao) into the npad-strided square at work[lo:], junk in its padding; deterministic mode: int64 bit patterns in
    units of 1 / det_scale"""
    if det_scale:
        reg = work.view(torch.int64)[lo:lo + npad * npad].view(npad, npad)
        reg.fill_(12345)
        reg[:nao, :nao] = torch.from_numpy(np.round(values * det_scale).astype(np.int64)).to(work.device)
    else:
        reg = work[lo:lo + npad * npad].view(npad, npad)
        reg.fill_(JUNK)
        reg[:nao, :nao] = _t(values, work.device)


def _finish(lib, dev, work, x, shape, inp, form, det):
    nao, north = shape
    with_k, vkind, kfrac, has_exc, has_core, want_j = ftc.FINISH_FORMS[form]
    npad, n2 = (nao + 7) // 8 * 8, ((nao + 7) // 8 * 8) ** 2
    _put(work, n2, npad, nao, inp["wj"], ftc.DET_SCALE if det else 0)
    _put(work, 2 * n2, npad, nao, inp["wk"], ftc.DET_SCALE if det else 0)  # (junk for the forms without K: never read)
    work[3 * n2] = ftc.DET_SCALE if det else float("nan")  # slot 0 of the eight-slot area: read in deterministic mode only
    v, vscale = None, None
    if vkind == "sym":  # a plain symmetric matrix in both modes, row stride nao + 5
        v = torch.full((nao, nao + 5), JUNK, dtype=torch.float64, device=dev)
        v[:, :nao] = _t(inp["vsym"], dev)
    if vkind == "raw":  # the layout of grid_vxc_raw: (ld, ld), fixed-point integers in deterministic mode
        ldv = lib.padded_nao(nao)
        v = torch.empty(ldv * ldv, dtype=torch.float64, device=dev)
        _put(v, 0, ldv, nao, inp["vraw"], ftc.DET_VSCALE if det else 0)
        v, vscale = v.view(ldv, ldv), (ftc.DET_VSCALE if det else 0.0)
    exc = torch.tensor([inp["exc"]], dtype=torch.float64, device=dev) if has_exc else None
    core = _t(inp["core"], dev) if has_core else None
    out = lib.fock_finish(work, x, nao, with_k, vxc_ao=v, core=core, want_j=want_j, vscale=vscale, kfrac=kfrac, exc=exc)
    torch.cuda.synchronize()
    return out


def _prepared(lib, dev, shape, inp):
    nao, north = shape
    x, c = _t(inp["x"], dev), _strided_c(inp["c"], dev)
    orb, _ = lib.fock_factor(x, c, _t(inp["sw"] * inp["sw"], dev), nao, lib.padded_nao(nao))
    work = lib.jk_workspace(nao, dev)
    _dirty(work, (nao + 7) // 8 * 8)  # (fock_prep has to reset the ticket for the finish to hand out its energies)
    lib.fock_prep(work, x, nao, True, orb=orb)
    return work, x


@pytest.mark.parametrize("form", list(ftc.FINISH_FORMS))
@pytest.mark.parametrize("shape", ftc.FINISH_SHAPES, ids=lambda s: "nao%d-north%d" % s)
def test_fock_finish_bitwise_in_both_modes(dev, shape, form):
    from dqc_amd import lib
    nao, north = shape
    with_k, vkind, kfrac, has_exc, has_core, want_j = ftc.FINISH_FORMS[form]
    inp, dao, refs = ftc.finish_case(shape)
    ref = refs[form]
    work, x = _prepared(lib, dev, shape, inp)
    npad = (nao + 7) // 8 * 8
    assert _eq(work[:npad * npad].view(npad, npad)[:nao, :nao], dao)
    prev = lib.set_deterministic(False)
    try:
        results = []
        for det in (False, True):
            lib.set_deterministic(det)
            fock, en, jao = _finish(lib, dev, work, x, shape, inp, form, det)
            mode = "deterministic" if det else "plain"
            assert _eq(fock, ref["fock"]), "F, %s mode" % mode
            f0 = fock.cpu() - (torch.from_numpy(inp["core"]) if has_core else 0.0)
            assert torch.equal(f0, f0.t()) and _eq(f0, ref["f0"]), "F - core is bitwise symmetric, %s mode" % mode
            assert (jao is not None) == want_j and (jao is None or _eq(jao, ref["j"])), "J_ao, %s mode" % mode
            e = en.cpu().numpy()
            assert e.shape == ((3,) if kfrac is not None else (2,))
            assert e[0] == ref["e_j"] and e[1] == (ref["e_k"] if with_k else 0.0), "the energy traces, %s mode" % mode
            if kfrac is not None:
                assert e[2] == (inp["exc"] if has_exc else 0.0), "E_xc handed through, %s mode" % mode
            assert int(_ticket(work, npad)[0]) == 0, "the ticket is back at zero"
            results.append((fock, en))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    finally:
        lib.set_deterministic(prev)


def test_fock_finish_refuses_a_scale_that_does_not_match_the_mode(dev):
    from dqc_amd import lib
    shape = ftc.FINISH_SHAPES[0]
    inp, _, _ = ftc.finish_case(shape)
    work, x = _prepared(lib, dev, shape, inp)
    ldv, npad = lib.padded_nao(shape[0]), (shape[0] + 7) // 8 * 8
    v = torch.zeros((ldv, ldv), dtype=torch.float64, device=dev)
    prev = lib.set_deterministic(False)
    try:
        for det, bad in ((False, ftc.DET_VSCALE), (True, 0.0)):
            lib.set_deterministic(det)
            work[3 * npad * npad] = ftc.DET_SCALE
            with pytest.raises(lib.DqcAmdError):
                lib.fock_finish(work, x, shape[0], False, vxc_ao=v, vscale=bad)
            with pytest.raises(lib.DqcAmdError):
                lib.fock_finish(work, x, shape[0], True, vxc_ao=v, vscale=bad, kfrac=0.25)
    finally:
        lib.set_deterministic(prev)


@pytest.mark.parametrize("form", ftc.GENERAL_FORMS)
@pytest.mark.parametrize("shape", ftc.GENERAL_FINISH, ids=lambda s: "nao%d-north%d" % s)
def test_fock_finish_general_inputs_within_the_composite_bound(dev, shape, form):
    from dqc_amd import lib
    nao, north = shape
    with_k, vkind, kfrac, has_exc, has_core, want_j = ftc.FINISH_FORMS[form]
    inp = ftc.finish_inputs(shape, general=True)
    li = _ld_inputs(inp)
    ref = ftc.finish_form_chain(li, ftc.finish_density(li), form)
    prev = lib.set_deterministic(False)
    try:
        work, x = _prepared(lib, dev, shape, inp)
        rp = lib.padded_norb(ftc.FINISH_R)
        fock, en, jao = _finish(lib, dev, work, x, shape, inp, form, False)
    finally:
        lib.set_deterministic(prev)
    b = ftc.finish_bounds(inp, form, rp)
    worst = {"fock": _ratio(fock, ref["fock"], b["fock"]), "e_j": _ratio(en[0], ref["e_j"], b["e_j"]),
             "e_k": _ratio(en[1], ref["e_k"], b["e_k"])}
    if want_j:
        worst["j"] = _ratio(jao, ref["j"], b["j"])
    print("fock_finish %s %s: worst error / bound %s" % (shape, form, {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0


def test_longdouble_reference_is_wide_enough():
    assert np.finfo(np.longdouble).eps < 2e-19
