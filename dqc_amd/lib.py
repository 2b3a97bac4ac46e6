"""ctypes binding of libdqc_amd.so (C ABI declared in include/dqc_amd.h).

The product path has no CPU fallback: if the HIP library cannot be loaded this module raises.
PyTorch is used only for device memory and streams (tensor.data_ptr(), current stream handle).
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("DQC_AMD_LIB") or os.path.join(_HERE, "libdqc_amd.so")  # override: perf-bisection variants
_lib = None

XC_IDS = {"lda_x": 1, "lda_c_vwn": 7, "lda_c_pw": 12, "lda_c_pw_mod": 13, "gga_x_pbe": 101, "gga_x_pbe_r": 102, "gga_x_b88": 106,
          "gga_x_pbe_sol": 116, "gga_x_rpbe": 117, "gga_c_pbe": 130, "gga_c_lyp": 131, "gga_c_pbe_sol": 133,
          "mgga_x_scan": 263, "mgga_c_scan": 267, "mgga_x_tpss": 202, "mgga_c_tpss": 231,
          "lda_c_pz": 9, "gga_x_b86": 103, "gga_x_g96": 107, "gga_x_pw86": 108, "gga_x_pw91": 109, "gga_x_optx": 110, "gga_x_wc": 118,
          "gga_c_p86": 132}


class DqcAmdError(RuntimeError):
    pass


def libpath():
    return _LIBPATH


def load():
    """Load libdqc_amd.so; raises (loudly) when it is missing -- there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIBPATH) and os.environ.get("DQC_AMD_AUTOBUILD", "0") == "1" and "DQC_AMD_LIB" not in os.environ:
        from . import build as _build  # fresh clone: compile the HIP sources in-tree (hipcc, ~1 min)
        _build.build()
    if not os.path.exists(_LIBPATH):
        raise DqcAmdError(
            "libdqc_amd.so not found at %s -- build it with `python -m dqc_amd.build` "
            "(hipcc --offload-arch=gfx950) or set DQC_AMD_AUTOBUILD=1; the MI355X path has no CPU fallback" % _LIBPATH)
    lib = ctypes.CDLL(_LIBPATH)
    c_int, c_sz, c_vp, c_dp = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    lib.dqc_last_error.restype = ctypes.c_char_p
    lib.dqc_version.restype = c_int
    lib.dqc_nao.argtypes = [ip, c_int]
    lib.dqc_padded_nao.argtypes = [c_int]
    lib.dqc_ao_stride.argtypes = [c_int]
    lib.dqc_ao_doubles.argtypes = [c_int, c_int, c_int]
    lib.dqc_ao_doubles.restype = c_sz
    lib.dqc_eri_tile_count.argtypes = [c_int]
    lib.dqc_eri_tile_count.restype = c_sz
    if hasattr(lib, "dqc_eri_store_doubles"):  # (absent from the pre-packing A/B build tools/gpu_jk_ab.py loads)
        lib.dqc_eri_store_doubles.argtypes = [c_int]
        lib.dqc_eri_store_doubles.restype = c_sz
    lib.dqc_eri_tile_offset.argtypes = [c_int, ctypes.c_longlong]
    lib.dqc_eri_tile_offset.restype = ctypes.c_longlong
    lib.dqc_eri_fill_tiles_part.argtypes = [c_dp, ip, c_int, ip, c_int, dp, c_int, ctypes.c_longlong, ctypes.c_longlong, c_vp]
    lib.dqc_jk_from_tiles_part.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_dp, ctypes.c_longlong, ctypes.c_longlong, c_vp]
    lib.dqc_jk_work_doubles.argtypes = [c_int]
    lib.dqc_jk_work_doubles.restype = c_sz
    tab = [ip, c_int, ip, c_int, dp, c_int]
    lib.dqc_int1e.argtypes = [c_int, c_dp] + tab + [dp, c_vp]
    lib.dqc_eri_fill_tiles.argtypes = [c_dp] + tab + [c_vp]
    lib.dqc_jk_direct.argtypes = [c_dp, c_dp, c_dp] + tab + [c_vp]
    lib.dqc_direct_create.argtypes = [ctypes.POINTER(c_vp)] + tab + [c_vp]
    lib.dqc_direct_jk.argtypes = [c_vp, c_dp, c_dp, c_dp, ctypes.c_double, c_vp]
    lib.dqc_direct_jk_part.argtypes = [c_vp, c_dp, c_dp, c_dp, ctypes.c_double, c_int, c_int, c_vp]
    lib.dqc_direct_stats.argtypes = [c_vp, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong), dp]
    lib.dqc_direct_npairs.argtypes = [c_vp]
    lib.dqc_eri_pair_stats.argtypes = [ip, c_int, ip, c_int, dp, c_int, c_int, ctypes.POINTER(ctypes.c_longlong)]
    lib.dqc_direct_bounds.argtypes = [c_vp, dp, ip]
    lib.dqc_direct_bounds_groups.argtypes = [c_vp, dp, ip, ip]
    lib.dqc_direct_destroy.argtypes = [c_vp]
    lib.dqc_int3c2e.argtypes = [c_dp] + tab + [c_int, c_int, c_int, c_int, c_vp]
    lib.dqc_int2c2e.argtypes = [c_dp] + tab + [c_int, c_int, c_vp]
    lib.dqc_ncart.argtypes = [ip, c_int]
    lib.dqc_cart2sph_matrix.argtypes = [dp, ip, c_int]
    lib.dqc_int1e_grad.argtypes = [c_dp, c_dp, c_dp] + tab + [dp, c_vp]
    lib.dqc_eri_grad.argtypes = [c_dp, c_dp, ctypes.c_double, ctypes.c_double] + tab + [c_vp]
    lib.dqc_eri_grad2.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double] + tab + [c_vp]
    lib.dqc_int1e_grad_basis.argtypes = [c_dp, c_dp, c_dp] + tab + [dp, c_vp]
    lib.dqc_eri_grad_basis.argtypes = [c_dp, c_dp, ctypes.c_double, ctypes.c_double] + tab + [c_vp]
    lib.dqc_int1e_potential.argtypes = [c_dp, c_dp, c_dp, c_int] + tab + [c_vp]
    lib.dqc_df_grad.argtypes = [c_dp, c_dp, c_dp] + tab + [c_int, c_int, c_int, c_int, c_vp]
    lib.dqc_df_grad3.argtypes = [c_dp, c_dp, c_sz, c_dp] + tab + [c_int, c_int, c_int, c_int, c_vp]
    lib.dqc_becke_weights.argtypes = [c_dp, c_dp, c_vp, c_dp, c_dp, c_dp, c_int, c_int, ctypes.c_double, c_vp]
    lib.dqc_becke_weights_grad.argtypes = [c_dp, c_dp, c_dp, c_dp, c_dp, c_vp, c_dp, c_dp, c_dp, c_int, c_int, ctypes.c_double, c_vp]
    lib.dqc_purify_tc2.argtypes = [c_dp, c_dp, c_int, ctypes.c_double, c_int, ctypes.c_double, c_dp, c_vp]
    lib.dqc_orth_factor.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_vp]
    lib.dqc_purify_tc2_batched.argtypes = [c_dp, c_dp, c_int, c_int, ctypes.c_double, c_int, ctypes.c_double, c_dp, c_vp]
    lib.dqc_orth_factor_batched.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_int, c_vp]
    lib.dqc_diis_solve.argtypes = [c_dp, c_dp, c_int, c_int, c_int, c_vp]
    lib.dqc_diis_solve_dev.argtypes = [c_dp, c_dp, c_int, c_int, c_vp, c_vp]
    lib.dqc_projector_work_doubles.argtypes = [c_int, c_int]
    lib.dqc_projector_work_doubles.restype = c_sz
    lib.dqc_projector_tc2.argtypes = [c_dp, c_dp, c_dp, c_int, ctypes.c_double, c_int, ctypes.c_double, c_dp, c_vp]
    lib.dqc_purify_tc2_persist.argtypes = [c_dp, c_dp, c_int, ctypes.c_double, c_int, ctypes.c_double, c_dp, c_vp, c_vp]
    lib.dqc_df_coulomb.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_int, c_dp, c_vp]
    lib.dqc_df_exchange.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_int, c_int, c_dp, c_vp]
    lib.dqc_df_exchange_work_doubles.argtypes = [c_int, c_int, c_int]
    lib.dqc_df_exchange_work_doubles.restype = c_sz
    lib.dqc_mp2_work_doubles.argtypes = [c_int] * 5
    lib.dqc_mp2_work_doubles.restype = c_sz
    lib.dqc_mp2_pair_energies.argtypes = [c_dp] * 8 + [c_int] * 8 + [c_dp, c_vp]
    lib.dqc_mp2_amplitudes.argtypes = [c_dp, c_dp, c_sz, c_dp, c_dp, c_dp] + [c_int] * 6 + [ctypes.c_double, ctypes.c_double, c_vp]
    lib.dqc_rpa_work_doubles.argtypes = [c_int] * 4
    lib.dqc_rpa_work_doubles.restype = c_sz
    lib.dqc_rpa_response.argtypes = [c_dp] * 5 + [c_int] * 5 + [ctypes.c_double, c_int, c_dp, c_vp]
    lib.dqc_gw_screened_diag.argtypes = [c_dp] * 3 + [c_int] * 5 + [c_vp]
    lib.dqc_bse_work_doubles.argtypes = [c_int] * 6
    lib.dqc_bse_work_doubles.restype = c_sz
    lib.dqc_bse_exchange.argtypes = [c_dp] * 4 + [c_int] * 8 + [c_dp, c_vp]
    lib.dqc_cc_ladder_work_doubles.argtypes = [c_int] * 6
    lib.dqc_cc_ladder_work_doubles.restype = c_sz
    lib.dqc_cc_ladder.argtypes = [c_dp] * 4 + [c_int] * 8 + [c_dp, c_vp]
    lib.dqc_eri_tiles_to_dense.argtypes = [c_dp, c_dp, c_int, c_vp]
    lib.dqc_jk_from_tiles.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_dp, c_vp]
    lib.dqc_jk_multi_work_doubles.argtypes = [c_int, c_int, c_int]
    lib.dqc_jk_multi_work_doubles.restype = c_sz
    lib.dqc_jk_from_tiles_multi.argtypes = [c_dp, c_dp, c_int, c_dp, c_dp, c_int, c_dp, c_int, c_dp, c_vp]
    lib.dqc_jk_from_tiles_multi_asym.argtypes = [c_dp, c_dp, c_int, c_dp, c_dp, c_int, ctypes.POINTER(c_int), c_dp, c_int, c_dp, c_vp]
    lib.dqc_eval_gto.argtypes = [c_int, c_dp, c_dp, c_int] + tab + [c_vp]
    lib.dqc_grid_density.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_int, c_dp, c_vp]
    lib.dqc_xc_eval.argtypes = [c_dp, c_dp, c_dp, c_dp, c_dp, c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_quad.argtypes = [c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_pol.argtypes = [c_dp] * 9 + [c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_fxc.argtypes = [c_dp] * 6 + [c_int, c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_kxc.argtypes = [c_dp] * 8 + [c_int, c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_fxc_pol.argtypes = [c_dp] * 12 + [c_int, c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_fxc_triplet.argtypes = [c_dp] * 6 + [c_int, c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_mgga.argtypes = [c_dp] * 7 + [c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_mgga_pol.argtypes = [c_dp] * 11 + [c_int, ip, dp, c_int, c_vp]
    lib.dqc_xc_eval_mgga_pol2.argtypes = [c_dp] * 12 + [c_int, ip, dp, c_int, c_vp]
    lib.dqc_stream_create_partition.argtypes = [ctypes.POINTER(c_vp), c_int, c_int, c_int]
    lib.dqc_stream_destroy.argtypes = [c_vp]
    lib.dqc_stream_cus.argtypes = [c_vp]
    lib.dqc_set_vxc_cus.argtypes = [c_int]
    lib.dqc_fock_factor.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_dp, c_int, c_int, c_int, c_int, c_int, c_vp]
    lib.dqc_fock_orb2dm.argtypes = [c_dp, c_dp, c_dp, c_dp, c_dp, c_int, c_dp, c_int, c_int, c_int, c_int, c_int, c_vp]
    lib.dqc_grid_vxc_raw.argtypes = [c_dp, c_dp, c_int, c_int, c_int, c_dp, c_dp, c_dp, dp, c_vp]
    lib.dqc_fock_finish_vraw.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, ctypes.c_double, c_dp, c_dp, c_int, c_int, c_vp]
    lib.dqc_fock_prep.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_int, c_int, c_int, c_vp]
    lib.dqc_jk_stream_prepared.argtypes = [c_dp, c_int, c_dp, c_int, c_vp]
    lib.dqc_fock_finish.argtypes = [c_dp, c_dp, c_dp, c_dp, c_dp, c_int, c_dp, c_dp, c_int, c_int, c_int, c_vp]
    lib.dqc_fock_finish_hybrid.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_int, ctypes.c_double, ctypes.c_double, c_dp, c_dp, c_dp, c_int,
                                           c_int, c_vp]
    ll = ctypes.c_longlong
    lib.dqc_resp_gemm.argtypes = [c_dp, c_dp, c_dp] + [c_int] * 6 + [ll, ll, ll, c_int, c_int, ctypes.c_double, c_dp, c_dp, c_dp, c_vp]
    lib.dqc_resp_kappa2dm.argtypes = [c_dp] * 5 + [c_int] * 4 + [ctypes.c_double, c_vp]
    lib.dqc_resp_kappa2dm_pm.argtypes = [c_dp] * 6 + [c_int] * 4 + [ctypes.c_double, c_vp]
    lib.dqc_padded_norb.argtypes = [c_int]
    lib.dqc_padded_norb.restype = c_int
    lib.dqc_grid_density_lr.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_int, c_dp, c_dp, c_int, c_vp]
    lib.dqc_grid_density_lr_pol.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_int, c_dp, c_dp, c_int, c_vp]
    lib.dqc_grid_xc_gradient_terms.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_dp, c_dp, c_dp, c_dp, c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_vp]
    lib.dqc_grid_density_lr_tau.argtypes = [c_dp, c_dp, c_dp, c_dp, c_int, c_int, c_int, c_dp, c_int, c_vp]
    lib.dqc_grid_density_pair.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_dp, c_vp]
    lib.dqc_grid_vxc_pair.argtypes = [c_dp, c_dp, c_dp, c_int, c_int, c_dp, c_dp, c_vp]
    lib.dqc_grid_vxc.argtypes = [c_dp, c_dp, c_int, c_int, c_int, c_dp, c_dp, c_dp, c_vp]
    lib.dqc_probe_stream_read.argtypes = [c_dp, c_sz, c_dp, c_vp]
    lib.dqc_probe_mfma_f64.argtypes = [c_dp, c_int, c_vp]
    lib.dqc_probe_rys.argtypes = [c_int, c_int, c_dp, c_int, c_dp, c_dp, c_vp]
    _lib = lib
    if os.environ.get("DQC_AMD_DETERMINISTIC", "0") == "1":
        lib.dqc_set_deterministic(1)
    return lib


def set_generic_eri(on=True):
    """every shell-quartet class through the runtime-angular-momentum integral kernel (include/dqc_amd.h:
    dqc_set_generic_eri) -- normally only the classes with a g shell take it.  Returns the previous setting."""
    return bool(load().dqc_set_generic_eri(1 if on else 0))


def set_deterministic(on=True):
    """bit-reproducible Fock builds: the cross-block sums (J / K accumulators, split-K Vxc, purification trace) use fixed-point
    integer atomics instead of fp64 atomics (include/dqc_amd.h: dqc_set_deterministic).  Returns the previous setting.
    Environment: DQC_AMD_DETERMINISTIC=1.

    Fixed point is exact in any order but only as fine as its scale, and each of the three users sets the scale its own way
    (tests/test_gpu_deterministic_kernels.py pins each against a host reference across input magnitudes):
      J / K from tiles   per call, 2^k with 2 gmax max_q sum|D_q| 2^k < 2^61: any magnitude of D.  ONE scale for all densities of a
                         jk_multi pass: every slot is exact to the largest slot's resolution (see jk_multi).
      Vxc                `grid_vxc`, `grid_vxc_pair`: the potential is divided by a power of two c taken on the device from the
                         call's own arrays -- 2^14 c >= B = sum_g A_g^2 |w_g| (|v_g| + 2 sum_d |vgrad_dg|) >= every partial sum, A_g
                         the largest |AO value| at the point (one pass over an AO array, remembered with it) -- summed on the constant
                         scale 2^47, and the result multiplied by c: any magnitude, no state shared between calls or streams.
                         `grid_vxc_raw` (the fused Fock build's form) and the C entry points sum on 2^47 as they are: right
                         for sums of order one (v_xc on normalised AOs); each addition rounds to 2^-47 ABSOLUTE and a sum beyond
                         2^16 wraps.
      purification       traces on the constant 2^46: spectra mapped to [0, 1], traces below 2^15 -- always the case."""
    return bool(load().dqc_set_deterministic(1 if on else 0))


_TRACE = None      # a list while `call_trace` is active: (entry point, start event, end event) per library call
_TRACE_OPEN = None


class call_trace:
    """measurement aid: `with lib.call_trace() as tr:` brackets every library call made inside with two HIP events on the stream
    the call is enqueued on; `tr.ms()` -> {entry point: (calls, mean ms per call)} (synchronises).  bench.py's per-kernel
    rooflines of the legs that have no hand-unrolled event chain come from here; nothing is recorded outside the block."""

    def __enter__(self):
        global _TRACE
        self.rows = _TRACE = []
        return self

    def __exit__(self, *a):
        global _TRACE, _TRACE_OPEN
        _TRACE = _TRACE_OPEN = None
        return False

    def ms(self):
        torch.cuda.synchronize()
        out = {}
        for what, e0, e1 in self.rows:
            n, t = out.get(what, (0, 0.0))
            out[what] = (n + 1, t + e0.elapsed_time(e1))
        return {k: (n, t / n) for k, (n, t) in out.items()}


def _check(rc, what):
    global _TRACE_OPEN
    if _TRACE is not None and _TRACE_OPEN is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(torch.cuda.current_stream(_TRACE_OPEN[1]))
        _TRACE.append((what, _TRACE_OPEN[0], e1))
        _TRACE_OPEN = None
    if rc != 0:
        raise DqcAmdError("%s failed (%d): %s" % (what, rc, load().dqc_last_error().decode()))


class _on:
    """Run a C entry point on the device that owns the tensors: the library launches on (and hipMallocs from) the CURRENT
    HIP device and on the stream it is handed, so both are taken from `dev`, not from whatever device happens to be
    current (Mol(..., device="cuda:1") while cuda:0 is current)."""

    def __init__(self, dev):
        dev = torch.device(dev)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self.idx = idx
        self.guard = None if idx == torch.cuda.current_device() else torch.cuda.device(idx)

    def __enter__(self):
        global _TRACE_OPEN
        if self.guard is not None:
            self.guard.__enter__()
        st = torch.cuda.current_stream(self.idx)
        if _TRACE is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _TRACE_OPEN = (e0, self.idx)
        return ctypes.c_void_p(st.cuda_stream)

    def __exit__(self, *a):
        if self.guard is not None:
            self.guard.__exit__(*a)
        return False


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous(), "need contiguous float64 device tensor"
    return ctypes.c_void_p(t.data_ptr())


class Tables:
    """Host-side libcint-style tables (atm, bas, env) -- see dqc_amd.basis.make_tables."""

    def __init__(self, atm, bas, env):
        self.atm = np.ascontiguousarray(atm, dtype=np.int32)
        self.bas = np.ascontiguousarray(bas, dtype=np.int32)
        self.env = np.ascontiguousarray(env, dtype=np.float64)
        self.natm, self.nbas = self.atm.shape[0], self.bas.shape[0]
        self.nao = int(sum(2 * int(b[1]) + 1 for b in self.bas))

    def args(self):
        ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        return (self.atm.ctypes.data_as(ip), self.natm, self.bas.ctypes.data_as(ip), self.nbas,
                self.env.ctypes.data_as(dp), self.env.shape[0])


def padded_nao(nao):
    """rows / columns of the zero-padded AO-indexed square matrices (D, V, the factor pair): whole 16 x 16 tiles"""
    return int(load().dqc_padded_nao(int(nao)))


def ao_stride(nao):
    """row stride of the AO-on-grid arrays (nao rounded up to 8 doubles: 64-byte rows, no tile padding in HBM)"""
    return int(load().dqc_ao_stride(int(nao)))


def ao_empty(ncomp, ngrid, nao, device, zero=False):
    """an AO-on-grid array for the grid kernels: (ngrid, lda) for ncomp = 0, else (ncomp, ngrid, lda), a view of a flat buffer
    of dqc_ao_doubles doubles -- the kernels read whole 16-column tiles, up to ld - lda doubles past the end of the last row
    (that slack is zeroed here)"""
    nc = max(int(ncomp), 1)
    lda = ao_stride(nao)
    tot = int(load().dqc_ao_doubles(nc, int(ngrid), int(nao)))
    flat = (torch.zeros if zero else torch.empty)(tot, dtype=torch.float64, device=device)
    body = nc * int(ngrid) * lda
    if not zero and tot > body:
        flat[body:].zero_()
    out = flat[:body].view(nc, int(ngrid), lda)
    return out[0] if ncomp == 0 else out


def ao_from(values, nao=None):
    """values (ngrid, n) or (ncomp, ngrid, n) with n >= nao (any device tensor / view, e.g. the sum of two AO arrays) -> a
    fresh array in the kernels' layout (row stride lda, zero padding columns, zeroed slack) holding values[..., :nao]"""
    nao = values.shape[-1] if nao is None else nao
    out = ao_empty(0 if values.dim() == 2 else values.shape[0], values.shape[-2], nao, values.device, zero=True)
    out[..., :nao] = values[..., :nao]
    return out


def int1e(which, tab, device, zs=None):
    """which: 'ovlp' | 'kin' | 'nuc' -> (nao, nao) device tensor; 'r0' -> (3, nao, nao), 'r0r0' -> (9, nao, nao): multipole
    moments about the origin (the reference's intor.int1e("r0" * n), hcgto.py:117-125)"""
    if which in ("r0", "r0r0"):
        return torch.stack([int1e(c, tab, device) for c in (range(3, 6) if which == "r0" else range(6, 15))])
    code = which if isinstance(which, int) else {"ovlp": 0, "kin": 1, "nuc": 2}[which]
    out = torch.zeros((tab.nao, tab.nao), dtype=torch.float64, device=device)
    zp = None
    if zs is not None:
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        zp = zs.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with _on(device) as st_:
        _check(load().dqc_int1e(code, _ptr(out), *tab.args(), zp, st_), "dqc_int1e")
    return out


def eri_store_doubles(nao):
    """doubles of the packed ERI tile store of `nao` functions"""
    return int(load().dqc_eri_store_doubles(int(nao)))


def eri_tiles(tab, device):
    tiles = torch.empty(eri_store_doubles(tab.nao), dtype=torch.float64, device=device)  # packed tiles
    with _on(device) as st_:
        _check(load().dqc_eri_fill_tiles(_ptr(tiles), *tab.args(), st_), "dqc_eri_fill_tiles")
    return tiles


def _range_nao(tab, s0, s1):
    return int(sum(2 * int(b[1]) + 1 for b in tab.bas[s0:s1]))


def int3c2e(tab, orb_range, aux_range, device):
    """(ij|k) over concatenated tables: orbital shells [s0, s1), auxiliary shells [k0, k1) -> (nao, nao, naux)"""
    (s0, s1), (k0, k1) = orb_range, aux_range
    nao, naux = _range_nao(tab, s0, s1), _range_nao(tab, k0, k1)
    out = torch.zeros((nao, nao, naux), dtype=torch.float64, device=device)
    with _on(device) as st_:
        _check(load().dqc_int3c2e(_ptr(out), *tab.args(), s0, s1, k0, k1, st_), "dqc_int3c2e")
    return out


def int2c2e(tab, aux_range, device):
    """(k|l) over the auxiliary shells [k0, k1) of concatenated tables -> (naux, naux)"""
    k0, k1 = aux_range
    naux = _range_nao(tab, k0, k1)
    out = torch.zeros((naux, naux), dtype=torch.float64, device=device)
    with _on(device) as st_:
        _check(load().dqc_int2c2e(_ptr(out), *tab.args(), k0, k1, st_), "dqc_int2c2e")
    return out


def df_coulomb(j3c, inv_j2c, dm_ao, work=None):
    """J_ao (nao, nao) = sum_k (ij|k) [inv_j2c (kl|D)]_k from the stored DF integrals; dm_ao (nao, nao) contiguous"""
    nao, _, naux = j3c.shape
    if work is None:
        work = torch.empty(2 * naux, dtype=torch.float64, device=j3c.device)
    out = torch.empty((nao, nao), dtype=torch.float64, device=j3c.device)
    with _on(j3c.device) as st_:
        _check(load().dqc_df_coulomb(_ptr(out), _ptr(j3c), _ptr(inv_j2c), _ptr(dm_ao), nao, naux, _ptr(work), st_),
               "dqc_df_coulomb")
    return out


def df_exchange_work(nao, naux, rp, device):
    """the work buffer of df_exchange for factors up to `rp` padded columns"""
    return torch.empty(int(load().dqc_df_exchange_work_doubles(int(nao), int(naux), int(rp))), dtype=torch.float64, device=device)


def df_exchange(b, factor_pair, work=None, naux=None):
    """K_ao (nao, nao) = sum_P (B_P L) (B_P L)^T of the density D = L L^T: b (naux, nao, nao) the whitened three-index tensor
    (one contiguous slab per auxiliary function), factor_pair = (orb (ld, rp), orbt (rp, ld)) the padded AO-basis factor of
    fock_factor / pad_factor; naux: contract the leading `naux` slabs of b only (default: all).  Symmetric; under set_deterministic
    bit-reproducible (the Vxc kernels' fixed point on 2^47: |K| < 2^16).  The arguments are checked before anything is launched"""
    if b.dim() != 3 or b.shape[1] != b.shape[2] or b.shape[1] == 0:
        raise DqcAmdError("df_exchange: b must be (naux, nao, nao), got %s" % (tuple(b.shape),))
    nao = int(b.shape[1])
    naux = int(b.shape[0]) if naux is None else int(naux)
    if naux < 0 or naux > b.shape[0]:
        raise DqcAmdError("df_exchange: naux = %d outside [0, %d]" % (naux, b.shape[0]))
    orb, orbt = factor_pair
    ld = padded_nao(nao)
    rp = int(orb.shape[1]) if orb.dim() == 2 else 0
    if orb.dim() != 2 or orb.shape[0] != ld or rp == 0 or padded_norb(rp) != rp:
        raise DqcAmdError("df_exchange: the factor must be (%d, rp) with rp a padded width (padded_norb), got %s" % (ld, tuple(orb.shape)))
    if orbt is not None and tuple(orbt.shape) != (rp, ld):
        raise DqcAmdError("df_exchange: the transposed factor must be (%d, %d), got %s" % (rp, ld, tuple(orbt.shape)))
    need = int(load().dqc_df_exchange_work_doubles(nao, naux, rp))
    if work is None or work.numel() < need:
        work = torch.empty(need, dtype=torch.float64, device=b.device)
    out = torch.empty((ld, ld), dtype=torch.float64, device=b.device)
    with _on(b.device) as st_:
        _check(load().dqc_df_exchange(_ptr(out), _ptr(b), _ptr(orb), _ptr(orbt), nao, naux, rp, _ptr(work), st_), "dqc_df_exchange")
    return out[:nao, :nao]


def mp2_pair_energies(bi, bj, eps_oi, eps_oj, eps_va, eps_vb, same, work=None):
    """RI-MP2 pair energies (csrc/mp2.hip): bi (noi, naux, ldva), bj (noj, naux, ldvb) the occupied-virtual three-index tensors, one
    (naux, ldv) slab per occupied orbital, ldv a multiple of 16 (columns >= nv are ignored); eps_*: the orbital energies, whose lengths
    are the orbital counts.  same=True (bj is bi): (e_os, e_ss), both (no, no) and symmetric; same=False: (e_os (noi, noj), None).
    e_os[i, j] = sum_ab V^2 / D, e_ss[i, j] = sum_ab V (V - V^T) / D.  No atomics: bit-reproducible.  The arguments are checked
    before anything is launched"""
    same = bool(same)
    for name, t in (("bi", bi), ("bj", bj)):
        if t.dim() != 3 or t.shape[2] % 16:
            raise DqcAmdError("mp2_pair_energies: %s must be (nocc, naux, ldv) with ldv a multiple of 16, got %s" % (name, tuple(t.shape)))
    noi, naux, ldva = (int(x) for x in bi.shape)
    noj, ldvb = int(bj.shape[0]), int(bj.shape[2])
    nva, nvb = int(eps_va.numel()), int(eps_vb.numel())
    if int(bj.shape[1]) != naux:
        raise DqcAmdError("mp2_pair_energies: bi and bj have %d and %d auxiliary functions" % (naux, bj.shape[1]))
    if int(eps_oi.numel()) != noi or int(eps_oj.numel()) != noj:
        raise DqcAmdError("mp2_pair_energies: %d and %d occupied energies for %d and %d slabs" % (eps_oi.numel(), eps_oj.numel(), noi, noj))
    if nva > ldva or nvb > ldvb:
        raise DqcAmdError("mp2_pair_energies: %d and %d virtual energies for slabs of %d and %d columns" % (nva, nvb, ldva, ldvb))
    if same and (bj is not bi and bj.data_ptr() != bi.data_ptr() or tuple(bi.shape) != tuple(bj.shape) or nva != nvb):
        raise DqcAmdError("mp2_pair_energies: same=True takes one tensor and one set of virtual energies on both sides")
    if bi.data_ptr() % 16 or bj.data_ptr() % 16:
        raise DqcAmdError("mp2_pair_energies: the tensors must be 16-byte aligned")
    L = load()
    need = int(L.dqc_mp2_work_doubles(noi, noj, nva, nvb, int(same)))
    if work is None or work.numel() < need:
        work = torch.empty(max(need, 1), dtype=torch.float64, device=bi.device)
    eos = torch.empty((noi, noj), dtype=torch.float64, device=bi.device)
    ess = torch.empty((noi, noj), dtype=torch.float64, device=bi.device) if same else None
    with _on(bi.device) as st_:
        _check(L.dqc_mp2_pair_energies(_ptr(eos), _ptr(ess), _ptr(bi), _ptr(bj), _ptr(eps_oi), _ptr(eps_oj), _ptr(eps_va), _ptr(eps_vb),
                                       noi, noj, nva, nvb, ldva, ldvb, naux, int(same), _ptr(work), st_), "dqc_mp2_pair_energies")
    return eos, ess


def _aligned16(who, t):
    if t.data_ptr() % 16:
        raise DqcAmdError("%s: the tensor must be 16-byte aligned" % who)


def _slabs(who, bov, eo, ev):
    """(nocc, naux, ldv, nv) of an occupied-virtual tensor (one (naux, ldv) slab per occupied orbital) and its orbital energies"""
    if bov.dim() != 3 or bov.shape[2] % 16:
        raise DqcAmdError("%s: bov must be (nocc, naux, ldv) with ldv a multiple of 16, got %s" % (who, tuple(bov.shape)))
    nocc, naux, ldv = (int(x) for x in bov.shape)
    nv = int(ev.numel())
    if int(eo.numel()) != nocc:
        raise DqcAmdError("%s: %d occupied energies for %d slabs" % (who, eo.numel(), nocc))
    if nv > ldv:
        raise DqcAmdError("%s: %d virtual energies for slabs of %d columns" % (who, nv, ldv))
    return nocc, naux, ldv, nv


def _out_like(who, out, shape, ref, name):
    """`out`, or a new float64 tensor of `shape` on the device of `ref` (the argument called `name`)"""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=ref.device)
    if tuple(out.shape) != shape or out.device != ref.device or out.dtype != torch.float64 or not out.is_contiguous():
        raise DqcAmdError("%s: out must be a contiguous float64 (%d, %d, %d) tensor on the device of %s, got %s"
                          % ((who,) + shape + (name, tuple(out.shape))))
    return out


def mp2_amplitudes(bov, eo, ev, i0, ni, c_os=1.0, c_ss=1.0, out=None):
    """RI-MP2 amplitudes of the occupied block [i0, i0 + ni) against every occupied orbital (csrc/mp2.hip: dqc_mp2_amplitudes), restricted:
    bov (nocc, naux, ldv) as `mp2_pair_energies` takes it, eo (nocc), ev (nv <= ldv) -> (t, tt), both (ni, nocc, ldv, ldv):
    t[i - i0, j, a, b] = V^{ij}_{ab} / D^{ij}_{ab}, tt = (c_os + c_ss) t - c_ss t^T (2 T - T^T by default).  Rows and columns >= nv are
    written as exactly 0.0.  out: a pair of contiguous float64 device tensors of at least ni * nocc * ldv^2 elements each to write into
    (the results are views of them).  No atomics: bit-reproducible.  The arguments are checked before anything is launched"""
    nocc, naux, ldv, nv = _slabs("mp2_amplitudes", bov, eo, ev)
    i0, ni = int(i0), int(ni)
    if i0 < 0 or ni < 0 or i0 + ni > nocc:
        raise DqcAmdError("mp2_amplitudes: the block [%d, %d) is not inside the %d occupied orbitals" % (i0, i0 + ni, nocc))
    _aligned16("mp2_amplitudes", bov)
    need = ni * nocc * ldv * ldv
    if out is None:
        out = (torch.empty(need, dtype=torch.float64, device=bov.device), torch.empty(need, dtype=torch.float64, device=bov.device))
    t, tt = out
    for o in (t, tt):
        if o.numel() < need or o.device != bov.device or o.dtype != torch.float64 or not o.is_contiguous():
            raise DqcAmdError("mp2_amplitudes: each output needs %d contiguous float64 elements on the device of bov, got %s"
                              % (need, tuple(o.shape)))
    if need and t.data_ptr() == tt.data_ptr():
        raise DqcAmdError("mp2_amplitudes: the two outputs must be different buffers")
    with _on(bov.device) as st_:
        _check(load().dqc_mp2_amplitudes(_ptr(t), _ptr(tt), min(t.numel(), tt.numel()), _ptr(bov), _ptr(eo), _ptr(ev), nocc, nv, ldv, naux,
                                         i0, ni, float(c_os), float(c_ss), st_), "dqc_mp2_amplitudes")
    shape = (ni, nocc, ldv, ldv)
    return t.reshape(-1)[:need].view(shape), tt.reshape(-1)[:need].view(shape)


def rpa_response(bov, eo, ev, freq, scale=1.0, out=None, accumulate=False, work=None):
    """RI-dRPA response matrices (csrc/rpa.hip: dqc_rpa_response): bov (nocc, naux, ldv) as `mp2_pair_energies` takes it, eo (nocc),
    ev (nv <= ldv), freq (nfreq) imaginary frequencies -> Q (nfreq, naux, naux),
    Q[k] = scale sum_ia bov[i, :, a] g_ia(w_k) bov[i, :, a]^T, g_ia(w) = D_ia / (D_ia^2 + w^2), D_ia = ev[a] - eo[i]; both triangles,
    bit-symmetric.  out: the tensor to write into; accumulate=True adds to `out` (the second spin) instead of overwriting it.
    No atomics: bit-reproducible.  The arguments are checked before anything is launched"""
    nocc, naux, ldv, nv = _slabs("rpa_response", bov, eo, ev)
    nfreq = int(freq.numel())
    if freq.dim() != 1:
        raise DqcAmdError("rpa_response: freq must be one-dimensional, got %s" % (tuple(freq.shape),))
    _aligned16("rpa_response", bov)
    accumulate = bool(accumulate)
    if out is None and accumulate:
        raise DqcAmdError("rpa_response: accumulate=True needs the tensor to add to (out=)")
    out = _out_like("rpa_response", out, (nfreq, naux, naux), bov, "bov")
    L = load()
    need = int(L.dqc_rpa_work_doubles(nocc, nv, naux, nfreq))
    if need and (work is None or work.numel() < need):
        work = torch.empty(need, dtype=torch.float64, device=bov.device)
    with _on(bov.device) as st_:
        _check(L.dqc_rpa_response(_ptr(out), _ptr(bov), _ptr(eo), _ptr(ev), _ptr(freq), nocc, nv, ldv, naux, nfreq, float(scale),
                                  int(accumulate), _ptr(work) if need else None, st_), "dqc_rpa_response")
    return out


def gw_screened_diag(wc, bn, nm, out=None):
    """diagonal of the screened interaction (csrc/gw.hip: dqc_gw_screened_diag): wc (nfreq, naux, naux) symmetric, of which only the
    elements P >= R are read; bn (ntarget, naux, ldm) as `mp2.transform_ov` makes it, nm <= ldm real columns ->
    W (nfreq, ntarget, nm), W[k, n, m] = sum_PR bn[n, P, m] wc[k, P, R] bn[n, R, m].  out: the tensor to write into.
    No atomics: bit-reproducible.  The arguments are checked before anything is launched"""
    if bn.dim() != 3 or bn.shape[2] % 16:
        raise DqcAmdError("gw_screened_diag: bn must be (ntarget, naux, ldm) with ldm a multiple of 16, got %s" % (tuple(bn.shape),))
    ntarget, naux, ldm = (int(x) for x in bn.shape)
    nm = int(nm)
    if nm < 0 or nm > ldm:
        raise DqcAmdError("gw_screened_diag: %d columns asked of slabs of %d" % (nm, ldm))
    if wc.dim() != 3 or int(wc.shape[1]) != naux or int(wc.shape[2]) != naux:
        raise DqcAmdError("gw_screened_diag: wc must be (nfreq, %d, %d) for bn of %d auxiliary functions, got %s"
                          % (naux, naux, naux, tuple(wc.shape)))
    nfreq = int(wc.shape[0])
    for name, t in (("wc", wc), ("bn", bn)):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise DqcAmdError("gw_screened_diag: %s must be a contiguous float64 tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
    if wc.device != bn.device or bn.device.type != "cuda":
        raise DqcAmdError("gw_screened_diag: wc and bn must be on one GPU, got %s and %s" % (wc.device, bn.device))
    _aligned16("gw_screened_diag", bn)
    out = _out_like("gw_screened_diag", out, (nfreq, ntarget, nm), bn, "bn")
    with _on(bn.device) as st_:
        _check(load().dqc_gw_screened_diag(_ptr(out), _ptr(wc), _ptr(bn), ntarget, nm, ldm, naux, nfreq, st_), "dqc_gw_screened_diag")
    return out


def bse_exchange(l, r, x, nr, ns, out=None, work=None):
    """product of trial vectors with a four-index quantity in two fitted factors (csrc/bse.hip: dqc_bse_exchange): l (np, naux, ldr) and
    r (nq, naux, lds) as `mp2.transform_ov` makes them, nr <= ldr and ns <= lds real columns, x (nvec, nr, ns) ->
    out (nvec, np, nq), out[v, p, q] = sum_P sum_rs l[p, P, r] x[v, r, s] r[q, P, s].  out: the tensor to write into; work: a buffer
    of at least dqc_bse_work_doubles doubles to reuse (one is allocated when it is missing or too small).
    No atomics: bit-reproducible.  The arguments are checked before anything is launched"""
    for name, t in (("l", l), ("r", r)):
        if t.dim() != 3 or t.shape[2] % 16:
            raise DqcAmdError("bse_exchange: %s must be (n, naux, ld) with ld a multiple of 16, got %s" % (name, tuple(t.shape)))
    np_, naux, ldr = (int(n) for n in l.shape)
    nq, lds = int(r.shape[0]), int(r.shape[2])
    nr, ns = int(nr), int(ns)
    if int(r.shape[1]) != naux:
        raise DqcAmdError("bse_exchange: l holds %d auxiliary functions and r %d" % (naux, int(r.shape[1])))
    if nr < 0 or nr > ldr or ns < 0 or ns > lds:
        raise DqcAmdError("bse_exchange: (%d, %d) columns asked of slabs of (%d, %d)" % (nr, ns, ldr, lds))
    if x.dim() != 3 or int(x.shape[1]) != nr or int(x.shape[2]) != ns:
        raise DqcAmdError("bse_exchange: x must be (nvec, %d, %d), got %s" % (nr, ns, tuple(x.shape)))
    nvec = int(x.shape[0])
    for name, t in (("l", l), ("r", r), ("x", x)):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise DqcAmdError("bse_exchange: %s must be a contiguous float64 tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
    if l.device != r.device or l.device != x.device or l.device.type != "cuda":
        raise DqcAmdError("bse_exchange: l, r and x must be on one GPU, got %s, %s and %s" % (l.device, r.device, x.device))
    _aligned16("bse_exchange", l)
    _aligned16("bse_exchange", r)
    out = _out_like("bse_exchange", out, (nvec, np_, nq), l, "l")
    L = load()
    need = int(L.dqc_bse_work_doubles(np_, nq, nr, ns, naux, nvec))
    if need and (work is None or work.numel() < need or work.dtype != torch.float64 or work.device != l.device or not work.is_contiguous()):
        work = torch.empty(need, dtype=torch.float64, device=l.device)
    with _on(l.device) as st_:
        _check(L.dqc_bse_exchange(_ptr(out), _ptr(l), _ptr(r), _ptr(x), np_, nq, nr, ns, ldr, lds, naux, nvec, _ptr(work) if need else None, st_),
               "dqc_bse_exchange")
    return out


def cc_ladder(l, r, x, nr, ns, out=None, work=None):
    """the particle-particle ladder of coupled-cluster doubles, integral-driven (csrc/cc.hip: dqc_cc_ladder): l (np, naux, ldr) and
    r (nq, naux, lds) as `postscf.transform_ov` makes them (they may be one tensor), nr <= ldr and ns <= lds real columns,
    x (nr, ns, nvec) -- THE VECTOR INDEX LAST -- -> out (nvec, np, nq),
    out[v, p, q] = sum_rs W[p, q, r, s] x[r, s, v], W[p, q, r, s] = sum_P l[p, P, r] r[q, P, s]: each tile of W is summed once and used
    by every vector; no element of it is stored.  out: the tensor to write into; work: taken for the symmetry of the fused entry
    points and never touched (dqc_cc_ladder_work_doubles is 0: no sum is split).  The kernel loads single doubles: no alignment is
    asked of the tensors.  No atomics: bit-reproducible.  The arguments are checked before anything is launched"""
    for name, t in (("l", l), ("r", r)):
        if t.dim() != 3 or t.shape[2] % 16:
            raise DqcAmdError("cc_ladder: %s must be (n, naux, ld) with ld a multiple of 16, got %s" % (name, tuple(t.shape)))
    np_, naux, ldr = (int(n) for n in l.shape)
    nq, lds = int(r.shape[0]), int(r.shape[2])
    nr, ns = int(nr), int(ns)
    if int(r.shape[1]) != naux:
        raise DqcAmdError("cc_ladder: l holds %d auxiliary functions and r %d" % (naux, int(r.shape[1])))
    if nr < 0 or nr > ldr or ns < 0 or ns > lds:
        raise DqcAmdError("cc_ladder: (%d, %d) columns asked of slabs of (%d, %d)" % (nr, ns, ldr, lds))
    if x.dim() != 3 or int(x.shape[0]) != nr or int(x.shape[1]) != ns:
        raise DqcAmdError("cc_ladder: x must be (%d, %d, nvec), got %s" % (nr, ns, tuple(x.shape)))
    nvec = int(x.shape[2])
    for name, t in (("l", l), ("r", r), ("x", x)):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise DqcAmdError("cc_ladder: %s must be a contiguous float64 tensor, got %s %s" % (name, t.dtype, tuple(t.shape)))
    if l.device != r.device or l.device != x.device or l.device.type != "cuda":
        raise DqcAmdError("cc_ladder: l, r and x must be on one GPU, got %s, %s and %s" % (l.device, r.device, x.device))
    out = _out_like("cc_ladder", out, (nvec, np_, nq), l, "l")
    with _on(l.device) as st_:
        _check(load().dqc_cc_ladder(_ptr(out), _ptr(l), _ptr(r), _ptr(x), np_, nq, nr, ns, ldr, lds, naux, nvec, None, st_), "dqc_cc_ladder")
    return out


def cart2sph_matrix(tab, device):
    """T (nao, ncart) block diagonal, chi_m = sum_c T[m, c] g_c (solid harmonics of the Cartesian Gaussians)"""
    ip = ctypes.POINTER(ctypes.c_int)
    ncart = int(load().dqc_ncart(tab.bas.ctypes.data_as(ip), tab.nbas))
    out = np.zeros((tab.nao, ncart))
    _check(load().dqc_cart2sph_matrix(out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tab.bas.ctypes.data_as(ip), tab.nbas),
           "dqc_cart2sph_matrix")
    return torch.as_tensor(out, device=device)


def int1e_grad(grad, dcart, wcart, tab, zs=None):
    """grad (natm, 3) += one-electron derivative terms; dcart / wcart (ncart, ncart) contiguous device tensors"""
    zp = None
    if zs is not None:
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        zp = zs.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with _on(grad.device) as st_:
        _check(load().dqc_int1e_grad(_ptr(grad), _ptr(dcart), _ptr(wcart), *tab.args(), zp, st_), "dqc_int1e_grad")
    return grad


def int1e_potential(dcart, points, tab):
    """(npts,) = sum_ab D_ab <a| 1/|r - P_C| |b> at the points (npts, 3); dcart (ncart, ncart) Cartesian-basis density (T^T D T)"""
    points = points.to(device=dcart.device, dtype=torch.float64).contiguous()
    npts = int(points.shape[0])
    assert points.shape == (npts, 3), "points must be (npts, 3)"
    out = torch.empty(npts, dtype=torch.float64, device=dcart.device)
    with _on(dcart.device) as st_:
        _check(load().dqc_int1e_potential(_ptr(out), _ptr(dcart), _ptr(points), npts, *tab.args(), st_), "dqc_int1e_potential")
    return out


def eri_grad(grad, dcart, kscale, tab, jscale=1.0):
    """grad (natm, 3) += two-electron derivative term  sum (d_A a b|c d) [2 jscale D_ab D_cd - kscale D_ac D_bd]"""
    with _on(grad.device) as st_:
        _check(load().dqc_eri_grad(_ptr(grad), _ptr(dcart), float(jscale), float(kscale), *tab.args(), st_), "dqc_eri_grad")
    return grad


def _parity(m):
    """+1 for an exactly symmetric matrix, -1 for an exactly antisymmetric one (a zero matrix counts as symmetric), else 0"""
    t = m.t()
    return 1 if torch.equal(m, t) else (-1 if torch.equal(m, -t) else 0)


def eri_grad2(grad, acart, bcart, jscale, kscale, tab):
    """grad (natm, 3) += sum_{a on atom A} sum_bcd (d_A a b|c d) [jscale (A_ab B_cd + B_ab A_cd) - kscale / 2 (A_ac B_bd + B_ac A_bd)]
    (csrc/grad.hip: dqc_eri_grad2, the ERI_OUT_GRAD2 kernels of csrc/grad2.hip): the symmetric bilinear form whose diagonal is
    `eri_grad` -- eri_grad2(D, D, j, k) = eri_grad(D, k, jscale=j), and Q(D + P) - Q(D) - Q(P) = 2 eri_grad2(D, P) for the quadratic
    form Q.  acart, bcart (ncart, ncart): contiguous float64 Cartesian-basis matrices on the device of grad, both EXACTLY symmetric
    or both EXACTLY antisymmetric (symmetrise explicitly: torch.equal with +- the transpose is the test), the antisymmetric pair
    with jscale == 0.  Everything is checked before anything is uploaded or launched: DqcAmdError."""
    ncart = int(((tab.bas[:, 1].astype(np.int64) + 1) * (tab.bas[:, 1].astype(np.int64) + 2) // 2).sum())
    if tuple(grad.shape) != (tab.natm, 3) or grad.dtype != torch.float64 or not grad.is_contiguous():
        raise DqcAmdError("eri_grad2: grad must be a contiguous float64 (%d, 3) tensor, got %s %s" % (tab.natm, grad.dtype, tuple(grad.shape)))
    for name, m in (("A", acart), ("B", bcart)):
        if tuple(m.shape) != (ncart, ncart) or m.dtype != torch.float64 or not m.is_contiguous() or m.device != grad.device:
            raise DqcAmdError("eri_grad2: %s must be a contiguous float64 (%d, %d) tensor on the device of grad (the Cartesian "
                              "functions of the table), got %s %s on %s" % (name, ncart, ncart, m.dtype, tuple(m.shape), m.device))
    pa, pb = _parity(acart), _parity(bcart)
    if pa == 0 or pb == 0:
        raise DqcAmdError("eri_grad2: %s is neither exactly symmetric nor exactly antisymmetric (symmetrise it explicitly: "
                          "(M + M^T) / 2 or (M - M^T) / 2)" % ("A" if pa == 0 else "B"))
    if pa != pb and bool(acart.any()) and bool(bcart.any()):
        raise DqcAmdError("eri_grad2: one matrix is symmetric and the other antisymmetric (the bilinear form needs a same-parity pair)")
    if pa != pb:  # (a zero matrix is both: it takes the parity of its partner)
        pa = pb = pb if bool(bcart.any()) else pa
    if pa == -1 and float(jscale) != 0.0:
        raise DqcAmdError("eri_grad2: an antisymmetric pair has no Coulomb part (jscale must be 0)")
    with _on(grad.device) as st_:
        _check(load().dqc_eri_grad2(_ptr(grad), _ptr(acart), _ptr(bcart), ncart, pa, pb, float(jscale), float(kscale), *tab.args(), st_),
               "dqc_eri_grad2")
    return grad


def _check_basis_grad(who, out, mats, tab):
    """out (nprim_total, 2) and the (ncart, ncart) matrices: float64, contiguous, on one device; orbital shells up to f"""
    nprim = int(tab.bas[:, 2].sum())
    ncart = int(((tab.bas[:, 1] + 1) * (tab.bas[:, 1] + 2) // 2).sum())
    if tab.nbas and int(tab.bas[:, 1].max()) > 3:
        raise NotImplementedError("%s: basis-parameter derivatives support orbital shells up to f (the exponent derivative of a "
                                  "g shell needs l + 2 = i integrals)" % who)
    if tuple(out.shape) != (nprim, 2) or out.dtype != torch.float64 or not out.is_contiguous():
        raise DqcAmdError("%s: out must be a contiguous float64 (%d, 2) tensor, got %s" % (who, nprim, tuple(out.shape)))
    for m in mats:
        if tuple(m.shape) != (ncart, ncart) or m.dtype != torch.float64 or not m.is_contiguous() or m.device != out.device:
            raise DqcAmdError("%s: the Cartesian matrices must be contiguous float64 (%d, %d) tensors on the device of out, got %s"
                              % (who, ncart, ncart, tuple(m.shape)))


def int1e_grad_basis(out, dcart, wcart, tab, zs=None):
    """out (nprim_total, 2) += one-electron Pulay terms by every primitive's exponent (column 0) and coefficient (column 1)"""
    _check_basis_grad("int1e_grad_basis", out, (dcart, wcart), tab)
    zp = None
    if zs is not None:
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        zp = zs.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with _on(out.device) as st_:
        _check(load().dqc_int1e_grad_basis(_ptr(out), _ptr(dcart), _ptr(wcart), *tab.args(), zp, st_), "dqc_int1e_grad_basis")
    return out


def eri_grad_basis(out, dcart, kscale, tab, jscale=1.0):
    """out (nprim_total, 2) += sum (d_theta a b|c d) [2 jscale D_ab D_cd - kscale D_ac D_bd], theta = alpha_p, c_p"""
    _check_basis_grad("eri_grad_basis", out, (dcart,), tab)
    with _on(out.device) as st_:
        _check(load().dqc_eri_grad_basis(_ptr(out), _ptr(dcart), float(jscale), float(kscale), *tab.args(), st_), "dqc_eri_grad_basis")
    return out


def becke_weights(xyz, atom_off, pos, inv_rij, aij, cut):
    """xyz (ngrid, 3) the atoms' grids concatenated, atom_off (natm + 1,) int32 device tensor -> Becke partition weights (ngrid,)"""
    ngrid, natm = xyz.shape[0], pos.shape[0]
    assert atom_off.dtype == torch.int32 and atom_off.is_cuda and atom_off.numel() == natm + 1
    w = torch.empty(ngrid, dtype=torch.float64, device=xyz.device)
    with _on(xyz.device) as st_:
        _check(load().dqc_becke_weights(_ptr(w), _ptr(xyz), ctypes.c_void_p(atom_off.data_ptr()), _ptr(pos.contiguous()),
                                        _ptr(inv_rij.contiguous()), _ptr(aij.contiguous()), natm, ngrid, float(cut), st_),
               "dqc_becke_weights")
    return w


def becke_weights_grad(cw, xyz, atom_off, pos, inv_rij, aij, cut):
    """backward of becke_weights: cw (ngrid,) = dL/dw -> (gpos (natm, 3) explicit nuclear part, gxyz (ngrid, 3) point part)"""
    ngrid, natm = xyz.shape[0], pos.shape[0]
    gpos = torch.zeros((natm, 3), dtype=torch.float64, device=xyz.device)
    gxyz = torch.empty((ngrid, 3), dtype=torch.float64, device=xyz.device)
    scratch = torch.empty((natm, ngrid), dtype=torch.float64, device=xyz.device)
    with _on(xyz.device) as st_:
        _check(load().dqc_becke_weights_grad(_ptr(gpos), _ptr(gxyz), _ptr(scratch), _ptr(cw.contiguous()), _ptr(xyz.contiguous()),
                                             ctypes.c_void_p(atom_off.data_ptr()), _ptr(pos.contiguous()), _ptr(inv_rij.contiguous()),
                                             _ptr(aij.contiguous()), natm, ngrid, float(cut), st_), "dqc_becke_weights_grad")
    return gpos, gxyz


def xc_eval_mgga_pol2(terms, rho_u, rho_d, grho_u, grho_d, tau_u, tau_d, want_e=True, want_v=True):
    """spin-polarised meta-GGA correlation terms with one gradient potential per spin (mgga_c_scan, mgga_c_tpss)
    -> edens, (vrho_u, vrho_d), (vgrad_u, vgrad_d) (3, n) each, vtau shared"""
    n = rho_u.shape[0]
    ids = (ctypes.c_int * len(terms))(*[XC_IDS[nm] for _, nm in terms])
    cfs = (ctypes.c_double * len(terms))(*[float(c) for c, _ in terms])
    e = torch.empty_like(rho_u) if want_e else None
    vu = torch.empty_like(rho_u) if want_v else None
    vd = torch.empty_like(rho_u) if want_v else None
    gu = torch.empty((3, n), dtype=torch.float64, device=rho_u.device) if want_v else None
    gd = torch.empty((3, n), dtype=torch.float64, device=rho_u.device) if want_v else None
    vt = torch.empty_like(rho_u) if want_v else None
    with _on(rho_u.device) as st_:
        _check(load().dqc_xc_eval_mgga_pol2(_ptr(e), _ptr(vu), _ptr(vd), _ptr(gu), _ptr(gd), _ptr(vt), _ptr(rho_u), _ptr(rho_d),
                                            _ptr(grho_u), _ptr(grho_d), _ptr(tau_u), _ptr(tau_d), n, ids, cfs, len(terms), st_),
               "dqc_xc_eval_mgga_pol2")
    return e, (vu, vd), (gu, gd), vt


def purify_tc2(x_pad, tmp, nocc, iters, tol, state):
    """in-place TC2 purification of the zero-padded (ld, ld) matrix x_pad (spectrum in [0, 1]); state: 2 (iters + 2)"""
    with _on(x_pad.device) as st_:
        _check(load().dqc_purify_tc2(_ptr(x_pad), _ptr(tmp), x_pad.shape[-1], float(nocc), int(iters), float(tol), _ptr(state),
                                     st_), "dqc_purify_tc2")
    return x_pad


def purify_tc2_persist(x_pad, tmp, nocc, iters, tol, state, ctl):
    """purify_tc2 as ONE persistent launch on one XCD (ld <= 256); ctl: 4-element int32 device scratch, ctl[2] != 0 afterwards =
    the kernel gave up and x_pad is not a projector (the caller's idempotency error shows it)"""
    assert ctl.dtype == torch.int32 and ctl.is_cuda and ctl.numel() >= 4
    with _on(x_pad.device) as st_:
        _check(load().dqc_purify_tc2_persist(_ptr(x_pad), _ptr(tmp), x_pad.shape[-1], float(nocc), int(iters), float(tol), _ptr(state),
                                             ctypes.c_void_p(ctl.data_ptr()), st_), "dqc_purify_tc2_persist")
    return x_pad


def projector_tc2(fock, nocc, iters, tol):
    """fock (n, n) symmetric, n <= 256 -> (P (n, n), err (0-dim)): ONE persistent launch (dqc_projector_tc2)"""
    n = fock.shape[-1]
    p = torch.empty((n, n), dtype=torch.float64, device=fock.device)
    err = torch.empty(1, dtype=torch.float64, device=fock.device)
    work = torch.empty(int(load().dqc_projector_work_doubles(n, int(iters))), dtype=torch.float64, device=fock.device)
    with _on(fock.device) as st_:
        _check(load().dqc_projector_tc2(_ptr(p), _ptr(err), _ptr(fock.contiguous()), n, float(nocc), int(iters), float(tol), _ptr(work), st_),
               "dqc_projector_tc2")
    return p, err[0]


def purify_tc2_batched(x_pad, tmp, nocc, iters, tol, state):
    """in-place TC2 purification of the (nmol, ld, ld) batch x_pad; state (nmol, 2 (iters + 2))"""
    nmol, ld = x_pad.shape[0], x_pad.shape[-1]
    with _on(x_pad.device) as st_:
        _check(load().dqc_purify_tc2_batched(_ptr(x_pad), _ptr(tmp), ld, nmol, float(nocc), int(iters), float(tol), _ptr(state),
                                             st_), "dqc_purify_tc2_batched")
    return x_pad


def orth_factor_batched(y, g, out=None):
    """y (nmol, n, r), g (nmol, r, r) = y^T y -> (nmol, n, r) orthonormal bases (one launch)"""
    nmol, n, r = y.shape
    q = torch.empty_like(y) if out is None else out
    with _on(y.device) as st_:
        _check(load().dqc_orth_factor_batched(_ptr(q), _ptr(y.contiguous()), _ptr(g.contiguous()), n, r, nmol, st_),
               "dqc_orth_factor_batched")
    return q


def diis_solve(gram, m, out=None):
    """gram (nmol, H, H) Gram matrices of the stored error vectors (first m slots valid) -> Pulay coefficients (nmol, H)"""
    nmol, H, _ = gram.shape
    c = torch.empty((nmol, H), dtype=torch.float64, device=gram.device) if out is None else out
    with _on(gram.device) as st_:
        _check(load().dqc_diis_solve(_ptr(c), _ptr(gram), nmol, H, int(m), st_), "dqc_diis_solve")
    return c


def diis_solve_dev(gram, count, out):
    """diis_solve with the number of valid slots min(count, H) read from the device (count: 0-dim / 1-element int64 device tensor)"""
    nmol, H, _ = gram.shape
    assert count.dtype == torch.int64 and count.is_cuda
    with _on(gram.device) as st_:
        _check(load().dqc_diis_solve_dev(_ptr(out), _ptr(gram), nmol, H, ctypes.c_void_p(count.data_ptr()), st_), "dqc_diis_solve_dev")
    return out


def orth_factor(y, g):
    """y (n, r) = P Omega, g (r, r) = y^T y -> (n, r) orthonormal basis of range(P) (Cholesky QR in one launch)"""
    n, r = y.shape
    q = torch.empty_like(y)
    with _on(y.device) as st_:
        _check(load().dqc_orth_factor(_ptr(q), _ptr(y.contiguous()), _ptr(g.contiguous()), n, r, st_), "dqc_orth_factor")
    return q


def df_grad(grad, dcart, ccart, tab, orb_range, aux_range):
    """grad (natm, 3) += gradient of the density-fitted Coulomb energy; dcart (ncart, ncart), ccart (ncart) over the
    Cartesian basis of the whole concatenated table"""
    (s0, s1), (k0, k1) = orb_range, aux_range
    with _on(grad.device) as st_:
        _check(load().dqc_df_grad(_ptr(grad), _ptr(dcart), _ptr(ccart), *tab.args(), s0, s1, k0, k1, st_), "dqc_df_grad")
    return grad


def _ncart_range(tab, rng):
    l = tab.bas[rng[0]:rng[1], 1].astype(np.int64)
    return int(((l + 1) * (l + 2) // 2).sum())


def df_grad3(grad, z, g, tab, orb_range, aux_range):
    """grad (natm of the table, 3) += sum Z[i, j, k] d(ij|k) - 1/2 sum G[k, l] d(k|l) (csrc/grad.hip: dqc_df_grad3) over the
    concatenated table.  z (no, no, nk), symmetric in its first two indices, and g (nk, nk), symmetric: contiguous float64 tensors on
    the device of grad over the Cartesian functions of the shells `orb_range` and `aux_range` alone; either may be None (that term is
    skipped: Z is walked in blocks of auxiliary shells with g=None, G passed once with z=None)"""
    (s0, s1), (k0, k1) = (int(x) for x in orb_range), (int(x) for x in aux_range)
    if not (0 <= s0 <= s1 <= tab.nbas and 0 <= k0 <= k1 <= tab.nbas):
        raise DqcAmdError("df_grad3: shell ranges outside the table")
    no, nk = _ncart_range(tab, (s0, s1)), _ncart_range(tab, (k0, k1))
    if tuple(grad.shape) != (tab.natm, 3) or grad.dtype != torch.float64 or not grad.is_contiguous():
        raise DqcAmdError("df_grad3: grad must be a contiguous float64 (%d, 3) tensor, got %s" % (tab.natm, tuple(grad.shape)))
    for name, m, shape in (("Z", z, (no, no, nk)), ("G", g, (nk, nk))):
        if m is not None and (tuple(m.shape) != shape or m.dtype != torch.float64 or not m.is_contiguous() or m.device != grad.device):
            raise DqcAmdError("df_grad3: %s must be a contiguous float64 %s tensor on the device of grad (the Cartesian functions of "
                              "the shell ranges), got %s %s on %s" % (name, shape, m.dtype, tuple(m.shape), m.device))
    with _on(grad.device) as st_:
        _check(load().dqc_df_grad3(_ptr(grad), None if z is None else _ptr(z), 0 if z is None else z.numel(),
                                   None if g is None else _ptr(g), *tab.args(), s0, s1, k0, k1, st_), "dqc_df_grad3")
    return grad


def eri_dense(tiles, nao):
    out = torch.empty((nao,) * 4, dtype=torch.float64, device=tiles.device)
    with _on(tiles.device) as st_:
        _check(load().dqc_eri_tiles_to_dense(_ptr(out), _ptr(tiles), nao, st_), "dqc_eri_tiles_to_dense")
    return out


def jk_workspace(nao, device):
    return torch.empty(load().dqc_jk_work_doubles(nao), dtype=torch.float64, device=device)


def jk(tiles, dm_ao, work, with_k=True):
    """dm_ao (nao,nao) -> J, K (K = None if not with_k); AO basis, symmetrised"""
    nao = dm_ao.shape[-1]
    J = torch.empty((nao, nao), dtype=torch.float64, device=dm_ao.device)
    K = torch.empty_like(J) if with_k else None
    with _on(dm_ao.device) as st_:
        _check(load().dqc_jk_from_tiles(_ptr(J), _ptr(K), _ptr(tiles), _ptr(dm_ao.contiguous()), nao, _ptr(work),
                                        st_), "dqc_jk_from_tiles")
    return J, K


def fock_max_nao():
    return int(load().dqc_fock_max_nao())


def fock_factor(x, c, w, nao, ld):
    """the padded AO-basis factor pair (orb (ld, rp), orbt (rp, ld)) of D = C diag(w) C^T: L = X (C sqrt(w)) in one launch; None when
    the factor is wider than the density kernel's widest instantiation.  c: (north, r) with unit column stride, w: (r,) >= 0"""
    r = c.shape[1]
    rp = padded_norb(r)
    if rp == 0:
        return None
    assert (c.shape[1] == 1 or c.stride(1) == 1) and c.dtype == torch.float64 and w.is_contiguous()  # (rows c.stride(0) apart)
    orb = torch.empty((ld, rp), dtype=torch.float64, device=x.device)
    orbt = torch.empty((rp, ld), dtype=torch.float64, device=x.device)
    with _on(x.device) as st_:
        _check(load().dqc_fock_factor(_ptr(orb), _ptr(orbt), _ptr(x), ctypes.c_void_p(c.data_ptr()), int(c.stride(0)), _ptr(w), int(nao),
                                      int(x.shape[1]), int(r), int(ld), int(rp), st_), "dqc_fock_factor")
    return orb, orbt


def fock_orb2dm(x, c, w, nao, ld):
    """ao_orb2dm and its AO-basis factor in one launch -> dm (north, north) = C diag(w) C^T and the padded factor pair (orb, orbt) of
    L = X (C sqrt(w)); None when the factor is wider than the density kernel's widest instantiation"""
    r = c.shape[1]
    rp = padded_norb(r)
    if rp == 0:
        return None
    assert (c.shape[1] == 1 or c.stride(1) == 1) and c.dtype == torch.float64 and w.is_contiguous()  # (rows c.stride(0) apart)
    north = x.shape[1]
    dm = torch.empty((north, north), dtype=torch.float64, device=x.device)
    orb = torch.empty((ld, rp), dtype=torch.float64, device=x.device)
    orbt = torch.empty((rp, ld), dtype=torch.float64, device=x.device)
    with _on(x.device) as st_:
        _check(load().dqc_fock_orb2dm(_ptr(dm), _ptr(orb), _ptr(orbt), _ptr(x), ctypes.c_void_p(c.data_ptr()), int(c.stride(0)), _ptr(w),
                                      int(nao), int(north), int(r), int(ld), int(rp), st_), "dqc_fock_orb2dm")
    return dm, (orb, orbt)


def fock_prep(work, x, nao, with_k, dm=None, orb=None):
    """work <- symmetric AO density + zeroed accumulators: from the orthogonal-basis `dm` (north, north) and the orthogonaliser `x`
    (nao, north), or from the AO-basis factor `orb` (rows >= nao zero, rp columns): D_ao = orb orb^T"""
    north = x.shape[1]
    with _on(work.device) as st_:
        _check(load().dqc_fock_prep(_ptr(work), _ptr(dm), _ptr(x), _ptr(orb), 0 if orb is None else orb.shape[1], int(nao), int(north),
                                    1 if with_k else 0, st_), "dqc_fock_prep")


def jk_stream_prepared(tiles, nao, work, with_k):
    with _on(work.device) as st_:
        _check(load().dqc_jk_stream_prepared(_ptr(tiles), int(nao), _ptr(work), 1 if with_k else 0, st_),
               "dqc_jk_from_tiles" if with_k else "dqc_jk_from_tiles[J only]")


def fock_finish(work, x, nao, with_k, vxc_ao=None, core=None, want_j=False, vscale=None, kfrac=None, exc=None):
    """the closing launch of a fused Fock build -> fock (north, north) = sym(X^T (J - kfrac K / 2 + V) X) + core, energies, J_ao or None.
    `vxc_ao`: a symmetric AO-basis matrix or, with their `vscale`, the raw sums of grid_vxc_raw.  Which entry point closes the build:
    dqc_fock_finish_hybrid when a fraction `kfrac` and a Vxc are given -- energies (3,) = [tr D J / 2, -kfrac tr D K / 4, E_xc handed
    through from the (1,) tensor `exc`]; dqc_fock_finish_vraw for raw sums without exchange; else dqc_fock_finish (K as a whole when
    `with_k`, J_ao on request) -- energies (2,) = [tr D J / 2, -tr D K / 4]"""
    north, nv = x.shape[1], 0 if vxc_ao is None else int(vxc_ao.shape[-1])
    hybrid, raw = kfrac is not None and vxc_ao is not None, vscale is not None
    assert (hybrid or kfrac is None) and not (want_j and (hybrid or raw)) and not (raw and with_k and not hybrid)
    fock = torch.empty((north, north), dtype=torch.float64, device=work.device)
    en = torch.empty(3 if hybrid else 2, dtype=torch.float64, device=work.device)
    jao = torch.empty((nao, nao), dtype=torch.float64, device=work.device) if want_j else None
    with _on(work.device) as st_:
        if hybrid:
            _check(load().dqc_fock_finish_hybrid(_ptr(fock), _ptr(en), _ptr(work), _ptr(vxc_ao), nv, 1 if raw else 0,
                                                 float(vscale) if raw else 0.0, float(kfrac), _ptr(exc), _ptr(core), _ptr(x),
                                                 int(nao), int(north), st_), "dqc_fock_finish_hybrid")
        elif raw:
            _check(load().dqc_fock_finish_vraw(_ptr(fock), _ptr(en), _ptr(work), _ptr(vxc_ao), nv, float(vscale), _ptr(core),
                                               _ptr(x), int(nao), int(north), st_), "dqc_fock_finish")
        else:
            _check(load().dqc_fock_finish(_ptr(fock), _ptr(en), _ptr(jao), _ptr(work), _ptr(vxc_ao), nv, _ptr(core), _ptr(x),
                                          int(nao), int(north), 1 if with_k else 0, st_), "dqc_fock_finish")
    return fock, en, jao


def jk_direct(tab, dm_ao, with_k=True):
    """direct SCF: J, K (K = None if not with_k) of one AO density straight from the shell quartets (no tile store)"""
    nao = dm_ao.shape[-1]
    J = torch.empty((nao, nao), dtype=torch.float64, device=dm_ao.device)
    K = torch.empty_like(J) if with_k else None
    with _on(dm_ao.device) as st_:
        _check(load().dqc_jk_direct(_ptr(J), _ptr(K), _ptr(dm_ao.contiguous()), *tab.args(), st_), "dqc_jk_direct")
    return J, K


def eri_pair_stats(tab, merge=True):
    """host-side size of the ERI pair tables (no GPU needed): dict(groups, pairs, primitive_pairs, primitive_quartets)"""
    out = (ctypes.c_longlong * 4)()
    _check(load().dqc_eri_pair_stats(*tab.args(), 1 if merge else 0, out), "dqc_eri_pair_stats")
    return {"groups": out[0], "pairs": out[1], "primitive_pairs": out[2], "primitive_quartets": out[3]}


class DirectContext:
    """screened direct SCF (include/dqc_amd.h: dqc_direct_*): pair tables and Schwarz bounds resident on the device.
    `jk(dm, with_k, tau)` skips the shell quartets whose contribution is bounded by `tau` (0: none skipped)."""

    def __init__(self, tab, device):
        self.device = torch.device(device)
        self.nao = tab.nao
        self._h = ctypes.c_void_p()
        with _on(self.device) as st_:
            _check(load().dqc_direct_create(ctypes.byref(self._h), *tab.args(), st_), "dqc_direct_create")

    def jk(self, dm_ao, with_k=True, tau=0.0, part=(0, 1)):
        """J, K (K = None if not with_k) of one AO density; part = (r, n): only every n-th block of shell quartets, starting
        with the r-th -- the partial sums of rank r when one molecule is spread over n GPUs (the caller all_reduces)"""
        J = torch.empty((self.nao, self.nao), dtype=torch.float64, device=dm_ao.device)
        K = torch.empty_like(J) if with_k else None
        with _on(dm_ao.device) as st_:
            _check(load().dqc_direct_jk_part(self._h, _ptr(J), _ptr(K), _ptr(dm_ao.contiguous()), float(tau), int(part[0]), int(part[1]),
                                             st_), "dqc_direct_jk_part")
        return J, K

    def stats(self):
        """(unique shell quartets, quartets launched, max |D|) of the last jk call"""
        a, b, d = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
        _check(load().dqc_direct_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(d)), "dqc_direct_stats")
        return a.value, b.value, d.value

    def bounds(self, groups=False):
        """(Q (npairs,), shells (npairs, 2)): Schwarz bound sqrt(max |(ab|ab)|) of every shell pair, table order; groups=True adds
        the index of the GROUP pair each shell pair is screened with (s shells of one atom over the same exponents are evaluated
        together, with the largest bound of their members)"""
        n = int(load().dqc_direct_npairs(self._h))
        q, sh, gr = np.zeros(n), np.zeros((n, 2), dtype=np.int32), np.zeros(n, dtype=np.int32)
        _check(load().dqc_direct_bounds_groups(self._h, q.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                               sh.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), gr.ctypes.data_as(ctypes.POINTER(ctypes.c_int))),
               "dqc_direct_bounds_groups")
        return (q, sh, gr) if groups else (q, sh)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            with _on(self.device):
                load().dqc_direct_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tile_slice(nao, part, nparts):
    """(tile_begin, tile_end, doubles) of the `part`-th of `nparts` contiguous slices of the packed tile store, equal in DOUBLES to
    within a tile (the tiles differ in size: diagonal block pairs, the truncated last block row), i.e. equal streaming work"""
    L = load()
    nao = int(nao)
    nt = int(L.dqc_eri_tile_count(nao))
    tot = int(L.dqc_eri_tile_offset(nao, nt))

    def cut(k):  # first tile whose offset reaches k / nparts of the store (bisection on the monotone offset function)
        if k <= 0:
            return 0
        if k >= nparts:
            return nt
        want, lo, hi = tot * k // nparts, 0, nt
        while lo < hi:
            mid = (lo + hi) // 2
            if int(L.dqc_eri_tile_offset(nao, mid)) < want:
                lo = mid + 1
            else:
                hi = mid
        return lo

    t0, t1 = cut(part), cut(part + 1)
    return t0, t1, int(L.dqc_eri_tile_offset(nao, t1) - L.dqc_eri_tile_offset(nao, t0))


def eri_tiles_part(tab, device, t0, t1):
    """the tiles [t0, t1) of the packed store (one rank's slice when the store is spread over several GPUs)"""
    L = load()
    n = int(L.dqc_eri_tile_offset(tab.nao, t1) - L.dqc_eri_tile_offset(tab.nao, t0))
    tiles = torch.empty(max(n, 1), dtype=torch.float64, device=device)
    with _on(device) as st_:
        _check(L.dqc_eri_fill_tiles_part(_ptr(tiles), *tab.args(), int(t0), int(t1), st_), "dqc_eri_fill_tiles_part")
    return tiles


def jk_part(tiles_part, dm_ao, work, with_k, t0, t1):
    """PARTIAL J, K (the contributions of the tiles [t0, t1) held in `tiles_part`): the caller sums the ranks' parts"""
    nao = dm_ao.shape[-1]
    J = torch.empty((nao, nao), dtype=torch.float64, device=dm_ao.device)
    K = torch.empty_like(J) if with_k else None
    with _on(dm_ao.device) as st_:
        _check(load().dqc_jk_from_tiles_part(_ptr(J), _ptr(K), _ptr(tiles_part), _ptr(dm_ao.contiguous()), nao, _ptr(work),
                                             int(t0), int(t1), st_), "dqc_jk_from_tiles_part")
    return J, K


def jk_multi(tiles, dms_j, dms_k, work=None, k_antisym=None):
    """ONE pass over the tiles for several density matrices: dms_j (nj, nao, nao) -> J (nj, nao, nao), dms_k (nk, nao, nao)
    -> K (nk, nao, nao) (plain K, not -K/2); either may be None.  AO basis, symmetrised.
    k_antisym: a sequence of nk flags; a flagged exchange density is ANTISYMMETRISED instead, (D - D^T) / 2, and its K[D]_pq =
    (pr|qs) D_rs is antisymmetric (dqc_jk_from_tiles_multi_asym; two exchange densities of either kind share a pass).
    Deterministic mode, the contract of the shared scale: the densities of one pass (all of dms_j and the first two of dms_k; then two of
    dms_k per pass) are summed on ONE fixed-point scale, set by the largest sum_ij |D_ij| among them.  Every J and K of the pass is
    therefore exact to 1e-12 of the LARGEST result of the pass, not of its own: a density 2^-27 times smaller than its partner keeps
    about eight digits less.  The scale depends on the largest density alone, so its results are bit for bit those it has beside any
    smaller partner.  Densities of very different size that each need full relative accuracy go in separate calls."""
    ref = dms_j if dms_j is not None else dms_k
    nao, dev = ref.shape[-1], ref.device
    nj = 0 if dms_j is None else dms_j.shape[0]
    nk = 0 if dms_k is None else dms_k.shape[0]
    need = load().dqc_jk_multi_work_doubles(nao, nj, nk)
    if work is None or work.numel() < need:
        work = torch.empty(need, dtype=torch.float64, device=dev)
    J = torch.empty((nj, nao, nao), dtype=torch.float64, device=dev) if nj else None
    K = torch.empty((nk, nao, nao), dtype=torch.float64, device=dev) if nk else None
    if k_antisym is not None:
        flags = [1 if f else 0 for f in k_antisym]
        if len(flags) != nk:
            raise ValueError("jk_multi: k_antisym needs one flag per exchange density (%d), got %d" % (nk, len(flags)))
        mask = (ctypes.c_int * max(nk, 1))(*flags)
        with _on(dev) as st_:
            _check(load().dqc_jk_from_tiles_multi_asym(_ptr(J), _ptr(None if dms_j is None else dms_j.contiguous()), nj,
                                                       _ptr(K), _ptr(None if dms_k is None else dms_k.contiguous()), nk, mask,
                                                       _ptr(tiles), nao, _ptr(work), st_), "dqc_jk_from_tiles_multi_asym")
        return J, K
    with _on(dev) as st_:
        _check(load().dqc_jk_from_tiles_multi(_ptr(J), _ptr(None if dms_j is None else dms_j.contiguous()), nj,
                                              _ptr(K), _ptr(None if dms_k is None else dms_k.contiguous()), nk,
                                              _ptr(tiles), nao, _ptr(work), st_), "dqc_jk_from_tiles_multi")
    return J, K


def eval_gto(tab, rgrid, deriv):
    """rgrid (ngrid,3) device -> (ngrid, lda) [deriv 0], (4, ngrid, lda) [deriv 1], (5, ngrid, lda) [deriv 2: + laplacian]
    or (10, ngrid, lda) [deriv 3: + xx xy xz yy yz zz]; lda = ao_stride(nao) (the array carries the kernels' slack, see ao_empty)"""
    ngrid = rgrid.shape[0]
    ncomp = {0: 0, 1: 4, 2: 5, 3: 10}[deriv]
    nc = max(ncomp, 1)
    lda = ao_stride(tab.nao)
    flat = torch.empty(int(load().dqc_ao_doubles(nc, int(ngrid), int(tab.nao))), dtype=torch.float64, device=rgrid.device)
    out = flat[:nc * ngrid * lda].view(nc, ngrid, lda)
    out = out[0] if ncomp == 0 else out
    with _on(rgrid.device) as st_:
        _check(load().dqc_eval_gto(deriv, _ptr(out), _ptr(rgrid.contiguous()), ngrid, *tab.args(), st_),
               "dqc_eval_gto")
    return out


def pad_matrix(m, ld):
    n = m.shape[-1]
    if n == ld:
        return m.contiguous()
    out = torch.zeros((ld, ld), dtype=m.dtype, device=m.device)
    out[:n, :n] = m
    return out


def grid_density(ao, nao, dm_pad, gga):
    """ao (ngrid, ld) or (4, ngrid, ld); dm_pad (ld, ld) -> rho (ngrid,), grho (3,ngrid) or None"""
    ncomp = 1 if ao.dim() == 2 else ao.shape[0]
    ngrid = ao.shape[-2]
    rho = torch.empty(ngrid, dtype=torch.float64, device=ao.device)
    grho = torch.empty((3, ngrid), dtype=torch.float64, device=ao.device) if gga else None
    with _on(ao.device) as st_:
        _check(load().dqc_grid_density(_ptr(rho), _ptr(grho), _ptr(ao), ncomp, ngrid, nao, _ptr(dm_pad), st_),
               "dqc_grid_density" if gga else "dqc_grid_density[value only]")
    return rho, grho


def padded_norb(norb):
    """factor width the low-rank density kernel is instantiated for (0: too wide, use grid_density)"""
    return int(load().dqc_padded_norb(int(norb)))


def pad_factor(l_ao, ld):
    """l_ao (nao, r) -> (orb (ld, rp), orbt (rp, ld)) zero padded, or None when r is too wide"""
    nao, r = l_ao.shape
    rp = padded_norb(r)
    if rp == 0:
        return None
    orb = torch.zeros((ld, rp), dtype=torch.float64, device=l_ao.device)
    orb[:nao, :r] = l_ao
    return orb, orb.t().contiguous()


def grid_density_lr(ao, nao, factor, gga):
    """density of D = L L^T from the padded factor pair of `pad_factor` -> rho, grho (same as grid_density)"""
    orb, orbt = factor
    ncomp = 1 if ao.dim() == 2 else ao.shape[0]
    ngrid = ao.shape[-2]
    rho = torch.empty(ngrid, dtype=torch.float64, device=ao.device)
    grho = torch.empty((3, ngrid), dtype=torch.float64, device=ao.device) if gga else None
    with _on(ao.device) as st_:
        _check(load().dqc_grid_density_lr(_ptr(rho), _ptr(grho), _ptr(ao), ncomp, ngrid, nao, _ptr(orb), _ptr(orbt),
                                          orb.shape[1], st_), "dqc_grid_density_lr" if gga else "dqc_grid_density_lr[value only]")
    return rho, grho


def grid_density_lr_pol(ao, nao, factor_u, factor_d):
    """both spin densities of D_u = L_u L_u^T, D_d = L_d L_d^T from ONE pass over the AO matrix (GGA form): padded factor pairs of
    `pad_factor`, brought to the same padded width (<= 64 columns each) -> rho (2, ngrid), grho (2, 3, ngrid); None when the
    widths do not fit"""
    rp = max(factor_u[0].shape[1], factor_d[0].shape[1])
    if rp > 64 or ao.dim() != 3 or ao.shape[0] < 4:
        return None

    def widen(f):
        orb, orbt = f
        if orb.shape[1] == rp:
            return orb, orbt
        o2 = torch.zeros((orb.shape[0], rp), dtype=orb.dtype, device=orb.device)
        o2[:, :orb.shape[1]] = orb
        return o2, o2.t().contiguous()
    (ou, otu), (od, otd) = widen(factor_u), widen(factor_d)
    orb = torch.cat([ou, od], dim=1).contiguous()
    orbt = torch.cat([otu, otd], dim=0).contiguous()
    ngrid = ao.shape[-2]
    rho = torch.empty((2, ngrid), dtype=torch.float64, device=ao.device)
    grho = torch.empty((2, 3, ngrid), dtype=torch.float64, device=ao.device)
    with _on(ao.device) as st_:
        _check(load().dqc_grid_density_lr_pol(_ptr(rho), _ptr(grho), _ptr(ao), ao.shape[0], ngrid, nao, _ptr(orb), _ptr(orbt), rp, st_),
               "dqc_grid_density_lr_pol")
    return rho, grho


def grid_xc_gradient_terms(ao, nao, b, c, w, vrho, u, grho, vtau=None):
    """per-point (ngrid, 3) and per-basis-function (nao, 3) grid sums of the XC nuclear gradient (dqc_amd/gradient.py) from one
    pass over the deriv-3 AO array `ao` (10, ngrid, lda); b, c[0..2]: (ngrid, ldb) = Phi D, d_i Phi D"""
    ngrid = ao.shape[-2]
    q = torch.empty((ngrid, 3), dtype=torch.float64, device=ao.device)
    per_ao = torch.empty((nao, 3), dtype=torch.float64, device=ao.device)
    b, c0, c1, c2 = b.contiguous(), c[0].contiguous(), c[1].contiguous(), c[2].contiguous()
    u, grho, w, vrho = u.contiguous(), grho.contiguous(), w.contiguous(), vrho.contiguous()
    vt = None if vtau is None else vtau.contiguous()
    with _on(ao.device) as st_:
        _check(load().dqc_grid_xc_gradient_terms(_ptr(q), _ptr(per_ao), _ptr(ao), ngrid, nao, _ptr(b), _ptr(c0), _ptr(c1), _ptr(c2),
                                                 b.shape[-1], _ptr(w), _ptr(vrho), _ptr(u), _ptr(grho), _ptr(vt), st_),
               "dqc_grid_xc_gradient_terms")
    return q, per_ao


def grid_density_lr_tau(ao, nao, factor):
    """rho, grad rho (3, ngrid), tau of D = L L^T from ONE pass over the four AO components (factor width <= 96 columns)"""
    orb = factor[0]
    ngrid = ao.shape[-2]
    rho = torch.empty(ngrid, dtype=torch.float64, device=ao.device)
    grho = torch.empty((3, ngrid), dtype=torch.float64, device=ao.device)
    tau = torch.empty(ngrid, dtype=torch.float64, device=ao.device)
    with _on(ao.device) as st_:
        _check(load().dqc_grid_density_lr_tau(_ptr(rho), _ptr(grho), _ptr(tau), _ptr(ao), ao.shape[0], ngrid, nao, _ptr(orb),
                                              orb.shape[1], st_), "dqc_grid_density_lr_tau")
    return rho, grho, tau


def xc_eval(terms, rho, grho, want_e=True, want_v=True):
    """terms: list of (coef, name).  -> edens, vrho, vgrad(3,n) (None where not requested/applicable)"""
    n = rho.shape[0]
    ids = (ctypes.c_int * len(terms))(*[XC_IDS[nm] for _, nm in terms])
    cfs = (ctypes.c_double * len(terms))(*[float(c) for c, _ in terms])
    e = torch.empty_like(rho) if want_e else None
    v = torch.empty_like(rho) if want_v else None
    vg = torch.empty((3, n), dtype=torch.float64, device=rho.device) if (want_v and grho is not None) else None
    with _on(rho.device) as st_:
        _check(load().dqc_xc_eval(_ptr(e), _ptr(v), _ptr(vg), _ptr(rho), _ptr(grho), n, ids, cfs, len(terms), st_),
               "dqc_xc_eval")
    return e, v, vg


def xc_eval_quad(terms, rho, grho, w, want_v=True):
    """potentials AND the quadrature E_xc = sum_i w_i e_i from one pass over the grid -> exc (result in exc[0]), vrho, vgrad (3, n) or None"""
    n = rho.shape[0]
    ids = (ctypes.c_int * len(terms))(*[XC_IDS[nm] for _, nm in terms])
    cfs = (ctypes.c_double * len(terms))(*[float(c) for c, _ in terms])
    exc = torch.empty(1025, dtype=torch.float64, device=rho.device)  # DQC_XC_QUAD_DOUBLES: result + per-block partials
    v = torch.empty_like(rho) if want_v else None
    vg = torch.empty((3, n), dtype=torch.float64, device=rho.device) if (want_v and grho is not None) else None
    with _on(rho.device) as st_:
        _check(load().dqc_xc_eval_quad(_ptr(exc), None, _ptr(v), _ptr(vg), _ptr(rho), _ptr(grho), _ptr(w), n, ids, cfs, len(terms),
                                       st_), "dqc_xc_eval_quad")
    return exc, v, vg


def xc_eval_pol(terms, rho_u, rho_d, grho_u, grho_d, want_e=True, want_v=True):
    """-> edens, (vrho_u, vrho_d), (vgrad_u, vgrad_d)   (None where not requested / LDA)"""
    n = rho_u.shape[0]
    ids = (ctypes.c_int * len(terms))(*[XC_IDS[nm] for _, nm in terms])
    cfs = (ctypes.c_double * len(terms))(*[float(c) for c, _ in terms])
    gga = grho_u is not None
    e = torch.empty_like(rho_u) if want_e else None
    vu = torch.empty_like(rho_u) if want_v else None
    vd = torch.empty_like(rho_u) if want_v else None
    gu = torch.empty((3, n), dtype=torch.float64, device=rho_u.device) if (want_v and gga) else None
    gd = torch.empty((3, n), dtype=torch.float64, device=rho_u.device) if (want_v and gga) else None
    with _on(rho_u.device) as st_:
        _check(load().dqc_xc_eval_pol(_ptr(e), _ptr(vu), _ptr(vd), _ptr(gu), _ptr(gd), _ptr(rho_u), _ptr(rho_d),
                                      _ptr(grho_u), _ptr(grho_d), n, ids, cfs, len(terms), st_), "dqc_xc_eval_pol")
    return e, (vu, vd), (gu, gd)


def _fxc_terms(terms, who):
    for _, nm in terms:
        if nm.startswith("mgga_"):
            raise NotImplementedError("%s: no second-order kernel for the meta-GGA functional %s (LDA and GGA only)" % (who, nm))
    ids = (ctypes.c_int * len(terms))(*[XC_IDS[nm] for _, nm in terms])
    cfs = (ctypes.c_double * len(terms))(*[float(c) for c, _ in terms])
    return ids, cfs


def xc_eval_fxc(terms, rho, grho, drho, dgrho):
    """second functional derivatives contracted with nvec trial responses: rho (n,), grho (3, n) or None (LDA); drho (nvec, n),
    dgrho (nvec, 3, n) or None -> dvrho (nvec, n), dvgrad (nvec, 3, n) or None = d(2 vsigma grad rho), the layout of xc_eval"""
    ids, cfs = _fxc_terms(terms, "xc_eval_fxc")
    nvec, n = drho.shape
    gga = grho is not None and dgrho is not None
    rho, drho = rho.contiguous(), drho.contiguous()
    grho, dgrho = (grho.contiguous(), dgrho.contiguous()) if gga else (None, None)
    dv = torch.empty_like(drho)
    dvg = torch.empty((nvec, 3, n), dtype=torch.float64, device=rho.device) if gga else None
    with _on(rho.device) as st_:
        _check(load().dqc_xc_eval_fxc(_ptr(dv), _ptr(dvg), _ptr(rho), _ptr(grho), _ptr(drho), _ptr(dgrho), n, nvec, ids, cfs,
                                      len(terms), st_), "dqc_xc_eval_fxc")
    return dv, dvg


def xc_eval_kxc(terms, rho, grho, drho1, dgrho1, drho2, dgrho2):
    """third functional derivatives contracted with npair PAIRS of responses (restricted closed shell): rho (n,), grho (3, n) or None
    (LDA); drho1, drho2 (npair, n), dgrho1, dgrho2 (npair, 3, n) or None -> d2vrho (npair, n), d2vgrad (npair, 3, n) or None = the
    second-order change of (v_rho, 2 vsigma grad rho), the layout of xc_eval_fxc; symmetric in the two responses"""
    ids, cfs = _fxc_terms(terms, "xc_eval_kxc")
    npair, n = drho1.shape
    gga = grho is not None and dgrho1 is not None and dgrho2 is not None
    if tuple(rho.shape) != (n,) or tuple(drho2.shape) != (npair, n) or (gga and not (
            tuple(grho.shape) == (3, n) and tuple(dgrho1.shape) == (npair, 3, n) and tuple(dgrho2.shape) == (npair, 3, n))):
        raise DqcAmdError("xc_eval_kxc: rho (n,), grho (3, n), drho1 / drho2 (npair, n), dgrho1 / dgrho2 (npair, 3, n) do not fit together")
    rho, drho1, drho2 = rho.contiguous(), drho1.contiguous(), drho2.contiguous()
    grho, dgrho1, dgrho2 = (grho.contiguous(), dgrho1.contiguous(), dgrho2.contiguous()) if gga else (None, None, None)
    d2v = torch.empty_like(drho1)
    d2vg = torch.empty((npair, 3, n), dtype=torch.float64, device=rho.device) if gga else None
    with _on(rho.device) as st_:
        _check(load().dqc_xc_eval_kxc(_ptr(d2v), _ptr(d2vg), _ptr(rho), _ptr(grho), _ptr(drho1), _ptr(dgrho1), _ptr(drho2), _ptr(dgrho2),
                                      n, npair, ids, cfs, len(terms), st_), "dqc_xc_eval_kxc")
    return d2v, d2vg


def xc_eval_fxc_triplet(terms, rho, grho, drho, dgrho):
    """the spin-flip (triplet) response of a closed shell, arguments and outputs as xc_eval_fxc (TOTAL density and response in): the
    spin-up output of xc_eval_fxc_pol at rho_u = rho_d = rho / 2 under d rho_u = -d rho_d = d rho / 2, halved inside the kernel"""
    ids, cfs = _fxc_terms(terms, "xc_eval_fxc_triplet")
    nvec, n = drho.shape
    gga = grho is not None and dgrho is not None
    rho, drho = rho.contiguous(), drho.contiguous()
    grho, dgrho = (grho.contiguous(), dgrho.contiguous()) if gga else (None, None)
    dv = torch.empty_like(drho)
    dvg = torch.empty((nvec, 3, n), dtype=torch.float64, device=rho.device) if gga else None
    with _on(rho.device) as st_:
        _check(load().dqc_xc_eval_fxc_triplet(_ptr(dv), _ptr(dvg), _ptr(rho), _ptr(grho), _ptr(drho), _ptr(dgrho), n, nvec, ids, cfs,
                                              len(terms), st_), "dqc_xc_eval_fxc_triplet")
    return dv, dvg


def xc_eval_fxc_pol(terms, rho_u, rho_d, grho_u, grho_d, drho_u, drho_d, dgrho_u, dgrho_d):
    """spin-polarised xc_eval_fxc -> (dvrho_u, dvrho_d), (dvgrad_u, dvgrad_d) (None for LDA), each (nvec, n) / (nvec, 3, n)"""
    ids, cfs = _fxc_terms(terms, "xc_eval_fxc_pol")
    nvec, n = drho_u.shape
    gga = grho_u is not None and dgrho_u is not None
    c = lambda t: None if (t is None or not gga) else t.contiguous()  # noqa: E731
    rho_u, rho_d, drho_u, drho_d = rho_u.contiguous(), rho_d.contiguous(), drho_u.contiguous(), drho_d.contiguous()
    grho_u, grho_d, dgrho_u, dgrho_d = c(grho_u), c(grho_d), c(dgrho_u), c(dgrho_d)
    dvu, dvd = torch.empty_like(drho_u), torch.empty_like(drho_u)
    dgu = torch.empty((nvec, 3, n), dtype=torch.float64, device=rho_u.device) if gga else None
    dgd = torch.empty((nvec, 3, n), dtype=torch.float64, device=rho_u.device) if gga else None
    with _on(rho_u.device) as st_:
        _check(load().dqc_xc_eval_fxc_pol(_ptr(dvu), _ptr(dvd), _ptr(dgu), _ptr(dgd), _ptr(rho_u), _ptr(rho_d), _ptr(grho_u), _ptr(grho_d),
                                          _ptr(drho_u), _ptr(drho_d), _ptr(dgrho_u), _ptr(dgrho_d), n, nvec, ids, cfs, len(terms), st_),
               "dqc_xc_eval_fxc_pol")
    return (dvu, dvd), (dgu, dgd)


def xc_eval_mgga(terms, rho, grho, tau, want_e=True, want_v=True):
    """-> edens, vrho, vgrad (3,n), vtau"""
    n = rho.shape[0]
    ids = (ctypes.c_int * len(terms))(*[XC_IDS[nm] for _, nm in terms])
    cfs = (ctypes.c_double * len(terms))(*[float(c) for c, _ in terms])
    e = torch.empty_like(rho) if want_e else None
    v = torch.empty_like(rho) if want_v else None
    vg = torch.empty((3, n), dtype=torch.float64, device=rho.device) if want_v else None
    vt = torch.empty_like(rho) if want_v else None
    with _on(rho.device) as st_:
        _check(load().dqc_xc_eval_mgga(_ptr(e), _ptr(v), _ptr(vg), _ptr(vt), _ptr(rho), _ptr(grho), _ptr(tau), n, ids, cfs,
                                       len(terms), st_), "dqc_xc_eval_mgga")
    return e, v, vg, vt


def xc_eval_mgga_pol(terms, rho_u, rho_d, grho_u, grho_d, tau_u, tau_d, want_e=True, want_v=True):
    """spin-polarised meta-GGA correlation terms -> edens, (vrho_u, vrho_d), vgrad (3,n) shared by both spins, vtau shared"""
    n = rho_u.shape[0]
    ids = (ctypes.c_int * len(terms))(*[XC_IDS[nm] for _, nm in terms])
    cfs = (ctypes.c_double * len(terms))(*[float(c) for c, _ in terms])
    e = torch.empty_like(rho_u) if want_e else None
    vu = torch.empty_like(rho_u) if want_v else None
    vd = torch.empty_like(rho_u) if want_v else None
    vg = torch.empty((3, n), dtype=torch.float64, device=rho_u.device) if want_v else None
    vt = torch.empty_like(rho_u) if want_v else None
    with _on(rho_u.device) as st_:
        _check(load().dqc_xc_eval_mgga_pol(_ptr(e), _ptr(vu), _ptr(vd), _ptr(vg), _ptr(vt), _ptr(rho_u), _ptr(rho_d), _ptr(grho_u),
                                           _ptr(grho_d), _ptr(tau_u), _ptr(tau_d), n, ids, cfs, len(terms), st_),
               "dqc_xc_eval_mgga_pol")
    return e, (vu, vd), vg, vt


def grid_density_pair(ao_a, ao_b, nao, dm_pad):
    """sum_ij a_gi D_ij b_gj on single-component (ngrid, ld) arrays"""
    ngrid = ao_a.shape[0]
    out = torch.empty(ngrid, dtype=torch.float64, device=ao_a.device)
    with _on(ao_a.device) as st_:
        _check(load().dqc_grid_density_pair(_ptr(out), _ptr(ao_a), _ptr(ao_b), ngrid, nao, _ptr(dm_pad), st_),
               "dqc_grid_density_pair")
    return out


def grid_vxc_pair(ao_a, ao_b, nao, w, v, what="dqc_grid_vxc_pair"):
    """sym( sum_g w_g v_g a_ga b_gb ) -> (ld, ld)   (`what`: the name this call is listed under by call_trace)"""
    ngrid, ld = ao_a.shape[0], padded_nao(nao)
    vm = torch.empty((ld, ld), dtype=torch.float64, device=ao_a.device)
    unit = None if not load().dqc_get_deterministic() else _vxc_det_unit(w, v, None, _ao_envelope(ao_a), _ao_envelope(ao_b))
    if unit is not None:
        v = v * unit[1]
    with _on(ao_a.device) as st_:
        _check(load().dqc_grid_vxc_pair(_ptr(vm), _ptr(ao_a), _ptr(ao_b), ngrid, nao, _ptr(w), _ptr(v), st_), what)
    return vm if unit is None else vm.mul_(unit[0])


def _ao_envelope(ao):
    """(ngrid,) max |a| over the AO axis of an (ngrid, lda) array, over the components as well of a (ncomp, ngrid, lda) one.  One
    pass over the array, made once: the result is kept on the tensor that owns the storage (the views a caller slices off a resident
    AO array share it), per view, per stream and per version of the storage (an in-place write makes a new one).  Not kept while a
    graph is being captured (the memory would belong to the graph)."""
    owner = ao._base if ao._base is not None else ao
    key = (ao.data_ptr(), tuple(ao.shape), tuple(ao.stride()), ao._version, torch.cuda.current_stream(ao.device).cuda_stream if ao.is_cuda else 0)
    memo = owner.__dict__.setdefault("_dqc_envelope", {})
    env = memo.get(key)
    if env is None:
        env = torch.linalg.vector_norm(ao, float("inf"), dim=-1)
        env = env if env.dim() == 1 else env.amax(0)
        if not (ao.is_cuda and torch.cuda.is_current_stream_capturing()):
            if len(memo) >= 16:
                memo.clear()
            memo[key] = env
    return env


def _pow2(e):
    """2^e as a float64 tensor from the integer tensor e (|e| <= 1000), put together from the exponent bits: exact"""
    return ((e.to(torch.int64).clamp(-1000, 1000) + 1023) << 52).view(torch.float64)


def _vxc_det_unit(w, vrho, vgrad, env_a, env_b):
    """deterministic mode: (c, 1 / c) as 0-dim device tensors, c a power of two that follows THIS call's arrays -- the split-K sums of
    the Vxc kernels are fixed-point integers on the CONSTANT scale 2^47 (csrc/grid_vxc.hip), which fits sums below 2^16; the wrappers
    hand the kernels v / c and return c V[v / c] = V[v], both exact.  c comes from the bound
        |sum_g a_gi w_g (v_g b_gj + 2 sum_d vg_dg d_d b_gj)| <= B = sum_g A_g B_g |w_g| (|v_g| + 2 sum_d |vg_dg|),
    A_g, B_g the envelopes max_i |a_gi|, max_j,comp |b_gj| of the two AO operands (_ao_envelope: no pass over the AO arrays per
    call), which holds for every partial sum too: c = 2^-14 times a power of two >= B, so |V[v / c]| <= 2^14 and one addition rounds
    to 2^-61 B -- the rule of the J / K accumulators (jk_det_scale_kernel).  B is summed EXACTLY: the terms are rounded up to
    30-bit integers relative to the largest and added as int64, so c does not depend on the order of a reduction and repeats bit for
    bit; nothing is read back to the host (the call can be captured in a graph) and nothing outlives the call.  None with the
    mode off (the kernels then run on the caller's arrays as they are) and for an empty grid."""
    if w.numel() == 0 or not load().dqc_get_deterministic():
        return None
    t = vrho.abs() if vgrad is None else vrho.abs() + 2.0 * vgrad.abs().sum(0)
    t = t * w.abs() * env_a * env_b
    e = torch.frexp(t.max())[1].clamp(-1000, 1000)            # every term < 2^e (frexp(0) = (0, 0))
    total = torch.ceil(t * _pow2(30 - e)).to(torch.int64).sum()   # terms <= 2^30 each: B <= total 2^(e - 30), exact below 2^33 points
    ec = torch.frexp(total.to(torch.float64))[1] + e - 44      # total <= 2^frexp: B 2^-14 <= 2^ec
    return _pow2(ec), _pow2(-ec)


def grid_vxc(ao, nao, w, vrho, vgrad):
    """-> (ld, ld) symmetric AO-basis Vxc matrix (zero padded).  Deterministic mode: any magnitude of the potential (_vxc_det_unit)"""
    ncomp = 1 if ao.dim() == 2 else ao.shape[0]
    ngrid = ao.shape[-2]
    ld = padded_nao(nao)
    vm = torch.empty((ld, ld), dtype=torch.float64, device=ao.device)
    unit = None
    if load().dqc_get_deterministic():
        env = _ao_envelope(ao if ao.dim() == 2 else (ao[0] if vgrad is None else ao[:4]))
        unit = _vxc_det_unit(w, vrho, vgrad, env, env)
    if unit is not None:
        vrho, vgrad = vrho * unit[1], None if vgrad is None else vgrad * unit[1]
    with _on(ao.device) as st_:
        _check(load().dqc_grid_vxc(_ptr(vm), _ptr(ao), ncomp, ngrid, nao, _ptr(w), _ptr(vrho), _ptr(vgrad), st_),
               "dqc_grid_vxc" if vgrad is not None else "dqc_grid_vxc[no gradient term]")
    return vm if unit is None else vm.mul_(unit[0])


class PartitionStream:
    """a HIP stream whose kernels run on compute units [cu_begin, cu_end) of every XCD only (dqc_stream_create_partition), wrapped
    as a torch stream (`.stream`) so that `with torch.cuda.stream(p.stream)` sends library calls and torch ops to it"""

    def __init__(self, device, cu_begin, cu_end):
        dev = torch.device(device)
        dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.device = dev
        self.cu_begin, self.cu_end = int(cu_begin), int(cu_end)
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _check(load().dqc_stream_create_partition(ctypes.byref(h), self.cu_begin, self.cu_end, 0), "dqc_stream_create_partition")
            self.cus = int(load().dqc_stream_cus(h))
        self._handle = h
        self.stream = torch.cuda.ExternalStream(h.value, device=dev)

    def close(self):
        """hand the stream back to the process-wide pool (partition_stream): PyTorch's caching allocator keeps events and block
        records that name a stream for as long as the process lives, so a stream it has seen is never destroyed"""
        if self._handle is not None:
            self.stream.synchronize()
            _PART_POOL.setdefault((self.device.index, self.cu_begin, self.cu_end), []).append(self)


_PART_POOL = {}


def partition_stream(device, cu_begin, cu_end):
    """a PartitionStream from the pool of closed ones, or a new one"""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    free = _PART_POOL.get((idx, int(cu_begin), int(cu_end)))
    if free:
        return free.pop()
    return PartitionStream(torch.device("cuda", idx), cu_begin, cu_end)


def set_vxc_cus(ncu):
    """cap on the CUs the one-block-per-CU Vxc kernels occupy (0: none); returns the previous setting"""
    return int(load().dqc_set_vxc_cus(int(ncu)))


def device_cu_count(device=None):
    with torch.cuda.device(device):
        return int(load().dqc_device_cu_count())


def grid_vxc_raw(ao, nao, w, vrho, vgrad):
    """dqc_grid_vxc without the closing symmetrisation launch -> (raw (ld, ld) cross-block sums, their fixed-point scale or 0.0);
    for fock_finish.  Deterministic mode: the scale is the constant 2^47 and the potential is summed as it is -- right for matrices
    with elements of order one (v_xc on normalised AOs), not for arbitrary magnitudes: those go through grid_vxc (set_deterministic)"""
    ncomp = 1 if ao.dim() == 2 else ao.shape[0]
    ngrid = ao.shape[-2]
    ld = padded_nao(nao)
    vm = torch.empty((ld, ld), dtype=torch.float64, device=ao.device)
    sc = ctypes.c_double(0.0)
    with _on(ao.device) as st_:
        _check(load().dqc_grid_vxc_raw(_ptr(vm), _ptr(ao), ncomp, ngrid, nao, _ptr(w), _ptr(vrho), _ptr(vgrad), ctypes.byref(sc), st_),
               "dqc_grid_vxc" if vgrad is not None else "dqc_grid_vxc[no gradient term]")
    return vm, float(sc.value)


def resp_kappa2dm(kappa, cv, co, scale):
    """kappa (nvec, nv, no), C_v (nao, nv), C_o (nao, no) -> dD (nvec, nao, nao) = scale (C_v kappa C_o^T + transpose), two launches"""
    nvec, nv, no = kappa.shape
    nao = cv.shape[0]
    dm = torch.empty((nvec, nao, nao), dtype=torch.float64, device=kappa.device)
    t = torch.empty((nvec, nao, no), dtype=torch.float64, device=kappa.device)
    with _on(kappa.device) as st_:
        _check(load().dqc_resp_kappa2dm(_ptr(dm), _ptr(t), _ptr(kappa.contiguous()), _ptr(cv), _ptr(co), nao, nv, no, nvec, float(scale), st_),
               "dqc_resp_kappa2dm")
    return dm


def resp_kappa2dm_pm(kappa, cv, co, scale, plus=True, minus=True):
    """-> (dD+, dD-) = scale (C_v kappa C_o^T +- transpose), each (nvec, nao, nao) or None when not asked for: one half-transformation
    C_v kappa and one launch per output"""
    nvec, nv, no = kappa.shape
    nao = cv.shape[0]
    dp = torch.empty((nvec, nao, nao), dtype=torch.float64, device=kappa.device) if plus else None
    dm = torch.empty((nvec, nao, nao), dtype=torch.float64, device=kappa.device) if minus else None
    t = torch.empty((nvec, nao, no), dtype=torch.float64, device=kappa.device)
    with _on(kappa.device) as st_:
        _check(load().dqc_resp_kappa2dm_pm(_ptr(dp), _ptr(dm), _ptr(t), _ptr(kappa.contiguous()), _ptr(cv), _ptr(co), nao, nv, no, nvec,
                                           float(scale), st_), "dqc_resp_kappa2dm_pm")
    return dp, dm


def resp_project(g, cv, co, alpha, ev=None, eo=None, kappa=None):
    """g (nvec, nao, nao) -> alpha (C_v^T g[v] C_o) (nvec, nv, no), plus alpha (ev[a] - eo[i]) kappa[v][a][i] when kappa is given: two
    launches (U = g C_o, then the projection with the diagonal term in its epilogue)"""
    nvec, nao = g.shape[0], g.shape[1]
    nv, no = cv.shape[1], co.shape[1]
    u = torch.empty((nvec, nao, no), dtype=torch.float64, device=g.device)
    out = torch.empty((nvec, nv, no), dtype=torch.float64, device=g.device)
    g = g.contiguous()
    with _on(g.device) as st_:
        _check(load().dqc_resp_gemm(_ptr(u), _ptr(g), _ptr(co), nao, no, nao, nao, no, no, nao * nao, 0, nao * no, 0, nvec, 1.0, None, None,
                                    None, st_), "dqc_resp_gemm[G C_o]")
    with _on(g.device) as st_:
        _check(load().dqc_resp_gemm(_ptr(out), _ptr(cv), _ptr(u), nv, no, nao, nv, no, no, 0, nao * no, nv * no, 1, nvec, float(alpha),
                                    _ptr(ev), _ptr(eo), _ptr(None if kappa is None else kappa.contiguous()), st_), "dqc_resp_gemm[C_v^T U]")
    return out


def probe_stream_read(buf):
    out = torch.zeros(1, dtype=torch.float64, device=buf.device)
    with _on(buf.device) as st_:
        _check(load().dqc_probe_stream_read(_ptr(buf), buf.numel(), _ptr(out), st_), "dqc_probe_stream_read")
    return out


def probe_rys(variant, n, x):
    """the integral kernels' own root / weight lookups at the arguments x (float64 device vector): (u, w), each (len(x), n) --
    variant 0 rys_roots, 1 rys_root1, 2 rys_root1_lds, 3 rys_root1_rt; variant 4 (n = 1): boys01_lds, u = F_0, w = F_1
    (include/dqc_amd.h: dqc_probe_rys)"""
    x = x.contiguous()
    u = torch.empty((x.numel(), max(int(n), 0)), dtype=torch.float64, device=x.device)
    w = torch.empty_like(u)
    with _on(x.device) as st_:
        _check(load().dqc_probe_rys(int(variant), int(n), _ptr(x), x.numel(), _ptr(u), _ptr(w), st_), "dqc_probe_rys")
    return u, w


def probe_mfma_f64_tflops(device, iters=4000):
    """measured fp64 MFMA ceiling of this GPU (TFLOP/s): 2048 waves x 8 independent accumulators"""
    out = torch.empty(512 * 256, dtype=torch.float64, device=device)
    L = load()
    with _on(device) as st_:
        _check(L.dqc_probe_mfma_f64(_ptr(out), 100, st_), "dqc_probe_mfma_f64")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    with _on(device) as st_:
        _check(L.dqc_probe_mfma_f64(_ptr(out), iters, st_), "dqc_probe_mfma_f64")
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * 16 * 16 * 4 * 8 * iters * 2048 / (e0.elapsed_time(e1) * 1e-3) / 1e12


def probe_hbm_read_gbs(device, nbytes=2 << 30):
    """measured streaming-read bandwidth (GB/s) over a buffer larger than the Infinity Cache"""
    buf = torch.empty(nbytes // 8, dtype=torch.float64, device=device).normal_()
    for _ in range(5):  # (the first launches after an idle spell run at a lower clock: 6.05 then 6.25 TB/s)
        probe_stream_read(buf)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        probe_stream_read(buf)
    e1.record()
    torch.cuda.synchronize()
    return 10.0 * nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9
