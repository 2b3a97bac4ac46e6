"""Nuclear gradient dE/dR of a converged SCF energy.

The reference obtains it by `torch.autograd.grad(energy, atompos)` through its "ip" derivative integrals
(dqc/hamilton/intor/molintor.py:463-500, gtoeval.py:173-193) and the implicit-function backward of the SCF fixed point
(dqc/qccalc/scf_qccalc.py:63-67, 109-113; its tests: test_hf.py:78-111, test_ks.py:114-137).  At the fixed point the
same derivative is the Hellmann-Feynman + Pulay expression -- no response equations:

    dE/dR_A = sum D dh/dR_A - sum W dS/dR_A                      one-electron terms      -> dqc_int1e_grad
            + sum (d_A a b|c d) [2 j D_ab D_cd - k D_ac D_bd]     two-electron term       -> dqc_eri_grad / dqc_df_grad
            + dE_xc/dR_A                                           LDA and GGA, INCLUDING the grid response
            + dE_nn/dR_A

Restricted and unrestricted (UHF / UKS: J from the total density, exchange and XC spin by spin); hybrid functionals scale the
exchange part of the two-electron term by their exact-exchange fraction (k = a).  The XC part
differentiates the discretised functional E_xc = sum_g w_g(R) e(rho_s(r_g(R))) exactly, as the reference's autograd does:
(i) Becke-weight derivative (torch autograd through dqc_amd.grid's own weight code, e_g held fixed), and for every spin,
with b = Phi D_s, c_i = d_i Phi D_s, u = the gradient part of the potential (`vgrad` of dqc_xc_eval*), S_j = sum_i u_i d_i d_j Phi:
(ii)  grid points riding on atom A:  sum_{g in A} w [v_rho d_j rho + 2 sum_mu (b S_j + c_j (u . grad phi))]
(iii) centres of the AOs on A:       -2 sum_g w sum_{mu in A} [d_j phi (v_rho b + u . c) + b S_j]
((ii) + (iii) summed over atoms cancel identically; LDA: u = 0; meta-GGA: the tau terms).  (ii) and (iii) are _xc_grid_terms, for the
ground state (_xc_gradient) and for any other matrix and potentials (_xc_potential_gradient); (i) is _xc_weight_gradient.  With
density fitting the two-electron term is _df_coulomb_gradient (dqc_df_grad).
"""
import torch

from . import lib
from .grid import get_predefined_grid
from .utils.datastruct import SpinParam

_HESS = ((4, 5, 6), (5, 7, 8), (6, 8, 9))  # component of d2/(d i d j) in the deriv-3 AO array


def nuclear_gradient(qc) -> torch.Tensor:
    """qc: a converged dqc_amd.HF / dqc_amd.KS.  Returns dE/dR, shape (natm, 3), Hartree / Bohr."""
    eng = qc._engine
    h = eng.hamilton
    mol = eng.get_system()
    dev = h.device
    ef = getattr(h, "_efield", None)
    if ef is not None and any(bool((e != 0).any()) for e in ef):
        # an all-zero field (the reference's property fixture attaches zeros so that autograd has a leaf) adds nothing
        raise NotImplementedError("nuclear gradients in a non-zero electric field are not implemented (derivative multipole "
                                  "integrals)")
    if getattr(h, "sharded", False):
        raise NotImplementedError("nuclear gradients of a Hamiltonian sharded over several GPUs (shard_over) are not implemented: "
                                  "the grid terms need the whole grid")
    if h._vext is not None:
        raise NotImplementedError("nuclear gradients with an external potential are not implemented: the vext term "
                                  "(grid points and basis centres moving in vext) is missing from dqc_amd.gradient")
    if h.df is not None and h.df.exchange and (not eng.is_ks or getattr(eng, "exx", 0.0) != 0.0):
        raise NotImplementedError("nuclear gradients with fitted exchange (densityfit(exchange=True)) are not implemented: the K "
                                  "term needs the derivative three-index integrals contracted with a three-index density, "
                                  "which is not built")
    d_aos, d_tot, w_ao = _pulay_densities(qc)
    T = lib.cart2sph_matrix(h._tab, dev)                                        # (nao, ncart)
    tocart = lambda m: (T.T @ m @ T).contiguous()  # noqa: E731
    natm = len(mol.atomzs)
    grad = torch.zeros((natm, 3), dtype=torch.float64, device=dev)
    lib.int1e_grad(grad, tocart(d_tot), tocart(w_ao), h._tab, h._zs)
    if h.df is not None:
        _df_coulomb_gradient(h, d_tot, grad)
    else:
        _two_electron_terms(lib.eri_grad, eng, grad, d_tot, d_aos, tocart, h._tab)
    if eng.is_ks:
        grad = grad + _xc_gradient(eng, d_aos)
    return grad + _nuclei_gradient(mol).to(dev)


def _pulay_densities(qc):
    """([D_s], D, W): the symmetrised AO densities spin by spin, their sum and the energy-weighted density of a converged run"""
    eng = qc._engine
    h = eng.hamilton
    X = h._orthozer
    pol = eng.polarized
    dms = [qc._dm.u, qc._dm.d] if pol else [qc._dm]
    focks = [qc._fock[0], qc._fock[1]] if pol else [qc._fock]
    weights = [eng.orb_weight.u, eng.orb_weight.d] if pol else [eng.orb_weight]
    norbs = [eng.norb.u, eng.norb.d] if pol else [eng.norb]
    d_aos, w_ao = [], 0.0
    for dm, fock, w, n in zip(dms, focks, weights, norbs):
        # (the shortcut below needs D = w0 P with P commuting with F: an ACCEPTED fixed point with equal, non-zero occupations --
        # a run that only warned keeps the energy-weighted density of the final Fock matrix's own orbitals; the flag is cached on
        # the engine: it reads the device)
        cache = eng.__dict__.setdefault("_uniform_occ_cache", {})
        if id(w) not in cache:  # (the occupation tensors live as long as the engine)
            cache[id(w)] = bool(w.numel() > 0 and bool((w == w[0]).all()) and float(w[0]) > 0.0)
        uniform = cache[id(w)] and getattr(eng, "_sinvh", None) is None and bool(getattr(qc, "accepted", False))
        if uniform:
            # equal occupations w0 in an orthonormal basis: D = w0 P with P the projector on the occupied space, and at the fixed
            # point sum_i w0 eps_i c_i c_i^T = w0 P F P = D F D / w0 -- no diagonalisation (a 208 x 208 eigh was 3 ms of the gradient)
            fs = (fock + fock.T) * 0.5
            w_ao = w_ao + X @ ((dm @ fs @ dm) / w[0]) @ X.T
        else:
            eps, C = eng._eigpairs(fock)  # generalised problem when the basis is not orthogonalised
            Cocc = C[:, :n]
            w_ao = w_ao + X @ ((Cocc * (w * eps[:n]).unsqueeze(0)) @ Cocc.T) @ X.T     # energy-weighted density
        d = X @ dm @ X.T
        d_aos.append((d + d.T) * 0.5)
    return d_aos, sum(d_aos), w_ao


def _two_electron_terms(contract, eng, out, d_tot, d_aos, tocart, tab):
    """the j / k cases of the exact two-electron term; contract = lib.eri_grad (out (natm, 3)) or lib.eri_grad_basis (out
    (nprim, 2)): out += sum (d a b|c d) [2 j D_ab D_cd - k D_ac D_bd]"""
    pol = eng.polarized
    if eng.is_ks and getattr(eng, "exx", 0.0) != 0.0:
        # hybrid functional, exact-exchange fraction a: the Hartree-Fock two-electron term with the exchange scaled by a
        a = float(eng.exx)
        if not pol:
            contract(out, tocart(d_tot), a, tab)
        else:  # J from the total density, -a K[D_s] spin by spin
            contract(out, tocart(d_tot), 0.0, tab)
            for d in d_aos:
                contract(out, tocart(d), 2.0 * a, tab, jscale=0.0)
    elif eng.is_ks:
        contract(out, tocart(d_tot), 0.0, tab)
    elif not pol:
        contract(out, tocart(d_tot), 1.0, tab)
    else:  # UHF: J from the total density, -K[D_s] spin by spin  (E_K = -1/2 sum_s sum D^s_ac D^s_bd (ab|cd))
        contract(out, tocart(d_tot), 0.0, tab)
        for d in d_aos:
            contract(out, tocart(d), 2.0, tab, jscale=0.0)


def basis_gradient(qc) -> torch.Tensor:
    """qc: a converged dqc_amd.HF / dqc_amd.KS.  Returns dE/d(basis parameters), shape (nprim_total, 2): one row per primitive of
    the Hamiltonian's table (dqc_amd.basis.make_tables order, shell by shell), column 0 by the exponent alpha_p, column 1 by the
    stored, normalised coefficient c_p.  The Pulay expression of nuclear_gradient with d/dR_A replaced by d/dtheta:

        dE/dtheta = 2 sum_{a has p} sum_b [D_ab (d_theta a|T+V|b) - W_ab (d_theta a|b)]       -> dqc_int1e_grad_basis
                  +   sum_{a has p} sum_bcd (d_theta a b|c d) [2 j D_ab D_cd - k D_ac D_bd]   -> dqc_eri_grad_basis
                  +   dE_xc/dtheta at fixed AO density                                        -> _xc_basis_gradient

    (no operator, Becke-weight or E_nn term: neither the nuclei nor the grid depend on the basis).  Orbital shells up to f."""
    from .basis import primitive_rows
    eng = qc._engine
    h = eng.hamilton
    dev = h.device
    if h.df is not None:
        raise NotImplementedError("basis-parameter gradients of a density-fitted Hamiltonian are not implemented: the fitted "
                                  "Coulomb / exchange energies need the derivative three-index integrals by exponent and coefficient")
    if getattr(h, "sharded", False):
        raise NotImplementedError("basis-parameter gradients of a Hamiltonian sharded over several GPUs (shard_over) are not "
                                  "implemented: the XC term needs the whole grid")
    ef = getattr(h, "_efield", None)
    if ef is not None and any(bool((e != 0).any()) for e in ef):
        raise NotImplementedError("basis-parameter gradients in a non-zero electric field are not implemented (multipole integrals "
                                  "differentiated by exponent and coefficient)")
    if h._vext is not None:
        raise NotImplementedError("basis-parameter gradients with an external potential are not implemented: the vext term "
                                  "(sum_g w vext d rho / d theta) is missing from dqc_amd.gradient")
    if int(h._tab.bas[:, 1].max()) > 3:
        raise NotImplementedError("basis-parameter gradients support orbital shells up to f: the exponent derivative of a g shell "
                                  "is an l + 2 = i shell, above the h limit of the integral kernels")
    if eng.is_ks and h.xcfamily >= 4:
        raise NotImplementedError("basis-parameter gradients of meta-GGA functionals are not implemented (the tau term of dE_xc/dtheta)")
    d_aos, d_tot, w_ao = _pulay_densities(qc)
    T = lib.cart2sph_matrix(h._tab, dev)                                        # (nao, ncart)
    tocart = lambda m: (T.T @ m @ T).contiguous()  # noqa: E731
    nprim = primitive_rows(h._tab.bas)[0].shape[0]
    out = torch.zeros((nprim, 2), dtype=torch.float64, device=dev)
    lib.int1e_grad_basis(out, tocart(d_tot), tocart(w_ao), h._tab, h._zs)
    _two_electron_terms(lib.eri_grad_basis, eng, out, d_tot, d_aos, tocart, h._tab)
    if eng.is_ks:
        out = out + _xc_basis_gradient(h, d_aos)
    return out


_XC_BASIS_CHUNK = 1 << 16  # grid points per pass of _xc_basis_gradient (bounds the per-primitive AO arrays)


def _xc_basis_gradient(h, d_aos):
    """dE_xc/dtheta_p = 2 sum_g w sum_{mu in shell(p)} [chi_mu (v_rho b_mu + u . c_mu) + b_mu u . grad chi_mu],  chi = d_theta phi_mu,
    at fixed AO density (b, c, u, v_rho as in _xc_gradient; LDA: u = 0); LDA and GGA, spin by spin.  chi comes from dqc_eval_gto on
    the table that lists every primitive as its own shell (dqc_amd.basis.companion_tables):
        chi_c = phi_prim,    chi_alpha = -c_p r_A^2 phi_prim,    grad chi_alpha = -c_p (2 (r - A) phi_prim + r_A^2 grad phi_prim)."""
    from .basis import companion_tables, primitive_rows
    from .utils.datastruct import ValGrad
    dev = h.device
    nao, ld = h._nao_ao, h._ld
    gga = h.xcfamily >= 2
    tab = h._tab
    prim_shell, _ = primitive_rows(tab.bas)
    nprim = prim_shell.shape[0]
    catm, cbas, cenv = companion_tables(tab.atm, tab.bas, tab.env)
    ptab = lib.Tables(catm, cbas[:nprim], cenv)                               # the primitives themselves (same l, coefficient 1)
    ao_off = [0]
    for b in tab.bas:
        ao_off.append(ao_off[-1] + 2 * int(b[1]) + 1)
    col_ao, col_prim, col_atom = [], [], []  # per column of the primitive table: the AO it belongs to, its primitive, its atom
    for p, ish in enumerate(prim_shell.tolist()):
        ns = 2 * int(tab.bas[ish, 1]) + 1
        col_ao.extend(range(ao_off[ish], ao_off[ish] + ns))
        col_prim.extend([p] * ns)
        col_atom.extend([int(tab.bas[ish, 0])] * ns)
    col_ao, col_prim, col_atom = (torch.tensor(x, device=dev) for x in (col_ao, col_prim, col_atom))
    ncol = col_ao.numel()
    coef = torch.as_tensor([tab.env[int(tab.bas[ish, 6]) + k] for ish in range(tab.nbas) for k in range(int(tab.bas[ish, 2]))],
                           dtype=torch.float64, device=dev)
    pos = torch.as_tensor(tab.env[tab.atm[:, 1, None] + [0, 1, 2]], dtype=torch.float64, device=dev)          # (natm, 3)
    dpads = [lib.pad_matrix(d, ld) for d in d_aos]
    col_c = torch.zeros(ncol, dtype=torch.float64, device=dev)
    col_a = torch.zeros(ncol, dtype=torch.float64, device=dev)
    for g0 in range(0, h.rgrid.shape[0], _XC_BASIS_CHUNK):
        pts = h.rgrid[g0:g0 + _XC_BASIS_CHUNK].contiguous()
        w = h.dvolume[g0:g0 + _XC_BASIS_CHUNK]
        ao = lib.eval_gto(tab, pts, 1)                                         # (4, n, lda)
        lda = ao.shape[-1]
        infos, bs, cs_ = [], [], []
        for dp in dpads:
            rho_s, grho_s = lib.grid_density(ao, nao, dp, True)
            dq = dp[:lda, :lda]
            bs.append(ao[0] @ dq)
            cs_.append([ao[1 + i] @ dq for i in range(3)] if gga else None)
            infos.append(ValGrad(value=rho_s, grad=grho_s if gga else None))
        dens = infos[0] if len(infos) == 1 else SpinParam(u=infos[0], d=infos[1])
        pot = h.xc.get_vxc(dens)
        pots = [pot] if len(infos) == 1 else [pot.u, pot.d]
        pao = lib.eval_gto(ptab, pts, 1 if gga else 0)
        phi = (pao[0] if gga else pao)[:, :ncol]                               # (n, ncol) primitive AOs
        dvec = pts.unsqueeze(1) - pos.unsqueeze(0)                             # (n, natm, 3)  r - A
        r2 = (dvec * dvec).sum(-1)[:, col_atom]                                # (n, ncol)  r_A^2
        for b, c, pt in zip(bs, cs_, pots):
            vrho, u = pt.value, pt.grad
            t1 = vrho.unsqueeze(-1) * b
            if gga:
                t1 = t1 + sum(u[i].unsqueeze(-1) * c[i] for i in range(3))
            e = phi * t1[:, col_ao]
            if gga:
                bcol = b[:, col_ao]
                e = e + bcol * sum(u[i].unsqueeze(-1) * pao[1 + i][:, :ncol] for i in range(3))
            col_c += w @ e
            ea = r2 * e
            if gga:
                ud = torch.einsum("ig,gai->ga", u, dvec)[:, col_atom]          # u . (r - A)
                ea = ea + 2.0 * bcol * ud * phi
            col_a += w @ ea
    out = torch.zeros((nprim, 2), dtype=torch.float64, device=dev)
    out[:, 1].index_add_(0, col_prim, 2.0 * col_c)
    out[:, 0].index_add_(0, col_prim, 2.0 * col_a)
    out[:, 0] *= -coef
    return out


def _df_coulomb_gradient(h, d_ao, grad):
    """density-fitted J (DFMol.get_elrep, dfmol.py:60-79):  E_J = 1/2 t^T M^-1 t  ->  sum D c d(ij|k) - 1/2 c^T dM c"""
    df = h.df
    dev = h.device
    nao, _, naux = df.j3c.shape
    t = (df.j3c.reshape(nao * nao, naux) * d_ao.reshape(-1, 1)).sum(0)        # t_k = sum_ij D_ij (ij|k)
    c = df._inv_j2c @ t
    T = lib.cart2sph_matrix(df._tab, dev)                                       # all shells: orbital, then auxiliary
    nall = T.shape[0]
    dbig = torch.zeros((nall, nall), dtype=torch.float64, device=dev)
    dbig[:nao, :nao] = d_ao
    cbig = torch.zeros(nall, dtype=torch.float64, device=dev)
    cbig[nao:] = c
    dcart = (T.T @ dbig @ T).contiguous()
    ccart = (T.T @ cbig).contiguous()
    # the concatenated table lists every atom twice (orbital parent, auxiliary parent): fold the two halves
    gbig = torch.zeros((df._tab.natm, 3), dtype=torch.float64, device=dev)
    lib.df_grad(gbig, dcart, ccart, df._tab, df._orb_range, df._aux_range)
    natm = grad.shape[0]
    grad += gbig[:natm] + gbig[natm:]


def _nuclei_gradient(mol):
    z = mol.atomzs.to(torch.float64).cpu()
    pos = mol.atompos.to(torch.float64).cpu()
    d = pos.unsqueeze(1) - pos.unsqueeze(0)                 # R_A - R_B
    r = d.norm(dim=-1) + torch.eye(len(z), dtype=torch.float64)
    f = (z.unsqueeze(1) * z.unsqueeze(0)) / r ** 3
    f = f - torch.diag(torch.diag(f))
    return -(f.unsqueeze(-1) * d).sum(1)


def _xc_gradient(eng, d_aos, fused=None):
    """d_aos: [D] (restricted) or [D_u, D_d]; LDA (deriv-1 AOs), GGA / meta-GGA (deriv-3 AOs).  The potentials come from
    the functional object itself (BaseXC.get_vxc on ValGrad / SpinParam densities), so every functional the Hamiltonian
    can run has a gradient: the terms (ii) and (iii) of the module docstring spin by spin (_xc_grid_terms; fused as it takes
    it) plus the Becke-weight term (i) on the energy density (_xc_weight_gradient)."""
    from .utils.datastruct import ValGrad
    h = eng.hamilton
    nao = h._nao_ao
    fam = h.xcfamily
    gga = fam >= 2
    ao = lib.eval_gto(h._tab, h.rgrid, 3 if gga else 1)                        # (10 | 4, ngrid, ld)
    bs, cs_, infos = [], [], []
    for d in d_aos:
        dp = lib.pad_matrix(d, h._ld)
        rho_s, grho_s = lib.grid_density(ao[:4], nao, dp, True)
        b, c = _phi_m(ao, dp, gga)
        tau = 0.5 * sum((c[i] * ao[1 + i]).sum(1) for i in range(3)) if fam == 4 else None
        bs.append(b)
        cs_.append(c)
        infos.append(ValGrad(value=rho_s, grad=grho_s if gga else None, kin=tau))
    dens = infos[0] if len(infos) == 1 else SpinParam(u=infos[0], d=infos[1])
    edens = h.xc.get_edensityxc(dens)
    pot = h.xc.get_vxc(dens)
    pots = [pot] if len(infos) == 1 else [pot.u, pot.d]
    g = sum(_xc_grid_terms(eng, ao, b, c, info.grad, pt.value, pt.grad, pt.kin if fam == 4 else None, fused)
            for info, b, c, pt in zip(infos, bs, cs_, pots))
    return g + _xc_weight_gradient(eng, edens)


def _phi_m(ao, mpad, gga):
    """(b = Phi M (ngrid, lda), c = [d_i Phi M] or None without gga) for a symmetric AO matrix M, padded by lib.pad_matrix"""
    lda = ao.shape[-1]  # row stride of the AO arrays (>= nao, zero padding columns)
    dq = mpad[:lda, :lda]
    return ao[0] @ dq, [ao[1 + i] @ dq for i in range(3)] if gga else None


def _xc_grid_terms(eng, ao, b, c, grho, vrho, u, vtau=None, fused=None):
    """The terms (ii) and (iii) of the module docstring, summed to (natm, 3), for ONE symmetric AO matrix M and ONE set of per-point
    factors: b = Phi M, c = [d_i Phi M] (None: LDA, u unused), grho = grad rho_M (3, ngrid) (None: formed here from b), vrho
    (ngrid,), u (3, ngrid), vtau (ngrid,) or None.  Meta-GGA (vtau) adds, with tau = 1/2 sum_d d_d Phi M d_d Phi:
        (ii)  + w v_tau sum_mu sum_d (d_d d_j phi_mu) c_{mu,d}        (iii)  - the same restricted to mu on A
    (v_lapl = 0 for every functional of the kernel set).  fused: None = one pass over the ten derivative arrays
    (dqc_grid_xc_gradient_terms, instead of ~40 element-wise passes) for a GGA / meta-GGA on the deriv-3 array with nao <= 512 and
    the torch passes otherwise; False forces the torch passes."""
    h = eng.hamilton
    mol = eng.get_system()
    dev = h.device
    nao = h._nao_ao
    gga = c is not None
    w = h.dvolume
    if grho is None:
        grho = torch.stack([_grad_rho(ao, b, j) for j in range(3)])
    if fused is None:
        fused = gga and ao.shape[0] == 10 and nao <= 512
    if fused:
        q, per_ao = lib.grid_xc_gradient_terms(ao, nao, b, c, w, vrho, u, grho, vtau)
    else:
        q = torch.empty((h.rgrid.shape[0], 3), dtype=torch.float64, device=dev)
        per_ao = torch.empty((nao, 3), dtype=torch.float64, device=dev)
        t1 = vrho.unsqueeze(-1) * b
        if gga:
            t1 = t1 + sum(u[i].unsqueeze(-1) * c[i] for i in range(3))
            ugphi = sum(u[i].unsqueeze(-1) * ao[1 + i] for i in range(3))      # u . grad phi
        for j in range(3):
            if gga:
                bsj = b * sum(u[i].unsqueeze(-1) * ao[_HESS[i][j]] for i in range(3))
                if vtau is not None:  # tau terms: v_tau sum_d (d_d d_j phi) c_d; same form in (ii) and (iii), without the factor 2
                    bsj = bsj + 0.5 * vtau.unsqueeze(-1) * sum(ao[_HESS[d][j]] * c[d] for d in range(3))
                q[:, j] = w * (vrho * grho[j] + 2.0 * (bsj.sum(1) + (c[j] * ugphi).sum(1)))
                per_ao[:, j] = ((ao[1 + j] * t1 + bsj) * w.unsqueeze(-1)).sum(0)[:nao]
            else:
                q[:, j] = w * vrho * grho[j]
                per_ao[:, j] = (ao[1 + j] * t1 * w.unsqueeze(-1)).sum(0)[:nao]
    g = _sum_by_owner(mol, _full_grid(h, q))                 # (ii)
    g.index_add_(0, _ao_owner(h, dev), -2.0 * per_ao)        # (iii)
    return g


def _full_grid(h, x):
    """per-point rows on the live points of the Hamiltonian (it keeps the points of non-zero weight only: setup_grid) -> rows on the
    caller's grid (zero elsewhere: zero weight, zero derivative)"""
    live = getattr(h, "live_index", None)
    if live is None:
        return x
    o = torch.zeros((h.ngrid_full,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    o[live] = x
    return o


def _xc_potential_gradient(eng, ao, m_ao, vrho, u, fused=None):
    """G(M; a, b) = sum_g w [a d rho_M + b . d grad rho_M] at fixed M (natm, 3), the AO centres and the grid points riding on their
    atoms: the terms (ii) and (iii) of the module docstring (_xc_grid_terms) for ANY symmetric AO matrix M = m_ao and ANY per-point
    pair a = vrho (ngrid,), b = u (3, ngrid) or None (LDA).  ao: the deriv-3 AO array (10, ngrid, ld) for a GGA pair, deriv-1
    (4, ngrid, ld) for LDA, evaluated once by the caller for all its calls (dqc_amd/excited.py makes three).  fused: as
    _xc_grid_terms takes it."""
    b, c = _phi_m(ao, lib.pad_matrix(m_ao, eng.hamilton._ld), u is not None)
    return _xc_grid_terms(eng, ao, b, c, None, vrho, u, None, fused)


def _xc_weight_gradient(eng, per_point):
    """sum_g (d w_g / dR) x_g (natm, 3) for a fixed per-point factor x = per_point (ngrid,) on the live points: torch autograd through
    the grid construction, the term (i) of the module docstring (_xc_gradient has the energy density as x)"""
    h = eng.hamilton
    mol = eng.get_system()
    dev = h.device
    with torch.enable_grad():  # (a caller may run under no_grad: the derivative is by the positions of this function's own copy)
        pos = mol.atompos.detach().to(dtype=torch.float64, device=dev).clone().requires_grad_(True)
        grid = get_predefined_grid(mol._grid_inp, mol.atomzs.tolist(), pos, dtype=torch.float64, device=dev)
        loss = (grid.get_dvolume() * _full_grid(h, per_point.detach())).sum()
        return torch.autograd.grad(loss, pos)[0]


def _grad_rho(ao, b, j):
    """d_j rho = 2 sum_mu (D phi)_mu d_j phi_mu"""
    return 2.0 * (b * ao[1 + j]).sum(1)


_ATOM_GRID_SIZE = {}


def _grid_sizes(mol, ngrid):
    """grid points of every atom: the atomic grids are concatenated atom by atom (dqc_amd.grid.get_grid)"""
    sizes = []
    for z in mol.atomzs.tolist():
        key = (str(mol._grid_inp), int(z))
        if key not in _ATOM_GRID_SIZE:  # the size of an atomic grid depends on the element and the grid recipe only
            one = get_predefined_grid(mol._grid_inp, [z], torch.zeros((1, 3), dtype=torch.float64), dtype=torch.float64, device="cpu")
            _ATOM_GRID_SIZE[key] = one.get_rgrid().shape[0]
        sizes.append(_ATOM_GRID_SIZE[key])
    assert sum(sizes) == ngrid
    return sizes


def _sum_by_owner(mol, q):
    """(ngrid, 3) per-point terms -> (natm, 3): every atom's points are one contiguous range (index_add_ over 350 000 rows into
    20 took 8 ms of same-address atomics)"""
    out, off = [], 0
    for n in _grid_sizes(mol, q.shape[0]):
        out.append(q[off:off + n].sum(0))
        off += n
    return torch.stack(out)


def _ao_owner(h, dev):
    out = []
    for b in h._tab.bas:
        out.extend([int(b[0])] * (2 * int(b[1]) + 1))
    return torch.tensor(out, device=dev)
