"""The converged SCF energy as a torch.autograd node: `torch.autograd.grad(qc.energy(), x)` for the inputs the reference
differentiates (dqc/test/test_hf.py:82-111, test_ks.py:117-240, examples/03-alchemy-gradient.py).

The SCF itself runs on detached values (dqc_amd.system.Mol keeps the caller's tensors aside).  At the converged density every
first derivative is a Hellmann-Feynman (+ Pulay) expression -- no response equations:

    atompos          dE/dR                                   dqc_amd.gradient.nuclear_gradient
    efield[0]  (3)   Tr(D r_d)                               multipole integrals r0
    efield[1]  (9)   1/2 Tr(D r_d r_e)                       r0r0 (the 1/n! of the field term, hamilton.py)
    vext             w_g rho(r_g), zero on pruned points     the density on the grid
    XC parameters    sum_g w_g d e_xc(rho_g; p) / dp         torch autograd of get_edensityxc at fixed rho
    atomzs           -V_C + sum_B Z_B / R_CB + dE/dN         dqc_int1e_potential at the nuclei; dE/dN: Janak, below
    orb_weights      eps_i of each channel (Janak)           eigenvalues of the converged Fock matrix
    basis            dE/d alpha_p, dE/d c_p (Pulay terms)    dqc_amd.gradient.basis_gradient, chained through wfnormalize_

dE/dN routes the derivative of the occupation numbers to orbital ceil(n) - 1 of each spin channel, as the reference's
occnumber backward does (dqc/utils/safeops.py:75-77).  Derivatives of derivatives are not provided: a backward with
create_graph=True raises (properties.hessian_pos gives second derivatives by finite differences)."""
import math
import warnings

import torch

from . import lib


def grad_inputs(qc):
    """(kinds, tensors): the caller's tensors the energy of `qc` depends on -- positions, floating-point charges, every efield
    element, vext, user orb_weights (u, d), the basis table's exponents and normalised coefficients (functions of the caller's
    CGTOBasis tensors, when one of them requires grad) and the parameters of a torch.nn.Module functional"""
    eng = qc._engine
    leaves = getattr(eng.get_system(), "_grad_leaves", {})
    kinds, tensors = [], []
    for key in ("atompos", "atomzs", "vext"):
        if key in leaves:
            kinds.append((key,))
            tensors.append(leaves[key])
    for i, ef in enumerate(leaves.get("efield", ())):
        if isinstance(ef, torch.Tensor):
            kinds.append(("efield", i))
            tensors.append(ef)
    if "orb_weights" in leaves:
        for s, w in enumerate(leaves["orb_weights"]):
            kinds.append(("orb_weights", s))
            tensors.append(w)
    if "basis" in leaves:
        # the table's exponents and normalised coefficients as torch functions of the caller's CGTOBasis tensors: autograd carries
        # dE/d(table rows) (gradient.basis_gradient) through the normalisation to the leaves and sums shared tensors
        from .basis import table_parameters
        for i, t in enumerate(table_parameters(eng.get_system()._basis_shells)):
            kinds.append(("basis", i))
            tensors.append(t)
    if eng.is_ks and isinstance(eng.xc, torch.nn.Module):
        for k, p in enumerate(eng.xc.parameters()):
            kinds.append(("xc", k))
            tensors.append(p)
    return kinds, tensors


class _SCFEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, qc, kinds, *leaves):
        ctx.qc, ctx.kinds = qc, kinds
        ctx.meta = [(t.shape, t.dtype, t.device) for t in leaves]
        return e.clone()

    @staticmethod
    def backward(ctx, grad_e):
        if torch.is_grad_enabled():
            raise NotImplementedError("the SCF energy has first derivatives only (no create_graph=True backward); second "
                                      "derivatives by finite differences: dqc_amd.properties.hessian_pos")
        need = ctx.needs_input_grad[3:]
        ders = energy_derivatives(ctx.qc, [k for k, n in zip(ctx.kinds, need) if n])
        out = []
        for k, n, (shape, dtype, device) in zip(ctx.kinds, need, ctx.meta):
            if not n:
                out.append(None)
                continue
            d = ders[k].to(device=grad_e.device, dtype=torch.float64)
            out.append((grad_e * d).reshape(shape).to(device=device, dtype=dtype))
        return (None, None, None) + tuple(out)


def energy(qc, e):
    """e (the detached converged energy) -> e itself when nothing is differentiated, else the autograd node"""
    if not torch.is_grad_enabled():
        return e
    kinds, tensors = grad_inputs(qc)
    if not any(t.requires_grad for t in tensors):
        return e
    return _SCFEnergy.apply(e.detach(), qc, kinds, *tensors)


def _eigvals(eng, fock):
    return eng._eigpairs(fock)[0]


def _occ_index(a, n):
    """the orbital the occupation derivative of `a` electrons goes to: ceil(a) - 1 (torch indexing: -1 is the last of `n`)"""
    k = int(math.ceil(a - 1e-12)) - 1
    return k + n if k < 0 else k


def energy_derivatives(qc, kinds):
    """{kind: dE/d(input)} (flat float64 tensors) for the requested kinds, at the converged density of `qc`"""
    from .gradient import nuclear_gradient
    from .properties import _total_ao_density
    eng = qc._engine
    h = eng.hamilton
    mol = eng.get_system()
    pol = eng.polarized
    if not getattr(qc, "accepted", False):
        warnings.warn("derivatives of an unconverged SCF energy (max|[F,D]| = %.2e) are not the derivatives of that energy"
                      % qc.scf_error)
    out = {}
    dao = None
    eps = None

    def ao_density():
        nonlocal dao
        if dao is None:
            dao = _total_ao_density(qc)[1]
            dao = (dao + dao.transpose(-2, -1)) * 0.5
        return dao

    def eigenvalues():  # (eps_u, eps_d) of the converged Fock matrices (the same array twice when restricted)
        nonlocal eps
        if eps is None:
            eps = (_eigvals(eng, qc._fock[0]), _eigvals(eng, qc._fock[1])) if pol else (_eigvals(eng, qc._fock),) * 2
        return eps

    for k in kinds:
        what = k[0]
        if what == "atompos":
            with torch.enable_grad():  # (the Becke-weight term of the XC gradient is itself a torch autograd pass)
                out[k] = nuclear_gradient(qc).reshape(-1)
        elif what == "efield":
            if k[1] > 1:
                raise NotImplementedError("energy derivatives by efield elements beyond the field gradient are not implemented")
            mats = lib.int1e("r0" * (k[1] + 1), h._tab, h.device)
            out[k] = torch.einsum("dab,ab->d", mats, ao_density()) / math.factorial(k[1] + 1)
        elif what == "vext":
            if getattr(h, "sharded", False):
                raise NotImplementedError("vext derivatives of a Hamiltonian sharded over several GPUs are not implemented")
            tot = qc._dm.u + qc._dm.d if pol else qc._dm
            wrho = h._dm2densinfo(tot).value * h.dvolume
            n = mol._grad_leaves["vext"].shape[-1]
            out[k] = h.grid_scatter(wrho) if n == h.ngrid_full else wrho
        elif what == "xc":
            if getattr(h, "sharded", False):
                raise NotImplementedError("XC-parameter derivatives of a Hamiltonian sharded over several GPUs are not implemented")
            if "xc" not in out:
                dens = h._dm2densinfo_pol(qc._dm) if pol else h._dm2densinfo(qc._dm)
                params = list(eng.xc.parameters())
                live = [p for p in params if p.requires_grad]
                with torch.enable_grad():
                    exc = torch.sum(h.dvolume * eng.xc.get_edensityxc(dens))
                    gs = torch.autograd.grad(exc, live, allow_unused=True) if live else []
                gmap = {id(p): g for p, g in zip(live, gs)}
                out["xc"] = [gmap.get(id(p)) if gmap.get(id(p)) is not None else torch.zeros_like(p) for p in params]
            out[k] = out["xc"][k[1]].detach().reshape(-1)
        elif what == "atomzs":
            T = lib.cart2sph_matrix(h._tab, h.device)
            pos = mol.atompos.to(device=h.device, dtype=torch.float64)
            v = lib.int1e_potential((T.T @ ao_density() @ T).contiguous(), pos, h._tab)
            z = mol.atomzs.to(device=h.device, dtype=torch.float64)
            r = torch.cdist(pos, pos)
            inv = torch.where(r > 0, 1.0 / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(r))
            d = -v + inv @ z
            if getattr(mol, "_user_weights", None) is None:
                # N = sum Z - charge at fixed charge and spin: n_up and n_dn each move by 1/2 per unit of Z
                eu, ed = eigenvalues()
                wts = eng.orb_weight
                nu, nd = (wts.u.numel(), wts.d.numel()) if pol else (wts.numel(), wts.numel())
                d = d + 0.5 * (eu[_occ_index(mol._nup, nu)] + ed[_occ_index(mol._ndn, nd)])
            out[k] = d
        elif what == "basis":
            if "basis" not in out:
                from .gradient import basis_gradient
                out["basis"] = basis_gradient(qc)                 # (nprim_total, 2): by alpha_p, by the normalised c_p
            out[k] = out["basis"][:, k[1]]
        elif what == "orb_weights":
            eu, ed = eigenvalues()
            e_s = eu if k[1] == 0 else ed
            n = mol._grad_leaves["orb_weights"][k[1]].numel()
            out[k] = e_s[:n]
        else:
            raise KeyError(k)
    return out
