"""dqc_amd -- MI355X (gfx950) native SCF Fock-build engine behind DQC's Hamiltonian API.

Public names mirror the reference's top-level API (dqc/__init__.py:1-3)."""
from .utils.datastruct import CGTOBasis, AtomCGTOBasis, SpinParam, ValGrad, DensityFitInfo  # noqa: F401
from .basis import loadbasis, parse_moldesc  # noqa: F401
from .xc import get_xc, BaseXC, LibXC  # noqa: F401
from .hamilton import HamiltonMI355  # noqa: F401
from .system import Mol  # noqa: F401
from .qccalc import HF, KS  # noqa: F401
from .grid import get_grid, get_predefined_grid  # noqa: F401
from .properties import edipole, equadrupole, optimal_geometry, hessian_pos, vibration, ir_spectrum, raman_spectrum  # noqa: F401
from .properties import lowest_eival_orb_hessian, is_orb_min, polarizability, excitations, Excitations  # noqa: F401
from .response import OrbitalHessian  # noqa: F401
from .mp2 import mp2, MP2, mp2_density, MP2Density, mp2_gradient, MP2Gradient  # noqa: F401
from .excited import excited_gradient, tddft_gradient, ExcitedGradient, ExcitedDensity  # noqa: F401
from .rpa import rpa, RPA  # noqa: F401
from .gw import gw, GW  # noqa: F401
from .bse import bse, BSE  # noqa: F401
from .ccsd import ccsd, CCSD  # noqa: F401

__version__ = "0.1.0"
