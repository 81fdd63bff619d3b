"""pyqed_amd — MI355X-native propagators behind pyqed's solver class surface.

Hot path (HIP, libqdyn.so): Lindblad RK4, ....
"""
from .deom import Bath, DEOMSolver
from .mol import LVC, LVCOp, LVCSolver, Mode, Result, load_result
from .wpd import SPO, SPO2, SPO2NH, SPO3
from .ldr import LDR2, LDR2_Jacobi, LDRN, ResultLDR, ldr_jacobi_run, ldr_run, sine_dvr
from .oqs import HEOMSolver, LindbladSolver, RedfieldSolver, glf_rk4, lindblad_rk4
from .superoperator import Lindblad_solver

__all__ = ["HEOMSolver", "Lindblad_solver", "Bath", "DEOMSolver", "SPO", "SPO2", "SPO2NH", "SPO3", "Result", "load_result", "LVC", "LVCOp", "LVCSolver", "Mode", "LindbladSolver", "RedfieldSolver", "glf_rk4", "lindblad_rk4", "LDR2", "LDRN", "ResultLDR", "ldr_run", "sine_dvr", "LDR2_Jacobi", "ldr_jacobi_run"]
__version__ = "0.1.0"
