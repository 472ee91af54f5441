"""-pynama_direct_band / -pynama_direct_band_max_gb reach the solver facade (no GPU needed: nothing is solved)."""
from pynama_amd.common.options import Options
from pynama_amd.solver.ksp_solver import KspSolver


def test_direct_band_options_host():
    try:
        Options([])
        k = KspSolver()
        k.createSolver(None, None)
        assert (k.ksp_type, k.pc_type, k.direct_band, k.direct_band_max_gb) == ("preonly", "lu", False, 16.0)
        Options(["-pynama_direct_band", "-pynama_direct_band_max_gb", "2.5"])
        k = KspSolver()
        k.createSolver(None, None)
        assert (k.direct_band, k.direct_band_max_gb) == (True, 2.5)
        Options(["-pynama_direct_band", "0"])
        k = KspSolver()
        k.createSolver(None, None)
        assert k.direct_band is False
    finally:
        Options([])
