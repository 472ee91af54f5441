"""-ksp_type cg -pc_type mg and the multigrid options reach the solver facade; gmres / preonly with mg are refused in setUp (no GPU
needed: nothing is solved)."""
import pytest

from pynama_amd import _lib
from pynama_amd.common.options import Options
from pynama_amd.solver.ksp_solver import KspSolver


def _solver(argv):
    Options(argv)
    k = KspSolver()
    k.createSolver(None, None)
    return k


def test_mg_options_host():
    try:
        k = _solver(["-ksp_type", "cg", "-pc_type", "mg"])
        assert (k.ksp_type, k.pc_type, k.mg_levels, k.mg_degree, k.mg_coarse_max_rows) == ("cg", "mg", 0, 0, 0)
        k = _solver(["-ksp_type", "cg", "-pc_type", "mg", "-pc_mg_levels", "3", "-mg_levels_ksp_max_it", "4",
                     "-pynama_mg_coarse_max_rows", "500"])
        assert (k.mg_levels, k.mg_degree, k.mg_coarse_max_rows) == (3, 4, 500)
        for ksp in ("gmres", "preonly"):
            with pytest.raises(ValueError, match="mg"):
                _solver(["-ksp_type", ksp, "-pc_type", "mg"])
        with pytest.raises(ValueError):
            _solver(["-ksp_type", "cg", "-pc_type", "ilu"])
    finally:
        Options([])


def test_mg_abi_host():
    assert _lib.PC_MG == 2
    assert [f[0] for f in _lib.MgOpts._fields_] == ["max_levels", "smooth_degree", "coarse_max_rows", "esteig_its", "esteig_min",
                                                     "esteig_max"]
    lib = _lib.load_library()
    for name in ("pyn_mg_setup", "pyn_mg_info", "pyn_mg_apply", "pyn_mg_level_get"):
        assert hasattr(lib, name)
