"""One solveKLE in a fresh process (options are process-wide): argv = case:mode, output .npz, scratch directory.
case gmsh2d / gmsh3d: UniformFlow on a Gmsh file of a jittered box in random node numbering and random cell order (the recipe of
tests/test_gpu_api.py: _write_permuted_box), 2-D [5, 4] at ngl 5 / 3-D [3, 3, 2] at ngl 4; mode on carries
-pynama_mat_free_ho_general, mode off does not.  case tg, mode both: the Taylor-Green box of tests/ho_matfree_facade_worker.py with
-pynama_mat_free_ho and -pynama_mat_free_ho_general.  Every run solves with -ksp_type cg -pc_type jacobi, -ksp_rtol 1e-12 (tg) or
1e-13 (gmsh2d / gmsh3d)."""
import os
import sys

import numpy as np
import yaml

import pynama_amd

pynama_amd.install_reference_layout()

CASES = os.path.join(os.path.dirname(pynama_amd.__file__), "cases")


def _write_permuted_box(path, nelem, upper, jitter=0.2, seed=5):
    from oracle import fem_oracle as fo
    from pynama_amd.domain.gmsh import write_msh
    dim = len(nelem)
    box = fo.box_mesh(nelem, [0.0] * dim, upper, 2, jitter=jitter)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(box.n_node)
    write_msh(path, box.xyz[np.argsort(perm)], perm[box.conn][rng.permutation(box.n_elem)])


def main():
    (case, mode), out, tmp = sys.argv[1].split(":"), sys.argv[2], sys.argv[3]
    from common.options import Options
    flags = {"on": ["-pynama_mat_free_ho_general"], "off": [], "both": ["-pynama_mat_free_ho", "-pynama_mat_free_ho_general"]}[mode]
    # (the Gmsh cases to 1e-13: with 1e-12 the error of the assembled solve ends between 0.5e-10 and 1.2e-10 from run to run, as the
    # order of the assembly's atomic adds moves the iteration CG stops at, and the test bounds it by 1e-10)
    Options(flags + ["-ksp_type", "cg", "-pc_type", "jacobi", "-ksp_rtol", "1e-12" if case == "tg" else "1e-13"])
    if case == "tg":
        from cases.custom_func import CustomFuncCase
        with open(os.path.join(CASES, "taylor-green.yaml")) as f:
            data = yaml.load(f, Loader=yaml.Loader)
        fem = CustomFuncCase(data, case="taylor-green", nelem=[6, 6], ngl=5)
        t0 = (0.0,)
    else:
        from cases.uniform import UniformFlow
        nelem, upper, ngl = ([5, 4], [1.0, 0.8], 5) if case == "gmsh2d" else ([3, 3, 2], [1.0, 0.8, 1.2], 4)
        path = os.path.join(tmp, f"{case}.msh")
        _write_permuted_box(path, nelem, upper)
        with open(os.path.join(CASES, "uniform.yaml")) as f:
            data = yaml.load(f, Loader=yaml.Loader)
        data["domain"] = {"ngl": ngl, "gmsh-file": path}
        fem = UniformFlow(data, case="uniform")
        t0 = ()
    fem.setUp()
    fem.setUpSolver()
    tag = fem.mat.K.matfree
    exactVel, exactVort = fem.generateExactVecs(*t0)
    fem.solveKLE(time=0.0, vort=exactVort)
    np.savez(out, vel=fem.vel.getArray(), tag=-1 if tag is None else int(tag), shell_used=bool(fem.solver.shell_used),
             err=float((exactVel - fem.vel).norm(norm_type=2)), topo=fem.dom.ctx.mesh_topology()[0])


if __name__ == "__main__":
    main()
