"""Banded LU (pyn_solve_direct_band) on the reference's case sizes above the dense limit, next to today's preonly/lu substitute
(Jacobi-PCG / GMRES to round-off) on the same right-hand side: kl / ku, factor bytes, factor ms, ms of a repeated solve.
usage: python tools/direct_band_case.py [--big]  (on the GPU box; --big adds 2-D 192 x 192 ngl 3, about 11 GB of factors)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import pynama_amd

pynama_amd.install_reference_layout()
import yaml
from cases.uniform import UniformFlow

from pynama_amd.solver.ksp_solver import KspSolver

CASES = os.path.join(os.path.dirname(pynama_amd.__file__), "cases")
with open(os.path.join(CASES, 'uniform.yaml')) as f:
    Y = yaml.load(f, Loader=yaml.Loader)

SYSTEMS = [("2-D 50x50 ngl 3 (ibm-static)", dict(nelem=[50, 50]), False),
           ("3-D 9^3 ngl 3 (taylor-green2d-3d)", dict(lower=[0, 0, 0], upper=[1, 1, 1], nelem=[9, 9, 9]), False),
           ("3-D 9^3 ngl 3, one diagonal entry zeroed (pivoting)", dict(lower=[0, 0, 0], upper=[1, 1, 1], nelem=[9, 9, 9]), True)]
if "--big" in sys.argv:
    SYSTEMS.append(("2-D 192x192 ngl 3", dict(nelem=[192, 192]), False))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, 1e3 * (time.perf_counter() - t0)


for name, kw, zero_diag in SYSTEMS:
    fem = UniformFlow(Y, case='uniform', ngl=3, **kw)
    fem.setUp()
    fem.setUpSolver()
    K = fem.mat.K
    ctx = K.ctx
    n = ctx.n_owned * K.br
    if zero_diag:                                    # an interior diagonal entry cancelled: the factorisation has to pivot
        i = n // 2 + 1
        K.setValue(i, i, 0.0)
        K.assemble()
    kl, ku, nbytes = ctx.direct_band_info(K.id)
    b, x = K.createVecLeft(), K.createVecRight()
    b.setArray(np.random.default_rng(1).standard_normal(n))
    i1, w1 = timed(lambda: ctx.solve_direct_band(K.id, b.id, x.id, max_bytes=1 << 40))
    line = (f"{name}: n={n} kl={kl} ku={ku} bytes={nbytes / 1e9:.3f} GB | first call {i1.solve_ms:.1f} ms device "
            f"({w1:.1f} ms wall, resid {i1.true_resid:.1e})")
    if not zero_diag:
        reps = [timed(lambda: ctx.solve_direct_band(K.id, b.id, x.id, max_bytes=1 << 40)) for _ in range(5)]
        dev = sorted(r[0].solve_ms for r in reps)[2]
        wall = sorted(r[1] for r in reps)[2]
        line += f" | repeated solve {dev:.2f} ms device ({wall:.2f} ms wall, median of 5)"
        ksp = KspSolver()
        ksp.createSolver(K, fem.comm)                # default options: today's substitute above the dense limit
        y = K.createVecRight()
        ik, wk = timed(lambda: ksp(b, y))
        ik, wk = timed(lambda: ksp(b, y))            # the symmetry probe of the first call excluded
        diff = np.abs(y.getArray() - x.getArray()).max() / np.abs(x.getArray()).max()
        line += (f" | substitute {wk:.1f} ms wall, {ik.iters} its (resid {ik.true_resid:.1e}, rel. diff to LU {diff:.1e})")
    print(line, flush=True)
    del fem, K, b, x
