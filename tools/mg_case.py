#!/usr/bin/env python3
"""Geometric multigrid PCG (pynama_amd/csrc/pyn_mg.hip) against Jacobi-PCG on the KLE stiffness K of a box mesh of order ngl (default
3; ngl >= 4: level 1 is the Q1 lattice of the same cells, the shell is the ngl >= 4 operator of -pynama_mat_free_ho) with the reference's Dirichlet boundary (every velocity DOF on the boundary imposed), in one process: for the assembled product and
the matrix-free shell at level 0, iterations to rtol 1e-10 (unpreconditioned norm), device solve time, the hierarchy's set-up time
(host clock, first build), the time of one V-cycle (mg_apply, median) and the true residual.  For ngl >= 4 the MG legs run with
Chebyshev degree 2 and 4, and the set-up line carries the time of the 3^dim * dim assembled products that probe level 1.
usage: mg_case.py dim nel [label] [ngl] [shell-mg]     (e.g. 2 1024, 3 64, 2 50 "50x50", 2 30 "cavity 30^2", 2 256 "" 5)
shell-mg: only the degree-2 MG-PCG solve with the shell (the run a kernel trace is taken of)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynama_amd import _lib  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2
nel = int(sys.argv[2]) if len(sys.argv) > 2 else (1024 if dim == 2 else 64)
ngl = int(sys.argv[4]) if len(sys.argv) > 4 else 3
shell_mg = len(sys.argv) > 5 and sys.argv[5] == "shell-mg"
label = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] else f"{dim}-D {nel}^{dim} ngl {ngl}"

dom = DMPlexDom(boxMesh={"nelem": [nel] * dim, "lower": [0] * dim, "upper": [1] * dim})
dom.setFemIndexing(ngl)
ctx = dom.ctx
for t in Spectral(ngl, dim).deviceTables():
    ctx.tables_set(*t)
bm = dom.boundaryMaskLocal()
ctx.bc_set(dim, np.repeat(bm[:, None], dim, axis=1))
n_rows, nnzb = ctx.csr_symbolic()
K = ctx.mat_create(dim, dim)
ctx.assemble_kle(1e3, 1e2, K)
ctx.matfree_set(_lib.MATFREE_KLE, 1e3, 1e2)
n = n_rows * dim
b = np.random.default_rng(0).standard_normal(n)
b[np.repeat(bm != 0, dim)] = 0.0
vb, vx, vz = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
ctx.vec_set(vb, b)
print(f"{label}: {n_rows} nodes, {n} DOFs, topology {ctx.mesh_topology()[0]}", flush=True)

kw = dict(rtol=1e-10, atol=1e-300, maxit=200000, norm_type=_lib.NORM_UNPRECONDITIONED)
jac = {}
for degree in ((0,) if ngl == 3 else (2,) if shell_mg else (2, 4)):      # 0: the default (degree 2), as the ngl 3 runs always had it
    t0 = time.perf_counter()
    ctx.mg_setup(K, smooth_degree=degree)         # defaults: Chebyshev degree 2, coarse_max_rows 4096
    t_setup_host = (time.perf_counter() - t0) * 1e3
    info = ctx.mg_info(K)
    if degree:
        print(f"  Chebyshev degree {degree}", flush=True)
    print(f"  hierarchy: {info['levels']} levels, rows {info['rows']}, lambda {[round(v, 3) for v in info['lambda'][:-1]]}, "
          f"set-up {info['setup_ms']:.1f} ms", flush=True)
    if ngl > 3 and not shell_mg:                  # what the probing products of the set-up cost: the same product, timed alone
        tp = []
        for r in range(7):
            t0 = time.perf_counter()
            ctx.spmv(K, vb, vz)
            if r >= 2:
                tp.append((time.perf_counter() - t0) * 1e3)
        n_probe = 3 ** dim * dim
        t_probe = float(np.median(tp)) * n_probe
        print(f"  set-up: {n_probe} probing products x {np.median(tp):.3f} ms = {t_probe:.1f} ms "
              f"({100 * t_probe / info['setup_ms']:.0f} % of the set-up)", flush=True)
    vc = []
    for r in range(7):                            # one V-cycle with the assembled level 0 (host clock around a synchronised call)
        t0 = time.perf_counter()
        ctx.mg_apply(K, vb, vz)
        if r >= 2:
            vc.append((time.perf_counter() - t0) * 1e3)
    t_vc = float(np.median(vc))
    print(f"  V-cycle (assembled level 0): {t_vc:.3f} ms", flush=True)
    for mf, name in ((_lib.MATFREE_OFF, "assembled"), (_lib.MATFREE_KLE, "shell    ")):
        if shell_mg:
            if mf == _lib.MATFREE_KLE:
                im = ctx.solve(K, vb, vx, pc=_lib.PC_MG, matfree=mf, **kw)
                print(f"  {name}: MG-PCG {im.iters} its {im.solve_ms:.1f} ms (true resid {im.true_resid:.1e})", flush=True)
            continue
        if mf not in jac:                         # Jacobi-PCG once per product
            ij = ctx.solve(K, vb, vx, pc=_lib.PC_JACOBI, matfree=mf, **kw)
            jac[mf] = (ij, ctx.vec_get(vx, dim))
        ij, xj = jac[mf]
        ctx.solve(K, vb, vx, pc=_lib.PC_MG, matfree=mf, fixed_iters=1, **kw)   # warm-up (the hierarchy is cached)
        im = ctx.solve(K, vb, vx, pc=_lib.PC_MG, matfree=mf, **kw)
        xm = ctx.vec_get(vx, dim)
        diff = float(np.abs(xm - xj).max() / np.abs(xj).max())
        mg_total = im.solve_ms + info["setup_ms"]
        print(f"  {name}: Jacobi-PCG {ij.iters} its {ij.solve_ms:.1f} ms (true resid {ij.true_resid:.1e}) | MG-PCG {im.iters} its "
              f"{im.solve_ms:.1f} ms + set-up {info['setup_ms']:.1f} ms = {mg_total:.1f} ms (true resid {im.true_resid:.1e}, "
              f"{im.solve_ms / max(im.iters, 1):.2f} ms/it) | speed-up {ij.solve_ms / mg_total:.2f}x incl. set-up, "
              f"{ij.solve_ms / im.solve_ms:.2f}x solve only | max rel diff of x {diff:.1e}", flush=True)
ctx.close()
