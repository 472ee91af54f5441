#!/usr/bin/env python3
"""Second-order (ngl = 3) KLE stiffness on a box mesh: the assembled product (block CSR, what CG multiplies with today) against the
matrix-free shell of pynama_amd/csrc/pyn_matfree_ho3.hip, in one process -- product times (alternating, median after a warm-up), the
largest relative difference of the two products, Jacobi-PCG rates (fixed iterations), a solve to 1e-10 with each, and the shell's own
bytes and flops counted from the shapes, with the bound they imply.
usage: ho3_matfree_case.py dim [nel] [reps] [iters]      (defaults: 2 1024 / 3 64, 7 repeats, 200 CG iterations)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynama_amd import _lib  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2
nel = int(sys.argv[2]) if len(sys.argv) > 2 else (1024 if dim == 2 else 64)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 200
PEAK_FP64 = 78.6e12        # MI355X vector FP64, datasheet
HBM_BW = 6.0e12            # practical HBM rate of this part (tools/write_bw.py: 6.3 TB/s store ceiling)

dom = DMPlexDom(boxMesh={"nelem": [nel] * dim, "lower": [0] * dim, "upper": [1] * dim})
dom.setFemIndexing(3)
ctx = dom.ctx
for t in Spectral(3, dim).deviceTables():
    ctx.tables_set(*t)
bm = dom.boundaryMaskLocal()
ctx.bc_set(dim, np.repeat(bm[:, None], dim, axis=1))
n_rows, nnzb = ctx.csr_symbolic()
K = ctx.mat_create(dim, dim)
ctx.assemble_kle(1e3, 1e2, K)
ctx.matfree_set(_lib.MATFREE_KLE, 1e3, 1e2)
n = n_rows * dim
print(f"{dim}-D {nel}^{dim} ngl 3: {n_rows} nodes, {n} DOFs, nnzb {nnzb}, topology {ctx.mesh_topology()[0]}", flush=True)

rng = np.random.default_rng(0)
x = rng.standard_normal(n)
vx, va, vm = (ctx.vec_create(dim) for _ in range(3))
ctx.vec_set(vx, x)
ta, tm = [], []
for r in range(reps + 2):                       # alternating; the first two rounds are the warm-up
    ctx.spmv(K, vx, va)
    a = ctx.timers()["spmv_ms"]
    ctx.matfree_apply(vx, vm, _lib.MATFREE_KLE)
    m = ctx.timers()["spmv_ms"]
    if r >= 2:
        ta.append(a)
        tm.append(m)
t_asm, t_mf = float(np.median(ta)), float(np.median(tm))
ya, ym = ctx.vec_get(va, dim), ctx.vec_get(vm, dim)
diff = float(np.abs(ya - ym).max() / np.abs(ya).max())

# the shell's work from the shapes of pyn_matfree_ho3.hip: tiles of T rows per axis (3-D 10, 2-D 30) recompute their border cells
T = 10 if dim == 3 else 30
E, N = nel, 2 * nel + 1


def cells_per_axis():
    tot = 0
    for x0 in range(0, N, T):
        lo, hi = x0 // 2 - 1, x0 // 2 + T // 2 - 1
        tot += max(0, min(hi, E - 1) - max(lo, 0) + 1)
    return tot


cells = cells_per_axis() ** dim
redundancy = cells / nel ** dim
if dim == 3:   # FMAs per cell (general J^-1): full-rule Laplacian 3 comps x 3 slices x 513, reduced rule 1080 + 1080
    fma_cell = 3 * 3 * 513 + 1080 + 1080
else:          # 2 comps x 252, reduced 152 + 152
    fma_cell = 2 * 252 + 152 + 152
flops = 2.0 * fma_cell * cells
# HBM bytes of the shell: x (+ halo re-reads served by L2) 8, y 8, mask 1 per DOF; node coordinates of the cell corners
bytes_mf = n * (8 + 8 + 1) + n_rows * 8 * dim
bytes_asm = nnzb * dim * dim * 8 + nnzb * 4 + (n_rows + 1) * 4 + 2 * n * 8
t_flop, t_byte = flops / PEAK_FP64 * 1e3, bytes_mf / HBM_BW * 1e3
print(f"product: assembled {t_asm:.3f} ms ({bytes_asm / t_asm / 1e6:.0f} GB/s of {bytes_asm / 1e9:.2f} GB), shell {t_mf:.3f} ms "
      f"({t_asm / t_mf:.2f}x), max rel diff {diff:.2e}")
print(f"shell work: {cells} cells computed ({redundancy:.2f}x the mesh), {fma_cell} FMA per cell = {flops / 1e9:.2f} GFLOP "
      f"({flops / t_mf / 1e9:.1f} TFLOP/s = {100 * flops / (t_mf * 1e-3) / PEAK_FP64:.0f} % of FP64 peak); "
      f"{bytes_mf / 1e9:.3f} GB HBM ({bytes_mf / t_mf / 1e6:.0f} GB/s); floors {t_flop:.3f} ms (FP64) / {t_byte:.3f} ms (HBM): "
      f"{'FP64 arithmetic' if t_flop > t_byte else 'HBM bytes'} bound the shell on paper", flush=True)

b = rng.standard_normal(n)
b[np.repeat(bm != 0, dim)] = 0.0
vb = ctx.vec_create(dim)
ctx.vec_set(vb, b)
for mf in (_lib.MATFREE_OFF, _lib.MATFREE_KLE):
    for _ in range(2):
        info = ctx.solve(K, vb, vx, fixed_iters=iters, norm_type=_lib.NORM_UNPRECONDITIONED, matfree=mf)
    print(f"  Jacobi-PCG {'shell    ' if mf else 'assembled'}: {info.iters / info.solve_ms * 1e3:.0f} it/s "
          f"({info.solve_ms / info.iters * 1e3:.1f} us/iter)", flush=True)
for mf in (_lib.MATFREE_OFF, _lib.MATFREE_KLE):
    ctx.vec_set(vx, np.zeros(n))
    info = ctx.solve(K, vb, vx, rtol=1e-10, atol=1e-300, maxit=100000, norm_type=_lib.NORM_UNPRECONDITIONED, matfree=mf)
    print(f"  solve to 1e-10 {'shell    ' if mf else 'assembled'}: {info.iters} its, {info.solve_ms:.1f} ms, reason {info.reason}, "
          f"true residual {info.true_resid:.2e}", flush=True)
ctx.close()
