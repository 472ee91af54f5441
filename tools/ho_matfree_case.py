#!/usr/bin/env python3
"""KLE stiffness at order ngl >= 4 on a box mesh: the assembled product (block CSR, what CG multiplies with without the shell) against
the matrix-free shell of pynama_amd/csrc/pyn_matfree_ho.hip, in one process -- product times (alternating, median after a warm-up),
the largest relative difference of the two products, Jacobi-PCG rates (fixed iterations), a solve to 1e-10 with each and its true
residual against the assembled matrix, and the shell's own bytes and flops counted from the shapes, with the bound they imply.
usage: ho_matfree_case.py dim nel ngl [reps] [iters]      (defaults: 7 repeats, 200 CG iterations)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynama_amd import _lib  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

if len(sys.argv) < 4:
    sys.exit(__doc__)
dim, nel, ngl = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
iters = int(sys.argv[5]) if len(sys.argv) > 5 else 200
PEAK_FP64 = 78.6e12        # MI355X vector FP64, datasheet
HBM_BW = 6.0e12            # practical HBM rate of this part (tools/write_bw.py: 6.3 TB/s store ceiling)

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
print(f"{dim}-D {nel}^{dim} ngl {ngl}: {n_rows} nodes, {n} DOFs, nnzb {nnzb} ({nnzb * dim * dim * 8 / 1e9:.2f} GB of values), "
      f"topology {ctx.mesh_topology()[0]}, high-order lattice {ctx.mesh_ho_lattice()}", flush=True)

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

# the shell's work from the shapes of pyn_matfree_ho.hip (every cell once; N nodes, Q = N - 1 reduced points per axis)
N, Q = ngl, ngl - 1
cells, NN, NPT = nel ** dim, ngl ** dim, (ngl - 1) ** dim
fma_full = dim * NN * (2 * dim * N + dim * dim)                     # per component: dim derivatives in, Q g, dim derivatives out
if dim == 3:
    s1, s2 = Q * N * N, Q * Q * N
    fma_red = 3 * (s1 * 2 * N + s2 * 3 * N + NPT * 3 * N) + NPT * 63 + 3 * (s2 * 3 * Q + s1 * 3 * Q + NN * 2 * Q)
else:
    s1 = Q * N
    fma_red = 2 * (s1 * 2 * N + NPT * 2 * N) + NPT * 22 + 2 * (s1 * 2 * Q + NN * 2 * Q)
fma_cell = fma_full + fma_red
flops = 2.0 * fma_cell * cells
# HBM bytes of the shell: pass 1 reads x and the mask once (shared nodes again from L2) and writes the per-cell results; pass 2 reads
# them back with x and the mask and writes y
scratch = cells * NN * dim * 8
bytes_mf = 2 * scratch + n * (8 + 1) + n * (8 + 1 + 8)
bytes_asm = nnzb * dim * dim * 8 + nnzb * 4 + (n_rows + 1) * 4 + 2 * n * 8
t_flop, t_byte = flops / PEAK_FP64 * 1e3, bytes_mf / HBM_BW * 1e3
print(f"product: assembled {t_asm:.3f} ms ({bytes_asm / t_asm / 1e6:.0f} GB/s of {bytes_asm / 1e9:.2f} GB), shell {t_mf:.3f} ms "
      f"({t_asm / t_mf:.2f}x), max rel diff {diff:.2e}")
print(f"shell work: {cells} cells, {fma_cell} FMA per cell = {flops / 1e9:.3f} GFLOP "
      f"({flops / t_mf / 1e9:.2f} TFLOP/s = {100 * flops / (t_mf * 1e-3) / PEAK_FP64:.1f} % of FP64 peak); "
      f"{bytes_mf / 1e9:.4f} GB HBM ({bytes_mf / t_mf / 1e9:.3f} TB/s = {100 * bytes_mf / (t_mf * 1e-3) / HBM_BW:.1f} % of {HBM_BW / 1e12:.1f} TB/s); "
      f"floors {t_flop:.4f} ms (FP64) / {t_byte:.4f} ms (HBM): "
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
