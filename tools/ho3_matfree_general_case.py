#!/usr/bin/env python3
"""KLE stiffness at order ngl 3 on a BENT, randomly renumbered box mesh: the assembled product (block CSR, the only product such a mesh
had before) against the general ngl 3 matrix-free shell of pynama_amd/csrc/pyn_matfree_ho3_general.hip (PYN_MATFREE_KLE_NGL3_GENERAL),
in one process -- what tools/ho_matfree_general_case.py prints at the orders ngl >= 4: product times (alternating, median after a
warm-up), the largest relative difference of the products, Jacobi-PCG rates (fixed iterations), a solve to 1e-10 with each and its
true residual against the assembled matrix.
The mesh: a box lattice whose interior corners are moved by bend * h, every second-order node recomputed from its cell's corners, the
nodes renumbered at random.  With bend 0 the mesh keeps its lexicographic numbering and THREE products alternate -- assembled, the affine
shell (PYN_MATFREE_KLE, pyn_matfree_ho3.hip) and the general shell: the price of the general path on a mesh the affine kernel also serves.
usage: ho3_matfree_general_case.py dim n [bend] [reps] [iters]      (defaults: bend 0.2, 7 repeats, 200 CG iterations)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynama_amd import _lib  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

if len(sys.argv) < 3:
    sys.exit(__doc__)
NGL = 3
dim, nel = int(sys.argv[1]), int(sys.argv[2])
bend = float(sys.argv[3]) if len(sys.argv) > 3 else 0.2
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
iters = int(sys.argv[5]) if len(sys.argv) > 5 else 200
G = _lib.MATFREE_KLE_NGL3_GENERAL

dom = DMPlexDom(boxMesh={"nelem": [nel] * dim, "lower": [0] * dim, "upper": [1] * dim})
dom.setFemIndexing(NGL)
elem = Spectral(NGL, dim)
conn, xyz, bm = np.asarray(dom.conn, np.int64), np.array(dom.xyz, dtype=np.float64), np.asarray(dom.boundaryMaskLocal()) != 0
dom.ctx.close()
nc = 2 ** dim
rng = np.random.default_rng(0)
if bend > 0.0:
    corner_ids = np.unique(conn[:, :nc])
    inner = corner_ids[~bm[corner_ids]]
    cxyz = xyz.copy()
    cxyz[inner] += bend / nel * rng.uniform(-1.0, 1.0, (len(inner), dim))
    H = np.asarray(elem.HCooOp)                                  # [nn, 2^dim]: the corner basis at the nodes
    for e0 in range(0, conn.shape[0], 65536):                    # every node = the multilinear image of its cell's corners
        ce = conn[e0:e0 + 65536]
        xyz[ce.ravel()] = np.einsum("gc,ecd->egd", H, cxyz[ce[:, :nc]]).reshape(-1, dim)
    xyz[corner_ids] = cxyz[corner_ids]
    perm = rng.permutation(xyz.shape[0])                         # new id of old node
    conn, xyz, bm = perm[conn], xyz[np.argsort(perm)], bm[np.argsort(perm)]

ctx = _lib.Context(_lib.default_device())
ctx.mesh_set(dim, np.ascontiguousarray(conn, dtype=np.int32), np.ascontiguousarray(xyz))
for t in elem.deviceTables():
    ctx.tables_set(*t)
ctx.bc_set(dim, np.repeat(bm[:, None], dim, axis=1).astype(np.uint8))
n_rows, nnzb = ctx.csr_symbolic()
K = ctx.mat_create(dim, dim)
ctx.assemble_kle(1e3, 1e2, K)
ops = [("assembled", _lib.MATFREE_OFF)]
if bend == 0.0:
    ctx.matfree_set(_lib.MATFREE_KLE, 1e3, 1e2)
    ops.append(("affine   ", _lib.MATFREE_KLE))
ctx.matfree_set(G, 1e3, 1e2)
ops.append(("general  ", G))
n = n_rows * dim
print(f"{dim}-D {nel}^{dim} ngl {NGL} bend {bend}: {n_rows} nodes, {n} DOFs, nnzb {nnzb} ({nnzb * dim * dim * 8 / 1e9:.2f} GB of values), "
      f"topology {ctx.mesh_topology()[0]}, numbering {'random' if bend > 0.0 else 'lexicographic'}", flush=True)

x = rng.standard_normal(n)
vx = ctx.vec_create(dim)
vy = {op: ctx.vec_create(dim) for _, op in ops}
ctx.vec_set(vx, x)
times = {op: [] for _, op in ops}
for r in range(reps + 2):                       # alternating; the first two rounds are the warm-up
    for _, op in ops:
        if op == _lib.MATFREE_OFF:
            ctx.spmv(K, vx, vy[op])
        else:
            ctx.matfree_apply(vx, vy[op], op)
        if r >= 2:
            times[op].append(ctx.timers()["spmv_ms"])
med = {op: float(np.median(v)) for op, v in times.items()}
ya = ctx.vec_get(vy[_lib.MATFREE_OFF], dim)
t_asm = med[_lib.MATFREE_OFF]
bytes_asm = nnzb * dim * dim * 8 + nnzb * 4 + (n_rows + 1) * 4 + 2 * n * 8
print(f"product: assembled {t_asm:.3f} ms ({bytes_asm / t_asm / 1e6:.0f} GB/s of {bytes_asm / 1e9:.2f} GB)", end="")
for name, op in ops[1:]:
    diff = float(np.abs(ya - ctx.vec_get(vy[op], dim)).max() / np.abs(ya).max())
    print(f", {name.strip()} {med[op]:.3f} ms ({t_asm / med[op]:.2f}x, max rel diff {diff:.2e})", end="")
if bend == 0.0:
    print(f", general / affine {med[G] / med[_lib.MATFREE_KLE]:.2f}", end="")
print(flush=True)

b = rng.standard_normal(n)
b[np.repeat(bm, dim)] = 0.0
vb = ctx.vec_create(dim)
ctx.vec_set(vb, b)
for name, mf in ops:
    for _ in range(2):
        info = ctx.solve(K, vb, vx, fixed_iters=iters, norm_type=_lib.NORM_UNPRECONDITIONED, matfree=mf)
    print(f"  Jacobi-PCG {name}: {info.iters / info.solve_ms * 1e3:.0f} it/s ({info.solve_ms / info.iters * 1e3:.1f} us/iter)", flush=True)
for name, mf in ops:
    ctx.vec_set(vx, np.zeros(n))
    info = ctx.solve(K, vb, vx, rtol=1e-10, atol=1e-300, maxit=100000, norm_type=_lib.NORM_UNPRECONDITIONED, matfree=mf)
    print(f"  solve to 1e-10 {name}: {info.iters} its, {info.solve_ms:.1f} ms, reason {info.reason}, "
          f"true residual {info.true_resid:.2e}", flush=True)
ctx.close()
