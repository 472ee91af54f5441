"""Worker of tests/test_gpu_ho3_matfree.py::test_ranks_sharing_one_gpu: one rank of a world_size-N job whose ranks SHARE ONE GPU
(the library's shared-memory test transport in the place of RCCL).  One second-order (ngl 3) KLE solve, single-reduction Jacobi-PCG,
with the assembled K and with the matrix-free shell; both against the serial oracle.
usage: ho3_matfree_dist_worker.py <rank> <size> <shm file> <nx,ny[,nz]>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

rank, size, shm = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
nelem = [int(v) for v in sys.argv[4].split(",")]
os.environ["PYNAMA_SHM_TRANSPORT"] = shm

from oracle import fem_oracle as fo  # noqa: E402
from pynama_amd import _lib  # noqa: E402
from pynama_amd.common.comm import Comm  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

dim = len(nelem)
lo, up = [0.0] * dim, [1.0, 0.8, 1.2][:dim]
dom = DMPlexDom(boxMesh={"nelem": nelem, "lower": lo, "upper": up}, comm=Comm(rank, size))
dom.setFemIndexing(3)
ctx = dom.ctx
for t in Spectral(3, dim).deviceTables():
    ctx.tables_set(*t)
assert ctx.mesh_topology()[0] == "lattice-ngl3"
ctx.bc_set(dim, np.repeat(dom.boundaryMaskLocal()[:, None], dim, axis=1))
ctx.csr_symbolic()
K = ctx.mat_create(dim, dim)
ctx.assemble_kle(1e3, 1e2, K)
ctx.matfree_set(_lib.MATFREE_KLE, 1e3, 1e2)

glob = fo.box_mesh(nelem, lo, up, 3)
ref = fo.assemble_kle_freeslip(glob, fo.Tables(3, dim))
bg = np.random.default_rng(5).standard_normal(glob.n_node * dim)
bg[np.repeat(np.isin(np.arange(glob.n_node), glob.boundary), dim)] = 0.0
rows = (np.arange(dom.rStart, dom.rEnd)[:, None] * dim + np.arange(dim)).ravel()
vb, vx, vy = ctx.vec_create(dim), ctx.vec_create(dim), ctx.vec_create(dim)
ctx.vec_set(vb, bg[rows])

msg = []
ok = True
# the product: ghosts travel through the halo exchange
y_ref = (ref["K"] @ bg)[rows]
ctx.matfree_apply(vb, vy, _lib.MATFREE_KLE)
e_mf = np.abs(ctx.vec_get(vy, dim) - y_ref).max() / np.abs(y_ref).max()
ok &= e_mf < 2e-13
msg.append(f"product {e_mf:.2e}")
kw = dict(method=_lib.KSP_CG, pc=_lib.PC_JACOBI, rtol=1e-10, atol=1e-300, maxit=100000, norm_type=_lib.NORM_UNPRECONDITIONED)
ctx.vec_set(vx, np.zeros(len(rows)))
ia = ctx.solve(K, vb, vx, **kw)
xa = ctx.vec_get(vx, dim)
ctx.vec_set(vx, np.zeros(len(rows)))
im = ctx.solve(K, vb, vx, matfree=_lib.MATFREE_KLE, **kw)
xm = ctx.vec_get(vx, dim)
x_ref = fo.pcg(ref["K"], bg, rtol=1e-10, norm_type=fo.NORM_UNPRECONDITIONED)[0][rows]
e_sol = np.abs(xm - xa).max() / np.abs(xa).max()
e_ref = np.abs(xm - x_ref).max() / np.abs(x_ref).max()
ok &= ia.reason > 0 and im.reason > 0 and abs(ia.iters - im.iters) <= 2 and im.true_resid <= 1e-10 and e_sol < 1e-9 and e_ref < 1e-8
msg.append(f"CG assembled {ia.iters} its / shell {im.iters} its, true residual {im.true_resid:.2e}, shell vs assembled {e_sol:.2e}, "
           f"vs oracle {e_ref:.2e}")
print(f"rank {rank}/{size}: " + "; ".join(msg), flush=True)
ctx.close()
sys.exit(0 if ok else 1)
