"""Worker of tests/test_gpu_ho_matfree.py::test_ranks_sharing_one_gpu: one rank of a world_size-N job whose ranks SHARE ONE GPU (the
library's shared-memory test transport in the place of RCCL).  One KLE solve at order ngl >= 4, single-reduction Jacobi-PCG with the
blocking halo exchange, with the assembled K and with the matrix-free shell; the product against the assembled product of the rank.
usage: ho_matfree_dist_worker.py <rank> <size> <shm file> <nx,ny[,nz]> <ngl>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

rank, size, shm = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
nelem = [int(v) for v in sys.argv[4].split(",")]
ngl = int(sys.argv[5])
os.environ["PYNAMA_SHM_TRANSPORT"] = shm

from pynama_amd import _lib  # noqa: E402
from pynama_amd.common.comm import Comm  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

dim = len(nelem)
lo, up = [0.0] * dim, [1.0, 0.8, 1.2][:dim]
dom = DMPlexDom(boxMesh={"nelem": nelem, "lower": lo, "upper": up}, comm=Comm(rank, size))
dom.setFemIndexing(ngl)
ctx = dom.ctx
for t in Spectral(ngl, dim).deviceTables():
    ctx.tables_set(*t)
assert ctx.mesh_topology()[0] == "general" and ctx.mesh_ho_lattice()[0] == ngl
ctx.bc_set(dim, np.repeat(dom.boundaryMaskLocal()[:, None], dim, axis=1))
ctx.csr_symbolic()
K = ctx.mat_create(dim, dim)
ctx.assemble_kle(1e3, 1e2, K)
ctx.matfree_set(_lib.MATFREE_KLE, 1e3, 1e2)

n_glob = int(np.prod([(ngl - 1) * n + 1 for n in nelem]))
bg = np.random.default_rng(5).standard_normal((n_glob, dim))          # the same global vector on every rank
bg[np.fromiter(dom.getBordersNodes(), dtype=np.int64)] = 0.0
rows = np.arange(dom.rStart, dom.rEnd)
vb, vx, vy, va = (ctx.vec_create(dim) for _ in range(4))
ctx.vec_set(vb, bg[rows].ravel())

msg = []
# the product: ghosts travel through the halo exchange
ctx.matfree_apply(vb, vy, _lib.MATFREE_KLE)
ctx.spmv(K, vb, va)
ya = ctx.vec_get(va, dim)
e_mf = np.abs(ctx.vec_get(vy, dim) - ya).max() / np.abs(ya).max()
ok = e_mf < 2e-13
msg.append(f"product {e_mf:.2e}")
kw = dict(method=_lib.KSP_CG, pc=_lib.PC_JACOBI, rtol=1e-10, atol=1e-300, maxit=100000, norm_type=_lib.NORM_UNPRECONDITIONED)
ctx.vec_set(vx, np.zeros(rows.size * dim))
ia = ctx.solve(K, vb, vx, **kw)
xa = ctx.vec_get(vx, dim)
ctx.vec_set(vx, np.zeros(rows.size * dim))
im = ctx.solve(K, vb, vx, matfree=_lib.MATFREE_KLE, **kw)
xm = ctx.vec_get(vx, dim)
e_sol = np.abs(xm - xa).max() / np.abs(xa).max()
ok &= ia.reason > 0 and im.reason > 0 and abs(ia.iters - im.iters) <= 1 and im.true_resid <= 1e-10 and e_sol < 1e-7
msg.append(f"CG assembled {ia.iters} its / shell {im.iters} its, true residual {im.true_resid:.2e}, shell vs assembled {e_sol:.2e}")
print(f"rank {rank}/{size}: " + "; ".join(msg), flush=True)
ctx.close()
sys.exit(0 if ok else 1)
