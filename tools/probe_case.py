#!/usr/bin/env python3
"""Point probes (pynama_amd/csrc/pyn_probe.hip) on a box mesh of nel^dim cells at order ngl: npoints random points of the box are located
once and a random velocity field (block size dim) is sampled at them.  Prints the path taken (0: binary search on the rectilinear
lattice, 1: bin grid + Newton), found / total, the most Newton steps and candidates of a point, the location time (host clock around
pyn_probe_create, which ends with a synchronise: upload, lattice check or bin build, location) and the mean time of 20 sample calls
after a warm-up (host clock around pyn_probe_sample, which copies the [n, dim] result to the host and synchronises), next to the bytes
the gather asks for: n nn bs 8 B of nodal values plus n nn 4 B of connectivity rows.
`bent`: the interior corners are moved by 0.2 h, every node recomputed from its cell's corners and the nodes renumbered at random, so
that the mesh is no lattice any more and the search path runs.
usage: probe_case.py dim nel ngl npoints [bent]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynama_amd import _lib  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

if len(sys.argv) < 5:
    sys.exit(__doc__)
dim, nel, ngl, npoints = (int(a) for a in sys.argv[1:5])
bent = len(sys.argv) > 5 and sys.argv[5] == "bent"
CALLS = 20

dom = DMPlexDom(boxMesh={"nelem": [nel] * dim, "lower": [0] * dim, "upper": [1] * dim})
dom.setFemIndexing(ngl)
rng = np.random.default_rng(0)
if bent:
    conn, xyz, bm = np.asarray(dom.conn, np.int64), np.array(dom.xyz, dtype=np.float64), np.asarray(dom.boundaryMaskLocal()) != 0
    nc = 2 ** dim
    corner_ids = np.unique(conn[:, :nc])
    inner = corner_ids[~bm[corner_ids]]
    cxyz = xyz.copy()
    cxyz[inner] += 0.2 / nel * rng.uniform(-1.0, 1.0, (len(inner), dim))
    H = np.asarray(Spectral(ngl, dim).HCooOp)                    # [nn, 2^dim]: the corner basis at the nodes
    for e0 in range(0, conn.shape[0], 65536):
        ce = conn[e0:e0 + 65536]
        xyz[ce.ravel()] = np.einsum("gc,ecd->egd", H, cxyz[ce[:, :nc]]).reshape(-1, dim)
    xyz[corner_ids] = cxyz[corner_ids]
    perm = rng.permutation(xyz.shape[0])                         # new id of old node
    ctx = _lib.Context(_lib.default_device())
    ctx.mesh_set(dim, np.ascontiguousarray(perm[conn], dtype=np.int32), np.ascontiguousarray(xyz[np.argsort(perm)]))
else:
    ctx = dom.ctx                                                # generated on the device (pyn_mesh_box)
nn, n_node = ngl ** dim, ctx.n_owned
pts = rng.uniform(0.0, 1.0, (npoints, dim))
vec = ctx.vec_create(dim)
ctx.vec_set(vec, rng.standard_normal(n_node * dim))

warm = ctx.probe_create(pts[:min(npoints, 1000)])                # the first call of every kernel pays for its code object
ctx.probe_sample(warm, vec)
ctx.probe_destroy(warm)
ctx.sync()
t0 = time.perf_counter()
pid = ctx.probe_create(pts)
t_locate = time.perf_counter() - t0
info = ctx.probe_info(pid)
for _ in range(3):
    out = ctx.probe_sample(pid, vec)
ctx.sync()
t0 = time.perf_counter()
for _ in range(CALLS):
    out = ctx.probe_sample(pid, vec)
t_sample = (time.perf_counter() - t0) / CALLS
again = ctx.probe_sample(pid, vec)
gather = npoints * nn * (dim * 8 + 4)
print(f"probe_case {dim}-D {nel}^{dim} cells ngl {ngl}{' bent' if bent else ''}: {n_node} nodes, {npoints} points, source {_lib.source_hash()}")
print(f"  path {info['path']}, found {info['found']} / {info['n']}, Newton steps <= {info['max_newton']}, candidates <= {info['max_candidates']}")
print(f"  location {t_locate * 1e3:.3f} ms;  sample (bs {dim}) mean of {CALLS}: {t_sample * 1e3:.3f} ms "
      f"= {npoints / t_sample * 1e-6:.1f} Mpoints/s;  gather {gather / 1e6:.1f} MB -> {gather / t_sample * 1e-9:.1f} GB/s asked for, "
      f"result copy {npoints * dim * 8 / 1e6:.1f} MB")
print(f"  two calls identical: {np.array_equal(out, again, equal_nan=True)}")
ctx.probe_destroy(pid)
ctx.close()
