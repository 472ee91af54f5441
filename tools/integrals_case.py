#!/usr/bin/env python3
"""Mesh integrals (pynama_amd/csrc/pyn_integrals.hip) of a random velocity field (block size dim) on a box mesh of nel^dim cells at
order ngl.  For each rule (nodal, Gauss with ngl + 1 points per axis), with and without the gradient moments: the mean device time of
20 calls (pyn_timers_get: HIP events around the cell pass and the pass over the partials) after 3 warm-up calls, and the time of
pyn_vec_norm on the same vector, taken alternately in the same process (host clock around the call, which ends with a synchronise;
the integrals' host-clock time is printed next to it for a like-for-like ratio).  Also the bytes one pass reads: the vector and the
connectivity.
`bent`: the interior corners are moved by 0.2 h, every node recomputed from its cell's corners and the nodes renumbered at random.
usage: integrals_case.py dim nel ngl [bent]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynama_amd import _lib  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.elements.spectral import Spectral  # noqa: E402

if len(sys.argv) < 4:
    sys.exit(__doc__)
dim, nel, ngl = (int(a) for a in sys.argv[1:4])
bent = len(sys.argv) > 4 and sys.argv[4] == "bent"
CALLS, WARM = 20, 3

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
nn, n_node, n_elem = ngl ** dim, ctx.n_owned, nel ** dim
vec = ctx.vec_create(dim)
ctx.vec_set(vec, rng.standard_normal(n_node * dim))
vec_bytes, conn_bytes = n_node * dim * 8, n_elem * nn * 4

print(f"integrals_case {dim}-D {nel}^{dim} cells ngl {ngl}{' bent' if bent else ''}: {n_node} nodes, source {_lib.source_hash()}")
print(f"  one pass reads: vector {vec_bytes / 1e6:.1f} MB + connectivity {conn_bytes / 1e6:.1f} MB = {(vec_bytes + conn_bytes) / 1e6:.1f} MB")
for rule, rname in ((_lib.RULE_NODAL, "nodal"), (_lib.RULE_GAUSS, "gauss")):
    for grad in (False, True):
        for _ in range(WARM):
            first = ctx.integrate(vec, None, rule, grad)
            ctx.vec_norm(vec)
        dev, host, norm = [], [], []
        for _ in range(CALLS):                                   # alternately: the two see the same clocks and the same neighbours
            t0 = time.perf_counter()
            out = ctx.integrate(vec, None, rule, grad)
            host.append(time.perf_counter() - t0)
            dev.append(ctx.timers()["integrate_ms"])
            t0 = time.perf_counter()
            ctx.vec_norm(vec)
            norm.append(time.perf_counter() - t0)
        d, h, n = np.mean(dev), 1e3 * np.mean(host), 1e3 * np.mean(norm)
        print(f"  {rname:5s} grad {int(grad)}: device {d:.3f} ms (min {np.min(dev):.3f}) = {(vec_bytes + conn_bytes) / d * 1e-6:.1f} GB/s of the bytes read; "
              f"call {h:.3f} ms; vec_norm call {n:.3f} ms; ratio of calls {h / n:.2f}; identical to the first call: "
              f"{out.tobytes() == first.tobytes()}")
ctx.close()
