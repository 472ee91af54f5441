"""Worker of tests/test_gpu_fields.py::test_two_ranks_fields: one rank of a 2-rank job whose ranks SHARE ONE GPU (the library's
shared-memory test transport in the place of RCCL).  Builds its slab of the 3-D box [2, 2, 4] at ngl 3, evaluates every 3-D field
on the device (-pynama_device_fields) over the boundary and over all nodes through DMPlexDom.applyFunctionVecToVec, and checks its
owned entries against the numpy restatement at the coordinates of its own nodes: a local-id mistake shows here, because the owned
planes are numbered first.
usage: fields_dist_gpu_worker.py <rank> <size> <shm file>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

rank, size, shm = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
os.environ["PYNAMA_SHM_TRANSPORT"] = shm

from pynama_amd.cases import fields  # noqa: E402
from pynama_amd.common.comm import Comm  # noqa: E402
from pynama_amd.common.options import Options  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.vectors import Vec  # noqa: E402
from tests import fields_model as fm  # noqa: E402

Options(argv=["-pynama_device_fields"])
FILL, NU, T = 7.25, 0.02, 0.37
dom = DMPlexDom(boxMesh={"nelem": [2, 2, 4], "lower": [0.0] * 3, "upper": [1.0] * 3}, comm=Comm(rank, size))
dom.setFemIndexing(3)
ctx = dom.ctx
n = dom.nOwned
bc = dom.nodeSet(dom.getNodesFromLabel("External Boundary"))
everything = dom.nodeSet(dom.getAllNodes())
ok = bool(0 < n < dom.nNodesGlobal and ctx.n_ghost > 0 and 0 < len(bc) < n and everything.id == -1)
worst = 0.0
try:
    for f in (f for f in fields.FIELDS if f.dim == 3):
        p = f.params(NU, T)
        for ns in (bc, everything):
            v = Vec(ctx, f.bs)
            v.set(FILL)
            dom.applyFunctionVecToVec(ns, f.bind(NU, T), v, f.bs)
            got = v.getArray().reshape(n, f.bs)
            ref = fm.restate(f.id, p, dom.getNodesCoordinates(ns.globalNodes))
            r = float(np.abs(got[ns.localNodes] - ref).max() / (fm.ULP * fm.amplitude(f.id, p)))
            worst = max(worst, r)
            rest = np.ones(n, bool)
            rest[ns.localNodes] = False
            ok = ok and r <= 32.0 and bool(np.all(got[rest] == FILL))
except Exception as e:      # the other rank waits in the all-reduce below: report and join it
    print(f"rank {rank}/{size}: {type(e).__name__}: {e}", flush=True)
    ok = False
print(f"rank {rank}/{size}: rows [{dom.rStart}, {dom.rEnd}) of {dom.nNodesGlobal}, {len(bc)} boundary nodes, "
      f"largest |device - numpy| / (2^-52 A) = {worst:.2f} ok={ok}", flush=True)
tot = ctx.allreduce([1.0 if ok else 0.0])[0]
ctx.close()
sys.exit(0 if tot == size else 1)
