"""Worker of tests/test_gpu_ts.py::test_two_ranks_adaptive: one rank of a 2-rank job whose ranks SHARE ONE GPU (the library's
shared-memory test transport in the place of RCCL).  Runs the adaptive RK solve of y' = lam .* y on its slab of the vector and
checks the step times and its owned entries against the serial run saved by the test.
usage: ts_dist_gpu_worker.py <rank> <size> <shm file> <nx,ny,nz> <serial npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

rank, size, shm = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
nelem = [int(v) for v in sys.argv[4].split(",")]
serial = np.load(sys.argv[5])
os.environ["PYNAMA_SHM_TRANSPORT"] = shm

from pynama_amd.common.comm import Comm  # noqa: E402
from pynama_amd.common.options import Options  # noqa: E402
from pynama_amd.domain.dmplex import DMPlexDom  # noqa: E402
from pynama_amd.solver.ts_solver import TsSolver  # noqa: E402
from pynama_amd.vectors import Vec  # noqa: E402

Options(argv=[])
dom = DMPlexDom(boxMesh={"nelem": nelem, "lower": [0.0] * 3, "upper": [1.0] * 3}, comm=Comm(rank, size))
dom.setFemIndexing(2)
ctx = dom.ctx
bs = 3
sl = slice(dom.rStart * bs, dom.rEnd * bs)
lv, u = Vec(ctx, bs), Vec(ctx, bs)
lv.setArray(serial["lam"][sl])
u.setArray(serial["y0"][sl])
ts = TsSolver(dom.comm)
ts.setTimeStep(0.5)
ts.setMaxTime(1.0)
ts.setTolerances(rtol=1e-8, atol=1e-8)
ts.setRHSFunction(lambda ts_, t, X, F: F.pointwiseMult(lv, X))
times = []
ts.setPostStep(lambda t: times.append(t.getTime()))
ts.solve(u)
ref_t = serial["times"]
same_steps = len(times) == len(ref_t) and np.all(np.abs(np.array(times) - ref_t) <= 1e-12 * np.abs(ref_t))
err = np.abs(u.getArray() - serial["x"][sl]).max()
ok = bool(same_steps and err <= 1e-12 and ts.getStepRejections() == int(serial["rejects"]) and ts.getConvergedReason() == 1
          and dom.rEnd - dom.rStart < len(serial["x"]) // bs)
print(f"rank {rank}/{size}: rows [{dom.rStart}, {dom.rEnd}) steps {len(times)} (serial {len(ref_t)}) rejections "
      f"{ts.getStepRejections()} (serial {int(serial['rejects'])}) max diff {err:.2e} ok={ok}", flush=True)
tot = ctx.allreduce([1.0 if ok else 0.0])[0]
ctx.close()
sys.exit(0 if tot == size else 1)
