#!/usr/bin/env python3
"""Time integration through the case classes: Taylor-Green 2-D (or a 3-D box) from t = 0 by TsSolver (rk 5bs, adaptive,
MATCHSTEP).  Prints accepted / rejected steps, RHS evaluations, wall time per accepted step split into the RHS (KLE solve, operator
chain and the per-stage analytic boundary fields, timed apart) and the RK vector passes + controller, and the relative L2 error
of the vorticity against the exact field at the end time.  Arguments that start with -pynama_ go to the option database:
-pynama_device_fields evaluates the analytic fields on the device instead of mapping the host functions over the nodes.
usage: ts_case.py [2d|3d] [nelem per direction] [ngl] [end time] [max steps] [rtol] [-pynama_<option> ...]"""
import os
import sys
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pynama_amd  # noqa: E402
from pynama_amd.cases.custom_func import CustomFuncCase  # noqa: E402
from pynama_amd.common.options import Options, flag_set  # noqa: E402

opts = [a for a in sys.argv[1:] if a.startswith("-pynama_")]
argv = [sys.argv[0]] + [a for a in sys.argv[1:] if a not in opts]
dim = 3 if (len(argv) > 1 and argv[1] == "3d") else 2
n = int(argv[2]) if len(argv) > 2 else 8
ngl = int(argv[3]) if len(argv) > 3 else 5
t_end = float(argv[4]) if len(argv) > 4 else 0.5
max_steps = int(argv[5]) if len(argv) > 5 else 5000
rtol = float(argv[6]) if len(argv) > 6 else 1e-6
Options(argv=opts)
where = "device" if flag_set(Options(), "pynama_device_fields") else "host"

with open(os.path.join(os.path.dirname(pynama_amd.__file__), "cases", "taylor-green.yaml")) as f:
    cfg = yaml.load(f, Loader=yaml.Loader)
t0 = time.perf_counter()
fem = CustomFuncCase(cfg, case="taylor-green", nelem=[n] * dim, ngl=ngl, lower=[0.0] * dim, upper=[1.0] * dim,
                     endTime=t_end, maxSteps=max_steps)
fem.setUp()
fem.setUpSolver()
fem.setUpTimeSolver()
ctx = fem.dom.ctx
ctx.sync()
t_setup = time.perf_counter() - t0
ts = fem.ts
ts.setTimeStep(0.1)
ts.setTolerances(rtol=rtol, atol=rtol)

acc = {"rhs": 0.0, "bc": 0.0}
rhs, bc = fem.evalRHS, fem.applyBoundaryConditions


def timed_bc(time_):
    s = time.perf_counter()
    bc(time_)
    if where == "device":      # the launches are asynchronous: wait for them, so that the figure is the fields' time on either path
        ctx.sync()
    acc["bc"] += time.perf_counter() - s


def timed_rhs(ts_, t, X, F):
    ctx.sync()
    s = time.perf_counter()
    rhs(ts_, t, X, F)
    ctx.sync()
    acc["rhs"] += time.perf_counter() - s


fem.applyBoundaryConditions = timed_bc
ts.setRHSFunction(timed_rhs)
fem.computeInitialCondition(ts.getTime())
ctx.sync()
s = time.perf_counter()
ts.solve(fem.vort)
ctx.sync()
wall = time.perf_counter() - s
_, exact = fem.generateExactVecs(ts.getTime())
err = np.linalg.norm(fem.vort.getArray() - exact.getArray()) / np.linalg.norm(exact.getArray())
steps = max(ts.getStepNumber(), 1)
nodes = fem.dom.ctx.n_owned
print(f"taylor-green {dim}-D nelem {n}^{dim} ngl {ngl} ({nodes} nodes), rk {ts.getRKType()} rtol = atol = {rtol:g}, kernel sources "
      f"{pynama_amd._lib.source_hash()}: setup {t_setup:.2f} s")
print(f"t = {ts.getTime():.6g} (reason {ts.getConvergedReason()}): {ts.getStepNumber()} accepted, {ts.getStepRejections()} rejected, "
      f"{ts.rhs_evals} RHS evaluations, last dt {ts.getTimeStep():.3e}")
print(f"wall {wall:.3f} s = {1e3 * wall / steps:.3f} ms per accepted step: RHS {1e3 * acc['rhs'] / steps:.3f} ms "
      f"(of which analytic boundary fields on the {where} {1e3 * acc['bc'] / steps:.3f} ms), RK passes + controller "
      f"{1e3 * (wall - acc['rhs']) / steps:.3f} ms")
print(f"relative L2 error of the vorticity against the exact field: {err:.3e}")
