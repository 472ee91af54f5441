#!/usr/bin/env python3
"""Same-process A/B of the Q1 lattice assembly on the bench mesh (nel^3 Q1 hexahedra on a rectilinear box, Dirichlet faces): the
variants are alternated round by round on ONE context, so box-to-box differences and clock drift hit all of them alike.

  rows        the default: the walking form of the rows kernel (assemble_q1_lattice_rows_walk_kernel): CSR runs out of the 1-D
              tables, one x-line per 256-thread workgroup, a class per line (lines without interior Dirichlet nodes read no flag)
  oneshot     PYNAMA_LATTICE_ROWS_ONESHOT=1: the one-shot form (assemble_q1_lattice_rows_kernel), flags staged for every line
  no_classes  PYNAMA_LATTICE_ROWS_NO_CLASSES=1: the walking form, every line through the flagged loop
  persistent  PYNAMA_LATTICE_ROWS_MAX_GRID=-1: the walking form with the workgroups the device holds at once, each walking its lines
  grid_half   PYNAMA_LATTICE_ROWS_MAX_GRID=<lines / 2>: two lines per workgroup
  rows_t128   PYNAMA_LATTICE_ROWS_THREADS=128: the one-shot form per 128-thread workgroup
  rows_t512   PYNAMA_LATTICE_ROWS_THREADS=512: ... per 512-thread workgroup
  rows_nl2    PYNAMA_LATTICE_ROWS_LINES=2: two x-lines per 256-thread workgroup (one staging phase for both)
  tile        PYNAMA_NO_LATTICE_ROWS=1: the 7x5x4 tile kernel with the axis tables and the per-tile Dirichlet map
  rows_rhs    `rows` with a full-pattern Arhs target (twice the stores until the target is known clean)
  oneshot_rhs `oneshot` with the same target
  tile_rhs    `tile` with the same target

Per variant: the median assembly time (ctx.timers()) of every round, then median / min / max over the rounds.
usage (GPU box): python tools/lattice_rows_ab.py [nel=215] [rounds=7] [reps=15] [out.json] [variant,variant,..]
A library without the rows kernel (PYNAMA_LIB_PATH=<older build>) runs its tile kernel under every name."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"rows": ({}, False), "oneshot": ({"PYNAMA_LATTICE_ROWS_ONESHOT": "1"}, False),
            "no_classes": ({"PYNAMA_LATTICE_ROWS_NO_CLASSES": "1"}, False), "persistent": ({"PYNAMA_LATTICE_ROWS_MAX_GRID": "-1"}, False),
            "grid_half": ({"PYNAMA_LATTICE_ROWS_MAX_GRID": None}, False), "rows_t128": ({"PYNAMA_LATTICE_ROWS_THREADS": "128"}, False),
            "rows_t512": ({"PYNAMA_LATTICE_ROWS_THREADS": "512"}, False), "rows_nl2": ({"PYNAMA_LATTICE_ROWS_LINES": "2"}, False),
            "tile": ({"PYNAMA_NO_LATTICE_ROWS": "1"}, False),
            "rows_rhs": ({}, True), "oneshot_rhs": ({"PYNAMA_LATTICE_ROWS_ONESHOT": "1"}, True), "tile_rhs": ({"PYNAMA_NO_LATTICE_ROWS": "1"}, True)}


def main():
    nel = int(sys.argv[1]) if len(sys.argv) > 1 else 215
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    out = sys.argv[4] if len(sys.argv) > 4 else None
    if len(sys.argv) > 5:
        for name in [v for v in VARIANTS if v not in sys.argv[5].split(",")]:
            del VARIANTS[name]
    from pynama_amd import _lib
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    dom = DMPlexDom(boxMesh={"nelem": [nel] * 3, "lower": [0, 0, 0], "upper": [1, 1, 1]})
    dom.setFemIndexing(2)
    ctx = dom.ctx
    if "grid_half" in VARIANTS:
        VARIANTS["grid_half"][0]["PYNAMA_LATTICE_ROWS_MAX_GRID"] = str(((nel + 1) ** 2 + 1) // 2)
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    ctx.bc_set(1, dom.boundaryMaskLocal())
    ctx.csr_symbolic()
    A, Arhs = ctx.mat_create(1, 1), ctx.mat_create(1, 1)
    ran = {}

    def run(name, n):
        env, rhs = VARIANTS[name]
        for k, v in env.items():
            os.environ[k] = v
        try:
            t = []
            for _ in range(n):
                ctx.assemble_scalar(_lib.FORM_LAPLACE, A, Arhs if rhs else -1)
                t.append(ctx.timers()["assemble_ms"])
            ran[name] = ctx.assemble_last()
            return float(np.median(t))
        finally:
            for k in env:
                del os.environ[k]

    for name in VARIANTS:                     # warm-up: code objects, the once-per-mesh checks, clocks
        run(name, 10)
    per_round = {name: [] for name in VARIANTS}
    for _ in range(rounds):
        for name in VARIANTS:
            per_round[name].append(run(name, reps))
    res = {"nel": nel, "rounds": rounds, "reps": reps, "source_hash": _lib.source_hash(), "library": os.path.basename(_lib.LIB_PATH),
           "last": ran, "ms": {}}
    for name, t in per_round.items():
        res["ms"][name] = {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": t}
        print("%-10s median %.4f ms  min %.4f  max %.4f  spread %.4f" % (name, np.median(t), min(t), max(t), max(t) - min(t)))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
