#!/usr/bin/env python3
"""Same-process A/B of the parallelepiped lattice tile kernel on the bench mesh (nel^3 Q1 hexahedra, Dirichlet faces): the variants
are alternated round by round on ONE context, so box-to-box differences and clock drift hit all of them alike.

  axes        the default: element geometry from the axis tables (rectilinear mesh), flag loads only in tiles whose bit of the
              per-tile Dirichlet map is set
  axes_flags  PYNAMA_NO_LATTICE_TILEBC=1: `axes` with the flag loads in every tile
  loads       PYNAMA_NO_LATTICE_AXES=1: four corner loads per element
  ablate32    PYNAMA_LATTICE_ABLATE=32: the coordinate-loading kernel with the loads cut out (the ceiling of `axes`; wrong values)
  axes_noflag PYNAMA_LATTICE_ABLATE=64: `axes` without the Dirichlet flag loads (the ceiling of a per-tile bitmap; wrong rows)

Per variant: the median assembly time (ctx.timers()) of every round, then median / min / max over the rounds.
usage (GPU box): python tools/lattice_axes_ab.py [nel=215] [rounds=7] [reps=15] [out.json]
A library without the table variant (PYNAMA_LIB_PATH=<older build>) runs its one kernel under `axes`, `axes_flags`, `loads` and `axes_noflag`."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"axes": {}, "axes_flags": {"PYNAMA_NO_LATTICE_TILEBC": "1"}, "loads": {"PYNAMA_NO_LATTICE_AXES": "1"}, "ablate32": {"PYNAMA_LATTICE_ABLATE": "32"},
            "axes_noflag": {"PYNAMA_LATTICE_ABLATE": "64"}}


def main():
    nel = int(sys.argv[1]) if len(sys.argv) > 1 else 215
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    out = sys.argv[4] if len(sys.argv) > 4 else None
    from pynama_amd import _lib
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    dom = DMPlexDom(boxMesh={"nelem": [nel] * 3, "lower": [0, 0, 0], "upper": [1, 1, 1]})
    dom.setFemIndexing(2)
    ctx = dom.ctx
    for t in Spectral(2, 3).deviceTables():
        ctx.tables_set(*t)
    ctx.bc_set(1, dom.boundaryMaskLocal())
    ctx.csr_symbolic()
    A = ctx.mat_create(1, 1)

    def run(env, n):
        for k, v in env.items():
            os.environ[k] = v
        try:
            t = []
            for _ in range(n):
                ctx.assemble_scalar(_lib.FORM_LAPLACE, A, -1)
                t.append(ctx.timers()["assemble_ms"])
            return float(np.median(t))
        finally:
            for k in env:
                del os.environ[k]

    for env in VARIANTS.values():             # warm-up: code objects, the once-per-mesh checks, clocks
        run(env, 10)
    per_round = {name: [] for name in VARIANTS}
    for _ in range(rounds):
        for name, env in VARIANTS.items():
            per_round[name].append(run(env, reps))
    res = {"nel": nel, "rounds": rounds, "reps": reps, "source_hash": _lib.source_hash(), "library": _lib.LIB_PATH,
           "last": ctx.assemble_last(), "ms": {}}
    for name, t in per_round.items():
        res["ms"][name] = {"median": float(np.median(t)), "min": min(t), "max": max(t), "rounds": t}
        print("%-12s median %.4f ms  min %.4f  max %.4f  spread %.4f" % (name, np.median(t), min(t), max(t), max(t) - min(t)))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
