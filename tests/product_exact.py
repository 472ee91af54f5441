"""Integer-valued matrices and vectors for exact tests of the product kernels (importable without a GPU).

Every value is a small integer, so every partial sum of y = A x and of b.(A b) is an integer far below 2^53: any summation
order, with or without fma, gives the same bits, and the tests compare with `==`.  The matrices follow the value layout of
include/pynama_hip.h on the node graph of a mesh:  val[(rowptr[i]*br + p*len_i + k)*bc + q].
"""
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from oracle import fem_oracle as fo


def storage_index(rowptr, colidx, br, bc):
    """scalar (row, column) of every stored value, in storage order"""
    rowptr = np.asarray(rowptr, np.int64)
    lens = np.diff(rowptr)
    n = lens.size
    per = lens * br * bc
    node = np.repeat(np.arange(n), per)
    o = np.arange(per.sum()) - np.repeat(rowptr[:-1] * br * bc, per)
    ln = np.repeat(lens, per)
    p, rem = o // (ln * bc), o % (ln * bc)
    k, q = rem // bc, rem % bc
    col_node = np.asarray(colidx, np.int64)[np.repeat(rowptr[:-1], per) + k]
    return node * br + p, col_node * bc + q


@dataclass
class Exact:
    br: int
    bc: int
    rowptr: np.ndarray
    colidx: np.ndarray
    n_cols_nodes: int
    val: np.ndarray          # int64, header layout
    A: sp.csr_matrix         # int64 [n_rows*br, n_cols_nodes*bc]
    x: np.ndarray            # int64 [n_cols_nodes*bc]
    y: np.ndarray            # int64, A x
    b: np.ndarray = None     # square shapes: int64 [n_rows*br], no zero entry
    Af: sp.csr_matrix = None # A with the ghost columns folded onto owned nodes
    pap: int = 0             # b.(Af b)
    bb: int = 0

    def x1(self):
        """first CG iterate from x0 = 0 without a preconditioner: fl(fl(bb / pap) * b)"""
        return np.float64(self.bb) / np.float64(self.pap) * self.b.astype(np.float64)


def build(rowptr, colidx, br, bc, n_cols_nodes=None, fold=None, seed=0):
    """Integer block-CSR matrix on the graph (rows = owned nodes, columns = local nodes) with its exact references.
    Off-diagonals from {-3..3}; without ghost columns a square shape is made symmetric (T + T^T on the scalar level); the scalar
    diagonal of a square shape is 1 + max(row, column) sum of |off-diagonals|, the column sums taken after `fold` (local node ->
    owned node; default: no ghosts) has folded the ghost columns onto owned nodes, so that b.(A b) > 0 there as well."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n = rowptr.size - 1
    ncn = n if n_cols_nodes is None else int(n_cols_nodes)
    rng = np.random.default_rng(1000 + seed)
    R, C = storage_index(rowptr, colidx, br, bc)
    shape = (n * br, ncn * bc)
    T = sp.coo_matrix((rng.integers(-3, 4, R.size), (R, C)), shape=shape).tocsr().astype(np.int64)
    square = br == bc
    if square and ncn == n:
        T = (T + T.T).tocsr()
    if square:
        fmap = np.arange(ncn) if fold is None else np.asarray(fold, np.int64)
        assert ncn == n or fold is None or fmap.size == ncn
        if fold is None and ncn > n:        # detached ghosts: no owner known, they stay off-diagonal columns
            F = None
        else:
            fs = (fmap[:, None] * bc + np.arange(bc)[None, :]).ravel()
            F = sp.csr_matrix((np.ones(fs.size, np.int64), (np.arange(fs.size), fs)), shape=(ncn * bc, n * bc))
        m = n * br
        ar = np.arange(m)

        def dmat(v):
            return sp.coo_matrix((v, (ar, ar)), shape=shape).tocsr()

        signed = (T - dmat(T.diagonal())).tocsr()
        off = abs(signed)
        rows = np.asarray(off.sum(axis=1)).ravel()
        offc = off if F is None else (off @ F).tocsr()
        cols = np.asarray(offc.sum(axis=0)).ravel()[:m]
        T = (signed + dmat(1 + np.maximum(rows, cols))).tocsr().astype(np.int64)
    T.sort_indices()
    val = np.asarray(T[R, C]).ravel().astype(np.int64)
    x = rng.integers(-4, 5, ncn * bc).astype(np.int64)
    ex = Exact(br, bc, rowptr.astype(np.int32), colidx.astype(np.int32), ncn, val, T, x, T @ x)
    if square and (ncn == n or fold is not None):
        b = rng.integers(1, 5, n * br).astype(np.int64) * rng.choice(np.array([-1, 1]), n * br)
        ex.b = b
        ex.Af = T if ncn == n else (T @ F).tocsr()
        ex.pap = int(b @ (ex.Af @ b))
        ex.bb = int(b @ b)
    return ex


def upload(ctx, mid, ex):
    """one mat_add_values(insert=True) per node row: br rows, len*bc columns"""
    br, bc = ex.br, ex.bc
    pr, pc = np.arange(br, dtype=np.int32), np.arange(bc, dtype=np.int32)
    v = ex.val.astype(np.float64)
    for i in range(ex.rowptr.size - 1):
        lo, hi = int(ex.rowptr[i]), int(ex.rowptr[i + 1])
        cols = (ex.colidx[lo:hi, None] * bc + pc[None, :]).ravel()
        ctx.mat_add_values(mid, i * br + pr, cols, v[lo * br * bc:hi * br * bc], insert=True)


# ---- meshes --------------------------------------------------------------------------------------------------------
def mesh_of(ngl, nelem):
    return fo.box_mesh(list(nelem), [0.0] * len(nelem), [1.0] * len(nelem), ngl)


def host_graph(mesh, n_owned=None):
    """the node graph the device builds, from the connectivity (rows of the owned nodes)"""
    rp, ci = fo.node_graph(mesh)
    if n_owned is None:
        return rp, ci
    return rp[:n_owned + 1], ci[:rp[n_owned]]


def hole_mesh(nelem):
    """One rank that is its own neighbour (Q1): ghost copies of the node planes (2-D: rows) 1 and nz-2, referenced by the bottom
    and the top cell layer, so that the rows needing ghosts are a prefix and a suffix of the slices.
    Returns (cut mesh, n_owned, send, fold)."""
    mesh = mesh_of(2, nelem)
    dim = len(nelem)
    N = mesh.n_node
    pp = int(np.prod([k + 1 for k in nelem[:-1]]))
    nzp = nelem[-1] + 1
    send = np.concatenate([np.arange(pp, 2 * pp), np.arange((nzp - 2) * pp, (nzp - 1) * pp)])
    ghost_of = np.full(N, -1)
    ghost_of[send] = N + np.arange(2 * pp)
    conn = mesh.conn.copy()
    cpl = int(np.prod(nelem[:-1]))
    for layer, plane in ((0, 1), (nelem[-1] - 1, nzp - 2)):
        blk = conn[layer * cpl:(layer + 1) * cpl]
        hit = (blk >= plane * pp) & (blk < (plane + 1) * pp)
        blk[hit] = ghost_of[blk][hit]
    xyz = np.vstack([mesh.xyz, mesh.xyz[send]])
    cut = fo.BoxMesh(dim, 2, tuple(nelem), mesh.lattice, conn.astype(np.int32), xyz, mesh.boundary, mesh.borders)
    fold = np.concatenate([np.arange(N), send])
    return cut, N, send.astype(np.int32), fold


# ---- the cases -----------------------------------------------------------------------------------------------------
RAW, SELL, SELLP, SELLB_X, SELLB_D, CSRL, CSRLB, BCSR = 1, 2, 3, 4, 5, 6, 7, 8
FAMILY = {0: "none", RAW: "raw", SELL: "sell", SELLP: "sellp", SELLB_X: "sellb-explicit", SELLB_D: "sellb-dict", CSRL: "csrl",
          CSRLB: "csrlb", BCSR: "bcsr"}


@dataclass
class Case:
    name: str
    block: tuple
    ngl: int
    nelem: tuple
    one_off: tuple                 # (family, param) expected of pyn_spmv; param None = not checked (bcsr: from the knobs)
    solver: tuple = None           # (family, param) expected inside pyn_solve (square shapes), None: plain only
    env: dict = field(default_factory=dict)
    max_grid1: bool = False        # run once more with PYNAMA_SPMV_MAX_GRID=1


CASES = [
    Case("1x1-q1-2d", (1, 1), 2, (33, 31), (CSRL, 27), (CSRL, 27), max_grid1=True),
    Case("1x1-q1-3d", (1, 1), 2, (7, 6, 5), (CSRL, 27), (CSRL, 27)),
    Case("1x1-ngl3-2d", (1, 1), 3, (5, 4), (CSRL, 27), (CSRL, 27)),
    Case("1x1-ngl4-strip", (1, 1), 4, (1, 40), (CSRL, 32), (CSRL, 32)),
    Case("1x1-q1-2d-image", (1, 1), 2, (33, 31), (SELLP, 0), (SELLP, 0), env={"PYNAMA_SELL_IMAGE": "1"}, max_grid1=True),
    Case("1x1-q1-3d-image", (1, 1), 2, (7, 6, 5), (SELLP, 0), (SELLP, 0), env={"PYNAMA_SELL_IMAGE": "1"}, max_grid1=True),
    Case("1x1-q1-3d-nopat", (1, 1), 2, (7, 6, 5), (SELL, 0), (SELL, 0), env={"PYNAMA_NO_PATTERNS": "1"}),
    Case("1x1-ngl4-2d", (1, 1), 4, (3, 3), (BCSR, None), (SELL, 0)),
    Case("1x1-ngl3-3d", (1, 1), 3, (2, 2, 2), (BCSR, None), (SELL, 0)),
    Case("1x1-ngl3-3d-minavg0", (1, 1), 3, (2, 2, 2), (BCSR, None), (BCSR, None), env={"PYNAMA_BCSR_MIN_AVG": "0"}),
    Case("1x1-q1-2d-nosell", (1, 1), 2, (9, 7), (RAW, 0), (RAW, 0), env={"PYNAMA_NO_SELL": "1"}),
    Case("2x2-q1-2d", (2, 2), 2, (33, 31), (CSRLB, 18), (CSRLB, 18), max_grid1=True),
    Case("2x2-ngl3-strip", (2, 2), 3, (1, 40), (CSRLB, 32), (CSRLB, 32)),
    Case("2x2-ngl3-2d", (2, 2), 3, (9, 7), (CSRLB, 50), (CSRLB, 50), max_grid1=True),
    Case("2x2-ngl4-strip", (2, 2), 4, (1, 40), (BCSR, None), (SELLB_D, 2)),
    Case("2x2-q1-2d-nocsrlb", (2, 2), 2, (33, 31), (BCSR, None), (SELLB_D, 2), env={"PYNAMA_NO_CSRLB": "1"}),
    Case("2x2-q1-2d-blocksell", (2, 2), 2, (33, 31), (SELLB_D, 2), (SELLB_D, 2), env={"PYNAMA_BLOCK_SELL": "1"}),
    Case("2x2-q1-2d-nopat", (2, 2), 2, (33, 31), (BCSR, None), (SELLB_X, 2), env={"PYNAMA_NO_PATTERNS": "1"}),
    Case("3x3-q1-3d", (3, 3), 2, (4, 3, 5), (BCSR, None), (SELLB_D, 3), max_grid1=True),
    Case("3x3-q1-3d-minavg0", (3, 3), 2, (4, 3, 5), (BCSR, None), (BCSR, None), env={"PYNAMA_BCSR_MIN_AVG": "0"}, max_grid1=True),
] + [Case(f"{r}x{c}-q1-2d", (r, c), 2, (9, 7), (BCSR, None)) for r, c in ((2, 1), (3, 1), (1, 2), (1, 3), (3, 2), (2, 3))] \
  + [Case(f"{r}x{c}-q1-3d", (r, c), 2, (4, 3, 5), (BCSR, None)) for r, c in ((6, 3), (3, 6))]

# 3b: rank r of 2, detached (ghost columns, no hole): (block, ngl, nelem, expected one-off family and parameter)
GHOST_CASES = [((1, 1), 2, (4, 3, 6), (CSRL, 27)), ((3, 3), 2, (4, 3, 6), (BCSR, None)), ((2, 2), 3, (5, 6), (CSRLB, 50))]
# 3c: the hole: (name, block, nelem, env, expected solver family and parameter)
HOLE_CASES = [("1x1", (1, 1), (8, 8, 12), {}, (CSRL, 27)),
              ("3x3-sellb", (3, 3), (8, 8, 12), {}, (SELLB_D, 3)),
              ("3x3-bcsr", (3, 3), (8, 8, 12), {"PYNAMA_BCSR_MIN_AVG": "0"}, (BCSR, None)),
              ("2x2-2d", (2, 2), (8, 12), {}, (CSRLB, 18))]
