"""Pivoting systems for the dense and the banded LU (importable without a GPU): the case table, the builders and the references.

Values go on the node graph of a Q1 box mesh with block size b, in the value layout of include/pynama_hip.h; every stored entry,
the diagonal included, is random (`int`: integers in -8..8, `uni`: uniform in [-1, 1)), so most columns interchange, at distances
up to kl, across the borders of the sub-blocks (8) and panels (64) of pyn_direct_band.hip and of the panels of pyn_direct.hip.
The exact solution holds integers in -4..4 and the right-hand side is A xs (exact for `int`).

The reference is LAPACK in band storage (dgbtrf / dgbtrs); the measure is the normwise backward error
    eta(x) = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf),
the residual formed from the host's copy of A in np.longdouble (64 mantissa bits; without them: exact products and math.fsum per
row).  It does not depend on the conditioning.  A device solution passes when eta(x_dev) <= MARGIN * max(eta(x_ref), eps): between
value kinds and seeds at one shape LAPACK's own eta varies by up to about 4; a blocked elimination with fma in another order is
one more such draw, and 16 leaves room for two of them, while a missed update or a wrong interchange leaves eta many orders of
magnitude above eps.
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import scipy.sparse as sp
from scipy.linalg import lapack

from tests import product_exact as pe

EPS = float(np.finfo(np.float64).eps)
MARGIN = 16.0
PANEL, SUB = 64, 8                      # panel and sub-block width of the two factorisations
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


@dataclass(frozen=True)
class Case:
    nelem: tuple
    b: int
    n: int
    kl: int                             # = ku, as pyn_direct_band_info reports them
    note: str
    kinds: tuple = ("int", "uni")
    main_only: bool = False             # the two largest: only the main eta test
    seed: int = 5

    @property
    def name(self):
        return "x".join(str(k) for k in self.nelem) + f"-b{self.b}"


CASES = [
    Case((1, 1), 1, 4, 3, "n < kl + 1, one short panel", seed=206),   # seed 5: largest interchange distance 2 < 3/4 kl
    Case((1, 30), 1, 62, 3, "single panel, nbp = 62 (not a multiple of 8)"),
    Case((1, 31), 1, 64, 3, "exactly one panel, no trailing update"),
    Case((4, 12), 1, 65, 6, "second panel of one column"),
    Case((3, 31), 1, 128, 5, "two full panels"),
    Case((2, 42), 1, 129, 4, "dense: 2x2 gemm grid with a one-row tail"),
    Case((1, 100), 1, 202, 3, "narrow band (kl + ku < 64) over four panels, nbp = 10 at the end"),
    Case((61, 3), 1, 248, 63, "kl one below the panel width"),
    Case((62, 3), 1, 252, 64, "kl at the panel width"),
    Case((63, 3), 1, 256, 65, "kl one above the panel width"),
    Case((9, 6), 2, 140, 23, "2x2 blocks"),
    Case((5, 7), 3, 144, 23, "3x3 blocks"),
    Case((2, 2, 6), 3, 189, 41, "3-D graph, 27-point rows"),
    Case((20, 20), 1, 441, 22, "dense: trsm over two workgroups, 6x6 gemm grid"),
    Case((1100, 2), 1, 3303, 1102, "kl > 1024 threads of the panel kernel; 52 panels", kinds=("uni",), main_only=True),
    Case((30, 43), 3, 4092, 98, "largest dense solve of the file", kinds=("uni",), main_only=True),
]
BY_NAME = {c.name: c for c in CASES}
MAIN = [(c, k) for c in CASES for k in c.kinds]
MAIN_IDS = [f"{c.name}-{k}" for c, k in MAIN]

SINGULAR_CASE = BY_NAME["1x100-b1"]
ZERO_COLUMNS = (0, 7, 8, 63, 64, 201)
NAN_ENTRIES = ((100, 100), (10, 12), (201, 201))       # diagonal, upper triangle, the last pivot
CACHE_CASES = (BY_NAME["4x12-b1"], BY_NAME["9x6-b2"])


@dataclass
class System:
    br: int
    bc: int
    rowptr: np.ndarray
    colidx: np.ndarray
    val: np.ndarray          # float64, header layout (what product_exact.upload sends)
    R: np.ndarray            # scalar row / column of every stored value
    C: np.ndarray
    A: sp.csr_matrix         # float64 [n, n], explicit zeros kept
    n: int
    kl: int
    ku: int
    xs: np.ndarray           # int64, the exact solution of the `int` kind
    b: np.ndarray            # float64, A xs
    exact_rhs: bool          # every value is an integer: b and sum(b^2) are exact


@dataclass
class Reference:
    info: int
    ipiv: np.ndarray         # 0-based: column k was interchanged with row ipiv[k]
    x: np.ndarray
    eta: float

    @property
    def bar(self):
        return MARGIN * max(self.eta, EPS)


@lru_cache(maxsize=None)
def graph(case):
    """(mesh, rowptr, colidx) of the case's Q1 box mesh"""
    mesh = pe.mesh_of(2, case.nelem)
    rp, ci = pe.host_graph(mesh)
    return mesh, np.asarray(rp, np.int32), np.asarray(ci, np.int32)


def graph_bandwidths(rowptr, colidx, b):
    """(kl, ku) of the scalar matrix: (largest node distance below / above the diagonal) b + b - 1"""
    node = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    d = np.asarray(colidx, np.int64) - node
    return int(-d.min()) * b + b - 1, int(d.max()) * b + b - 1


def draw_values(kind, count, rng):
    if kind == "int":
        return rng.integers(-8, 9, count).astype(np.float64)
    assert kind == "uni", kind
    return rng.uniform(-1.0, 1.0, count)


def system_of(rowptr, colidx, b, val, xs):
    """the scalar system of stored values `val` (header layout) on the graph, with right-hand side A xs"""
    rowptr, colidx = np.asarray(rowptr, np.int32), np.asarray(colidx, np.int32)
    val = np.ascontiguousarray(val, np.float64)
    R, C = pe.storage_index(rowptr, colidx, b, b)
    n = (rowptr.size - 1) * b
    assert val.size == R.size and xs.size == n
    A = sp.csr_matrix((val, (R, C)), shape=(n, n))
    A.sort_indices()
    kl, ku = graph_bandwidths(rowptr, colidx, b)
    exact = bool(np.all(val == np.rint(val)) and np.abs(val).max() < 2.0 ** 20)
    return System(b, b, rowptr, colidx, val, R, C, A, n, kl, ku, xs, A @ xs.astype(np.float64), exact)


def draw_solution(n, rng):
    return rng.integers(-4, 5, n).astype(np.int64)


@lru_cache(maxsize=None)
def build(case, kind):
    _, rp, ci = graph(case)
    rng = np.random.default_rng(case.seed)
    val = draw_values(kind, int(rp[-1]) * case.b * case.b, rng)
    return system_of(rp, ci, case.b, val, draw_solution((rp.size - 1) * case.b, rng))


def band_storage(s):
    """LAPACK's ab[kl + ku + i - j, j] = A[i, j] with kl extra rows on top for the fill of the interchanges"""
    ab = np.zeros((2 * s.kl + s.ku + 1, s.n), order="F")
    ab[s.kl + s.ku + s.R - s.C, s.C] = s.val
    return ab


def _two_prod(a, b):
    """a b = p + e exactly (Dekker; no overflow at these magnitudes)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def residual_inf(s, x, b=None, longdouble=None):
    """||b - A x||_inf from the host's A beyond double precision"""
    b = s.b if b is None else b
    A = s.A
    use_ld = LONGDOUBLE_OK if longdouble is None else longdouble
    if use_ld:
        L = np.longdouble
        prod = A.data.astype(L) * np.asarray(x, np.float64).astype(L)[A.indices]
        r = b.astype(L) - np.add.reduceat(prod, A.indptr[:-1])
        return float(np.abs(r).max())
    p, e = _two_prod(A.data, np.asarray(x, np.float64)[A.indices])
    worst = 0.0
    for i in range(s.n):
        lo, hi = A.indptr[i], A.indptr[i + 1]
        worst = max(worst, abs(math.fsum([b[i], *(-p[lo:hi]), *(-e[lo:hi])])))
    return worst


def scale_of(s, x, b=None):
    """||A||_inf ||x||_inf + ||b||_inf"""
    b = s.b if b is None else b
    return float(abs(s.A).sum(axis=1).max()) * float(np.abs(x).max()) + float(np.abs(b).max())


def eta(s, x, b=None, longdouble=None):
    """normwise backward error of x; nan / inf for a solution that is not finite"""
    x = np.asarray(x, np.float64)
    if not np.all(np.isfinite(x)):
        return float("nan")
    return residual_inf(s, x, b, longdouble) / scale_of(s, x, b)


def lapack_factor(s):
    lu, ipiv, info = lapack.dgbtrf(band_storage(s), s.kl, s.ku)
    return lu, np.asarray(ipiv, np.int64), int(info)


def reference(s, b=None):
    """dgbtrf / dgbtrs of the system; x and eta only where the factorisation succeeded"""
    b = s.b if b is None else b
    lu, ipiv, info = lapack_factor(s)
    if info != 0:
        return Reference(info, ipiv, None, float("nan"))
    x, info2 = lapack.dgbtrs(lu, s.kl, s.ku, b, ipiv.astype(np.int32))
    assert info2 == 0
    return Reference(info, ipiv, x, eta(s, x, b))


@lru_cache(maxsize=None)
def reference_of(case, kind):
    return reference(build(case, kind))


def pivot_stats(ipiv):
    """share of the columns that interchange, the largest distance, whether one crosses a sub-block / a panel border"""
    i = np.arange(ipiv.size)
    assert np.all(ipiv >= i)
    return {"share": float(np.mean(ipiv != i)), "dist": int((ipiv - i).max()),
            "cross_sub": bool(np.any(ipiv // SUB != i // SUB)), "cross_panel": bool(np.any(ipiv // PANEL != i // PANEL))}


def column_entries(s, k):
    """(rows, values) of the stored entries of scalar column k"""
    m = s.C == k
    return s.R[m], s.val[m]


def with_values(s, val, xs=None):
    """the same graph with other stored values (and, with xs, another exact solution)"""
    return system_of(s.rowptr, s.colidx, s.br, val, s.xs if xs is None else xs)


def true_resid_bound(s, ref_bar, x, b=None):
    """what eta <= ref_bar implies for ||b - A x||_2 / ||b||_2:  sqrt(n) eta_bar (||A||_inf ||x||_inf + ||b||_inf) / ||b||_2"""
    b = s.b if b is None else b
    return math.sqrt(s.n) * ref_bar * scale_of(s, x, b) / float(np.linalg.norm(b))
