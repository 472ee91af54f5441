"""Meshes away from the unit box, with references that need no extended precision (host only).

Every geometry-reading kernel is invariant under translation and homogeneous under scaling, and both maps can be made EXACT in
binary64, so the float64 oracle on the base mesh is the reference for the device on the transformed one:

  translate(L)   t = 2^L (1, -1, 1.5)[:dim] has one or two mantissa bits per component.  y = fl(x + t), xb = y - t: the subtraction
                 is exact, so the mesh y is the exact translate of the mesh xb (asserted: xb + t == y bit for bit, and y - t == xb in
                 long double).  Reference: the oracle on xb, which sits at the origin and has no cancellation.  Device: y.
  scale(p)       s = 2^p maps every coordinate exactly; every operator then scales by an exact power of two (scale_power).
  stretch(pw)    the axes scaled by 2^pw[d], exact as well; the aspect ratio changes, so the reference is the oracle on the same mesh.

A Pair holds `base` (the reference's mesh), `moved` (the device's mesh), the same for a point set, and the exact factor.  The mesh
builders keep the coordinates of the affine families dyadic (cell sizes and shears that are multiples of 2^-6), so that their
translates stay exactly affine and a detector has no rounding to excuse it; the jittered, bent, imported and simplicial meshes keep
their full mantissas."""
import copy
import functools
from dataclasses import dataclass

import numpy as np

from oracle import fem_oracle as fo
from tests import ho_general_meshes as gm
from tests.util import rel_err, sp_rel_err

EPS = np.finfo(np.float64).eps
FP_TOL = 2e-13                       # the bar of every existing oracle-parity test (tests/test_gpu_kernels.py, test_gpu_ho3.py, ...)
MARGIN = 16.0                        # device error allowed in units of the oracle's own sensitivity to the translation
T_DIR = (1.0, -1.0, 1.5)
STRETCHES = ((8, 0, -8), (-8, 0, 8))


# ---- the three transformations -------------------------------------------------------------------------------------------------------
@dataclass
class Pair:
    name: str
    kind: str                        # "translate" | "scale" | "stretch"
    base: object                     # the reference's mesh (translate: xb; scale: x; stretch: the moved mesh itself)
    moved: object                    # the device's mesh
    s: float = 1.0                   # scale: the factor
    shift: object = None             # translate: t
    axes: object = None              # stretch / scale: the factor per axis

    def points(self, P):
        """(base, moved) images of the points P [n, dim], built like the mesh's nodes"""
        P = np.asarray(P, dtype=np.float64)
        if self.kind == "translate":
            y = P + self.shift
            return _exact_translate(y, self.shift), y
        y = P * self.axes
        assert np.array_equal(y / self.axes, P)
        return (P if self.kind == "scale" else y), y


def with_xyz(mesh, xyz):
    out = copy.copy(mesh)
    out.xyz = np.ascontiguousarray(xyz)
    return out


def _exact_translate(y, t):
    """xb = y - t with the two equalities that make y the exact translate of xb"""
    xb = y - t
    assert np.array_equal(xb + t, y), "xb + t != y: the case is not an exact translation"
    assert np.array_equal(y.astype(np.longdouble) - t.astype(np.longdouble), xb.astype(np.longdouble)), "y - t is not exact"
    return xb


def shift_of(dim, L):
    return 2.0 ** L * np.array(T_DIR[:dim])


def translate(L):
    def apply(mesh):
        t = shift_of(mesh.dim, L)
        y = mesh.xyz + t
        return Pair(f"translate({L})", "translate", with_xyz(mesh, _exact_translate(y, t)), with_xyz(mesh, y), shift=t)
    apply.__name__ = f"translate{L}"
    return apply


def scale(p):
    def apply(mesh):
        s = 2.0 ** p
        y = mesh.xyz * s
        assert np.array_equal(y / s, mesh.xyz) and np.isfinite(y).all()
        return Pair(f"scale({p})", "scale", mesh, with_xyz(mesh, y), s=s, axes=np.full(mesh.dim, s))
    apply.__name__ = f"scale{p:+d}"
    return apply


def stretch(powers):
    def apply(mesh):
        a = 2.0 ** np.array(powers[:mesh.dim], dtype=np.float64)
        y = mesh.xyz * a
        assert np.array_equal(y / a, mesh.xyz)
        moved = with_xyz(mesh, y)
        return Pair(f"stretch{tuple(powers[:mesh.dim])}", "stretch", moved, moved, axes=a)
    apply.__name__ = "stretch" + "".join("p" if q > 0 else "m" if q < 0 else "0" for q in powers)
    return apply


TRANSFORMS = {"translate10": translate(10), "translate20": translate(20), "scale-24": scale(-24), "scale+24": scale(24),
              "stretch_pm": stretch(STRETCHES[0]), "stretch_mp": stretch(STRETCHES[1])}
ISOTROPIC = ("translate10", "translate20", "scale-24", "scale+24")


# ---- exact factors under x -> s x ----------------------------------------------------------------------------------------------------
def scale_power(op, dim):
    """the operator `op` of the mesh s x is s^power times that of x (free rows; the unit rows of imposed DOFs do not scale)"""
    return {"laplace": dim - 2, "K": dim - 2, "Krhs": dim - 2, "Rw": dim - 1, "mass": dim,
            "SrT_raw": dim - 1, "DivSrT_raw": dim - 1, "Curl_raw": dim - 1,          # before the lumped row scaling (a mass: s^dim)
            "SrT": -1, "DivSrT": -1, "Curl": -1,
            "volume": dim, "value": dim, "square": dim, "grad2": dim - 2, "div2": dim - 2, "curl2": dim - 2}[op]


def integral_powers(dim, bs, grad):
    """scale_power per entry of pyn_integrate's flat layout: volume, value[bs], square[bs], grad2[bs], div2, curl2[dim_w]"""
    p = [dim] * (1 + 2 * bs)
    if grad:
        p += [dim - 2] * bs
        if bs == dim:
            p += [dim - 2] * (1 + (3 if dim == 3 else 1))
    return np.array(p, dtype=np.float64)


# ---- conditioning ----------------------------------------------------------------------------------------------------------------------
def kappa(mesh):
    """|x|_max / h_min, h_min the shortest distance between two corners of a cell: eps * kappa is the scale of the cancellation
    error of anything formed from absolute coordinates"""
    nc = mesh.nc or 2 ** mesh.dim
    X = mesh.xyz[mesh.conn[:, :nc]]
    d = np.linalg.norm(X[:, :, None, :] - X[:, None, :, :], axis=3)
    d[:, np.arange(nc), np.arange(nc)] = np.inf
    return float(np.abs(mesh.xyz).max() / d.min())


def oracle_sensitivity(fn, pair):
    """the float64 reference `fn(mesh) -> {name: matrix or vector}` on the moved mesh against itself on the base mesh, in the
    suite's max-norm measures: what absolute coordinates cost a straightforward float64 evaluation.  Also returns the base result"""
    ref, far = fn(pair.base), fn(pair.moved)
    return {k: err_of(far[k], ref[k]) for k in ref}, ref


def err_of(a, b):
    return sp_rel_err(a, b) if hasattr(b, "nnz") else rel_err(a, b)


def translate_bound(e_o):
    return max(FP_TOL, MARGIN * e_o)


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
SHEAR = np.array([[1.0, 0.25, -0.25], [0.125, 1.0, 0.25], [-0.125, 0.25, 1.0]])      # dyadic: an affine image stays exactly affine
RECT_STEPS = ((1, 2, 1, 3, 2, 1, 2), (2, 1, 1, 3, 2, 1, 1), (1, 3, 2, 1, 2, 2, 1))  # in units of 2^-4


def dyadic_box(nelem, ngl):
    """fo.box_mesh with cells of size 2^-3: every corner a multiple of 2^-3"""
    return fo.box_mesh(list(nelem), [0.0] * len(nelem), [n / 8.0 for n in nelem], ngl)


def rectilinear_box(nelem):
    """Q1 lattice with unequal dyadic steps per axis, every coordinate copied from a 1-D table"""
    mesh = dyadic_box(nelem, 2)
    ax = [np.concatenate([[0.0], np.cumsum(RECT_STEPS[d][:n])]) / 16.0 for d, n in enumerate(nelem)]
    lat = [n + 1 for n in nelem]
    ids = np.arange(mesh.n_node)
    cols = [ax[0][ids % lat[0]], ax[1][(ids // lat[0]) % lat[1]]] + ([ax[2][ids // (lat[0] * lat[1])]] if len(nelem) == 3 else [])
    return with_xyz(mesh, np.stack(cols, axis=1))


def sheared_box(nelem, ngl):
    mesh = dyadic_box(nelem, ngl)
    dim = mesh.dim
    assert np.linalg.det(SHEAR[:dim, :dim]) > 0
    return with_xyz(mesh, mesh.xyz @ SHEAR[:dim, :dim].T)


def no_boundary(mesh):
    out = copy.copy(mesh)
    out.boundary = np.zeros(0, dtype=np.int64)
    return out


@functools.lru_cache(maxsize=None)
def tables_of(dim, ngl, simplex):
    return fo.SimplexTables(dim) if simplex else fo.Tables(ngl, dim)


def is_simplex(mesh):
    return bool(mesh.nc and mesh.nc == mesh.dim + 1)


def tables(mesh):
    return tables_of(mesh.dim, mesh.ngl, is_simplex(mesh))


# ---- the oracle's matrices of a mesh ---------------------------------------------------------------------------------------------------
def oracle_matrices(mesh, masked, ops):
    """{name: scipy matrix} for the names in ops, out of: laplace, Arhs, mass, K, Krhs, Rw, SrT, DivSrT, Curl.  masked: the mesh's
    boundary nodes are imposed (every component), else nothing is"""
    m = mesh if masked else no_boundary(mesh)
    tb = tables(mesh)
    out = {}
    if "laplace" in ops or "Arhs" in ops:
        r = fo.assemble_scalar(m, tb, "laplace", dirichlet=m.boundary if masked else None)
        out["laplace"], out["Arhs"] = r["A"], r["Arhs"]
    if "mass" in ops:
        out["mass"] = fo.assemble_scalar(m, tb, "mass", dirichlet=m.boundary if masked else None)["A"]
    if {"K", "Krhs", "Rw"} & set(ops):
        out.update(fo.assemble_kle_freeslip(m, tb) if masked else _kle_nothing_imposed(mesh, tb))
    if {"SrT", "DivSrT", "Curl"} & set(ops):
        r = fo.assemble_operators(mesh, tb)
        out.update({k: r[k] for k in ("SrT", "DivSrT", "Curl")})
    return {k: v for k, v in out.items() if k in ops}


def _kle_nothing_imposed(mesh, tb):
    """K, Krhs (empty), Rw of fo.assemble_kle_freeslip with no imposed DOF (its own routine takes a non-empty node set)"""
    dim, dw, n = tb.dim, tb.dim_w, mesh.n_node
    Ke, Rwe, _ = fo.elem_kle_matrices(tb, mesh.corners())
    vdof, wdof = fo.dof_indices(mesh.conn, dim), fo.dof_indices(mesh.conn, dw)
    K = fo._scatter((n * dim, n * dim), np.broadcast_to(vdof[:, :, None], Ke.shape), np.broadcast_to(vdof[:, None, :], Ke.shape), Ke)
    Rw = fo._scatter((n * dim, n * dw), np.broadcast_to(vdof[:, :, None], Rwe.shape), np.broadcast_to(wdof[:, None, :], Rwe.shape), Rwe)
    return {"K": K, "Krhs": 0.0 * K, "Rw": Rw}


def free_rows(M, mesh, ndof_rows):
    """the rows of the DOFs that are not imposed (boundary nodes imposed, every component)"""
    keep = np.ones(mesh.n_node, bool)
    keep[mesh.boundary] = False
    return M[np.nonzero(np.repeat(keep, ndof_rows))[0]]


def imposed_rows_are_unit(M, mesh, ndof):
    """rows of imposed DOFs of a square matrix hold 1 on the diagonal and nothing else"""
    import scipy.sparse as sps
    idx = (np.asarray(mesh.boundary)[:, None] * ndof + np.arange(ndof)).ravel()
    D = M.tocsr()[idx] - sps.identity(M.shape[0], format="csr")[idx]
    return D.nnz == 0 or abs(D).max() == 0.0


# ---- the table of cases: one per kernel family -----------------------------------------------------------------------------------------
KLE_OPS, SCALAR_OPS, OPERATOR_OPS = ("K", "Krhs", "Rw"), ("laplace", "mass"), ("SrT", "DivSrT", "Curl")


@dataclass(frozen=True)
class AssemblyCase:
    name: str
    build: object                    # () -> mesh
    kle: str                         # kernel family (pynama_amd._lib.ASSEMBLY_KINDS) expected of K / Krhs / Rw on the BASE mesh
    laplace: str                     # ... of the scalar Laplacian
    operators: str = ""              # ... of SrT / DivSrT / Curl ("": not run on this mesh)
    require: tuple = ()              # environment switches that make the library refuse another family
    plan: tuple = ()                 # patch-plan tile: the tiled kernels with a user plan
    closed: int = 0                  # K and Rw took the closed forms of affine cells (slots k_closed, rw_closed of assemble_last)
    laplace_closed: int = 0          # ... and the scalar Laplacian (slot k_closed)
    geometry: tuple = ()             # (affine, diag) the row-run geometry pre-pass must find: diag 1 the diagonal forms of J^-1
                                     # (axis-aligned cells), 0 the full J^-1; (): only compared between the base and the moved mesh


ASSEMBLY_CASES = [
    AssemblyCase("q1_uniform_543", lambda: dyadic_box([5, 4, 3], 2), "kle_lattice", "lattice", "rowrun", closed=1, laplace_closed=1, geometry=(1, 1)),
    AssemblyCase("q1_uniform_213", lambda: dyadic_box([2, 1, 3], 2), "kle_lattice", "lattice", "rowrun", closed=1, laplace_closed=1, geometry=(1, 1)),
    AssemblyCase("q1_rectilinear_543", lambda: rectilinear_box([5, 4, 3]), "kle_lattice", "lattice", "rowrun",
                 require=("PYNAMA_LATTICE_ROWS_REQUIRE",), closed=1, laplace_closed=1, geometry=(1, 1)),
    AssemblyCase("q1_jittered_543", lambda: fo.box_mesh([5, 4, 3], [0.0] * 3, [1.0, 0.8, 1.1], 2, jitter=0.2), "kle_lattice", "march",
                 "generic"),
    AssemblyCase("q1_sheared_543", lambda: sheared_box([5, 4, 3], 2), "kle_lattice", "lattice", "rowrun", closed=1, laplace_closed=1, geometry=(1, 0)),
    AssemblyCase("q1_sheared_543_plan", lambda: sheared_box([5, 4, 3], 2), "patch", "patch", plan=(3, 3, 3), closed=1, laplace_closed=1),
    AssemblyCase("q1_box2d_54", lambda: dyadic_box([5, 4], 2), "rowrun", "rowrun", "rowrun", require=("PYNAMA_HO3_REQUIRE",), closed=1, laplace_closed=1, geometry=(1, 1)),
    AssemblyCase("ngl3_box2d_54", lambda: dyadic_box([5, 4], 3), "rowrun", "rowrun", "rowrun", require=("PYNAMA_HO3_REQUIRE",), closed=1, laplace_closed=1, geometry=(1, 1)),
    AssemblyCase("ngl3_box3d_323", lambda: dyadic_box([3, 2, 3], 3), "rowrun", "rowrun", "rowrun", require=("PYNAMA_HO3_REQUIRE",), closed=1, laplace_closed=1, geometry=(1, 1)),
    AssemblyCase("ngl3_sheared2d_54", lambda: sheared_box([5, 4], 3), "rowrun", "rowrun", "rowrun", require=("PYNAMA_HO3_REQUIRE",), closed=1, laplace_closed=1, geometry=(1, 0)),
    AssemblyCase("ngl3_sheared3d_323", lambda: sheared_box([3, 2, 3], 3), "rowrun", "rowrun", "rowrun",
                 require=("PYNAMA_HO3_REQUIRE",), closed=1, laplace_closed=1, geometry=(1, 0)),
    AssemblyCase("ngl4_box2d_32", lambda: dyadic_box([3, 2], 4), "generic", "generic", "generic"),
    AssemblyCase("ngl4_box3d_222", lambda: dyadic_box([2, 2, 2], 4), "generic", "generic", "generic"),
    AssemblyCase("ngl3_bent2d_54", lambda: gm.bent_lattice(2, [5, 4], 3, seed=3), "generic", "generic", "generic", geometry=(0, 0)),
    AssemblyCase("ngl3_bent3d_323", lambda: gm.bent_lattice(3, [3, 2, 3], 3, seed=3), "generic", "generic", "generic", geometry=(0, 0)),
    AssemblyCase("ngl4_bent2d_32", lambda: gm.bent_lattice(2, [3, 2], 4, seed=3), "generic", "generic", "generic"),
    AssemblyCase("triangles_54", lambda: fo.simplex_box_mesh([5, 4], [0.0, 0.0], [1.0, 0.8], jitter=0.2, permute_seed=7), "generic",
                 "p1"),
    AssemblyCase("tetrahedra_323", lambda: fo.simplex_box_mesh([3, 2, 3], [0.0] * 3, [1.0, 0.8, 1.1], jitter=0.2, permute_seed=7),
                 "generic", "patch"),
]


@dataclass(frozen=True)
class MatfreeCase:
    name: str
    build: object
    op: str                          # MATFREE_* name in pynama_amd._lib
    scalar: bool = False
    diag: int = -1                   # second-order lattices: 1 the operator must take the diagonal form of J^-1, 0 the full one


MATFREE_CASES = [
    MatfreeCase("q1_laplace_543", lambda: fo.box_mesh([5, 4, 3], [0.0] * 3, [1.0, 0.8, 1.1], 2, jitter=0.2), "MATFREE_LAPLACE", True),
    MatfreeCase("q1_kle_543", lambda: fo.box_mesh([5, 4, 3], [0.0] * 3, [1.0, 0.8, 1.1], 2, jitter=0.2), "MATFREE_KLE"),
    MatfreeCase("ngl3_affine2d_54", lambda: dyadic_box([5, 4], 3), "MATFREE_KLE", diag=1),
    MatfreeCase("ngl3_affine3d_323", lambda: sheared_box([3, 2, 3], 3), "MATFREE_KLE", diag=0),
    MatfreeCase("ngl3_box3d_323", lambda: dyadic_box([3, 2, 3], 3), "MATFREE_KLE", diag=1),
    MatfreeCase("ngl3_sheared2d_54", lambda: sheared_box([5, 4], 3), "MATFREE_KLE", diag=0),
    MatfreeCase("ngl3_general2d_54", lambda: gm.bent_lattice(2, [5, 4], 3, seed=3), "MATFREE_KLE_NGL3_GENERAL"),
    MatfreeCase("ngl3_general3d_323", lambda: gm.bent_lattice(3, [3, 2, 3], 3, seed=3), "MATFREE_KLE_NGL3_GENERAL"),
    MatfreeCase("ho_shell2d_32_ngl4", lambda: dyadic_box([3, 2], 4), "MATFREE_KLE"),
    MatfreeCase("ho_shell3d_212_ngl5", lambda: dyadic_box([2, 1, 2], 5), "MATFREE_KLE"),
    MatfreeCase("ho_general2d_32_ngl4", lambda: gm.bent_lattice(2, [3, 2], 4, seed=3), "MATFREE_KLE_GENERAL"),
    MatfreeCase("ho_general3d_222_ngl4", lambda: gm.bent_lattice(3, [2, 2, 2], 4, seed=3), "MATFREE_KLE_GENERAL"),
]

# name -> (builder, expected probe path: 0 rectilinear binary search, 1 bin grid + Newton)
PROBE_CASES = {
    "box2d_ngl3": (lambda: fo.box_mesh([4, 3], [0.0, 0.0], gm.UPPER[:2], 3), 0),
    "box3d_ngl4": (lambda: fo.box_mesh([2, 3, 2], [0.0] * 3, gm.UPPER, 4), 0),
    "bent2d_ngl5": (lambda: gm.bent_lattice(2, [4, 3], 5, seed=3), 1),
    "bent3d_ngl3": (lambda: gm.bent_lattice(3, [2, 3, 2], 3, seed=3), 1),
    "imported2d_ngl4": (lambda: gm.imported(2, [4, 3], 4), 1),
    "imported3d_ngl3": (lambda: gm.imported(3, [2, 3, 2], 3), 1),
}

INTEGRAL_CASES = {f"{kind}{dim}d_ngl{ngl}": (lambda kind=kind, dim=dim, ngl=ngl, ne=ne:
                                             dyadic_box(ne, ngl) if kind == "box" else gm.bent_lattice(dim, ne, ngl, seed=3))
                  for kind in ("box", "bent") for dim, ne in ((2, [4, 3]), (3, [2, 3, 2])) for ngl in (2, 3, 5)}

_BUILT = {}


def built(table_name, name, builder):
    """the base mesh of a case: built once, shared, never modified (the transformations copy)"""
    key = (table_name, name)
    if key not in _BUILT:
        _BUILT[key] = builder()
    return _BUILT[key]


# ---- probe points ----------------------------------------------------------------------------------------------------------------------
FACE_MARGIN = 4e-3                   # in xi: at least 1e-3 h from every cell face on these meshes (cells bent by at most 0.2 h)


def interior_points(mesh, n=200, n_outside=20, seed=1):
    """n images of random cells at random xi in (-1 + FACE_MARGIN, 1 - FACE_MARGIN)^dim: far enough from every face that no rounding
    of a translation moves a point into another cell; and n_outside points outside the bounding box.  dict(pts, inside, cell, xi)"""
    from tests import probe_model as pm
    dim = mesh.dim
    rng = np.random.default_rng(seed)
    Xc = pm.corners(mesh)
    e = rng.integers(Xc.shape[0], size=n)
    xi = rng.uniform(-1.0 + FACE_MARGIN, 1.0 - FACE_MARGIN, (n, dim))
    inside_pts = pm.image(Xc[e], xi)
    lo, hi = mesh.xyz.min(axis=0), mesh.xyz.max(axis=0)
    out = rng.uniform(lo, hi, (n_outside, dim))
    for k in range(n_outside):
        d = k % dim
        step = (0.05 + rng.random()) * (hi[d] - lo[d])
        out[k, d] = lo[d] - step if (k // dim) % 2 else hi[d] + step
    pts = np.ascontiguousarray(np.concatenate([inside_pts, out]))
    inside = np.zeros(len(pts), bool)
    inside[:n] = True
    return dict(pts=pts, inside=inside, cell=e, xi=xi)


# ---- the float64 Newton iteration on ABSOLUTE coordinates (what the bin-grid path of the probes did before it took differences) ----------
def newton_absolute(Xc, p, tol=1e-13, cap=16):
    """Newton from xi = 0 on x(xi) = p with the residual p - sum_c N_c X_c formed from the absolute corner coordinates, stopped at
    |d xi|_inf < tol within cap steps.  Returns converged [M].  The residual's rounding noise is about 2 eps |x| / h in xi"""
    from tests import probe_model as pm
    M, _, dim = Xc.shape
    xi = np.zeros((M, dim))
    conv, active = np.zeros(M, bool), np.ones(M, bool)
    for _ in range(cap):
        N, dN = pm.corner_basis(dim, xi)
        r = p - np.einsum("mc,mcd->md", N, Xc)
        J = np.einsum("mcq,mcd->mdq", dN, Xc)
        dx = np.linalg.solve(J, r[:, :, None])[:, :, 0]
        xi[active] += dx[active]
        done = active & (np.abs(dx).max(axis=1) < tol)
        conv |= done
        active &= ~done
        if not active.any():
            break
    return conv
