"""Meshes for the general matrix-free KLE operator (PYN_MATFREE_KLE_GENERAL, pynama_amd/csrc/pyn_matfree_ho_general.hip): bent
lattices, imported-style meshes (random numbering, cell order and cell orientation) and stars around a vertex of valence 3 / 5, at any
order.  Every builder returns an fo.BoxMesh container (conn in the reference's local order, xyz, boundary), so tests.test_gpu_ho3.make_ctx
and fo.elem_kle_matrices(tables, mesh.corners()) work on it.  Also the per-cell oracle K and a numpy model of the kernel's cell product
with a pointwise Jacobian, built from the library's 1-D tables and local-lattice table alone."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import fem_oracle as fo

UPPER = [1.0, 0.8, 1.2]


@functools.lru_cache(maxsize=None)
def tables(ngl, dim):
    return fo.Tables(ngl, dim)


def _corner_image(ngl, dim, corners):
    """multilinear image of the GLL points of cells with corners [E, 2^dim, dim] (reference order) -> [E, nn, dim]"""
    return np.einsum("gc,ecd->egd", tables(ngl, dim).coo_op.H, corners)


def bent_lattice(dim, nelem, ngl, bend=0.2, seed=0):
    """the lexicographic box lattice of fo.box_mesh with its interior corner nodes moved by at most bend * h along every axis and
    every high-order node recomputed as the multilinear image of its cell's corners"""
    mesh = fo.box_mesh(nelem, [0.0] * dim, UPPER[:dim], ngl)
    nc = 2 ** dim
    h = min(u / n for u, n in zip(UPPER[:dim], nelem))
    inner = np.setdiff1d(np.unique(mesh.conn[:, :nc]), mesh.boundary)
    cxyz = mesh.xyz.copy()
    cxyz[inner] += bend * h * np.random.default_rng(seed).uniform(-1.0, 1.0, (len(inner), dim))
    xyz = cxyz.copy()
    xyz[mesh.conn.ravel()] = _corner_image(ngl, dim, cxyz[mesh.conn[:, :nc]]).reshape(-1, dim)
    corner_ids = np.unique(mesh.conn[:, :nc])
    xyz[corner_ids] = cxyz[corner_ids]
    mesh.xyz = xyz
    return mesh


def warped_lattice(dim, nelem, ngl, warp=0.15, seed=0):
    """the box lattice of fo.box_mesh with EVERY corner node, those on the boundary included, moved by at most warp * h along every
    axis and every high-order node recomputed as the multilinear image of its cell's corners: a single cell is already bilinear /
    trilinear (bent_lattice moves interior corners only, and a [2, 1, 2] box has none).  `boundary` and `borders` stay the node
    sets of the box: valid Dirichlet and wall sets of a domain whose shape alone has changed."""
    mesh = fo.box_mesh(nelem, [0.0] * dim, UPPER[:dim], ngl)
    nc = 2 ** dim
    h = min(u / n for u, n in zip(UPPER[:dim], nelem))
    corner_ids = np.unique(mesh.conn[:, :nc])
    cxyz = mesh.xyz.copy()
    cxyz[corner_ids] += warp * h * np.random.default_rng(seed).uniform(-1.0, 1.0, (len(corner_ids), dim))
    xyz = cxyz.copy()
    xyz[mesh.conn.ravel()] = _corner_image(ngl, dim, cxyz[mesh.conn[:, :nc]]).reshape(-1, dim)
    xyz[corner_ids] = cxyz[corner_ids]
    mesh.xyz = xyz
    return mesh


def _rotations(dim):
    from tests.test_highorder_import_host import _rotations as rot
    return rot(dim)


def _lifted(dim, conn, xyz, ngl, nelem=()):
    from pynama_amd.domain.dmplex import _lift_high_order
    ch, xh, ho = _lift_high_order(np.asarray(conn, np.int64), xyz, ngl, dim)
    return fo.BoxMesh(dim, ngl, tuple(nelem), (), np.ascontiguousarray(ch, dtype=np.int32), np.ascontiguousarray(xh),
                      np.unique(ho["ext_nodes"]), {})


def imported(dim, nelem, ngl, jitter=0.2, seed=5):
    """what the Gmsh import path produces: fo.box_mesh(..., 2, jitter) in a random node numbering and a random cell order, every cell
    relabelled by a random orientation-preserving symmetry, lifted to order ngl with _lift_high_order"""
    m1 = fo.box_mesh(nelem, [0.0] * dim, UPPER[:dim], 2, jitter=jitter)
    rng = np.random.default_rng(seed)
    rots = _rotations(dim)
    conn = np.stack([c[rots[rng.integers(len(rots))]] for c in m1.conn.astype(np.int64)])
    perm = rng.permutation(m1.n_node)                              # new id of old vertex
    conn, xyz = perm[conn][rng.permutation(conn.shape[0])], m1.xyz[np.argsort(perm)]
    return _lifted(dim, conn, xyz, ngl, nelem)


def star(k, ngl, layers=0):
    """k quadrilaterals around one vertex (valence k at the centre, 2 on the k spokes, 1 elsewhere); layers > 0: extruded to that many
    layers of hexahedra.  Every cell's corner order starts at another corner (a rotation of the counter-clockwise order)."""
    from pynama_amd.elements.spectral import _local_lattice
    ang = 2.0 * np.pi * np.arange(k) / k
    pts = [np.zeros(2)] + [np.array([np.cos(a), np.sin(a)]) for a in ang]
    pts += [1.35 * np.array([np.cos(a + np.pi / k), np.sin(a + np.pi / k)]) for a in ang]
    xy = np.array(pts)                                             # 0: centre, 1..k: spokes, k+1..2k: outer corners
    ccw = [[0, 1 + i, 1 + k + i, 1 + (i + 1) % k] for i in range(k)]
    quads = np.array([np.roll(q, i) for i, q in enumerate(ccw)])   # the reference's corner order is counter-clockwise
    if not layers:
        return _lifted(2, quads, xy, ngl)
    n2 = xy.shape[0]
    xyz = np.concatenate([np.column_stack([xy, np.full(n2, 0.6 * l)]) for l in range(layers + 1)])
    at2 = {tuple(c): q for q, c in enumerate(_local_lattice(2, 2))}
    clat3 = _local_lattice(2, 3)
    hexes = [[q[at2[(c[0], c[1])]] + n2 * (l + c[2]) for c in clat3] for l in range(layers) for q in quads]
    return _lifted(3, np.array(hexes), xyz, ngl)


def valences(mesh):
    """cells per node"""
    return np.bincount(mesh.conn.ravel(), minlength=mesh.n_node)


_KE = {}


def elem_K(mesh, alpha_d, alpha_w):
    """K_e of EVERY cell (the cells are not congruent)"""
    key = (mesh.dim, mesh.ngl, alpha_d, alpha_w, mesh.conn.tobytes(), mesh.xyz.tobytes())
    if key not in _KE:
        _KE.clear()                                                # one mesh at a time: the matrices are large
        tb, X = tables(mesh.ngl, mesh.dim), mesh.corners()
        # (cell by cell: the oracle's batched einsum falls out of cache at 3-D ngl >= 5; numpy releases the GIL inside it)
        with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
            _KE[key] = np.stack(list(ex.map(lambda e: fo.elem_kle_matrices(tb, X[e:e + 1], alpha_d, alpha_w)[0][0], range(mesh.n_elem))))
    return _KE[key]


def oracle_K(mesh, mask, alpha_d, alpha_w):
    """K of assemble_kle_freeslip with a per-DOF mask [n_node, dim] (None: nothing imposed): imposed columns eliminated, imposed rows
    identity (tests/test_gpu_ho_matfree.py: oracle_K, with one K_e per cell)"""
    import scipy.sparse as sp
    dim = mesh.dim
    Ke = elem_K(mesh, alpha_d, alpha_w)
    n = mesh.n_node
    vdof = fo.dof_indices(mesh.conn, dim)
    is_bc = np.zeros(n * dim, bool) if mask is None else np.asarray(mask, bool).reshape(-1)
    rfree = ~is_bc[vdof]
    R = np.broadcast_to(vdof[:, :, None], Ke.shape)
    C = np.broadcast_to(vdof[:, None, :], Ke.shape)
    mff = rfree[:, :, None] & rfree[:, None, :]
    K = fo._scatter((n * dim, n * dim), R[mff], C[mff], Ke[mff])
    bc_idx = np.nonzero(is_bc)[0]
    return (K + sp.coo_matrix((np.ones(len(bc_idx)), (bc_idx, bc_idx)), shape=K.shape)).tocsr()


def boundary_mask(mesh):
    m = np.zeros((mesh.n_node, mesh.dim), np.uint8)
    m[mesh.boundary] = 1
    return m


def masks(mesh):
    dim, n = mesh.dim, mesh.n_node
    per_dof = np.zeros((n, dim), np.uint8)
    per_dof[mesh.boundary, 0] = 1
    rnd = (np.random.default_rng(7).random((n, dim)) < 0.3).astype(np.uint8)
    return {"none": None, "boundary": boundary_mask(mesh), "per_dof": per_dof, "random": rnd}


def cell_product_pointwise(t, loc, cell_conn, xyz, x, alpha_d, alpha_w):
    """y_e = K_e x_e as hog_cell_kernel forms it, from the library's 1-D tables `t` and local-lattice table `loc` alone: the cell's
    nodes through its connectivity row, J(xi) from its 2^dim corners in LATTICE orientation at every Lobatto node and Gauss point.
    x, result: [n_node, dim] global vectors (the result holds this cell's contributions)"""
    ngl, dim = len(t["xl"]), loc.shape[1]
    m, nc = ngl - 1, 2 ** dim
    t_of_a = loc @ np.array([ngl ** d for d in range(dim)])
    a_of_t = np.argsort(t_of_a)
    nodes_t = np.asarray(cell_conn)[a_of_t]                          # node of tensor position t, x fastest
    xe = x[nodes_t].reshape((ngl,) * dim + (dim,))                   # array axes slow to fast: lattice axis r = array axis dim-1-r
    Xc = np.zeros((2,) * dim + (dim,))                               # corner coordinates by lattice bits [b0][b1][b2]
    for a in range(nc):
        Xc[tuple(loc[a] // m)] = xyz[cell_conn[a]]
    Dl, wl, Br, Gr, wr = t["Dl"], t["wl"], t["Br"], t["Gr"], t["wr"]

    def along(M, r, v):                                              # contract lattice axis r of v with M[out, in]
        return np.moveaxis(np.tensordot(M, v, axes=(1, dim - 1 - r)), 0, dim - 1 - r)

    def jac(pts):
        """J[..., r, x] at the tensor grid of the 1-D points (array axes slow to fast), its inverse Ji[..., x, r] and det"""
        n = len(pts)
        xi = np.meshgrid(*([pts] * dim), indexing="ij")              # xi[ax]: coordinate along array axis ax = lattice axis dim-1-ax
        xi = [xi[dim - 1 - r] for r in range(dim)]                   # by lattice axis
        J = np.zeros((n,) * dim + (dim, dim))
        for b in np.ndindex(*(2,) * dim):
            for r in range(dim):
                dn = np.full((n,) * dim, 0.5 if b[r] else -0.5)
                for e in range(dim):
                    if e != r:
                        dn = dn * 0.5 * (1.0 + (1.0 if b[e] else -1.0) * xi[e])
                J[..., r, :] += dn[..., None] * Xc[b]
        return J, np.linalg.inv(J), np.linalg.det(J)

    def tensor_w(w1):
        w = w1
        for _ in range(dim - 1):
            w = np.multiply.outer(w, w1)
        return w

    y = np.zeros_like(xe)
    # full rule: collocated Laplacian of every component
    _, Ji, det = jac(t["xl"])
    assert det.min() > 0
    Q = det[..., None, None] * np.einsum("...dr,...ds->...rs", Ji, Ji)
    w = tensor_w(wl)
    for p in range(dim):
        g = [along(Dl, r, xe[..., p]) for r in range(dim)]
        for r in range(dim):
            y[..., p] += along(Dl.T, r, w * sum(Q[..., r, s] * g[s] for s in range(dim)))
    # reduced rule
    _, Ji, det = jac(t["xr"])
    assert det.min() > 0
    w = tensor_w(wr)

    def interp(v, r_der):
        for r in range(dim):
            v = along(Gr if r == r_der else Br, r, v)
        return v

    def interp_t(f, r_der):
        for r in range(dim):
            f = along((Gr if r == r_der else Br).T, r, f)
        return f

    D = np.zeros((dim, dim) + w.shape)                               # D[q][d] = d u_q / d x_d
    for q in range(dim):
        g = [interp(xe[..., q], r) for r in range(dim)]
        for d in range(dim):
            D[q, d] = sum(Ji[..., d, r] * g[r] for r in range(dim))
    tr = sum(D[q, q] for q in range(dim))
    for p in range(dim):
        W = [w * det * (alpha_d * tr if d == p else alpha_w * (D[p, d] - D[d, p])) for d in range(dim)]
        for r in range(dim):
            y[..., p] += interp_t(sum(Ji[..., d, r] * W[d] for d in range(dim)), r)
    out = np.zeros_like(x)
    out[nodes_t] = y.reshape(-1, dim)
    return out
