"""numpy model of the point probes (pynama_amd/csrc/pyn_probe.hip), built from fo.local_lattice, fo.gauss_lobatto and
fo.lagrange_1d alone: the multilinear corner basis and its Jacobian, the location of points (bounding-box candidates, Newton from
xi = 0, lowest accepting cell), the nodal basis phi(ngl, dim, xi) and the sampled value.  Also the point sets the probe tests use."""
import functools

import numpy as np

from oracle import fem_oracle as fo

NEWTON_CAP, NEWTON_TOL, ACCEPT, PAD = 16, 1e-13, 1e-10, 1e-9
EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def corner_signs(dim):
    """[2^dim, dim]: +-1 per axis of corner c, which sits at reference position fo.local_lattice(2, dim)[c]"""
    return 2.0 * np.array(fo.local_lattice(2, dim), dtype=np.float64) - 1.0


def corner_basis(dim, xi):
    """N [M, 2^dim] and dN [M, 2^dim, dim] (d N_c / d xi_q) at xi [M, dim]"""
    s = corner_signs(dim)
    f = 0.5 * (1.0 + s[None, :, :] * xi[:, None, :])                # [M, nc, dim]
    N = np.prod(f, axis=2)
    dN = np.empty(f.shape)
    for q in range(dim):
        others = [d for d in range(dim) if d != q]
        dN[:, :, q] = 0.5 * s[None, :, q] * np.prod(f[:, :, others], axis=2)
    return N, dN


def corners(mesh):
    """[E, 2^dim, dim]: the first 2^dim entries of every connectivity row"""
    return mesh.xyz[mesh.conn[:, :2 ** mesh.dim]]


def image(Xc, xi):
    """x(xi) of the cells with corners Xc [M, 2^dim, dim]"""
    N, _ = corner_basis(Xc.shape[2], xi)
    return np.einsum("mc,mcd->md", N, Xc)


def newton(Xc, p):
    """Newton from xi = 0 on x(xi) = p for the pairs (cell corners Xc [M, nc, dim], point p [M, dim]).  Returns the raw xi, the steps
    taken, converged (|d xi|_inf < NEWTON_TOL within NEWTON_CAP steps) and ok (det J > 0 at every iterate).  As on the device, the
    iteration runs on coordinates relative to the cell's first corner: the residual then rounds at eps h and not at eps |x|"""
    M, _, dim = Xc.shape
    p = p - Xc[:, 0, :]
    Xc = Xc - Xc[:, :1, :]
    xi = np.zeros((M, dim))
    steps = np.zeros(M, dtype=int)
    active, ok, conv = np.ones(M, bool), np.ones(M, bool), np.zeros(M, bool)
    for _ in range(NEWTON_CAP):
        if not active.any():
            break
        N, dN = corner_basis(dim, xi)
        r = p - np.einsum("mc,mcd->md", N, Xc)
        J = np.einsum("mcq,mcd->mdq", dN, Xc)                       # J[d][q] = d x_d / d xi_q
        det = np.linalg.det(J)
        bad = active & ~(det > 0.0)
        ok[bad] = False
        active[bad] = False
        J[~active] = np.eye(dim)
        dx = np.linalg.solve(J, r[:, :, None])[:, :, 0]
        xi[active] += dx[active]
        steps[active] += 1
        done = active & (np.abs(dx).max(axis=1) < NEWTON_TOL)
        conv[done] = True
        active[done] = False
    return xi, steps, conv, ok


def locate(mesh, pts):
    """dict over the points [P, dim]: cell (lowest accepting cell, -1: none), xi (clipped to [-1, 1]; NaN where not found), steps
    (Newton steps of the accepted cell), ncand (cells whose padded corner box holds the point), near (some candidate's margin
    |xi|_inf - 1 lies within 1e-12 of the acceptance threshold: a rounding error could decide it either way)"""
    dim = mesh.dim
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, dim)
    Xc = corners(mesh)
    lo, hi = Xc.min(axis=1), Xc.max(axis=1)
    pad = PAD * (hi - lo)
    inb = np.all((pts[:, None, :] >= (lo - pad)[None]) & (pts[:, None, :] <= (hi + pad)[None]), axis=2)     # [P, E]
    pi, ei = np.nonzero(inb)                                        # sorted by point, then by cell
    raw, steps, conv, ok = newton(Xc[ei], pts[pi])
    amax = np.abs(raw).max(axis=1) if len(pi) else np.zeros(0)
    acc = ok & conv & (amax <= 1.0 + ACCEPT)
    P = pts.shape[0]
    out = dict(cell=np.full(P, -1, dtype=np.int64), xi=np.full((P, dim), np.nan), steps=np.zeros(P, dtype=int),
               ncand=np.bincount(pi, minlength=P), near=np.zeros(P, bool))
    near_pair = ok & conv & (np.abs(amax - 1.0 - ACCEPT) <= 1e-12)
    out["near"][pi[near_pair]] = True
    for m in np.nonzero(acc)[0][::-1]:                              # descending: the lowest cell of a point is written last
        out["cell"][pi[m]] = ei[m]
        out["xi"][pi[m]] = np.clip(raw[m], -1.0, 1.0)
        out["steps"][pi[m]] = steps[m]
    return out


def residual(mesh, pts, cell, xi):
    """|x(xi) - p|_inf per found point (NaN where cell < 0)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, mesh.dim)
    res = np.full(pts.shape[0], np.nan)
    f = cell >= 0
    res[f] = np.abs(image(corners(mesh)[cell[f]], xi[f]) - pts[f]).max(axis=1)
    return res


@functools.lru_cache(maxsize=None)
def _lattice(ngl, dim):
    return np.array(fo.local_lattice(ngl, dim), dtype=np.int64)


def phi(ngl, dim, xi):
    """phi_a(xi) [M, ngl^dim] in the reference's local order: the product over the axes of the Lagrange functions of the ascending
    Lobatto(ngl) nodes, local node a at lattice position fo.local_lattice(ngl, dim)[a]"""
    xi = np.asarray(xi, dtype=np.float64).reshape(-1, dim)
    nodes, _ = fo.gauss_lobatto(ngl)
    t = _lattice(ngl, dim)
    out = np.ones((xi.shape[0], t.shape[0]))
    for d in range(dim):
        h, _ = fo.lagrange_1d(nodes, xi[:, d])                      # [M, ngl]
        out *= h[:, t[:, d]]
    return out


def sample(mesh, cell, xi, u, order=None, with_bound=False, ph=None):
    """sum_a phi_a(xi) u[conn[cell][a]] per point and component ([P, bs]; NaN rows where cell < 0), summed over a in the local order,
    or in the permutation `order`; with_bound: also sum_a |phi_a| |u_a|; ph: phi(ngl, dim, xi[cell >= 0]) when the caller has it"""
    u = np.asarray(u, dtype=np.float64).reshape(mesh.n_node, -1)
    P, bs = len(cell), u.shape[1]
    out, bound = np.full((P, bs), np.nan), np.full((P, bs), np.nan)
    f = np.nonzero(cell >= 0)[0]
    ph = phi(mesh.ngl, mesh.dim, xi[f]) if ph is None else ph       # [F, nn]
    ua = u[mesh.conn[cell[f]]]                                      # [F, nn, bs]
    terms = ph[:, :, None] * ua
    if order is not None:
        terms = terms[:, order, :]
    acc = np.zeros((len(f), bs))
    for a in range(terms.shape[1]):                                 # one term at a time: the order is the point
        acc += terms[:, a, :]
    out[f] = acc
    bound[f] = np.abs(terms).sum(axis=1)
    return (out, bound) if with_bound else out


# ---- the point sets of the tests ------------------------------------------------------------------------------------------------
def probe_points(mesh, seed=0, box_boundary=False, extra_outside=None, max_nodes=None):
    """about 300 points and what is known of them by construction: `pts` [P, dim], `inside` (images of cells: must be found),
    `outside` (must not be found).  Images of random cells at random xi in (-1, 1)^dim; the same with one, two or all components set
    to +-1 (faces, edges, vertices); every mesh node (max_nodes: every corner node and that many of the others, for the checks whose
    reference costs a Python loop per point); on request points exactly on the boundary of the box [0, upper]; 20 points
    outside the bounding box; and `extra_outside` (points inside the bounding box that lie in no cell)"""
    dim = mesh.dim
    rng = np.random.default_rng(seed)
    Xc = corners(mesh)
    E = Xc.shape[0]

    def images(n, pinned):
        e = rng.integers(E, size=n)
        xi = rng.uniform(-1.0, 1.0, (n, dim))
        for k in range(n):
            axes = rng.permutation(dim)[:pinned if pinned < dim else dim]
            xi[k, axes] = rng.choice([-1.0, 1.0], size=len(axes))
        return image(Xc[e], xi)

    parts = [images(100, 0), images(40, 1), images(30, 2)] + ([images(30, 3)] if dim == 3 else [])
    nodes = mesh.xyz
    if max_nodes is not None and nodes.shape[0] > max_nodes:
        keep = np.unique(np.concatenate([np.unique(mesh.conn[:, :2 ** dim]), rng.choice(nodes.shape[0], max_nodes, replace=False)]))
        nodes = nodes[keep]
    parts.append(nodes)
    lo, hi = mesh.xyz.min(axis=0), mesh.xyz.max(axis=0)
    if box_boundary:
        b = rng.uniform(lo, hi, (24, dim))
        for k in range(24):
            b[k, k % dim] = (lo, hi)[(k // dim) % 2][k % dim]
        parts.append(b)
    n_in = sum(len(p) for p in parts)
    out = rng.uniform(lo, hi, (20, dim))
    for k in range(20):
        d = k % dim
        out[k, d] = (lo[d] - (0.05 + rng.random()) * (hi[d] - lo[d])) if (k // dim) % 2 else (hi[d] + (0.05 + rng.random()) * (hi[d] - lo[d]))
    parts.append(out)
    if extra_outside is not None:
        parts.append(np.asarray(extra_outside, dtype=np.float64).reshape(-1, dim))
    pts = np.ascontiguousarray(np.concatenate(parts))
    inside = np.zeros(len(pts), bool)
    inside[:n_in] = True
    return dict(pts=pts, inside=inside, outside=~inside)


def bbox_corners(mesh):
    """the corners of the bounding box"""
    lo, hi = mesh.xyz.min(axis=0), mesh.xyz.max(axis=0)
    return np.array([[(lo, hi)[(k >> d) & 1][d] for d in range(mesh.dim)] for k in range(2 ** mesh.dim)])


def linear_field(mesh, pts=None):
    """f(x) = 0.3 + sum_d (d + 1.5) x_d at the mesh nodes (or at pts)"""
    x = mesh.xyz if pts is None else np.asarray(pts).reshape(-1, mesh.dim)
    return 0.3 + x @ (np.arange(mesh.dim) + 1.5)


def tensor_poly(mesh, pts=None):
    """a polynomial of degree ngl - 1 per axis: prod_d (1 + 0.5 x_d)^(ngl - 1)"""
    x = mesh.xyz if pts is None else np.asarray(pts).reshape(-1, mesh.dim)
    return np.prod((1.0 + 0.5 * x) ** (mesh.ngl - 1), axis=1)
