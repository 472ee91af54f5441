"""numpy model of the mesh integrals (pynama_amd/csrc/pyn_integrals.hip), built from oracle.fem_oracle alone: fo.gauss_lobatto(ngl)
and fo.gauss_legendre(ngl + 1) for the rules, fo.tensor_tables for the field's basis and for the corner basis, fo._geom for the
physical gradients G and w det J.  The dense restatement of the forms: every moment is the math.fsum of its contributions over all
cells and points, and S = sum |contribution| is the scale of every bar.  Also the closed forms the tests compare with."""
import functools
import math

import numpy as np

from oracle import fem_oracle as fo

NODAL, GAUSS = 0, 1


def tensor_tables(nodes1d, pts1d, w1d, dim):
    """fo.tensor_tables without its Python loop over (point, node) pairs, which takes 10 s at 3-D ngl 8: the same products of
    fo.lagrange_1d values in the same order, taken for all pairs at once (tests/test_integrals_model_host.py holds the two equal
    bit for bit at low order)"""
    h, dh = fo.lagrange_1d(nodes1d, pts1d)
    nod = np.array(fo.local_lattice(len(nodes1d), dim))
    gp = np.array(fo.local_lattice(len(pts1d), dim))
    vals = [h[gp[:, d]][:, nod[:, d]] for d in range(dim)]          # [g, a] per axis
    ders = [dh[gp[:, d]][:, nod[:, d]] for d in range(dim)]

    def prod(fs):
        out = fs[0]
        for f in fs[1:]:
            out = out * f
        return out

    H = prod(vals)
    Hrs = np.stack([prod([ders[e] if e == d else vals[e] for e in range(dim)]) for d in range(dim)], axis=1)
    pts = np.stack([np.asarray(pts1d)[gp[:, d]] for d in range(dim)], axis=1)
    w = prod([np.asarray(w1d)[gp[:, d]] for d in range(dim)])
    return fo.Quad(H, Hrs, pts, w)


@functools.lru_cache(maxsize=None)
def rule_tables(ngl, dim, rule):
    """(q, q_geo): the field's tables and the corner basis at the points of the rule, both in the reference's order"""
    nod, w_nod = fo.gauss_lobatto(ngl)
    pts, w = fo.gauss_legendre(ngl + 1) if rule == GAUSS else (nod, w_nod)
    cor, _ = fo.gauss_lobatto(2)
    return tensor_tables(nod, pts, w, dim), tensor_tables(cor, pts, w, dim)


def n_entries(dim, bs, grad):
    return 1 + (3 if grad else 2) * bs + ((1 + (3 if dim == 3 else 1)) if grad and bs == dim else 0)


def contributions(mesh, u, rule=GAUSS, grad=False, minus=None):
    """list of arrays [E, ngp], one per entry of pyn_integrate's layout: volume, value[bs], square[bs], grad2[bs], div2, curl2[dim_w]"""
    dim, nc = mesh.dim, 2 ** mesh.dim
    u = np.asarray(u, dtype=np.float64).reshape(mesh.n_node, -1)
    if minus is not None:
        u = u - np.asarray(minus, dtype=np.float64).reshape(mesh.n_node, -1)      # per node, one rounding, before anything else
    bs = u.shape[1]
    q, qg = rule_tables(mesh.ngl, dim, rule)
    X = mesh.xyz[mesh.conn[:, :nc]]
    G, c = fo._geom(qg, q, X)                                       # G [E, g, d, a], c [E, g]
    ue = u[mesh.conn]                                               # [E, nn, bs]
    val = np.einsum("ga,eab->egb", q.H, ue)
    out = [c] + [c * val[:, :, b] for b in range(bs)] + [c * val[:, :, b] ** 2 for b in range(bs)]
    if grad:
        D = np.einsum("egda,eab->egbd", G, ue)                      # D[..., b, d] = d u_b / d x_d
        out += [c * np.sum(D[:, :, b, :] ** 2, axis=2) for b in range(bs)]
        if bs == dim:
            out.append(c * sum(D[:, :, b, b] for b in range(dim)) ** 2)
            curl = [0.0] * (3 if dim == 3 else 1)
            for r, comp, der, sign in fo._curl_rows(dim)[1]:
                curl[r] = curl[r] + sign * D[:, :, comp, der]
            out += [c * w ** 2 for w in curl]
    assert len(out) == n_entries(dim, bs, grad)
    return out


def moments(mesh, u, rule=GAUSS, grad=False, minus=None):
    """(values, S): every entry summed exactly (math.fsum), and the sum of the absolute contributions"""
    terms = contributions(mesh, u, rule, grad, minus)
    return (np.array([math.fsum(t.ravel()) for t in terms]), np.array([math.fsum(np.abs(t).ravel()) for t in terms]))


def component_scale(mesh, u, minus=None):
    """(S of div2, S of curl2 [dim_w]) taken from the signed gradient components: sum of w det J (sum |d u_b / d x_d|)^2 over the
    components that enter the divergence or the curl row.  The divergence of a solenoidal field is a sum of dim gradient components
    that cancel, each rounded relative to itself and not to their sum, so |contribution| of div2 under-states the rounding by
    (|d u / d x| / |div u|)^2; for random fields the two scales agree within a small factor.  Gauss rule, bs == dim."""
    dim, nc = mesh.dim, 2 ** mesh.dim
    u = np.asarray(u, dtype=np.float64).reshape(mesh.n_node, dim)
    if minus is not None:
        u = u - np.asarray(minus, dtype=np.float64).reshape(mesh.n_node, dim)
    q, qg = rule_tables(mesh.ngl, dim, GAUSS)
    G, c = fo._geom(qg, q, mesh.xyz[mesh.conn[:, :nc]])
    D = np.abs(np.einsum("egda,eab->egbd", G, u[mesh.conn]))
    div = c * sum(D[:, :, b, b] for b in range(dim)) ** 2
    curl = [0.0] * (3 if dim == 3 else 1)
    for r, comp, der, _ in fo._curl_rows(dim)[1]:
        curl[r] = curl[r] + D[:, :, comp, der]
    return math.fsum(div.ravel()), np.array([math.fsum((c * w ** 2).ravel()) for w in curl])


def named(flat, dim, bs, grad):
    """dict of the entries of a flat result"""
    d = {"volume": flat[0], "value": flat[1:1 + bs], "square": flat[1 + bs:1 + 2 * bs]}
    if grad:
        d["grad2"] = flat[1 + 2 * bs:1 + 3 * bs]
        if bs == dim:
            d["div2"], d["curl2"] = flat[1 + 3 * bs], flat[2 + 3 * bs:]
    return d


def shoelace_area(mesh):
    """area of a 2-D mesh: the shoelace formula over the corners of every cell (counter-clockwise in the reference's order)"""
    X = mesh.xyz[mesh.conn[:, :4]]
    x, y = X[:, :, 0], X[:, :, 1]
    return math.fsum((0.5 * np.sum(x * np.roll(y, -1, axis=1) - np.roll(x, -1, axis=1) * y, axis=1)).ravel())


# ---- the tensor polynomial p(x) = prod_d (1 + x_d / 2)^(ngl - 1) on the box [0, upper], sheared by x' = x + s y ----------------------
def sheared(mesh, s):
    """the mesh with every node moved by x' = x + s y: an affine map of determinant 1"""
    xyz = mesh.xyz.copy()
    xyz[:, 0] += s * xyz[:, 1]
    return fo.BoxMesh(mesh.dim, mesh.ngl, mesh.nelem, mesh.lattice, mesh.conn, xyz, mesh.boundary, mesh.borders)


def poly_nodal(mesh):
    """p at the nodes of the UNSHEARED box mesh: on the sheared mesh the same nodal values are u(x') = p(x(x'))"""
    return np.prod((1.0 + 0.5 * mesh.xyz) ** (mesh.ngl - 1), axis=1)


def poly_closed_form(ngl, upper, s=0.0):
    """(int u^2, int |grad u|^2) of u(x') = p(x' - s y' e_x) over the sheared box: d u / d x' = p_x, d u / d y' = p_y - s p_x"""
    m = ngl - 1
    I0 = [((1.0 + 0.5 * U) ** (2 * m + 1) - 1.0) / (0.5 * (2 * m + 1)) for U in upper]                      # int f^2
    I1 = [(0.5 * m) ** 2 * ((1.0 + 0.5 * U) ** (2 * m - 1) - 1.0) / (0.5 * (2 * m - 1)) for U in upper]     # int f'^2
    Cx = [0.5 * ((1.0 + 0.5 * U) ** (2 * m) - 1.0) for U in upper]                                          # int f f'
    dim = len(upper)
    P = [I1[d] * math.prod(I0[e] for e in range(dim) if e != d) for d in range(dim)]
    Pxy = Cx[0] * Cx[1] * math.prod(I0[e] for e in range(2, dim))
    return math.prod(I0), (1.0 + s * s) * P[0] + sum(P[1:]) - 2.0 * s * Pxy
