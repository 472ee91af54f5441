"""A numpy model of the cell product of PYN_MATFREE_KLE_NGL3_GENERAL (pynama_amd/csrc/pyn_matfree_ho3_general.hip) as h3g_cell_kernel
forms it, built from the library's 1-D tables and local-lattice table alone: the cell's nodes through its connectivity row, J(xi) from
its 2^dim corners in LATTICE orientation at every point of the Gauss(3)^dim full rule and of the Gauss(2)^dim reduced rule.  Also the
host models of what pyn_matfree_set builds and checks for this operator: the node -> (cell, t) incidence list and the comparison of the
element tables with the tensor products of the 1-D tables."""
import numpy as np


def lagrange3(nodes, pts):
    """values and first derivatives [len(pts), 3] of the three quadratic Lagrange functions on `nodes` at `pts`"""
    nodes, pts = np.asarray(nodes, float), np.asarray(pts, float)
    h, dh = np.zeros((len(pts), 3)), np.zeros((len(pts), 3))
    for a in range(3):
        b, c = [k for k in range(3) if k != a]
        den = (nodes[a] - nodes[b]) * (nodes[a] - nodes[c])
        h[:, a] = (pts - nodes[b]) * (pts - nodes[c]) / den
        dh[:, a] = ((pts - nodes[b]) + (pts - nodes[c])) / den
    return h, dh


def tables_1d(lib):
    """the 1-D tables of the operator from the library's own rules: Lobatto(3) nodes xl, the Gauss(3) full rule xf / wf with
    Bf[q, a] = h_a(xf_q), Gf[q, a] = h_a'(xf_q), the Gauss(2) reduced rule xr / wr with Br, Gr"""
    t3, t4 = lib.ho_tables_1d(3), lib.ho_tables_1d(4)                # Gauss(3) = the reduced rule of order 4
    Bf, Gf = lagrange3(t3["xl"], t4["xr"])
    Br, Gr = lagrange3(t3["xl"], t3["xr"])
    assert np.abs(Br - t3["Br"]).max() < 1e-15 and np.abs(Gr - t3["Gr"]).max() < 1e-15
    return dict(xl=t3["xl"], xf=t4["xr"], wf=t4["wr"], Bf=Bf, Gf=Gf, xr=t3["xr"], wr=t3["wr"], Br=t3["Br"], Gr=t3["Gr"])


def a_of_t(loc, ngl=3):
    """the local node at tensor position t (x fastest): the inverse of the local-lattice table"""
    return np.argsort(np.asarray(loc) @ np.array([ngl ** d for d in range(loc.shape[1])]))


def cell_geometry(t, loc, cell_conn, xyz):
    """(Ji [..., x, r], det) at the tensor grids of both rules, array axes slow to fast, from the cell's corners by lattice bits"""
    dim = loc.shape[1]
    Xc = np.zeros((2,) * dim + (dim,))
    for a in range(2 ** dim):
        Xc[tuple(loc[a] // 2)] = xyz[cell_conn[a]]

    def jac(pts):
        n = len(pts)
        xi = np.meshgrid(*([pts] * dim), indexing="ij")              # xi[ax]: along array axis ax = lattice axis dim-1-ax
        xi = [xi[dim - 1 - r] for r in range(dim)]
        J = np.zeros((n,) * dim + (dim, dim))
        for b in np.ndindex(*(2,) * dim):
            for r in range(dim):
                dn = np.full((n,) * dim, 0.5 if b[r] else -0.5)
                for e in range(dim):
                    if e != r:
                        dn = dn * 0.5 * (1.0 + (1.0 if b[e] else -1.0) * xi[e])
                J[..., r, :] += dn[..., None] * Xc[b]
        return np.linalg.inv(J), np.linalg.det(J)

    return jac(t["xf"]), jac(t["xr"])


def cell_product(t, loc, cell_conn, xyz, x, alpha_d, alpha_w):
    """y_e = K_e x_e in two rules; x, result: [n_node, dim] global vectors (the result holds this cell's contributions)"""
    dim = loc.shape[1]
    nodes_t = np.asarray(cell_conn)[a_of_t(loc)]
    xe = x[nodes_t].reshape((3,) * dim + (dim,))                     # array axes slow to fast: lattice axis r = array axis dim-1-r
    (Jif, detf), (Jir, detr) = cell_geometry(t, loc, cell_conn, xyz)
    assert detf.min() > 0 and detr.min() > 0

    def along(M, r, v):                                              # contract lattice axis r of v with M[out, in]
        return np.moveaxis(np.tensordot(M, v, axes=(1, dim - 1 - r)), 0, dim - 1 - r)

    def tensor_w(w1):
        w = w1
        for _ in range(dim - 1):
            w = np.multiply.outer(w, w1)
        return w

    def interp(B, G, v, r_der):
        for r in range(dim):
            v = along(G if r == r_der else B, r, v)
        return v

    def interp_t(B, G, f, r_der):
        for r in range(dim):
            f = along((G if r == r_der else B).T, r, f)
        return f

    y = np.zeros_like(xe)
    # full rule, Gauss(3)^dim: the Laplacian of every component
    Bf, Gf = t["Bf"], t["Gf"]
    Q = (tensor_w(t["wf"]) * detf)[..., None, None] * np.einsum("...dr,...ds->...rs", Jif, Jif)
    for p in range(dim):
        g = [interp(Bf, Gf, xe[..., p], r) for r in range(dim)]
        for r in range(dim):
            y[..., p] += interp_t(Bf, Gf, sum(Q[..., r, s] * g[s] for s in range(dim)), r)
    # reduced rule, Gauss(2)^dim: alpha_d (div u)(div v) + alpha_w curl u . curl v in the per-point form
    Br, Gr = t["Br"], t["Gr"]
    w = tensor_w(t["wr"]) * detr
    D = np.zeros((dim, dim) + w.shape)                               # D[q][d] = d u_q / d x_d
    for q in range(dim):
        g = [interp(Br, Gr, xe[..., q], r) for r in range(dim)]
        for d in range(dim):
            D[q, d] = sum(Jir[..., d, r] * g[r] for r in range(dim))
    tr = sum(D[q, q] for q in range(dim))
    for p in range(dim):
        W = [w * (alpha_d * tr if d == p else alpha_w * (D[p, d] - D[d, p])) for d in range(dim)]
        for r in range(dim):
            y[..., p] += interp_t(Br, Gr, sum(Jir[..., d, r] * W[d] for d in range(dim)), r)
    out = np.zeros_like(x)
    out[nodes_t] = y.reshape(-1, dim)
    return out


def incidence(conn, n_node, aoft):
    """the node -> (cell, t) incidence list in CSR form, entries cell * nn + t ascending within a row: (ptr, inc)"""
    conn = np.asarray(conn)
    nn = conn.shape[1]
    node_of = conn[:, aoft].reshape(-1)                              # node of entry cell * nn + t
    order = np.argsort(node_of, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(node_of, minlength=n_node))])
    assert nn == len(aoft)
    return ptr.astype(np.int32), order.astype(np.int32)


def tensor_rule_error(q, loc_pts, loc_nodes, w1, B1):
    """largest difference between a rule's tables (weights q.w [ngp], values q.H [ngp, nn], reference order of points and nodes) and
    the tensor products of the 1-D weights w1 and values B1[q, a]: what the set-time check of the operator measures"""
    dim = loc_nodes.shape[1]
    worst = 0.0
    for g, gi in enumerate(loc_pts):
        worst = max(worst, abs(q.w[g] - np.prod([w1[gi[d]] for d in range(dim)])))
        for a, ai in enumerate(loc_nodes):
            worst = max(worst, abs(q.H[g, a] - np.prod([B1[gi[d], ai[d]] for d in range(dim)])))
    return worst
