"""numpy / scipy restatement of the multigrid hierarchy on box lattices of order ngl >= 4 (pynama_amd/csrc/pyn_mg.hip): the step P0
from the GLL node lattice to the Q1 lattice of the same cells, the 2:1 levels below it, the decoupling rule, the Chebyshev V-cycle of
tests/test_gpu_mg.py and PCG around it.  Shared by tests/test_mg_ho_host.py (no GPU) and tests/test_gpu_mg_ho.py."""
import itertools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import fem_oracle as fo
from tests.test_gpu_mg import decoupled, interpolation, lex_ids, numpy_vcycle


def ho_lattice_of(mesh, nel, ngl):
    """nodes per axis and the node id at every lattice point [x, y(, z)] of a box mesh of order ngl (GLL spacing inside a cell)"""
    nper = [(ngl - 1) * e + 1 for e in nel]
    c = np.empty((mesh.n_node, len(nel)), np.int64)
    for a, n in enumerate(nper):
        u, inv = np.unique(np.round(mesh.xyz[:, a], 12), return_inverse=True)
        assert len(u) == n
        c[:, a] = inv.ravel()
    ids = np.full(nper, -1, np.int64)
    ids[tuple(c.T)] = np.arange(mesh.n_node)
    assert (ids >= 0).all()
    return nper, ids


def p0_1d(E, ngl):
    """1-D rule: fine node x of cell e = min(x div m, E - 1), local node i = x - e m, takes (1 - xi_i) / 2 of coarse node e and
    (1 + xi_i) / 2 of e + 1; at a cell vertex the one coincident coarse node, weight exactly 1"""
    m = ngl - 1
    xi = fo.gauss_lobatto(ngl)[0]
    P = np.zeros((m * E + 1, E + 1))
    for x in range(m * E + 1):
        e = min(x // m, E - 1)
        i = x - e * m
        if i == 0:
            P[x, e] = 1.0
        elif i == m:
            P[x, e + 1] = 1.0
        else:
            P[x, e] = (1.0 - xi[i]) / 2
            P[x, e + 1] = (1.0 + xi[i]) / 2
    return P


def interpolation_ho(ids_f, nel, ngl):
    """scalar P0 (fine nodes x coarse nodes, coarse nodes lexicographic): tensor product of the 1-D rule over the axes"""
    P = sp.csr_matrix(np.ones((1, 1)))
    for E in nel:                                   # x fastest: kron(Pz, kron(Py, Px))
        P = sp.kron(sp.csr_matrix(p0_1d(E, ngl)), P, format="csr")
    fine_of_lex = ids_f.T.ravel()                   # lexicographic fine index (x fastest) -> node id
    n = fine_of_lex.size
    perm = sp.csr_matrix((np.ones(n), (fine_of_lex, np.arange(n))), shape=(n, n))
    return (perm @ P).tocsr()


def ho_levels(A, ids0, nel, ngl, b, nlev):
    """[(A_l, P_l (to level l+1), dec_l, nper_l)] as tests/test_gpu_mg.py::galerkin_levels, with P0 as the first step: P zero in
    decoupled fine rows and decoupled coarse columns, decoupled coarse rows given the coincident fine diagonal"""
    m = ngl - 1
    out = []
    ids, nper, dec = ids0, [m * e + 1 for e in nel], decoupled(A)
    for l in range(nlev):
        if l == nlev - 1:
            out.append((A, None, dec, nper))
            break
        s = m if l == 0 else 2
        assert all((n - 1) % s == 0 for n in nper)
        nper_c = [(n - 1) // s + 1 for n in nper]
        idc = lex_ids(nper_c)
        coinc = np.empty(int(np.prod(nper_c)), np.int64)
        for c in itertools.product(*[range(n) for n in nper_c]):
            coinc[idc[c]] = ids[tuple(s * x for x in c)]
        dof_c = (coinc[:, None] * b + np.arange(b)).ravel()
        dec_c = dec[dof_c]
        Ps = interpolation_ho(ids, nel, ngl) if l == 0 else interpolation(ids, nper, nper_c)
        P = sp.kron(Ps, sp.eye(b)).tocsr()
        P = sp.diags((~dec).astype(float)) @ P @ sp.diags((~dec_c).astype(float))
        Ac = (P.T @ A @ P).tolil()
        dA = A.diagonal()
        for r in np.nonzero(dec_c)[0]:
            Ac[r, r] = dA[dof_c[r]]
        out.append((A, P.tocsr(), dec, nper))
        A, ids, nper, dec = Ac.tocsr(), idc, nper_c, dec_c
    return out


def ho_level_count(nel, ngl, b, coarse_max_rows=4096, max_levels=16):
    """the library's level rule: the first step always possible, every later one needs even cell counts; stop at <= coarse_max_rows"""
    cells, nlev = list(nel), 1
    rows = int(np.prod([(ngl - 1) * e + 1 for e in cells])) * b
    while nlev < max_levels and rows > coarse_max_rows:
        if nlev > 1:
            if any(e % 2 for e in cells):
                break
            cells = [e // 2 for e in cells]
        rows = int(np.prod([e + 1 for e in cells])) * b
        nlev += 1
    return nlev


def exact_lambdas(levels):
    """lambda_max(D^-1 A) of every smoothed level"""
    lam = []
    for A, P, _, _ in levels:
        if P is None:
            lam.append(0.0)
            continue
        s = sp.diags(1.0 / np.sqrt(A.diagonal()))
        lam.append(float(spla.eigsh((s @ A @ s).tocsc(), k=1, which="LA", return_eigenvectors=False, tol=1e-10)[0]))
    return lam


def pcg(A, rhs, prec, rtol=1e-10, maxit=100000):
    """PCG from zero, stopped on the unpreconditioned residual norm: (x, iterations)"""
    x = np.zeros_like(rhs)
    r = rhs.copy()
    z = prec(r)
    p = z.copy()
    rz = r @ z
    stop = rtol * np.linalg.norm(rhs)
    for it in range(1, maxit + 1):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if np.linalg.norm(r) <= stop:
            return x, it
        z = prec(r)
        rz1 = r @ z
        p = z + (rz1 / rz) * p
        rz = rz1
    return x, maxit


def jacobi_pcg(A, rhs, rtol=1e-10):
    dinv = 1.0 / A.diagonal()
    return pcg(A, rhs, lambda r: dinv * r, rtol)


def mg_pcg(levels, lam, degree, rhs, rtol=1e-10):
    """PCG preconditioned with one V-cycle (tests/test_gpu_mg.py::numpy_vcycle) per iteration"""
    return pcg(levels[0][0], rhs, lambda r: numpy_vcycle(levels, lam, degree, r), rtol)
