"""Geometric multigrid preconditioner for CG on structured lattice meshes (pynama_amd/csrc/pyn_mg.hip): the Galerkin coarse
operators against P^T A P built independently in scipy from the lattice coordinates, one V-cycle against a numpy restatement, the
symmetry of the preconditioner, CG+MG against Jacobi-PCG (iterations, mesh independence, solution; assembled and matrix-free level 0),
the hierarchy cache, the refusals and the KspSolver facade."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import fem_oracle as fo
from tests.test_gpu_ho3 import boundary_mask, make_ctx
from tests.util import mat_to_scipy, rel_err, sp_rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


# ---- independent restatement: lattice, P, decoupled DOFs, Galerkin operators ----------------------------------------------------
def lattice_of(mesh, nel, ngl):
    """nodes per axis and the node id at every lattice point [x, y(, z)] of a unit box mesh"""
    nper = [(ngl - 1) * e + 1 for e in nel]
    c = np.rint(mesh.xyz * (np.array(nper) - 1)).astype(int)
    ids = np.full(nper, -1, np.int64)
    ids[tuple(c.T)] = np.arange(mesh.n_node)
    assert (ids >= 0).all()
    return nper, ids


def lex_ids(nper):
    """lexicographic numbering (x fastest) of a coarse level, indexed [x, y(, z)]"""
    return np.arange(int(np.prod(nper))).reshape(nper[::-1]).T


def interpolation(ids_f, nper_f, nper_c):
    """scalar P (fine nodes x coarse nodes): tensor-product linear interpolation, coarse node I at fine node 2I"""
    rows, cols, vals = [], [], []
    ids_c = lex_ids(nper_c)
    for f in itertools.product(*[range(n) for n in nper_f]):
        par = [[(x // 2, 1.0)] if x % 2 == 0 else [((x - 1) // 2, 0.5), ((x + 1) // 2, 0.5)] for x in f]
        for combo in itertools.product(*par):
            rows.append(ids_f[f])
            cols.append(ids_c[tuple(p for p, _ in combo)])
            vals.append(np.prod([w for _, w in combo]))
    return sp.csr_matrix((vals, (rows, cols)), shape=(int(np.prod(nper_f)), int(np.prod(nper_c))))


def decoupled(A):
    off = (A - sp.diags(A.diagonal())).tocsr()
    off.eliminate_zeros()
    return np.diff(off.indptr) == 0


def galerkin_levels(A, ids0, nper0, b, nlev):
    """[(A_l, P_l (to level l+1), dec_l, nper_l)] with P zero in decoupled fine rows and decoupled coarse columns, and the
    decoupled coarse rows given the coincident fine diagonal"""
    out = []
    ids, nper, dec = ids0, list(nper0), decoupled(A)
    for l in range(nlev):
        if l == nlev - 1:
            out.append((A, None, dec, nper))
            break
        nper_c = [(n - 1) // 2 + 1 for n in nper]
        coinc = np.empty(int(np.prod(nper_c)), np.int64)
        idc = lex_ids(nper_c)
        for c in itertools.product(*[range(n) for n in nper_c]):
            coinc[idc[c]] = ids[tuple(2 * x for x in c)]
        dof_c = (coinc[:, None] * b + np.arange(b)).ravel()
        dec_c = dec[dof_c]
        P = sp.kron(interpolation(ids, nper, nper_c), sp.eye(b)).tocsr()
        P = sp.diags((~dec).astype(float)) @ P @ sp.diags((~dec_c).astype(float))
        Ac = (P.T @ A @ P).tolil()
        dA = A.diagonal()
        for r in np.nonzero(dec_c)[0]:
            Ac[r, r] = dA[dof_c[r]]
        out.append((A, P.tocsr(), dec, nper))
        A, ids, nper, dec = Ac.tocsr(), idc, nper_c, dec_c
    return out


def stencil_to_scipy(S, nper, b):
    """[node][3^d][b][b] -> sparse, nodes lexicographic; entries that point outside the lattice must be zero"""
    dim = len(nper)
    ids = lex_ids(nper)
    rows, cols, vals = [], [], []
    for c in itertools.product(*[range(n) for n in nper]):
        I = ids[c]
        for k, off in enumerate(itertools.product(*[(-1, 0, 1)] * dim)):
            o = off[::-1]                            # itertools varies the last axis fastest; offsets are x fastest
            J = tuple(ci + oi for ci, oi in zip(c, o))
            blk = S[I, k]
            if all(0 <= j < n for j, n in zip(J, nper)):
                for p in range(b):
                    for q in range(b):
                        rows.append(I * b + p)
                        cols.append(ids[J] * b + q)
                        vals.append(blk[p, q])
            else:
                assert not blk.any()
    n = int(np.prod(nper)) * b
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def system(lib, case, nel, mask_kind):
    """(ctx, matrix id, A scipy, b, nper, ids) of the four checked operators"""
    dim = len(nel)
    ngl = 2 if case in ("q1hex", "q1lap") else 3
    mesh = fo.box_mesh(nel, [0.0] * dim, [1.0] * dim, ngl)
    b = 1 if case == "q1lap" else dim
    mask = np.zeros((mesh.n_node, b), np.uint8)
    mask[mesh.boundary] = 1
    if mask_kind == "partial":
        mask = (np.random.default_rng(5).random((mesh.n_node, b)) < 0.25).astype(np.uint8)
    ctx = make_ctx(lib, mesh, mask if b > 1 else mask[:, 0], b, ngl=ngl)
    M = ctx.mat_create(b, b)
    if case == "q1lap":
        ctx.assemble_scalar(lib.FORM_LAPLACE, M)
    else:
        ctx.assemble_kle(1e3, 1e2, M)
    nper, ids = lattice_of(mesh, nel, ngl)
    return ctx, M, mat_to_scipy(ctx, M, b, b), b, nper, ids


CASES = [("ho3", [8, 8], 20), ("ho3", [4, 4, 4], 100), ("q1hex", [8, 8, 8], 100), ("q1lap", [8, 8], 10)]


@pytest.mark.parametrize("mask_kind", ["faces", "partial"])
@pytest.mark.parametrize("case,nel,cmax", CASES)
def test_galerkin_levels(lib, case, nel, cmax, mask_kind):
    """every coarse level == P^T A P of the scipy restatement (1e-12 relative)"""
    ctx, M, A, b, nper, ids = system(lib, case, nel, mask_kind)
    ctx.mg_setup(M, coarse_max_rows=cmax)
    info = ctx.mg_info(M)
    assert info["levels"] >= 3 and info["rows"][0] == A.shape[0]
    ref = galerkin_levels(A, ids, nper, b, info["levels"])
    for l in range(1, info["levels"]):
        Al, _, _, nl = ref[l]
        assert info["rows"][l] == Al.shape[0]
        S = ctx.mg_level_get(M, l, b)
        assert sp_rel_err(stencil_to_scipy(S, nl, b), Al) < 1e-12, l
    ctx.close()


def numpy_vcycle(levels, lam, k, r, l=0, emin=0.1, emax=1.1):
    A, P, dec, _ = levels[l]
    if P is None:
        return spla.spsolve(A.tocsc(), r)
    diag = A.diagonal()
    dinv = 1.0 / diag

    def smooth(z, zero):
        lo, hi = emin * lam[l], emax * lam[l]
        theta, delta = (hi + lo) / 2, (hi - lo) / 2
        sigma = theta / delta
        rho, d = 0.0, None
        for j in range(k):
            t = r if (zero and j == 0) else r - A @ z
            if j == 0:
                rho, d = 1.0 / sigma, dinv * t / theta
            else:
                rn = 1.0 / (2 * sigma - rho)
                d, rho = rn * rho * d + 2 * rn / delta * dinv * t, rn
            z = d.copy() if (zero and j == 0) else z + d
            z[dec] = r[dec] / diag[dec]
        return z

    z = smooth(np.zeros_like(r), True)
    ec = numpy_vcycle(levels, lam, k, P.T @ (r - A @ z), l + 1, emin, emax)
    return smooth(z + P @ ec, False)


@pytest.mark.parametrize("degree", [2, 3])
def test_vcycle_matches_numpy(lib, degree):
    """one V-cycle (mg_apply) == the numpy restatement from mg_info's lambda estimates (1e-11)"""
    ctx, M, A, b, nper, ids = system(lib, "ho3", [4, 4], "faces")
    ctx.mg_setup(M, coarse_max_rows=20, smooth_degree=degree)
    info = ctx.mg_info(M)
    assert info["levels"] == 3 and all(v > 0 for v in info["lambda"][:-1])
    levels = galerkin_levels(A, ids, nper, b, info["levels"])
    r = np.random.default_rng(2).standard_normal(A.shape[0])
    vr, vz = ctx.vec_create(b), ctx.vec_create(b)
    ctx.vec_set(vr, r)
    ctx.mg_apply(M, vr, vz)
    ref = numpy_vcycle(levels, info["lambda"], degree, r)
    assert rel_err(ctx.vec_get(vz, b), ref) < 1e-11
    ctx.close()


@pytest.mark.parametrize("case,nel,cmax", [("ho3", [8, 8], 20), ("ho3", [4, 4, 4], 100), ("q1lap", [8, 8], 10)])
def test_preconditioner_is_spd(lib, case, nel, cmax):
    """u' M^-1 v == v' M^-1 u, u' M^-1 u > 0; decoupled rows give r / a_ii"""
    ctx, M, A, b, nper, ids = system(lib, case, nel, "faces")
    ctx.mg_setup(M, coarse_max_rows=cmax)
    n = A.shape[0]
    rng = np.random.default_rng(11)
    vecs = [ctx.vec_create(b) for _ in range(4)]
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    ctx.vec_set(vecs[0], u)
    ctx.vec_set(vecs[1], v)
    ctx.mg_apply(M, vecs[0], vecs[2])
    ctx.mg_apply(M, vecs[1], vecs[3])
    Mu, Mv = ctx.vec_get(vecs[2], b), ctx.vec_get(vecs[3], b)
    assert abs(u @ Mv - v @ Mu) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv)
    assert u @ Mu > 0 and v @ Mv > 0
    dec = decoupled(A)
    assert dec.any()
    assert np.array_equal(Mu[dec], u[dec] / A.diagonal()[dec])
    ctx.close()


def kle_system(lib, dim, nel):
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.elements.spectral import Spectral
    dom = DMPlexDom(boxMesh={"nelem": [nel] * dim, "lower": [0] * dim, "upper": [1] * dim})
    dom.setFemIndexing(3)
    ctx = dom.ctx
    for t in Spectral(3, dim).deviceTables():
        ctx.tables_set(*t)
    bm = dom.boundaryMaskLocal()
    ctx.bc_set(dim, np.repeat(bm[:, None], dim, axis=1))
    n_rows, _ = ctx.csr_symbolic()
    K = ctx.mat_create(dim, dim)
    ctx.assemble_kle(1e3, 1e2, K)
    ctx.matfree_set(lib.MATFREE_KLE, 1e3, 1e2)
    rhs = np.random.default_rng(0).standard_normal(n_rows * dim)
    rhs[np.repeat(bm != 0, dim)] = 0.0
    vb, vx = ctx.vec_create(dim), ctx.vec_create(dim)
    ctx.vec_set(vb, rhs)
    return dom, ctx, K, vb, vx


@pytest.mark.parametrize("matfree", [False, True])
@pytest.mark.parametrize("dim,sizes", [(2, (64, 256)), (3, (8, 16))])
def test_cg_mg_converges_mesh_independently(lib, dim, sizes, matfree):
    """CG+MG to rtol 1e-10: true residual <= 1e-9, the same solution as Jacobi-PCG (1e-8), at most 2x more iterations on the finer
    mesh, with the assembled product and with the ngl 3 shell at level 0.  Iterations against Jacobi-PCG's (measured with the
    default degree 2 on an MI355X): 2-D 106 / 1,026 at 64^2, 124 / 4,007 at 256^2; 3-D 101 / 314 at 8^3, 175 / 558 at 16^3 -- the
    penalty terms of K (alpha_d = 1e3 on div, reduced rule) are what point smoothers and Q1 coarse spaces handle worst, so the
    reduction reaches 10x only on the large 2-D mesh."""
    its = []
    for nel in sizes:
        dom, ctx, K, vb, vx = kle_system(lib, dim, nel)
        mf = lib.MATFREE_KLE if matfree else lib.MATFREE_OFF
        kw = dict(rtol=1e-10, atol=1e-300, maxit=200000, norm_type=lib.NORM_UNPRECONDITIONED, matfree=mf)
        ij = ctx.solve(K, vb, vx, pc=lib.PC_JACOBI, **kw)
        xj = ctx.vec_get(vx, dim)
        im = ctx.solve(K, vb, vx, pc=lib.PC_MG, **kw)
        xm = ctx.vec_get(vx, dim)
        assert ij.reason == 2 and im.reason == 2, (ij.reason, im.reason)
        assert im.true_resid <= 1e-9
        assert 2 * im.iters <= ij.iters, (nel, im.iters, ij.iters)
        if dim == 2 and nel == sizes[1]:
            assert 10 * im.iters <= ij.iters, (nel, im.iters, ij.iters)
        assert rel_err(xm, xj) < 1e-8
        its.append(im.iters)
        ctx.close()
    assert its[1] <= 2 * its[0], its


def test_hierarchy_cache(lib):
    """a second solve does not rebuild; new values (mat_zero + assembly with other data) do, and equal a fresh hierarchy"""
    dom, ctx, K, vb, vx = kle_system(lib, 2, 32)
    kw = dict(pc=lib.PC_MG, rtol=1e-10, atol=1e-300, norm_type=lib.NORM_UNPRECONDITIONED)
    ctx.solve(K, vb, vx, **kw)
    n0 = ctx.mg_info(K)["builds"]
    i1 = ctx.solve(K, vb, vx, **kw)
    assert ctx.mg_info(K)["builds"] == n0
    ctx.mg_setup(K)                                    # same (default) options, same values: no rebuild
    assert ctx.mg_info(K)["builds"] == n0
    ctx.mat_zero(K)
    ctx.assemble_kle(2e3, 3e2, K)
    i2 = ctx.solve(K, vb, vx, **kw)
    x2 = ctx.vec_get(vx, 2)
    info = ctx.mg_info(K)
    assert info["builds"] == n0 + 1 and i2.reason == 2 and i1.reason == 2
    K2 = ctx.mat_create(2, 2)
    ctx.assemble_kle(2e3, 3e2, K2)
    ctx.mg_setup(K2)
    info2 = ctx.mg_info(K2)
    assert info2["rows"] == info["rows"]
    assert np.allclose(info2["lambda"], info["lambda"], rtol=1e-10, atol=0)
    for l in range(1, info["levels"]):
        assert rel_err(ctx.mg_level_get(K, l, 2), ctx.mg_level_get(K2, l, 2)) < 1e-13
    i3 = ctx.solve(K2, vb, vx, **kw)
    assert abs(i3.iters - i2.iters) <= 1 and rel_err(ctx.vec_get(vx, 2), x2) < 1e-9
    ctx.mg_setup(K2, smooth_degree=3)                  # other options rebuild
    assert ctx.mg_info(K2)["builds"] == info2["builds"] + 1
    ctx.close()


def test_refusals(lib):
    """each refusal raises with its message"""
    # general (kind 0) mesh: a Q1 hex box whose node numbering is shuffled
    mesh = fo.box_mesh([4, 4, 4], [0.0] * 3, [1.0] * 3, 2)
    perm = np.random.default_rng(1).permutation(mesh.n_node)
    inv = np.argsort(perm)
    mesh.conn = inv[mesh.conn].astype(mesh.conn.dtype)
    mesh.xyz = mesh.xyz[perm]
    ctx = make_ctx(lib, mesh, None, 3, ngl=2)
    assert ctx.mesh_topology()[0] == "general"
    K = ctx.mat_create(3, 3)
    ctx.assemble_kle(1e3, 1e2, K)
    with pytest.raises(lib.PynamaHipError, match="general connectivity"):
        ctx.mg_setup(K)
    ctx.close()
    # 2-D ngl 3 lattice: non-square blocks, compact rhs, too few levels, coarsest above the dense limit, GMRES, several ranks
    mesh = fo.box_mesh([16, 16], [0.0] * 2, [1.0] * 2, 3)
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), 2)
    K = ctx.mat_create(2, 2)
    ctx.assemble_kle(1e3, 1e2, K)
    with pytest.raises(lib.PynamaHipError, match="square blocks"):
        ctx.mg_setup(ctx.mat_create(2, 1))
    with pytest.raises(lib.PynamaHipError, match="compact imposed-column"):
        ctx.mg_setup(ctx.mat_create_rhs(2, 2))
    with pytest.raises(lib.PynamaHipError, match="fewer than 2 levels"):
        ctx.mg_setup(K)                                 # 33^2 nodes = 2,178 rows <= 4096
    with pytest.raises(lib.PynamaHipError, match="fewer than 2 levels"):
        ctx.mg_setup(K, coarse_max_rows=20, max_levels=1)
    vb, vx = ctx.vec_create(2), ctx.vec_create(2)
    with pytest.raises(lib.PynamaHipError, match="CG only"):
        ctx.solve(K, vb, vx, method=lib.KSP_GMRES, pc=lib.PC_MG)
    ctx.comm_init(0, 2, None)                           # detached second rank
    with pytest.raises(lib.PynamaHipError, match="one rank"):
        ctx.mg_setup(K, coarse_max_rows=20)
    ctx.close()
    mesh = fo.box_mesh([65, 65], [0.0] * 2, [1.0] * 2, 3)   # 130 cells per axis: one halving, 66^2 nodes = 8,712 rows
    ctx = make_ctx(lib, mesh, boundary_mask(mesh), 2)
    K = ctx.mat_create(2, 2)
    ctx.assemble_kle(1e3, 1e2, K)
    with pytest.raises(lib.PynamaHipError, match="above the dense LU limit"):
        ctx.mg_setup(K)
    ctx.close()


def test_facade_solveKLE_uniform():
    """UniformFlow.solveKLE with -ksp_type cg -pc_type mg -ksp_rtol 1e-12 (2-D 10x10 and 3-D 3^3 ngl 3) reproduces the exact
    uniform flow, checked as tests/test_gpu_api.py checks the Jacobi-PCG run (src/tests/test_solver.py:20-27, 52-62)"""
    import pynama_amd
    from tests.test_gpu_api import setFemProblem
    from common.options import Options
    pynama_amd.install_reference_layout()
    base = ["-ksp_type", "cg", "-pc_type", "mg", "-ksp_rtol", "1e-12", "-ksp_norm_type", "unpreconditioned",
            "-pynama_mg_coarse_max_rows", "100"]
    try:
        for kw in ({}, dict(lower=[0, 0, 0], upper=[1, 1, 1], nelem=[3, 3, 3], ngl=3)):
            Options(base)
            fem = setFemProblem('uniform', **kw)
            exactVel, exactVort = fem.generateExactVecs()
            fem.solveKLE(time=0.0, vort=exactVort)
            assert fem.solver.getConvergedReason() == 2
            assert fem.solver.info.true_resid <= 1e-10
            assert (exactVel - fem.vel).norm(norm_type=3) < 1e-8
            A = fem.solver.mat
            assert A.ctx.mg_info(A.id)["levels"] >= 2
    finally:
        Options([])
