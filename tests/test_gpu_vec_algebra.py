"""Vector and matrix algebra of pyn_ctx.hip / pyn_krylov.hip against numpy, bit for bit (run on a real MI355X with `-m gpu`).

Element-wise kernels make one rounding per result, so they must equal numpy exactly; where a kernel adds two products (fma or
not) the data are integers.  Reductions are exact on integer data and within the a-priori bound of any summation order on
random data.  Sizes: 4 nodes, 272 nodes (lengths 272 .. 1,632 straddle one block's 256 and 512 entries) and, with block size 6,
1,060,920 entries: more than PYN_MAX_PARTIALS x 512, so the grid cap binds and the grid-stride loops turn."""
import dataclasses
import math

import numpy as np
import pytest

from tests import product_exact as pe
from tests.util import mat_to_scipy

pytestmark = pytest.mark.gpu

MAX_PARTIALS = 2048          # PYN_MAX_PARTIALS
U = 2.0 ** -53
SIZES = {"tiny": (1, 1), "mid": (15, 16), "big": (420, 419)}
PARAMS = [(s, bs) for s in ("tiny", "mid", "ghost") for bs in (1, 2, 3, 6)] + [("big", 6)]


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@pytest.fixture(scope="module")
def ctxs(lib):
    """contexts by size name, made on first use: only mesh_set (the ghosted one: rank 0 of 2, detached, + the node graph)"""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        ctx = lib.Context(0)
        if name == "ghost":
            from pynama_amd.common.comm import Comm
            from pynama_amd.domain.dmplex import DMPlexDom
            dom = DMPlexDom(boxMesh={'nelem': [4, 3, 6], 'lower': [0.0] * 3, 'upper': [1.0] * 3}, comm=Comm(0, 2))
            dom.setFemIndexing(2)
            ctx.comm_init(0, 2, None)
            ctx.halo_set(*dom._halo_plan())
            ctx.mesh_set(3, dom.conn, dom.xyz)
            ctx.csr_symbolic()
            assert ctx.n_ghost > 0
        else:
            mesh = pe.mesh_of(2, SIZES[name])
            ctx.mesh_set(2, mesh.conn, mesh.xyz)
        made[name] = ctx
        return ctx

    yield get
    for c in made.values():
        c.close()


class GhostProbe:
    """reads the ghost entries of a vector through a product: a 1 x bs matrix that is 1 on every ghost column, 0 elsewhere"""

    def __init__(self, ctx, bs):
        rp, ci = ctx.csr_get()
        nl = ctx.n_owned + ctx.n_ghost
        ex = pe.build(rp, ci, 1, bs, n_cols_nodes=nl)
        _, C = pe.storage_index(rp, ci, 1, bs)
        val = (C >= ctx.n_owned * bs).astype(np.int64)
        assert val.sum() > 0
        self.ex = dataclasses.replace(ex, val=val)
        self.E = pe.sp.csr_matrix((val, ci.astype(np.int64).repeat(bs) * bs + np.tile(np.arange(bs), ci.size), rp.astype(np.int64) * bs),
                                  shape=(ctx.n_owned, nl * bs))
        self.ctx, self.bs, self.n = ctx, bs, ctx.n_owned * bs
        self.mid = ctx.mat_create(1, bs)
        pe.upload(ctx, self.mid, self.ex)
        self.vy = ctx.vec_create(1)

    def sums(self, vid):
        self.ctx.spmv(self.mid, vid, self.vy)
        return self.ctx.vec_get(self.vy, 1)

    def expect(self, ghosts):
        full = np.concatenate([np.zeros(self.n), np.asarray(ghosts, np.float64)])
        return self.E @ full


def _ints(rng, n, lo=-9, hi=9):
    return rng.integers(lo, hi + 1, n).astype(np.float64)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("size,bs", PARAMS)
def test_elementwise(ctxs, size, bs):
    ctx = ctxs(size)
    n = ctx.n_owned * bs
    ng = ctx.n_ghost * bs
    rng = np.random.default_rng(7 + bs)
    ghost = size == "ghost"
    probe = GhostProbe(ctx, bs) if ghost else None
    gw = 1000.0 + np.arange(ng)                        # ghosts of every output vector; inputs carry other ghosts

    def put(vid, owned, ghosts=None):
        if ghost:
            ctx.vec_set_local(vid, np.concatenate([owned, gw if ghosts is None else ghosts]))
        else:
            ctx.vec_set(vid, owned)

    def check(vid, ref, what):
        got = ctx.vec_get(vid, bs)
        assert _same(got, ref), f"{what}: {np.count_nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))} of {n} differ"
        if ghost and np.isfinite(ref).all():          # (the probe multiplies the owned entries by 0)
            assert np.array_equal(probe.sums(vid), probe.expect(gw)), f"{what}: ghosts of the output changed"

    vw, vx, vy = (ctx.vec_create(bs) for _ in range(3))
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    xn, yn = x.copy(), y.copy()
    xn[n // 2] = np.nan
    yn[0] = yn[-1] = np.nan
    g7 = np.full(ng, 7.0)

    ctx.vec_fill(vw, 2.5)
    assert np.array_equal(ctx.vec_get(vw, bs), np.full(n, 2.5))
    if ghost:
        assert np.array_equal(probe.sums(vw), probe.expect(np.full(ng, 2.5))), "vec_fill must reach the ghosts"

    # axpby: one term (the other operand is not read, NaN or not), no term, two terms on integers, aliasing
    for a, b, xs, ys, ref in ((1.75, 0.0, x, yn, 0.0 + 1.75 * x), (0.0, -0.3, xn, y, 0.0 + -0.3 * y), (0.0, 0.0, xn, yn, np.zeros(n)),
                              (1.75, 0.0, xn, y, 0.0 + 1.75 * xn)):
        put(vw, np.full(n, 5.0)); put(vx, xs, g7); put(vy, ys, g7)
        ctx.vec_axpby(vw, a, vx, b, vy)
        check(vw, ref, f"axpby a {a} b {b}")
    xi, yi = _ints(rng, n), _ints(rng, n)
    put(vw, np.full(n, 5.0)); put(vx, xi, g7); put(vy, yi, g7)
    ctx.vec_axpby(vw, 3.0, vx, -2.0, vy)
    check(vw, 3.0 * xi - 2.0 * yi, "axpby two terms")
    put(vx, xi); put(vy, yi, g7)
    ctx.vec_axpby(vx, 3.0, vx, -2.0, vy)
    check(vx, 3.0 * xi - 2.0 * yi, "axpby w is x")
    put(vx, xi, g7); put(vy, yi)
    ctx.vec_axpby(vy, 3.0, vx, -2.0, vy)
    check(vy, 3.0 * xi - 2.0 * yi, "axpby w is y")
    put(vx, xi)
    ctx.vec_axpby(vx, 3.0, vx, -2.0, vx)
    check(vx, xi, "axpby w is x is y")

    put(vw, np.full(n, 5.0)); put(vx, x, g7); put(vy, y, g7)
    ctx.vec_pointwise_mult(vw, vx, vy)
    check(vw, x * y, "pointwise_mult")
    put(vx, x)
    ctx.vec_pointwise_mult(vx, vx, vy)
    check(vx, x * y, "pointwise_mult w is x")
    put(vx, x)
    ctx.vec_pointwise_mult(vx, vx, vx)
    check(vx, x * x, "pointwise_mult w is x is y")
    put(vx, x)
    ctx.vec_reciprocal(vx)
    check(vx, 1.0 / x, "reciprocal")

    # scatter: insert at distinct places, add with every index given three times (integers: any order of the atomics)
    m = max(1, n // 3)
    idx = rng.permutation(n)[:m].astype(np.int32)
    vals = rng.standard_normal(m)
    put(vw, x)
    ctx.vec_scatter(vw, idx, vals)
    ref = x.copy()
    ref[idx] = vals
    check(vw, ref, "scatter insert")
    put(vw, xi)
    idx3 = np.concatenate([idx, idx[::-1], idx]).astype(np.int32)
    vals3 = _ints(rng, idx3.size)
    ctx.vec_scatter(vw, idx3, vals3, add=True)
    ref = xi.copy()
    np.add.at(ref, idx3, vals3)
    check(vw, ref, "scatter add, repeated indices")

    if bs in (2, 3):
        nb = 3 if bs == 2 else 6
        vo = ctx.vec_create(nb)
        v = x.reshape(-1, bs)
        if bs == 2:
            ref = np.stack([v[:, 0] * v[:, 0], v[:, 0] * v[:, 1], v[:, 1] * v[:, 1]], axis=1)
        else:
            ref = np.stack([v[:, 0] * v[:, 0], v[:, 0] * v[:, 1], v[:, 1] * v[:, 1], v[:, 1] * v[:, 2], v[:, 2] * v[:, 2],
                            v[:, 2] * v[:, 0]], axis=1)
        go = 2000.0 + np.arange(ctx.n_ghost * nb)
        if ghost:
            ctx.vec_set_local(vo, np.concatenate([np.zeros(ctx.n_owned * nb), go]))
        put(vx, x, g7)
        ctx.vec_vtensv(vx, vo)
        assert np.array_equal(ctx.vec_get(vo, nb), ref.ravel())
        if ghost:
            p2 = GhostProbe(ctx, nb)
            assert np.array_equal(p2.sums(vo), p2.expect(go)), "vtensv: ghosts of the output changed"
            ctx.mat_destroy(p2.mid)
        ctx.vec_destroy(vo)
    for v in (vw, vx, vy):
        ctx.vec_destroy(v)
    if ghost:
        ctx.mat_destroy(probe.mid)


def _places(n):
    """entry 0, the last one, the last of the first grid pass and the first of the second (256 entries per workgroup and pass)"""
    grid = max(1, min((n + 511) // 512, MAX_PARTIALS))
    first = grid * 256
    return sorted({0, n - 1} | ({first - 1, first} if first < n else set()))


@pytest.mark.parametrize("size,bs", PARAMS)
def test_reductions(ctxs, size, bs):
    ctx = ctxs(size)
    n = ctx.n_owned * bs
    ng = ctx.n_ghost * bs
    rng = np.random.default_rng(17 + bs)
    vx, vy = ctx.vec_create(bs), ctx.vec_create(bs)
    if size == "big":
        assert n > MAX_PARTIALS * 512 and len(_places(n)) == 4

    def put(vid, owned):
        if ng:
            ctx.vec_set_local(vid, np.concatenate([owned, np.full(ng, 1e300)]))      # ghost entries never enter a reduction
        else:
            ctx.vec_set(vid, owned)

    # integers: one correct answer
    xi, yi = _ints(rng, n), _ints(rng, n)
    put(vx, xi); put(vy, yi)
    assert ctx.vec_dot(vx, vy) == float(int(xi.astype(np.int64) @ yi.astype(np.int64)))
    assert ctx.vec_norm(vx, 1) == float(int(np.abs(xi).sum()))
    assert ctx.vec_norm(vx, 2) == np.sqrt(np.float64(int((xi.astype(np.int64) ** 2).sum())))
    assert ctx.vec_norm(vx, 3) == np.abs(xi).max()

    # random data: any summation order, fma or not, stays within 2 n u sum |x_i y_i| of the exact sum
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    put(vx, x); put(vy, y)
    ref, mag = math.fsum(x * y), math.fsum(np.abs(x * y))           # the products' own roundings: u |x_i y_i| each, inside the factor 2
    got = ctx.vec_dot(vx, vy)
    print(f"dot n {n}: |got - ref| {abs(got - ref):.3e} bound {2 * n * U * mag:.3e}")
    assert abs(got - ref) <= 2 * n * U * mag
    ref1 = math.fsum(np.abs(x))
    got = ctx.vec_norm(vx, 1)
    print(f"norm1 n {n}: |got - ref| {abs(got - ref1):.3e} bound {2 * n * U * ref1:.3e}")
    assert abs(got - ref1) <= 2 * n * U * ref1
    # ||x||_2 = sqrt(S (1 + d)), |d| <= 2 n u, and sqrt(1 + d) lies within 1 +- |d|; + the roundings of the two square roots and of S
    S = math.fsum(x * x)
    got = ctx.vec_norm(vx, 2)
    print(f"norm2 n {n}: |got - ref| {abs(got - math.sqrt(S)):.3e} bound {math.sqrt(S) * (2 * n + 3) * U:.3e}")
    assert abs(got - math.sqrt(S)) <= math.sqrt(S) * (2 * n + 3) * U
    assert ctx.vec_norm(vx, 3) == np.abs(x).max()

    # one NaN, wherever it sits, reaches dot and all three norms; one +-inf gives inf from all three norms
    one = np.ones(1)
    for k in _places(n):
        at = np.array([k], np.int32)
        ctx.vec_scatter(vx, at, one * np.nan)
        assert math.isnan(ctx.vec_dot(vx, vy)) and math.isnan(ctx.vec_dot(vy, vx)), f"dot, NaN at {k} of {n}"
        for t in (1, 2, 3):
            assert math.isnan(ctx.vec_norm(vx, t)), f"norm type {t}, NaN at {k} of {n}"
        for v in (np.inf, -np.inf):
            ctx.vec_scatter(vx, at, one * v)
            for t in (1, 2, 3):
                assert ctx.vec_norm(vx, t) == np.inf, f"norm type {t}, {v} at {k} of {n}"
        ctx.vec_scatter(vx, at, x[k:k + 1])
    assert ctx.vec_norm(vx, 3) == np.abs(x).max()
    ctx.vec_destroy(vx)
    ctx.vec_destroy(vy)


MAT_MESHES = {"2d": (2, (9, 7)), "3d": (2, (4, 3, 5))}


@pytest.mark.parametrize("block", [(1, 1), (2, 2), (3, 3), (3, 2)], ids=lambda b: f"{b[0]}x{b[1]}")
@pytest.mark.parametrize("mname", list(MAT_MESHES))
def test_matrix_algebra(lib, mname, block):
    ngl, nelem = MAT_MESHES[mname]
    mesh = pe.mesh_of(ngl, nelem)
    br, bc = block
    ctx = lib.Context(0)
    try:
        ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
        ctx.csr_symbolic()
        rp, ci = ctx.csr_get()
        X, Y = pe.build(rp, ci, br, bc, seed=1), pe.build(rp, ci, br, bc, seed=2)
        mx, my = ctx.mat_create(br, bc), ctx.mat_create(br, bc)
        XA, YA = X.A.astype(np.float64), Y.A.astype(np.float64)

        def equal(mid, ref):
            d = abs(mat_to_scipy(ctx, mid, br, bc) - ref)
            return d.nnz == 0 or d.max() == 0

        pe.upload(ctx, mx, X)
        assert equal(mx, XA)
        for a in (0.0, 1.0, -1.0, 0.5):
            pe.upload(ctx, my, Y)
            ctx.mat_axpy(my, a, mx)
            assert equal(my, YA + a * XA), f"mat_axpy a {a}"
            pe.upload(ctx, my, Y)
            ctx.mat_axpy(my, a, my)
            assert equal(my, YA + a * YA), f"mat_axpy a {a}, y is x"

        rng = np.random.default_rng(5)
        n = ctx.n_owned
        for sbs in {br, 1}:
            s = rng.integers(-3, 4, n * sbs).astype(np.float64)
            vs = ctx.vec_create(sbs)
            ctx.vec_set(vs, s)
            pe.upload(ctx, my, Y)
            ctx.mat_row_scale(my, vs)
            per_row = s if sbs == br else np.repeat(s, br)
            assert equal(my, pe.sp.diags(per_row) @ YA), f"mat_row_scale, vector block size {sbs}"
        if br == bc:
            vd = ctx.vec_create(br)
            ctx.mat_diagonal(mx, vd)
            assert np.array_equal(ctx.vec_get(vd, br), XA.diagonal())

        # mat_add_values on top of the inserted values
        pe.upload(ctx, my, Y)
        i = n // 2
        lo, hi = int(rp[i]), int(rp[i + 1])
        rows = i * br + np.arange(br)
        cols = (ci[lo:hi, None].astype(np.int64) * bc + np.arange(bc)[None, :]).ravel()
        blk = rng.integers(-5, 6, (br, cols.size)).astype(np.float64)
        ctx.mat_add_values(my, rows, cols, blk)
        ref = YA.tolil()
        ref[np.ix_(rows, cols)] = ref[np.ix_(rows, cols)].toarray() + blk
        assert equal(my, ref.tocsr()), "add after insert"
        # a repeated (row, column) in ONE call accumulates; negative rows / columns are ignored
        r0, c0 = int(rows[0]), int(cols[-1])
        ctx.mat_add_values(my, [r0, -1, r0], [c0, -3, c0], np.array([[1., 100., 2.], [100., 100., 100.], [4., 100., 8.]]))
        ref[r0, c0] += 15.0
        assert equal(my, ref.tocsr()), "repeated entry / negative indices"
        far = int(np.setdiff1d(np.arange(n), ci[lo:hi])[0])          # a node that row i is not coupled to
        with pytest.raises(lib.PynamaHipError):
            ctx.mat_add_values(my, [r0], [far * bc], [1.0])
        ctx.mat_zero(my)
        assert not ctx.mat_values(my, br, bc).any()
    finally:
        ctx.close()
