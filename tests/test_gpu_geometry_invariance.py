"""Every kernel that reads node coordinates, far from the origin, at another scale and at another aspect ratio, against references
that are exact by construction (tests/geometry_cases.py): the float64 oracle of the BASE mesh under an exact translation, the base
result times an exact power of two under scaling, the oracle of the same mesh under an anisotropic stretch.

Bars.
  translate   e_D <= max(FP_TOL, 16 e_O).  e_D: device on y = fl(x + t) against the oracle on xb = y - t (sp_rel_err / rel_err);
              e_O: the oracle (or the numpy model) on y against itself on xb, computed in the same test: what absolute coordinates
              cost a plain float64 evaluation, about eps kappa.  16 covers summation order, FMA contraction and the luck of one
              realisation; a conditioning defect costs another factor kappa (1e4 and more here).
  scale       FP_TOL against the device's base result times the exact factor, and against the oracle times it.  Whether the device
              results are identical bit for bit is printed (they should be: every threshold is meant to be relative), next to
              whether two runs of the base are: the kernels that add in no fixed order differ in the last bit by themselves.
  stretch     FP_TOL against the oracle on the same mesh.
  probes      found, cells and path identical to the base mesh's, every inside point found, xi within 16 x the model's own
              base-to-moved difference (the model works from differences: that difference is zero, so xi is identical), samples
              within that times the field's gradient bound.
Every case asserts the kernel family it ran on the base mesh (Context.assemble_last with its closed-form slots, a REQUIRE switch,
Context.ho3_geometry for the diagonal / full J^-1 form of the row-run kernels and of the second-order matrix-free operator, probe
path, acceptance by pyn_matfree_set) and that the moved mesh ran the same one with the same slots; the family is printed in the assertion message."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from tests import geometry_cases as gc
from tests import ibm_model
from tests import integrals_model as im
from tests import probe_model as pm
from tests.util import mat_to_scipy, rel_err

pytestmark = pytest.mark.gpu

FP_TOL = gc.FP_TOL
TNAMES = list(gc.TRANSFORMS)
ALPHA = (1e3, 1e2)


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    assert _lib.device_count() > 0, "GPU tests need an MI355X"
    return _lib


@contextmanager
def switches(names):
    """the switches are read per assembly call: set for the block, the previous values restored after it"""
    old = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def element_of(mesh):
    if gc.is_simplex(mesh):
        from pynama_amd.elements.simplex import Simplex
        return Simplex(mesh.dim)
    from pynama_amd.elements.spectral import Spectral
    return Spectral(mesh.ngl, mesh.dim)


def open_ctx(lib, mesh, symbolic=True):
    ctx = lib.Context(0)
    ctx.mesh_set(mesh.dim, mesh.conn, mesh.xyz)
    for t in element_of(mesh).deviceTables():
        ctx.tables_set(*t)
    if symbolic:
        ctx.csr_symbolic()
    return ctx


def node_mask(mesh, ndof):
    m = np.zeros((mesh.n_node, ndof), np.uint8)
    m[mesh.boundary] = 1
    return m


def set_vec(ctx, u):
    u = np.asarray(u, dtype=np.float64)
    v = ctx.vec_create(1 if u.ndim == 1 else u.shape[1])
    ctx.vec_set(v, u.ravel())
    return v


def family(lib, ctx):
    rec = ctx.assemble_last()
    rec.pop("count")
    rec["kind"] = lib.ASSEMBLY_KINDS[rec["kind"]]
    return rec


def report(tag, op, e_d, e_o, bound, fam=""):
    ratio = e_d / e_o if e_o > 0 else float("nan")
    print(f"GEOM {tag} {op}: e_D {e_d:.2e} e_O {e_o:.2e} ratio {ratio:.2f} bound {bound:.2e} {fam}")


# ---- assembly through the C ABI ----------------------------------------------------------------------------------------------------------
def ops_of(case, mesh):
    return gc.KLE_OPS + gc.SCALAR_OPS + (gc.OPERATOR_OPS if case.operators else ())


def device_matrices(lib, case, mesh, masked):
    """({name: scipy matrix}, {group: family record}) of one context on `mesh`: the operators and their lumped row scaling first (no
    Dirichlet set), then K / Krhs / Rw (masked: boundary nodes imposed, and the compact Krhs as well), then the scalar forms"""
    dim = mesh.dim
    dw = 1 if dim == 2 else 3
    ctx = open_ctx(lib, mesh)
    out, fam = {}, {}
    with switches(case.require):
        if case.plan:
            from tests.test_gpu_kernels import tile_plan
            for kind in (0, 1):
                ctx.patch_plan_set(*tile_plan(mesh, case.plan), kind=kind)
        if case.operators:
            mass = ctx.mat_create(1, 1)
            ctx.assemble_scalar(lib.FORM_MASS_NODAL, mass, -1, 0)
            vw = ctx.vec_create(1)
            ctx.mat_diagonal(mass, vw)
            w = ctx.vec_get(vw, 1)
            for name, (br, bc, terms, coef) in ((n, element_of(mesh).operatorTerms()[n]) for n in gc.OPERATOR_OPS):
                m = ctx.mat_create(br, bc)
                ctx.assemble_operator(lib.Q_NODAL, terms, coef, m)
                fam["operators"] = family(lib, ctx)
                vs = ctx.vec_create(br)
                ctx.vec_set(vs, np.repeat(1.0 / w, br))
                ctx.mat_row_scale(m, vs)
                out[name] = mat_to_scipy(ctx, m, br, bc)
        if masked:
            ctx.bc_set(dim, node_mask(mesh, dim))
        K, Krhs, Rw = ctx.mat_create(dim, dim), ctx.mat_create(dim, dim), ctx.mat_create(dim, dw)
        ctx.assemble_kle(*ALPHA, K, Krhs, Rw, -1)
        fam["kle"] = family(lib, ctx)
        out.update(K=mat_to_scipy(ctx, K, dim, dim), Krhs=mat_to_scipy(ctx, Krhs, dim, dim), Rw=mat_to_scipy(ctx, Rw, dim, dw))
        if masked:
            K2, Krc = ctx.mat_create(dim, dim), ctx.mat_create_rhs(dim, dim)
            ctx.assemble_kle(*ALPHA, K2, Krc, -1, -1)
            fam["kle_compact"] = family(lib, ctx)
            out["Krhs_compact"] = mat_to_scipy(ctx, Krc, dim, dim)
            ctx.bc_set(1, node_mask(mesh, 1))
        A, Ar, M = ctx.mat_create(1, 1), ctx.mat_create(1, 1), ctx.mat_create(1, 1)
        ctx.assemble_scalar(lib.FORM_LAPLACE, A, Ar)
        fam["laplace"] = family(lib, ctx)
        ctx.assemble_scalar(lib.FORM_MASS_NODAL, M, -1)
        fam["mass"] = family(lib, ctx)
        out.update(laplace=mat_to_scipy(ctx, A, 1, 1), Arhs=mat_to_scipy(ctx, Ar, 1, 1), mass=mat_to_scipy(ctx, M, 1, 1))
    fam["geometry"] = ctx.ho3_geometry()                              # the row-run pre-pass: affine, and diagonal or full J^-1
    ctx.close()
    return out, fam


_BASE = {}


def base_run(lib, case, mesh, masked):
    """the device's matrices and families on the case's own mesh, once per module; the families are those the case names"""
    key = (case.name, masked)
    if key not in _BASE:
        got, fam = device_matrices(lib, case, mesh, masked)
        for group, want in (("kle", case.kle), ("laplace", case.laplace), ("operators", case.operators)):
            if want:
                assert fam[group]["kind"] == want, f"{case.name}: {group} assembled by {fam[group]['kind']}, the case is about {want}: {fam}"
        closed = (fam["kle"]["k_closed"], fam["kle"]["rw_closed"], fam["laplace"]["k_closed"])
        assert closed == (case.closed, case.closed, case.laplace_closed), f"{case.name}: closed forms {closed} (K, Rw, Laplace): {fam}"
        if case.geometry:
            g = fam["geometry"]
            assert (g["affine"], g["diag"]) == case.geometry, f"{case.name}: the geometry pre-pass found {g}, the case is about {case.geometry}"
        _BASE[key] = (got, fam)
    return _BASE[key]


_ORACLE = {}


def base_oracle(case, mesh, masked):
    key = (case.name, masked)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_all(case, mesh, masked)
    return _ORACLE[key]


def oracle_all(case, mesh, masked):
    ref = gc.oracle_matrices(mesh, masked, ops_of(case, mesh) + ("Arhs",))
    if masked:
        ref["Krhs_compact"] = ref["Krhs"]
    return ref


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("case", gc.ASSEMBLY_CASES, ids=lambda c: c.name)
def test_assembly(lib, case, tname):
    """translate and stretch with the boundary imposed (Krhs is empty without), scale without a Dirichlet set (unit rows do not scale)"""
    mesh = gc.built("assembly", case.name, case.build)
    pair = gc.TRANSFORMS[tname](mesh)
    masked = pair.kind != "scale"
    base, base_fam = base_run(lib, case, mesh, masked)
    got, fam = device_matrices(lib, case, pair.moved, masked)
    assert fam == base_fam, f"{case.name} {pair.name}: ran {fam}, the base mesh ran {base_fam}"
    tag = f"{case.name} {pair.name} kappa {gc.kappa(pair.moved):.3g}"
    kinds = "/".join(f"{g}:{r['kind']}" for g, r in fam.items() if g != "geometry") + f" diag:{fam['geometry']['diag']}"
    if pair.kind == "translate":
        e_o, ref = gc.oracle_sensitivity(lambda m: oracle_all(case, m, masked), pair)
        for op in ref:
            e_d, bound = gc.err_of(got[op], ref[op]), gc.translate_bound(e_o[op])
            report(tag, op, e_d, e_o[op], bound, kinds)
            assert e_d <= bound, f"{op}: e_D {e_d:.2e} > max(FP_TOL, 16 e_O = {16 * e_o[op]:.2e}); families {kinds}"
    elif pair.kind == "scale":
        ref = base_oracle(case, mesh, masked)
        again, _ = device_matrices(lib, case, mesh, masked)              # a second run of the base: what the order of the adds alone moves
        for op in ref:
            f = pair.s ** gc.scale_power(op if op != "Arhs" else "laplace", mesh.dim)
            e_dev, e_ref = gc.err_of(got[op], base[op] * f), gc.err_of(got[op], ref[op] * f)
            same, rerun = (got[op] != base[op] * f).nnz == 0, (again[op] != base[op]).nnz == 0
            print(f"GEOM {tag} {op}: against base x factor {e_dev:.2e}, against the oracle {e_ref:.2e}, bit-identical {same}, "
                  f"two runs of the base identical {rerun} {kinds}")
            assert e_dev <= FP_TOL and e_ref <= FP_TOL, f"{op}: {e_dev:.2e} / {e_ref:.2e}; families {kinds}"
    else:
        ref = oracle_all(case, pair.moved, masked)
        for op in ref:
            e_d = gc.err_of(got[op], ref[op])
            print(f"GEOM {tag} {op}: against the oracle {e_d:.2e} {kinds}")
            assert e_d <= FP_TOL, f"{op}: {e_d:.2e}; families {kinds}"


@pytest.mark.parametrize("case", gc.ASSEMBLY_CASES, ids=lambda c: c.name)
def test_assembly_scaled_with_imposed_rows(lib, case):
    """scale(+24) with the boundary imposed: the free rows scale, the imposed rows stay unit rows"""
    mesh = gc.built("assembly", case.name, case.build)
    pair = gc.TRANSFORMS["scale+24"](mesh)
    base, base_fam = base_run(lib, case, mesh, True)
    got, fam = device_matrices(lib, case, pair.moved, True)
    assert fam == base_fam, f"{case.name} {pair.name}: ran {fam}, the base mesh ran {base_fam}"
    ref = base_oracle(case, mesh, True)
    dim = mesh.dim
    for op, nd in (("K", dim), ("Krhs", dim), ("Krhs_compact", dim), ("Rw", dim), ("laplace", 1), ("Arhs", 1), ("mass", 1)):
        f = pair.s ** gc.scale_power({"Krhs_compact": "Krhs", "Arhs": "laplace"}.get(op, op), dim)
        rows = lambda M: gc.free_rows(M.tocsr(), mesh, nd)
        if rows(ref[op]).shape[0] == 0:                               # (a mesh one cell thick has no free node: unit rows only)
            assert len(mesh.boundary) == mesh.n_node and (op == "Rw" or gc.imposed_rows_are_unit(got[op], mesh, nd))
            continue
        e_dev, e_ref = gc.err_of(rows(got[op]), rows(base[op]) * f), gc.err_of(rows(got[op]), rows(ref[op]) * f)
        print(f"GEOM {case.name} {pair.name} masked {op}: free rows against base x factor {e_dev:.2e}, against the oracle {e_ref:.2e}")
        assert e_dev <= FP_TOL and e_ref <= FP_TOL, op
        if op != "Rw":
            assert gc.imposed_rows_are_unit(got[op], mesh, nd), f"{op}: an imposed row is no unit row"


# ---- matrix-free operators ---------------------------------------------------------------------------------------------------------------
def matfree_product(lib, case, mesh, masked, x):
    nd = 1 if case.scalar else mesh.dim
    ctx = open_ctx(lib, mesh, symbolic=False)
    if masked:
        ctx.bc_set(nd, node_mask(mesh, nd))
    ctx.csr_symbolic()
    op = getattr(lib, case.op)
    ctx.matfree_set(op, *ALPHA)                                        # a mesh the operator does not accept is refused here
    vx, vy = set_vec(ctx, x.reshape(mesh.n_node, nd)), ctx.vec_create(nd)
    ctx.matfree_apply(vx, vy, op)
    y = ctx.vec_get(vy, nd)
    form = ctx.ho3_geometry()["matfree_diag"]
    ctx.close()
    assert form == case.diag, f"{case.name}: the operator took form {form} (1 diagonal J^-1, 0 full, -1 no second-order lattice), the case is about {case.diag}"
    return y


_MATFREE_REF = {}


def matfree_reference(case, mesh, masked, x):
    """{"y": R x}, R the oracle's matrix; kept per corner geometry (the oracle reads nothing else), so a dyadic box, whose corners
    do not round under translation, is integrated once"""
    op = "laplace" if case.scalar else "K"
    key = (case.name, masked, mesh.corners().tobytes())
    if key not in _MATFREE_REF:
        if len(_MATFREE_REF) > 16:
            _MATFREE_REF.clear()
        _MATFREE_REF[key] = gc.oracle_matrices(mesh, masked, (op,))[op]
    return {"y": _MATFREE_REF[key] @ x}


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("case", gc.MATFREE_CASES, ids=lambda c: c.name)
def test_matfree(lib, case, tname):
    mesh = gc.built("matfree", case.name, case.build)
    pair = gc.TRANSFORMS[tname](mesh)
    nd = 1 if case.scalar else mesh.dim
    masked = pair.kind != "scale"
    x = np.random.default_rng(2).standard_normal(mesh.n_node * nd)
    y = matfree_product(lib, case, pair.moved, masked, x)
    tag = f"{case.name} {pair.name} kappa {gc.kappa(pair.moved):.3g}"
    if pair.kind == "translate":
        e_o, ref = gc.oracle_sensitivity(lambda m: matfree_reference(case, m, masked, x), pair)
        e_d, bound = rel_err(y, ref["y"]), gc.translate_bound(e_o["y"])
        report(tag, case.op, e_d, e_o["y"], bound)
        assert e_d <= bound, f"e_D {e_d:.2e} > max(FP_TOL, 16 e_O = {16 * e_o['y']:.2e})"
    elif pair.kind == "scale":
        f = pair.s ** gc.scale_power("laplace" if case.scalar else "K", mesh.dim)
        y0, y1 = matfree_product(lib, case, mesh, masked, x), matfree_product(lib, case, mesh, masked, x)
        e_dev, e_ref = rel_err(y, y0 * f), rel_err(y, matfree_reference(case, mesh, masked, x)["y"] * f)
        print(f"GEOM {tag} {case.op}: against base x factor {e_dev:.2e}, against the oracle {e_ref:.2e}, bit-identical "
              f"{np.array_equal(y, y0 * f)}, two runs of the base identical {np.array_equal(y0, y1)}")
        assert e_dev <= FP_TOL and e_ref <= FP_TOL
    else:
        e_d = rel_err(y, matfree_reference(case, pair.moved, masked, x)["y"])
        print(f"GEOM {tag} {case.op}: against the oracle {e_d:.2e}")
        assert e_d <= FP_TOL


@pytest.mark.parametrize("case", gc.MATFREE_CASES, ids=lambda c: c.name)
def test_matfree_scaled_with_imposed_rows(lib, case):
    mesh = gc.built("matfree", case.name, case.build)
    pair = gc.TRANSFORMS["scale+24"](mesh)
    nd = 1 if case.scalar else mesh.dim
    x = np.random.default_rng(2).standard_normal(mesh.n_node * nd)
    y, y0 = matfree_product(lib, case, pair.moved, True, x), matfree_product(lib, case, mesh, True, x)
    ref = matfree_reference(case, mesh, True, x)["y"]
    free = np.ones(mesh.n_node, bool)
    free[mesh.boundary] = False
    free = np.repeat(free, nd)
    f = pair.s ** gc.scale_power("laplace" if case.scalar else "K", mesh.dim)
    e_dev, e_ref = rel_err(y[free], y0[free] * f), rel_err(y[free], ref[free] * f)
    print(f"GEOM {case.name} {pair.name} masked {case.op}: free rows against base x factor {e_dev:.2e}, against the oracle {e_ref:.2e}")
    assert e_dev <= FP_TOL and e_ref <= FP_TOL
    assert np.array_equal(y[~free], x[~free]) and np.array_equal(y0[~free], x[~free])       # unit rows


# ---- probes ------------------------------------------------------------------------------------------------------------------------------
def smooth_field(mesh):
    """two smooth components at the nodes of the case's own mesh: the same nodal values on every transformed copy"""
    x = mesh.xyz
    return np.column_stack([np.sin(2.0 * x[:, 0]) + np.cos(3.0 * x[:, -1]), np.prod(1.0 + 0.5 * x, axis=1)])


def probe_run(lib, mesh, pts, u):
    ctx = open_ctx(lib, mesh)
    pid = ctx.probe_create(pts)
    info, (cell, xi) = ctx.probe_info(pid), ctx.probe_get(pid)
    s = ctx.probe_sample(pid, set_vec(ctx, u))
    ctx.close()
    return info, cell, xi, s


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("name", sorted(gc.PROBE_CASES))
def test_probes(lib, name, tname):
    build, path = gc.PROBE_CASES[name]
    mesh = gc.built("probe", name, build)
    P = gc.interior_points(mesh)
    inside = P["inside"]
    pair = gc.TRANSFORMS[tname](mesh)
    pb, py = pair.points(P["pts"])
    u = smooth_field(mesh)
    info, cell, xi, s = probe_run(lib, pair.moved, py, u)
    lost = np.count_nonzero(cell[inside] < 0)
    print(f"GEOM {name} {pair.name} kappa {gc.kappa(pair.moved):.3g}: path {info['path']}, {info['found']} / {info['n']} found, "
          f"{lost} of {inside.sum()} inside points lost, Newton steps <= {info['max_newton']}")
    assert info["path"] == path, f"located by path {info['path']}, the case is about path {path}"
    assert lost == 0, f"{lost} of {inside.sum()} points inside the mesh were not found (path {info['path']})"
    assert (cell[~inside] == -1).all() and np.array_equal(cell[inside], P["cell"])
    # xi against the construction: exact under scaling and stretching; a translation rounds the point and the corners by eps |y| / 2
    # each, which J^-1 (at most 2 / h_min per component, doubled for the bent cells) turns into 8 eps kappa
    xi_bar = 64.0 * gc.EPS + (8.0 * gc.EPS * gc.kappa(pair.moved) if pair.kind == "translate" else 0.0)
    e_built = np.abs(xi[inside] - P["xi"]).max()
    print(f"GEOM {name} {pair.name}: |xi - xi of the construction| {e_built:.2e} (bar {xi_bar:.2e})")
    assert e_built <= xi_bar
    model = pm.locate(pair.moved, py)
    if pair.kind == "stretch":                                        # the model on the same mesh, at the bars of tests/test_gpu_probe.py
        assert np.array_equal(cell, model["cell"])
        res_dev = np.nanmax(pm.residual(pair.moved, py, cell.astype(np.int64), xi))
        res_mod = np.nanmax(pm.residual(pair.moved, py, model["cell"], model["xi"]))
        assert res_dev <= max(8.0 * res_mod, 64.0 * gc.EPS * np.abs(pm.corners(pair.moved)).max())
        ref, bound = pm.sample(pair.moved, cell.astype(np.int64), xi, u, with_bound=True)
        const = mesh.ngl ** mesh.dim + 2 * mesh.dim * mesh.ngl + 8
        assert (np.abs(s - ref)[inside] <= const * gc.EPS * bound[inside]).all()
        return
    info0, cell0, xi0, s0 = probe_run(lib, pair.base, pb, u)
    assert info0["path"] == info["path"] and info0["found"] == info["found"] and np.array_equal(cell0, cell)
    e_model = np.nanmax(np.abs(model["xi"] - pm.locate(pair.base, pb)["xi"])[inside])
    e_xi = np.abs(xi - xi0)[inside].max()
    grad = mesh.dim * (mesh.ngl - 1) ** 2 * np.abs(pm.phi(mesh.ngl, mesh.dim, xi0[inside])).sum(axis=1).max() * np.abs(u).max()
    e_s = np.abs(s - s0)[inside].max()
    print(f"GEOM {name} {pair.name}: |xi - xi_base| {e_xi:.2e} (model {e_model:.2e}), |sample - base| {e_s:.2e}")
    assert e_xi <= gc.MARGIN * e_model and e_s <= gc.MARGIN * e_model * grad
    assert np.isnan(xi[~inside]).all() and np.isnan(s[~inside]).all()


# ---- integrals ---------------------------------------------------------------------------------------------------------------------------
def integrals_run(lib, mesh, u):
    ctx = open_ctx(lib, mesh)
    va = set_vec(ctx, u)
    out = {rule: ctx.integrate(va, None, rule, True) for rule in (im.NODAL, im.GAUSS)}
    ctx.close()
    return out


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("name", sorted(gc.INTEGRAL_CASES))
def test_integrals(lib, name, tname):
    mesh = gc.built("integrals", name, gc.INTEGRAL_CASES[name])
    dim = mesh.dim
    pair = gc.TRANSFORMS[tname](mesh)
    u = np.random.default_rng(9).uniform(-1.0, 1.0, (mesh.n_node, dim))
    dev = integrals_run(lib, pair.moved, u)
    dev0 = integrals_run(lib, mesh, u) if pair.kind == "scale" else None
    f = pair.s ** gc.integral_powers(dim, dim, True)
    for rule in (im.NODAL, im.GAUSS):
        ref, S = im.moments(pair.base, u, rule, True)
        assert len(dev[rule]) == len(ref)
        if pair.kind == "translate":
            far, _ = im.moments(pair.moved, u, rule, True)
            e_o, e_d = (np.abs(far - ref) / S).max(), (np.abs(dev[rule] - ref) / S).max()
            bound = gc.translate_bound(e_o)
            report(f"{name} {pair.name} kappa {gc.kappa(pair.moved):.3g}", f"integrals rule {rule}", e_d, e_o, bound)
            assert e_d <= bound
        elif pair.kind == "scale":
            e_dev, e_ref = (np.abs(dev[rule] - dev0[rule] * f) / (S * f)).max(), (np.abs(dev[rule] - ref * f) / (S * f)).max()
            print(f"GEOM {name} {pair.name} integrals rule {rule}: against base x factor {e_dev:.2e}, against the model {e_ref:.2e}, "
                  f"bit-identical {np.array_equal(dev[rule], dev0[rule] * f)}")
            assert e_dev <= FP_TOL and e_ref <= FP_TOL
        else:
            e_d = (np.abs(dev[rule] - ref) / S).max()
            print(f"GEOM {name} {pair.name} integrals rule {rule}: against the model {e_d:.2e}")
            assert e_d <= FP_TOL


# ---- immersed boundary -------------------------------------------------------------------------------------------------------------------
IBM_GRIDS = {"2d": ([16, 16], 2), "3d": ([4, 4, 4], 3)}            # node spacing 2^-4 / 2^-3 on the unit box


def ibm_run(lib, nelem, ngl, lower, upper, X, dl, u, q, kernel):
    from pynama_amd.domain.dmplex import DMPlexDom
    from pynama_amd.vectors import Vec
    dim = len(nelem)
    dom = DMPlexDom(boxMesh={"nelem": nelem, "lower": list(lower), "upper": list(upper)})
    dom.setFemIndexing(ngl)
    ctx = dom.ctx
    n = (ngl - 1) * np.array(nelem) + 1
    h = (np.asarray(upper) - np.asarray(lower)) / (n - 1)
    ctx.ibm_set(kernel, X, dl, np.asarray(lower, dtype=np.float64), h)       # refuses nodes that are not lower + i h
    vu, vs = Vec(ctx, dim), Vec(ctx, dim)
    vu.setArray(u)
    vs.set(0.0)
    Hu = ctx.ibm_interp(vu.id)
    ctx.ibm_spread(q, vs.id)
    return Hu, vs.getArray().reshape(-1, dim), h, n


@pytest.mark.parametrize("kernel", ["four", "three"])
@pytest.mark.parametrize("tname", ["translate10", "scale-24", "scale+24"])
@pytest.mark.parametrize("grid", sorted(IBM_GRIDS))
def test_ibm(lib, grid, tname, kernel):
    import pynama_amd
    pynama_amd.install_reference_layout()
    nelem, ngl = IBM_GRIDS[grid]
    dim = len(nelem)
    n = (ngl - 1) * np.array(nelem) + 1
    h0 = 1.0 / (n - 1)
    rng = np.random.default_rng(13)
    X0 = h0 * rng.uniform(2.0, n - 4.0, (31, dim))                     # the 4-point support stays inside lines 1 .. n - 2
    dl0 = rng.uniform(0.5, 1.5, 31) * h0.min() ** (dim - 1)
    u, q = rng.standard_normal((int(np.prod(n)), dim)), rng.standard_normal((31, dim))
    kid = {"four": 0, "three": 1}[kernel]
    zero, one = np.zeros(dim), np.ones(dim)
    if tname.startswith("translate"):
        t = gc.shift_of(dim, 10)
        Xy = X0 + t
        Xb = gc._exact_translate(Xy, t)
        Hu, Sq, h, _ = ibm_run(lib, nelem, ngl, t, t + one, Xy, dl0, u, q, kid)
        assert np.array_equal(h, h0)
        Hb, Sb, _ = ibm_model.operators(Xb, dl0, zero, h0, n, kernel)
        Hy, Sy, _ = ibm_model.operators(Xy, dl0, t, h0, n, kernel)
        for what, dev, ref, far in (("interp", Hu, Hb @ u, Hy @ u), ("spread", Sq, Sb @ q, Sy @ q)):
            e_d, e_o = rel_err(dev, ref), rel_err(far, ref)
            bound = max(1e-13, gc.MARGIN * e_o)                        # 1e-13: the bar of tests/test_gpu_ibm.py
            report(f"ibm {grid} {kernel} translate(10)", what, e_d, e_o, bound)
            assert e_d <= bound
    else:
        s = 2.0 ** int(tname[len("scale"):])
        Hu, Sq, h, _ = ibm_run(lib, nelem, ngl, zero, s * one, X0 * s, dl0 * s ** (dim - 1), u, q, kid)
        H0, S0, _, _ = ibm_run(lib, nelem, ngl, zero, one, X0, dl0, u, q, kid)
        assert np.array_equal(h, h0 * s)
        Hb, Sb, _ = ibm_model.operators(X0, dl0, zero, h0, n, kernel)
        for what, dev, dev0, ref, f in (("interp", Hu, H0, Hb @ u, 1.0), ("spread", Sq, S0, Sb @ q, 1.0 / s)):
            e_dev, e_ref = rel_err(dev, dev0 * f), rel_err(dev, ref * f)
            print(f"GEOM ibm {grid} {kernel} {tname} {what}: against base x factor {e_dev:.2e}, against the model {e_ref:.2e}, "
                  f"bit-identical {np.array_equal(dev, dev0 * f)}")
            assert e_dev <= 1e-13 and e_ref <= 1e-13


# ---- pyn_mesh_box ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nelem,ngl", [([5, 4], 3), ([4, 3, 5], 2), ([2, 2, 2], 4)])
@pytest.mark.parametrize("how", ["translated", "scaled_down", "scaled_up"])
def test_generated_box_mesh(lib, nelem, ngl, how):
    """the device-generated coordinates of a box far from the origin (or tiny, or huge) are the host construction's, bit for bit"""
    from pynama_amd.domain.dmplex import DMPlexDom
    from tests.test_gpu_mesh_box import box_ctx, host_ctx
    dim = len(nelem)
    lo, up = np.array([0.25, -1.0, 0.0][:dim]), np.array([1.0, 0.8, 1.7][:dim])
    if how == "translated":
        lo, up = lo + gc.shift_of(dim, 20), up + gc.shift_of(dim, 20)
    else:
        lo, up = lo * 2.0 ** (-24 if how == "scaled_down" else 24), up * 2.0 ** (-24 if how == "scaled_down" else 24)
    dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': list(lo), 'upper': list(up)})
    dom.setFemIndexing(ngl)
    ctx = box_ctx(lib, dom, 0, 1)
    conn, xyz = ctx.mesh_get()
    assert np.array_equal(conn, dom.conn) and np.array_equal(xyz, dom.xyz)
    assert np.array_equal(xyz.min(axis=0), lo)
    ref = host_ctx(lib, dom, 0, 1)
    assert ctx.mesh_topology() == ref.mesh_topology()
    ref.close()
    ctx.close()


# ---- classification ----------------------------------------------------------------------------------------------------------------------
CLASSIFIED = {"q1_3d": ([5, 4, 3], 2), "q1_2d": ([5, 4], 2), "ngl3_2d": ([5, 4], 3), "ngl3_3d": ([3, 2, 3], 3), "ngl4_2d": ([3, 2], 4)}


def classify(lib, mesh):
    ctx = open_ctx(lib, mesh)
    dim = mesh.dim
    K, Rw = ctx.mat_create(dim, dim), ctx.mat_create(dim, 1 if dim == 2 else 3)
    ctx.assemble_kle(*ALPHA, K, -1, Rw, -1)
    out = dict(topology=ctx.mesh_topology(), ho_lattice=ctx.mesh_ho_lattice(), kle=family(lib, ctx))
    A = ctx.mat_create(1, 1)
    ctx.assemble_scalar(lib.FORM_LAPLACE, A, -1)
    out["laplace"] = family(lib, ctx)
    if mesh.ngl == 3:
        ctx.matfree_set(lib.MATFREE_KLE, *ALPHA)
    out["geometry"] = ctx.ho3_geometry()
    ctx.close()
    return out


@pytest.mark.parametrize("tname", gc.ISOTROPIC)
@pytest.mark.parametrize("name", sorted(CLASSIFIED))
def test_classification_of_exact_boxes(lib, name, tname):
    """an exactly rectilinear box (dyadic cells, moved exactly) is the same lattice, takes the same family with the same slots"""
    nelem, ngl = CLASSIFIED[name]
    mesh = gc.built("classified", name, lambda: gc.dyadic_box(nelem, ngl))
    pair = gc.TRANSFORMS[tname](mesh)
    corner = np.unique(mesh.conn[:, :2 ** mesh.dim])
    assert np.array_equal(pair.base.xyz[corner], mesh.xyz[corner])      # the translation did not round a corner
    base, moved = classify(lib, mesh), classify(lib, pair.moved)
    assert base["topology"][0] != "general" or base["ho_lattice"][0] == ngl, base
    if name != "q1_3d" and ngl < 4:                                   # the row-run families: axis-aligned boxes take the diagonal forms
        assert base["geometry"]["affine"] == 1 and base["geometry"]["diag"] == 1, base
        assert base["geometry"]["matfree_diag"] == (1 if ngl == 3 else -1), base
    assert moved == base, f"{name} {pair.name}: classified {moved}, the base mesh {base}"
