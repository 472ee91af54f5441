"""The numpy model of the point probes (tests/probe_model.py) against itself, without a device: location and sampling on fo.box_mesh
and on the bent, warped, imported and star meshes of tests/ho_general_meshes.py.

Bars.  A linear function and, on affine cells, a tensor polynomial of degree ngl - 1 per axis are reproduced by the interpolant up to
rounding: 64 eps max|f| for the linear function (its nodal sum has at most ngl^dim <= 64 terms here, and the location residual enters
times the gradient), the same bar times ngl^dim for the polynomial, whose terms alternate in sign.  Newton needs at most 8 steps from
xi = 0 -- half the device's cap of 16, so a mesh family that needs more shows up here first."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import ho_general_meshes as gm
from tests import probe_model as pm

EPS = pm.EPS

MESHES = {
    "box2d_ngl3": lambda: fo.box_mesh([4, 3], [0.0, 0.0], gm.UPPER[:2], 3),
    "box2d_ngl5": lambda: fo.box_mesh([4, 3], [0.0, 0.0], gm.UPPER[:2], 5),
    "box3d_ngl4": lambda: fo.box_mesh([2, 3, 2], [0.0] * 3, gm.UPPER, 4),
    "bent2d_ngl5": lambda: gm.bent_lattice(2, [4, 3], 5, seed=3),
    "bent3d_ngl4": lambda: gm.bent_lattice(3, [2, 3, 2], 4, seed=3),
    "warped2d": lambda: gm.warped_lattice(2, [1, 1], 3),
    "warped3d": lambda: gm.warped_lattice(3, [2, 1, 2], 3),
    "imported2d_ngl4": lambda: gm.imported(2, [4, 3], 4),
    "imported3d_ngl3": lambda: gm.imported(3, [2, 3, 2], 3),
    "star3": lambda: gm.star(3, 4),
    "star5": lambda: gm.star(5, 4),
    "star5_layers": lambda: gm.star(5, 3, layers=2),
}
AFFINE = ("box2d_ngl3", "box2d_ngl5", "box3d_ngl4")
_CACHE = {}


def case(name):
    if name not in _CACHE:
        mesh = MESHES[name]()
        extra = pm.bbox_corners(mesh) if name.startswith(("star", "warped")) else None
        P = pm.probe_points(mesh, seed=1, box_boundary=name.startswith("box"), extra_outside=extra, max_nodes=120)
        _CACHE[name] = (mesh, P, pm.locate(mesh, P["pts"]))
    return _CACHE[name]


def test_corner_basis_is_the_reference_order():
    """N_c is 1 at corner c and 0 at the others; the Jacobian of a box cell is diagonal and positive"""
    for dim in (2, 3):
        s = pm.corner_signs(dim)
        N, dN = pm.corner_basis(dim, s)
        assert np.array_equal(N, np.eye(2 ** dim))
        mesh = fo.box_mesh([1] * dim, [0.0] * dim, [2.0] * dim, 2)
        J = np.einsum("mcq,mcd->mdq", pm.corner_basis(dim, np.zeros((1, dim)))[1], pm.corners(mesh)[:1])[0]
        assert np.allclose(J, np.diag(np.diag(J))) and np.all(np.abs(np.diag(J)) == 1.0)
        assert np.linalg.det(J) > 0


def test_phi_is_a_nodal_basis():
    for ngl, dim in ((3, 2), (5, 2), (4, 3)):
        nodes, _ = fo.gauss_lobatto(ngl)
        at = nodes[np.array(fo.local_lattice(ngl, dim))]              # reference position of every local node
        assert np.array_equal(pm.phi(ngl, dim, at), np.eye(ngl ** dim))
        xi = np.random.default_rng(0).uniform(-1, 1, (20, dim))
        assert np.abs(pm.phi(ngl, dim, xi).sum(axis=1) - 1.0).max() <= 64 * EPS


@pytest.mark.parametrize("name", sorted(MESHES))
def test_found_set_and_newton(name):
    mesh, P, L = case(name)
    found = L["cell"] >= 0
    assert found[P["inside"]].all(), "a point built as the image of a cell was not found"
    assert not found[P["outside"]].any(), "a point outside the mesh was found"
    assert np.isnan(L["xi"][~found]).all() and np.abs(L["xi"][found]).max() <= 1.0
    print(f"{name}: {found.sum()} / {len(found)} found, Newton steps <= {L['steps'].max()}, candidates <= {L['ncand'].max()}, "
          f"near the threshold {L['near'].sum()}")
    assert L["steps"].max() <= 8
    assert L["ncand"][found].min() >= 1
    assert L["near"].mean() < 0.02
    res = pm.residual(mesh, P["pts"], L["cell"], L["xi"])
    assert np.nanmax(res) <= 64 * EPS * np.abs(pm.corners(mesh)).max()


@pytest.mark.parametrize("name", [n for n in sorted(MESHES) if n.startswith("box")])
def test_face_points_go_to_the_lower_cell(name):
    mesh, _, _ = case(name)
    Xc = pm.corners(mesh)
    dim = mesh.dim
    for e in range(mesh.n_elem):
        lo = Xc[e].min(axis=0)
        mid = 0.5 * (Xc[e].min(axis=0) + Xc[e].max(axis=0))
        for d in range(dim):
            if lo[d] > 0.0:                                          # an interior face: the lower neighbour wins
                p = mid.copy()
                p[d] = lo[d]
                stride = int(np.prod(mesh.nelem[:d]))
                assert pm.locate(mesh, p[None])["cell"][0] == e - stride


@pytest.mark.parametrize("name", sorted(MESHES))
def test_linear_function_is_reproduced(name):
    mesh, P, L = case(name)
    s = pm.sample(mesh, L["cell"], L["xi"], pm.linear_field(mesh))[:, 0]
    f = pm.linear_field(mesh, P["pts"])
    found = L["cell"] >= 0
    err = np.abs(s[found] - f[found]).max()
    print(f"{name}: linear function to {err:.2e}")
    assert err <= 64 * EPS * np.abs(f[found]).max()
    assert np.isnan(s[~found]).all()


@pytest.mark.parametrize("name", AFFINE)
def test_tensor_polynomial_on_affine_cells(name):
    mesh, P, L = case(name)
    s = pm.sample(mesh, L["cell"], L["xi"], pm.tensor_poly(mesh))[:, 0]
    f = pm.tensor_poly(mesh, P["pts"])
    found = L["cell"] >= 0
    err = np.abs(s[found] - f[found]).max()
    print(f"{name}: polynomial to {err:.2e}")
    assert err <= 64 * EPS * mesh.ngl ** mesh.dim * np.abs(f[found]).max()


def test_summation_order_stays_inside_the_sampling_bound():
    """the bound the device is held to, (nn + 2 dim ngl + 8) eps sum |phi_a| |u_a|, holds between two summation orders of the model"""
    for name in ("box2d_ngl5", "bent3d_ngl4", "imported2d_ngl4"):
        mesh, _, L = case(name)
        u = np.random.default_rng(2).standard_normal((mesh.n_node, mesh.dim))
        a, bound = pm.sample(mesh, L["cell"], L["xi"], u, with_bound=True)
        b = pm.sample(mesh, L["cell"], L["xi"], u, order=np.random.default_rng(3).permutation(mesh.ngl ** mesh.dim))
        found = L["cell"] >= 0
        const = mesh.ngl ** mesh.dim + 2 * mesh.dim * mesh.ngl + 8
        ratio = (np.abs(a - b)[found] / (EPS * bound[found])).max()
        print(f"{name}: two summation orders differ by {ratio:.2f} eps sum|phi||u| (bound {const})")
        assert ratio <= const
