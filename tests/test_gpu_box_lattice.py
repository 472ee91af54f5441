"""What pyn_mesh_set / pyn_mesh_box recognise as the reference's box mesh (src/domain/dmplex.py:8-21, 42-61) or a rank's slab of one,
at every element order: mesh_topology() and mesh_ho_lattice() in full against the closed form of the mesh -- (ngl - 1) nelem + 1
nodes per axis, the slow axis counted in local planes (ghost planes included).  Every fast path starts from this answer, so the
cases pin it down per order, per rank of a slab decomposition, for connectivities that must be refused, and under each view's
off switch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GENERAL, NO_HO = ("general", 0, 0, 0), (0, 0, 0, 0)


@pytest.fixture(scope="module")
def lib():
    from pynama_amd import _lib
    return _lib


def make_dom(nelem, ngl, rank=0, size=1):
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom
    dim = len(nelem)
    dom = DMPlexDom(boxMesh={'nelem': nelem, 'lower': [0.25, -1.0, 0.0][:dim], 'upper': [1.0, 0.8, 1.7][:dim]}, comm=Comm(rank, size))
    dom.setFemIndexing(ngl)
    return dom


def make_ctx(lib, dom, how, conn=None, xyz=None):
    ctx = lib.Context(0)
    if dom.comm.size > 1:
        ctx.comm_init(dom.comm.rank, dom.comm.size, None)        # detached: no transport, the mesh is all that is looked at
        ctx.halo_set(*dom._halo_plan())
    if how == "box":
        k0, k1 = dom._layers
        ctx.mesh_box(dom.dim, dom.ngl, dom.nelem[:-1] + [k1 - k0], k0, dom.lattice, dom._loc, dom._local_plane_ids(), dom._axes())
    else:
        ctx.mesh_set(dom.dim, dom.conn if conn is None else conn, dom.xyz if xyz is None else xyz)
    return ctx


def expected(nelem, ngl, local_planes):
    """(mesh_topology(), mesh_ho_lattice()) of a box mesh of nelem cells whose local part holds `local_planes` planes"""
    dim, m = len(nelem), ngl - 1
    nx = m * nelem[0] + 1
    shape = (nx, m * nelem[1] + 1, local_planes) if dim == 3 else (nx, local_planes, 1)
    if ngl >= 4:
        return GENERAL, (ngl,) + shape
    kind = "lattice-ngl3" if ngl == 3 else ("lattice" if dim == 3 else "lattice-q1-2d")
    return (kind,) + shape, NO_HO


def answers(ctx):
    out = ctx.mesh_topology(), ctx.mesh_ho_lattice()
    ctx.close()
    return out


ONE_RANK = [([5, 3], 2), ([5, 3], 3), ([5, 3], 4), ([5, 3], 5), ([4, 3, 2], 2), ([4, 3, 2], 3), ([2, 3, 2], 4), ([2, 3, 2], 5)]


@pytest.mark.parametrize("how", ["set", "box"])
@pytest.mark.parametrize("nelem,ngl", ONE_RANK)
def test_one_rank_unequal_cell_counts(lib, nelem, ngl, how):
    """cell counts differ per axis, so a swapped EX / EY / EL shows in the node counts"""
    dom = make_dom(nelem, ngl)
    assert answers(make_ctx(lib, dom, how)) == expected(nelem, ngl, (ngl - 1) * nelem[-1] + 1)


@pytest.mark.parametrize("how", ["set", "box"])
@pytest.mark.parametrize("nelem,ngl", [([3, 7], 3), ([3, 2, 7], 2), ([2, 7], 4)])
def test_rank_slabs_with_ghost_planes(lib, nelem, ngl, how):
    """every rank of three: the plane count is the local one (owned + ghost planes), the middle rank's owned planes do not come first
    along the slow axis"""
    m, size = ngl - 1, 3
    n_planes = m * nelem[-1] + 1
    bounds = [(r * n_planes) // size for r in range(size + 1)]
    for r in range(size):
        a, b = bounds[r], bounds[r + 1]
        # element layers that touch an owned plane [a, b): their planes are the local ones
        k0, k1 = max(0, -(-(a - m) // m)), min(nelem[-1] - 1, (b - 1) // m) + 1
        local = m * (k1 - k0) + 1
        dom = make_dom(nelem, ngl, r, size)
        planes = dom._local_plane_ids()
        assert len(planes) == local and dom.nOwned == (b - a) * dom.strides[-1]
        if r == 1:
            assert min(planes) < a and max(planes) >= b                  # ghost planes below and above: p_own0 > 0
        assert answers(make_ctx(lib, dom, how)) == expected(nelem, ngl, local), r


def _swap_local_nodes_of_last_element(dom, rng):
    conn = dom.conn.copy()
    conn[-1, [1, 2]] = conn[-1, [2, 1]]
    return conn, dom.xyz


def _swap_two_elements(dom, rng):
    conn = dom.conn.copy()
    conn[[1, -1]] = conn[[-1, 1]]
    return conn, dom.xyz


def _permute_node_ids(dom, rng):
    perm = rng.permutation(dom.nLocal)
    xyz = np.empty_like(dom.xyz)
    xyz[perm] = dom.xyz
    return perm[dom.conn].astype(np.int32), xyz


def _shift_one_plane(dom, rng):
    """the ids of plane 1 move up by one and the first node of plane 2 takes the id that frees: still a numbering of all nodes, but
    plane 1 is no block of ids that starts at a multiple of the plane size"""
    ps = dom.strides[-1]
    new = np.arange(dom.nLocal)
    new[ps:2 * ps] += 1
    new[2 * ps] = ps
    xyz = np.empty_like(dom.xyz)
    xyz[new] = dom.xyz
    return new[dom.conn].astype(np.int32), xyz


@pytest.mark.parametrize("damage", [_swap_local_nodes_of_last_element, _swap_two_elements, _permute_node_ids, _shift_one_plane])
@pytest.mark.parametrize("nelem,ngl", [([4, 3, 2], 2), ([5, 3], 2), ([5, 3], 3), ([4, 3, 2], 3), ([5, 3], 4), ([2, 3, 2], 4)])
def test_other_connectivities_are_refused(lib, nelem, ngl, damage):
    """the exchange inside the last element leaves every entry the host looks at (first cells of element rows and layers) intact: only
    the check of the whole connectivity on the device can refuse it"""
    dom = make_dom(nelem, ngl)
    conn, xyz = damage(dom, np.random.default_rng(7))
    assert conn.shape == dom.conn.shape and not np.array_equal(conn, dom.conn)
    assert np.array_equal(np.unique(conn), np.arange(dom.nLocal))
    assert answers(make_ctx(lib, dom, "set", conn, xyz)) == (GENERAL, NO_HO)


@pytest.mark.parametrize("switch", ["PYNAMA_NO_LATTICE", "PYNAMA_NO_HO3", "PYNAMA_NO_HO_LATTICE"])
@pytest.mark.parametrize("nelem,ngl,own", [([4, 3, 2], 2, "PYNAMA_NO_LATTICE"), ([5, 3], 3, "PYNAMA_NO_HO3"), ([5, 3], 4, "PYNAMA_NO_HO_LATTICE")])
def test_off_switches_reach_their_own_view_only(lib, monkeypatch, nelem, ngl, own, switch):
    """read at pyn_mesh_set: the hexahedron view (3-D first order), the row-run view (ngl <= 3) and the ngl >= 4 view each have one;
    a 3-D first-order mesh stays 'lattice' without its row-run view and turns 'general' without its hexahedron view"""
    dom = make_dom(nelem, ngl)
    monkeypatch.setenv(switch, "1")
    want = (GENERAL, NO_HO) if switch == own else expected(nelem, ngl, (ngl - 1) * nelem[-1] + 1)
    for how in ("set", "box"):
        assert answers(make_ctx(lib, dom, how)) == want, how
