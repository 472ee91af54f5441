"""The case table of the generic assembly kernel's launch forms (generic_pick in pynama_amd/csrc/pyn_assemble.hip): which mesh reaches
which form under which switches.  tests/test_generic_forms_host.py proves every row on the host (the chooser names the form, the
mesh is valid and not affine), tests/test_gpu_generic_forms.py compares what each row computes with the oracle.

Forms: 2 = 256 threads with the point data in LDS, 3 = point data in global scratch, 4 = Gauss points staged through LDS with a 2x2
micro-block of node pairs per lane, 5 = the FP64 matrix cores.  A mesh is (kind, nelem, ngl): kind "W" = ho_general_meshes.
warped_lattice, "I" = ho_general_meshes.imported (random numbering, cell order and cell orientation)."""
import functools

from tests import ho_general_meshes as gm

# the switches that move a stageable KLE assembly from its default form (5 where nn >= 48) to the staged and the per-pair form
KLE_KNOBS = {5: (), 4: ("no_ho_mfma",), 3: ("no_ho",), 2: ()}

# (mesh, forms, targets): plain KLE assemblies, pyn_assemble_kle(variant=0)
ALL4 = ("K", "Krhs", "Rw", "Rd")
KLE_CASES = [
    # nn 49: the clamped second node of an odd micro-block; 625 micro-blocks = three lane rounds, the last partial; 85 points in chunks
    # of 16: a partial last chunk; the first order whose point data leaves the LDS
    (("W", (3, 2), 7), (5, 4, 3), ALL4),
    (("W", (2, 2), 8), (5, 4, 3), ALL4),                       # nn 64, even: no clamp
    (("W", (2, 2), 12), (5, 4), ALL4),                         # the largest 2-D order the shells serve
    (("W", (2, 1), 11), (5, 4), ALL4),                         # nn 121, nn16 128: pad rows of the matrix-core tiles
    (("W", (2, 1, 2), 4), (5, 4, 3), ALL4),                    # nn 64, 91 points
    (("W", (2, 1, 1), 5), (5, 4), ALL4),                       # nn 125 odd, staged chunks of 12 over 189 points
    (("W", (1, 1, 1), 6), (5,), ("K", "Rw", "Rd")),            # matrix-core chunks of 12 with a partial last chunk (341 points)
    (("I", (3, 2), 7), (5, 4), ALL4),                          # find_slot on unsorted neighbour ids, rotated cells
    (("W", (3, 2), 6), (2,), ALL4),                            # form 2 on bent cells
    (("W", (2, 2, 1), 3), (2,), ALL4),
]
# one cell: no atomic has a partner, forms 3 and 4 must agree bit for bit
ONE_CELL = [("W", (1, 1), 7), ("W", (1, 1, 1), 4)]
# more cells than the grid has workgroups (1024): the grid-stride loop reuses scratch and LDS
STRIDE_CASE = ("W", (36, 30), 7)
# two rank slabs: ghost rows in all three scatters
SLAB_CASE = (("W", (2, 4), 7), (5, 4, 3), ("K", "Rw"))

# (mesh, form): never stageable, so these are the default forms
SCALAR_CASES = [(("W", (2, 2), 8), 3), (("W", (2, 1, 2), 4), 3)]
SCALAR_FORMS = ("laplace", "mass_nodal", "mass_full")
OPERATOR_CASES = [(("W", (2, 2), 8), 3), (("W", (2, 1, 2), 4), 3), (("W", (3, 2), 5), 2)]
NOSLIP_CASES = [(("W", (3, 2), 3), 2), (("W", (2, 2), 8), 3), (("W", (2, 1, 2), 4), 3)]


@functools.lru_cache(maxsize=None)
def mesh_of(spec):
    """the mesh of a table row; shared by every test that names it and never written to"""
    kind, nelem, ngl = spec
    build = gm.warped_lattice if kind == "W" else gm.imported
    return build(len(nelem), list(nelem), ngl)


def tag(spec):
    return f"{spec[0]}{len(spec[1])}d_{'x'.join(map(str, spec[1]))}_ngl{spec[2]}"


def case_id(v):
    """pytest id of a mesh among the parameters of a row (the other parameters keep pytest's own ids)"""
    return tag(v) if isinstance(v, tuple) and len(v) == 3 and isinstance(v[1], tuple) and isinstance(v[2], int) else None


def all_meshes():
    """every mesh the tables name, once"""
    specs = [c[0] for c in KLE_CASES] + ONE_CELL + [STRIDE_CASE, SLAB_CASE[0]]
    specs += [c[0] for c in SCALAR_CASES + OPERATOR_CASES + NOSLIP_CASES]
    return list(dict.fromkeys(specs))
