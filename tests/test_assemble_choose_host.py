"""The rule that picks the kernel family of a numeric assembly (asm_choose, exported as pyn_assemble_choose): a table of
(request, facts, knobs) -> (kind, shape, flags) that walks every branch of the cascade row-run -> lattice / march -> KLE lattice ->
patch plan -> P1 -> generic, and every switch of the library's knob table once set and once not.  Host only: no GPU.  The expected
values were read off the dispatch the chooser replaced (it could not report them); the GPU tests assert the same families from
Context.assemble_last()."""
import pytest

from pynama_amd import _lib
from pynama_amd._lib import (AK_GENERIC, AK_KLE_LATTICE, AK_LATTICE, AK_MARCH, AK_P1, AK_PATCH, AK_ROWRUN, FORM_KLE, FORM_LAPLACE,
                             FORM_MASS_FULL, FORM_MASS_NODAL, FORM_OPERATOR, Q_FULL, Q_NODAL)

STD = dict(q1_gauss_standard=1, q1_red_standard=1, aff_standard=1, aff_rw_standard=1)
# 3-D Q1 box lattice of parallelepipeds with the standard tables; the row-run view is valid on it too (it serves the operators there)
HEX = dict(dim=3, nn=8, nc=8, ngl=2, ngp0=8, ngp1=1, ngp2=8, lat_valid=1, lat_std_ok=1, mesh_affine=1, ho3_valid=1, ho3_affine=1,
           ho3_tabs_nn=8, ho3_tabs_ok0=1, ho3_tabs_ok1=1, ho3_tabs_ok2=1, **STD)
JIT = dict(HEX, mesh_affine=0, ho3_affine=0)                       # the same lattice with jittered nodes
PERM = dict(HEX, lat_valid=0, lat_std_ok=-1, ho3_valid=0, ho3_affine=-1)   # Q1 hexahedra without structured numbering
TET = dict(dim=3, nn=4, nc=4, ngl=2, ngp0=4, ngp1=1, ngp2=4, const_grad=1, mesh_affine=-1, lat_std_ok=-1, ho3_affine=-1)


def ho3(dim, ngl, **kw):
    """second-order (or 2-D first-order) box lattice of parallelograms / parallelepipeds with every table the row-run view wants"""
    nn = ngl ** dim
    return dict(dict(dim=dim, nn=nn, nc=2 ** dim, ngl=ngl, ngp0=ngl ** dim, ngp1=(ngl - 1) ** dim, ngp2=nn, ho3_valid=1, ho3_affine=1,
                     ho3_tabs_nn=nn, ho3_tabs_ok0=1, ho3_tabs_ok1=1, ho3_tabs_ok2=1, mesh_affine=-1, lat_std_ok=-1), **kw)


LAP = dict(form=FORM_LAPLACE, K=1, Krhs=1)
KLE = dict(form=FORM_KLE, K=1, Krhs=1, Rw=1)
OP = dict(form=FORM_OPERATOR, K=1, op_rule=Q_NODAL, op_nterms=9)


def choose(request, facts, **knobs):
    return _lib.assemble_choose(request, facts, knobs)


def check(request, facts, knobs, kind, **want):
    got = choose(request, facts, **knobs)
    assert got["kind"] == kind, (_lib.ASSEMBLY_KINDS[got["kind"]], got)
    for key, val in want.items():
        assert got[key] == val, (key, got)
    return got


def test_layout_names_every_knob_of_the_table():
    layout = _lib.assemble_choose_layout()
    assert layout["request"] == ("form", "variant", "K", "Krhs", "Rw", "Rd", "krhs_compact", "op_rule", "op_nterms")
    assert len(layout["knobs"]) == 30 and len(set(layout["knobs"])) == 30
    assert {"lattice_tile", "march_tile", "kle_lattice_tile", "ho3_run", "ho3_require", "no_dinv"} <= set(layout["knobs"])
    with pytest.raises(_lib.PynamaHipError):
        _lib.assemble_choose(LAP, HEX, {"no_such_knob": 1})


@pytest.mark.parametrize("request_", [LAP, KLE, dict(form=FORM_MASS_NODAL, K=1), dict(form=FORM_MASS_FULL, K=1)])
@pytest.mark.parametrize("facts", [HEX, JIT, PERM, ho3(2, 3), ho3(3, 3)])
def test_variant_0_is_the_generic_kernel(request_, facts):
    got = check(dict(request_, variant=0), facts, {}, AK_GENERIC, krhs_completed=0, dinv=0, rowrun_candidate=0)
    assert got["generic"] == (1 if facts["nn"] <= 8 else 2)


def test_variant_0_on_linear_simplices_is_the_p1_kernel():
    # the scatter-add fall-through has always preferred the constant-gradient kernel, whatever the variant
    check(dict(LAP, variant=0), TET, {}, AK_P1)
    check(dict(LAP, variant=0), TET, dict(no_p1=1), AK_GENERIC, generic=1)


# ---- row-run view ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,ngl,R", [(2, 3, 32), (3, 3, 4), (2, 2, 32)])
def test_rowrun_orders(dim, ngl, R):
    for rq, kc, rc in ((LAP, 1, 0), (KLE, 1, 1), (dict(form=FORM_KLE, Rw=1), 0, 1), (dict(form=FORM_KLE, K=1), 1, 0)):
        check(rq, ho3(dim, ngl), {}, AK_ROWRUN, shape=R, k_closed=kc, rw_closed=rc, krhs_completed=0, dinv=0, rowrun_candidate=1)


def test_rowrun_not_for_first_order_3d():
    # 3-D first-order cells have kernels of their own; the view still serves the operators there
    check(LAP, HEX, {}, AK_LATTICE, rowrun_candidate=1)
    check(KLE, HEX, {}, AK_KLE_LATTICE, rowrun_candidate=1)
    check(OP, HEX, {}, AK_ROWRUN, shape=8)


@pytest.mark.parametrize("knob,runs3d,runs2d", [(0, 4, 32), (2, 2, 32), (8, 8, 32), (16, 4, 16), (64, 4, 64), (5, 4, 32)])
def test_rowrun_run_lengths(knob, runs3d, runs2d):
    kn = dict(ho3_run=knob) if knob else {}
    check(KLE, ho3(3, 3), kn, AK_ROWRUN, shape=runs3d)
    check(KLE, ho3(2, 3), kn, AK_ROWRUN, shape=runs2d)
    check(KLE, ho3(2, 2), kn, AK_ROWRUN, shape=32)      # first order: one length
    check(OP, ho3(3, 3), kn, AK_ROWRUN, shape=2)        # operators: the LDS fixes it
    check(OP, ho3(2, 3), kn, AK_ROWRUN, shape=16)


@pytest.mark.parametrize("decline", [dict(ho3_tabs_ok0=0), dict(ho3_tabs_nn=8), dict(ho3_affine=0), dict(ho3_valid=0)])
def test_rowrun_declines_to_generic(decline):
    f = dict(ho3(3, 3), **decline)
    check(LAP, f, {}, AK_GENERIC, generic=2, rowrun_candidate=f["ho3_valid"])
    check(KLE, f, {}, AK_GENERIC, generic=2)


def test_rowrun_declines_each_on_its_own():
    f = ho3(3, 3)
    check(KLE, dict(f, ho3_tabs_ok1=0), {}, AK_GENERIC)             # KLE needs the reduced-rule records ...
    check(LAP, dict(f, ho3_tabs_ok1=0), {}, AK_ROWRUN)              # ... the Laplacian does not
    check(dict(KLE, Rd=1), f, {}, AK_GENERIC, rowrun_candidate=0)   # Rd has the generic kernel only
    check(dict(form=FORM_KLE, Krhs=1, Rw=1), f, {}, AK_GENERIC, rowrun_candidate=0)   # Krhs without K
    check(dict(form=FORM_LAPLACE, Krhs=1), f, {}, AK_GENERIC, rowrun_candidate=0)
    check(dict(form=FORM_MASS_FULL, K=1), f, {}, AK_GENERIC, rowrun_candidate=0)
    check(KLE, f, dict(no_ho3_lattice=1), AK_GENERIC, rowrun_candidate=1)
    check(KLE, f, {}, AK_ROWRUN)
    # a compact Krhs is addressed by the row-run kernels themselves
    check(dict(KLE, krhs_compact=1), f, {}, AK_ROWRUN, krhs_completed=0)
    check(dict(LAP, krhs_compact=1), f, {}, AK_ROWRUN, krhs_completed=0)


def test_rowrun_knobs_that_do_not_move_the_choice():
    for kn in (dict(ho3_no_diag=1), dict(ho3_no_pstd=1), dict(ho3_ablate=3), dict(ho3_wgs_per_cu=2), dict(ho3_grid=7), dict(ho3_require=1)):
        check(KLE, ho3(2, 3), kn, AK_ROWRUN, shape=32)
    # PYNAMA_HO3_REQUIRE errors in the actor: the chooser says for which requests
    assert choose(KLE, dict(ho3(3, 3), ho3_affine=0), ho3_require=1)["rowrun_candidate"] == 1


# ---- scalar Laplacian on Q1 lattices: tiles vs march -----------------------------------------------------------------------------
def test_lattice_affine_default_tile():
    check(LAP, HEX, {}, AK_LATTICE, shape=0, k_closed=1, dinv=1, krhs_completed=0)
    check(dict(form=FORM_LAPLACE, K=1), HEX, {}, AK_LATTICE, shape=0, k_closed=1, dinv=1)


def test_march_for_general_geometry_and_what_switches_it_off():
    check(LAP, JIT, {}, AK_MARCH, shape=0, k_closed=0, dinv=1)
    check(LAP, JIT, dict(no_march=1), AK_LATTICE, shape=1, k_closed=0)            # quadrature: 7x7x7 tiles
    check(LAP, dict(JIT, q1_gauss_standard=0), {}, AK_LATTICE, shape=1, k_closed=0)
    check(LAP, dict(JIT, lat_std_ok=0), {}, AK_LATTICE, shape=1, k_closed=0)
    check(LAP, JIT, dict(lattice_tile=0), AK_LATTICE, shape=0, k_closed=0)        # a tile request keeps the tile kernel
    check(LAP, HEX, dict(no_affine=1), AK_MARCH, shape=0, k_closed=0)             # parallelepipeds through the quadrature
    check(LAP, dict(HEX, aff_standard=0), {}, AK_MARCH, shape=0, k_closed=0)
    check(LAP, dict(HEX, mesh_affine=-1), {}, AK_MARCH, k_closed=0)               # no affine tables uploaded: never checked


@pytest.mark.parametrize("tile", range(-1, 13))
def test_lattice_tile_ids(tile):
    want = tile if 1 <= tile <= 9 else 0
    kn = dict(lattice_tile=tile) if tile >= 0 else {}
    check(LAP, HEX, kn, AK_LATTICE, shape=want, k_closed=1)
    if tile >= 0:
        check(LAP, JIT, kn, AK_LATTICE, shape=want, k_closed=0)


@pytest.mark.parametrize("tile", range(-1, 18))
def test_march_tile_ids(tile):
    want = tile if 1 <= tile <= 14 and tile != 4 else 0     # the table numbers 1, 2, 3, 5 .. 14
    check(LAP, JIT, dict(march_tile=tile) if tile >= 0 else {}, AK_MARCH, shape=want)
    check(LAP, HEX, dict(march_tile=tile) if tile >= 0 else {}, AK_LATTICE, shape=0)


def test_lattice_declines():
    check(LAP, dict(HEX, ngp0=27), {}, AK_GENERIC)                                 # not the 2x2x2 rule: no patch kernel either
    check(LAP, dict(HEX, plan0_present=1, plan0_user=1), {}, AK_PATCH, k_closed=1)   # a user plan bypasses the lattice family
    check(LAP, dict(HEX, plan0_present=1), {}, AK_LATTICE)                         # the automatic plan does not
    check(LAP, dict(HEX, plan1_present=1, plan1_user=1), {}, AK_LATTICE)           # the KLE plan is not the scalar plan
    check(dict(form=FORM_MASS_FULL, K=1), HEX, {}, AK_GENERIC, dinv=0)
    check(dict(form=FORM_MASS_NODAL, K=1), HEX, {}, AK_GENERIC, dinv=0)
    check(dict(form=FORM_LAPLACE, Krhs=1), HEX, {}, AK_GENERIC, dinv=0)


def test_dinv_only_laplace_through_lattice_or_march():
    check(LAP, HEX, {}, AK_LATTICE, dinv=1)
    check(LAP, JIT, {}, AK_MARCH, dinv=1)
    check(LAP, HEX, dict(no_dinv=1), AK_LATTICE, dinv=0)
    check(LAP, JIT, dict(no_dinv=1), AK_MARCH, dinv=0)
    check(LAP, PERM, {}, AK_PATCH, dinv=0)
    check(LAP, ho3(3, 3), {}, AK_ROWRUN, dinv=0)
    check(KLE, HEX, {}, AK_KLE_LATTICE, dinv=0)
    check(dict(LAP, variant=0), HEX, {}, AK_GENERIC, dinv=0)


# ---- KLE on Q1 lattices ----------------------------------------------------------------------------------------------------------
def test_kle_lattice_affine_general_neither():
    check(KLE, HEX, {}, AK_KLE_LATTICE, shape=0, k_closed=1, rw_closed=1)
    check(dict(form=FORM_KLE, Rw=1), HEX, {}, AK_KLE_LATTICE, k_closed=0, rw_closed=1)     # Rw alone is a legal request
    check(dict(form=FORM_KLE, K=1), HEX, {}, AK_KLE_LATTICE, k_closed=1, rw_closed=0)
    check(KLE, JIT, {}, AK_KLE_LATTICE, shape=0, k_closed=0, rw_closed=0)
    check(KLE, JIT, dict(kle_lattice_tile=3), AK_KLE_LATTICE, shape=0)                     # general geometry has one shape
    check(KLE, HEX, dict(no_affine=1), AK_KLE_LATTICE, k_closed=0, rw_closed=0)
    check(KLE, dict(HEX, aff_rw_standard=0), {}, AK_KLE_LATTICE, k_closed=0, rw_closed=0)
    # neither: the patch-plan kernels with the table-driven quadrature
    check(KLE, JIT, dict(no_kle_general=1), AK_PATCH, k_closed=0, rw_closed=0)
    check(KLE, dict(JIT, q1_red_standard=0), {}, AK_PATCH)
    check(KLE, dict(JIT, q1_gauss_standard=0), {}, AK_PATCH)
    check(KLE, HEX, dict(no_kle_general=1), AK_KLE_LATTICE, k_closed=1)                    # the affine form does not need it
    check(KLE, HEX, dict(no_kle_lattice=1), AK_PATCH, k_closed=1, rw_closed=1)
    check(KLE, dict(HEX, plan1_present=1, plan1_user=1), {}, AK_PATCH, k_closed=1, rw_closed=1)
    check(KLE, dict(HEX, plan0_present=1, plan0_user=1), {}, AK_KLE_LATTICE)
    check(dict(form=FORM_KLE, Krhs=1, Rw=1), HEX, {}, AK_GENERIC)                          # Krhs without K: generic
    check(dict(KLE, Rd=1), HEX, {}, AK_GENERIC)
    check(KLE, dict(HEX, ngp1=8), {}, AK_GENERIC)


@pytest.mark.parametrize("tile", range(-1, 7))
def test_kle_lattice_tile_ids(tile):
    check(KLE, HEX, dict(kle_lattice_tile=tile) if tile >= 0 else {}, AK_KLE_LATTICE, shape=tile if 1 <= tile <= 4 else 0, k_closed=1)


# ---- patch plans -----------------------------------------------------------------------------------------------------------------
def test_patch_plan_hexahedra():
    for plan in ({}, dict(plan0_present=1, plan1_present=1), dict(plan0_present=1, plan0_user=1, plan1_present=1, plan1_user=1)):
        check(LAP, dict(PERM, **plan), {}, AK_PATCH, shape=0, k_closed=1, rw_closed=0)
        check(KLE, dict(PERM, **plan), {}, AK_PATCH, shape=0, k_closed=1, rw_closed=1)
    check(dict(form=FORM_KLE, K=1), PERM, {}, AK_PATCH, k_closed=1, rw_closed=0)
    check(dict(form=FORM_KLE, Rw=1), PERM, {}, AK_GENERIC)          # the patch kernels want K
    check(KLE, dict(PERM, mesh_affine=0), {}, AK_PATCH, k_closed=0, rw_closed=0)
    check(KLE, dict(PERM, aff_rw_standard=0), {}, AK_PATCH, k_closed=1, rw_closed=0)
    check(KLE, dict(PERM, aff_standard=0), {}, AK_PATCH, k_closed=0, rw_closed=1)
    check(KLE, PERM, dict(no_affine=1), AK_PATCH, k_closed=0, rw_closed=0)
    check(LAP, PERM, dict(no_affine=1), AK_PATCH, k_closed=0)
    check(LAP, PERM, dict(no_lean_plan=1), AK_PATCH, k_closed=0)
    check(LAP, PERM, dict(tiled_ablate=1), AK_PATCH, k_closed=0)
    check(KLE, PERM, dict(no_lean_plan=1, tiled_ablate=1, kle_ablate=1), AK_PATCH, k_closed=1, rw_closed=1)
    # no plan and none to be had (the automatic one did not fit, or is switched off): scatter-add
    check(LAP, dict(PERM, plan0_unfit=1), {}, AK_GENERIC, generic=1)
    check(KLE, dict(PERM, plan1_unfit=1), {}, AK_GENERIC, generic=1)
    check(KLE, dict(PERM, plan0_unfit=1), {}, AK_PATCH)
    check(LAP, dict(PERM, ngp0=27), {}, AK_GENERIC)
    check(LAP, dict(PERM, dim=2, nn=4, nc=4, ngp0=4), {}, AK_GENERIC)


def test_patch_plan_tets_and_the_unfit_loop_back():
    check(LAP, TET, {}, AK_PATCH, k_closed=0)
    check(LAP, dict(TET, plan0_present=1), {}, AK_PATCH)
    check(LAP, dict(TET, plan0_unfit=1), {}, AK_P1)                  # rows longer than 32 entries: what the actor chooses again
    check(LAP, dict(TET, plan0_unfit=1), dict(no_p1=1), AK_GENERIC, generic=1)
    check(LAP, TET, dict(no_p1_tiled=1), AK_P1)
    check(LAP, dict(TET, plan0_present=1, plan0_user=1), dict(no_p1_tiled=1), AK_P1)
    check(LAP, TET, dict(no_p1_tiled=1, no_p1=1), AK_GENERIC)
    check(LAP, dict(TET, const_grad=0), {}, AK_GENERIC)
    check(dict(form=FORM_MASS_FULL, K=1), TET, {}, AK_GENERIC)
    check(dict(form=FORM_LAPLACE, K=1), dict(dim=2, nn=3, nc=3, ngl=2, ngp0=3, const_grad=1), {}, AK_P1)


def test_compact_krhs_completion_flag():
    c = dict(krhs_compact=1)
    check(dict(LAP, **c), HEX, {}, AK_LATTICE, krhs_completed=1)
    check(dict(LAP, **c), JIT, {}, AK_MARCH, krhs_completed=1)
    check(dict(LAP, **c), PERM, {}, AK_PATCH, krhs_completed=1)
    check(dict(KLE, **c), PERM, {}, AK_PATCH, krhs_completed=1)
    check(dict(LAP, **c), TET, {}, AK_PATCH, krhs_completed=1)
    check(dict(KLE, **c), HEX, {}, AK_KLE_LATTICE, krhs_completed=0)     # native
    check(dict(KLE, **c), JIT, {}, AK_KLE_LATTICE, krhs_completed=0)
    check(dict(KLE, **c), ho3(3, 3), {}, AK_ROWRUN, krhs_completed=0)    # native
    check(dict(LAP, **c), dict(TET, plan0_unfit=1), {}, AK_P1, krhs_completed=0)
    check(dict(KLE, **c, variant=0), HEX, {}, AK_GENERIC, krhs_completed=0)
    check(dict(form=FORM_KLE, K=1, krhs_compact=1), PERM, {}, AK_PATCH, krhs_completed=0)   # no Krhs target: nothing to complete
    check(LAP, HEX, {}, AK_LATTICE, krhs_completed=0)


# ---- operators -------------------------------------------------------------------------------------------------------------------
def test_operators():
    for f, R in ((ho3(2, 3), 16), (ho3(3, 3), 2), (ho3(2, 2), 32), (HEX, 8)):
        check(OP, f, {}, AK_ROWRUN, shape=R, k_closed=1, rowrun_candidate=0)
        check(OP, f, dict(no_ho3_operator=1), AK_GENERIC)
        check(OP, f, dict(no_ho3_lattice=1), AK_GENERIC)
        check(dict(OP, op_nterms=32), f, {}, AK_ROWRUN)
        check(dict(OP, op_nterms=33), f, {}, AK_GENERIC)                 # more terms than the kernel arguments carry
        check(dict(OP, op_rule=Q_FULL), f, {}, AK_GENERIC)               # the closed forms are those of the nodal rule
        check(OP, dict(f, ho3_tabs_ok2=0), {}, AK_GENERIC)
        check(OP, dict(f, ho3_tabs_ok0=0), {}, AK_ROWRUN)                # the operators read the nodal records only
        check(OP, dict(f, ho3_affine=0), {}, AK_GENERIC)
        check(dict(OP, variant=0), f, {}, AK_ROWRUN)                     # operators have no variant
    check(OP, PERM, {}, AK_GENERIC, generic=1)
    check(OP, TET, {}, AK_GENERIC, generic=1)


# ---- generic sub-variants and the knobs that steer launches, not the family ------------------------------------------------------
def test_generic_sub_variants():
    def ho(dim, ngl):
        return ho3(dim, ngl, ho3_valid=0)
    g = lambda rq, f, **kn: choose(dict(rq, variant=0), f, **kn)["generic"]
    assert g(KLE, HEX) == 1 and g(LAP, TET, no_p1=1) == 1                          # up to 8 nodes: 64 threads
    assert g(KLE, ho(2, 3)) == 2 and g(KLE, ho(3, 3)) == 2 and g(KLE, ho(2, 6)) == 2   # the point data fits the LDS
    assert g(LAP, ho(3, 4)) == 3 and g(LAP, ho(2, 8)) == 3                # 64 nodes, 193 / 133 doubles per point: global scratch
    for f in (ho(2, 7), ho(3, 4), ho(2, 8)):                              # KLE there: 48 nodes and more, the FP64 matrix cores
        assert g(KLE, f) == 5
        assert g(KLE, f, no_ho_mfma=1) == 4                               # ... else the points staged through LDS
        assert g(KLE, f, no_ho=1) == 3 and g(KLE, f, no_ho=1, no_ho_mfma=1) == 3
    assert g(dict(form=FORM_OPERATOR, K=1, op_rule=Q_NODAL, op_nterms=3), ho(3, 4)) == 3


@pytest.mark.parametrize("knob", ["no_lean", "rhs_full_write", "no_std_lattice", "march_stamps", "march_zlen", "lattice_ablate", "kle_ablate"])
def test_launch_knobs_do_not_move_the_choice(knob):
    for rq, f in ((LAP, HEX), (LAP, JIT), (KLE, HEX), (KLE, JIT), (LAP, PERM), (KLE, PERM), (LAP, TET), (KLE, ho3(3, 3))):
        assert choose(rq, f, **{knob: 1}) == choose(rq, f)
