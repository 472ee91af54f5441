"""Analytic-field objects of pynama_amd/cases/fields.py on the host: the same values as the static methods of custom_func.py,
params equal to their Python sub-expressions, ids and block sizes consistent with the library's table, and the node-set
bookkeeping of DMPlexDom that needs no device."""
from math import exp, pi

import numpy as np
import pytest

from pynama_amd import _lib
from pynama_amd.cases import fields
from pynama_amd.cases.custom_func import CustomFuncCase as C

NU_T = [(0.01, 0.0), (0.02, 0.37), (1.3, 2.5)]
STATIC = {"taylorGreenVel_2D": C.taylorGreenVel_2D, "taylorGreenVort_2D": C.taylorGreenVort_2D,
          "taylorGreenVel_3D": C.taylorGreenVel_3D, "taylorGreenVort_3D": C.taylorGreenVort_3D,
          "taylorGreen3dConvective": C.taylorGreen3dConvective, "taylorGreen3dDiffusive": C.taylorGreen3dDiffusive,
          "senoidalVel_2D": C.senoidalVel_2D, "senoidalVort_2D": C.senoidalVort_2D,
          "senoidalConvective": C.senoidalConvective, "senoidalDiffusive": C.senoidalDiffusive}


@pytest.mark.parametrize("field", fields.FIELDS, ids=lambda f: f.name)
def test_field_objects_equal_the_static_methods(field):
    coords = np.random.default_rng(20).uniform(-1.0, 2.0, size=(20, field.dim))
    static = STATIC[field.name]
    for nu, t in NU_T:
        bound = field.bind(nu, t)
        for c in coords:
            want = static(c, nu, t=t)
            assert len(want) == field.bs
            assert field(c, nu, t=t) == want            # exactly: lists of floats
            assert field(c, nu, t) == want
            assert bound(c) == want


def test_params_are_the_python_subexpressions():
    assert 4 * pi == 2 * (2 * pi)                       # the device forms 4 pi as 2 k: exact
    for nu, t in NU_T:
        e2 = exp(-4 * (pi ** 2) * nu * t * (1.0 / 1 ** 2 + 1.0 / 1 ** 2))
        e3 = exp(-12 * (pi ** 2) * nu * t)
        want = {
            "taylorGreenVel_2D": [2 * pi, e2],
            "taylorGreenVort_2D": [2 * pi, -2 * pi * (1.0 / 1 + 1.0 / 1), e2],
            "taylorGreenVel_3D": [2 * pi, e3],
            "taylorGreenVort_3D": [2 * pi, 2 * pi * e3],
            "taylorGreen3dConvective": [2 * pi, 6 * (2 * pi * e3) ** 2],
            "taylorGreen3dDiffusive": [2 * pi, 9 * nu * e3 * (2 * pi) ** 3],
            "senoidalVel_2D": [2 * pi],
            "senoidalVort_2D": [2 * pi],
            "senoidalConvective": [2 * pi, (2 * pi) ** 2 - (4 * pi) ** 2],
            "senoidalDiffusive": [2 * pi, nu, (2 * pi) ** 3, (4 * pi) ** 3],
        }
        for f in fields.FIELDS:
            assert f.params(nu, t) == want[f.name], f.name
            dev = f.bind(nu, t).deviceField
            assert (dev.id, dev.bs, dev.params) == (f.id, f.bs, want[f.name])


def test_ids_and_block_sizes_match_the_library():
    assert sorted(f.id for f in fields.FIELDS) == list(range(_lib.FIELD_COUNT))
    by_name = {"taylorGreenVel_2D": _lib.FIELD_TG2D_VEL, "taylorGreenVort_2D": _lib.FIELD_TG2D_VORT,
               "taylorGreenVel_3D": _lib.FIELD_TG3D_VEL, "taylorGreenVort_3D": _lib.FIELD_TG3D_VORT,
               "taylorGreen3dConvective": _lib.FIELD_TG3D_CONV, "taylorGreen3dDiffusive": _lib.FIELD_TG3D_DIFF,
               "senoidalVel_2D": _lib.FIELD_SEN2D_VEL, "senoidalVort_2D": _lib.FIELD_SEN2D_VORT,
               "senoidalConvective": _lib.FIELD_SEN2D_CONV, "senoidalDiffusive": _lib.FIELD_SEN2D_DIFF}
    for f in fields.FIELDS:
        assert f.id == by_name[f.name]
        dim, bs, nparams = _lib.field_info(f.id)           # the library's own table
        assert (f.dim, f.bs) == (dim, bs), f.name
        assert len(f.params(0.01, 0.2)) == nparams <= _lib.FIELD_MAX_PARAMS, f.name
        assert bs == (f.dim if "Vel" in f.name else (1 if f.dim == 2 else 3))
    for bad in (-1, _lib.FIELD_COUNT):
        with pytest.raises(_lib.PynamaHipError):
            _lib.field_info(bad)


def test_header_constants_match_the_binding():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pynama_hip.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"PYN_(FIELD_[A-Z0-9_]+) = (\d+)", text)}
    assert len(got) == _lib.FIELD_COUNT + 1
    for name, value in got.items():
        assert getattr(_lib, name) == value, name
    assert int(re.search(r"#define PYN_FIELD_MAX_PARAMS (\d+)", text).group(1)) == _lib.FIELD_MAX_PARAMS


def test_node_set_bookkeeping():
    """sorted owned local ids, duplicates dropped, every owned node -> the set -1; the apply helpers accept the object"""
    from pynama_amd.common.comm import Comm
    from pynama_amd.domain.dmplex import DMPlexDom, NodeSet
    dom = DMPlexDom(boxMesh={"nelem": [2, 2, 4], "lower": [0.0] * 3, "upper": [1.0] * 3}, comm=Comm(1, 2))
    dom.setFemIndexing(3)
    assert 0 < dom.nOwned < dom.nNodesGlobal and dom.rStart > 0
    bc = dom.getNodesFromLabel("External Boundary")
    ns = dom.nodeSet(bc)
    assert isinstance(ns, NodeSet) and dom.nodeSet(ns) is ns and not ns.everything
    own = np.array(sorted(n for n in bc if dom.rStart <= n < dom.rEnd))
    assert np.array_equal(ns.globalNodes, own) and np.array_equal(ns.localNodes, own - dom.rStart)
    assert np.all(np.diff(ns.localNodes) > 0) and len(ns) == own.size
    gn, ln = dom._owned_local(ns)
    assert gn is ns.globalNodes and ln is ns.localNodes
    allset = dom.nodeSet(dom.getAllNodes())
    assert allset.everything and allset.id == -1 and len(allset) == dom.nOwned     # no device needed for -1
    dup = dom.nodeSet([dom.rStart + 3, dom.rStart + 1, dom.rStart + 3, 0])
    assert dup.localNodes.tolist() == [1, 3]
    assert len(dom.nodeSet([])) == 0
