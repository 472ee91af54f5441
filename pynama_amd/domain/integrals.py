"""Mesh integrals: the moments of a nodal vector over the domain's mesh in one pass on the device (pyn_integrate): volume, int u_c,
int u_c^2 and, on request, int |grad u_c|^2, int (div u)^2, int (curl u)_k^2, of u = vec or u = vec - minus.  DMPlexDom.integrate,
normL2, seminormH1 and volume are the entry points; `calls` counts the device passes of this process."""
from dataclasses import dataclass

import numpy as np

from pynama_amd import _lib

RULES = {"nodal": _lib.RULE_NODAL, "gauss": _lib.RULE_GAUSS}
calls = 0


@dataclass
class Moments:
    """What one pass returns; an entry that was not computed is None"""
    volume: float
    value: np.ndarray            # [bs] int u_c
    square: np.ndarray           # [bs] int u_c^2
    grad2: np.ndarray = None     # [bs] int |grad u_c|^2 (grad=True)
    div2: float = None           # int (div u)^2 (grad=True and bs == dim)
    curl2: np.ndarray = None     # [dim_w] int (curl u)_k^2 (grad=True and bs == dim)

    @classmethod
    def from_flat(cls, flat, dim, bs, grad):
        flat = np.asarray(flat, dtype=np.float64)
        if flat.size != _lib.integrate_len(dim, bs, grad):
            raise ValueError(f"{flat.size} entries are not the moments of a block size {bs} vector in {dim}-D (grad={bool(grad)})")
        m = cls(float(flat[0]), flat[1:1 + bs].copy(), flat[1 + bs:1 + 2 * bs].copy())
        if grad:
            m.grad2 = flat[1 + 2 * bs:1 + 3 * bs].copy()
            if bs == dim:
                m.div2 = float(flat[1 + 3 * bs])
                m.curl2 = flat[2 + 3 * bs:].copy()
        return m


def rule_code(rule):
    if rule in RULES:
        return RULES[rule]
    if rule in RULES.values():
        return int(rule)
    raise ValueError(f"rule {rule!r}: 'gauss' (Gauss-Legendre, ngl + 1 points per axis) or 'nodal' (the lumped nodal weights)")


def integrate(dom, vec, minus=None, rule="gauss", grad=False):
    """Moments of vec (- minus) over the mesh of `dom`"""
    global calls
    if minus is not None and minus.bs != vec.bs:
        raise ValueError(f"integrate: minus has block size {minus.bs}, vec has {vec.bs}")
    flat = dom.ctx.integrate(vec.id, None if minus is None else minus.id, rule_code(rule), grad)
    calls += 1
    return Moments.from_flat(flat, dom.dim, vec.bs, grad)
