"""numpy restatement of the closed-form fields of pynama_amd/cases/custom_func.py, shared by tests/test_gpu_fields.py and
tests/fields_dist_gpu_worker.py: the same formulas as pyn_field_eval, factor by factor and in the same order, with np.sin / np.cos
on given coordinates and the host-computed params.  `amplitude` is the product of a field's constant factors (for the two
two-term fields: the sum over the terms), the A of the tests' bar."""
import numpy as np

from pynama_amd import _lib

ULP = 2.0 ** -52
BAR = 32 * ULP      # |device - numpy| <= BAR * amplitude: three trigonometric factors of up to 6 + 1 ulp and four roundings


def restate(fid, p, xyz):
    """[n, bs] values of field `fid` at xyz [n, dim] for params p"""
    k = p[0]
    z0 = np.zeros(xyz.shape[0])
    if fid in (_lib.FIELD_TG2D_VEL, _lib.FIELD_TG2D_VORT):
        x, y = k * xyz[:, 0], k * xyz[:, 1]
        sx, cx, sy, cy = np.sin(x), np.cos(x), np.sin(y), np.cos(y)
        if fid == _lib.FIELD_TG2D_VEL:
            return np.stack([cx * sy * p[1], -sx * cy * p[1]], axis=1)
        return np.stack([p[1] * cx * cy * p[2]], axis=1)
    if _lib.FIELD_TG3D_VEL <= fid <= _lib.FIELD_TG3D_DIFF:
        x, y, z = k * xyz[:, 0], k * xyz[:, 1], k * xyz[:, 2]
        sx, cx, sy, cy, sz, cz = np.sin(x), np.cos(x), np.sin(y), np.cos(y), np.sin(z), np.cos(z)
        a = p[1]
        if fid == _lib.FIELD_TG3D_VEL:
            return np.stack([cx * sy * sz * a, sx * cy * sz * a, -2 * sx * sy * cz * a], axis=1)
        if fid == _lib.FIELD_TG3D_VORT:
            return np.stack([-3 * a * sx * cy * cz, 3 * a * cx * sy * cz, z0], axis=1)
        if fid == _lib.FIELD_TG3D_CONV:
            return np.stack([-a * sy * cy * sz * cz, a * sx * cx * sz * cz, z0], axis=1)
        return np.stack([a * sx * cy * cz, -a * cx * sy * cz, z0], axis=1)
    k2 = 2 * k
    y1, x2 = k * xyz[:, 1], k2 * xyz[:, 0]
    if fid == _lib.FIELD_SEN2D_VEL:
        return np.stack([np.sin(y1), np.sin(x2)], axis=1)
    if fid == _lib.FIELD_SEN2D_VORT:
        return np.stack([k2 * np.cos(x2) - k * np.cos(y1)], axis=1)
    if fid == _lib.FIELD_SEN2D_CONV:
        return np.stack([p[1] * np.sin(y1) * np.sin(x2)], axis=1)
    assert fid == _lib.FIELD_SEN2D_DIFF
    return np.stack([p[1] * (p[2] * np.cos(y1) - p[3] * np.cos(x2))], axis=1)


def amplitude(fid, p):
    """largest product of constant factors among the field's components"""
    return {
        _lib.FIELD_TG2D_VEL: lambda: abs(p[1]),
        _lib.FIELD_TG2D_VORT: lambda: abs(p[1] * p[2]),
        _lib.FIELD_TG3D_VEL: lambda: 2 * abs(p[1]),
        _lib.FIELD_TG3D_VORT: lambda: 3 * abs(p[1]),
        _lib.FIELD_TG3D_CONV: lambda: abs(p[1]),
        _lib.FIELD_TG3D_DIFF: lambda: abs(p[1]),
        _lib.FIELD_SEN2D_VEL: lambda: 1.0,
        _lib.FIELD_SEN2D_VORT: lambda: 3 * abs(p[0]),
        _lib.FIELD_SEN2D_CONV: lambda: abs(p[1]),
        _lib.FIELD_SEN2D_DIFF: lambda: abs(p[1]) * (abs(p[2]) + abs(p[3])),
    }[fid]()
