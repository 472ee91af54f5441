"""The closed-form fields of ``custom_func.py`` as objects the device can evaluate.

An ``AnalyticField`` is callable like the static method it wraps (``field(coord, nu, t=...)``, the same function, so the same
bits) and also knows its ``PYN_FIELD_*`` id, its dimension and block size, and how to compute the field's coordinate-independent
factors -- ``params(nu, t)`` -- with the very Python sub-expressions of ``custom_func.py``.  Those travel by value to
``pyn_field_eval``, which computes the phases, one sincos per axis, and multiplies in the expression's left-to-right order: the
time dependence of the device path is bit-equal to the host's, and the two differ only by the last bits of sin and cos.

``field.bind(nu, t)`` gives the one-argument callable the ``apply*ToVec`` helpers of ``DMPlexDom`` take; with
``-pynama_device_fields`` they hand its ``deviceField`` to the library instead of mapping it over the nodes."""
from math import exp, pi

from pynama_amd import _lib
from pynama_amd.cases.custom_func import CustomFuncCase as _C


def _tg2_decay(nu, t):
    Lx = Ly = 1
    return exp(-4 * (pi ** 2) * nu * t * (1.0 / Lx ** 2 + 1.0 / Ly ** 2))


def _tg2_vel(nu, t):
    return [2 * pi, _tg2_decay(nu, t)]


def _tg2_vort(nu, t):
    Lx = Ly = 1
    return [2 * pi, -2 * pi * (1.0 / Lx + 1.0 / Ly), _tg2_decay(nu, t)]


def _tg3_decay(nu, t):
    return exp(-12 * (pi ** 2) * nu * t)


def _tg3_vel(nu, t):
    return [2 * pi, _tg3_decay(nu, t)]


def _tg3_vort(nu, t):
    e = _tg3_decay(nu, t)
    return [2 * pi, 2 * pi * e]


def _tg3_conv(nu, t):
    e = _tg3_decay(nu, t)
    return [2 * pi, 6 * (2 * pi * e) ** 2]


def _tg3_diff(nu, t):
    e = _tg3_decay(nu, t)
    return [2 * pi, 9 * nu * e * (2 * pi) ** 3]


# the sinusoidal field has no time dependence; its second wave number 4 pi is 2 (2 pi) exactly and is formed on the device
def _sen_k(nu, t):
    return [2 * pi]


def _sen_conv(nu, t):
    return [2 * pi, (2 * pi) ** 2 - (4 * pi) ** 2]


def _sen_diff(nu, t):
    return [2 * pi, nu, (2 * pi) ** 3, (4 * pi) ** 3]


class DeviceField:
    """what pyn_field_eval needs: the field id and the factors for one (nu, t)"""
    __slots__ = ("id", "bs", "params")

    def __init__(self, fid, bs, params):
        self.id, self.bs, self.params = fid, bs, params


class BoundField:
    """field(., nu, t=t): a callable of the coordinates alone; `deviceField` is its device form"""

    def __init__(self, field, nu, t):
        self.field, self.nu, self.t = field, nu, t

    def __call__(self, coord):
        return self.field.function(coord, self.nu, t=self.t)

    @property
    def deviceField(self):
        return DeviceField(self.field.id, self.field.bs, self.field.params(self.nu, self.t))


class AnalyticField:
    def __init__(self, name, fid, dim, bs, function, params):
        self.name, self.id, self.dim, self.bs, self.function, self._params = name, fid, dim, bs, function, params

    def __call__(self, coord, nu, t=None):
        return self.function(coord, nu, t=t)

    def params(self, nu, t):
        """the coordinate-independent factors, in the order include/pynama_hip.h lists them for this field"""
        return [float(v) for v in self._params(nu, t)]

    def bind(self, nu, t):
        return BoundField(self, nu, t)

    def __repr__(self):
        return f"AnalyticField({self.name}, id {self.id}, {self.dim}-D, {self.bs} components)"


taylorGreenVel_2D = AnalyticField("taylorGreenVel_2D", _lib.FIELD_TG2D_VEL, 2, 2, _C.taylorGreenVel_2D, _tg2_vel)
taylorGreenVort_2D = AnalyticField("taylorGreenVort_2D", _lib.FIELD_TG2D_VORT, 2, 1, _C.taylorGreenVort_2D, _tg2_vort)
taylorGreenVel_3D = AnalyticField("taylorGreenVel_3D", _lib.FIELD_TG3D_VEL, 3, 3, _C.taylorGreenVel_3D, _tg3_vel)
taylorGreenVort_3D = AnalyticField("taylorGreenVort_3D", _lib.FIELD_TG3D_VORT, 3, 3, _C.taylorGreenVort_3D, _tg3_vort)
taylorGreen3dConvective = AnalyticField("taylorGreen3dConvective", _lib.FIELD_TG3D_CONV, 3, 3, _C.taylorGreen3dConvective, _tg3_conv)
taylorGreen3dDiffusive = AnalyticField("taylorGreen3dDiffusive", _lib.FIELD_TG3D_DIFF, 3, 3, _C.taylorGreen3dDiffusive, _tg3_diff)
senoidalVel_2D = AnalyticField("senoidalVel_2D", _lib.FIELD_SEN2D_VEL, 2, 2, _C.senoidalVel_2D, _sen_k)
senoidalVort_2D = AnalyticField("senoidalVort_2D", _lib.FIELD_SEN2D_VORT, 2, 1, _C.senoidalVort_2D, _sen_k)
senoidalConvective = AnalyticField("senoidalConvective", _lib.FIELD_SEN2D_CONV, 2, 1, _C.senoidalConvective, _sen_conv)
senoidalDiffusive = AnalyticField("senoidalDiffusive", _lib.FIELD_SEN2D_DIFF, 2, 1, _C.senoidalDiffusive, _sen_diff)

FIELDS = (taylorGreenVel_2D, taylorGreenVort_2D, taylorGreenVel_3D, taylorGreenVort_3D, taylorGreen3dConvective,
          taylorGreen3dDiffusive, senoidalVel_2D, senoidalVort_2D, senoidalConvective, senoidalDiffusive)
