"""The error type and the ctypes idioms of the Python surface, each written once: the status check, out-parameter reads, arrays in
and out with their typed pointers, and the base of the read-only result records."""
import ctypes as C

import numpy as np

from . import _lib


class TgnhError(RuntimeError):
    """Stands for OpenMMException; .status is the C-ABI status code."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def _check(rc):
    if rc != _lib.TGNH_OK:
        raise TgnhError(rc, _lib.load().tgnh_last_error().decode())


def out(fn, types, *args, check=True):
    """fn(*args, &v...) -> v: an out-parameter read.  types: one ctypes type (-> its value) or a tuple of them (-> a tuple);
    check=False ignores the status."""
    vs = [t() for t in (types if isinstance(types, tuple) else (types,))]
    rc = fn(*args, *[C.byref(v) for v in vs])
    if check:
        _check(rc)
    return tuple(v.value for v in vs) if isinstance(types, tuple) else vs[0].value


def _array(x, dtype, ptype, shape, who, what):
    a = np.ascontiguousarray(x, dtype)
    if shape is not None and -1 in shape:
        a = a.reshape(shape)                                 # (a size that is no whole number of rows: numpy's ValueError)
    elif shape is not None and a.shape != shape:
        raise TgnhError(_lib.ERR_ARG, f"{who}: {what}")
    return a, a.ctypes.data_as(ptype)


def f64(x, shape=None, who=None, what=None):
    """-> (x as a contiguous float64 array, its double*).  shape with a -1: reshaped to it; fixed: any other is ERR_ARG, "who: what"."""
    return _array(x, np.float64, _lib.c_f64p, shape, who, what)


def i32(x, shape=None, who=None, what=None):
    """f64's twin for int32 / int32_t*"""
    return _array(x, np.int32, _lib.c_i32p, shape, who, what)


class Record:
    """Base of the read-only result records: the constructor sets every field once (_fill), arrays are frozen, .raw is the struct
    as the library filled it in, and any assignment raises AttributeError."""
    __slots__ = ()

    def _fill(self, st, **fields):
        object.__setattr__(self, "raw", bytes(st))
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is read-only")
