"""Who owns a library handle in Python (``_lib.Handle``, ``_lib.HandleOwner``), with a fake
library that records its calls: no device."""
import ctypes
import gc

import pytest

from pyratslam_amd import _lib


class FakeLib:
    """``rs_x_create(value, &h)`` / ``rs_y_create``, ``rs_x_destroy(h)`` / ``rs_y_destroy``:
    statuses from ``status`` (RS_OK without an entry), every call recorded."""

    def __init__(self, **status):
        self.status = status
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('rs_'):
            raise AttributeError(name)

        def call(*args):
            st = self.status.get(name, _lib.RS_OK)
            if name.endswith('_create') and st == _lib.RS_OK:
                args[-1]._obj.value = args[0]
            self.calls.append((name, args[0].value if name.endswith('_destroy') else args[0]))
            return st
        return call


class Owner(_lib.HandleOwner):
    _handles = ('_h', '_second')

    def __init__(self, lib, second=True):
        self.more = 0
        self._h = _lib.Handle.create(lib, 'rs_x_create', 'rs_x_destroy', 0x1000)
        self._second = _lib.Handle.create(lib, 'rs_y_create', 'rs_y_destroy', 0x2000) if second else None

    def _close_more(self):
        self.more += 1


def test_a_refused_create_raises_the_mapped_exception_and_leaves_nothing_to_destroy():
    for status, exc in ((_lib.RS_ERR_ARG, ValueError), (_lib.RS_ERR_TYPE, TypeError),
                        (_lib.RS_ERR_NOMEM, MemoryError), (_lib.RS_ERR_HIP, _lib.HipLibraryError)):
        lib = FakeLib(rs_x_create=status)
        with pytest.raises(exc):
            Owner(lib)
        gc.collect()                      # (the half-made Owner is finalised: _h was never set)
        assert lib.calls == [('rs_x_create', 0x1000)]
    lib = FakeLib(rs_y_create=_lib.RS_ERR_NOMEM)     # the second create refused: the first is released
    with pytest.raises(MemoryError):
        Owner(lib)
    gc.collect()
    assert lib.calls == [('rs_x_create', 0x1000), ('rs_y_create', 0x2000), ('rs_x_destroy', 0x1000)]


def test_close_destroys_once():
    lib = FakeLib()
    o = Owner(lib, second=False)
    assert isinstance(o._h, ctypes.c_void_p) and o._h.value == 0x1000
    h = o._h
    o.close()
    assert o._h is None and o._second is None and o.more == 1
    assert lib.calls == [('rs_x_create', 0x1000), ('rs_x_destroy', 0x1000)]
    o.close()
    del o
    gc.collect()
    assert len(lib.calls) == 2
    assert h.destroy() == _lib.RS_OK and len(lib.calls) == 2     # the Handle itself: no second call


def test_with_block_closes():
    lib = FakeLib()
    with Owner(lib) as o:
        assert o._second.value == 0x2000
    assert o._h is None and o._second is None
    assert [c[0] for c in lib.calls[2:]] == ['rs_x_destroy', 'rs_y_destroy']


def test_an_error_of_the_first_destroy_is_raised_after_everything_is_released():
    lib = FakeLib(rs_x_destroy=_lib.RS_ERR_HIP, rs_y_destroy=_lib.RS_ERR_ARG)
    o = Owner(lib)
    with pytest.raises(_lib.HipLibraryError):      # the first status that is not RS_OK
        o.close()
    assert lib.calls[2:] == [('rs_x_destroy', 0x1000), ('rs_y_destroy', 0x2000)]
    assert o._h is None and o._second is None and o.more == 1
    o.close()                                       # nothing left: no call, no error
    assert len(lib.calls) == 4 and o.more == 2


def test_finalisation_swallows():
    lib = FakeLib(rs_x_destroy=_lib.RS_ERR_HIP)
    o = Owner(lib)
    o.__del__()
    assert [c[0] for c in lib.calls[2:]] == ['rs_x_destroy', 'rs_y_destroy'] and o.more == 1
    del o
    gc.collect()
    assert len(lib.calls) == 4


def test_an_instance_without_attributes_can_be_closed_and_finalised():
    o = object.__new__(Owner)
    o.more = 0
    o.close()
    assert o._h is None and o._second is None and o.more == 1
    bare = object.__new__(_lib.DeviceBuffer)
    bare.close()
    assert bare.ptr is None
    del bare
    half = object.__new__(Owner)        # _close_more raises AttributeError (no ``more``): swallowed
    half.__del__()


def test_a_handle_passes_where_the_abi_takes_a_void_pointer():
    lib = FakeLib()
    h = _lib.Handle.create(lib, 'rs_x_create', 'rs_x_destroy', 0x1234)
    seen = []

    @ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)
    def by_value(p):
        seen.append(p)
        return 0

    @ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(ctypes.c_void_p))
    def by_reference(pp):
        seen.append(pp[0])
        pp[0] = 0x5678
        return 0

    by_value.argtypes = [ctypes.c_void_p]
    assert by_value(h) == 0 and seen == [0x1234]
    assert by_reference(ctypes.byref(h)) == 0 and seen == [0x1234, 0x1234]
    assert h.value == 0x5678                       # written through byref, as a create call does
    assert h.destroy() == _lib.RS_OK and lib.calls[-1] == ('rs_x_destroy', 0x5678)
    assert not h.value
