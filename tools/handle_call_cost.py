#!/usr/bin/env python3
"""What passing a ``c_void_p`` subclass (``_lib.Handle``) costs per call against a plain
``c_void_p``, through a prebound ``CFUNCTYPE`` of ``_update_odom``'s prototype (host only:
the C function ignores its arguments, so the marshalling is what is timed).  Alternating
samples; figures in profiles/py_bindings/README.md."""
import ctypes
import statistics
import time

libc = ctypes.CDLL(None)
proto = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p)
f = proto(('getpid', libc))


class Handle(ctypes.c_void_p):
    _destroy = None


def run(h, n=200000):
    t0 = time.perf_counter()
    for _ in range(n):
        f(h, 0.2, 0.01, 12345)
    return 1e9 * (time.perf_counter() - t0) / n


if __name__ == '__main__':
    plain, sub = ctypes.c_void_p(0x1000), Handle(0x1000)
    sub._destroy = f
    res = {'plain c_void_p': [], 'Handle': []}
    for _ in range(9):
        res['plain c_void_p'].append(run(plain))
        res['Handle'].append(run(sub))
    for k, v in res.items():
        print('%s: ns per call, median %.1f min %.1f max %.1f' % (k, statistics.median(v), min(v), max(v)))
