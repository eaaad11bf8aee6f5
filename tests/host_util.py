"""What the host tests of the C entry points and the Python wrappers share."""
import contextlib
import ctypes as C

D = C.c_void_p(64)                         # 16-byte aligned, never dereferenced: the calls made with it are refused by their checks or do no work


def lib():
    from colosseumrl_amd import _native
    return _native.lib()


def fake(cls, **attrs):
    """an instance of a batch class made without a device, for the argument checks that run before any device work"""
    import torch
    obj = cls.__new__(cls)
    obj.device = torch.device("cpu")
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def refused(lib, rc, *words):
    """the call returned -1 and the library's last error names every word"""
    msg = lib.crl_last_error()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


@contextlib.contextmanager
def ttt_context(d0=1, d1=3, d2=3, K=3, P=2):
    """a TicTacToe context of the library (by default 3x3, two players), destroyed on the way out"""
    h = C.c_void_p()
    assert lib().crl_ttt_create(d0, d1, d2, K, P, C.byref(h)) == 0
    try:
        yield h
    finally:
        lib().crl_destroy(h)


@contextlib.contextmanager
def tron_context(N=5, P=2, heads=(0, 24), dirs=(0, 2)):
    """a Tron context of the library (by default 5x5, two players in opposite corners), destroyed on the way out"""
    h = C.c_void_p()
    sh, sd = (C.c_int16 * P)(*[int(x) for x in heads]), (C.c_int8 * P)(*[int(x) for x in dirs])
    assert lib().crl_tron_create(N, P, sh, sd, C.byref(h)) == 0
    try:
        yield h
    finally:
        lib().crl_destroy(h)
