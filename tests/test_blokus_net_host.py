"""The policy-value MLP of the Blokus search (crl_blokus_net_*) on the host: every CRL_EINVAL case is refused with its message
before any device work (the context is checked last, so the others need no device) and the prototypes.  The packed
size needs a Blokus context, which needs a device: that one test is marked gpu."""
import ctypes as C

import pytest

from tests.host_util import D, lib as _lib, refused, ttt_context

ODD = C.c_void_p(72)                       # 8-byte aligned only
PTRS = (C.c_void_p * 6)(*[64] * 6)         # a host array of L + 3 non-NULL "device" pointers (never dereferenced)
EVAL = dict(B=4, net=D, H=64, L=2, W=16, board=D, pieces=D, cand=D, n_cand=D, mover=D, pending=D, prior=D, value=D, flags=0)


def _pack(lib, ctx=None, H=64, L=2, weight=PTRS, bias=PTRS, net=D):
    return lib.crl_blokus_net_pack(ctx, H, L, weight, bias, net, None)


def _eval(lib, ctx=None, **kw):
    a = dict(EVAL, **kw)
    return lib.crl_blokus_net_eval(ctx, a["B"], a["net"], a["H"], a["L"], a["W"], a["board"], a["pieces"], a["cand"], a["n_cand"],
                                   a["mover"], a["pending"], a["prior"], a["value"], a["flags"], None)


REFUSALS = ([(fn, dict(net=None), b"NULL net") for fn in (_pack, _eval)] + [(fn, dict(net=ODD), b"16-byte aligned") for fn in (_pack, _eval)]
            + [(fn, dict(H=bad), b"H=") for fn in (_pack, _eval) for bad in (0, 8, 24, 272, -16)]
            + [(fn, dict(L=bad), b"L=") for fn in (_pack, _eval) for bad in (0, 4, -1)]
            + [(_eval, dict(W=bad), b"W=") for bad in (0, 65, -1)]
            + [(_eval, dict(B=bad), b"B=") for bad in (0, -1, (1 << 31) + 1)]
            + [(_eval, {name: None}, b"NULL input") for name in ("board", "pieces", "cand", "n_cand", "mover")]
            + [(_eval, {name: None}, b"NULL output") for name in ("prior", "value")]
            + [(_eval, dict(flags=bad), b"flags") for bad in (1, 0x80000000)]
            + [(_eval, dict(pending=None, H=256, L=3, W=64, flags=1), b"flags")]     # pending may be NULL, the greatest shape passes
            + [(_pack, {name: None}, b"NULL weight or bias array") for name in ("weight", "bias")]
            + [(_pack, {name: (C.c_void_p * 5)(64, 64, 64, None, 64)}, b"matrix 3") for name in ("weight", "bias")]
            + [(fn, {}, b"blokus context") for fn in (_pack, _eval)])                # everything else in order: the context


@pytest.mark.parametrize("fn, bad, word", REFUSALS, ids=["%d%s_%s" % (i, fn.__name__, "_".join(bad) or "ctx") for i, (fn, bad, _) in enumerate(REFUSALS)])
def test_refusals(fn, bad, word):
    lib = _lib()
    refused(lib, fn(lib, **bad), b"crl_blokus_net_", word)


def test_context_and_prototypes():
    lib = _lib()
    with ttt_context() as ttt:
        refused(lib, _pack(lib, ttt), b"blokus context")
        refused(lib, _eval(lib, ttt), b"blokus context")
        assert lib.crl_blokus_net_bytes(ttt, 64, 2) == -1 and b"blokus context" in lib.crl_last_error()
    assert lib.crl_blokus_net_bytes(None, 40, 2) == -1 and b"H=" in lib.crl_last_error()
    assert lib.crl_blokus_net_bytes(None, 64, 0) == -1 and b"L=" in lib.crl_last_error()
    from colosseumrl_amd import _native                      # the three prototypes are bound, under the same revision
    assert _native.CRL_ABI_VERSION == 113 and lib.crl_version() == 113
    assert all("crl_blokus_net_" + name in _native.PROTOTYPES and hasattr(lib, "crl_blokus_net_" + name) for name in ("bytes", "pack", "eval"))


@pytest.mark.gpu
def test_net_bytes():
    lib, h = _lib(), C.c_void_p()
    assert lib.crl_blokus_create(C.byref(h)) == 0
    try:
        size = {(H, L): lib.crl_blokus_net_bytes(h, H, L) for H in range(16, 257, 16) for L in (1, 2, 3)}
    finally:
        lib.crl_destroy(h)
    assert all(n > 0 and n % 16 == 0 for n in size.values())
    assert all(size[H, L] < size[H + 16, L] for H in range(16, 256, 16) for L in (1, 2, 3))           # grows with H
    assert all(size[H, 1] < size[H, 2] < size[H, 3] for H in range(16, 257, 16))                        # and with L
    assert all(n >= 4 * (H * 1684 + (L - 1) * H * H + 425 * H + L * H + 425) for (H, L), n in size.items())

