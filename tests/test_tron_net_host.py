"""The policy-value MLP of the Tron search (crl_tron_net_*) on the host: every CRL_EINVAL case is refused with its message before
any device work, the board limit, the packed size, the prototypes, and the Python wrappers' argument checks."""
import ctypes as C

import pytest

from tests.host_util import D, fake as _fake, lib as _lib, refused, tron_context, ttt_context

ODD = C.c_void_p(72)                       # 8-byte aligned only
PTRS = (C.c_void_p * 5)(*[64] * 5)         # a host array of L + 2 non-NULL "device" pointers (never dereferenced)


def _pack(lib, ctx, H=64, L=2, weight=PTRS, bias=PTRS, net=D):
    return lib.crl_tron_net_pack(ctx, H, L, weight, bias, net, None)


def _eval(lib, ctx, B=4, net=D, H=64, L=2, board=D, heads=D, dirs=D, pending=D, prior=D, value=D, flags=0):
    return lib.crl_tron_net_eval(ctx, B, net, H, L, board, heads, dirs, pending, prior, value, flags, None)


def test_argument_checks():
    lib = _lib()
    with tron_context() as h:
        for fn in (_pack, _eval):
            refused(lib, fn(lib, h, net=None), b"NULL net")
            refused(lib, fn(lib, h, net=ODD), b"16-byte aligned")
            for bad in (0, 8, 24, 272, -16):
                refused(lib, fn(lib, h, H=bad), b"H=")
            for bad in (0, 4, -1):
                refused(lib, fn(lib, h, L=bad), b"L=")
            refused(lib, fn(lib, None), b"tron")
        for B in (0, -1, (1 << 31) + 1):
            refused(lib, _eval(lib, h, B=B), b"B=")
        for name in ("board", "heads", "dirs"):
            refused(lib, _eval(lib, h, **{name: None}), b"NULL input")
        for name in ("prior", "value"):
            refused(lib, _eval(lib, h, **{name: None}), b"NULL output")
        for flags in (1, 0x80000000):
            refused(lib, _eval(lib, h, flags=flags), b"flags")
        refused(lib, _eval(lib, h, pending=None, H=256, L=3, flags=1), b"flags")    # pending may be NULL, the greatest shape passes
        for name in ("weight", "bias"):
            refused(lib, _pack(lib, h, **{name: None}), b"NULL weight or bias array")
            refused(lib, _pack(lib, h, **{name: (C.c_void_p * 5)(64, 64, 64, None, 64)}), b"matrix 3")
    with ttt_context() as ttt:
        refused(lib, _pack(lib, ttt), b"tron")
        refused(lib, _eval(lib, ttt), b"tron")
        assert lib.crl_tron_net_bytes(ttt, 64, 2) == -1 and b"tron" in lib.crl_last_error()
    with tron_context(41, 2, (0, 1680), (0, 2)) as big:                              # above the LDS plan: CRL_EUNSUPPORTED (-4)
        assert lib.crl_tron_net_bytes(big, 64, 2) == -4 and b"40x40" in lib.crl_last_error()
        assert _pack(lib, big) == -4 and _eval(lib, big) == -4
        refused(lib, _eval(lib, big, H=8), b"H=")


@pytest.mark.parametrize("N, p", [(5, 2), (11, 4), (20, 4), (40, 8)])
def test_net_bytes(N, p):
    lib = _lib()
    with tron_context(N, p, range(p), [0] * p) as h:
        size = {(H, L): lib.crl_tron_net_bytes(h, H, L) for H in range(16, 257, 16) for L in (1, 2, 3)}
        assert all(n > 0 and n % 16 == 0 for n in size.values())
        assert all(size[H, L] < size[H + 16, L] for H in range(16, 256, 16) for L in (1, 2, 3))       # grows with H
        assert all(size[H, 1] < size[H, 2] < size[H, 3] for H in range(16, 257, 16))                    # and with L
        assert all(n >= 4 * (H * (4 * N * N + 4) + (L - 1) * H * H + 4 * H + L * H + 4) for (H, L), n in size.items())
        assert all(lib.crl_tron_net_bytes(h, *bad) == -1 and lib.crl_last_error() for bad in ((40, 2), (64, 0)))
    assert lib.crl_tron_net_bytes(None, 64, 2) == -1
    from colosseumrl_amd import _native                      # the three prototypes are bound, under the same revision
    assert _native.CRL_ABI_VERSION == 113 and lib.crl_version() == 113
    assert all("crl_tron_net_" + name in _native.PROTOTYPES and hasattr(lib, "crl_tron_net_" + name) for name in ("bytes", "pack", "eval"))


def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch, TronNet
    tb = _fake(TronBatch, B=5, P=2, N=5)

    def layer(n_out, n_in, dtype=torch.float32):
        return torch.zeros((n_out, n_in), dtype=dtype), torch.zeros((n_out,), dtype=dtype)
    good = dict(hidden=[layer(32, 104), layer(32, 32)], policy=layer(3, 32), value=layer(1, 32))
    bad_nets = [dict(hidden=[]), dict(hidden=[layer(32, 104)] + [layer(32, 32)] * 3), dict(hidden=None),    # counts of layers
                dict(hidden=[layer(24, 104), layer(24, 24)], policy=layer(3, 24), value=layer(1, 24)),        # H not a multiple of 16
                dict(hidden=[layer(32, 100), layer(32, 32)]), dict(hidden=[layer(32, 104), layer(32, 16)]),   # shapes
                dict(policy=layer(4, 32)), dict(value=layer(2, 32)), dict(value=(torch.zeros((1, 32)), torch.zeros((2,)))),
                dict(policy=layer(3, 32, torch.float64)), dict(hidden=[layer(32, 104, torch.float16), layer(32, 32)]),   # dtypes
                dict(policy=torch.zeros((3, 32))), dict(value=(torch.zeros((1, 32)), None))]                   # a missing bias
    for bad in bad_nets:
        with pytest.raises(ValueError):
            tb.net_pack(**dict(good, **bad))
    net = TronNet(tb, 5, 32, 2, torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="repack"):
        net.repack([layer(32, 104)], good["policy"], good["value"])
    board, heads, dirs = torch.zeros((5, 25), dtype=torch.int8), torch.zeros((2, 5), dtype=torch.int16), torch.zeros((2, 5), dtype=torch.int8)
    pending, out = torch.ones((5,), dtype=torch.uint8), (torch.zeros((5, 3), dtype=torch.int16), torch.zeros((5,), dtype=torch.int32))
    with pytest.raises(ValueError, match="net_pack"):                                                          # a net of another board
        tb.net_eval(TronNet(_fake(TronBatch, B=5, P=2, N=6), 6, 32, 2, net.packed), board, heads, dirs, pending, out)
    for args in ((board.to(torch.int32), heads, dirs, pending, out), (board[:, :24].contiguous(), heads, dirs, pending, out),
                 (None, heads, dirs, pending, out), (board, heads.to(torch.int32), dirs, pending, out), (board, heads[:1], dirs, pending, out),
                 (board, heads, None, pending, out), (board, heads, dirs[:, :4].contiguous(), pending, out),
                 (board, heads, dirs, pending.to(torch.int8), out), (board, heads, dirs, pending[:4], out),
                 (board, heads, dirs, pending, (out[0].to(torch.int32), out[1])), (board, heads, dirs, pending, (out[0], out[1][:4]))):
        with pytest.raises(ValueError):
            tb.net_eval(net, *args)
