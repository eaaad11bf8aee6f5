"""The policy-value MLP of the TicTacToe search (crl_ttt_net_*) on the host: every CRL_EINVAL case is refused with its message
before any device work, the packed size, the prototypes, and the Python wrappers' argument checks."""
import ctypes as C

import pytest

from tests.host_util import D, fake as _fake, lib as _lib, refused, tron_context, ttt_context

ODD = C.c_void_p(72)                       # 8-byte aligned only
PTRS = (C.c_void_p * 5)(*[64] * 5)         # a host array of L + 2 non-NULL "device" pointers (never dereferenced)


def _pack(lib, ctx, C_=2, H=64, L=2, weight=PTRS, bias=PTRS, net=D):
    return lib.crl_ttt_net_pack(ctx, C_, H, L, weight, bias, net, None)


def _eval(lib, ctx, B=4, net=D, C_=2, H=64, L=2, board=D, valid=D, pending=D, prior=D, value=D, flags=0):
    return lib.crl_ttt_net_eval(ctx, B, net, C_, H, L, board, valid, pending, prior, value, flags, None)


def test_argument_checks():
    lib = _lib()
    with ttt_context() as h:
        for fn in (_pack, _eval):
            refused(lib, fn(lib, h, net=None), b"NULL net")
            refused(lib, fn(lib, h, net=ODD), b"16-byte aligned")
            for bad in (0, -1, 9):
                refused(lib, fn(lib, h, C_=bad), b"C=")
            for bad in (0, 8, 24, 272, -16):
                refused(lib, fn(lib, h, H=bad), b"H=")
            for bad in (0, 4, -1):
                refused(lib, fn(lib, h, L=bad), b"L=")
            refused(lib, fn(lib, None), b"tictactoe")
        for B in (0, -1, (1 << 31) + 1):
            refused(lib, _eval(lib, h, B=B), b"B=")
        for name in ("board", "valid"):
            refused(lib, _eval(lib, h, **{name: None}), b"NULL input")
        for name in ("prior", "value"):
            refused(lib, _eval(lib, h, **{name: None}), b"NULL output")
        for flags in (1, 0x80000000):
            refused(lib, _eval(lib, h, flags=flags), b"flags")
        refused(lib, _eval(lib, h, pending=None, C_=8, H=256, L=3, flags=1), b"flags")   # pending may be NULL, the greatest shape passes
        for name in ("weight", "bias"):
            refused(lib, _pack(lib, h, **{name: None}), b"NULL weight or bias array")
            refused(lib, _pack(lib, h, **{name: (C.c_void_p * 5)(64, 64, 64, None, 64)}), b"matrix 3")
    with tron_context() as tron:
        refused(lib, _pack(lib, tron), b"tictactoe")
        refused(lib, _eval(lib, tron), b"tictactoe")
        assert lib.crl_ttt_net_bytes(tron, 2, 64, 2) == -1 and b"tictactoe" in lib.crl_last_error()


@pytest.mark.parametrize("d3, p", [((1, 3, 3), 2), ((3, 3, 3), 4), ((1, 5, 5), 3)])
def test_net_bytes(d3, p):
    lib, cells = _lib(), d3[0] * d3[1] * d3[2]
    with ttt_context(*d3, 3, p) as h:
        for c in (1, p, 8):
            size = {(H, L): lib.crl_ttt_net_bytes(h, c, H, L) for H in range(16, 257, 16) for L in (1, 2, 3)}
            assert all(n > 0 and n % 16 == 0 for n in size.values())
            assert all(size[H, L] < size[H + 16, L] for H in range(16, 256, 16) for L in (1, 2, 3))       # grows with H
            assert all(size[H, 1] < size[H, 2] < size[H, 3] for H in range(16, 257, 16))                    # and with L
            assert all(n >= 4 * (H * cells * c + (L - 1) * H * H + (cells + p) * H + L * H + cells + p) for (H, L), n in size.items())
        assert all(lib.crl_ttt_net_bytes(h, *bad) == -1 and lib.crl_last_error() for bad in ((0, 64, 2), (2, 40, 2), (2, 64, 0)))
    assert lib.crl_ttt_net_bytes(None, 2, 64, 2) == -1
    from colosseumrl_amd import _native                      # the three prototypes are bound, under the same revision
    assert _native.CRL_ABI_VERSION == 113 and lib.crl_version() == 113
    assert all("crl_ttt_net_" + name in _native.PROTOTYPES and hasattr(lib, "crl_ttt_net_" + name) for name in ("bytes", "pack", "eval"))


def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TTTBatch, TTTNet
    tb = _fake(TTTBatch, B=5, P=2, n_cells=9)

    def layer(n_out, n_in, dtype=torch.float32):
        return torch.zeros((n_out, n_in), dtype=dtype), torch.zeros((n_out,), dtype=dtype)
    good = dict(hidden=[layer(32, 18), layer(32, 32)], policy=layer(9, 32), value=layer(2, 32))
    bad_nets = [dict(hidden=[]), dict(hidden=[layer(32, 18)] + [layer(32, 32)] * 3), dict(hidden=None),      # counts of layers
                dict(hidden=[layer(24, 18), layer(24, 24)], policy=layer(9, 24), value=layer(2, 24)),          # H not a multiple of 16
                dict(hidden=[layer(32, 27), layer(32, 32)]), dict(hidden=[layer(32, 18), layer(32, 16)]),      # shapes
                dict(policy=layer(8, 32)), dict(value=layer(3, 32)), dict(value=(torch.zeros((2, 32)), torch.zeros((3,)))),
                dict(policy=layer(9, 32, torch.float64)), dict(hidden=[layer(32, 18, torch.float16), layer(32, 32)]),   # dtypes
                dict(policy=torch.zeros((9, 32))), dict(value=(torch.zeros((2, 32)), None)), dict(planes=0), dict(planes=9), dict(planes=3)]
    for bad in bad_nets:
        with pytest.raises(ValueError):
            tb.net_pack(**dict(good, **bad))
    net = TTTNet(tb, 2, 32, 2, torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="repack"):
        net.repack([layer(32, 18)], good["policy"], good["value"])
    board, valid, pending = torch.zeros((5, 9), dtype=torch.int8), torch.zeros((5,), dtype=torch.int32), torch.ones((5,), dtype=torch.uint8)
    out = (torch.zeros((5, 9), dtype=torch.int16), torch.zeros((5, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="net_pack"):
        tb.net_eval(TTTNet(_fake(TTTBatch), 2, 32, 2, net.packed), board, valid, pending, out)
    for args in ((board.to(torch.int32), valid, pending, out), (board[:, :8].contiguous(), valid, pending, out), (None, valid, pending, out),
                 (board, valid.to(torch.int64), pending, out), (board, valid[:4], pending, out), (board, valid, pending.to(torch.int8), out),
                 (board, valid, pending, (out[0].to(torch.int32), out[1])), (board, valid, pending, (out[0], out[1][:4]))):
        with pytest.raises(ValueError):
            tb.net_eval(net, *args)
