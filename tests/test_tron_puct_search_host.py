"""The one-launch Tron search (crl_tron_puct_search) on the host: every CRL_EINVAL case is refused with its message before any
device work, boards above 40x40 are unsupported, the prototype is bound, and the Python wrappers check their arguments."""
import ctypes as C

import pytest

from tests.host_util import D, fake as _fake, lib as _lib, refused, tron_context, ttt_context

ODD = C.c_void_p(72)                       # 8-byte aligned only
GOOD = dict(B=4, tree=D, S_cap=8, n_sims=8, net=D, H=64, L=2, cpuct=320, fpu=32768, flags=0)
REFUSALS = [(dict(B=0), b"B="), (dict(B=-1), b"B="), (dict(B=(1 << 31) + 1), b"B="),
            (dict(tree=None), b"NULL tree"), (dict(tree=ODD), b"tree must be 16-byte aligned"),
            (dict(S_cap=0), b"S_cap="), (dict(S_cap=4096), b"S_cap="),
            (dict(n_sims=0), b"n_sims="), (dict(n_sims=-3), b"n_sims="), (dict(n_sims=4096), b"n_sims="),
            (dict(H=0), b"H="), (dict(H=8), b"H="), (dict(H=24), b"H="), (dict(H=272), b"H="),
            (dict(L=0), b"L="), (dict(L=4), b"L="),
            (dict(net=None), b"NULL net"), (dict(net=ODD), b"net must be 16-byte aligned"),
            (dict(cpuct=65536), b"cpuct="), (dict(fpu=65537), b"fpu="),
            (dict(flags=1), b"flags"), (dict(flags=0x80000000), b"flags"),
            (dict(n_sims=4095, S_cap=4095, H=256, L=3, cpuct=65535, fpu=65536, flags=2), b"flags")]      # the greatest shape passes


def _search(lib, ctx, **kw):
    a = dict(GOOD, **kw)
    return lib.crl_tron_puct_search(ctx, a["B"], a["tree"], a["S_cap"], a["n_sims"], a["net"], a["H"], a["L"], a["cpuct"], a["fpu"],
                                    a["flags"], None)


@pytest.mark.parametrize("bad, word", REFUSALS, ids=["%s=%r" % kv for bad, _ in REFUSALS for kv in list(bad.items())[:1]])
def test_refusals(bad, word):
    lib = _lib()
    with tron_context() as h:
        refused(lib, _search(lib, h, **bad), b"crl_tron_puct_search", word)


def test_contexts_and_prototype():
    lib = _lib()
    refused(lib, _search(lib, None), b"crl_tron_puct_search", b"tron context")
    with ttt_context() as ttt:
        refused(lib, _search(lib, ttt), b"tron context")
    with tron_context(41, 2, (0, 41 * 41 - 1), (0, 2)) as big:     # above the LDS plan: unsupported, not invalid
        assert _search(lib, big) == -4 and b"41" in lib.crl_last_error()
    from colosseumrl_amd import _native
    assert _native.CRL_ABI_VERSION == 113 and lib.crl_version() == 113
    assert len(_native.PROTOTYPES["crl_tron_puct_search"][1]) == 12 and hasattr(lib, "crl_tron_puct_search")


def test_wrapper_argument_checks():
    import torch
    from colosseumrl_amd.batched import TronBatch, TronNet
    tb = _fake(TronBatch, B=5, P=2, N=5)
    net = TronNet(tb, 5, 32, 2, torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="puct_begin"):
        tb.puct_search(net, 4)
    tb._puct_tree, tb._puct_cap = torch.zeros((5, 4, 2), dtype=torch.int64), 8
    other = TronNet(_fake(TronBatch, N=7), 7, 32, 2, net.packed)
    for fn in (tb.puct_search, tb.puct_net, tb.puct_net_action):
        for bad_net in (other, None, net.evaluator()):
            with pytest.raises(ValueError, match="net_pack"):
                fn(bad_net, 4)
        for kw in (dict(simulations=0), dict(simulations=4096), dict(simulations=2.0), dict(simulations=True),
                   dict(simulations=4, exploration=-1.0), dict(simulations=4, exploration=256.0), dict(simulations=4, fpu=1.5),
                   dict(simulations=4, fpu=float("nan"))):
            with pytest.raises(ValueError):
                fn(net, **kw)
    with pytest.raises(ValueError, match="callable"):       # puct keeps its contract: a handle is not an evaluator
        tb.puct(net, 4)
