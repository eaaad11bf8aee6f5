"""The scripted avoid agent (crl_tron_sample_avoid / crl_tron_rollout_avoid) on the host: its numpy restatement against
games the reference's own SimpleAvoidAgent played (tests/golden/tron_avoid_*.npz), the fixture generator, and the
argument checks of the C entry points (they fail before any device work)."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rng_ref, tron_ref
from tests.host_util import D, lib as _lib, tron_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "tron_avoid_*.npz")))


def _load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_fixture_set():
    names = {os.path.basename(p) for p in GOLDEN}
    assert len(names) >= 8
    recs = [_load(p) for p in GOLDEN]
    assert {int(r["N"]) for r in recs} >= {15, 19, 20, 40}
    assert {int(r["P"]) for r in recs} >= {2, 3, 4}
    assert {(int(r["noise_num"]), int(r["noise_den"])) for r in recs} >= {(0, 10), (1, 10), (10, 10)}
    assert sum(int(r["n_wall"]) for r in recs) > 0 and sum(int(r["n_boxed"]) for r in recs) > 0
    for r in recs:
        for k, v in r.items():
            assert v.dtype.kind in "iu", (k, v.dtype)


def test_philox_matches_oracle():
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    for _ in range(40):
        ctr = rng.integers(0, 2 ** 32, size=4, dtype=np.uint64)
        seed = int(rng.integers(0, 2 ** 63))
        want = O.philox4x32(ctr.astype(np.uint32), [seed & 0xFFFFFFFF, seed >> 32])
        got = rng_ref.philox(*[np.uint64(c) for c in ctr], seed)
        assert [int(x) for x in got] == [int(x) for x in want]


def test_threshold():
    assert rng_ref.threshold(0.0) == 0
    assert rng_ref.threshold(1.0) == 1 << 32
    assert rng_ref.threshold(0.5) == 1 << 31
    assert rng_ref.threshold(1e-12) == 1


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_numpy_contract_reproduces_reference_actions(path):
    r = _load(path)
    N, P, seed = int(r["N"]), int(r["P"]), int(r["seed"])
    noise = int(r["noise_num"]) / int(r["noise_den"])
    S = len(r["c"])
    g = np.arange(S, dtype=np.uint64)
    w = np.stack(tron_ref.words(g[None, :], r["c"].astype(np.uint64)[None, :], np.arange(P, dtype=np.uint64)[:, None], seed), -1)
    assert np.array_equal(w.transpose(1, 0, 2), r["words"])
    act = tron_ref.decide(N, r["board"], r["heads"].T.copy(), r["dirs"].T.copy(), r["deaths"].T.copy(), g, r["c"], seed, noise)
    assert np.array_equal(act.T, r["actions"])
    # ... and the CPU oracle's step of those actions is the reference's next_state
    from oracle import oracle as O
    st = O.TronState(N, P, S)
    st.board[...] = r["board"]
    st.heads[...] = r["heads"].T
    st.dirs[...] = r["dirs"].T
    st.deaths[...] = r["deaths"].T
    O.tron_step(st, np.ascontiguousarray(act))
    assert np.array_equal(st.board, r["next_board"]) and np.array_equal(st.heads.T, r["next_heads"])
    assert np.array_equal(st.dirs.T, r["next_dirs"]) and np.array_equal(st.deaths.T, r["next_deaths"])


def _reference_present():
    from oracle import ref_loader
    return ref_loader.available()


def test_generator_regenerates_fixtures():
    if not _reference_present():
        pytest.skip("the reference tree is only present where the fixtures are generated")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_avoid.py"), "--check"],
                          capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr


def test_generator_contract_random():
    """Generator smoke test: the stand-in for the reference's ``random`` answers as the contract says."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_golden_avoid as G
    finally:
        sys.path.pop(0)
    fake = G.ContractRandom()
    for noise in (0.0, 0.1, 1.0):
        fake.noise, fake.thr = noise, rng_ref.threshold(noise)
        for w0 in (0, 1, fake.thr - 1, fake.thr, 2 ** 32 - 1):
            if not 0 <= w0 < 2 ** 32:
                continue
            fake.w = np.array([w0, 0, 0], np.uint32)
            assert (fake.random() <= noise) == (w0 < fake.thr)
    fake.w = np.array([0, 2 ** 32 - 1, 2 ** 31], np.uint32)
    assert fake.choice(["forward", "right", "left"]) == "left"
    assert fake.choice([(1, "right", "left"), (-1, "left", "right")])[0] == -1
    fake.w = np.array([0, 0, 2 ** 31 - 1], np.uint32)
    assert fake.choice(["forward", "right", "left"]) == "forward"
    assert fake.choice([(1, "right", "left"), (-1, "left", "right")])[0] == 1
    assert G.file_name(19, 4, 1, 10) == "tron_avoid_n19p4_z10.npz"


# ---- argument checks of the C entry points (rejected before anything touches a device)
def _ctx(N=9, P=4):
    from oracle import oracle as O
    return tron_context(N, P, *O.tron_start_positions(N, P))


def test_sample_avoid_argument_checks():
    from colosseumrl_amd import _native
    lib = _lib()
    with _ctx() as h:
        def call(noise=0.1, mask=0xF, ptrs=(D,) * 6):
            tc, board, heads, dirs, deaths, acts = ptrs
            return lib.crl_tron_sample_avoid(h, 4, 1, 0, tc, 1, noise, mask, board, heads, dirs, deaths, acts, None)
        for noise in (-0.01, 1.01, float("nan"), float("inf")):
            assert call(noise=noise) == -1
            assert b"noise" in lib.crl_last_error()
        assert call(mask=0x10) == -1 and b"player_mask" in lib.crl_last_error()
        assert call(mask=0x80000000) == -1
        for i in range(6):
            ptrs = [D] * 6
            ptrs[i] = None
            assert call(ptrs=tuple(ptrs)) == -1 and b"NULL" in lib.crl_last_error()
        assert lib.crl_tron_sample_avoid(None, 4, 1, 0, D, 1, 0.1, 1, D, D, D, D, D, None) == -1
        assert lib.crl_tron_sample_avoid(h, 0, 1, 0, D, 1, 0.1, 1, D, D, D, D, D, None) == -1
    assert _native.PROTOTYPES["crl_tron_sample_avoid"][1][6] is C.c_double


def test_rollout_avoid_argument_checks():
    from colosseumrl_amd._native import TronStats
    lib = _lib()
    full = TronStats(*([64] * 8 + [None, None]))
    with _ctx() as h:
        def call(noise=0.1, T=4, flags=0, stats=full, state=(D,) * 4):
            return lib.crl_tron_rollout_avoid(h, 4, 1, 0, T, noise, *state, stats, flags, None)
        for noise in (-1.0, 2.0, float("nan")):
            assert call(noise=noise) == -1 and b"noise" in lib.crl_last_error()
        assert call(T=-1) == -1
        assert call(flags=1) == -1 and b"flags" in lib.crl_last_error()
        for i in range(4):
            st = [D] * 4
            st[i] = None
            assert call(state=tuple(st)) == -1 and b"NULL" in lib.crl_last_error()
        for i in range(8):
            vals = [64] * 8 + [None, None]
            vals[i] = None
            assert call(stats=TronStats(*vals)) == -1 and b"NULL" in lib.crl_last_error()
        assert call(T=0) == 0                                      # nothing to do: no launch


def test_step_single_argument_checks():
    lib = _lib()
    with _ctx() as h:
        for i in range(9):
            ptrs = [D] * 9
            ptrs[i] = None
            assert lib.crl_tron_step_single(h, 4, *ptrs, None) == -1 and b"NULL" in lib.crl_last_error()
