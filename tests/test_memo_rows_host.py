"""k_memo_rows on the host build (tests/memo_rows_host.cpp): the row copies of the pose memo, byte for byte.

Every case fills the output array, the pool and a guard band around each with distinct NaN-payload words, runs ONE launch
and compares the whole backing buffers as uint32 with numpy fancy indexing: the rows named are moved bit for bit, and every
other word - rows and slots that are not named, the bytes behind a row's end, the guards - comes back untouched.
Row sizes: 5 (4-byte path), 3380 (the 16 kHz spectrogram row, 16-byte path), 8970 (the 44.1 kHz spectrogram row: even, no
multiple of 4 - 8-byte path), 32000 and 88200 (audiogoal rows: 8 and 22 chunks per row); bases pushed 4 and 8 bytes off 16-byte
alignment take the narrower paths for a row size that would allow 16."""
import ctypes
import os

import numpy as np
import pytest

hs = pytest.importorskip("hostsim.hs")

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
N_ROWS, N_SLOTS = 40, 50


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("memo_rows", tmp_path_factory.mktemp("memo_rows"))
    L = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.hs_memo_rows.argtypes = [vp, vp, vp, ci, vp, ci, ci, ci]
    L.hs_memo_rows.restype = ci
    return L


class Arr:
    """rows x rf float32 words inside a guarded backing buffer whose first row sits `off` bytes behind a 16-byte boundary"""

    def __init__(self, rows, rf, off, seed):
        assert off % 4 == 0
        self.back = np.empty((rows * rf + 2 * GUARD + 8,), np.uint32)
        start = GUARD + ((-(self.back.ctypes.data + 4 * GUARD)) % 16) // 4 + off // 4
        # quiet-NaN words with distinct payloads: any float arithmetic or a wrong source would change them
        self.back[:] = 0x7fc00000 | ((np.arange(self.back.shape[0], dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)) & 0x3fffff)
        self.view = self.back[start:start + rows * rf].reshape(rows, rf)
        assert self.view.ctypes.data % 16 == off
        self.lo, self.hi = start, start + rows * rf
        self.before = self.back.copy()

    def expect(self, rows_view_update):
        exp = self.before.copy()
        rows_view_update(exp[self.lo:self.hi].reshape(self.view.shape))
        return exp


def _moves(n_store, n_fetch, rng):
    n = n_store + n_fetch
    rows = rng.permutation(N_ROWS)[:n]
    slots = rng.permutation(N_SLOTS)[:n]
    return np.ascontiguousarray(np.stack([rows, slots], 1).astype(np.int32))


def _run(lib, pairs, moves, n_store, n_fetch, tab):
    """pairs: [(out Arr, pool Arr)] -> asserts the whole buffers against numpy"""
    outs = (ctypes.c_void_p * len(pairs))(*[o.view.ctypes.data for o, _ in pairs])
    pools = (ctypes.c_void_p * len(pairs))(*[p.view.ctypes.data for _, p in pairs])
    rf = np.asarray([o.view.shape[1] for o, _ in pairs], np.int32)
    assert lib.hs_memo_rows(outs, pools, rf.ctypes.data, len(pairs), moves.ctypes.data, n_store, n_fetch, int(tab)) == 0
    st, ft = moves[:n_store], moves[n_store:n_store + n_fetch]
    for o, p in pairs:
        out0 = o.before[o.lo:o.hi].reshape(o.view.shape)
        pool0 = p.before[p.lo:p.hi].reshape(p.view.shape)

        def upd_pool(v):
            v[st[:, 1]] = out0[st[:, 0]]

        def upd_out(v):
            v[ft[:, 0]] = pool0[ft[:, 1]]
        assert np.array_equal(p.back, p.expect(upd_pool))
        assert np.array_equal(o.back, o.expect(upd_out))


LISTS = {"stores": lambda n: (n, 0), "fetches": lambda n: (0, n), "mixed": lambda n: ((n + 1) // 2, n // 2)}


@pytest.mark.parametrize("tab", [False, True], ids=["moves-by-pointer", "moves-in-kernel-arguments"])
@pytest.mark.parametrize("n,kind", [(1, "stores"), (1, "fetches"), (37, "stores"), (37, "fetches"), (37, "mixed")])
@pytest.mark.parametrize("rf", [5, 3380, 8970, 32000, 88200])
def test_one_pair_moves_exactly_the_named_rows(lib, rf, n, kind, tab):
    rng = np.random.default_rng(rf + n)
    n_store, n_fetch = LISTS[kind](n)
    _run(lib, [(Arr(N_ROWS, rf, 0, 1), Arr(N_SLOTS, rf, 0, 2))], _moves(n_store, n_fetch, rng), n_store, n_fetch, tab)


@pytest.mark.parametrize("tab", [False, True], ids=["moves-by-pointer", "moves-in-kernel-arguments"])
@pytest.mark.parametrize("kind", list(LISTS))
@pytest.mark.parametrize("rfs", [(3380, 32000), (8970, 88200), (5, 3380)], ids=["16k", "44k", "scalar-and-vector"])
def test_two_pairs_with_different_row_sizes_in_one_launch(lib, rfs, kind, tab):
    rng = np.random.default_rng(sum(rfs))
    n_store, n_fetch = LISTS[kind](37)
    pairs = [(Arr(N_ROWS, rf, 0, 3 + k), Arr(N_SLOTS, rf, 0, 5 + k)) for k, rf in enumerate(rfs)]
    _run(lib, pairs, _moves(n_store, n_fetch, rng), n_store, n_fetch, tab)


@pytest.mark.parametrize("offs", [(4, 4), (8, 8), (0, 4), (8, 0), (4, 8)], ids=lambda o: f"out+{o[0]}-pool+{o[1]}")
@pytest.mark.parametrize("rf", [3380, 8970, 5])
def test_bases_off_16_byte_alignment_take_the_narrower_access(lib, rf, offs):
    rng = np.random.default_rng(rf + 16 * offs[0] + offs[1])
    n_store, n_fetch = LISTS["mixed"](37)
    _run(lib, [(Arr(N_ROWS, rf, offs[0], 7), Arr(N_SLOTS, rf, offs[1], 8))], _moves(n_store, n_fetch, rng), n_store, n_fetch, False)


def test_no_moves_touch_nothing(lib):
    o, p = Arr(N_ROWS, 3380, 0, 9), Arr(N_SLOTS, 3380, 0, 10)
    _run(lib, [(o, p)], np.zeros((1, 2), np.int32), 0, 0, False)
