"""ss_memo_rows_f32 (include/ss_hip.h "Pose memo on the column path"): every refusal is SS_EINVAL (-1) from the argument
checks, before a device is touched (this file runs without a GPU: a call that got past the checks would come back with a HIP
error, not -1), and a list without moves returns 0 without a launch.  ``ops.memo_rows_`` refuses what it can see in Python."""
import ctypes

import pytest
import torch

from ss_amd import _lib, ops

ONE = 4096                          # non-null, 16-byte aligned dummy pointers: never dereferenced on these paths
TWO = 8192
MOVES = 12288
ODD = 4098                          # not 4-byte aligned


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _io(*rows):
    arr = (_lib.SsMemoIo * max(1, len(rows)))()
    for k, (out, pool, rf) in enumerate(rows):
        arr[k] = _lib.SsMemoIo(out, pool, rf, 0)
    return ctypes.cast(arr, ctypes.c_void_p), arr


GOOD = (ONE, TWO, 3380)


@pytest.mark.parametrize("label,rows,n_io,moves,n_store,n_fetch", [
    ("n_io 0", [GOOD], 0, MOVES, 1, 1),
    ("n_io 5", [GOOD] * 5, 5, MOVES, 1, 1),
    ("negative n_io", [GOOD], -1, MOVES, 1, 1),
    ("null out", [(None, TWO, 3380)], 1, MOVES, 1, 0),
    ("null pool", [(ONE, None, 3380)], 1, MOVES, 0, 1),
    ("null pool in the second pair", [GOOD, (ONE, None, 32000)], 2, MOVES, 1, 1),
    ("null moves", [GOOD], 1, None, 1, 1),
    ("row_floats 0", [(ONE, TWO, 0)], 1, MOVES, 1, 1),
    ("row_floats negative", [(ONE, TWO, -4)], 1, MOVES, 1, 1),
    ("row_floats 0 in the fourth pair", [GOOD, GOOD, GOOD, (ONE, TWO, 0)], 4, MOVES, 1, 1),
    ("out not 4-byte aligned", [(ODD, TWO, 3380)], 1, MOVES, 1, 1),
    ("pool not 4-byte aligned", [(ONE, ODD + 1, 3380)], 1, MOVES, 1, 1),
    ("negative n_store", [GOOD], 1, MOVES, -1, 2),
    ("negative n_fetch", [GOOD], 1, MOVES, 2, -1),
    ("counts that overflow", [GOOD], 1, MOVES, 0x7fffffff, 1),
], ids=lambda v: v if isinstance(v, str) else None)
def test_refusals_are_einval_before_a_device_is_touched(lib, label, rows, n_io, moves, n_store, n_fetch):
    p, keep = _io(*rows)
    assert lib.ss_memo_rows_f32(p, n_io, moves, n_store, n_fetch, None) == -1, label


def test_null_io_with_moves_pending_is_einval(lib):
    assert lib.ss_memo_rows_f32(None, 1, MOVES, 1, 0, None) == -1


def test_no_moves_return_zero_without_a_launch(lib):
    p, keep = _io(GOOD)
    assert lib.ss_memo_rows_f32(p, 1, MOVES, 0, 0, None) == 0
    assert lib.ss_memo_rows_f32(p, 1, None, 0, 0, None) == 0            # nothing pending: nothing is looked at
    assert lib.ss_memo_rows_f32(None, 4, None, 0, 0, None) == 0
    assert lib.ss_memo_rows_f32(p, 0, MOVES, 0, 0, None) == -1          # ... but the counts themselves are


def test_python_op_refuses_host_tensors_and_bad_lists_before_the_library():
    out, pool = torch.zeros((4, 8)), torch.zeros((6, 8))
    mv = torch.zeros((2, 2), dtype=torch.int32)
    with pytest.raises(_lib.SsHipError):                                  # CPU tensors: this path has no CPU implementation
        ops.memo_rows_([(out, pool)], mv, 1, 1)
    with pytest.raises(ValueError):
        ops.memo_rows_([], mv, 0, 0)
    with pytest.raises(ValueError):
        ops.memo_rows_([(out, pool)] * 5, mv, 0, 0)
