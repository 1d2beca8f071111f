"""The one-pass scatter of the half-precision time-domain rows (k_scatter_rows16_max, ss_kernels.hpp) on the host-compiled
kernels (tests/scatter_rows16_max_host.cpp on the host-sim fibers): byte for byte what k_scatter_rows16 writes, and both the numpy
rule (tests/rir16_ref.py).

Capacities 2, 510, 512, 514, 1026, 16000 (below, on and just past a chunk of 512 frames, several chunks); per capacity rows of
0, 1, 2, 511, 512, 513, cap - 1, cap frames and one whose length lies above cap (clamped); rows of zeros, rows with one silent ear,
the maximum on the last kept frame, a maximum of exactly 1.0 and of exactly 2^-20 (frexp's boundary: 2^(e-1) <= mx < 2^e).  The
staging block behind every row's length is poison (NaN and 1e30 in turn): frames at or behind the length are never read.  Slots are
non-contiguous and descending; the bank is pre-filled with a byte pattern and the entries not named keep it.  Staging: rows 2 cap
floats apart from a 16-byte aligned base (the 16-byte loads), rows 2 cap + 6 apart and a base that is only 8-byte aligned (the
8-byte loads).  A row_max that is NOT the rows' maxima (NaN, inf, negative, far too small, far too large) leaves every other entry
and the lengths as they are."""
import ctypes

import numpy as np
import pytest

import rir16_ref as R
hs = pytest.importorskip("hostsim.hs")

CAPS = (2, 510, 512, 514, 1026, 16000)
PATTERN = 0xA5


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = hs.build_driver("scatter_rows16_max", tmp_path_factory.mktemp("scatter_rows16_max"))
    lib = ctypes.CDLL(so)
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.hs_scatter_rows16.argtypes = [vp, ll, vp, vp, ci, vp, vp, ci, vp]
    lib.hs_scatter_rows16_max.argtypes = [vp, ll, vp, vp, vp, ci, vp, vp, ci, vp]
    return lib


def make_rows(cap, seed=0):
    """-> (rows [n, cap, 2] wav layout, zero behind each length; lens [n] as handed to the kernels; kept [n] = the clamped lengths)"""
    rng = np.random.default_rng(1000 + cap + seed)
    rows, lens = [], []

    def add(ln, fill):
        k = min(max(ln, 0), cap)
        r = np.zeros((cap, 2), np.float32)
        if k:
            r[:k] = fill(k)
        rows.append(r)
        lens.append(ln)

    rand = lambda k: (rng.standard_normal((k, 2)) * 10.0 ** rng.integers(-6, 5)).astype(np.float32)      # noqa: E731
    for ln in sorted({0, 1, 2, 511, 512, 513, cap - 1, cap} | {cap + 7}):
        if ln <= cap or ln == cap + 7:
            add(ln, rand)
    full = cap
    add(full, lambda k: np.zeros((k, 2), np.float32))                                     # all-zero
    add(full, lambda k: rand(k) * np.asarray([1.0, 0.0], np.float32))                     # ear 1 silent
    add(full, lambda k: rand(k) * np.asarray([0.0, 1.0], np.float32))                     # ear 0 silent

    def last_peak(k):
        r = rng.uniform(-1, 1, (k, 2)).astype(np.float32)
        r[k - 1] = [-3.0, 5.0]                                                            # the maximum on the last kept frame
        return r
    add(full, last_peak)
    add(max(cap - 1, 1), last_peak)

    def exact(peak):
        def f(k):
            r = (rng.uniform(-1, 1, (k, 2)) * peak * 0.999).astype(np.float32)
            r[rng.integers(0, k)] = [peak, -peak]
            return r
        return f
    add(full, exact(np.float32(1.0)))                                                     # mx = 2^0: e = 1
    add(full, exact(np.float32(2.0 ** -20)))                                              # mx = 2^-20: e = -19
    return np.stack(rows), np.asarray(lens, np.int32), np.minimum(np.maximum(np.asarray(lens), 0), cap)


def stage(rows, kept, stride, offset):
    """the rows in a staging block of `stride` floats per row starting `offset` floats into a 16-byte aligned buffer, poison behind
    every row's length and between the rows"""
    n, cap = rows.shape[0], rows.shape[1]
    buf = np.empty((n * stride + offset + 4,), np.float32)
    base = (-buf.ctypes.data // 4) % 4                                                    # floats up to the next 16-byte boundary
    buf[0::2] = np.nan
    buf[1::2] = 1e30
    view = buf[base + offset: base + offset + n * stride].reshape(n, stride)
    for i in range(n):
        view[i, :2 * kept[i]] = rows[i, :kept[i]].reshape(-1)
    assert (view.ctypes.data % 16 == 0) == (offset % 4 == 0)
    return buf, view


def reference(rows, kept):
    planar = np.ascontiguousarray(rows.transpose(0, 2, 1))                                # [n, 2, cap], zero behind the lengths
    q, s = R.quantise(planar)
    return np.ascontiguousarray(q), np.ascontiguousarray(s, np.float32)


def run(lib, which, view, stride, slots, lens, row_max, cap, entries):
    q = np.full((entries, 2, cap), 0, np.float16)
    q.view(np.uint8)[...] = PATTERN
    s = np.empty((entries, 2), np.float32)
    s.view(np.uint8)[...] = PATTERN
    bl = np.empty((entries,), np.int32)
    bl.view(np.uint8)[...] = PATTERN
    n = len(slots)
    if which == "max":
        rc = lib.hs_scatter_rows16_max(view.ctypes.data, stride, slots.ctypes.data, lens.ctypes.data, row_max.ctypes.data, n,
                                       q.ctypes.data, s.ctypes.data, cap, bl.ctypes.data)
    else:
        rc = lib.hs_scatter_rows16(view.ctypes.data, stride, slots.ctypes.data, lens.ctypes.data, n, q.ctypes.data, s.ctypes.data, cap,
                                   bl.ctypes.data)
    assert rc == 0, rc
    return q, s, bl


@pytest.mark.parametrize("layout", ["aligned16", "stride_plus_6", "base_plus_2"])
@pytest.mark.parametrize("cap", CAPS)
def test_one_pass_scatter_equals_the_two_pass_kernel_and_numpy(lib, cap, layout):
    rows, lens, kept = make_rows(cap)
    n = rows.shape[0]
    stride, offset = {"aligned16": (2 * cap, 0), "stride_plus_6": (2 * cap + 6, 0), "base_plus_2": (2 * cap, 2)}[layout]
    buf, view = stage(rows, kept, stride, offset)
    slots = (3 * np.arange(n)[::-1] + 1).astype(np.int32)                                 # non-contiguous, descending
    entries = int(slots.max()) + 3
    row_max = np.zeros((n, 2), np.float32)
    for i in range(n):
        if kept[i]:
            row_max[i] = np.abs(rows[i, :kept[i]]).max(0)
    want_q, want_s = reference(rows, kept)
    got = {w: run(lib, w, view, stride, slots, lens, row_max, cap, entries) for w in ("max", "two_pass")}
    for w, (q, s, bl) in got.items():
        for i in range(n):
            assert q[slots[i]].tobytes() == want_q[i].tobytes(), (w, cap, layout, i, int(lens[i]))
            assert s[slots[i]].tobytes() == want_s[i].tobytes(), (w, cap, layout, i, int(lens[i]))
            assert bl[slots[i]] == kept[i], (w, i)
        others = np.setdiff1d(np.arange(entries), slots)
        assert (q[others].view(np.uint8) == PATTERN).all() and (s[others].view(np.uint8) == PATTERN).all()
        assert (bl[others].view(np.uint8) == PATTERN).all()
    for a, b in zip(got["max"], got["two_pass"]):
        assert a.tobytes() == b.tobytes()
    # the special rows did what they are there for
    zero_row = int(np.flatnonzero((np.abs(rows).max((1, 2)) == 0) & (kept == cap))[0])
    assert not got["max"][0][slots[zero_row]].view(np.uint16).any() and (got["max"][1][slots[zero_row]] == 1.0).all()
    one = int(np.flatnonzero((row_max == 1.0).all(1))[0])
    tiny = int(np.flatnonzero((row_max == np.float32(2.0 ** -20)).all(1))[0])
    assert (got["max"][1][slots[one]] == 2.0 ** -14).all() and (got["max"][1][slots[tiny]] == 2.0 ** -34).all()
    assert np.abs(got["max"][0][slots[one]].astype(np.float32)).max() == 16384.0


@pytest.mark.parametrize("cap", [514, 16000])
def test_bank_len_may_be_null_and_a_second_launch_overwrites(lib, cap):
    rows, lens, kept = make_rows(cap, seed=1)
    n = rows.shape[0]
    buf, view = stage(rows, kept, 2 * cap, 0)
    slots = np.arange(n, dtype=np.int32)
    row_max = np.stack([np.abs(rows[i, :kept[i]]).max(0) if kept[i] else np.zeros(2, np.float32) for i in range(n)]).astype(np.float32)
    want_q, want_s = reference(rows, kept)
    q = np.full((n, 2, cap), 3.0, np.float16)                                             # an entry that held a longer row before
    s = np.full((n, 2), 9.0, np.float32)
    assert lib.hs_scatter_rows16_max(view.ctypes.data, 2 * cap, slots.ctypes.data, lens.ctypes.data, row_max.ctypes.data, n,
                                     q.ctypes.data, s.ctypes.data, cap, None) == 0
    assert q.tobytes() == want_q.tobytes() and s.tobytes() == want_s.tobytes()              # +0 halves behind every length


@pytest.mark.parametrize("cap", [2, 514, 1026])
def test_a_wrong_row_max_stays_inside_the_rows_own_entries(lib, cap):
    rows, lens, kept = make_rows(cap, seed=2)
    n = rows.shape[0]
    buf, view = stage(rows, kept, 2 * cap + 6, 0)
    before = buf.copy()
    slots = (2 * np.arange(n)[::-1] + 1).astype(np.int32)
    entries = int(slots.max()) + 2
    bad = np.resize(np.asarray([np.nan, np.inf, -1.0, 1e-38, 3e38, -np.inf, 0.0, 1e-45], np.float32), (n, 2)).copy()
    q, s, bl = run(lib, "max", view, 2 * cap + 6, slots, lens, bad, cap, entries)
    others = np.setdiff1d(np.arange(entries), slots)
    assert (q[others].view(np.uint8) == PATTERN).all() and (s[others].view(np.uint8) == PATTERN).all()
    assert (bl[others].view(np.uint8) == PATTERN).all() and bl[slots].tolist() == kept.tolist()
    assert buf.tobytes() == before.tobytes()                                              # the staging block is only read
