"""Guarded device buffers for the kernel parity tests.

Every buffer a test hands to a kernel is one allocation: a front guard, the body, a back guard.  Output bodies start as
BODY_WORD (a NaN as fp32, an implausible index as int32), so an element the call under test never wrote cannot pass for the
right answer; output guards and the gap columns of an `ld > n` output hold GUARD_WORD, and `check()` asserts they are
bit-identical afterwards.  Input guards and gaps hold a quiet NaN, so a kernel that reads past its input and feeds the value into
arithmetic (even times a zero padding weight) produces a NaN; `check()` also asserts that every input body is unchanged.

The `guards` fixture turns the ctx debug poison on for the test (include/ssdseg.h `ssdseg_ctx_debug_poison`: fresh allocations and
every workspace / arena handout start as BODY_WORD), checks every guard at teardown and turns the poison off again.

The reporting functions at the top are pure NumPy so that the CPU suite can test them on hand-made arrays.
"""
import numpy as np
import pytest

BODY_WORD = 0x7FF0DEAD     # an output body element no kernel wrote (same word as the ctx poison)
GUARD_WORD = 0x7FBADBAD    # output guards and gap columns
INPUT_WORD = 0x7FC00000    # input guards and gap columns: the canonical quiet NaN
GUARD_UNIT = 64 << 10      # guards are multiples of this, so the body keeps the allocation's alignment
TILE_ROWS = 256            # the back guard covers at least one 256-row tile of the buffer's row pitch


def pattern_bytes(word: int, nbytes: int) -> np.ndarray:
    """`nbytes` bytes of the little-endian 32-bit `word` repeated from offset 0"""
    n = (nbytes + 3) // 4
    return np.full(n, word, np.uint32).view(np.uint8)[:nbytes]


def first_mismatch(got: np.ndarray, want: np.ndarray):
    """(offset of the first differing 32-bit word, number of differing words) of two equal-length byte arrays, or None.
    Words are counted from the start of the region; a trailing partial word counts as one."""
    got = np.asarray(got, np.uint8).ravel()
    want = np.asarray(want, np.uint8).ravel()
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    words = np.unique(bad // 4)
    return int(words[0]), int(words.size)


def gap_hits(body: np.ndarray, n: int, word: int):
    """indices (row, col) of the gap columns [n, ld) of a (rows, ld) array of 32-bit words that no longer hold `word`"""
    body = np.asarray(body).view(np.uint32)
    gap = body[:, n:]
    return [(int(r), int(c) + n) for r, c in np.argwhere(gap != np.uint32(word))]


def unwritten_indices(body: np.ndarray, word: int = BODY_WORD) -> np.ndarray:
    """indices (as from np.argwhere, in the array's own shape) of the elements whose bytes still equal the body pattern.
    4-byte elements are compared with `word`; 1-byte elements with the pattern byte at their offset."""
    body = np.ascontiguousarray(body)
    if body.dtype.itemsize == 4:
        return np.argwhere(body.view(np.uint32) == np.uint32(word))
    pat = pattern_bytes(word, body.nbytes).reshape(body.size, body.dtype.itemsize)
    raw = body.view(np.uint8).reshape(body.size, body.dtype.itemsize)
    hit = (raw == pat).all(axis=1).reshape(body.shape)
    return np.argwhere(hit)


def assert_finite_rows(table: np.ndarray, name: str = "table"):
    """every row of a partial-sum table [nparts][...] finite: an unwritten (poisoned) row is reported as such, not as a
    tolerance miss of the folded sums"""
    t = np.asarray(table)
    bad = np.flatnonzero(~np.isfinite(t.reshape(t.shape[0], -1)).all(axis=1))
    assert bad.size == 0, f"{name}: {bad.size} of {t.shape[0]} partial rows not finite (first: row {int(bad[0])})"


def _rows_cols(shape):
    shape = tuple(int(s) for s in shape)
    if len(shape) == 0:
        return 1, 1
    return int(np.prod(shape[:-1])) if len(shape) > 1 else 1, shape[-1]


class _Alloc:
    """one guarded allocation: front guard | body (rows x ld elements) | back guard"""

    def __init__(self, name, whole, front, body_bytes, back, rows, cols, ld, itemsize, kind, guard_word, body_host=None):
        self.name, self.whole = name, whole
        self.front, self.body_bytes, self.back = front, body_bytes, back
        self.rows, self.cols, self.ld, self.itemsize = rows, cols, ld, itemsize
        self.kind, self.guard_word = kind, guard_word
        self.body_host = body_host      # inputs: the bytes the body must still hold

    def region(self, offset, nbytes):
        return self.whole.ctx.borrow(self.whole.ptr + offset, (nbytes,), np.uint8, owner=self.whole).download()


def _make_buffer_class():
    from ssdseglib import _hip as H

    class GuardedBuffer(H.DeviceBuffer):
        """the body of a guarded allocation; with a row pitch `ld` > the last dimension, download / upload move only the
        logical columns and leave the gaps alone"""

        def __init__(self, ctx, shape, dtype, ptr, owner, alloc):
            super().__init__(ctx, shape, dtype, ptr=ptr, owner=owner)
            self.alloc = alloc
            self.nbytes = alloc.body_bytes      # views may reach into the pitched body

        def _pitched(self):
            return self.alloc.ld != self.alloc.cols

        def download(self):
            if not self._pitched():
                return super().download()
            a = self.alloc
            raw = a.region(a.front, a.body_bytes).view(self.dtype).reshape(a.rows, a.ld)
            return raw[:, :a.cols].reshape(self.shape).copy()

        def upload(self, array):
            if not self._pitched():
                return super().upload(array)
            a = self.alloc
            raw = a.region(a.front, a.body_bytes).view(self.dtype).reshape(a.rows, a.ld).copy()
            raw[:, :a.cols] = np.asarray(array, self.dtype).reshape(a.rows, a.cols)
            self.ctx.borrow(self.ptr, raw.shape, self.dtype, owner=self).upload(raw)
            return self

    return GuardedBuffer


class Guards:
    """guarded inputs and outputs of one test (see the module docstring)"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.allocs = []
        self._cls = _make_buffer_class()

    # ---- allocation
    def _alloc(self, shape, dtype, ld, kind, name):
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        rows, cols = _rows_cols(shape)
        ld = cols if ld is None else int(ld)
        assert ld >= cols, (ld, cols)
        pitch = ld * dtype.itemsize
        body_bytes = rows * pitch if shape else dtype.itemsize
        front = GUARD_UNIT
        back = max(GUARD_UNIT, -(-(TILE_ROWS * pitch) // GUARD_UNIT) * GUARD_UNIT)
        whole = self.ctx.empty((front + body_bytes + back,), np.uint8)
        guard_word = GUARD_WORD if kind == "out" else INPUT_WORD
        if name is None:
            name = f"{kind}[{len(self.allocs)}] {shape} {dtype.name}" + (f" ld={ld}" if ld != cols else "")
        a = _Alloc(name, whole, front, body_bytes, back, rows, cols, ld, dtype.itemsize, kind, guard_word)
        buf = self._cls(self.ctx, shape, dtype, whole.ptr + front, whole, a)
        self._fill(a, 0, pattern_bytes(guard_word, front))
        self._fill(a, front + body_bytes, pattern_bytes(guard_word, back))
        self.allocs.append(a)
        return a, buf

    def _fill(self, a, offset, data):
        self.ctx.borrow(a.whole.ptr + offset, (data.size,), np.uint8, owner=a.whole).upload(data)

    def _body_pattern(self, a):
        """the bytes of a poisoned output body: BODY_WORD, GUARD_WORD in the gap columns"""
        body = pattern_bytes(BODY_WORD, a.body_bytes)
        if a.ld != a.cols:
            words = body.copy().view(np.uint32).reshape(a.rows, a.ld)
            words[:, a.cols:] = GUARD_WORD
            body = words.view(np.uint8).ravel()
        return body

    def out(self, shape, dtype=np.float32, ld=None, name=None):
        """an output: body = BODY_WORD, guards and gap columns = GUARD_WORD"""
        a, buf = self._alloc(shape, dtype, ld, "out", name)
        assert a.ld == a.cols or a.itemsize == 4, "row pitch gaps need 4-byte elements"
        if a.ld != a.cols or not self.ctx.poison:
            self._fill(a, a.front, self._body_pattern(a))
        return buf

    def zeros(self, shape, dtype=np.float32, ld=None, name=None):
        """an output that an accumulate-mode call adds into: a guarded body that starts at zero"""
        buf = self.out(shape, dtype, ld, name)
        return buf.upload(np.zeros(buf.shape, buf.dtype))

    def inp(self, array, ld=None, dtype=None, name=None):
        """an input: the body holds `array` (its gap columns a quiet NaN), the guards a quiet NaN; the host copy is kept"""
        arr = np.ascontiguousarray(array if dtype is None else np.asarray(array, dtype))
        a, buf = self._alloc(arr.shape, arr.dtype, ld, "inp", name)
        if a.ld != a.cols:
            assert a.itemsize == 4, "row pitch gaps need 4-byte elements"
            body = np.full((a.rows, a.ld), INPUT_WORD, np.uint32)
            body[:, :a.cols] = arr.reshape(a.rows, a.cols).view(np.uint32)
            host = body.view(np.uint8).ravel()
        else:
            host = arr.view(np.uint8).ravel().copy()
        a.body_host = host
        self._fill(a, a.front, host)
        return buf

    def repoison(self, buf):
        """refill the body of an output with BODY_WORD before an overwrite-mode call reuses it"""
        a = buf.alloc
        assert a.kind == "out", f"{a.name} is an input"
        self._fill(a, a.front, self._body_pattern(a))
        return buf

    # ---- checks
    def unwritten(self, buf) -> np.ndarray:
        """indices (in the buffer's shape) of the body elements that still hold BODY_WORD"""
        return unwritten_indices(buf.download())

    def check(self):
        """every guard and gap bit-identical, every input body unchanged; names the buffer, the side and the first offset"""
        problems = []
        for a in self.allocs:
            for side, off, size in (("front", 0, a.front), ("back", a.front + a.body_bytes, a.back)):
                hit = first_mismatch(a.region(off, size), pattern_bytes(a.guard_word, size))
                if hit:
                    problems.append(f"{a.name}: {side} guard written at word offset {hit[0]} ({hit[1]} words)")
            if a.kind == "inp":
                hit = first_mismatch(a.region(a.front, a.body_bytes), a.body_host)
                if hit:
                    problems.append(f"{a.name}: input body changed at word offset {hit[0]} ({hit[1]} words)")
            elif a.ld != a.cols:
                body = a.region(a.front, a.body_bytes).view(np.uint32).reshape(a.rows, a.ld)
                hits = gap_hits(body, a.cols, GUARD_WORD)
                if hits:
                    problems.append(f"{a.name}: gap written at (row, col) {hits[0]} ({len(hits)} words)")
        assert not problems, "guard check failed:\n  " + "\n  ".join(problems)

    def release(self):
        self.allocs.clear()


@pytest.fixture
def guards(ctx):
    """Guards for one test, with the ctx debug poison on for its duration; every guard is checked at teardown"""
    ctx.debug_poison(True)
    g = Guards(ctx)
    try:
        yield g
        ctx.sync()
        g.check()
    finally:
        ctx.debug_poison(False)
        g.release()


@pytest.fixture(scope="module")
def poisoned_ctx(ctx):
    """the session ctx with the debug poison on for a whole module (engine-level tests: every activation, stats table and
    workspace region starts as NaN)"""
    ctx.debug_poison(True)
    try:
        yield ctx
    finally:
        ctx.debug_poison(False)
