"""DecodeSet's two window sources on their own: what decode_windows / held_windows and their rows and span-rows forms
hand the C layer for a list of windows -- the argument list's head, with null pointers for empty tables, and the arrays
behind it in the types the C side reads.  numpy alone: no library is loaded and no device is touched."""
import numpy as np

from flake_amd import DecodeSet


def test_the_bytes_source_concatenates_the_runs():
    a, b = bytes(range(10, 17)), np.arange(40, 52, dtype=np.uint8)
    windows = [(a, [3, 4], 4096, 100, 50), (b, np.array([5, 5, 2]), 0, 2 ** 40, 7)]
    head, count, (fow, st, sizes, fixed, first) = DecodeSet._bytes_source(windows)
    assert fow.tolist() == [2, 3] and sizes.tolist() == [3, 4, 5, 5, 2]
    assert st.tobytes() == a + b.tobytes()
    assert fixed.tolist() == [4096, 0] and first.tolist() == [100, 2 ** 40] and count.tolist() == [50, 7]
    assert (fow.dtype, st.dtype, sizes.dtype) == (np.int32, np.uint8, np.int32)
    assert (fixed.dtype, first.dtype, count.dtype) == (np.uint32, np.uint64, np.int64)
    assert all(x.flags["C_CONTIGUOUS"] for x in (fow, st, sizes, fixed, first, count))
    assert head == (2, fow.ctypes.data, st.ctypes.data, 19, sizes.ctypes.data, fixed.ctypes.data, first.ctypes.data,
                    count.ctypes.data)


def test_the_bytes_source_of_no_windows_is_null_pointers():
    head, count, _ = DecodeSet._bytes_source([])
    assert head == (0, None, None, 0, None, None, None, None) and len(count) == 0 and count.dtype == np.int64
    # windows without a frame: their tables are there, the stream and the sizes are not
    head, count, (fow, st, sizes, _, _) = DecodeSet._bytes_source([(b"", [], 0, 0, 5)])
    assert head[0] == 1 and head[1] == fow.ctypes.data and head[2:5] == (None, 0, None) and fow.tolist() == [0]


def test_the_held_source():
    head, count, (ids, first) = DecodeSet._held_source([(3, 100, 50), (0, 2 ** 40, 7)])
    assert ids.tolist() == [3, 0] and first.tolist() == [100, 2 ** 40] and count.tolist() == [50, 7]
    assert (ids.dtype, first.dtype, count.dtype) == (np.int32, np.uint64, np.int64)
    assert head == (2, ids.ctypes.data, first.ctypes.data, count.ctypes.data)
    head, count, _ = DecodeSet._held_source([])
    assert head == (0, None, None, None) and len(count) == 0
