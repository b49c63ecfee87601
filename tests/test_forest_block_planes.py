"""forest_common.h's dword-plane layout of the block tier's bin stash (stash_plane_base /
stash_plane_byte) through the host runtime's exports of the same text the HIP kernels compile.
A block-tier node owns bytes [16 start, 16 (start + cnt)) of the scratch; the bins of visiting
positions q < g <= 16 of row position p live in byte q & 3 of word p of plane q >> 2.  Checked
here, where a wrong address costs nothing: every (p, q) has a byte of its own, inside the node's
range, and every plane starts on a word."""
import ctypes

import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.utils import native

COUNTS = (1, 255, 256, 257, 6001, 65536)
STARTS = (0, 1, 257, 1_265_003, (1 << 31) + 12345)   # the last: byte offsets past 2^35


def _lib():
    lib = native.cpu_lib()
    lib.dml_stash_planes.restype = ctypes.c_int32
    lib.dml_stash_planes.argtypes = [ctypes.c_int32]
    lib.dml_stash_plane_base.restype = ctypes.c_int64
    lib.dml_stash_plane_base.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    lib.dml_stash_plane_bytes.restype = None
    lib.dml_stash_plane_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    return lib


def test_plane_count():
    lib = _lib()
    for g in range(1, 17):
        assert lib.dml_stash_planes(g) == (g + 3) // 4
    assert lib.dml_stash_planes(20) == 4          # a wider group stashes its first 16 positions


@pytest.mark.parametrize("cnt", COUNTS)
def test_planes_tile_the_node_range(cnt):
    lib = _lib()
    for start in STARTS:
        lo, hi = 16 * start, 16 * (start + cnt)
        for g in range(1, 17):
            planes = lib.dml_stash_planes(g)
            bases = [lib.dml_stash_plane_base(start, cnt, w) for w in range(planes)]
            assert all(b % 4 == 0 for b in bases)
            assert bases == [lo + 4 * cnt * w for w in range(planes)]
            out = np.empty(cnt * g, dtype=np.int64)
            lib.dml_stash_plane_bytes(start, cnt, g, out.ctypes.data)
            assert out.min() >= lo and out.max() < hi
            # distinct bytes: no byte of the range is named twice
            assert np.bincount(out - lo, minlength=16 * cnt).max() == 1
            # (p, q) sits in byte q & 3 of word p of plane q >> 2
            pq = out.reshape(cnt, g)
            q = np.arange(g)
            assert np.array_equal(pq[0], np.asarray(bases)[q >> 2] + (q & 3))
            assert np.array_equal(pq - pq[0], np.broadcast_to(4 * np.arange(cnt, dtype=np.int64)[:, None], (cnt, g)))
        # g = 16 fills the range exactly
        out = np.empty(cnt * 16, dtype=np.int64)
        lib.dml_stash_plane_bytes(STARTS[1], cnt, 16, out.ctypes.data)
        assert np.array_equal(np.sort(out), np.arange(16 * STARTS[1], 16 * (STARTS[1] + cnt)))
