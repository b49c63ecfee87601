"""forest_common.h's narrow binary histogram word (pack_bin32: class-0 weight in bits 0-11,
class-1 weight in bits 12-23, rows in bits 24-31) through the host runtime's exports of the
same text the HIP kernels compile.  The overflow corner -- 255 rows of the largest weight the
row word can carry in ONE bin for each class -- cannot be produced on the GPU (Poisson
weights stop at 12), so it is checked here."""
import ctypes

import numpy as np

from cs230_distributed_machine_learning_amd.utils import native


def _lib():
    lib = native.cpu_lib()
    lib.dml_pack_bin32.restype = ctypes.c_uint32
    lib.dml_pack_bin32.argtypes = [ctypes.c_int32, ctypes.c_uint32]
    lib.dml_bin32_fields.restype = None
    lib.dml_bin32_fields.argtypes = [ctypes.c_uint32, ctypes.c_void_p]
    lib.dml_pack32_limits.restype = None
    lib.dml_pack32_limits.argtypes = [ctypes.c_void_p]
    return lib


def _fields(lib, v):
    out = np.zeros(3, dtype=np.uint32)
    lib.dml_bin32_fields(ctypes.c_uint32(v), out.ctypes.data)
    return tuple(int(x) for x in out)


def test_pack32_limits():
    lib = _lib()
    lim = np.zeros(3, dtype=np.int32)
    lib.dml_pack32_limits(lim.ctypes.data)
    rows, wmax, pois = (int(x) for x in lim)
    assert (rows, wmax) == (255, 16)
    assert pois < wmax and wmax * rows < 4096 and rows < 256


def test_pack32_single_rows():
    lib = _lib()
    for w in (0, 1, 7, 12, 15, 16):
        assert _fields(lib, lib.dml_pack_bin32(0, w)) == (w, 0, 1)
        assert _fields(lib, lib.dml_pack_bin32(1, w)) == (0, w, 1)


def test_pack32_full_node_does_not_carry():
    """255 rows of weight 16 of one class in one bin: 4080 in that class's field, 255 rows;
    both classes' full sums in one word (the cumulative word of a scan) read 4080, 4080 and
    their row counts; one more word added to a full field's neighbours leaves the full field
    alone (no carry out of, or into, a field that is within its bound)."""
    lib = _lib()
    for cls in (0, 1):
        acc = 0
        for _ in range(255):
            acc = (acc + lib.dml_pack_bin32(cls, 16)) & 0xFFFFFFFF
        want = (4080, 0, 255) if cls == 0 else (0, 4080, 255)
        assert _fields(lib, acc) == want
    # each class's 255-row sum, as the three fields hold them side by side
    both = 4080 | (4080 << 12) | (255 << 24)
    assert _fields(lib, both) == (4080, 4080, 255)
    # a node's cumulative sums: 128 rows of class 0 and 127 of class 1, all of weight 16,
    # then one more word on top of a word whose class-0 field is full
    acc = 0
    for i in range(255):
        acc = (acc + lib.dml_pack_bin32(i & 1, 16)) & 0xFFFFFFFF
    assert _fields(lib, acc) == (128 * 16, 127 * 16, 255)
    full0 = 0
    for _ in range(254):
        full0 = (full0 + lib.dml_pack_bin32(0, 16)) & 0xFFFFFFFF
    assert _fields(lib, full0) == (254 * 16, 0, 254)
    nxt = (full0 + lib.dml_pack_bin32(1, 16)) & 0xFFFFFFFF       # the 255th row, other class
    assert _fields(lib, nxt) == (254 * 16, 16, 255)
    nxt = (full0 + lib.dml_pack_bin32(0, 16)) & 0xFFFFFFFF       # the 255th row, same class
    assert _fields(lib, nxt) == (4080, 0, 255)
