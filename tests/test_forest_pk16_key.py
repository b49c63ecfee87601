"""forest_common.h's 16-bit subtree sort key (pk16_key: bin in bits 5-12, class in bit 4,
bootstrap weight in bits 0-3) and the packed scan word of the sorted rows (all weight in bits
0-15, class 1's in bits 16-31), through the host runtime's exports of the same text the HIP
kernels compile.  Two such keys share one register in the subtree tier's packed sorts, so a
key must stay below 0xFFFF (an absent row) and a 64-row node's sums inside 16 bits."""
import ctypes

import numpy as np

from cs230_distributed_machine_learning_amd.utils import native


def _lib():
    lib = native.cpu_lib()
    lib.dml_pk16_key.restype = ctypes.c_uint32
    lib.dml_pk16_key.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32]
    lib.dml_pk16_fields.restype = None
    lib.dml_pk16_fields.argtypes = [ctypes.c_uint32, ctypes.c_void_p]
    lib.dml_pk16_scan_word.restype = ctypes.c_uint32
    lib.dml_pk16_scan_word.argtypes = [ctypes.c_int32, ctypes.c_uint32]
    lib.dml_pk16_limits.restype = None
    lib.dml_pk16_limits.argtypes = [ctypes.c_void_p]
    return lib


def _limits(lib):
    lim = np.zeros(3, dtype=np.int32)
    lib.dml_pk16_limits(lim.ctypes.data)
    return tuple(int(x) for x in lim)


def _fields(lib, k):
    out = np.zeros(3, dtype=np.uint32)
    lib.dml_pk16_fields(ctypes.c_uint32(k), out.ctypes.data)
    return tuple(int(x) for x in out)


def test_pk16_limits():
    rows, absent, pois = _limits(_lib())
    assert (rows, absent, pois) == (64, 0xFFFF, 12)


def test_pk16_key_is_13_bits_and_round_trips():
    lib = _lib()
    _, absent, pois = _limits(lib)
    top = lib.dml_pk16_key(255, 1, pois)            # the largest bin, class 1, the largest weight
    assert top == (255 << 5 | 1 << 4 | 12) and top < (1 << 13) and top < absent
    assert lib.dml_pk16_key(255, 1, 15) < absent    # and the largest weight the row word can carry
    for b in (0, 1, 77, 254, 255):
        for cls in (0, 1):
            for w in (0, 1, 7, pois, 15):
                k = lib.dml_pk16_key(b, cls, w)
                assert k < absent
                assert _fields(lib, k) == (b, cls, w)


def test_pk16_key_orders_by_bin_first():
    """Sorting the keys sorts the rows by bin: any key of bin b is below any key of bin b + 1,
    whatever the class and the weight."""
    lib = _lib()
    for b in (0, 100, 254):
        assert lib.dml_pk16_key(b, 1, 15) < lib.dml_pk16_key(b + 1, 0, 0)


def test_pk16_scan_fields_hold_a_full_node():
    """64 rows of weight 12 (and of 15, the row word's largest): the running sum of the scan
    words keeps the all-class weight in bits 0-15 and class 1's in bits 16-31 with no carry."""
    lib = _lib()
    rows, _, pois = _limits(lib)
    for w in (pois, 15):
        for ncls1 in (0, 1, 32, 63, 64):
            acc = 0
            for i in range(rows):
                acc += lib.dml_pk16_scan_word(1 if i < ncls1 else 0, w)
                assert acc < (1 << 32)
            assert acc & 0xFFFF == rows * w and acc >> 16 == ncls1 * w
            assert (acc & 0xFFFF) - (acc >> 16) == (rows - ncls1) * w
