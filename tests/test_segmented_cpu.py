"""CPU: the host side of the segmented sort -- argument validation, class
bounds, temporary-buffer sizing -- through ctypes with null device pointers
(no device call is made), and the C++ header's new methods."""
import ctypes
import os
import subprocess

import pytest

import tinyhipradixsort_amd as T

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEY_BYTES = {0: 4, 1: 8, 2: 4, 3: 8}
VALUE_BYTES = {0: 4, 1: 8, 2: 16}
HEADER_BYTES = 16640      # the temporary buffer's header (error word, class counts)


def seg_bytes(kt, vt, n, ns, pairs):
    out = ctypes.c_uint64()
    cfg = T._CConfig(1, kt, vt, 0)
    assert T.lib().thrs_get_segmented_temporary_bytes(ctypes.byref(cfg), n, ns, int(pairs), ctypes.byref(out)) == 0
    return int(out.value)


def test_argument_validation_needs_no_device():
    L = T.lib()
    cfg = T._CConfig(1, 0, 0, 0)
    c = ctypes.byref(cfg)
    keys_fn, pairs_fn = L.thrs_sort_segments_keys, L.thrs_sort_segments_pairs
    # bad bit range -> THRS_ERROR_BIT_RANGE, before any HIP call
    assert keys_fn(c, None, 10, None, 3, None, 0, 31, None) == -2
    assert pairs_fn(c, None, None, 10, None, 3, None, 3, 8, None) == -2
    # n == 0, numSegments == 0, an empty window, a window wholly past the key width: no-ops
    assert keys_fn(c, None, 0, None, 3, None, 0, 32, None) == 0
    assert keys_fn(c, None, 10, None, 0, None, 0, 32, None) == 0
    assert keys_fn(c, None, 10, None, 3, None, 16, 16, None) == 0
    assert keys_fn(c, None, 10, None, 3, None, 40, 32, None) == 0
    assert keys_fn(c, None, 10, None, 3, None, 32, 64, None) == 0
    assert pairs_fn(c, None, None, 0, None, 3, None, 0, 32, None) == 0
    assert pairs_fn(c, None, None, 10, None, 3, None, 32, 64, None) == 0
    # bad enums, null config / keys / offsets / temp / values, negative startBits
    for bad in (T._CConfig(1, 9, 0, 0), T._CConfig(1, -1, 0, 0), T._CConfig(1, 0, 0, 2)):
        assert keys_fn(ctypes.byref(bad), None, 10, None, 3, None, 0, 32, None) == -1
    assert pairs_fn(ctypes.byref(T._CConfig(1, 0, 7, 0)), None, None, 10, None, 3, None, 0, 32, None) == -1
    assert keys_fn(ctypes.byref(T._CConfig(1, 0, 7, 0)), None, 10, None, 3, None, 16, 16, None) == 0  # keys: value type unused
    assert keys_fn(None, None, 10, None, 3, None, 0, 32, None) == -1
    assert keys_fn(c, None, 10, None, 3, None, -8, 32, None) == -1
    fake = ctypes.c_void_p(4096)     # never dereferenced: a null among the others is refused first
    assert keys_fn(c, None, 10, fake, 3, fake, 0, 32, None) == -1        # keys
    assert keys_fn(c, fake, 10, None, 3, fake, 0, 32, None) == -1        # offsets
    assert keys_fn(c, fake, 10, fake, 3, None, 0, 32, None) == -1        # temporary buffer
    assert pairs_fn(c, fake, None, 10, fake, 3, fake, 0, 32, None) == -1  # values
    with pytest.raises(T.ThrsError) as e:
        T.RadixSort([], T.RadixSort.Config()).sortKeysSegmented(0, 10, 0, 3, 0, 0, 12, 0)
    assert e.value.status == -2


@pytest.mark.parametrize("kt", [0, 1, 2, 3])
@pytest.mark.parametrize("vb", [0, 4, 8, 16])
def test_segment_class_caps(kt, vb):
    c0, c1 = T.segment_class_caps(kt, vb)
    assert 0 < c0 < c1 and c1 >= 4096


def test_segment_class_caps_rejects_bad_enums():
    caps = (ctypes.c_uint32 * 2)()
    L = T.lib()
    assert L.thrs_segment_class_caps(4, 0, caps) == -1
    assert L.thrs_segment_class_caps(-1, 4, caps) == -1
    assert L.thrs_segment_class_caps(0, 2, caps) == -1
    assert L.thrs_segment_class_caps(0, 32, caps) == -1
    assert L.thrs_segment_class_caps(0, 4, None) == -1


@pytest.mark.parametrize("kt", [0, 1, 2, 3])
@pytest.mark.parametrize("vt", [0, 1, 2])
def test_segmented_temporary_bytes(kt, vt):
    kb, vb = KEY_BYTES[kt], VALUE_BYTES[vt]
    sizes = [0, 1, 1000, 99999, 1 << 20, 1 << 24]
    for pairs in (False, True):
        for ns in (1, 1000, 1 << 20):
            prev = 0
            for n in sizes:
                b = seg_bytes(kt, vt, n, ns, pairs)
                assert b > 0 and b % 16 == 0 and b >= prev          # non-decreasing in n
                prev = b
        for n in (1000, 1 << 20):
            prev = 0
            for ns in (0, 1, 77, 1000, 1 << 20, 1 << 24):
                b = seg_bytes(kt, vt, n, ns, pairs)
                assert b > 0 and b % 16 == 0 and b >= prev          # non-decreasing in numSegments
                prev = b
    for n, ns in ((1000, 10), (1 << 20, 1 << 20)):
        assert seg_bytes(kt, vt, n, ns, True) > seg_bytes(kt, vt, n, ns, False)
    n = ns = 1 << 20
    for pairs in (False, True):
        b = seg_bytes(kt, vt, n, ns, pairs)
        payload = n * (kb + (vb if pairs else 0))
        assert b <= payload + 16 * ns + (1 << 20)
        # what the layout needs: the header, three u32 lists of numSegments
        # entries (one per size class, each rounded up to 256 bytes), keyOut
        # and valueOut (each rounded up to 16 bytes)
        assert b <= HEADER_BYTES + 3 * (4 * ns + 255) + payload + 48
        assert b >= HEADER_BYTES + 12 * ns + payload
    # pairs without a valid value type are refused; keys-only ignores it
    out = ctypes.c_uint64()
    bad = T._CConfig(1, kt, 9, 0)
    assert T.lib().thrs_get_segmented_temporary_bytes(ctypes.byref(bad), 10, 2, 1, ctypes.byref(out)) == -1
    assert T.lib().thrs_get_segmented_temporary_bytes(ctypes.byref(bad), 10, 2, 0, ctypes.byref(out)) == 0
    assert T.lib().thrs_get_segmented_temporary_bytes(None, 10, 2, 0, ctypes.byref(out)) == -1
    assert T.lib().thrs_get_segmented_temporary_bytes(ctypes.byref(T._CConfig(1, 5, 0, 0)), 10, 2, 0,
                                                      ctypes.byref(out)) == -1
    rs = T.RadixSort([], T.RadixSort.Config(keyType=T.KeyType(kt), valueType=T.ValueType(vt)))
    assert rs.getSegmentedTemporaryBufferBytes(1000, 10, True) == seg_bytes(kt, vt, 1000, 10, True)


# RadixSort.getTemporaryBufferBytes of the commit before the segmented sort,
# for the parametrised sizes of test_temporary_buffer_layout:
# (keyType, valueType, n) -> (pSumBuffer, keyOutBuffer, valueOutBuffer)
PARENT_TEMP = {
    (0, 0, 0): (2219008, 0, 0),
    (0, 0, 1): (2219264, 16, 16),
    (0, 0, 2047): (2221056, 8192, 8192),
    (0, 0, 2048): (2221056, 8192, 8192),
    (0, 0, 99999): (2380544, 400000, 400000),
    (0, 0, 1048576): (4211712, 4194304, 4194304),
    (0, 0, 2147483748): (2872911104, 8589934992, 8589934992),
    (1, 2, 0): (2223104, 0, 0),
    (1, 2, 1): (2223104, 16, 16),
    (1, 2, 2047): (2223104, 16384, 32752),
    (1, 2, 2048): (2223104, 16384, 32768),
    (1, 2, 99999): (2386944, 800000, 1599984),
    (1, 2, 1048576): (4238336, 8388608, 16777216),
    (1, 2, 2147483748): (1880957952, 17179869984, 34359739968),
    (2, 1, 0): (2219008, 0, 0),
    (2, 1, 1): (2219264, 16, 16),
    (2, 1, 2047): (2221056, 8192, 16384),
    (2, 1, 2048): (2221056, 8192, 16384),
    (2, 1, 99999): (2374400, 400000, 800000),
    (2, 1, 1048576): (4135936, 4194304, 8388608),
    (2, 1, 2147483748): (2872911104, 8589934992, 17179869984),
}


def test_existing_temporary_buffer_sizes_are_unchanged():
    assert T.ABI_VERSION == 7 and T.lib().thrs_abi_version() == 7
    for (kt, vt, n), want in PARENT_TEMP.items():
        cfg = T.RadixSort.Config(keyType=T.KeyType(kt), valueType=T.ValueType(vt))
        d = T.RadixSort([], cfg).getTemporaryBufferBytes(n)
        assert (d.pSumBuffer, d.keyOutBuffer, d.valueOutBuffer) == want, (kt, vt, n)


def test_header_with_segmented_methods_compiles_without_hip_headers(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(
        '#include <thrs/tinyhipradixsort.hpp>\n'
        'int main(int argc, char**) {\n'
        '  thrs::RadixSort::Config c; c.configureWithKeyPair<float, uint64_t>();\n'
        '  uint64_t (thrs::RadixSort::*size)(uint32_t, uint32_t, bool) const =\n'
        '      &thrs::RadixSort::getSegmentedTemporaryBufferBytes;\n'
        '  void (thrs::RadixSort::*keys)(void*, uint32_t, const uint32_t*, uint32_t, void*, int, int, oroStream) =\n'
        '      &thrs::RadixSort::sortKeysSegmented;\n'
        '  void (thrs::RadixSort::*pairs)(void*, void*, uint32_t, const uint32_t*, uint32_t, void*, int, int,\n'
        '                                 oroStream) = &thrs::RadixSort::sortPairsSegmented;\n'
        '  uint32_t caps[2];\n'
        '  int (*capsFn)(int, int, uint32_t*) = &thrs_segment_class_caps;\n'
        '  static_assert(THRS_ABI_VERSION == 7, "");\n'
        '  return (size && keys && pairs && capsFn && argc > 100) ? (int)caps[0] : 0;\n'
        '}\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
