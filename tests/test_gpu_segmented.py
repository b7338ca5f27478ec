"""GPU: the segmented sort (sortKeysSegmented / sortPairsSegmented) against the
oracle run on every segment alone -- bit for bit, keys and values, every
segment of every case; nothing is sampled."""
import os
import subprocess

import numpy as np
import pytest

import cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KTS = [O.U32, O.U64, O.F32, O.F64]


def to_dev(torch, a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def from_dev(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def make_sorter(kt, vb, desc):
    import tinyhipradixsort_amd as T
    cfg = T.RadixSort.Config()
    cfg.keyType = T.KeyType(kt)
    cfg.valueType = {0: T.ValueType.U32, 4: T.ValueType.U32, 8: T.ValueType.U64, 16: T.ValueType.U128}[vb]
    cfg.sortOrder = T.SortOrder.Descending if desc else T.SortOrder.Ascending
    return T.RadixSort([], cfg)


def caps_of(kt, vb):
    import tinyhipradixsort_amd as T
    return T.segment_class_caps(kt, vb)


def boundary_sizes(kt, vb):
    c0, c1 = caps_of(kt, vb)
    return [0, 1, 2, 63, 64, 65, c0 - 1, c0, c0 + 1, 0, c1 - 1, c1, c1 + 1, 3 * c1 + 17]


def offsets_of(sizes, first=0):
    return (first + np.concatenate([[0], np.cumsum(np.asarray(sizes, np.uint64))])).astype(np.uint32)


def host_classes(kt, vb, offsets):
    c0, c1 = caps_of(kt, vb)
    sz = np.diff(offsets.astype(np.int64))
    return (int((sz <= 1).sum()), int(((sz > 1) & (sz <= c0)).sum()), int(((sz > c0) & (sz <= c1)).sum()),
            int((sz > c1).sum()))


def random_keys(kt, n, seed=0):
    return O.randomize_np(kt, O.splitmix64_stream(seed, n))


def expected(kt, keys, vals, offsets, start, end, desc, valid=None):
    """oracle.lsd_sort on each segment alone; the rest of the arrays as given"""
    ek = keys.copy()
    ev = None if vals is None else vals.copy()
    for s in range(offsets.shape[0] - 1):
        if valid is not None and not valid[s]:
            continue
        a, b = int(offsets[s]), int(offsets[s + 1])
        if b - a < 1:
            continue
        k, v = O.lsd_sort(kt, keys[a:b], None if vals is None else vals[a:b], start, end, desc)
        ek[a:b] = k
        if ev is not None:
            ev[a:b] = v
    return ek, ev


def run(torch, kt, vb, desc, keys, vals, offsets, n, start, end, checked=True, rs=None, tmp=None):
    """one segmented sort; returns (keys, values, classes, tmp)"""
    import tinyhipradixsort_amd as T
    rs = rs or make_sorter(kt, vb, desc)
    ns = offsets.shape[0] - 1
    kd = to_dev(torch, keys)
    vd = to_dev(torch, vals) if vb else None
    od = to_dev(torch, offsets.astype(np.uint32))
    if tmp is None:
        tmp = torch.empty(rs.getSegmentedTemporaryBufferBytes(n, ns, bool(vb)), dtype=torch.uint8, device="cuda")
    if vb:
        rs.sortPairsSegmented(kd, vd, n, od, ns, tmp, start, end, checked=checked)
    else:
        rs.sortKeysSegmented(kd, n, od, ns, tmp, start, end, checked=checked)
    torch.cuda.synchronize()
    classes = T.debug_segment_classes(tmp)
    k = from_dev(kd, keys.dtype, keys.shape)
    v = from_dev(vd, vals.dtype, vals.shape) if vb else None
    return k, v, classes, tmp


def check(torch, kt, vb, desc, keys, vals, offsets, start=0, end=None, **kw):
    end = O.KEY_BYTES[kt] * 8 if end is None else end
    n = keys.shape[0]
    k, v, classes, _ = run(torch, kt, vb, desc, keys, vals, offsets, n, start, end, **kw)
    ek, ev = expected(kt, keys, vals, offsets, start, end, desc)
    assert np.array_equal(k, ek), (kt, vb, desc, start, end, first_bad_segment(k, ek, offsets))
    if vb:
        assert np.array_equal(v, ev), (kt, vb, desc, start, end, first_bad_segment(v, ev, offsets))
    return k, v, classes


def first_bad_segment(got, want, offsets):
    g = got.reshape(got.shape[0], -1)
    w = want.reshape(want.shape[0], -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    if bad.size == 0:
        return None
    s = int(np.searchsorted(offsets, bad[0], side="right")) - 1
    return {"element": int(bad[0]), "segment": s, "range": (int(offsets[max(s, 0)]), int(offsets[min(s + 1, len(offsets) - 1)]))}


# ------------------------------------------------------------ 1. class boundaries
@pytest.mark.parametrize("kt", KTS)
@pytest.mark.parametrize("vb", [0, 4, 8, 16])
@pytest.mark.parametrize("desc", [False, True])
def test_class_boundaries(gpu, kt, vb, desc):
    """Sizes around both class bounds in one call, empty segments between them,
    odd sizes leaving later segments misaligned; the class counts prove each
    kernel ran."""
    offsets = offsets_of(boundary_sizes(kt, vb))
    n = int(offsets[-1])
    keys = random_keys(kt, n, seed=kt * 10 + vb)
    vals = C._values(n, vb) if vb else None
    _, _, classes = check(gpu, kt, vb, desc, keys, vals, offsets)
    assert classes == host_classes(kt, vb, offsets)
    assert classes[1] >= 6 and classes[2] >= 3 and classes[3] >= 2


# ------------------------------------------------------------ 2. windows
@pytest.mark.parametrize("kt,vb,window", [(O.U64, 4, w) for w in [(0, 8), (8, 24), (16, 48), (32, 64)]] +
                         [(O.F32, 0, w) for w in [(0, 8), (8, 24), (16, 48), (32, 64)]])
def test_windows(gpu, kt, vb, window):
    offsets = offsets_of(boundary_sizes(kt, vb))
    n = int(offsets[-1])
    keys = random_keys(kt, n, seed=77)
    vals = C._values(n, vb) if vb else None
    k, _, _ = check(gpu, kt, vb, False, keys, vals, offsets, window[0], window[1])
    if kt == O.F32 and window == (32, 64):
        assert np.array_equal(k, keys)        # every digit past the key width: the identity


# ------------------------------------------------------------ 3. ties and stability
@pytest.mark.parametrize("kt", KTS)
def test_ties_and_stability(gpu, kt):
    """Keys from 4 distinct values, all-equal segments and segments whose keys
    differ only in the top byte, one segment per class each; values are an iota,
    so the oracle comparison on them is the stability check."""
    c0, c1 = caps_of(kt, 4)
    per_class = [c0 - 3, c1 - 5, c1 + 1001]
    sizes = per_class * 3
    offsets = offsets_of(sizes)
    n = int(offsets[-1])
    dt = O.KEY_DTYPE[kt]
    width = O.KEY_BYTES[kt] * 8
    draws = O.splitmix64_stream(5, n)
    four = O.randomize_np(kt, O.splitmix64_stream(900, 4))
    keys = four[(draws % np.uint64(4)).astype(np.int64)].astype(dt)
    a = int(offsets[3])
    keys[a:int(offsets[6])] = four[1]                                    # all-equal segments
    b, e = int(offsets[6]), int(offsets[9])
    top = (draws[b:e] % np.uint64(3)).astype(dt) << dt(width - 8)        # differ in the top byte only
    keys[b:e] = (four[2] & dt((1 << (width - 8)) - 1)) | top
    vals = C._values(n, 4)
    for desc in (False, True):
        _, _, classes = check(gpu, kt, 4, desc, keys, vals, offsets)
        assert classes == (0, 3, 3, 3)


# ------------------------------------------------------------ 4. float specials
@pytest.mark.parametrize("kt", [O.F32, O.F64])
@pytest.mark.parametrize("desc", [False, True])
def test_float_specials(gpu, kt, desc):
    """NaN, +-Inf, denormals and +-0 tiled through one segment of each class:
    original bit patterns come back, +-0 ties in input order."""
    c0, c1 = caps_of(kt, 4)
    offsets = offsets_of([c0 - 1, c1 - 1, c1 + 333])
    n = int(offsets[-1])
    f32 = np.array(C.F32_SPECIALS, np.uint32)
    if kt == O.F32:
        spec = f32
    else:  # the f64 counterparts: the same classes at double width
        spec = np.array([0x7FF8000000000000, 0x0000000000000000, 0xFFF0000000000000, 0x8000000000000000,
                         0x0000000000000001, 0x3FF0000000000000, 0xFFF8000000000000, 0x800FFFFFFFFFFFFF,
                         0x7FF0000000000000, 0xBFF0000000000000, 0x8000000000000001, 0x000FFFFFFFFFFFFF,
                         0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF], np.uint64)
    keys = np.tile(spec, n // spec.shape[0] + 1)[:n].copy()
    vals = C._values(n, 4)
    k, v, classes = check(gpu, kt, 4, desc, keys, vals, offsets)
    assert classes == (0, 1, 1, 1)
    assert np.array_equal(np.sort(k), np.sort(keys))                      # the original bit patterns
    pz, nz = spec[1], spec[3]
    for s in range(3):                                                    # +-0 tie: input order kept
        a, b = int(offsets[s]), int(offsets[s + 1])
        z = (k[a:b] == pz) | (k[a:b] == nz)
        zv = v[a:b][z]
        assert zv.size > 0 and np.all(np.diff(zv.astype(np.int64)) > 0)
        assert np.array_equal(keys[zv], k[a:b][z])


# ------------------------------------------------------------ 5. many tiny segments
@pytest.mark.parametrize("kt,vb", [(O.U32, 4), (O.U64, 8)])
def test_many_tiny_segments(gpu, kt, vb):
    """20 011 segments of 0..40 keys: the wave class's grid-stride loop and its
    tail (the count is no multiple of the segments per workgroup)."""
    rng = np.random.default_rng(20011)
    sizes = rng.integers(0, 41, size=20011)
    offsets = offsets_of(sizes)
    n = int(offsets[-1])
    keys = random_keys(kt, n, seed=3)
    vals = C._values(n, vb)
    _, _, classes = check(gpu, kt, vb, False, keys, vals, offsets)
    assert classes == host_classes(kt, vb, offsets)
    assert classes[1] > 19000 and classes[2] == 0 and classes[3] == 0


# ------------------------------------------------------------ 6. uniform rows
@pytest.mark.parametrize("kt,L", [(O.U32, 1000), (O.F32, 5000)])
def test_uniform_rows(gpu, kt, L):
    rows = 257
    n = rows * L
    offsets = (np.arange(rows + 1, dtype=np.uint64) * L).astype(np.uint32)
    keys = random_keys(kt, n, seed=11)
    k, _, classes = check(gpu, kt, 0, False, keys, None, offsets)
    assert classes == (0, 0, rows, 0)
    img = O.key_bits_np(kt, keys).reshape(rows, L)
    assert np.array_equal(O.key_bits_np(kt, k).reshape(rows, L), np.sort(img, axis=1))


# ------------------------------------------------------------ 7. outside the segments
@pytest.mark.parametrize("kt,vb", [(O.U32, 4), (O.F64, 16)])
def test_outside_the_segments_is_untouched(gpu, kt, vb):
    """Head and tail of [0, n) outside the offsets, and the bytes of an
    over-allocated buffer past n, hold a sentinel pattern afterwards."""
    torch = gpu
    import tinyhipradixsort_amd as T
    sizes = boundary_sizes(kt, vb)
    inner = int(np.sum(sizes))
    n = 37 + inner + 53
    extra = 301
    offsets = offsets_of(sizes, first=37)
    assert int(offsets[0]) == 37 and int(offsets[-1]) == n - 53
    dt = O.KEY_DTYPE[kt]
    keys = np.empty(n + extra, dt)
    keys[:n] = random_keys(kt, n, seed=21)
    sentinel = dt(0xA5A5A5A5A5A5A5A5 & ((1 << (8 * O.KEY_BYTES[kt])) - 1))
    keys[:37] = sentinel
    keys[n - 53:] = sentinel
    vals = C._values(n + extra, vb)
    vals[:37] = 0xC3
    vals[n - 53:] = 0xC3
    rs = make_sorter(kt, vb, False)
    kd, vd, od = to_dev(torch, keys), to_dev(torch, vals), to_dev(torch, offsets)
    tmp = torch.empty(rs.getSegmentedTemporaryBufferBytes(n, len(sizes), True), dtype=torch.uint8, device="cuda")
    rs.sortPairsSegmented(kd, vd, n, od, len(sizes), tmp, 0, O.KEY_BYTES[kt] * 8, checked=True)
    torch.cuda.synchronize()
    k = from_dev(kd, keys.dtype, keys.shape)
    v = from_dev(vd, vals.dtype, vals.shape)
    ek, ev = expected(kt, keys, vals, offsets, 0, O.KEY_BYTES[kt] * 8, False)
    assert np.array_equal(k, ek) and np.array_equal(v, ev)
    for arr, orig in ((k, keys), (v, vals)):
        assert np.array_equal(arr[:37], orig[:37]) and np.array_equal(arr[n - 53:], orig[n - 53:])
    assert T.debug_segment_classes(tmp) == host_classes(kt, vb, offsets)


# ------------------------------------------------------------ 8. bad offsets
def test_bad_offsets_are_rejected_not_followed(gpu):
    """One decreasing entry and one entry of n + 5 in a 6-segment table: a range
    check taken before any access (no fault is provoked).  checked=True raises
    status -6; the valid segments are sorted; the bad ranges and everything
    outside are unchanged; the next valid sort on the buffer reports nothing."""
    torch = gpu
    import tinyhipradixsort_amd as T
    kt, vb = O.U32, 4
    n = 12000
    # s0 [0,200) and s1 [200,5000) are valid; s2 [5000,4000) decreases; s3
    # [4000,4000) is empty; s4 [4000,n+5) ends past n; s5 [n+5,n) starts past n
    offsets = np.array([0, 200, 5000, 4000, 4000, n + 5, n], np.uint32)
    valid = [True, True, False, True, False, False]
    keys = random_keys(kt, n, seed=31)
    vals = C._values(n, vb)
    rs = make_sorter(kt, vb, False)
    tmp = torch.empty(rs.getSegmentedTemporaryBufferBytes(n, 6, True), dtype=torch.uint8, device="cuda")
    kd, vd, od = to_dev(torch, keys), to_dev(torch, vals), to_dev(torch, offsets)
    torch.cuda.synchronize()
    T.lib().thrs_take_device_error()                     # clear what earlier sorts left in the sticky word
    with pytest.raises(T.ThrsError) as e:
        rs.sortPairsSegmented(kd, vd, n, od, 6, tmp, 0, 32, checked=True)
    assert e.value.status == -6
    assert T.lib().thrs_take_device_error() == -6        # the sticky word saw it too
    k, v = from_dev(kd, keys.dtype, keys.shape), from_dev(vd, vals.dtype, vals.shape)
    ek, ev = expected(kt, keys, vals, offsets, 0, 32, False, valid=valid)
    assert np.array_equal(k, ek) and np.array_equal(v, ev)                                   # valid segments sorted
    assert np.array_equal(k[5000:], keys[5000:]) and np.array_equal(v[5000:], vals[5000:])   # bad ranges, the rest
    assert T.debug_segment_classes(tmp) == (1, 1, 1, 0)
    # a following valid sort on the same buffer succeeds and reports no error
    good = np.array([0, 1000, 1000, 3000, 6000, 6001, n], np.uint32)
    k2, v2, classes, _ = run(torch, kt, vb, False, keys, vals, good, n, 0, 32, checked=True, rs=rs, tmp=tmp)
    ek2, ev2 = expected(kt, keys, vals, good, 0, 32, False)
    assert np.array_equal(k2, ek2) and np.array_equal(v2, ev2)
    rs.checkDeviceError(tmp)
    assert T.lib().thrs_take_device_error() == 0


# ------------------------------------------------------------ 9. offsets made on the device
def test_offsets_produced_on_the_device(gpu):
    """The offsets are written by a torch op on the same stream right before
    the sort, no synchronisation between: the host never reads them."""
    torch = gpu
    kt, vb = O.U32, 4
    sizes = np.array(boundary_sizes(kt, vb) + [300] * 50)
    offsets = offsets_of(sizes)
    n = int(offsets[-1])
    keys = random_keys(kt, n, seed=51)
    vals = C._values(n, vb)
    rs = make_sorter(kt, vb, False)
    ns = sizes.shape[0]
    tmp = torch.empty(rs.getSegmentedTemporaryBufferBytes(n, ns, True), dtype=torch.uint8, device="cuda")
    kd, vd = to_dev(torch, keys), to_dev(torch, vals)
    sz = torch.from_numpy(sizes.astype(np.int32)).to("cuda")
    od = torch.zeros(ns + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    od[1:] = torch.cumsum(sz, 0).to(torch.int32)           # device op on the current stream ...
    rs.sortPairsSegmented(kd, vd, n, od, ns, tmp, 0, 32)   # ... and the sort right behind it
    torch.cuda.synchronize()
    rs.checkDeviceError(tmp)
    ek, ev = expected(kt, keys, vals, offsets, 0, 32, False)
    assert np.array_equal(from_dev(kd, keys.dtype, keys.shape), ek)
    assert np.array_equal(from_dev(vd, vals.dtype, vals.shape), ev)


# ------------------------------------------------------------ 10. the C++ header
def test_cpp_header_segmented(gpu):
    exe = os.path.join(ROOT, "tests", "cpp", "segmented_thrs")
    assert os.path.exists(exe), "tests/cpp/segmented_thrs is built by `make`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
