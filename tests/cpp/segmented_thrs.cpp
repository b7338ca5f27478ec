// segmented_thrs.cpp -- the segmented sort through the drop-in header
// <thrs/tinyhipradixsort.hpp>: sortPairsSegmented on u32 keys + u32 values,
// segment sizes around both class bounds, against std::stable_sort run on each
// segment alone.  Compiled with plain g++ (the header needs no HIP headers).
// Exit status 0 = every segment matches.
#include <thrs/tinyhipradixsort.hpp>

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <utility>
#include <vector>

struct splitmix64 {
  uint64_t x = 0;
  uint64_t next() {
    uint64_t z = (x += 0x9e3779b97f4a7c15);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;
    z = (z ^ (z >> 27)) * 0x94d049bb133111eb;
    return z ^ (z >> 31);
  }
};

int main() {
  uint32_t caps[2] = {0, 0};
  if (thrs_segment_class_caps(THRS_KEY_U32, 4, caps) != THRS_SUCCESS || !(0 < caps[0] && caps[0] < caps[1])) {
    std::printf("thrs_segment_class_caps failed\n");
    return 2;
  }
  const uint32_t c0 = caps[0], c1 = caps[1];
  const std::vector<uint32_t> sizes = {0, 1, 2, 63, 64, 65, c0 - 1, c0, c0 + 1, 0, c1 - 1, c1, c1 + 1, 3 * c1 + 17};
  std::vector<uint32_t> offsets(sizes.size() + 1, 0);
  for (size_t i = 0; i < sizes.size(); ++i) offsets[i + 1] = offsets[i] + sizes[i];
  const uint32_t n = offsets.back(), numSegments = (uint32_t)sizes.size();

  splitmix64 rng;
  std::vector<uint32_t> keys(n), values(n);
  for (uint32_t i = 0; i < n; ++i) keys[i] = (uint32_t)rng.next() & 0xFFFFu;  // 16 bits: ties in every segment
  std::iota(values.begin(), values.end(), 0u);

  thrs::RadixSort::Config config;
  config.configureWithKeyPair<uint32_t, uint32_t>();
  thrs::RadixSort sorter({}, config);
  thrs::Buffer dKeys((int64_t)n * 4), dValues((int64_t)n * 4), dOffsets((int64_t)offsets.size() * 4);
  thrs::Buffer tmp((int64_t)sorter.getSegmentedTemporaryBufferBytes(n, numSegments, true));
  hipStream_t stream = nullptr;
  thrs::check(thrs_stream_create(&stream));
  thrs::check(thrs_memcpy_htod_async(dKeys.data(), keys.data(), (uint64_t)n * 4, stream));
  thrs::check(thrs_memcpy_htod_async(dValues.data(), values.data(), (uint64_t)n * 4, stream));
  thrs::check(thrs_memcpy_htod_async(dOffsets.data(), offsets.data(), offsets.size() * 4, stream));
  sorter.sortPairsSegmented(dKeys.data(), dValues.data(), n, reinterpret_cast<const uint32_t*>(dOffsets.data()),
                            numSegments, tmp.data(), 0, 32, stream);
  thrs::check(thrs_check_device_error(tmp.data(), stream));
  std::vector<uint32_t> gotK(n), gotV(n);
  thrs::check(thrs_memcpy_dtoh(gotK.data(), dKeys.data(), (uint64_t)n * 4));
  thrs::check(thrs_memcpy_dtoh(gotV.data(), dValues.data(), (uint64_t)n * 4));
  uint32_t counts[4] = {};
  thrs::check(thrs_debug_segment_classes(tmp.data(), stream, counts));
  thrs::check(thrs_stream_destroy(stream));

  int bad = 0;
  for (uint32_t s = 0; s < numSegments; ++s) {
    std::vector<std::pair<uint32_t, uint32_t>> ref;
    for (uint32_t i = offsets[s]; i < offsets[s + 1]; ++i) ref.emplace_back(keys[i], values[i]);
    std::stable_sort(ref.begin(), ref.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (uint32_t i = offsets[s]; i < offsets[s + 1]; ++i) {
      const auto& e = ref[i - offsets[s]];
      if (gotK[i] != e.first || gotV[i] != e.second) {
        if (bad++ < 5) std::printf("segment %u (size %u): element %u differs\n", s, sizes[s], i - offsets[s]);
        break;
      }
    }
  }
  uint32_t want[4] = {0, 0, 0, 0};
  for (uint32_t sz : sizes) ++want[sz <= 1 ? 0 : sz <= c0 ? 1 : sz <= c1 ? 2 : 3];
  for (int c = 0; c < 4; ++c)
    if (counts[c] != want[c]) {
      std::printf("class %d: %u segments, expected %u\n", c, counts[c], want[c]);
      ++bad;
    }
  std::printf("%s: %u segments, %u keys, %d mismatches\n", bad ? "FAILED" : "ok", numSegments, n, bad);
  return bad ? 1 : 0;
}
