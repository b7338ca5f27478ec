// thrs_segmented.hpp -- segmented sort: many independent ranges of one buffer
// sorted by one call (thrs_sort_segments_keys / thrs_sort_segments_pairs).
//
// Segment s is [segOffsets[s], segOffsets[s+1]) of the caller's keys (and
// values); each is sorted exactly as thrs_sort_keys / thrs_sort_pairs would
// sort it alone: by the 8-bit digits of kimg (getKeyBits ^ ORDER_MASK) that
// the window covers, least significant first, stable, in place.
//
//   thrs_seg_classify   one thread per segment reads its two offsets, checks
//                       them against n BEFORE anything is formed from them (a
//                       decreasing pair or an end past n raises kErrCheck and
//                       the segment is dropped), and appends the segment's
//                       index to the list of its size class (wave-aggregated
//                       atomics: one per class and wave).
//   thrs_seg_wave       size <= SegWave::CAP: one wave per segment, four
//                       segments per workgroup, no workgroup barrier.
//   thrs_seg_block      size <= SegBlock<key bytes>::CAP: one workgroup sorts
//                       the segment in LDS, every round of the window.
//   thrs_seg_stream     any larger size: one workgroup runs an LSD pass per
//                       digit between the segment's range in the caller's
//                       buffer and the same range of keyOut / valueOut.
//
// The class kernels run a GRID-STRIDE loop over their list: the host sizes
// each grid from numSegments and the CU count alone (it never reads the
// counts), and a workgroup whose first list index is past the count exits at
// once -- a million 30-key segments cost a few thousand workgroups.
//
// The streaming class never waits on another workgroup, so it cannot hang,
// and it is correct for any size; but ONE workgroup moves the whole segment
// once per digit, which is slow for a very large segment.  A caller with a
// handful of huge segments should call thrs_sort_keys / thrs_sort_pairs on
// each of them instead.
//
// All three engines rank with the ballot match (wave_rank<false>): stable on
// every device, no per-device probe.  Slots past a segment's end are padding:
// they take digit 255 in every round and sit after every real key in slot
// order, so the stable rank leaves them last; a slot is padding exactly when
// its position is >= the segment's size, in every round.
//
// Values never ride through the LDS rounds: each key carries the u16 slot it
// started at, and the values are gathered by that index afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thrs_kernels.hpp"

namespace thrs_dev {
namespace {

// raised by the classify step (and re-checked by every class kernel): an
// offset pair that decreases or ends past n.  The same bit as a clamped run:
// thrs_check_device_error maps both to THRS_ERROR_DEVICE_CHECK.
constexpr uint32_t kErrCheck = kErrRunClamped;

// words of the segmented sort's counter block in the temporary buffer
// (thrs_host::kCounterOff, next to the error word): segments by class
enum : int { kSegEmpty = 0, kSegWaveC = 1, kSegBlockC = 2, kSegStreamC = 3 };

template <int VB> struct SegVal { using T = uint32_t; };
template <> struct SegVal<8> { using T = uint64_t; };
template <> struct SegVal<16> { using T = uint4; };

// Geometry.  LDS per CU is 160 KiB; a workgroup may use 64 KiB without the
// opt-in.  Every geometry here stays below 64 KiB, and several workgroups
// fit a CU, so one workgroup's barriers and HBM waits are covered by another.
//   wave:   64 lanes x 4 keys = 256 keys per wave, 4 waves (segments) per
//           workgroup.  Per wave 1 KiB of counters + 256 x (8 + 2) B of
//           stage = 3.5 KiB; 14 KiB per workgroup -> 11 workgroups per CU by
//           LDS: the CU's 32 resident waves (8 workgroups) bind first.
//   block:  512 threads (8 waves), a segment's slots spread over all of
//           them.  4-byte keys: 16 keys per thread = 8192
//           keys, 32 KiB keys + 16 KiB u16 indices + 8 KiB counters = 56 KiB
//           -> 2 workgroups (16 waves) per CU.  8-byte keys: 8 per thread =
//           4096 keys, 32 + 8 + 8 = 48 KiB -> 3 workgroups (24 waves) per CU.
//   stream: 512 threads x 4 keys = 2048-key tiles; 8 KiB counters + 1 KiB
//           bases: LDS never limits it.
struct SegWave {
  static constexpr int KPT = 4, WAVES = 4, THREADS = 64 * WAVES;
  static constexpr uint32_t CAP = 64 * KPT;
};
template <int KB> struct SegBlock {
  static constexpr int WAVES = 8, THREADS = 64 * WAVES;
  static constexpr int KPT = KB == 4 ? 16 : 8;
  static constexpr uint32_t CHUNK = 64 * KPT;  // slots of one wave
  static constexpr uint32_t CAP = CHUNK * WAVES;
  static constexpr size_t LDS = (size_t)CAP * KB + (size_t)CAP * 2 + (size_t)WAVES * kBins * 4 + 64;
};
struct SegStream {
  static constexpr int WAVES = 8, THREADS = 64 * WAVES, KPT = 4;
  static constexpr uint32_t CHUNK = 64 * KPT;
  static constexpr uint32_t TILE = CHUNK * WAVES;
};

// orders this wave's LDS accesses (a wave's DS operations execute in issue
// order; the clobber keeps the compiler from moving any across)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---------------------------------------------------------------- classify
__global__ __launch_bounds__(256) void thrs_seg_classify(const uint32_t* __restrict__ off, uint32_t numSegments,
                                                         uint32_t n, uint32_t cap0, uint32_t cap1,
                                                         uint32_t* __restrict__ counts, uint32_t* __restrict__ listW,
                                                         uint32_t* __restrict__ listB, uint32_t* __restrict__ listS,
                                                         uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  // whole waves iterate together (the bound is rounded up to the wave), so
  // the ballots below see every lane
  const uint64_t end = ((uint64_t)numSegments + 63) & ~63ull;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < end; s += stride) {
    int cls = -1;  // -1: no segment, or a rejected one
    bool bad = false;
    if (s < numSegments) {
      const uint32_t a = off[s], b = off[s + 1];
      bad = b < a || b > n;
      if (!bad) {
        const uint32_t size = b - a;
        cls = size <= 1 ? kSegEmpty : size <= cap0 ? kSegWaveC : size <= cap1 ? kSegBlockC : kSegStreamC;
      }
    }
    if (__ballot(bad) != 0 && lane == 0) atomicOr(err, kErrCheck);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint64_t m = __ballot(cls == c);
      if (m == 0) continue;
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&counts[c], (uint32_t)__builtin_popcountll(m));
      base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
      if (cls == c && c != kSegEmpty) {
        const uint32_t pos = base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        uint32_t* list = c == kSegWaveC ? listW : c == kSegBlockC ? listB : listS;
        if (pos < numSegments) list[pos] = (uint32_t)s;
      }
    }
  }
}

// a listed segment's range, re-checked: nothing is formed from a bad pair
__device__ __forceinline__ bool seg_range(const uint32_t* __restrict__ off, uint32_t s, uint32_t numSegments,
                                          uint32_t n, uint32_t& a, uint32_t& size) {
  if (s >= numSegments) return false;
  a = off[s];
  const uint32_t b = off[s + 1];
  if (b < a || b > n) return false;
  size = b - a;
  return true;
}

template <int KT> __device__ __forceinline__ uint32_t seg_digit(const KeyMap<typename KeyTraits<KT>::U>& km,
                                                                typename KeyTraits<KT>::U key, int shift, bool real) {
  return real ? (uint32_t)(kimg<KT>(km, key) >> shift) & 0xFFu : 0xFFu;
}

// ---------------------------------------------------------------- wave class
// One wave sorts one segment of up to 256 keys.  The keys live in registers
// (slot j*64 + lane in item j); a round counts the digits into the wave's own
// counter row, scans the row (4 bins per lane), ranks item by item in slot
// order with the ballot match, and exchanges the keys through the wave's own
// stage.  Only this wave touches its row and stage: no workgroup barrier.
template <int KT, int VB>
__global__ __launch_bounds__(SegWave::THREADS) void thrs_seg_wave(
    typename KeyTraits<KT>::U* keys, void* valsV, const uint32_t* __restrict__ off, uint32_t numSegments, uint32_t n,
    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ list, KeyMap<typename KeyTraits<KT>::U> km,
    int startBits, int nPass) {
  using U = typename KeyTraits<KT>::U;
  using V = typename SegVal<VB>::T;
  constexpr int KPT = SegWave::KPT;
  constexpr uint32_t CAP = SegWave::CAP;
  __shared__ uint32_t s_cnt[SegWave::WAVES][kBins];
  __shared__ U s_key[SegWave::WAVES][CAP];
  __shared__ uint16_t s_idx[SegWave::WAVES][CAP];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* cnt = s_cnt[w];
  U* stK = s_key[w];
  uint16_t* stI = s_idx[w];
  V* vals = static_cast<V*>(valsV);
  const uint32_t count = min(counts[kSegWaveC], numSegments);
  for (uint64_t i = (uint64_t)blockIdx.x * SegWave::WAVES + w; i < count; i += (uint64_t)gridDim.x * SegWave::WAVES) {
    uint32_t a = 0, size = 0;
    if (!seg_range(off, list[i], numSegments, n, a, size) || size > CAP || size < 2) continue;  // wave-uniform
    const int nItems = (int)((size + 63) >> 6);
    U* kseg = keys + a;
    U k[KPT];
    uint32_t ix[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const uint32_t slot = (uint32_t)j * 64 + lane;
      k[j] = kseg[min(slot, size - 1)];  // clamped into the segment: padding slots repeat its last key
      ix[j] = slot;
    }
    for (int r = 0; r < nPass; ++r) {
      const int shift = startBits + 8 * r;
#pragma unroll
      for (int q = 0; q < kBins / 64; ++q) cnt[q * 64 + lane] = 0;
      wave_lds_sync();
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (j < nItems)
          __hip_atomic_fetch_add(&cnt[seg_digit<KT>(km, k[j], shift, (uint32_t)j * 64 + lane < size)], 1u,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      wave_lds_sync();
      {  // exclusive scan of the 256 bins: lane l owns bins 4l .. 4l+3
        const uint32_t c0 = cnt[4 * lane], c1 = cnt[4 * lane + 1], c2 = cnt[4 * lane + 2], c3 = cnt[4 * lane + 3];
        const uint32_t tot = c0 + c1 + c2 + c3;
        const uint32_t ex = wave_incl_scan(tot, lane) - tot;
        wave_lds_sync();
        cnt[4 * lane] = ex;
        cnt[4 * lane + 1] = ex + c0;
        cnt[4 * lane + 2] = ex + c0 + c1;
        cnt[4 * lane + 3] = ex + c0 + c1 + c2;
      }
      wave_lds_sync();
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        if (j < nItems) {  // wave-uniform: every lane takes part in the ballots
          const bool real = (uint32_t)j * 64 + lane < size;
          const uint32_t dst = wave_rank<false>(cnt, seg_digit<KT>(km, k[j], shift, real), lane, false);
          wave_lds_sync();
          if (real && dst < CAP) {  // a real key's slot is below size (padding ranks last)
            stK[dst] = k[j];
            if (VB) stI[dst] = (uint16_t)ix[j];
          }
        }
      }
      wave_lds_sync();
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        if (j < nItems) {
          const uint32_t slot = min((uint32_t)j * 64 + lane, size - 1);
          k[j] = stK[slot];
          if (VB) ix[j] = stI[slot];
        }
      }
      wave_lds_sync();
    }
    if constexpr (VB != 0) {
      // In-place gather: every value load of the segment is issued by this
      // wave, and vmcnt(0) below waits for all of them before the wave's first
      // store of the segment issues.
      V* vseg = vals + a;
      V v[KPT];
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (j < nItems) v[j] = vseg[min(ix[j], size - 1)];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (j < nItems && (uint32_t)j * 64 + lane < size) vseg[(uint32_t)j * 64 + lane] = v[j];
    }
    // (the keys were all loaded before the first round's counts were read)
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (j < nItems && (uint32_t)j * 64 + lane < size) kseg[(uint32_t)j * 64 + lane] = k[j];
  }
}

// ------------------------------------------------- workgroup-wide tile rank
// The shared rank step of the block and streaming classes.  On entry every
// wave has counted its items' digits into its own row of s_cnt (rows zeroed
// before, a barrier after).  Threads d < 256 turn the rows into running
// offsets: row[w][d] = s_base[d] + the counts of digit d in waves < w, and
// s_base[d] advances by the tile's count of d (the streaming class's next
// tile starts there).  After the closing barrier each wave ranks its items in
// slot order against its row.
template <int WAVES>
__device__ __forceinline__ void seg_rows_to_offsets(uint32_t* s_cnt, uint32_t* s_base) {
  const uint32_t tid = threadIdx.x;
  if (tid < (uint32_t)kBins) {
    uint32_t run = s_base[tid];
#pragma unroll
    for (int ww = 0; ww < WAVES; ++ww) {
      const uint32_t c = s_cnt[ww * kBins + tid];
      s_cnt[ww * kBins + tid] = run;
      run += c;
    }
    s_base[tid] = run;
  }
}
// s_base[d] = exclusive scan over d of s_tot[d] (threads d < 256; s_w: 4 words)
__device__ __forceinline__ void seg_scan_bins(const uint32_t* s_tot, uint32_t* s_base, uint32_t* s_w) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t tot = 0, inc = 0;
  if (tid < (uint32_t)kBins) {
    tot = s_tot[tid];
    inc = wave_incl_scan(tot, lane);
    if (lane == 63) s_w[w] = inc;
  }
  __syncthreads();
  if (tid < (uint32_t)kBins) {
    const uint32_t w0 = s_w[0], w1 = s_w[1], w2 = s_w[2];
    s_base[tid] = inc - tot + (w > 0 ? w0 : 0u) + (w > 1 ? w1 : 0u) + (w > 2 ? w2 : 0u);
  }
  __syncthreads();
}

// ---------------------------------------------------------------- block class
// One workgroup sorts one segment of up to CAP keys in LDS: per round, count
// per wave, scan, lane-ordered stable rank, scatter into the stage, reload
// (the manner of loc_rounds, for 4- and 8-byte keys and as many rounds as the
// window has digits).  With ipw = ceil(size / 512) items per wave, wave w
// holds slots [w*ipw*64, (w+1)*ipw*64), item j of lane l the slot
// w*ipw*64 + j*64 + l.
template <int KT, int VB>
__global__ __launch_bounds__(SegBlock<sizeof(typename KeyTraits<KT>::U)>::THREADS) void thrs_seg_block(
    typename KeyTraits<KT>::U* keys, void* valsV, const uint32_t* __restrict__ off, uint32_t numSegments, uint32_t n,
    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ list, KeyMap<typename KeyTraits<KT>::U> km,
    int startBits, int nPass) {
  using U = typename KeyTraits<KT>::U;
  using V = typename SegVal<VB>::T;
  using G = SegBlock<sizeof(U)>;
  constexpr int KPT = G::KPT;
  extern __shared__ __attribute__((aligned(16))) unsigned char seg_smem[];
  U* stK = reinterpret_cast<U*>(seg_smem);
  uint16_t* stI = reinterpret_cast<uint16_t*>(seg_smem + (size_t)G::CAP * sizeof(U));
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(seg_smem + (size_t)G::CAP * (sizeof(U) + 2));
  uint32_t* s_w = s_cnt + G::WAVES * kBins;  // 4 words
  __shared__ uint32_t s_base[kBins];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t* cnt = s_cnt + w * kBins;
  V* vals = static_cast<V*>(valsV);
  const uint32_t count = min(counts[kSegBlockC], numSegments);
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    uint32_t a = 0, size = 0;
    if (!seg_range(off, list[i], numSegments, n, a, size) || size > G::CAP || size < 2) continue;  // block-uniform
    // the segment is spread over all the waves: ipw items per wave (KPT for a
    // full segment), so a 1000-key segment keeps 8 waves busy, not one
    const uint32_t ipw = min((uint32_t)KPT, (size + 64 * G::WAVES - 1) / (64 * G::WAVES));
    const uint32_t w0 = w * ipw * 64;
    // items j of this wave with j*64 < limw hold a real key in some lane; the
    // others are padding in every lane and take no part (they rank last)
    const int32_t limw = (int32_t)size - (int32_t)w0;
    const int nItems = limw <= 0 ? 0 : (int)min(ipw, (uint32_t)(limw + 63) >> 6);
    U* kseg = keys + a;
    U k[KPT];
    uint32_t ix[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const uint32_t slot = w0 + (uint32_t)j * 64 + lane;
      ix[j] = slot;
      if (j < nItems) k[j] = kseg[min(slot, size - 1)];
    }
    for (int r = 0; r < nPass; ++r) {
      const int shift = startBits + 8 * r;
#pragma unroll
      for (int q = 0; q < kBins / 64; ++q) cnt[q * 64 + lane] = 0;
      wave_lds_sync();
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (j < nItems)
          __hip_atomic_fetch_add(&cnt[seg_digit<KT>(km, k[j], shift, w0 + (uint32_t)j * 64 + lane < size)], 1u,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __syncthreads();
      // digit totals over the waves -> exclusive scan -> s_base
      if (tid < (uint32_t)kBins) {
        uint32_t tot = 0;
#pragma unroll
        for (int ww = 0; ww < G::WAVES; ++ww) tot += s_cnt[ww * kBins + tid];
        s_base[tid] = tot;
      }
      __syncthreads();
      seg_scan_bins(s_base, s_base, s_w);
      seg_rows_to_offsets<G::WAVES>(s_cnt, s_base);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        if (j < nItems) {  // wave-uniform: every lane takes part in the ballots
          const bool real = w0 + (uint32_t)j * 64 + lane < size;
          const uint32_t dst = wave_rank<false>(cnt, seg_digit<KT>(km, k[j], shift, real), lane, false);
          wave_lds_sync();
          if (real && dst < G::CAP) {
            stK[dst] = k[j];
            if (VB) stI[dst] = (uint16_t)ix[j];
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        if (j < nItems) {
          const uint32_t slot = min(w0 + (uint32_t)j * 64 + lane, size - 1);
          k[j] = stK[slot];
          if (VB) ix[j] = stI[slot];
        }
      }
      __syncthreads();  // the stage and the rows are rewritten by the next round / segment
    }
    if constexpr (VB != 0) {
      // In-place gather: each thread waits for ALL of its value loads
      // (vmcnt(0)), and the barrier then holds every thread's stores of this
      // segment until every thread has passed that wait -- no store of the
      // segment issues before every load of it has completed.
      V* vseg = vals + a;
      V v[KPT];
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (j < nItems) v[j] = vseg[min(ix[j], size - 1)];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#pragma unroll
      for (int j = 0; j < KPT; ++j)
        if (j < nItems && w0 + (uint32_t)j * 64 + lane < size) vseg[w0 + (uint32_t)j * 64 + lane] = v[j];
    }
    // (every key load completed before the first round's first barrier)
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (j < nItems && w0 + (uint32_t)j * 64 + lane < size) kseg[w0 + (uint32_t)j * 64 + lane] = k[j];
  }
}

// ------------------------------------------------------------ streaming class
// One workgroup owns the segment.  Per digit: a 256-bin histogram of the
// segment in LDS, an exclusive scan, then tile after tile in order -- count
// per wave, rows to running offsets (s_base advances by the tile's counts),
// stable rank, scatter of keys and values straight to base[d] + rank in the
// other buffer.  The source and destination swap per pass; after an odd
// number of passes the range is copied back.  Between passes (and before the
// copy) a workgroup-scope fence and a barrier make one wave's stores visible
// to the other waves' loads: only this workgroup touches the segment's two
// ranges, and its waves share one CU's vector cache.  (A device-scope fence
// here writes the XCD's L2 back once per pass and segment: the 4096 x 16384
// u64 + u32 shape took 31.8 ms with it.)  Nothing here waits on another
// workgroup.
template <int KT, int VB>
__global__ __launch_bounds__(SegStream::THREADS) void thrs_seg_stream(
    typename KeyTraits<KT>::U* keys, void* valsV, typename KeyTraits<KT>::U* keyOut, void* valOutV,
    const uint32_t* __restrict__ off, uint32_t numSegments, uint32_t n, const uint32_t* __restrict__ counts,
    const uint32_t* __restrict__ list, KeyMap<typename KeyTraits<KT>::U> km, int startBits, int nPass) {
  using U = typename KeyTraits<KT>::U;
  using V = typename SegVal<VB>::T;
  using G = SegStream;
  constexpr int KPT = G::KPT;
  __shared__ uint32_t s_cnt[G::WAVES * kBins];
  __shared__ uint32_t s_base[kBins];
  __shared__ uint32_t s_w[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t* cnt = s_cnt + w * kBins;
  const uint32_t count = min(counts[kSegStreamC], numSegments);
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    uint32_t a = 0, size = 0;
    if (!seg_range(off, list[i], numSegments, n, a, size) || size < 2) continue;  // block-uniform
    U* src = keys + a;
    U* dst = keyOut + a;
    V* vsrc = static_cast<V*>(valsV) + (VB ? a : 0);
    V* vdst = static_cast<V*>(valOutV) + (VB ? a : 0);
    for (int r = 0; r < nPass; ++r) {
      const int shift = startBits + 8 * r;
      if (tid < (uint32_t)kBins) s_base[tid] = 0;
      __syncthreads();
      for (uint32_t p = tid; p < size; p += G::THREADS)
        __hip_atomic_fetch_add(&s_base[seg_digit<KT>(km, src[p], shift, true)], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
      __syncthreads();
      seg_scan_bins(s_base, s_base, s_w);
      for (uint32_t t0 = 0; t0 < size; t0 += G::TILE) {  // (size - t0 never wraps: t0 < size)
        const uint32_t left = size - t0;                  // keys from this tile's start on
        const uint32_t w0 = w * G::CHUNK;
        const int nItems = left <= w0 ? 0 : (int)min((uint32_t)KPT, (left - w0 + 63) >> 6);
        U k[KPT];
        V v[KPT];
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          if (j < nItems) {
            const uint32_t slot = min(w0 + (uint32_t)j * 64 + lane, left - 1);  // clamped into the segment
            k[j] = src[(uint64_t)t0 + slot];
            if constexpr (VB != 0) v[j] = vsrc[(uint64_t)t0 + slot];
          }
        }
#pragma unroll
        for (int q = 0; q < kBins / 64; ++q) cnt[q * 64 + lane] = 0;
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < KPT; ++j)
          if (j < nItems)
            __hip_atomic_fetch_add(&cnt[seg_digit<KT>(km, k[j], shift, w0 + (uint32_t)j * 64 + lane < left)], 1u,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        seg_rows_to_offsets<G::WAVES>(s_cnt, s_base);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          if (j < nItems) {  // wave-uniform: every lane takes part in the ballots
            const bool real = w0 + (uint32_t)j * 64 + lane < left;
            const uint32_t d = wave_rank<false>(cnt, seg_digit<KT>(km, k[j], shift, real), lane, false);
            // a real key's destination is below size: base[d] + rank counts
            // real keys only ahead of it (padding ranks after every real key)
            if (real && d < size) {
              dst[d] = k[j];
              if constexpr (VB != 0) vdst[d] = v[j];
            }
          }
        }
        __syncthreads();  // the rows are zeroed again by the next tile
      }
      __threadfence_block();
      __syncthreads();
      U* tk = src;
      src = dst;
      dst = tk;
      V* tv = vsrc;
      vsrc = vdst;
      vdst = tv;
    }
    if (nPass & 1) {  // the result is in keyOut / valueOut: copy the range back
      for (uint32_t p = tid; p < size; p += G::THREADS) {
        dst[p] = src[p];
        if constexpr (VB != 0) vdst[p] = vsrc[p];
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

}  // namespace
}  // namespace thrs_dev

// ------------------------------------------------------------------- host side
#include "thrs_host.hpp"

namespace thrs_host {

// Temporary buffer of a segmented sort:
//   [header: kHeaderBytes, of which the class counts u32[4] at kCounterOff and
//    the error word at kErrOff -- where thrs_check_device_error looks]
//   [wave list u32[numSegments]] [block list] [stream list]   (256-byte steps)
//   [keyOut: n keys] [valueOut: n values, pairs only]
// keyOut / valueOut are the streaming class's ping-pong partners; a segment
// uses its own range of them, so one segment may hold all n keys.
struct SegLayout {
  uint64_t listOff[3];
  uint64_t keyOutOff, valOutOff, bytes;
};
inline SegLayout seg_layout(int kb, int vb, uint32_t n, uint32_t numSegments) {
  SegLayout L{};
  const uint64_t listBytes = round_up((uint64_t)numSegments * 4, kAlign);
  for (int c = 0; c < 3; ++c) L.listOff[c] = kHeaderBytes + (uint64_t)c * listBytes;
  L.keyOutOff = kHeaderBytes + 3 * listBytes;
  L.valOutOff = L.keyOutOff + round_up((uint64_t)kb * n, 16);
  L.bytes = round_up(L.valOutOff + round_up((uint64_t)vb * n, 16), 16);
  return L;
}
inline uint32_t seg_cap_wave() { return SegWave::CAP; }
inline uint32_t seg_cap_block(int kb) { return kb == 4 ? SegBlock<4>::CAP : SegBlock<8>::CAP; }

#ifdef THRS_SEG_KT
// The launch sequence: clear counts + error word, classify, the three class
// kernels (grid-stride over their lists; grids from numSegments and the CU
// count only), publish the error word.  No synchronisation, no allocation.
template <int KT, int VB>
int run_segments_kv(void* keysV, void* vals, uint32_t n, const uint32_t* off, uint32_t numSegments, void* tmp,
                    int startBits, int nPass, bool desc, hipStream_t stream) {
  using U = typename KeyTraits<KT>::U;
  using GB = SegBlock<sizeof(U)>;
  char* base = static_cast<char*>(tmp);
  const SegLayout L = seg_layout((int)sizeof(U), VB, n, numSegments);
  uint32_t* counts = reinterpret_cast<uint32_t*>(base + kCounterOff);
  uint32_t* err = reinterpret_cast<uint32_t*>(base + kErrOff);
  uint32_t* listW = reinterpret_cast<uint32_t*>(base + L.listOff[0]);
  uint32_t* listB = reinterpret_cast<uint32_t*>(base + L.listOff[1]);
  uint32_t* listS = reinterpret_cast<uint32_t*>(base + L.listOff[2]);
  U* keys = static_cast<U*>(keysV);
  U* keyOut = reinterpret_cast<U*>(base + L.keyOutOff);
  void* valOut = base + L.valOutOff;
  static_assert(kErrOff == kCounterOff + 32, "counts and error word are cleared by one memset");
  if (hipMemsetAsync(counts, 0, 36, stream) != hipSuccess) return THRS_ERROR_HIP;
  if (allow_lds(thrs_seg_block<KT, VB>, GB::LDS) != hipSuccess) return THRS_ERROR_HIP;
  KeyMap<U> km;
  km.mask = desc ? ~(U)0 : (U)0;
  const uint64_t cu = (uint64_t)std::max(1, cu_count());
  const uint64_t ns = numSegments;
  const int gridC = (int)std::max<uint64_t>(1, std::min<uint64_t>((ns + 255) / 256, cu * 8));
  const int gridW = (int)std::max<uint64_t>(1, std::min<uint64_t>((ns + SegWave::WAVES - 1) / SegWave::WAVES, cu * 32));
  const int gridB = (int)std::max<uint64_t>(1, std::min<uint64_t>(ns, cu * 8));
  const int gridS = (int)std::max<uint64_t>(1, std::min<uint64_t>(ns, cu * 4));
  hipLaunchKernelGGL(thrs_seg_classify, dim3(gridC), dim3(256), 0, stream, off, numSegments, n, SegWave::CAP, GB::CAP,
                     counts, listW, listB, listS, err);
  hipLaunchKernelGGL((thrs_seg_wave<KT, VB>), dim3(gridW), dim3(SegWave::THREADS), 0, stream, keys, vals, off,
                     numSegments, n, counts, listW, km, startBits, nPass);
  hipLaunchKernelGGL((thrs_seg_block<KT, VB>), dim3(gridB), dim3(GB::THREADS), GB::LDS, stream, keys, vals, off,
                     numSegments, n, counts, listB, km, startBits, nPass);
  hipLaunchKernelGGL((thrs_seg_stream<KT, VB>), dim3(gridS), dim3(SegStream::THREADS), 0, stream, keys, vals, keyOut,
                     valOut, off, numSegments, n, counts, listS, km, startBits, nPass);
  uint32_t* sticky = sticky_dev(stream);
  if (sticky) hipLaunchKernelGGL(thrs_err_publish, dim3(1), dim3(1), 0, stream, err, sticky);
  return hipGetLastError() == hipSuccess ? THRS_SUCCESS : THRS_ERROR_HIP;
}

template <int KT>
int run_segments(int vb, void* keys, void* vals, uint32_t n, const uint32_t* off, uint32_t numSegments, void* tmp,
                 int startBits, int nPass, bool desc, hipStream_t stream) {
  switch (vb) {
    case 0: return run_segments_kv<KT, 0>(keys, vals, n, off, numSegments, tmp, startBits, nPass, desc, stream);
    case 4: return run_segments_kv<KT, 4>(keys, vals, n, off, numSegments, tmp, startBits, nPass, desc, stream);
    case 8: return run_segments_kv<KT, 8>(keys, vals, n, off, numSegments, tmp, startBits, nPass, desc, stream);
    default: return run_segments_kv<KT, 16>(keys, vals, n, off, numSegments, tmp, startBits, nPass, desc, stream);
  }
}
#else
template <int KT>
int run_segments(int vb, void* keys, void* vals, uint32_t n, const uint32_t* off, uint32_t numSegments, void* tmp,
                 int startBits, int nPass, bool desc, hipStream_t stream);
#endif

}  // namespace thrs_host
