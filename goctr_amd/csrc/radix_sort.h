// radix_sort.h -- rocPRIM's device radix sort over bits [0, end_bit), behind one call: the scratch size query, the high-water growth
// of the caller's scratch buffer and the sort.  Included only by the translation units that sort (metrics.hip, metrics_group.hip,
// negsample.hip, huffman.hip, emb_plan.hip): rocPRIM's headers are heavy.
#pragma once
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace goctr {
namespace {

// the one place that names rocPRIM's entry points; temp == nullptr asks for the scratch size only
template <bool Desc, class KI, class KO, class VI, class VO>
hipError_t radix_pairs_call(void* temp, size_t& bytes, KI kin, KO kout, VI vin, VO vout, size_t n, unsigned int end_bit, hipStream_t s) {
  if constexpr (Desc) return rocprim::radix_sort_pairs_desc(temp, bytes, kin, kout, vin, vout, n, 0u, end_bit, s);
  else return rocprim::radix_sort_pairs(temp, bytes, kin, kout, vin, vout, n, 0u, end_bit, s);
}

// high-water growth of a sort's scratch (at least 16 bytes: the pointer is valid however little rocPRIM asks for)
inline int radix_sort_scratch(DevBuf<char>& temp, size_t bytes) { return temp.ensure(std::max<size_t>(bytes, 16), false); }

// scratch bytes of a sort of n (K, V) pairs, for callers that allocate it together with their other buffers
template <bool Desc, class K, class V>
int radix_sort_pairs_bytes(size_t n, unsigned int end_bit, hipStream_t s, size_t* bytes) {
  *bytes = 0;
  GOCTR_HIP((radix_pairs_call<Desc>(nullptr, *bytes, (K*)nullptr, (K*)nullptr, (V*)nullptr, (V*)nullptr, n, end_bit, s)));
  return 0;
}

// stable sort of (key, value) pairs by key, ascending or descending.  -1 with the arena's error if the scratch cannot grow.
template <bool Desc = false, class KI, class KO, class VI, class VO>
int radix_sort_pairs(DevBuf<char>& temp, KI kin, KO kout, VI vin, VO vout, size_t n, unsigned int end_bit, hipStream_t s) {
  size_t bytes = 0;
  GOCTR_HIP((radix_pairs_call<Desc>(nullptr, bytes, kin, kout, vin, vout, n, end_bit, s)));
  if (radix_sort_scratch(temp, bytes)) return -1;
  GOCTR_HIP((radix_pairs_call<Desc>(temp.p, bytes, kin, kout, vin, vout, n, end_bit, s)));
  return 0;
}

// keys alone, ascending
template <class KI, class KO>
int radix_sort_keys(DevBuf<char>& temp, KI kin, KO kout, size_t n, unsigned int end_bit, hipStream_t s) {
  size_t bytes = 0;
  GOCTR_HIP(rocprim::radix_sort_keys(nullptr, bytes, kin, kout, n, 0u, end_bit, s));
  if (radix_sort_scratch(temp, bytes)) return -1;
  GOCTR_HIP(rocprim::radix_sort_keys(temp.p, bytes, kin, kout, n, 0u, end_bit, s));
  return 0;
}

}  // namespace
}  // namespace goctr
