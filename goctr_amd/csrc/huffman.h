// huffman.h -- interface of huffman.hip (the Huffman tree: on the host, or with the device -- rocPRIM sort + host merge + device
// path fill; both through the same merge).
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

namespace goctr {

// The two-queue merge with the reference's tie-breaking (huffman.go:23-57) in sorted-rank space: sval [V] = the counts sorted
// stably ascending.  parent / code [2V - 1] (resized here): leaf r = rank r, merged node k = V + k, the root has parent -1.
void huffman_merge(const long long* sval, int64_t V, std::vector<int>& parent, std::vector<unsigned char>& code);

// The host builder: root-to-leaf paths of every word (node.go:39-42, at most max_depth - 1 entries), off [V + 1] / nodes / codes
// in word order.  Negative counts are accepted.
void build_huffman(const int64_t* counts, int64_t V, int max_depth, std::vector<long long>& off,
                   std::vector<int>& nodes, std::vector<unsigned char>& codes);

// vocabularies from 50 000 words on are built with the device; below that the host builder is faster than the copies.
// GOCTR_HUFFMAN_DEVICE=0 / 1 forces either.
bool huffman_on_device(int64_t V);

// counts_host [V] >= 0.  Leaves off [V + 1], nodes / codes [total] resident on the calling thread's engine.  parts_ms (may be
// null) = {sort + copy of the sorted counts to the host, host merge, path lengths + prefix sum + fill, total}.
int huffman_build_device(const long long* counts_host, int64_t V, int max_depth, DevBuf<long long>& off, DevBuf<int>& nodes,
                         DevBuf<unsigned char>& codes, long long* total_out, double parts_ms[4]);

}  // namespace goctr
