// Index arithmetic of the first-fit-decreasing order kernel (tokens_ffd.hip), shared with host code:
// csrc/kernels/tests/tokens_ffd_check.cpp replays the kernel's per-lane loops with it under ASan/UBSan.
// Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of HIP).
//
// The definition is ddl_amd.models.tokens.ffd_if_it_wins (ffd_order_py and in_order_rows_py): sequence i of the
// batch has length len_i and is the item (len_i > S ? len_i % S : len_i); an item of size 0 takes part in no bin.
// Items are sorted by descending size, stable in batch position, and placed first fit over the bins in creation
// order; a bin takes at most one long (len > S) sequence, which is emitted at the bin's head. The sequences
// without an item follow the bins in batch order. ffd_rows = bins + sum(len // S over the long sequences).
//
// One workgroup of kFfdThreads lanes: (1) every lane loads its sequences' lengths and makes their item words,
// (2) a bitonic sort of (item word, batch position) in LDS, (3) wave 0 places the sorted items one after another
// over a two-level 64-ary maximum tree of the bins' free space while one lane of wave 1 runs the in-order
// next-fit over the batch order, (4) the bins' sizes are scanned and every item's position is its bin's start +
// its rank in the bin.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DDL_FFD_HD __host__ __device__ __forceinline__
#else
#define DDL_FFD_HD inline
#endif

namespace ddl {

constexpr int kFfdThreads = 1024;   // lanes of the one workgroup
constexpr int kFfdWave = 64;        // = bins per group = groups of the tree
constexpr int kFfdWaves = kFfdThreads / kFfdWave;
constexpr int kFfdMaxSeqs = 4096;   // sequences per batch = bins of the tree (kFfdWave * kFfdWave)
constexpr int kFfdBinsPerLane = kFfdMaxSeqs / kFfdThreads;  // of the scan over the bins' sizes

// ---- item words: the item's size in bits 0 .. 62, "its sequence is long" in bit 63 (a size is < 2^63 for any S)
constexpr uint64_t kFfdFlag = uint64_t{1} << 63;

DDL_FFD_HD uint64_t ffd_item(int64_t len, int64_t S) {
  if (len > S) return static_cast<uint64_t>(len % S) | kFfdFlag;
  return static_cast<uint64_t>(len > 0 ? len : 0);
}
DDL_FFD_HD int64_t ffd_item_size(uint64_t w) { return static_cast<int64_t>(w & ~kFfdFlag); }
DDL_FFD_HD bool ffd_item_long(uint64_t w) { return (w & kFfdFlag) != 0; }
// the full rows a sequence takes besides its item: len // S of a long one
DDL_FFD_HD int64_t ffd_full_rows(int64_t len, int64_t S) { return len > S ? len / S : 0; }

// ---- the sort: descending size, ties by ascending batch position (a total order: positions are distinct). The
// padding entries of the power-of-two sort size are (size 0, position >= n): they sort behind every sequence,
// and the sequences without an item (size 0) end up behind the items in batch order: their final places.
DDL_FFD_HD bool ffd_before(uint64_t wa, uint32_t pa, uint64_t wb, uint32_t pb) {
  const int64_t a = ffd_item_size(wa), b = ffd_item_size(wb);
  return a != b ? a > b : pa < pb;
}
DDL_FFD_HD int64_t ffd_sort_size(int64_t n) {  // the power of two >= max(n, 2)
  int64_t p = 2;
  while (p < n) p <<= 1;
  return p;
}
// compare-exchange p (0 <= p < P / 2) of the bitonic step (k, j), j < k powers of two: elements lo and lo + j,
// in order when (lo & k) == 0 and in reverse order otherwise
DDL_FFD_HD int64_t ffd_pair_lo(int64_t p, int64_t j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }
DDL_FFD_HD bool ffd_pair_forward(int64_t lo, int64_t k) { return (lo & k) == 0; }

// ---- the tree: bin b is slot b % 64 of group b / 64; lane g of the placing wave keeps group g's two maxima
DDL_FFD_HD int ffd_group(int64_t b) { return static_cast<int>(b / kFfdWave); }
DDL_FFD_HD int ffd_slot(int64_t b) { return static_cast<int>(b % kFfdWave); }
DDL_FFD_HD int64_t ffd_bin(int g, int slot) { return static_cast<int64_t>(g) * kFfdWave + slot; }

// ---- bin words: the free space in bits 0 .. 62, "holds a long sequence" in bit 63. Two views of one word: what
// a short item may take, and what a long item may take (nothing of a bin that holds a long one). -1: no room for
// any item (an item's size is >= 1), also the view of a bin that does not exist yet.
DDL_FFD_HD uint64_t ffd_bin_open(int64_t S, uint64_t item) {  // a new bin with its first item
  return static_cast<uint64_t>(S - ffd_item_size(item)) | (item & kFfdFlag);
}
DDL_FFD_HD uint64_t ffd_bin_take(uint64_t bin, uint64_t item) {
  return static_cast<uint64_t>(ffd_item_size(bin) - ffd_item_size(item)) | ((bin | item) & kFfdFlag);
}
DDL_FFD_HD int64_t ffd_room_short(uint64_t bin) { return ffd_item_size(bin); }
DDL_FFD_HD int64_t ffd_room_long(uint64_t bin) { return (bin & kFfdFlag) ? -1 : ffd_item_size(bin); }
DDL_FFD_HD int64_t ffd_room(uint64_t bin, bool for_long) { return for_long ? ffd_room_long(bin) : ffd_room_short(bin); }
// a group's maxima need a new reduction only when the bin that shrank held one of them
DDL_FFD_HD bool ffd_needs_refresh(uint64_t old_bin, int64_t max_short, int64_t max_long) {
  return ffd_room_short(old_bin) == max_short || (ffd_room_long(old_bin) >= 0 && ffd_room_long(old_bin) == max_long);
}

// ---- positions: a bin's sequences are its long one, then its short ones in placement order
DDL_FFD_HD int64_t ffd_bin_size(uint32_t n_short, uint64_t bin) { return n_short + (ffd_item_long(bin) ? 1 : 0); }
DDL_FFD_HD int64_t ffd_position(int64_t bin_start, bool is_long, uint32_t rank, uint64_t bin) {
  return is_long ? bin_start : bin_start + rank + (ffd_item_long(bin) ? 1 : 0);
}

// ---- in-order next-fit (in_order_rows_py) over the item words: `cur` = the tokens in the open row (S: none).
// The full rows of the long sequences are counted apart (ffd_full_rows); a long sequence's chunks leave a full row
// behind them, then its remainder is placed like any item.
DDL_FFD_HD void ffd_next_fit(uint64_t item, int64_t S, int64_t* rows, int64_t* cur) {
  const int64_t s = ffd_item_size(item);
  if (ffd_item_long(item)) *cur = S;
  if (s > 0) {
    if (s > S - *cur) {
      ++*rows;
      *cur = 0;
    }
    *cur += s;
  }
}

}  // namespace ddl
