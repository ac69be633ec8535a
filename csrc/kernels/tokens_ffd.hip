// First-fit-decreasing order of a token batch, built on the device: the n selected sequences of a corpus ->
// index_out [n], their corpus indices in the order of ddl_amd.models.tokens.ffd_if_it_wins, and ffd_counts =
// [ffd_rows, in_order_rows, used]. One launch of one workgroup in front of the unchanged token_batch_descriptor,
// which takes index_out as an explicit index: pack_order="ffd" without the host.
//
// Shape (all the index arithmetic is tokens_ffd.h):
//  1. lane t makes the item words of sequences t, t + 1024, ... (the Feistel permutation inline, an explicit
//     index, or base + i; the descriptor's tp_index_ok / tp_len rules) into LDS, in batch order and as the sort's
//     input, and the full rows of the long sequences are summed (wave sums through __shfl_xor, one total per wave).
//  2. a bitonic sort of (item word, batch position) in LDS by ffd_before: exact for any seq_len, nothing is
//     bucketed by size.
//  3. wave 0 places the sorted items one after another. The bins' words live in LDS; lane g keeps the two maxima
//     of group g (the room for a short item, the room for a long one) in registers. An item costs one __ballot over
//     the groups' maxima, one LDS read and __ballot over the group's 64 bins, one store by the bin's lane, and --
//     only when the bin that shrank held one of the group's maxima -- a wave reduction. The bin's lane also counts
//     the bin's short items, which is each item's rank in its bin (placement order = sorted order), so no pass
//     over the placements is needed for it. Lane 0 of wave 1 runs the in-order next-fit over the batch order at the
//     same time; both are serial chains, on different SIMDs.
//  4. the bins' sizes are scanned (four bins per lane, wave scans joined through LDS) and every sequence goes to
//     its bin's start + its rank; the sequences without an item keep their sorted place behind the bins.
// Every barrier and exit is block-uniform; there are no atomics, and every store is a plain vector store.
//
// Bounded reads: corpus_offsets[q] and corpus_offsets[q + 1] only for 0 <= q < n_corpus (anything else is an
// empty sequence); an explicit index at [0, n). Bounded writes: index_out[0 .. n) and ffd_counts[0 .. 3), each
// exactly once; n = 0 writes only the counts. n <= kFfdMaxSeqs is checked by the launcher.
#include "common.h"
#include "launch.h"
#include "tokens_ffd.h"
#include "tokens_plan.h"

namespace ddl {
namespace {

__device__ __forceinline__ int64_t ffd_wave_sum(int64_t v) {
#pragma unroll
  for (int d = kFfdWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kFfdWave);
  return v;
}

__device__ __forceinline__ int64_t ffd_wave_max(int64_t v) {
#pragma unroll
  for (int d = kFfdWave / 2; d > 0; d >>= 1) {
    const int64_t u = __shfl_xor(v, d, kFfdWave);
    v = u > v ? u : v;
  }
  return v;
}

__device__ __forceinline__ int64_t ffd_wave_incl_scan(int64_t v) {
  const int lane = threadIdx.x & (kFfdWave - 1);
#pragma unroll
  for (int d = 1; d < kFfdWave; d <<= 1) {
    const int64_t u = __shfl_up(v, d, kFfdWave);
    if (lane >= d) v += u;
  }
  return v;
}

// the corpus index and the length of sequence i of the batch, by the descriptor's rules
__device__ __forceinline__ int64_t ffd_len(const FfdOrderSpec& sp, int64_t q) {
  if (!tp_index_ok(q, sp.n_corpus)) return 0;
  return tp_len(sp.corpus_offsets[q], sp.corpus_offsets[q + 1]);
}

__global__ void __launch_bounds__(kFfdThreads) token_ffd_order_kernel(FfdOrderSpec sp) {
  __shared__ uint64_t item[kFfdMaxSeqs];   // item words in batch order; step 4: the bins' starts
  __shared__ uint64_t skey[kFfdMaxSeqs];   // item words, sorted
  __shared__ uint64_t bins[kFfdMaxSeqs];   // bin words
  __shared__ uint16_t spos[kFfdMaxSeqs];   // batch position of sorted entry m
  __shared__ uint16_t n_short[kFfdMaxSeqs];  // short items of bin b
  __shared__ uint16_t bin_of[kFfdMaxSeqs];   // bin of sorted entry m
  __shared__ uint16_t rank_of[kFfdMaxSeqs];  // its rank among the bin's short items
  __shared__ int64_t wave_tot[kFfdWaves];
  __shared__ int64_t sh_bins, sh_items, sh_rows;
  const int t = threadIdx.x, lane = t & (kFfdWave - 1), wv = t / kFfdWave;
  const int64_t n = sp.n, S = sp.seq_len;
  if (n == 0) {  // block-uniform
    if (t < 3) sp.counts[t] = 0;
    return;
  }
  const int64_t P = ffd_sort_size(n);

  // ---- 1. item words
  int64_t full = 0;
  for (int64_t i = t; i < P; i += kFfdThreads) {
    uint64_t w = 0;
    if (i < n) {
      const int64_t len = ffd_len(sp, source_row(sp.ri, i));
      w = ffd_item(len, S);
      full += ffd_full_rows(len, S);
      item[i] = w;
    }
    skey[i] = w;
    spos[i] = static_cast<uint16_t>(i);
  }
  full = ffd_wave_sum(full);
  if (lane == 0) wave_tot[wv] = full;
  __syncthreads();
  full = 0;
  for (int k = 0; k < kFfdWaves; ++k) full += wave_tot[k];

  // ---- 2. bitonic sort (block-uniform trip counts)
  for (int64_t k = 2; k <= P; k <<= 1) {
    for (int64_t j = k >> 1; j > 0; j >>= 1) {
      for (int64_t p = t; p < (P >> 1); p += kFfdThreads) {
        const int64_t lo = ffd_pair_lo(p, j), hi = lo + j;
        const uint64_t wa = skey[lo], wb = skey[hi];
        const uint16_t pa = spos[lo], pb = spos[hi];
        if (ffd_before(wb, pb, wa, pa) == ffd_pair_forward(lo, k)) {
          skey[lo] = wb, skey[hi] = wa;
          spos[lo] = pb, spos[hi] = pa;
        }
      }
      __syncthreads();
    }
  }

  // ---- 3. wave 0: first-fit placement; lane 0 of wave 1: the in-order next-fit
  if (wv == 0) {
    int64_t max_short = -1, max_long = -1;  // of group `lane`
    int64_t n_bins = 0, m = 0;
    for (; m < n; ++m) {  // wave-uniform: every lane reads the same entry
      const uint64_t it = skey[m];
      const int64_t s = ffd_item_size(it);
      if (s == 0) break;  // the items are in front
      const bool lng = ffd_item_long(it);
      const unsigned long long groups = __ballot((lng ? max_long : max_short) >= s);
      int g = 0, slot = 0;
      uint64_t w = 0;
      unsigned long long fits = 0;
      if (groups) {
        g = __ffsll(groups) - 1;
        const int64_t b = ffd_bin(g, lane);
        w = b < n_bins ? bins[b] : 0;
        fits = __ballot(b < n_bins && ffd_room(w, lng) >= s);
      }
      if (fits) {
        slot = __ffsll(fits) - 1;
        const int64_t b = ffd_bin(g, slot);
        // the bin's old word and the group's maxima, broadcast
        const uint64_t old = __shfl(static_cast<int64_t>(w), slot, kFfdWave);
        const int64_t cur_short = __shfl(max_short, g, kFfdWave), cur_long = __shfl(max_long, g, kFfdWave);
        if (lane == slot) {
          w = ffd_bin_take(w, it);
          bins[b] = w;
          const uint16_t r = n_short[b];
          rank_of[m] = r;
          if (!lng) n_short[b] = r + 1;
          bin_of[m] = static_cast<uint16_t>(b);
        }
        if (ffd_needs_refresh(old, cur_short, cur_long)) {  // wave-uniform
          const bool live = ffd_bin(g, lane) < n_bins;
          const int64_t ms = ffd_wave_max(live ? ffd_room_short(w) : -1);
          const int64_t ml = ffd_wave_max(live ? ffd_room_long(w) : -1);
          if (lane == g) max_short = ms, max_long = ml;
        }
      } else {  // a new bin
        const int64_t b = n_bins++;
        const uint64_t nw = ffd_bin_open(S, it);
        if (lane == 0) {
          bins[b] = nw;
          rank_of[m] = 0;
          n_short[b] = lng ? 0 : 1;
          bin_of[m] = static_cast<uint16_t>(b);
        }
        if (lane == ffd_group(b)) {
          const int64_t rs = ffd_room_short(nw), rl = ffd_room_long(nw);
          max_short = rs > max_short ? rs : max_short;
          max_long = rl > max_long ? rl : max_long;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next item reads what this one's lane stored
    }
    if (lane == 0) sh_bins = n_bins, sh_items = m;
  } else if (t == kFfdWave) {
    int64_t rows = 0, cur = S;
#pragma unroll 8
    for (int64_t i = 0; i < n; ++i) ffd_next_fit(item[i], S, &rows, &cur);
    sh_rows = rows;
  }
  __syncthreads();

  // ---- 4. the bins' starts and every sequence's place
  const int64_t n_bins = sh_bins, n_items = sh_items;
  const int64_t ffd_rows = n_bins + full, in_order = sh_rows + full;
  const bool used = ffd_rows < in_order;  // block-uniform
  if (t == 0) {
    sp.counts[0] = ffd_rows;
    sp.counts[1] = in_order;
    sp.counts[2] = used ? 1 : 0;
  }
  if (!used) {
    for (int64_t i = t; i < n; i += kFfdThreads) sp.index_out[i] = source_row(sp.ri, i);
    return;
  }
  int64_t size[kFfdBinsPerLane], mine = 0;
#pragma unroll
  for (int k = 0; k < kFfdBinsPerLane; ++k) {
    const int64_t b = static_cast<int64_t>(t) * kFfdBinsPerLane + k;
    size[k] = b < n_bins ? ffd_bin_size(n_short[b], bins[b]) : 0;
    mine += size[k];
  }
  const int64_t incl = ffd_wave_incl_scan(mine);
  if (lane == kFfdWave - 1) wave_tot[wv] = incl;
  __syncthreads();  // also: the next-fit lane is done with item[]
  int64_t start = tp_exclusive(tp_before(wave_tot, wv, 0), incl, mine);
#pragma unroll
  for (int k = 0; k < kFfdBinsPerLane; ++k) {
    item[static_cast<int64_t>(t) * kFfdBinsPerLane + k] = static_cast<uint64_t>(start);
    start += size[k];
  }
  __syncthreads();
  for (int64_t m = t; m < n; m += kFfdThreads) {
    int64_t at = m;  // a sequence without an item: behind the bins, in batch order
    if (m < n_items) {
      const int64_t b = bin_of[m];
      at = ffd_position(static_cast<int64_t>(item[b]), ffd_item_long(skey[m]), rank_of[m], bins[b]);
    }
    sp.index_out[at] = source_row(sp.ri, spos[m]);
  }
}

}  // namespace

int token_ffd_order(const FfdOrderSpec& spec, hipStream_t st) {
  if (spec.n < 0 || spec.n > kFfdMaxSeqs || spec.seq_len <= 0 || spec.n_corpus < 0) return -2;
  if (!spec.counts || (spec.n > 0 && !spec.index_out)) return -2;
  if (spec.n_corpus > 0 && !spec.corpus_offsets) return -2;
  if (!row_index_ok(spec.ri, spec.n)) return -2;
  hipLaunchKernelGGL(token_ffd_order_kernel, dim3(1), dim3(kFfdThreads), 0, st, spec);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
