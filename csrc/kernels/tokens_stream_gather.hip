// Stream piece gather: the tokens of one token stream batch copied out of the corpus into a flat staging window in
// HBM, driven by the plan token_stream_plan / token_stream_plan_rows left in device memory. The source may be pinned,
// device-mapped host memory (the zero-copy token stream loader: every byte of a batch crosses PCIe once) or HBM; the
// unchanged pad_pack_tokens_indexed then renders the batch with the window as its corpus (seg_src = the plan's
// seg_offsets: piece s starts at window element seg_offsets[s]). All the index arithmetic is tokens_stream_gather.h.
//
// As in gather_ragged (ragged.hip) the source side decides the shape: mapped host memory is uncached on the device,
// every load instruction is a PCIe read, so a lane issues naturally aligned 16-byte non-temporal loads, kRgUnroll of
// them before its first store, and the surviving elements go out as element stores into HBM. Unlike there the host
// knows no piece -- not even how many there are -- so the grid is static: tiles are kSgChunkBytes chunks of the
// DESTINATION window, workgroups grid-stride over the chunks the plan's counts give (max_blocks caps the grid), and
// a workgroup finds its chunk's first and last piece by the wave-wide search of seg_offsets (ts_wave_last_le, every
// wave on its own: no barrier) and walks the pieces between them.
//
// Short pieces: the pieces of a chunk are taken in groups of kSgGroup = 256, one per lane; the lanes' unit counts are
// scanned into LDS (an LDS prefix) and the group's units are dealt to the lanes 4 at a time, a lane finding its
// unit's piece by a binary search of the 257 prefix entries (8 LDS reads). A loop piece by piece would leave 255
// lanes idle behind every short document; here a pass holds 1024 units of however many pieces. What a window of
// 1-token documents costs: every piece is one unit, so 16 bytes cross the link for 2 or 4 (8x / 4x the traffic of
// long documents), a group has 256 units -- one load per lane, nothing of the 4-deep unroll -- and a 16 KB chunk of
// uint16 ids is 32 groups of two barriers each. Real corpora (documents of hundreds of tokens) have 8 - 64 pieces per
// chunk: one group, its units a few more than the chunk's 1024.
//
// Bounded reads: nothing outside the 16-byte aligned hulls of the clipped pieces (a naturally aligned 16-byte load
// never crosses a page, and the loader registers the page-rounded mapping of the corpus, so every byte of a hull lies
// in a mapped page); a piece whose source range [seg_src[s], seg_src[s] + len_s) is not inside [0, corpus_elems) --
// a corrupt plan -- is not dereferenced; a negative row count (an overflowed or invalid plan), n_seg = 0 and n_seg >
// max_segs read only the two counts and write nothing. Of the plan seg_offsets[0 .. n_seg] and seg_src[0 .. n_seg)
// are read, n_seg <= max_segs.
// Bounded writes: only dst[g] for g < min(seg_offsets[n_seg], rows * S), each exactly once: chunks partition those
// positions, the clipped pieces partition a chunk, and element p of a clipped piece is stored only for 0 <= p < len.
// All byte offsets are 64-bit (a corpus is larger than 4 GB). Every barrier is reached by the whole workgroup: the
// chunk, group and pass loops have block-uniform trip counts.
#include "common.h"
#include "launch.h"
#include "tokens_stream_gather.h"
#include "tokens_stream_wave.h"

namespace ddl {
namespace {

constexpr int kSgWaves = kRgThreads / kTpWave;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ T sg_unit_elem(const u32x4& v, int e) {
  constexpr int per_word = 4 / static_cast<int>(sizeof(T));
  const uint32_t w = v[e / per_word];
  if constexpr (sizeof(T) == 4)
    return w;
  else
    return static_cast<T>(w >> (16 * (e % per_word)));
}

struct StreamGatherArgs {
  const uint8_t* src;
  int64_t corpus_elems;
  const int64_t* seg_src;
  const int64_t* seg_offsets;
  const int64_t* counts;
  int64_t max_segs, rows, seq_len;
};

template <typename T>
__global__ void __launch_bounds__(kRgThreads) gather_stream_pieces_kernel(T* __restrict__ dst, StreamGatherArgs g) {
  constexpr int eb = static_cast<int>(sizeof(T));
  constexpr int per_unit = kRgUnitBytes / eb;
  __shared__ int64_t upre_lds[kSgGroup + 1];  // exclusive scan of the group's unit counts, entry kSgGroup = their sum
  __shared__ uint64_t a_lds[kSgGroup];
  __shared__ int64_t d0_lds[kSgGroup], len_lds[kSgGroup];
  __shared__ int64_t wave_tot[kSgWaves];
  const int tid = static_cast<int>(threadIdx.x), lane = tid & (kTpWave - 1), wv = tid / kTpWave;
  const int64_t n_rows = g.counts[0], n_seg = g.counts[1];  // block-uniform
  if (!sg_plan_ok(n_rows, n_seg, g.max_segs)) return;
  const int64_t limit = sg_limit(n_rows, g.rows, g.seq_len, g.seg_offsets[n_seg]);
  const int64_t n_chunks = sg_chunks(limit, eb);
  const uint64_t src = reinterpret_cast<uint64_t>(g.src);
  const auto seg_at = [&](int64_t i) { return g.seg_offsets[i]; };
  const auto src_at = [&](int64_t i) { return g.seg_src[i]; };
  const auto upre = [&](int64_t j) { return upre_lds[j]; };
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    int64_t c0, c1;
    sg_chunk(c, limit, eb, &c0, &c1);
    // the pieces that hold the chunk's first and last position (seg_offsets[0] = 0 <= c0 < c1 <= seg_offsets[n_seg])
    const int64_t s0 = ts_wave_last_le(g.seg_offsets, n_seg, c0);
    const int64_t s1 = ts_wave_last_le(g.seg_offsets, n_seg, c1 - 1);
    for (int64_t gb = s0; gb <= s1; gb += kSgGroup) {  // block-uniform trip count
      SgPiece p{0, 0, 0, 0};
      if (gb + tid <= s1) p = sg_piece(seg_at, src_at, gb + tid, n_seg, c0, c1, src, g.corpus_elems, eb);
      const int64_t incl = ts_wave_incl_scan(p.units);
      if (lane == kTpWave - 1) wave_tot[wv] = incl;
      a_lds[tid] = p.a;
      d0_lds[tid] = p.d0;
      len_lds[tid] = p.len;
      __syncthreads();
      const int64_t before = tp_before(wave_tot, wv, 0);
      upre_lds[tid] = tp_exclusive(before, incl, p.units);
      if (tid == kRgThreads - 1) upre_lds[kSgGroup] = before + incl;
      __syncthreads();
      const int64_t total = upre_lds[kSgGroup];
      for (int64_t base = 0; base < total; base += kRgTileUnits) {
        u32x4 v[kRgUnroll];
        int pj[kRgUnroll];
        int64_t pu[kRgUnroll];
#pragma unroll
        for (int k = 0; k < kRgUnroll; ++k) {
          const int64_t w = sg_unit(base, k, tid);
          pj[k] = -1;
          if (w < total) {
            pj[k] = static_cast<int>(sg_unit_piece(upre, kSgGroup, w));
            pu[k] = w - upre_lds[pj[k]];
            // the unit's address as an offset from the kernel argument (negative in a first unit in front of an
            // unaligned src), so the load stays a global one
            v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(
                g.src + static_cast<int64_t>(rg_unit_addr(a_lds[pj[k]], pu[k]) - src)));
          }
        }
#pragma unroll
        for (int k = 0; k < kRgUnroll; ++k) {
          if (pj[k] >= 0) {
            const int64_t len = len_lds[pj[k]];
            const int64_t head = rg_head_elems(a_lds[pj[k]], eb);
            T* d = dst + d0_lds[pj[k]];
#pragma unroll
            for (int e = 0; e < per_unit; ++e) {
              const int64_t q = rg_elem_pos(pu[k], e, head, eb);
              if (q >= 0 && q < len) d[q] = sg_unit_elem<T>(v[k], e);
            }
          }
        }
      }
      __syncthreads();  // every lane has read the group's LDS
    }
  }
}

}  // namespace

int gather_stream_pieces(void* dst, const void* src, int64_t corpus_elems, const int64_t* seg_src,
                         const int64_t* seg_offsets, const int64_t* counts, int64_t max_segs, int64_t rows,
                         int64_t seq_len, int elem_bytes, int64_t max_blocks, hipStream_t st) {
  if (elem_bytes != 2 && elem_bytes != 4) return -1;
  if (rows < 1 || seq_len < 1 || max_segs < 1 || corpus_elems < 0 || max_blocks < 0) return -2;
  if (!dst || !src || !seg_src || !seg_offsets || !counts) return -2;
  if (rows > 0x7FFFFFFF / seq_len) return -2;  // a batch's positions fit the int32 cu_seqlens, as the plans check
  if (reinterpret_cast<uintptr_t>(src) % elem_bytes || reinterpret_cast<uintptr_t>(dst) % elem_bytes) return -2;
  const int64_t chunks = sg_chunks(rows * seq_len, elem_bytes);  // what the plan can fill at most: the host knows no more
  const int64_t grid = (max_blocks > 0 && max_blocks < chunks) ? max_blocks : chunks;
  const StreamGatherArgs g{static_cast<const uint8_t*>(src), corpus_elems, seg_src, seg_offsets, counts, max_segs, rows,
                           seq_len};
  if (elem_bytes == 4)
    hipLaunchKernelGGL(gather_stream_pieces_kernel<uint32_t>, dim3(static_cast<uint32_t>(grid)), dim3(kRgThreads), 0, st,
                       static_cast<uint32_t*>(dst), g);
  else
    hipLaunchKernelGGL(gather_stream_pieces_kernel<uint16_t>, dim3(static_cast<uint32_t>(grid)), dim3(kRgThreads), 0, st,
                       static_cast<uint16_t*>(dst), g);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
