// Indexed pad/pack: model inputs packed straight out of a token corpus that is resident in HBM (the resident
// token loader). The output is exactly what pad_pack_tokens (tokens.hip) writes for the virtual flat stream
// concat(corpus[src_start[i] : src_start[i] + len_i]) -- but that stream never exists: gather_ragged into a
// flat window followed by pad_pack_tokens out of it is two launches and one extra HBM write and read of every
// token; here every token is read once, from the corpus, by the lane that writes it.
//
// Shape: pad_pack_kernel's. One workgroup per (row, chunk of kTiSpan = 512 positions), 4 positions per lane,
// 16-byte stores of ids / i32 position ids / segment ids (2 x 16 B for i64 position ids) and a 4-byte mask
// store, per-element stores where the row width is no multiple of 4. Pack mode stages seg_offsets and seg_src
// in LDS (2 x 8 KB) when n_seg + 1 <= kTiSegCap and binary-searches global memory otherwise; a lane searches
// once and then advances. The kernel is write-bound (~17 B stored per token against 2-4 B read), so the source
// side stays simple: one element load per token at element alignment, non-temporal (the corpus streams
// through; the fresh batch is what should stay in the cache). All the index arithmetic is tokens_indexed.h.
//
// Bounded reads: a corpus element is read only for a position p < min(len, S) of a data row, at
//   pad   src_start[row] + p,                    p < len_row
//   pack  seg_src[s] + (g - seg_offsets[s]),     seg_offsets[s] <= g < seg_offsets[s + 1]
// i.e. only inside [src_start[i], src_start[i] + len_i) of the selected sequences (a segment is a piece of one
// sequence). An empty sequence, a padding position and a padding row read nothing. On top of that contract an
// element index outside [0, corpus_elems) -- a corrupt descriptor -- is not dereferenced: pad_id is written.
// Bounded writes: workgroup (row, chunk) writes positions [chunk * 512, min((chunk + 1) * 512, S)) of row
// `row` < max(rows, fill_rows) of every output, each exactly once (the vector path only where all 4 positions
// are inside the row), so every element of every [R, S] output is written once and nothing outside;
// cu_seqlens_out[0 .. n_seg] is written by block 0, and with a capacity (cu_cap) also (n_seg, cu_cap].
// A plan built on the device (dev_counts, pack mode): rows and n_seg are two block-uniform loads of the plan's
// counts, clamped as pad_pack_block (tokens.hip) clamps them -- a negative row count, an overflowed plan, makes
// every row padding; the grid covers fill_rows, the plan's row capacity, and pack_plan_device never reports
// more rows or segments than its capacities, which are the sizes of row_start / row_end / seg_offsets / seg_src.
#include "common.h"
#include "launch.h"
#include "tokens_indexed.h"

namespace ddl {
namespace {

struct IndexedSpec {
  TokenSpec tok;  // tokens == nullptr: every token comes from the corpus
  const void* corpus;
  int64_t corpus_elems;
  const int64_t* src_start;  // [B]: corpus element of each selected sequence
  const int64_t* seg_src;    // pack mode, [n_seg]: corpus element of each segment's first token
  int64_t cu_cap;            // > 0: cu_seqlens_out holds cu_cap + 1 entries, those past n_seg = the token count
};

template <typename SegAt, typename SrcAt>
__device__ __forceinline__ void emit4_indexed(const IndexedSpec& ix, int64_t row, int64_t p0, int64_t start,
                                              int64_t len, int64_t src0, SegAt seg_at, SrcAt src_at) {
  const TokenSpec& sp = ix.tok;
  const int64_t S = sp.seq_len;
  TiLane4 ln;
  ti_lane4(sp.mode, p0, start, len, src0, sp.n_seg, seg_at, src_at, &ln);
  const int32_t* c32 = static_cast<const int32_t*>(ix.corpus);
  const uint16_t* c16 = static_cast<const uint16_t*>(ix.corpus);
  int32_t tok[kTiLane];
#pragma unroll
  for (int k = 0; k < kTiLane; ++k) {
    const int64_t e = ln.src[k];
    if (static_cast<uint64_t>(e) < static_cast<uint64_t>(ix.corpus_elems))  // -1 (padding) fails it too
      tok[k] = sp.tok16 ? static_cast<int32_t>(__builtin_nontemporal_load(c16 + e)) : __builtin_nontemporal_load(c32 + e);
    else
      tok[k] = sp.pad_id;
  }
  const int64_t o = row * S + p0;
  if (ti_vector_store(p0, S)) {
    *reinterpret_cast<int4*>(sp.out_tokens + o) = make_int4(tok[0], tok[1], tok[2], tok[3]);
    if (sp.attn_mask) {
      const uint32_t m = ln.msk[0] | (ln.msk[1] << 8) | (ln.msk[2] << 16) | (static_cast<uint32_t>(ln.msk[3]) << 24);
      *reinterpret_cast<uint32_t*>(sp.attn_mask + o) = m;
    }
    if (sp.position_ids) {
      if (sp.pos_is_i64) {
        int64_t* pp = static_cast<int64_t*>(sp.position_ids) + o;
        *reinterpret_cast<longlong2*>(pp) = make_longlong2(ln.pos[0], ln.pos[1]);
        *reinterpret_cast<longlong2*>(pp + 2) = make_longlong2(ln.pos[2], ln.pos[3]);
      } else {
        *reinterpret_cast<int4*>(static_cast<int32_t*>(sp.position_ids) + o) =
            make_int4(ln.pos[0], ln.pos[1], ln.pos[2], ln.pos[3]);
      }
    }
    if (sp.segment_ids)
      *reinterpret_cast<int4*>(sp.segment_ids + o) = make_int4(ln.seg[0], ln.seg[1], ln.seg[2], ln.seg[3]);
  } else {
    for (int k = 0; k < kTiLane && p0 + k < S; ++k) {
      sp.out_tokens[o + k] = tok[k];
      if (sp.attn_mask) sp.attn_mask[o + k] = ln.msk[k];
      if (sp.position_ids) {
        if (sp.pos_is_i64)
          static_cast<int64_t*>(sp.position_ids)[o + k] = ln.pos[k];
        else
          static_cast<int32_t*>(sp.position_ids)[o + k] = ln.pos[k];
      }
      if (sp.segment_ids) sp.segment_ids[o + k] = ln.seg[k];
    }
  }
}

__global__ void __launch_bounds__(kTiThreads) pad_pack_indexed_kernel(IndexedSpec ix, int32_t chunks) {
  __shared__ int64_t seg_lds[kTiSegCap];
  __shared__ int64_t src_lds[kTiSegCap];
  TokenSpec& sp = ix.tok;
  if (sp.dev_counts != nullptr) {  // plan built on the device: its row / segment counts (block-uniform loads)
    const int64_t n_rows = sp.dev_counts[0];
    sp.rows = n_rows < 0 ? 0 : n_rows;
    sp.n_seg = n_rows < 0 ? 0 : sp.dev_counts[1];
  }
  int64_t row, p0;
  ti_lane_origin(blockIdx.x, chunks, static_cast<int>(threadIdx.x), &row, &p0);
  const bool live = row < (sp.fill_rows > sp.rows ? sp.fill_rows : sp.rows);  // data row or padding row
  int64_t start = 0, len = 0, src0 = 0;  // a padding row: len 0, every position written as padding
  if (row < sp.rows) {
    if (sp.mode == 0) {
      start = sp.offsets[row];
      len = sp.offsets[row + 1] - start;
      src0 = ix.src_start[row];
    } else {
      start = sp.row_start[row];
      len = sp.row_end[row] - start;
    }
  }
  len = ti_row_len(len, sp.seq_len);
  const bool staged = sp.mode == 1 && sp.n_seg + 1 <= kTiSegCap;  // batch-uniform
  if (staged && live)
    for (int64_t i = threadIdx.x; i <= sp.n_seg; i += kTiThreads) {
      seg_lds[i] = sp.seg_offsets[i];
      if (i < sp.n_seg) src_lds[i] = ix.seg_src[i];
    }
  if (sp.cu_seqlens_out != nullptr && blockIdx.x == 0) {  // owned copy of the sequence starts (cu_seqlens)
    const int64_t n_cu = ti_cu_entries(sp.n_seg, ix.cu_cap);
    for (int64_t i = threadIdx.x; i <= n_cu; i += kTiThreads)
      sp.cu_seqlens_out[i] = static_cast<int32_t>(sp.seg_offsets[i]);
    if (ix.cu_cap > n_cu) {  // the tail of a fixed-capacity cu_seqlens: zero-length sequences at the token count
      const int32_t total = static_cast<int32_t>(sp.seg_offsets[n_cu]);
      for (int64_t i = n_cu + 1 + threadIdx.x; i <= ix.cu_cap; i += kTiThreads) sp.cu_seqlens_out[i] = total;
    }
  }
  __syncthreads();
  if (!live || p0 >= sp.seq_len) return;
  if (staged)
    emit4_indexed(ix, row, p0, start, len, src0, [&](int64_t i) { return seg_lds[i]; },
                  [&](int64_t i) { return src_lds[i]; });
  else
    emit4_indexed(ix, row, p0, start, len, src0, [&](int64_t i) { return sp.seg_offsets[i]; },
                  [&](int64_t i) { return ix.seg_src[i]; });
}

}  // namespace

int pad_pack_tokens_indexed(const TokenSpec& spec, const void* corpus, int64_t corpus_elems, const int64_t* src_start,
                            const int64_t* seg_src, hipStream_t st, int64_t cu_cap) {
  if (spec.seq_len <= 0 || spec.rows < 0 || spec.n_seg < 0 || corpus_elems < 0 || cu_cap < 0) return -2;
  if (spec.tokens != nullptr) return -2;  // the corpus is the only source
  if (spec.mode != 0 && spec.mode != 1) return -2;
  const bool dev_plan = spec.dev_counts != nullptr;
  if (dev_plan) {  // rows and n_seg are the device's: every array the kernel may then read must be there
    if (spec.mode != 1 || spec.fill_rows <= 0 || !corpus) return -2;
    if (!spec.row_start || !spec.row_end || !spec.seg_offsets || !seg_src) return -2;
  }
  if ((spec.rows > 0 || spec.fill_rows > 0) && !spec.out_tokens) return -2;
  if (spec.rows > 0) {
    if (!corpus) return -2;
    if (spec.mode == 0 && (!spec.offsets || !src_start)) return -2;
    if (spec.mode == 1 && (!spec.row_start || !spec.row_end || !spec.seg_offsets || !seg_src || spec.n_seg == 0))
      return -2;
  }
  if (spec.mode == 1 && !spec.seg_offsets) return -2;  // read (entry 0 at least) even by a batch of padding rows
  const bool has_cu = spec.mode == 1 && spec.cu_seqlens_out != nullptr;
  const uintptr_t elem = spec.tok16 ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(corpus) % elem) return -2;
  if (spec.seq_len % kTiLane == 0) {  // the vector path: 16-byte stores of the 4- and 8-byte outputs, 4-byte of the mask
    if (reinterpret_cast<uintptr_t>(spec.out_tokens) % 16 || reinterpret_cast<uintptr_t>(spec.position_ids) % 16 ||
        reinterpret_cast<uintptr_t>(spec.segment_ids) % 16 || reinterpret_cast<uintptr_t>(spec.attn_mask) % 4)
      return -2;
  }
  const int64_t grid = ti_grid(dev_plan ? 0 : spec.rows, spec.fill_rows, spec.seq_len, has_cu);
  if (grid < 0) return -4;
  if (grid == 0) return 0;
  IndexedSpec ix{spec, corpus, corpus_elems, src_start, seg_src, has_cu ? cu_cap : 0};
  if (spec.mode == 0 || !has_cu) ix.tok.cu_seqlens_out = nullptr;
  hipLaunchKernelGGL(pad_pack_indexed_kernel, dim3(static_cast<uint32_t>(grid)), dim3(kTiThreads), 0, st, ix,
                     static_cast<int32_t>(ti_chunks(spec.seq_len)));
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
