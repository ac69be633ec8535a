// Indexed pad/pack: model inputs packed straight out of a token corpus that is resident in HBM (the resident
// token loader). The output is exactly what pad_pack_tokens (tokens.hip) writes for the virtual flat stream
// concat(corpus[src_start[i] : src_start[i] + len_i]) -- but that stream never exists: gather_ragged into a
// flat window followed by pad_pack_tokens out of it is two launches and one extra HBM write and read of every
// token; here every token is read once, from the corpus, by the lane that writes it.
//
// The grid, the prologue and the stores are tokens_emit.h / tokens_indexed.h, shared with pad_pack_kernel. This
// file's part: the lane loop (ti_lane4: the element follows from the searched segment), seg_src staged next to
// seg_offsets in pack mode (a second 8 KB LDS array), the tail of a fixed-capacity cu_seqlens, and the load.
// The kernel is write-bound (~17 B stored per token against 2-4 B read), so the source side stays simple: one
// element load per token at element alignment, bounds-checked, non-temporal (the corpus streams through; the
// fresh batch is what should stay in the cache).
//
// Bounded reads: a corpus element is read only for a position p < min(len, S) of a data row, at
//   pad   src_start[row] + p,                    p < len_row
//   pack  seg_src[s] + (g - seg_offsets[s]),     seg_offsets[s] <= g < seg_offsets[s + 1]
// i.e. only inside [src_start[i], src_start[i] + len_i) of the selected sequences (a segment is a piece of one
// sequence). An empty sequence, a padding position and a padding row read nothing. With labels the lane also
// reads the token at p0 + 4, the target of its last position, only where p0 + 4 < len and (pack) g + 1 lies in
// the same segment: the element after its fourth, inside the same bounds (ti_labels4). On top of that contract an
// element index outside [0, corpus_elems) -- a corrupt descriptor -- is not dereferenced: pad_id is written.
// Bounded writes: workgroup (row, chunk) writes positions [chunk * 512, min((chunk + 1) * 512, S)) of row
// `row` < max(rows, fill_rows) of every output, each exactly once (the vector path only where all 4 positions
// are inside the row), so every element of every [R, S] output is written once and nothing outside;
// cu_seqlens_out[0 .. n_seg] is written by block 0, and with a capacity (cu_cap) also (n_seg, cu_cap].
// A plan built on the device (dev_counts, pack mode): rows and n_seg are two block-uniform loads of the plan's
// counts, clamped by ti_prologue (tokens_emit.h) -- a negative row count, an overflowed plan, makes every row
// padding; the grid covers fill_rows, the plan's row capacity, and pack_plan_device never reports
// more rows or segments than its capacities, which are the sizes of row_start / row_end / seg_offsets / seg_src.
#include "common.h"
#include "launch.h"
#include "tokens_emit.h"

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

__global__ void __launch_bounds__(kTiThreads) pad_pack_indexed_kernel(IndexedSpec ix, int32_t chunks) {
  __shared__ int64_t seg_lds[kTiSegCap];
  __shared__ int64_t src_lds[kTiSegCap];
  TokenSpec& sp = ix.tok;
  const TiRow r =
      ti_prologue(sp, blockIdx.x, chunks, seg_lds, ix.cu_cap, [&](int64_t i) { src_lds[i] = ix.seg_src[i]; });
  if (sp.cu_seqlens_out != nullptr && blockIdx.x == 0 && ix.cu_cap > r.n_cu) {
    // the tail of a fixed-capacity cu_seqlens, behind the prologue's copy: zero-length sequences at the token count
    const int32_t total = static_cast<int32_t>(sp.seg_offsets[r.n_cu]);
    for (int64_t i = r.n_cu + 1 + threadIdx.x; i <= ix.cu_cap; i += kTiThreads) sp.cu_seqlens_out[i] = total;
  }
  if (!r.live || r.p0 >= sp.seq_len) return;
  const int64_t src0 = sp.mode == 0 && r.row < sp.rows ? ix.src_start[r.row] : 0;
  const int32_t* c32 = static_cast<const int32_t*>(ix.corpus);
  const uint16_t* c16 = static_cast<const uint16_t*>(ix.corpus);
  const bool labels = sp.labels != nullptr;  // block-uniform, like attn_mask
  TiLane4 ln;
  TiLabel4 lb;
  if (r.staged) {
    const auto seg_at = [&](int64_t i) { return seg_lds[i]; };
    ti_lane4(sp.mode, r.p0, r.start, r.len, src0, sp.n_seg, seg_at, [&](int64_t i) { return src_lds[i]; }, &ln);
    if (labels) ti_labels4(sp.mode, r.p0, r.start, r.len, seg_at, ln, &lb);
  } else {
    const auto seg_at = [&](int64_t i) { return sp.seg_offsets[i]; };
    ti_lane4(sp.mode, r.p0, r.start, r.len, src0, sp.n_seg, seg_at, [&](int64_t i) { return ix.seg_src[i]; }, &ln);
    if (labels) ti_labels4(sp.mode, r.p0, r.start, r.len, seg_at, ln, &lb);
  }
  const auto load = [&](int64_t e) {
    if (static_cast<uint64_t>(e) < static_cast<uint64_t>(ix.corpus_elems))  // -1 (padding) fails it too
      return sp.tok16 ? static_cast<int32_t>(__builtin_nontemporal_load(c16 + e)) : __builtin_nontemporal_load(c32 + e);
    return sp.pad_id;  // a corrupt descriptor's element outside the corpus is not dereferenced
  };
  int32_t tok[kTiLane], lab[kTiLane];
#pragma unroll
  for (int k = 0; k < kTiLane; ++k) tok[k] = load(ln.src[k]);
  if (labels) {
    // the label of position p is the token at p + 1: the lane's own next token, and for its last position one
    // more element, adjacent to the lane's fourth (the neighbouring lane loads it as its first)
#pragma unroll
    for (int k = 0; k + 1 < kTiLane; ++k) lab[k] = lb.has[k] ? tok[k + 1] : sp.ignore_index;
    lab[kTiLane - 1] = lb.has[kTiLane - 1] ? load(lb.src4) : sp.ignore_index;
  }
  ti_store4(sp, r.row, r.p0, tok, ln.pos, ln.seg, ln.msk, lab);
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
        reinterpret_cast<uintptr_t>(spec.segment_ids) % 16 || reinterpret_cast<uintptr_t>(spec.attn_mask) % 4 ||
        reinterpret_cast<uintptr_t>(spec.labels) % 16)
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
