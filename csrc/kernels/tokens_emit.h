// Device half shared by the two pad/pack kernels: pad_pack_kernel / pad_pack_multi_kernel (tokens.hip), which read a
// flat token stream, and pad_pack_indexed_kernel (tokens_indexed.hip), which reads the corpus the stream would have
// been gathered from. The workgroup prologue and the store half are here, the constants and the grid / row
// arithmetic in tokens_indexed.h; each kernel keeps its lane loop (where a token comes from, and when its load
// can issue).
//
// Grid: one workgroup per (row, chunk of kTiSpan = 512 positions), so a 64 x 4096 batch is 512 workgroups. A lane
// writes 4 consecutive positions: 16-byte stores of ids / i32 position ids / segment ids (2 x 16 B for i64 position
// ids, and for the i64 next-token labels where they are asked for) and a 4-byte mask store, per-element stores where the row width is no multiple of 4. Pack mode copies the
// segment starts into LDS once per workgroup when n_seg + 1 <= kTiSegCap and binary-searches there, global memory
// otherwise; a lane searches once and then advances.
#pragma once

#include "launch.h"
#include "tokens_indexed.h"

namespace ddl {

// What a workgroup's prologue hands to its lanes
struct TiRow {
  int64_t row, p0;     // the lane's row and first position
  int64_t start, len;  // the row's first position of the (virtual) flat stream; its tokens, <= seq_len
  bool live;           // a data row or a padding row: false past max(rows, fill_rows) (block-uniform)
  bool staged;         // pack mode: seg_lds holds seg_offsets[0 .. n_seg] (batch-uniform)
  int64_t n_cu;        // block 0 copied seg_offsets[0 .. n_cu] into cu_seqlens_out (where there is one)
};

// One workgroup = (row, chunk) `bx` of batch `sp`. A plan built on the device (dev_counts) replaces sp.rows /
// sp.n_seg by its counts, two block-uniform loads: a negative row count, an overflowed plan, makes every row
// padding. Stages seg_offsets in seg_lds (stage_src(i), i < n_seg, lets the caller stage more next to it), copies
// seg_offsets[0 .. ti_cu_entries(n_seg, cu_cap)] into cu_seqlens_out from block 0, and ends with the barrier.
// Workgroups past the batch's rows (a multi-batch launch is sized for its largest sub-batch) only do that copy.
template <typename StageSrc>
__device__ __forceinline__ TiRow ti_prologue(TokenSpec& sp, uint32_t bx, int32_t chunks, int64_t* seg_lds,
                                             int64_t cu_cap, StageSrc stage_src) {
  if (sp.dev_counts != nullptr) {
    const int64_t n_rows = sp.dev_counts[0];
    sp.rows = n_rows < 0 ? 0 : n_rows;
    sp.n_seg = n_rows < 0 ? 0 : sp.dev_counts[1];
  }
  TiRow r;
  ti_lane_origin(bx, chunks, static_cast<int>(threadIdx.x), &r.row, &r.p0);
  r.live = r.row < (sp.fill_rows > sp.rows ? sp.fill_rows : sp.rows);
  r.start = r.len = 0;  // a padding row: len 0, every position written as padding
  if (r.row < sp.rows) {
    r.start = sp.mode == 0 ? sp.offsets[r.row] : sp.row_start[r.row];
    r.len = (sp.mode == 0 ? sp.offsets[r.row + 1] : sp.row_end[r.row]) - r.start;
  }
  r.len = ti_row_len(r.len, sp.seq_len);
  r.staged = sp.mode == 1 && sp.n_seg + 1 <= kTiSegCap;
  if (r.staged && r.live)
    for (int64_t i = threadIdx.x; i <= sp.n_seg; i += kTiThreads) {
      seg_lds[i] = sp.seg_offsets[i];
      if (i < sp.n_seg) stage_src(i);
    }
  r.n_cu = ti_cu_entries(sp.n_seg, cu_cap);
  // cu_seqlens is int32 by its consumers' contract: a batch's own stream stays below 2^31 tokens (the ops refuse
  // more). A flat stream that starts further into a buffer gets the low 32 bits, which is no contract.
  if (sp.cu_seqlens_out != nullptr && bx == 0)  // owned copy of the sequence starts (cu_seqlens)
    for (int64_t i = threadIdx.x; i <= r.n_cu; i += kTiThreads)
      sp.cu_seqlens_out[i] = static_cast<int32_t>(sp.seg_offsets[i]);
  __syncthreads();
  return r;
}

// The store half: 4 values of every output at (row, p0), as vectors where ti_vector_store allows. lab: the lane's
// 4 next-token labels, read (and stored, widened to i64: 2 x 16 B) only where sp.labels is set (block-uniform)
__device__ __forceinline__ void ti_store4(const TokenSpec& sp, int64_t row, int64_t p0, const int32_t* tok,
                                          const int32_t* pos, const int32_t* seg, const uint8_t* msk,
                                          const int32_t* lab) {
  const int64_t S = sp.seq_len;
  const int64_t o = row * S + p0;
  if (ti_vector_store(p0, S)) {
    *reinterpret_cast<int4*>(sp.out_tokens + o) = make_int4(tok[0], tok[1], tok[2], tok[3]);
    if (sp.attn_mask) {
      const uint32_t m = msk[0] | (msk[1] << 8) | (msk[2] << 16) | (static_cast<uint32_t>(msk[3]) << 24);
      *reinterpret_cast<uint32_t*>(sp.attn_mask + o) = m;
    }
    if (sp.position_ids) {
      if (sp.pos_is_i64) {
        int64_t* pp = static_cast<int64_t*>(sp.position_ids) + o;
        *reinterpret_cast<longlong2*>(pp) = make_longlong2(pos[0], pos[1]);
        *reinterpret_cast<longlong2*>(pp + 2) = make_longlong2(pos[2], pos[3]);
      } else {
        *reinterpret_cast<int4*>(static_cast<int32_t*>(sp.position_ids) + o) =
            make_int4(pos[0], pos[1], pos[2], pos[3]);
      }
    }
    if (sp.segment_ids)
      *reinterpret_cast<int4*>(sp.segment_ids + o) = make_int4(seg[0], seg[1], seg[2], seg[3]);
    if (sp.labels) {
      *reinterpret_cast<longlong2*>(sp.labels + o) = make_longlong2(lab[0], lab[1]);
      *reinterpret_cast<longlong2*>(sp.labels + o + 2) = make_longlong2(lab[2], lab[3]);
    }
  } else {
    for (int k = 0; k < kTiLane && p0 + k < S; ++k) {
      sp.out_tokens[o + k] = tok[k];
      if (sp.attn_mask) sp.attn_mask[o + k] = msk[k];
      if (sp.position_ids) {
        if (sp.pos_is_i64)
          static_cast<int64_t*>(sp.position_ids)[o + k] = pos[k];
        else
          static_cast<int32_t*>(sp.position_ids)[o + k] = pos[k];
      }
      if (sp.segment_ids) sp.segment_ids[o + k] = seg[k];
      if (sp.labels) sp.labels[o + k] = lab[k];
    }
  }
}

}  // namespace ddl
