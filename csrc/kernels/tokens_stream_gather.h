// Index arithmetic of the stream piece gather (tokens_stream_gather.hip), shared with host code:
// csrc/kernels/tests/tokens_stream_gather_check.cpp replays the kernel's per-lane loops with it under ASan/UBSan, in
// which only the wave collectives (the search of the chunk's first piece, the scan of the unit counts) have a host
// stand-in. Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of
// HIP).
//
// A stream plan (tokens_stream.h, tokens_stream_rows.h) cuts a batch of rows * S positions into n_seg pieces: piece s
// is the positions [seg_offsets[s], seg_offsets[s + 1]) and starts at corpus element seg_src[s]. The gather copies
//   dst[g] = corpus[seg_src[s] + (g - seg_offsets[s])]        seg_offsets[s] <= g < seg_offsets[s + 1], s < n_seg
// for g < limit = min(seg_offsets[n_seg], rows * S): the batch's tokens as one flat staging window.
// A CHUNK is kSgChunkBytes of that window (a destination range, the one thing the host can count); a workgroup finds
// the pieces that intersect its chunk, clips each to the chunk and reads the clipped piece as the 16-byte units of its
// aligned hull (ragged_index.h), first and last unit loaded whole and masked. A unit that straddles a chunk boundary
// inside a piece belongs to the hulls of both clipped halves and is loaded by both chunks: at most one 16-byte unit
// per piece and boundary, 16 bytes in kSgChunkBytes of link traffic.
// The pieces of a chunk are taken in GROUPS of kSgGroup, one piece per lane: the lanes' unit counts are scanned into
// LDS, and the group's units -- of however many pieces -- are then dealt to the lanes kRgUnroll at a time, a lane
// finding its unit's piece by a search of that prefix. Long pieces and short ones cost the same per unit.
#pragma once

#include <stdint.h>

#include "ragged_index.h"
#include "tokens_stream.h"

#define DDL_SG_HD DDL_RG_HD

namespace ddl {

constexpr int kSgChunkBytes = kRgTileUnits * kRgUnitBytes;  // 16 KB of the staging window per chunk: one pass of an
                                                            // aligned piece (kRgThreads lanes x kRgUnroll units)
constexpr int kSgGroup = kRgThreads;                        // pieces per group: one per lane

// destination elements of a chunk
DDL_SG_HD int64_t sg_chunk_elems(int eb) { return kSgChunkBytes / eb; }

// chunks of a window of `elems` elements (the launcher: elems = rows * S; the kernel: elems = limit)
DDL_SG_HD int64_t sg_chunks(int64_t elems, int eb) {
  return elems > 0 ? (elems + sg_chunk_elems(eb) - 1) / sg_chunk_elems(eb) : 0;
}

// The elements the gather writes: none for a plan that cannot be rendered (a negative row count), for no piece and
// for a piece count beyond the plan's capacity; else min(end, rows * S), `end` = seg_offsets[n_seg], with the plan's
// rows held inside the window's capacity `cap_rows`. n_seg is checked first: `end` is read only for a valid count.
DDL_SG_HD bool sg_plan_ok(int64_t n_rows, int64_t n_seg, int64_t max_segs) {
  return n_rows > 0 && n_seg > 0 && n_seg <= max_segs;
}
DDL_SG_HD int64_t sg_limit(int64_t n_rows, int64_t cap_rows, int64_t S, int64_t end) {
  const int64_t rows = n_rows < cap_rows ? n_rows : cap_rows;
  const int64_t cap = rows > 0 ? rows * S : 0;
  const int64_t lim = end < cap ? end : cap;
  return lim > 0 ? lim : 0;
}

// chunk c of a window of `limit` elements: the positions [*c0, *c1), not empty for c < sg_chunks(limit, eb)
DDL_SG_HD void sg_chunk(int64_t c, int64_t limit, int eb, int64_t* c0, int64_t* c1) {
  *c0 = c * sg_chunk_elems(eb);
  const int64_t e = *c0 + sg_chunk_elems(eb);
  *c1 = e < limit ? e : limit;
}

// One lane of a group: piece s clipped to the chunk [c0, c1)
struct SgPiece {
  uint64_t a;     // byte address of the clipped piece's first element (src + element * eb)
  int64_t d0;     // its first position of the window
  int64_t len;    // its elements, 0: nothing of it is read or written
  int64_t units;  // 16-byte units of its aligned hull
};

// seg_at(i) = seg_offsets[i], i <= n_seg; src_at(i) = seg_src[i], i < n_seg. s >= n_seg: no piece. A piece whose
// whole source range [seg_src[s], seg_src[s] + its length) is not inside [0, corpus_elems) -- a corrupt plan -- is
// not dereferenced: len = 0.
template <typename SegAt, typename SrcAt>
DDL_SG_HD SgPiece sg_piece(SegAt seg_at, SrcAt src_at, int64_t s, int64_t n_seg, int64_t c0, int64_t c1, uint64_t src,
                           int64_t corpus_elems, int eb) {
  SgPiece p{0, 0, 0, 0};
  if (s < 0 || s >= n_seg) return p;
  const int64_t lo = seg_at(s), hi = seg_at(s + 1);
  const int64_t g0 = lo > c0 ? lo : c0, g1 = hi < c1 ? hi : c1;
  if (g1 <= g0) return p;
  const int64_t e0 = src_at(s);
  if (e0 < 0 || e0 > corpus_elems || hi - lo > corpus_elems - e0) return p;
  p.a = src + static_cast<uint64_t>(e0 + (g0 - lo)) * static_cast<uint64_t>(eb);
  p.d0 = g0;
  p.len = g1 - g0;
  p.units = rg_units(p.a, p.len, eb);
  return p;
}

// unit w of a group's pass: round k of lane tid in the pass that starts at unit `base` (consecutive lanes:
// consecutive units, so the lanes of a long piece read consecutive 16-byte blocks)
DDL_SG_HD int64_t sg_unit(int64_t base, int k, int tid) { return base + static_cast<int64_t>(k) * kRgThreads + tid; }

// the piece of unit w < upre(cnt): the last j < cnt with upre(j) <= w, upre = the exclusive scan of the group's unit
// counts with entry cnt = their sum. Pieces without units share their successor's entry and are never selected.
template <typename At>
DDL_SG_HD int64_t sg_unit_piece(At upre, int64_t cnt, int64_t w) { return rg_find_seq(upre, cnt, w); }

}  // namespace ddl
