// Index arithmetic of the pad/pack kernels, shared with host code. The constants, the grid, the lane origin, the
// row length, the vector-store predicate and the search serve the flat kernel (tokens.hip) and the indexed one
// (tokens_indexed.hip) alike (their shared device half is tokens_emit.h); ti_lane4 is the indexed kernel's lane
// loop, which csrc/kernels/tests/tokens_indexed_check.cpp replays under ASan/UBSan; ti_labels4 is its next-token
// label arithmetic (tests/token_labels_check.cpp). Both checks share their harness, tests/check_common.h.
// Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of HIP).
//
// The indexed kernel writes what pad_pack_tokens (tokens.hip) writes for the VIRTUAL flat stream
//   concat(corpus[src_start[i] : src_start[i] + len_i]),   len_i = offsets[i + 1] - offsets[i],
// which never exists: a token is read from the corpus at
//   pad mode   corpus[src_start[row] + p]                     p < min(len_row, S)
//   pack mode  corpus[seg_src[s] + g - seg_offsets[s]]        g = row_start[row] + p < row_end[row], g in segment s
// (seg_src[s] = the corpus element of segment s's first token; row_start / row_end / seg_offsets are positions
// of the virtual stream, exactly the pack plan pad_pack_tokens takes).
// One workgroup = (row, chunk of kTiSpan positions); a lane = 4 consecutive positions.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DDL_TI_HD __host__ __device__ __forceinline__
#else
#define DDL_TI_HD inline
#endif

namespace ddl {

constexpr int kTiThreads = 128;             // lanes per workgroup
constexpr int kTiLane = 4;                  // positions per lane (one 16-byte store of int32)
constexpr int kTiSpan = kTiThreads * kTiLane;  // positions per workgroup
constexpr int kTiSegCap = 1024;             // segment starts (and their corpus elements) staged in LDS: 2 x 8 KB

// chunks of kTiSpan positions per row
DDL_TI_HD int64_t ti_chunks(int64_t seq_len) { return (seq_len + kTiSpan - 1) / kTiSpan; }

// workgroups of a launch: one per (row, chunk), at least one when block 0 has cu_seqlens to write; -1: the
// grid does not fit 31 bits. The test is rows >= 2^31 / chunks: where chunks does not divide 2^31 it also refuses
// the last fewer-than-chunks grids below 2^31, which pad_pack_tokens' former rows * chunks >= 2^31 let through
// (about 2^31 workgroups: 18 TB of outputs, beyond any device)
DDL_TI_HD int64_t ti_grid(int64_t rows, int64_t fill_rows, int64_t seq_len, bool has_cu) {
  const int64_t r = fill_rows > rows ? fill_rows : rows;
  const int64_t chunks = ti_chunks(seq_len);
  if (r > 0 && chunks > 0 && r >= (int64_t{1} << 31) / chunks) return -1;
  const int64_t g = r > 0 ? r * chunks : 0;
  return g == 0 && has_cu ? 1 : g;
}

// block 0 copies seg_offsets[0 .. n] into cu_seqlens: n = n_seg, held inside the capacity where one is given
// (cu_cap > 0: cu_seqlens has cu_cap + 1 entries; the entries (n, cu_cap] are then written as seg_offsets[n])
DDL_TI_HD int64_t ti_cu_entries(int64_t n_seg, int64_t cu_cap) { return cu_cap > 0 && n_seg > cu_cap ? cu_cap : n_seg; }

// workgroup bx, lane tid -> row and the lane's first position
DDL_TI_HD void ti_lane_origin(uint32_t bx, int32_t chunks, int tid, int64_t* row, int64_t* p0) {
  const uint32_t r = bx / static_cast<uint32_t>(chunks);
  *row = static_cast<int64_t>(r);
  *p0 = static_cast<int64_t>(bx - r * static_cast<uint32_t>(chunks)) * kTiSpan + static_cast<int64_t>(tid) * kTiLane;
}

// tokens of a row that are written as data: its span, truncated to the row width
DDL_TI_HD int64_t ti_row_len(int64_t len, int64_t seq_len) {
  if (len > seq_len) len = seq_len;
  return len < 0 ? 0 : len;
}

// the lane's 4 positions go out as vectors (16 B ids) iff they all lie in the row and rows keep 16-byte alignment
DDL_TI_HD bool ti_vector_store(int64_t p0, int64_t seq_len) { return p0 + kTiLane <= seq_len && seq_len % kTiLane == 0; }

// index of the last entry <= v of the sorted a[0..n) (a[0] <= v)
template <typename At>
DDL_TI_HD int64_t ti_last_le(At at, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (at(mid) <= v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - 1;
}

// What one lane writes at positions p0 .. p0 + 3 of its row, and where it reads
struct TiLane4 {
  int64_t src[kTiLane];  // corpus element of the token, -1: padding (nothing is read)
  int32_t pos[kTiLane];
  int32_t seg[kTiLane];
  uint8_t msk[kTiLane];
};

// mode 0 (pad): the row is sequence `row`: start = its first position of the virtual stream (unused), src0 =
// src_start[row]. mode 1 (pack): start = row_start[row]; seg_at(i) = seg_offsets[i], i <= n_seg, src_at(i) =
// seg_src[i], i < n_seg. len = ti_row_len(...) of the row. The segment is searched once per lane, then advanced.
template <typename SegAt, typename SrcAt>
DDL_TI_HD void ti_lane4(int mode, int64_t p0, int64_t start, int64_t len, int64_t src0, int64_t n_seg, SegAt seg_at,
                        SrcAt src_at, TiLane4* out) {
  int64_t s = -1;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < kTiLane; ++k) {
    const int64_t p = p0 + k;
    const bool valid = p < len;
    out->msk[k] = valid ? 1 : 0;
    out->src[k] = -1;
    out->pos[k] = 0;
    out->seg[k] = mode == 0 ? 0 : -1;
    if (!valid) continue;
    if (mode == 0) {
      out->src[k] = src0 + p;
      out->pos[k] = static_cast<int32_t>(p);
    } else {
      const int64_t g = start + p;  // position in the virtual stream
      if (s < 0) {  // a plan's g lies in [seg_offsets[0], seg_offsets[n_seg]): 0 <= s < n_seg (kept so regardless)
        s = ti_last_le(seg_at, n_seg, g);
        if (s < 0) s = 0;
      } else {
        while (s + 1 < n_seg && seg_at(s + 1) <= g) ++s;
      }
      const int64_t in_seg = g - seg_at(s);
      out->src[k] = src_at(s) + in_seg;
      out->pos[k] = static_cast<int32_t>(in_seg);
      out->seg[k] = static_cast<int32_t>(s);
    }
  }
}

// Next-token labels of the lane's 4 positions: position p has a target iff p + 1 is a data position of the row
// (p + 1 < len <= S) and, in pack mode, of p's segment; every other label is the caller's ignore_index.
struct TiLabel4 {
  uint8_t has[kTiLane];  // 1: the label of p0 + k is the token at p0 + k + 1 (k < 3: the lane's own token k + 1)
  int64_t src4;          // has[3]: the corpus element of the token at p0 + 4, else -1 (nothing is read)
};

// `ln` = ti_lane4 of the same arguments. The token at p0 + 4 of the same segment is corpus element ln.src[3] + 1:
// in pad mode p0 + 4 < len_row, in pack mode g + 1 < seg_at(s + 1) (entry n_seg exists), so it lies inside the
// selected sequence that position p0 + 3 was read from, and the kernel's bounded-reads contract holds.
template <typename SegAt>
DDL_TI_HD void ti_labels4(int mode, int64_t p0, int64_t start, int64_t len, SegAt seg_at, const TiLane4& ln,
                          TiLabel4* out) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k + 1 < kTiLane; ++k)
    out->has[k] = ln.msk[k + 1] != 0 && (mode == 0 || ln.seg[k + 1] == ln.seg[k]) ? 1 : 0;
  const int64_t p4 = p0 + kTiLane;
  bool has = p4 < len;  // then p0 + 3 is data as well: ln.src[3] and (pack mode) ln.seg[3] are its
  if (has && mode != 0) has = start + p4 < seg_at(static_cast<int64_t>(ln.seg[kTiLane - 1]) + 1);
  out->has[kTiLane - 1] = has ? 1 : 0;
  out->src4 = has ? ln.src[kTiLane - 1] + 1 : -1;
}

}  // namespace ddl
