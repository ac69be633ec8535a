// Host-side launchers of the ddl_amd gfx950 kernels. Every launcher enqueues on
// the given stream, never synchronises, never allocates (graph-capturable,
// guide G9) and returns 0 or a hipError_t / negative argument error.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "tokens_fim.h"
#include "tokens_mix.h"

namespace ddl {

// permute.hip ---------------------------------------------------------------
// dst[r, :] = cast(src[source_row(ri, r), :]) (scatter=0)
// dst[source_row(ri, r), :] = src[r, :]       (scatter=1, same dtype only)
// scatter | kHostSource: src is pinned, device-mapped host memory (a zero-copy gather): plain loads; device
// sources are gathered with non-temporal loads (they stream through once; the fresh batch stays in the MALL)
// max_blocks > 0 caps the grid (grid-stride over tiles), e.g. to keep a
// zero-copy gather out of pinned host memory on a few CUs.
constexpr int kHostSource = 2;
int gather_rows(void* dst, int32_t out_dt, const void* src, int32_t in_dt, int64_t n_rows, int64_t row_elems,
                const RowIndex& ri, const Affine& aff, int scatter, int64_t max_blocks, hipStream_t st);
// out[i] = feistel_perm(base + i), i < count
int feistel_indices(int64_t* out, int64_t count, int64_t base, const FeistelKeys& keys, hipStream_t st);

// collate.hip ---------------------------------------------------------------
// Image collate: src [B, H*W, C] (HWC, u8 / f32 / bf16) -> dst [B, C, H*W]
// bf16 / f32 with out = x * scale[c] + bias[c]; rows gathered through ri.
// Checked in this order, all before anything is launched: ri and channels (-2), the input then the output
// dtype (-1), the LDS a tile needs (-5), the grid (-4).
int collate_hwc_to_chw(void* dst, int32_t out_dt, const void* src, int32_t in_dt, int64_t batch, int64_t pixels,
                       int32_t channels, const RowIndex& ri, const Affine& aff, hipStream_t st);
// Column-group split of a [n, nValues] row batch into up to 8 contiguous
// outputs dst_k [n, width_k] (reference tuple-of-splits batches,
// ddl/mpi_dataloader.py:195-196, made contiguous), with fused gather + cast.
struct SplitSpec {
  void* dst[8];
  int32_t width[8];
  int32_t n_groups;
  int32_t out_dt;
  // split only: rows land in consecutive output slots of slot_rows rows, slot_stride bytes apart
  // (a whole window's batches in one launch); 0 = one contiguous [n_rows, width] block per group
  int64_t slot_rows;
  int64_t slot_stride;
};
int split_columns(const SplitSpec& spec, const void* src, int32_t in_dt, int64_t n_rows, int64_t n_values,
                  const RowIndex& ri, hipStream_t st);
// Inverse: spec.dst[g] are the SOURCE groups [*, width[g]] (dtype in_dt), dst is [n_rows, n_values] of
// spec.out_dt; row r of dst is row source_row(ri, r) of every group.
int pack_columns(const SplitSpec& spec, void* dst, int32_t in_dt, int64_t n_rows, int64_t n_values,
                 const RowIndex& ri, hipStream_t st);

// augment.hip ---------------------------------------------------------------
// RandomResizedCrop (+ flip, + per-channel affine, + cast) of gathered images:
// src rows [in_h, in_w, C] (hwc=1) or [C, in_h, in_w]; out [B, C, out_h, out_w].
// Crop parameters are drawn on the device from hash(seed, sample_base + source
// row) by a per-image pre-pass into boxes_out (required, [B, 5] int32 device
// buffer: y, x, h, w, flip), which the resampling kernel then reads.
struct AugmentSpec {
  uint64_t seed;
  int64_t sample_base;
  // optional [batch] crop keys (e.g. global sample ids of rows that were exchanged between ranks);
  // null: the key is sample_base + the image's source row
  const int64_t* sample_ids;
  int32_t in_h, in_w, out_h, out_w, channels;
  float scale_min, scale_max, ratio_min, ratio_max, flip_p;
};
struct CropBox {
  int32_t y, x, h, w, flip;
};
// Checked in this order, all before the boxes are drawn: ri (-2), boxes_out (-3), the geometry and path (-2), the
// input then the output dtype (-1), the LDS path's budget (-5), the grid (-4). A refused call leaves boxes_out alone.
int random_resized_crop(void* dst, int32_t out_dt, const void* src, int32_t in_dt, int64_t batch,
                        const AugmentSpec& a, int hwc, const RowIndex& ri, const Affine& aff, int32_t* boxes_out,
                        int path, hipStream_t st);

// tokens.hip ----------------------------------------------------------------
// Pad: row b takes tokens[offsets[b] : offsets[b+1]] (truncated to seq_len);
// writes out_tokens [B, S] (pad_id fill), attn_mask [B, S] (u8 or null) and
// position_ids [B, S] (i32/i64 or null).
// Pack: row r holds the token span [row_start[r], row_end[r]) of the flat
// stream; seg_offsets (sorted sequence starts, n_seg+1 entries) drive the
// per-token position id (reset at every sequence start) and segment id.
struct TokenSpec {
  const void* tokens;          // int32 tokens, or uint16 when tok16 (narrow on the wire, widened here)
  const int64_t* offsets;      // pad mode: [B+1]
  const int64_t* row_start;    // pack mode: [R]
  const int64_t* row_end;      // pack mode: [R]
  const int64_t* seg_offsets;  // pack mode: [n_seg+1]
  int64_t n_seg;
  int32_t* out_tokens;
  uint8_t* attn_mask;
  void* position_ids;
  int32_t* segment_ids;        // pack mode only (or null)
  int32_t* cu_seqlens_out;     // pack mode: int32 copy of seg_offsets[0..n_seg] (varlen-attention ABI; or null)
  int64_t rows;
  int64_t seq_len;
  int32_t pad_id;
  int32_t pos_is_i64;
  int32_t mode;  // 0 pad, 1 pack
  int32_t tok16;  // 1: tokens are uint16 (vocabularies < 65536 cross PCIe at 2 B per token)
  // > rows: rows [rows, fill_rows) are written as padding (pad_id, mask 0, position 0, segment -1), so a
  // packed batch has a fixed shape [fill_rows, seq_len] (static shapes for graphs / compiled steps)
  int64_t fill_rows;
  // pack mode, plan built on the device (pack_plan_device): {n_rows, n_seg} read by the kernel instead of
  // `rows` / `n_seg`, so plan and pack are two launches with no host round trip (fill_rows = the plan's
  // row capacity; n_rows < 0, an overflowed plan, writes every row as padding)
  const int64_t* dev_counts;
  // next-token labels [R, S] i64 (or null: off), what cross_entropy(ignore_index) takes: labels[r, p] =
  // out_tokens[r, p + 1] where p + 1 is a data position of the same row and (pack mode) of the same segment,
  // ignore_index everywhere else (a row's last position, a segment's last token, padding positions and rows)
  int64_t* labels;
  int32_t ignore_index;
};
int pad_pack_tokens(const TokenSpec& spec, hipStream_t st);

// In-order greedy packing plan of B ragged sequences, computed on the device (one workgroup): the same
// plan as the host's pack_plan (runtime/arena.cpp). Sequences longer than seq_len are split into seq_len
// segments; row r = segments [P(r), P(r + 1)) where P(r + 1) = the furthest segment end within seq_len of
// P(r)'s start. The row starts are the orbit of segment 0 under that jump, built by pointer doubling
// (orbit[2^t + i] = jump^(2^t)(orbit[i])), log2(rows) rounds instead of a rows-long dependent chain.
struct PackPlanSpec {
  const int64_t* offsets;  // [n + 1] flat token offsets of the sequences
  int64_t n;
  int64_t seq_len;
  int64_t max_segs;      // seg_offsets holds max_segs + 1 entries
  int64_t max_rows;      // row_start / row_end hold max_rows entries
  int64_t* seg_offsets;  // out: segment starts + the end
  int64_t* row_start;    // out
  int64_t* row_end;      // out
  int64_t* counts;       // out: {n_rows, n_seg}; n_rows = -1 when a capacity was exceeded
  int32_t* scratch;      // >= pack_plan_scratch_ints(max_segs, max_rows) ints (used when LDS is too small)
};
int64_t pack_plan_scratch_ints(int64_t max_segs, int64_t max_rows);
int pack_plan_device(const PackPlanSpec& spec, hipStream_t st);
// Several independent token batches (the sub-batches of one multi-batch window) in one launch per
// kMaxTokenSubs of them: grid.y = sub-batch.
constexpr int kMaxTokenSubs = 16;
int pad_pack_tokens_multi(const TokenSpec* specs, int n, hipStream_t st);

// tokens_indexed.hip --------------------------------------------------------
// pad_pack_tokens for the virtual flat stream concat(corpus[src_start[i] : src_start[i] + len_i]), every token
// read from the corpus (HBM) instead: spec.tokens is null, the plan arrays (offsets [B + 1] in pad mode,
// row_start / row_end / seg_offsets in pack mode) are positions of that virtual stream as for pad_pack_tokens.
// corpus: int32, or uint16 when spec.tok16, corpus_elems elements; src_start [B] (pad mode) and seg_src
// [n_seg] (pack mode: the corpus element of each segment's first token) are device-readable. Outputs of a row
// width that is a multiple of 4 must be 16-byte aligned (the mask 4-byte; the labels 16, like i64 position ids).
// Block 0 writes cu_seqlens_out even when there is no row.
// A plan built on the device (pack mode, spec.dev_counts = pack_plan_device's counts): the kernel reads
// {n_rows, n_seg} there instead of spec.rows / spec.n_seg, the grid is sized by spec.fill_rows (> 0, the plan's
// row capacity) and n_rows < 0, an overflowed plan, writes every row as padding.
// cu_cap > 0: cu_seqlens_out holds cu_cap + 1 entries, and the entries (n_seg, cu_cap] are written as
// seg_offsets[n_seg], the token count: a fixed-capacity cu_seqlens describes zero-length trailing sequences.
int pad_pack_tokens_indexed(const TokenSpec& spec, const void* corpus, int64_t corpus_elems, const int64_t* src_start,
                            const int64_t* seg_src, hipStream_t st, int64_t cu_cap = 0);

// tokens_plan.hip -----------------------------------------------------------
// The descriptor of a token batch, built on the device (one workgroup): sequence i of the batch is corpus
// sequence q_i = source_row(ri, i) (identity base + i, an explicit device index, or the Feistel permutation
// of position base + i), i.e. corpus elements [corpus_offsets[q_i], corpus_offsets[q_i + 1]). Writes what
// pack_plan_device and pad_pack_tokens_indexed take: src_start [n], offsets [n + 1] (the exclusive scan of the
// lengths: the virtual flat stream) and seg_src [max_segs] (segment j of sequence i = src_start[i] + j *
// seq_len, numbered by the exclusive scan of ceil(len_i / seq_len) as pack_plan_device numbers seg_offsets),
// counts[2] = the token count and counts[3] = the longest segment, min(max len, seq_len). counts[0 .. 1] are
// pack_plan_device's; pad_counts != 0 (no plan follows) writes them as {n, 0}. Segments past max_segs are not
// written (pack_plan_device reports the overflow); an index outside [0, n_corpus) is an empty sequence.
struct BatchDescSpec {
  const int64_t* corpus_offsets;  // [n_corpus + 1], device
  int64_t n_corpus;
  RowIndex ri;
  int64_t n;
  int64_t seq_len;
  int64_t max_segs;
  int64_t* src_start;
  int64_t* offsets;
  int64_t* seg_src;
  int64_t* counts;  // [4]
  int32_t pad_counts;
  int32_t pad;
};
int token_batch_descriptor(const BatchDescSpec& spec, hipStream_t st);

// tokens_ffd.hip ------------------------------------------------------------
// The first-fit-decreasing order of a token batch, built on the device (one workgroup; tokens_ffd.h): of the n
// sequences the selector names (as BatchDescSpec names them, lengths by the same rules), index_out [n] = their
// corpus indices in the order of ffd_if_it_wins -- the first-fit-decreasing order when it packs rows of seq_len
// tokens into fewer rows than the given order does, else the given order -- and counts = [ffd_rows,
// in_order_rows, used (1: the FFD order, 0: the given one)]. token_batch_descriptor then takes index_out as an
// explicit index. n <= kFfdMaxSeqs (4096), else -2. n = 0 writes only the counts.
struct FfdOrderSpec {
  const int64_t* corpus_offsets;  // [n_corpus + 1], device
  int64_t n_corpus;
  RowIndex ri;
  int64_t n;
  int64_t seq_len;
  int64_t* index_out;  // [n]
  int64_t* counts;     // [3]
};
int token_ffd_order(const FfdOrderSpec& spec, hipStream_t st);

// tokens_stream.hip ---------------------------------------------------------
// The token stream of an epoch: concat(document q_0 .. q_{n-1}), q_k = source_row(ri, k) (the Feistel order of
// the epoch, an explicit device index, or the identity), cut into rows of seq_len tokens.
// token_stream_table: table[i] = the tokens in front of document i, i = 0 .. n (table[n] = the stream's length):
// a device-wide exclusive scan, three launches on `st` (tile sums, the scan of the tile sums by one workgroup,
// the tiles' scans), no atomics and no waiting between workgroups. tile_sums: token_stream_table_scratch(n)
// int64 of device scratch. An index outside [0, n_corpus) is an empty document.
struct StreamTableSpec {
  const int64_t* corpus_offsets;  // [n_corpus + 1], device
  int64_t n_corpus;
  RowIndex ri;
  int64_t n;          // documents of the order
  int64_t* table;     // out: [n + 1]
  int64_t* tile_sums; // scratch
};
int64_t token_stream_table_scratch(int64_t n);
int token_stream_table(const StreamTableSpec& spec, hipStream_t st);
// What both stream plans read and write. Either turns `rows` rows of seq_len tokens of the stream into the pack plan
// pad_pack_tokens_indexed takes in pack mode with dev_counts = counts, fill_rows = rows, cu_cap = max_segs. A segment
// is a maximal run of one document inside one row, numbered row-major over the batch's rows: seg_offsets[k] = its
// first token's position in the batch (entry n_seg = the batch's tokens), seg_src[k] = the corpus element of that
// token; row_start / row_end [rows] = the rows' limits in the batch; counts = {rows or -1, n_seg, tokens, longest
// segment}. counts[0] = -1 marks a plan that cannot be rendered, n_seg > max_segs among them: nothing is written
// past the capacity, and pad_pack_tokens_indexed then writes padding.
struct StreamPlanOut {
  const int64_t* table;           // [n + 1], token_stream_table of the same ri and n
  const int64_t* corpus_offsets;  // [n_corpus + 1], device
  int64_t n_corpus;
  RowIndex ri;  // the documents' order
  int64_t n;
  int64_t rows;
  int64_t seq_len;
  int64_t max_segs;      // seg_offsets holds max_segs + 1 entries, seg_src max_segs
  int64_t* seg_offsets;  // out
  int64_t* seg_src;      // out
  int64_t* row_start;    // out: [rows]
  int64_t* row_end;      // out: [rows]
  int64_t* counts;       // out: [4]
};
// the argument checks both launchers make before their own (a failure is the argument error -2)
inline bool ts_plan_args_ok(const StreamPlanOut& p) {
  if (p.n < 0 || p.n_corpus < 0 || p.seq_len <= 0 || p.rows < 1 || p.max_segs < 1) return false;
  if (!p.table || !p.seg_offsets || !p.seg_src || !p.row_start || !p.row_end || !p.counts) return false;
  if (p.n_corpus > 0 && !p.corpus_offsets) return false;
  if (p.rows > 0x7FFFFFFF / p.seq_len) return false;  // a batch's positions fit the int32 cu_seqlens
  return row_index_ok(p.ri, p.n);
}
// token_stream_plan (one workgroup): rows [row_base, row_base + rows) of the stream, i.e. the window [T0, T1) =
// [row_base * seq_len, min((row_base + rows) * seq_len, table[n])). Segment starts are relative to T0, the rows'
// limits are clamped to the window's tokens, counts[0] = the rows holding a token.
struct StreamPlanSpec {
  StreamPlanOut p;
  int64_t row_base;
};
int token_stream_plan(const StreamPlanSpec& spec, hipStream_t st);

// tokens_stream_rows.hip ----------------------------------------------------
// token_stream_plan for rows picked anywhere in the stream: batch row k is stream row rho_k = source_row(rows_ri,
// k) (mode 0: base + k; mode 1: a device index of `rows` entries, repeats allowed; mode 2: a Feistel permutation of
// [0, stream_rows) at position base + k), i.e. the window [rho_k * seq_len, (rho_k + 1) * seq_len). Two launches on
// `st` of ceil(rows / 16) workgroups, one wave per row (the rows' documents counted, then the plan written behind
// a per-workgroup reduction of the counts): no atomics, no waiting between workgroups. row_start / row_end [k] =
// k * seq_len, (k + 1) * seq_len, counts = {rows, n_seg, rows * seq_len, longest segment}. Only full rows can be
// selected: rho_k < 0 or (rho_k + 1) * seq_len > table[n] makes the batch invalid -- counts[0] = -1 and
// counts[1 .. 3] taken over the valid rows, seg_offsets[0] = 0 and no other segment entry written.
struct StreamRowsSpec {
  StreamPlanOut p;
  RowIndex rows_ri;     // the rows' selection
  int64_t stream_rows;  // the full rows of the stream as the host knows them, the domain a mode 2 rows_ri must have
  int64_t* scratch;     // [4 * rows] int64 of device memory between the two launches
};
int token_stream_plan_rows(const StreamRowsSpec& spec, hipStream_t st);

// tokens_mix.hip ------------------------------------------------------------
// The document order of one epoch of a weighted mixture of corpus parts (tokens_mix.h has the definition):
// order[i], i < n, is a corpus document id, a document of part p appearing floor(repeat_p) or one more times. The
// order is what token_stream_table and the two stream plans take as an explicit index (RowIndex mode 1, n =
// the order's length). One launch, one thread and one 8-byte store per entry; the whole spec travels as the kernel's
// argument, nothing is uploaded. ri: the epoch's permutation of [0, n) (mode 2, base 0), the identity, or an
// explicit index of n values; inner_shuffle != 0: keys[p] is part p's fixed permutation of its n_docs documents
// (checked for every part with extra documents), 0: the identity.
struct MixOrderSpec {
  RowIndex ri;
  int32_t parts;
  int32_t inner_shuffle;
  int64_t n_corpus;
  int64_t cbase[kMixMaxParts + 1];
  MixPart part[kMixMaxParts];
  FeistelKeys keys[kMixMaxParts];
  int64_t n;       // entries of the order = cbase[parts]
  int64_t* order;  // out: [n], device
};
int token_mix_order(const MixOrderSpec& spec, hipStream_t st);

// tokens_fim.hip ------------------------------------------------------------
// Fill-in-the-middle rearrangement of a rendered token batch (tokens_fim.h has the definition): every sound segment
// of ids [rows, seq_len] whose draw selects it is written rearranged into out, every other position is copied;
// labels (null: none) are the next-token labels of out. seg / pos: the batch's segment and position ids, int32 or
// int64; cu [cap + 1]: cu_seqlens; seg_keys [cap]; counts (null: none): counts[0] < 0 marks a batch that is not
// rearranged. One workgroup per (row, chunk of 512 positions), 4 positions per lane. out and labels must not
// overlap the inputs; with seq_len a multiple of 4, ids, seg, pos, out and labels must be 16-byte aligned.
struct TokenFimSpec {
  FimParams fp;
  const int32_t* ids;
  const void* seg;
  const void* pos;
  int32_t seg_is_i64;
  int32_t pos_is_i64;
  const int32_t* cu;
  int64_t cap;
  const int64_t* seg_keys;
  const int64_t* counts;
  int32_t* out;
  int64_t* labels;
  int32_t ignore_index;
  int32_t pad;
  int64_t rows;
  int64_t seq_len;
};
int token_fim(const TokenFimSpec& spec, hipStream_t st);

// ragged.hip ----------------------------------------------------------------
// Device twin of the host gather_ragged: sequence i (src_start[i] elements into src, dst_offsets[i + 1] -
// dst_offsets[i] elements of elem_bytes = 2 or 4) -> dst[dst_offsets[i] ...). src: HBM or pinned,
// device-mapped host memory (16-byte aligned non-temporal loads of each sequence's aligned hull; nothing
// outside the hulls is read); dst: HBM. tile_start[n + 1] / n_tiles: the tile map of ragged_index.h
// (ragged_tile_plan, host-built); the three arrays are device-readable. max_blocks > 0 caps the grid.
// n == 0 or n_tiles == 0 launches nothing.
constexpr int kRaggedMapCap = 2047;  // sequences whose tile map (n + 1 int32) is searched in LDS
int gather_ragged(void* dst, const void* src, const int64_t* src_start, const int64_t* dst_offsets,
                  const int32_t* tile_start, int64_t n, int64_t n_tiles, int elem_bytes, int64_t max_blocks,
                  hipStream_t st);

// tokens_stream_gather.hip --------------------------------------------------
// The tokens of a stream plan (StreamPlanOut of either plan kernel: seg_src [max_segs], seg_offsets [max_segs + 1],
// counts) copied into the flat window dst [rows * seq_len] of elem_bytes = 2 or 4 byte elements in HBM:
// dst[g] = src[seg_src[s] + g - seg_offsets[s]] for seg_offsets[s] <= g < seg_offsets[s + 1], s < n_seg = counts[1];
// positions at or past seg_offsets[n_seg] are not written, and a plan with counts[0] < 0, n_seg = 0 or n_seg >
// max_segs writes nothing. src: HBM or pinned, device-mapped host memory of corpus_elems elements (16-byte aligned
// non-temporal loads of the pieces' aligned hulls; a piece outside [0, corpus_elems) is not dereferenced). The grid is
// static -- the chunks of rows * seq_len elements, the kernel reads the counts -- and max_blocks > 0 caps it.
// pad_pack_tokens_indexed renders the batch from dst with corpus = dst, corpus_elems = rows * seq_len and seg_src =
// seg_offsets.
int gather_stream_pieces(void* dst, const void* src, int64_t corpus_elems, const int64_t* seg_src,
                         const int64_t* seg_offsets, const int64_t* counts, int64_t max_segs, int64_t rows,
                         int64_t seq_len, int elem_bytes, int64_t max_blocks, hipStream_t st);

// bucket.hip ----------------------------------------------------------------
// Owner bucketing of a global batch for the resident loader's exchange: positions
// [pos0, pos0 + count) of the Feistel permutation `keys`, sample idx owned by rank
// idx / shard_rows. bucket_send writes this rank's samples (idx - lo) in position
// order (count = GB); bucket_recv maps each position of this rank's slice
// (count = LB) to its row in the all-to-all receive buffer, whose block from
// source q starts at offsets[q].
constexpr int kMaxBucketWorld = 64;
struct BucketSpec {
  FeistelKeys keys;
  int64_t pos0;
  int64_t count;
  int64_t shard_rows;
  int64_t lo;
  int32_t rank;
  int32_t world;
  int64_t offsets[kMaxBucketWorld];
};
int bucket_send(const BucketSpec& sp, int64_t* send_rows, hipStream_t st);
int bucket_recv(const BucketSpec& sp, int64_t* inv, hipStream_t st);

// misc.hip ------------------------------------------------------------------
// Sum of the 32-bit words of [ptr, ptr+bytes) added into *out (u64). Two
// stages through `scratch` (>= kChecksumMaxBlocks u64). Debug batch checksums
// and the bench consumer step.
constexpr int64_t kChecksumMaxBlocks = 1024;
// Streaming 16 B copy (bandwidth roofline probe); bytes and both pointers 16 B aligned.
int stream_copy(const void* src, void* dst, int64_t bytes, int blocks, hipStream_t st);
// One 4 B read per `page` bytes of [ptr, ptr + bytes) (e.g. a host-mapped source before zero-copy gathers);
// sink >= blocks u32 (device memory).
int touch_pages(const void* ptr, int64_t bytes, int64_t page, uint32_t* sink, int blocks, hipStream_t st);
int checksum_words(const void* ptr, int64_t bytes, uint64_t* out, uint64_t* scratch, int64_t scratch_len,
                   hipStream_t st);
// Streaming form: partials[b] += block b's share (grid = n_partials, fixed for the
// life of the accumulator); checksum_finalize adds sum(partials) into *out.
int checksum_accumulate(const void* ptr, int64_t bytes, uint64_t* partials, int64_t n_partials, hipStream_t st);
int checksum_finalize(const uint64_t* partials, int64_t n_partials, uint64_t* out, hipStream_t st);
// Per-column sum / sum of squares (float64, accumulated onto zeroed outputs) and min / max (float32, onto
// +inf / -inf) of an [n, cols] f32 matrix (reference harness normalisation stats, tests/run_ddl.py:45-77).
int column_stats(const float* src, int64_t n, int64_t cols, double* out_sum, double* out_sumsq, float* out_min,
                 float* out_max, hipStream_t st);

}  // namespace ddl
