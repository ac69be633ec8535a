// Fill-in-the-middle rearrangement of a rendered token batch: a share of the segments of a [R, S] batch rewritten as
// <PRE> prefix <SUF> suffix <MID> middle (PSM) or <PRE> <SUF> suffix <MID> prefix middle (SPM), keyed by counter-based
// hashes of the segment's key and the epoch's key. All the arithmetic is tokens_fim.h; a second ids buffer is written,
// so a lane may read any column of its row while its neighbours write.
//
// Geometry of the emit kernels (tokens_indexed.h): one workgroup per (row, chunk of kTiSpan = 512 positions), a lane
// = 4 consecutive positions. A lane loads its 4 ids, segment ids and position ids (16-byte loads where
// ti_vector_store allows), computes the parameters of each distinct segment among them once (cu_seqlens[s],
// cu_seqlens[s + 1], seg_keys[s], the segment's last token where an EOD id is given, four draws), gathers the tokens
// that moved -- the map is piecewise contiguous, so neighbouring lanes mostly read neighbouring columns, out of lines
// the workgroup has just loaded -- and stores 16 B of ids and 2 x 16 B of labels: 4 + 4 + (4 or 8) B read and
// 4 (+ 8) B written per position.
//
// Bounded reads: ids / seg / pos at the lane's own positions p < S of row < rows; cu[s], cu[s + 1] and seg_keys[s]
// only for 0 <= s < cap; ids[row, col] only for 0 <= col < S (tf_lane4 asks for a column only inside a sound
// segment, which lies inside the row); counts[0]. Bounded writes: out and labels at the lane's own positions, each
// exactly once (the vector path only where all 4 positions are inside the row).
#include "common.h"
#include "launch.h"
#include "tokens_fim.h"

namespace ddl {
namespace {

// the lane's 4 values of an int32 or int64 [R, S] array at flat element o, widened
__device__ __forceinline__ void tf_load4(const void* base, bool is_i64, int64_t o, bool vec, int n, int64_t* v) {
  if (is_i64) {
    const int64_t* p = static_cast<const int64_t*>(base) + o;
    if (vec) {
      const longlong2 lo = *reinterpret_cast<const longlong2*>(p), hi = *reinterpret_cast<const longlong2*>(p + 2);
      v[0] = lo.x, v[1] = lo.y, v[2] = hi.x, v[3] = hi.y;
    } else {
#pragma unroll
      for (int k = 0; k < kTiLane; ++k)
        if (k < n) v[k] = p[k];
    }
  } else {
    const int32_t* p = static_cast<const int32_t*>(base) + o;
    if (vec) {
      const int4 q = *reinterpret_cast<const int4*>(p);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < kTiLane; ++k)
        if (k < n) v[k] = p[k];
    }
  }
}

__global__ void __launch_bounds__(kTiThreads) token_fim_kernel(TokenFimSpec sp, int32_t chunks) {
  int64_t row, p0;
  ti_lane_origin(blockIdx.x, chunks, static_cast<int>(threadIdx.x), &row, &p0);
  const int64_t S = sp.seq_len;
  if (row >= sp.rows || p0 >= S) return;
  const bool live = sp.counts == nullptr || sp.counts[0] >= 0;  // block-uniform
  const bool vec = ti_vector_store(p0, S);
  const int n = S - p0 < kTiLane ? static_cast<int>(S - p0) : kTiLane;
  const int64_t o = row * S + p0;
  const int32_t* rowp = sp.ids + row * S;
  int64_t seg[kTiLane] = {-1, -1, -1, -1}, pos[kTiLane] = {0, 0, 0, 0};
  int32_t own[kTiLane] = {0, 0, 0, 0};
  tf_load4(sp.seg, sp.seg_is_i64 != 0, o, vec, n, seg);
  tf_load4(sp.pos, sp.pos_is_i64 != 0, o, vec, n, pos);
  if (vec) {
    const int4 q = *reinterpret_cast<const int4*>(sp.ids + o);
    own[0] = q.x, own[1] = q.y, own[2] = q.z, own[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < kTiLane; ++k)
      if (k < n) own[k] = sp.ids[o + k];
  }
  int32_t out[kTiLane];
  int64_t lab[kTiLane];
  const bool labels = sp.labels != nullptr;
  tf_lane4(
      sp.fp, S, sp.cap, live, p0, seg, pos, own, [&](int64_t i) { return sp.cu[i]; },
      [&](int64_t s) { return sp.seg_keys[s]; }, [&](int64_t col) { return rowp[col]; }, labels, sp.ignore_index, out,
      lab);
  if (vec) {
    *reinterpret_cast<int4*>(sp.out + o) = make_int4(out[0], out[1], out[2], out[3]);
    if (labels) {
      *reinterpret_cast<longlong2*>(sp.labels + o) = make_longlong2(lab[0], lab[1]);
      *reinterpret_cast<longlong2*>(sp.labels + o + 2) = make_longlong2(lab[2], lab[3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kTiLane; ++k) {
      if (k >= n) continue;
      sp.out[o + k] = out[k];
      if (labels) sp.labels[o + k] = lab[k];
    }
  }
}

bool overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && x < y + static_cast<uintptr_t>(b_bytes) && y < x + static_cast<uintptr_t>(a_bytes);
}

}  // namespace

int token_fim(const TokenFimSpec& spec, hipStream_t st) {
  if (spec.rows < 1 || spec.seq_len < 1 || spec.cap < 0) return -2;
  if (spec.rows > 0x7FFFFFFF / spec.seq_len) return -2;  // a batch's positions fit the int32 cu_seqlens
  if (!spec.ids || !spec.seg || !spec.pos || !spec.out) return -2;
  if (spec.cap > 0 && (!spec.cu || !spec.seg_keys)) return -2;
  if (spec.fp.min_len < 4 || spec.fp.rate_q > (1u << 24) || spec.fp.spm_q > (1u << 24)) return -2;
  const int64_t n = spec.rows * spec.seq_len;
  const void* ins[3] = {spec.ids, spec.seg, spec.pos};
  const int64_t in_bytes[3] = {4 * n, (spec.seg_is_i64 ? 8 : 4) * n, (spec.pos_is_i64 ? 8 : 4) * n};
  for (int i = 0; i < 3; ++i)
    if (overlap(spec.out, 4 * n, ins[i], in_bytes[i]) || overlap(spec.labels, 8 * n, ins[i], in_bytes[i])) return -2;
  if (overlap(spec.out, 4 * n, spec.labels, 8 * n)) return -2;
  const uintptr_t seg_a = spec.seg_is_i64 ? 8 : 4, pos_a = spec.pos_is_i64 ? 8 : 4;
  const bool vec = spec.seq_len % kTiLane == 0;  // 16-byte loads and stores
  if (reinterpret_cast<uintptr_t>(spec.ids) % (vec ? 16 : 4) || reinterpret_cast<uintptr_t>(spec.out) % (vec ? 16 : 4) ||
      reinterpret_cast<uintptr_t>(spec.seg) % (vec ? 16 : seg_a) ||
      reinterpret_cast<uintptr_t>(spec.pos) % (vec ? 16 : pos_a) ||
      reinterpret_cast<uintptr_t>(spec.labels) % (vec ? 16 : 8) || reinterpret_cast<uintptr_t>(spec.cu) % 4 ||
      reinterpret_cast<uintptr_t>(spec.seg_keys) % 8 || reinterpret_cast<uintptr_t>(spec.counts) % 8)
    return -2;
  const int64_t grid = ti_grid(spec.rows, 0, spec.seq_len, false);
  if (grid < 0) return -4;
  hipLaunchKernelGGL(token_fim_kernel, dim3(static_cast<uint32_t>(grid)), dim3(kTiThreads), 0, st, spec,
                     static_cast<int32_t>(ti_chunks(spec.seq_len)));
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
