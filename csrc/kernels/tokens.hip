// Variable-length token collate (BASELINE config 4:
// seq_len = 4096 token sequences, on-device pad/pack).
//
// Pad mode: B ragged sequences -> [B, S] tokens padded with pad_id, a u8
// attention mask and position ids, truncated to S.
// Tokens arrive as int32, or as uint16 (tok16: vocabularies below 65536 ship 2 B per token over PCIe and
// are widened to int32 here, in the same pass).
// Pack mode: consecutive sequences are packed into rows of S tokens (plan
// computed on the host: row r = flat token span [row_start, row_end)); the
// position id restarts at every sequence boundary and a segment id marks
// which sequence a token belongs to (what varlen attention consumes).
//
// The grid, the prologue and the stores are tokens_emit.h / tokens_indexed.h, shared with the indexed kernel
// (tokens_indexed.hip). This file's part is the lane loop: a token is a plain load of tokens[start + p], whose
// address does not wait for the segment search -- no bounds check (the plan is the caller's and indexes its
// own stream), one LDS array (the segment starts; there is no second descriptor to stage). The indexed
// kernel's ti_lane4, which derives the element from the searched segment, made pack mode 18% slower here
// (profiles/token_refactor), so the two lane loops stay apart.
#include "common.h"
#include "launch.h"
#include "tokens_emit.h"

namespace ddl {
namespace {

template <typename At>
__device__ __forceinline__ void emit4(const TokenSpec& sp, const TiRow& r, At seg_at) {
  const int32_t* src = static_cast<const int32_t*>(sp.tokens) + r.start;
  const uint16_t* src16 = static_cast<const uint16_t*>(sp.tokens) + r.start;
  int32_t tok[kTiLane], pos[kTiLane], seg[kTiLane];
  uint8_t msk[kTiLane];
  int64_t s = -1;  // current sequence (pack mode): searched once, then advanced
#pragma unroll
  for (int k = 0; k < kTiLane; ++k) {
    const int64_t p = r.p0 + k;
    const bool valid = p < r.len;
    tok[k] = valid ? (sp.tok16 ? static_cast<int32_t>(src16[p]) : src[p]) : sp.pad_id;
    msk[k] = valid ? 1 : 0;
    if (sp.mode == 0) {
      pos[k] = valid ? static_cast<int32_t>(p) : 0;
      seg[k] = 0;
    } else if (valid) {
      const int64_t g = r.start + p;  // flat token index
      if (s < 0)
        s = ti_last_le(seg_at, sp.n_seg + 1, g);
      else
        while (s + 1 <= sp.n_seg && seg_at(s + 1) <= g) ++s;
      pos[k] = static_cast<int32_t>(g - seg_at(s));
      seg[k] = static_cast<int32_t>(s);
    } else {
      pos[k] = 0;
      seg[k] = -1;
    }
  }
  int32_t lab[kTiLane];
  if (sp.labels) {  // block-uniform, like attn_mask
    // position p's label is the token at p + 1 where that is data of the same row and (pack) segment: the lane's
    // own next token, and for its last position src[p0 + 4], one more load next to the fourth (p0 + 4 < len keeps
    // it inside the row's span of the stream; seg_at(s + 1) exists, s < n_seg being position p0 + 3's segment)
#pragma unroll
    for (int k = 0; k + 1 < kTiLane; ++k)
      lab[k] = msk[k + 1] && (sp.mode == 0 || seg[k + 1] == seg[k]) ? tok[k + 1] : sp.ignore_index;
    const int64_t p4 = r.p0 + kTiLane;
    bool has = p4 < r.len;
    if (has && sp.mode != 0) has = r.start + p4 < seg_at(s + 1);
    lab[kTiLane - 1] = has ? (sp.tok16 ? static_cast<int32_t>(src16[p4]) : src[p4]) : sp.ignore_index;
  }
  ti_store4(sp, r.row, r.p0, tok, pos, seg, msk, lab);
}

__device__ __forceinline__ void pad_pack_block(const TokenSpec& spec, uint32_t bx, int32_t chunks, int64_t* seg_lds) {
  TokenSpec sp = spec;
  const TiRow r = ti_prologue(sp, bx, chunks, seg_lds, 0, [](int64_t) {});
  if (!r.live || r.p0 >= sp.seq_len) return;
  if (r.staged)
    emit4(sp, r, [&](int64_t i) { return seg_lds[i]; });
  else
    emit4(sp, r, [&](int64_t i) { return sp.seg_offsets[i]; });
}

__global__ void __launch_bounds__(kTiThreads) pad_pack_kernel(TokenSpec sp, int32_t chunks) {
  __shared__ int64_t seg_lds[kTiSegCap];
  pad_pack_block(sp, blockIdx.x, chunks, seg_lds);
}

struct TokenMulti {
  TokenSpec sub[kMaxTokenSubs];
};

__global__ void __launch_bounds__(kTiThreads) pad_pack_multi_kernel(TokenMulti m, int32_t chunks) {
  __shared__ int64_t seg_lds[kTiSegCap];
  pad_pack_block(m.sub[blockIdx.y], blockIdx.x, chunks, seg_lds);
}

// ---- device packing plan (one workgroup) ----------------------------------------------------------------
constexpr int kPlanThreads = 1024;
constexpr int kPlanWaves = kPlanThreads / 64;
constexpr int64_t kPlanLdsInts = 12288;  // 48 KB of LDS for the jump tables + the orbit, else global scratch

__device__ __forceinline__ int64_t wave_incl_scan(int64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__global__ void __launch_bounds__(kPlanThreads) pack_plan_kernel(PackPlanSpec sp) {
  __shared__ int64_t wave_tot[kPlanWaves];
  __shared__ int64_t carry_s;
  __shared__ int32_t lds[kPlanLdsInts];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t S = sp.seq_len;
  if (t == 0) carry_s = 0;
  __syncthreads();
  // 1. segments: c_i = ceil(len_i / S) per sequence, exclusive scan over the sequences in 1024-wide tiles
  for (int64_t b = 0; b < sp.n; b += kPlanThreads) {
    const int64_t i = b + t;
    int64_t s0 = 0, len = 0;
    if (i < sp.n) {
      s0 = sp.offsets[i];
      len = sp.offsets[i + 1] - s0;
    }
    const int64_t c = len > 0 ? (len + S - 1) / S : 0;
    const int64_t incl = wave_incl_scan(c);
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int64_t before = carry_s;
    for (int k = 0; k < wv; ++k) before += wave_tot[k];
    const int64_t first = before + incl - c;
    for (int64_t j = 0; j < c; ++j)
      if (first + j < sp.max_segs) sp.seg_offsets[first + j] = s0 + j * S;
    __syncthreads();
    if (t == kPlanThreads - 1) carry_s = before + incl;
    __syncthreads();
  }
  const int64_t n_seg = carry_s;
  if (n_seg > sp.max_segs) {  // block-uniform exit
    if (t == 0) {
      sp.counts[0] = -1;
      sp.counts[1] = n_seg;
    }
    return;
  }
  if (t == 0) sp.seg_offsets[n_seg] = n_seg > 0 ? sp.offsets[sp.n] : 0;
  __syncthreads();
  // 2. jump tables (ping-pong) and the orbit: LDS when they fit, else the caller's scratch
  const int64_t need = 2 * (n_seg + 1) + sp.max_rows + 1;
  int32_t* base = need <= kPlanLdsInts ? lds : sp.scratch;
  int32_t* J = base;
  int32_t* J2 = base + (n_seg + 1);
  int32_t* P = base + 2 * (n_seg + 1);
  const int64_t cap = sp.max_rows + 1;  // orbit entries: the rows' starts + the terminal n_seg
  for (int64_t k = t; k <= n_seg; k += kPlanThreads) {
    int32_t m = static_cast<int32_t>(n_seg);
    if (k < n_seg) {  // furthest segment end m within S tokens of segment k's start (every segment >= 1 token)
      const int64_t lim = sp.seg_offsets[k] + S;
      int64_t lo = k + 1, hi = n_seg - k > S ? k + S : n_seg;  // seg_offsets[lo] <= lim always
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (sp.seg_offsets[mid] <= lim)
          lo = mid;
        else
          hi = mid - 1;
      }
      m = static_cast<int32_t>(lo);
    }
    J[k] = m;
  }
  if (t == 0) P[0] = 0;
  __syncthreads();
  int64_t len = 1;
  while (P[len - 1] < n_seg && len < cap) {  // P[0..len) known, J = jump^len: P[len + i] = J[P[i]]
    const int64_t add = len < cap - len ? len : cap - len;
    for (int64_t i = t; i < add; i += kPlanThreads) P[len + i] = J[P[i]];
    for (int64_t k = t; k <= n_seg; k += kPlanThreads) J2[k] = J[J[k]];
    __syncthreads();
    int32_t* tmp = J;
    J = J2;
    J2 = tmp;
    len += add;
  }
  if (P[len - 1] < n_seg) {  // more rows than max_rows (block-uniform)
    if (t == 0) {
      sp.counts[0] = -1;
      sp.counts[1] = n_seg;
    }
    return;
  }
  // 3. rows: the orbit entries before the terminal one (P strictly increases until it reaches n_seg)
  for (int64_t i = t; i < len; i += kPlanThreads) {
    if (P[i] < n_seg) {
      sp.row_start[i] = sp.seg_offsets[P[i]];
      sp.row_end[i] = sp.seg_offsets[P[i + 1]];
      if (P[i + 1] == n_seg) {
        sp.counts[0] = i + 1;
        sp.counts[1] = n_seg;
      }
    }
  }
  if (t == 0 && n_seg == 0) {
    sp.counts[0] = 0;
    sp.counts[1] = 0;
  }
}

}  // namespace

int64_t pack_plan_scratch_ints(int64_t max_segs, int64_t max_rows) { return 2 * (max_segs + 1) + max_rows + 1; }

int pack_plan_device(const PackPlanSpec& spec, hipStream_t st) {
  if (spec.seq_len <= 0 || spec.n < 0 || spec.max_segs < 0 || spec.max_rows < 0) return -2;
  if (!spec.offsets || !spec.seg_offsets || !spec.row_start || !spec.row_end || !spec.counts || !spec.scratch)
    return -2;
  if (spec.max_segs >= (int64_t{1} << 31) - 1) return -4;  // int32 segment ids in the jump tables
  hipLaunchKernelGGL(pack_plan_kernel, dim3(1), dim3(kPlanThreads), 0, st, spec);
  return static_cast<int>(hipGetLastError());
}

int pad_pack_tokens(const TokenSpec& spec, hipStream_t st) {
  const int64_t grid = spec.seq_len > 0 ? ti_grid(spec.rows, spec.fill_rows, spec.seq_len, false) : 0;
  if (grid == 0) return 0;
  if (spec.mode == 0 && !spec.offsets) return -2;
  if (spec.mode == 1 && (!spec.row_start || !spec.row_end || !spec.seg_offsets)) return -2;
  if (spec.seq_len % kTiLane == 0 && reinterpret_cast<uintptr_t>(spec.labels) % 16) return -2;  // 16-byte stores
  if (grid < 0) return -4;
  hipLaunchKernelGGL(pad_pack_kernel, dim3(static_cast<uint32_t>(grid)), dim3(kTiThreads), 0, st, spec,
                     static_cast<int32_t>(ti_chunks(spec.seq_len)));
  return static_cast<int>(hipGetLastError());
}

int pad_pack_tokens_multi(const TokenSpec* specs, int n, hipStream_t st) {
  for (int g = 0; g < n; g += kMaxTokenSubs) {
    TokenMulti m{};
    const int cnt = n - g < kMaxTokenSubs ? n - g : kMaxTokenSubs;
    int64_t max_rows = 1, seq_len = 0;  // >= 1 block per sub-batch: block 0 writes its cu_seqlens
    for (int j = 0; j < cnt; ++j) {
      const TokenSpec& sp = specs[g + j];
      if (sp.seq_len <= 0 || (sp.mode == 0 && !sp.offsets) ||
          (sp.mode == 1 && (!sp.row_start || !sp.row_end || !sp.seg_offsets)))
        return -2;
      if (sp.seq_len % kTiLane == 0 && reinterpret_cast<uintptr_t>(sp.labels) % 16) return -2;
      if (j > 0 && sp.seq_len != seq_len) return -2;  // one chunking for the launch
      seq_len = sp.seq_len;
      if (sp.rows > max_rows) max_rows = sp.rows;
      if (sp.fill_rows > max_rows) max_rows = sp.fill_rows;
      m.sub[j] = sp;
    }
    const int64_t grid = ti_grid(max_rows, 0, seq_len, false);
    if (grid < 0) return -4;
    hipLaunchKernelGGL(pad_pack_multi_kernel, dim3(static_cast<uint32_t>(grid), static_cast<uint32_t>(cnt)),
                       dim3(kTiThreads), 0, st, m, static_cast<int32_t>(ti_chunks(seq_len)));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
  }
  return 0;
}

}  // namespace ddl
