// Per-lane arithmetic of the fill-in-the-middle kernel (tokens_fim.hip), shared with host code:
// csrc/kernels/tests/tokens_fim_check.cpp replays tf_lane4 for every lane under ASan/UBSan over index-checked views.
// Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of HIP; the
// batch comes in as callables).
//
// A segment is a maximal run of one document in one row of a rendered [R, S] batch: tokens t[0 .. L) at columns
// [col0, col0 + L) of its row, with key k (the loaders: the corpus element of its first token) and the epoch's key
// ekey. Everything is integer arithmetic:
//   u_c  = mix64(ekey ^ mix64(4 * k + c)), c = 0 .. 3             (k as uint64, the sum modulo 2^64)
//   tail = eod given and t[L - 1] == eod ? 1 : 0      M = L - tail      K = M - 3
//   rearranged iff M >= min_len and (u_0 >> 40) < rate_q;   SPM iff (u_1 >> 40) < spm_q, else PSM
//   x = ((u_2 >> 32) * (K + 1)) >> 32,  y likewise of u_3,  a = min(x, y),  b = max(x, y)
//   prefix = t[0 .. a), middle = t[a .. b), suffix = t[b .. K); t[K .. M) make room for the three sentinels
//   PSM  [PRE] prefix [SUF] suffix [MID] middle          then t[L - 1] if tail
//   SPM  [PRE] [SUF] suffix [MID] prefix middle          then t[L - 1] if tail
// The map is piecewise contiguous: output position j of the segment is a sentinel or t[tf_src(g, j)].
#pragma once

#include <stdint.h>

#include "tokens_indexed.h"

#define DDL_TF_HD DDL_TI_HD

namespace ddl {

struct FimParams {
  uint64_t ekey;        // the epoch's key
  uint32_t rate_q;      // round(rate * 2^24): a segment is rearranged iff its 24-bit draw lies below
  uint32_t spm_q;       // round(spm_rate * 2^24): the SPM share of the rearranged
  int32_t prefix_id, middle_id, suffix_id;
  int32_t eod_id;       // read only where has_eod
  int32_t has_eod;
  int32_t min_len;      // >= 4: the shortest body (without its EOD) that is rearranged
};

constexpr int kTfKeep = 0, kTfPsm = 1, kTfSpm = 2;      // FimSeg.mode
constexpr int64_t kTfPre = -1, kTfSuf = -2, kTfMid = -3;  // tf_src: a sentinel instead of a source offset

struct FimSeg {
  int64_t L;     // positions of the segment
  int64_t a, b;  // the cuts, 0 <= a <= b <= K
  int64_t K;     // body tokens kept
  int32_t mode;
  int32_t tail;
};

DDL_TF_HD uint64_t tf_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

DDL_TF_HD uint64_t tf_draw(uint64_t ekey, uint64_t key, uint64_t c) { return tf_mix64(ekey ^ tf_mix64(4 * key + c)); }

// a cut in [0, K]: the high 32 bits of the draw scaled by K + 1 (K + 1 <= 2^31: the product fits 64 bits)
DDL_TF_HD int64_t tf_cut(uint64_t u, int64_t K) {
  return static_cast<int64_t>(((u >> 32) * static_cast<uint64_t>(K + 1)) >> 32);
}

// The parameters of a segment of L >= 1 tokens with key `key`; last_is_eod: t[L - 1] == eod_id (asked only where
// has_eod). L < 2^31.
DDL_TF_HD FimSeg tf_segment(const FimParams& fp, uint64_t key, int64_t L, bool last_is_eod) {
  FimSeg g;
  g.L = L;
  g.tail = fp.has_eod && last_is_eod ? 1 : 0;
  const int64_t M = L - g.tail;
  g.K = M - 3;
  g.a = g.b = 0;
  g.mode = kTfKeep;
  if (M < fp.min_len || M < 4) return g;
  if ((tf_draw(fp.ekey, key, 0) >> 40) >= fp.rate_q) return g;
  g.mode = (tf_draw(fp.ekey, key, 1) >> 40) < fp.spm_q ? kTfSpm : kTfPsm;
  const int64_t x = tf_cut(tf_draw(fp.ekey, key, 2), g.K), y = tf_cut(tf_draw(fp.ekey, key, 3), g.K);
  g.a = x < y ? x : y;
  g.b = x < y ? y : x;
  return g;
}

// Output position j, 0 <= j < L, of segment g: the offset in [0, L) of the token it takes, or kTfPre / kTfSuf / kTfMid
DDL_TF_HD int64_t tf_src(const FimSeg& g, int64_t j) {
  if (g.mode == kTfKeep || j >= g.K + 3) return j;  // untouched, or the EOD that stays last
  const int64_t n_suf = g.K - g.b;
  if (j == 0) return kTfPre;
  if (g.mode == kTfPsm) {
    if (j <= g.a) return j - 1;                      // prefix
    if (j == g.a + 1) return kTfSuf;
    if (j < g.a + 2 + n_suf) return g.b + (j - (g.a + 2));  // suffix
    if (j == g.a + 2 + n_suf) return kTfMid;
    return g.a + (j - (g.a + 3 + n_suf));            // middle
  }
  if (j == 1) return kTfSuf;
  if (j < 2 + n_suf) return g.b + (j - 2);           // suffix
  if (j == 2 + n_suf) return kTfMid;
  return j - (3 + n_suf);                            // prefix and middle: t[0 .. b)
}

DDL_TF_HD int32_t tf_sentinel(const FimParams& fp, int64_t code) {
  return code == kTfPre ? fp.prefix_id : code == kTfSuf ? fp.suffix_id : fp.middle_id;
}

// One lane of the kernel: positions p0 .. p0 + 3 of one row of S columns (those below S). seg / pos / own: the lane's
// segment ids, position ids and tokens (entries at or past S are not read). cu_at(i), 0 <= i <= cap: cu_seqlens;
// key_at(s), 0 <= s < cap: seg_keys; tok_at(col), 0 <= col < S: the row's rendered token at column col. A position
// is rewritten only where its segment is sound: 0 <= s < cap, L = cu[s + 1] - cu[s] >= 1, 0 <= pos < L and the
// segment's columns [p - pos, p - pos + L) inside the row -- so every column asked of tok_at lies in [0, S); anything
// else keeps its token and gets the label ignore_index. live = false (an overflowed or invalid batch): nothing is
// rearranged. The label of position j of a segment is its rearranged token j + 1, ignore_index at j = L - 1:
// ref_token_labels of the rearranged row. The segment's parameters are computed once per distinct segment.
template <typename CuAt, typename KeyAt, typename TokAt>
DDL_TF_HD void tf_lane4(const FimParams& fp, int64_t S, int64_t cap, bool live, int64_t p0, const int64_t* seg,
                        const int64_t* pos, const int32_t* own, CuAt cu_at, KeyAt key_at, TokAt tok_at, bool labels,
                        int32_t ignore_index, int32_t* out, int64_t* lab) {
  int64_t cur = -1, col0 = 0;
  FimSeg g;
  g.L = 0;
  g.a = g.b = g.K = 0;
  g.mode = kTfKeep;
  g.tail = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < kTiLane; ++k) {
    const int64_t p = p0 + k;
    if (p >= S) continue;
    out[k] = own[k];
    lab[k] = ignore_index;
    const int64_t s = seg[k], j = pos[k];
    if (s < 0 || s >= cap || j < 0 || j > p) continue;
    const int64_t c0 = p - j;  // the segment's first column, in [0, p]
    if (s != cur || c0 != col0) {
      cur = -1;
      const int64_t L = static_cast<int64_t>(cu_at(s + 1)) - static_cast<int64_t>(cu_at(s));
      if (L < 1 || j >= L || c0 > S - L) continue;
      cur = s;
      col0 = c0;
      if (live) {
        const bool eod = fp.has_eod && tok_at(c0 + L - 1) == fp.eod_id;
        g = tf_segment(fp, static_cast<uint64_t>(key_at(s)), L, eod);
      } else {
        g.L = L;
        g.mode = kTfKeep;
      }
    }
    if (j >= g.L) continue;  // the cached segment's run ended in front of this position: not a sound one
    const int64_t c = tf_src(g, j);
    if (c < 0)
      out[k] = tf_sentinel(fp, c);
    else if (c != j)
      out[k] = tok_at(col0 + c);
    if (labels && j + 1 < g.L) {
      const int64_t n = tf_src(g, j + 1);
      lab[k] = n < 0 ? tf_sentinel(fp, n) : n == j + 1 && k + 1 < kTiLane ? own[k + 1] : tok_at(col0 + n);
    }
  }
}

}  // namespace ddl
