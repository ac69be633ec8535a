// Index arithmetic and the per-lane routine of the mixture order kernel (tokens_mix.hip), shared with host code:
// csrc/kernels/tests/tokens_mix_check.cpp replays the routine for every entry under ASan/UBSan over index-checked
// views. Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of
// HIP; the permutations come in as callables: the kernel passes source_row and feistel_perm of common.h).
//
// A mixture is P <= kMixMaxParts parts, part p = the corpus documents [doc_lo, doc_lo + n_docs), taken c_p =
// full_span + k_p times per epoch: full_span = (whole passes) * n_docs entries walk the part round and round, the
// k_p <= n_docs entries behind them are the first k_p documents of the part's own fixed permutation sigma_p.
// cbase = the exclusive scan of c (cbase[P] = N', the order's length). Entry i of the epoch's order:
//   v = phi(i)                      the epoch's permutation of [0, N'), or the identity
//   p: cbase[p] <= v < cbase[p+1]   j = v - cbase[p]
//   order[i] = doc_lo_p + (j < full_span_p ? j % n_docs_p : sigma_p(j - full_span_p))
#pragma once

#include <stdint.h>

#include "tokens_plan.h"

#define DDL_TM_HD DDL_TP_HD

namespace ddl {

constexpr int kMixMaxParts = 16;
constexpr int kTmThreads = 256;  // lanes of a workgroup = order entries per workgroup

struct MixPart {
  int64_t doc_lo;     // first corpus document of the part
  int64_t n_docs;     // its documents, >= 1
  int64_t full_span;  // whole passes * n_docs
};

// workgroups of an order of n entries
DDL_TM_HD int64_t tm_blocks(int64_t n) { return n > 0 ? (n + kTmThreads - 1) / kTmThreads : 0; }

// the part of value v, 0 <= v < cbase[parts]: the last p with cbase[p] <= v, by a walk every lane makes alike
// (a part without entries, cbase[p] == cbase[p + 1], is stepped over)
template <typename CBase>
DDL_TM_HD int tm_part_of(const CBase& cbase, int parts, int64_t v) {
  int p = 0;
  for (int q = 1; q < parts; ++q) p += cbase[q] <= v ? 1 : 0;
  return p;
}

// One lane of the kernel: entry i of the order. phi(i) = the outer order's value at position i; cbase [parts + 1]
// and part [parts] are anything indexable by int (the kernel: its copies in LDS; the replay: checked views);
// sigma(p, r) = part p's inner permutation at r, asked only for 0 <= r < k_p. A value outside [0, cbase[parts])
// -- an explicit outer index may hold anything -- gives -1, which every stream kernel reads as an empty document.
template <typename Phi, typename CBase, typename Parts, typename Sigma>
DDL_TM_HD int64_t tm_order_at(const Phi& phi, const CBase& cbase, const Parts& part, int parts, const Sigma& sigma,
                              int64_t i) {
  const int64_t v = phi(i);
  if (static_cast<uint64_t>(v) >= static_cast<uint64_t>(cbase[parts])) return -1;
  const int p = tm_part_of(cbase, parts, v);
  const int64_t j = v - cbase[p];
  const MixPart pt = part[p];
  if (j < pt.full_span) return pt.doc_lo + j % pt.n_docs;
  return pt.doc_lo + sigma(p, j - pt.full_span);
}

// What the launcher checks of the part table before a launch (the keys of the inner permutations are its own
// check): 1 <= parts <= kMixMaxParts, every part non-empty and inside [0, n_corpus], full_span a whole number of
// passes, cbase[0] = 0 and every step cbase[p + 1] - cbase[p] = full_span + k with 0 <= k <= n_docs, cbase[parts] = n.
DDL_TM_HD bool tm_parts_ok(const int64_t* cbase, const MixPart* part, int parts, int64_t n_corpus, int64_t n) {
  if (parts < 1 || parts > kMixMaxParts || n_corpus < 0 || cbase[0] != 0) return false;
  for (int p = 0; p < parts; ++p) {
    const MixPart& pt = part[p];
    if (pt.n_docs < 1 || pt.doc_lo < 0 || pt.doc_lo > n_corpus || pt.n_docs > n_corpus - pt.doc_lo) return false;
    if (pt.full_span < 0 || pt.full_span % pt.n_docs != 0) return false;
    if (cbase[p + 1] < cbase[p]) return false;
    const int64_t k = cbase[p + 1] - cbase[p] - pt.full_span;
    if (k < 0 || k > pt.n_docs) return false;
  }
  return cbase[parts] == n;
}

// the extra documents of part p: c_p - full_span_p
DDL_TM_HD int64_t tm_extras(const int64_t* cbase, const MixPart* part, int p) {
  return cbase[p + 1] - cbase[p] - part[p].full_span;
}

}  // namespace ddl
