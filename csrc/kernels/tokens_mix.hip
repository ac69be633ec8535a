// Token stream loader, weighted mixture of corpus parts: the epoch's document order written into HBM, once per
// epoch. token_stream_table and the stream plans then run on it as on any explicit index (RowIndex mode 1), so a
// mixture costs this one kernel and 8 bytes per order entry; all the index arithmetic is tokens_mix.h.
//
// One thread per order entry (orders of 2^32 entries or more: a grid-stride loop), one 8-byte store per lane, consecutive lanes to consecutive entries. The spec (the
// outer RowIndex, the part table, the inner permutations' keys: about 1.6 KB) is the kernel's argument. A lane's
// part number differs from its neighbour's, and a kernel argument indexed by it would be copied to scratch, so each
// workgroup first stages the part table into LDS -- part q by lane q, the argument indexed by the loop counter only
// -- and the lanes read their part there.
//
// Bounded reads: ri.idx[0 .. n) in mode 1; nothing else of global memory. Bounded writes: order[0 .. n), each once.
// The launcher refuses what would make a lane's cycle walk endless: an outer permutation whose domain does not
// cover the positions (row_index_ok), and inner keys that are no permutation of the part's documents.
#include "common.h"
#include "launch.h"
#include "tokens_mix.h"

namespace ddl {
namespace {

struct TmPhi {
  const RowIndex& ri;
  __device__ int64_t operator()(int64_t i) const { return source_row(ri, i); }
};

struct TmSigma {
  const FeistelKeys* keys;  // LDS
  int32_t shuffle;
  __device__ int64_t operator()(int p, int64_t r) const {
    return shuffle ? static_cast<int64_t>(feistel_perm(static_cast<uint64_t>(r), keys[p])) : r;
  }
};

__global__ void __launch_bounds__(kTmThreads) token_mix_order_kernel(MixOrderSpec sp) {
  __shared__ int64_t cbase[kMixMaxParts + 1];
  __shared__ MixPart part[kMixMaxParts];
  __shared__ FeistelKeys keys[kMixMaxParts];
  const int t = threadIdx.x;
  for (int q = 0; q < sp.parts; ++q) {  // q is uniform: the argument is read through scalar loads
    if (t == q) {
      cbase[q] = sp.cbase[q];
      part[q] = sp.part[q];
      keys[q] = sp.keys[q];
    }
  }
  if (t == 0) cbase[sp.parts] = sp.cbase[sp.parts];
  __syncthreads();
  // grid-stride: a launch holds fewer than 2^32 threads (kTmMaxBlocks), an order may hold more entries
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kTmThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kTmThreads + t; i < sp.n; i += stride)
    sp.order[i] = tm_order_at(TmPhi{sp.ri}, cbase, part, sp.parts, TmSigma{keys, sp.inner_shuffle}, i);
}

bool inner_keys_ok(const FeistelKeys& f, int64_t n_docs) {
  if (f.n != static_cast<uint64_t>(n_docs) || f.half_bits < 1 || f.half_bits > 32) return false;
  return f.half_bits == 32 || f.n <= (uint64_t{1} << (2 * f.half_bits));
}

}  // namespace

int token_mix_order(const MixOrderSpec& spec, hipStream_t st) {
  if (spec.parts < 1 || spec.parts > kMixMaxParts || spec.n < 1 || !spec.order) return -2;
  if (!tm_parts_ok(spec.cbase, spec.part, spec.parts, spec.n_corpus, spec.n)) return -2;
  if (!row_index_ok(spec.ri, spec.n)) return -2;
  if (spec.inner_shuffle) {
    for (int p = 0; p < spec.parts; ++p) {
      if (tm_extras(spec.cbase, spec.part, p) > 0 && !inner_keys_ok(spec.keys[p], spec.part[p].n_docs)) return -2;
    }
  }
  // One thread per entry up to kTmMaxBlocks workgroups; past that the lanes stride. A grid of 2^32 threads or more
  // ran only its count modulo 2^32: an order of 2^32 + k entries had just its first k written.
  constexpr int64_t kTmMaxBlocks = (int64_t{1} << 32) / kTmThreads - 1;
  const int64_t blocks = tm_blocks(spec.n) < kTmMaxBlocks ? tm_blocks(spec.n) : kTmMaxBlocks;
  hipLaunchKernelGGL(token_mix_order_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kTmThreads), 0, st, spec);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
