// Host check of row_index_ok (csrc/kernels/common.h), the check every launcher that takes a RowIndex makes before
// it launches, built with -fsanitize=address,undefined by tests/test_row_index_check.py. The selectors a kernel
// would not survive -- an empty or oversized Feistel domain, a position past the domain (the cycle walk of
// feistel_perm does not end on a non-bijection), a missing index vector, a negative base -- are asserted here and
// only here: no GPU test hands one to a launcher. Each mode's accepting boundary is in the table too, and every
// accepted Feistel selector with a small domain is walked on the host: source_row ends and lands inside the domain.
#include "../common.h"
#include "check_common.h"

namespace {

ddl::RowIndex selector(int mode, int64_t base, uint64_t n, uint32_t half_bits, const int64_t* idx = nullptr) {
  ddl::RowIndex ri{};
  ri.mode = mode;
  ri.base = base;
  ri.idx = idx;
  ri.keys.n = n;
  ri.keys.half_bits = half_bits;
  for (int i = 0; i < ddl::kFeistelRounds; ++i) ri.keys.k[i] = 0x9E3779B97F4A7C15ull * (i + 1);
  return ri;
}

void expect(const char* name, const ddl::RowIndex& ri, int64_t n, bool want) {
  ++g_cases;
  if (ddl::row_index_ok(ri, n) != want) fail(name, want ? "refused" : "accepted");
  if (!want || ri.mode != 2 || ri.keys.n > 4096) return;
  std::vector<int> seen(ri.keys.n, 0);  // an accepted small Feistel selector: distinct rows inside the domain
  for (int64_t r = 0; r < n; ++r) {
    const int64_t s = ddl::source_row(ri, r);
    if (s < 0 || static_cast<uint64_t>(s) >= ri.keys.n || seen[s]++) fail(name, "source_row outside the domain");
  }
}

void run_all() {
  const int64_t index[4] = {3, 0, 2, 1};
  const uint64_t max64 = ~uint64_t{0};
  // mode 0: base + r, no domain to stay in
  expect("identity", selector(0, 0, 0, 0), 4, true);
  expect("identity, base > 0", selector(0, int64_t{1} << 40, 0, 0), 4, true);
  expect("identity, negative base", selector(0, -1, 0, 0), 4, false);
  // mode 1: an index vector for every launch that reads one
  expect("index", selector(1, 0, 0, 0, index), 4, true);
  expect("index, null", selector(1, 0, 0, 0, nullptr), 4, false);
  expect("index, null, no rows", selector(1, 0, 0, 0, nullptr), 0, true);
  expect("index, base ignored", selector(1, -5, 0, 0, index), 4, true);
  // unknown modes
  expect("mode 3", selector(3, 0, 5, 2), 4, false);
  expect("mode -1", selector(-1, 0, 5, 2), 4, false);
  // mode 2: a domain of 1 .. 2^(2h) rows, h in 1 .. 32, and every position inside it
  expect("feistel", selector(2, 0, 5, 2), 5, true);
  expect("feistel, base + n == domain", selector(2, 3, 5, 2), 2, true);
  expect("feistel, base + n one past the domain", selector(2, 3, 5, 2), 3, false);
  expect("feistel, positions 5 and 6 of 5", selector(2, 3, 5, 2), 4, false);
  expect("feistel, base == domain, no rows", selector(2, 5, 5, 2), 0, true);
  expect("feistel, base past the domain", selector(2, 6, 5, 2), 0, false);
  expect("feistel, negative base", selector(2, -1, 5, 2), 1, false);
  expect("feistel, n == 0", selector(2, 0, 0, 2), 0, false);
  expect("feistel, n == 0, one row", selector(2, 0, 0, 2), 1, false);
  expect("feistel, half_bits 0", selector(2, 0, 1, 0), 1, false);
  expect("feistel, half_bits 33", selector(2, 0, 5, 33), 1, false);
  expect("feistel, domain == 2^(2h)", selector(2, 0, 16, 2), 16, true);
  expect("feistel, domain > 2^(2h)", selector(2, 0, 17, 2), 1, false);
  expect("feistel, domain == 2^62, h 31", selector(2, 0, uint64_t{1} << 62, 31), 4, true);
  expect("feistel, domain > 2^62, h 31", selector(2, 0, (uint64_t{1} << 62) + 1, 31), 4, false);
  expect("feistel, h 32, domain 2^64 - 1", selector(2, 0, max64, 32), 4, true);
  expect("feistel, h 32, last positions", selector(2, INT64_MAX - 3, max64, 32), 4, true);
  expect("feistel, h 32, base + n == domain in 64 bits", selector(2, INT64_MAX, uint64_t{INT64_MAX} + 4, 32), 4, true);
  expect("feistel, h 32, one past in 64 bits", selector(2, INT64_MAX, uint64_t{INT64_MAX} + 4, 32), 5, false);
  expect("negative row count", selector(2, 0, 5, 2), -1, false);
}

// The two refused selectors tests/test_row_index_check_gpu.py hands to the launchers (5 source rows, 4 output rows)
// must be harmless if a launcher forgot the check: every row then ends, inside the source. The unknown mode is the
// identity from base 0. The Feistel one (WALK_KEYS there) starts two of its walks outside the domain, where a cycle
// of the network may never enter it: the walk is replayed here with a bound of the network's 16 values.
const uint64_t kGpuTestKeys[ddl::kFeistelRounds] = {31, 32, 33, 34, 35, 36};

void run_gpu_test_selectors() {
  ++g_cases;
  ddl::RowIndex unknown = selector(3, 0, 1, 1);
  if (ddl::row_index_ok(unknown, 4)) fail("gpu test, unknown mode", "accepted");
  for (int64_t r = 0; r < 4; ++r)
    if (ddl::source_row(unknown, r) != r) fail("gpu test, unknown mode", "not the identity");
  ++g_cases;
  ddl::RowIndex past = selector(2, 3, 5, 2);
  for (int i = 0; i < ddl::kFeistelRounds; ++i) past.keys.k[i] = kGpuTestKeys[i];
  if (ddl::row_index_ok(past, 4)) fail("gpu test, positions past the domain", "accepted");
  for (int64_t r = 0; r < 4; ++r) {
    uint64_t x = ddl::feistel_once(static_cast<uint64_t>(past.base + r), past.keys);
    int steps = 1;
    for (; x >= past.keys.n && steps < 16; ++steps) x = ddl::feistel_once(x, past.keys);
    if (x >= past.keys.n) fail("gpu test, positions past the domain", "the cycle walk does not reach the domain");
  }
  past.base = 1;  // the accepted twin of the same test: positions 1 .. 4
  expect("gpu test, positions inside the domain", past, 4, true);
}

}  // namespace

int main() {
  run_all();
  run_gpu_test_selectors();
  return finish("row index check");
}
