// Host check of the mixture order kernel (tokens_mix.hip): the kernel's per-lane routine tm_order_at of tokens_mix.h
// replayed for every entry of every workgroup, over views that name an index outside an exact-size buffer, against
// an order written out independently here: each part's sequence (its whole passes round and round, then the first
// k documents of its inner permutation) materialised and concatenated, and entry i read at phi(i). Stand-alone:
// no HIP; the permutations are the host Feistel network of runtime/feistel.h. Built with
// -fsanitize=address,undefined (tests/host_check.py).
#include "../../runtime/feistel.h"
#include "../tokens_mix.h"
#include "check_common.h"

namespace {

struct Perm {  // a Feistel permutation of [0, n), or the identity (h = 0)
  uint64_t k[6];
  uint32_t h;
  uint64_t n;
  int64_t at(int64_t r) const {
    return h == 0 ? r : static_cast<int64_t>(ddl::host_feistel_perm(static_cast<uint64_t>(r), k, h, n));
  }
};

Perm make_perm(int64_t n, bool shuffle, Lcg* rng) {
  Perm p{};
  p.n = static_cast<uint64_t>(n);
  if (!shuffle) return p;
  int bits = 0;
  while (bits < 63 && (int64_t{1} << bits) < n) ++bits;  // bit length of n - 1
  p.h = static_cast<uint32_t>((bits + 1) / 2 > 1 ? (bits + 1) / 2 : 1);
  for (uint64_t& key : p.k) key = static_cast<uint64_t>(rng->next()) * 0x9E3779B97F4A7C15ull;
  return p;
}

template <typename T>
struct Checked {  // n elements of an exact-size buffer; an index outside is named before the load
  const T* p;
  int64_t n;
  const char* name;
  const char* what;
  T operator[](int64_t i) const {
    if (i < 0 || i >= n) fail(name, what);
    return p[i];
  }
};

struct Mix {
  const char* name;
  int parts;
  int64_t n_corpus;
  int64_t* cbase;      // [parts + 1]
  ddl::MixPart* part;  // [parts]
  std::vector<int64_t> extras;
  std::vector<Perm> inner;
  int64_t n() const { return cbase[parts]; }
};

// parts of n_docs[p] documents laid end to end from document `first`, `full[p]` whole passes and k[p] extras each
Mix make_mix(const char* name, int64_t first, const std::vector<int64_t>& n_docs, const std::vector<int64_t>& full,
             const std::vector<int64_t>& k, int64_t tail_docs, bool shuffle, Lcg* rng) {
  Mix m;
  m.name = name;
  m.parts = static_cast<int>(n_docs.size());
  m.cbase = exact<int64_t>(m.parts + 1);
  m.part = exact<ddl::MixPart>(m.parts);
  m.cbase[0] = 0;
  int64_t lo = first;
  for (int p = 0; p < m.parts; ++p) {
    m.part[p] = ddl::MixPart{lo, n_docs[p], full[p] * n_docs[p]};
    m.cbase[p + 1] = m.cbase[p] + full[p] * n_docs[p] + k[p];
    m.extras.push_back(k[p]);
    m.inner.push_back(make_perm(n_docs[p], shuffle, rng));
    lo += n_docs[p];
  }
  m.n_corpus = lo + tail_docs;
  return m;
}

void free_mix(Mix* m) {
  free(m->cbase);
  free(m->part);
}

// the order, written out: every part's sequence in full, then read through phi
std::vector<int64_t> written_order(const Mix& m, const std::vector<int64_t>& phi) {
  std::vector<int64_t> seq;
  for (int p = 0; p < m.parts; ++p) {
    const ddl::MixPart& pt = m.part[p];
    for (int64_t pass = 0; pass < pt.full_span / pt.n_docs; ++pass)
      for (int64_t d = 0; d < pt.n_docs; ++d) seq.push_back(pt.doc_lo + d);
    for (int64_t r = 0; r < m.extras[p]; ++r) seq.push_back(pt.doc_lo + m.inner[p].at(r));
  }
  std::vector<int64_t> out;
  for (int64_t v : phi) out.push_back(v >= 0 && v < static_cast<int64_t>(seq.size()) ? seq[v] : -1);
  return out;
}

// the kernel: tm_blocks(n) workgroups of kTmThreads lanes, lane t of workgroup b owns entry b * kTmThreads + t
void replay(const Mix& m, const std::vector<int64_t>& phi, const char* name) {
  ++g_cases;
  const int64_t n = static_cast<int64_t>(phi.size());
  if (!ddl::tm_parts_ok(m.cbase, m.part, m.parts, m.n_corpus, m.n())) fail(name, "a valid part table is refused");
  int64_t* phi_buf = exact<int64_t>(n);
  for (int64_t i = 0; i < n; ++i) phi_buf[i] = phi[i];
  int64_t* order = exact<int64_t>(n);
  int* writes = exact<int>(n);
  for (int64_t i = 0; i < n; ++i) writes[i] = 0;
  const Checked<int64_t> phi_v{phi_buf, n, name, "outer order read out of range"};
  const Checked<int64_t> cbase_v{m.cbase, m.parts + 1, name, "cbase read out of range"};
  const Checked<ddl::MixPart> part_v{m.part, m.parts, name, "part table read out of range"};
  auto outer = [&](int64_t i) { return phi_v[i]; };
  auto sigma = [&](int p, int64_t r) {
    if (p < 0 || p >= m.parts) {
      fail(name, "inner permutation of a part that does not exist");
      return int64_t{0};
    }
    if (r < 0 || r >= m.extras[p]) fail(name, "inner permutation asked outside its extra documents");
    if (r < 0 || r >= m.part[p].n_docs) return int64_t{0};  // the network's cycle walk would not end
    return m.inner[p].at(r);
  };
  for (int64_t b = 0; b < ddl::tm_blocks(n); ++b) {
    for (int t = 0; t < ddl::kTmThreads; ++t) {
      const int64_t i = b * ddl::kTmThreads + t;
      if (i >= n) continue;
      order[i] = ddl::tm_order_at(outer, cbase_v, part_v, m.parts, sigma, i);
      ++writes[i];
    }
  }
  const std::vector<int64_t> want = written_order(m, phi);
  for (int64_t i = 0; i < n; ++i) {
    if (writes[i] != 1) fail(name, "an entry is not written exactly once");
    if (order[i] != want[i]) {
      fail(name, "entry differs from the written-out order");
      break;
    }
    if (order[i] != -1 && (order[i] < 0 || order[i] >= m.n_corpus)) fail(name, "entry outside the corpus");
  }
  free(phi_buf);
  free(order);
  free(writes);
}

std::vector<int64_t> outer_order(int64_t n, bool shuffle, Lcg* rng) {
  const Perm p = make_perm(n, shuffle, rng);
  std::vector<int64_t> v;
  for (int64_t i = 0; i < n; ++i) v.push_back(p.at(i));
  return v;
}

void check_mix(const char* name, int64_t first, const std::vector<int64_t>& n_docs, const std::vector<int64_t>& full,
               const std::vector<int64_t>& k, Lcg* rng) {
  for (int shuffle = 0; shuffle < 2; ++shuffle) {
    Mix m = make_mix(name, first, n_docs, full, k, 3, shuffle != 0, rng);
    for (int epoch = 0; epoch < 2; ++epoch) replay(m, outer_order(m.n(), shuffle != 0, rng), name);
    // an explicit outer index may hold anything: values outside [0, N') are empty documents, nothing is read for them
    std::vector<int64_t> wild = outer_order(m.n(), shuffle != 0, rng);
    wild[0] = -1;
    wild[wild.size() / 2] = m.n();
    wild.back() = INT64_MAX;
    wild.push_back(INT64_MIN);
    wild.push_back(0);
    replay(m, wild, name);
    free_mix(&m);
  }
}

void check_refusals() {
  ++g_cases;
  const char* name = "refusals";
  int64_t cbase[3] = {0, 10, 16};
  ddl::MixPart part[2] = {{0, 4, 8}, {4, 6, 6}};
  if (!ddl::tm_parts_ok(cbase, part, 2, 10, 16)) fail(name, "the valid table");
  if (ddl::tm_parts_ok(cbase, part, 0, 10, 16)) fail(name, "no part");
  if (ddl::tm_parts_ok(cbase, part, 17, 10, 16)) fail(name, "17 parts");
  if (ddl::tm_parts_ok(cbase, part, 2, 9, 16)) fail(name, "a part past the corpus");
  if (ddl::tm_parts_ok(cbase, part, 2, 10, 15)) fail(name, "n is not cbase[parts]");
  cbase[1] = 13;  // 5 extras of 4 documents
  if (ddl::tm_parts_ok(cbase, part, 2, 10, 16)) fail(name, "more extras than documents");
  cbase[1] = 7;  // fewer entries than the whole passes
  if (ddl::tm_parts_ok(cbase, part, 2, 10, 16)) fail(name, "cbase below the whole passes");
  cbase[1] = 10;
  part[0].full_span = 7;
  if (ddl::tm_parts_ok(cbase, part, 2, 10, 16)) fail(name, "a span that is no whole number of passes");
  part[0].full_span = 8;
  part[1].n_docs = 0;
  if (ddl::tm_parts_ok(cbase, part, 2, 10, 16)) fail(name, "an empty part");
  part[1].n_docs = 6;
  part[0].doc_lo = -1;
  if (ddl::tm_parts_ok(cbase, part, 2, 10, 16)) fail(name, "a negative first document");
  part[0].doc_lo = 0;
  cbase[0] = 1;
  if (ddl::tm_parts_ok(cbase, part, 2, 10, 16)) fail(name, "cbase[0] != 0");
}

// Far case: a table whose cbase and documents pass 2^32 and 2^40 (nothing of that size is materialised): chosen
// entries through tm_order_at against the definition evaluated here part by part, inner permutations included.
void check_far(Lcg* rng) {
  const char* name = "far table";
  const std::vector<int64_t> n_docs = {(int64_t{1} << 33) + 3, 1000, (int64_t{1} << 40) + 11, 7};
  const std::vector<int64_t> full = {1, 5000000, 2, 0};
  const std::vector<int64_t> k = {int64_t{1} << 31, 999, (int64_t{1} << 39) + 1, 7};
  Mix m = make_mix(name, (int64_t{1} << 32) + 7, n_docs, full, k, 3, true, rng);
  if (!ddl::tm_parts_ok(m.cbase, m.part, m.parts, m.n_corpus, m.n())) fail(name, "a valid part table is refused");
  if (m.cbase[1] <= (int64_t{1} << 32) || m.n() <= (int64_t{1} << 41)) fail(name, "the table is not far");
  const Checked<int64_t> cbase_v{m.cbase, m.parts + 1, name, "cbase read out of range"};
  const Checked<ddl::MixPart> part_v{m.part, m.parts, name, "part table read out of range"};
  auto sigma = [&](int p, int64_t r) {
    if (p < 0 || p >= m.parts || r < 0 || r >= m.extras[p]) {
      fail(name, "inner permutation asked outside its extra documents");
      return int64_t{0};
    }
    return m.inner[p].at(r);
  };
  std::vector<int64_t> entries = {0, (int64_t{1} << 31) - 1, int64_t{1} << 31, (int64_t{1} << 32) - 1, int64_t{1} << 32,
                                  (int64_t{1} << 32) + 1, int64_t{1} << 40, m.n() - 1, m.n(), -1, INT64_MAX};
  for (int p = 0; p <= m.parts; ++p)  // both sides of every part border and of every border between passes and extras
    for (int64_t d : {-1, 0, 1}) {
      entries.push_back(m.cbase[p] + d);
      if (p < m.parts) entries.push_back(m.cbase[p] + m.part[p].full_span + d);
    }
  for (int c = 0; c < 200; ++c) entries.push_back(((rng->next() << 20) ^ rng->next()) % m.n());
  for (int64_t v : entries) {
    ++g_cases;
    int64_t want = -1;
    for (int p = 0; p < m.parts && v >= 0; ++p) {
      if (v >= m.cbase[p + 1]) continue;
      const int64_t j = v - m.cbase[p];
      const ddl::MixPart& pt = m.part[p];
      want = pt.doc_lo + (j < pt.full_span ? j % pt.n_docs : m.inner[p].at(j - pt.full_span));
      break;
    }
    const int64_t got = ddl::tm_order_at([&](int64_t) { return v; }, cbase_v, part_v, m.parts, sigma, 0);
    if (got != want) fail(name, "entry differs from the definition");
    if (got != -1 && (got < m.part[0].doc_lo || got >= m.n_corpus)) fail(name, "entry outside the parts");
  }
  free_mix(&m);
}

}  // namespace

int main() {
  Lcg rng{12345};
  check_mix("one part once", 0, {1}, {1}, {0}, &rng);
  check_mix("one part, 257 documents", 0, {257}, {1}, {0}, &rng);
  check_mix("2.5 / 1 / 0.25", 0, {100, 57, 100}, {2, 1, 0}, {50, 0, 25}, &rng);
  check_mix("a one-document part three times", 0, {40, 1, 215}, {1, 3, 1}, {0, 0, 0}, &rng);
  check_mix("a part without entries in between", 0, {30, 200, 26}, {1, 0, 1}, {7, 0, 13}, &rng);
  check_mix("parts without entries at both ends", 0, {5, 300, 9}, {0, 1, 0}, {0, 213, 0}, &rng);
  check_mix("extras only", 0, {64, 64}, {0, 0}, {1, 63}, &rng);
  check_mix("every document an extra", 0, {19}, {0}, {19}, &rng);
  {
    std::vector<int64_t> n_docs, full, k;
    for (int p = 0; p < ddl::kMixMaxParts; ++p) {
      n_docs.push_back(1 + (p * 7) % 23);
      full.push_back(p % 3);
      k.push_back(p % 2 ? n_docs.back() / 2 : 0);
    }
    check_mix("16 parts", 0, n_docs, full, k, &rng);
  }
  for (int c = 0; c < 40; ++c) {  // random part tables
    const int parts = 1 + static_cast<int>(rng.next() % ddl::kMixMaxParts);
    std::vector<int64_t> n_docs, full, k;
    int64_t total = 0;
    for (int p = 0; p < parts; ++p) {
      n_docs.push_back(1 + rng.next() % 70);
      full.push_back(rng.next() % 4);
      k.push_back(rng.next() % (n_docs.back() + 1));
      total += full.back() * n_docs.back() + k.back();
    }
    if (total == 0) k[0] = 1;
    check_mix("random", 0, n_docs, full, k, &rng);
  }
  check_refusals();
  check_far(&rng);
  return finish("tokens mix check");
}
