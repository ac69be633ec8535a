// What the two token stream checks share on top of check_common.h: views that name an index outside an exact-size
// buffer, the corpus set-up and the replay of the wave-wide search of tokens_stream.h.
#pragma once

#include "../tokens_stream.h"
#include "check_common.h"

namespace {

// n elements of an exact-size buffer as the shared per-lane routines read them, by [] or (): an index outside
// [0, n) is reported by name before the load that the sanitizer stops
struct View {
  const int64_t* p;
  int64_t n;
  const char* name;
  const char* what;
  int64_t operator[](int64_t i) const {
    if (i < 0 || i >= n) fail(name, what);
    return p[i];
  }
  int64_t operator()(int64_t i) const { return (*this)[i]; }
};

// a corpus, an order of its documents and the order's table, each of exactly its size
struct Corpus {
  int64_t n_corpus;
  int64_t* coffs;  // [n_corpus + 1]
  int64_t n;
  int64_t* order;  // [n]: any value (out-of-range ones are empty documents)
  int64_t* table;  // [n + 1], or null until the check has built it
  const char* name;
  View offs_view() const { return {coffs, n_corpus + 1, name, "corpus offsets read out of range"}; }
  View order_view() const { return {order, n, name, "order read out of range"}; }
  View table_view() const { return {table, n + 1, name, "table read out of range"}; }
};

Corpus make_corpus(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& order) {
  Corpus c;
  c.name = name;
  c.n_corpus = static_cast<int64_t>(lens.size());
  c.n = static_cast<int64_t>(order.size());
  c.coffs = exact<int64_t>(c.n_corpus + 1);
  c.coffs[0] = 0;
  for (int64_t i = 0; i < c.n_corpus; ++i) c.coffs[i + 1] = c.coffs[i] + lens[i];
  c.order = exact<int64_t>(c.n);
  for (int64_t i = 0; i < c.n; ++i) c.order[i] = order[i];
  c.table = nullptr;
  return c;
}

// the table of an order whose every index is inside the corpus, by a plain serial sum
void serial_table(Corpus* c) {
  c->table = exact<int64_t>(c->n + 1);
  c->table[0] = 0;
  for (int64_t i = 0; i < c->n; ++i) {
    const int64_t q = c->order[i];
    c->table[i + 1] = c->table[i] + (c->coffs[q + 1] - c->coffs[q]);
  }
}

void free_corpus(Corpus* c) {
  free(c->table);
  free(c->coffs);
  free(c->order);
}

// ts_wave_last_le: the 64 lanes of one wave
int64_t replay_search(const char* name, const int64_t* table, int64_t n1, int64_t v) {
  int64_t lo = 0, hi = n1;
  int steps = 0;
  while (hi - lo > 1) {
    const int64_t stride = ddl::ts_search_stride(lo, hi);
    int k = 0;
    for (int lane = 0; lane < ddl::kTpWave; ++lane) {
      const int64_t p = ddl::ts_search_probe(lo, stride, lane);
      if (p < hi) {
        if (p < 0 || p >= n1) fail(name, "search probe outside the table");
        if (table[p] <= v) ++k;
      }
    }
    if (k < 1) k = 1;
    ddl::ts_search_narrow(&lo, &hi, stride, k);
    if (++steps > 64) {
      fail(name, "search does not terminate");
      break;
    }
  }
  return lo;
}

}  // namespace
