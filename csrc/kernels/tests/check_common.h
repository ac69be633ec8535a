// What the host check programs of this directory share: the failure and case counters, exact-size buffers, the
// generated corpora, the LCG of the random cases and the host pack plan; it includes no kernel header. Each program
// is one translation unit built with -fsanitize=address,undefined (tests/host_check.py).
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

namespace {

int g_failures = 0;
int64_t g_cases = 0;  // bumped once per executed case

void fail(const char* name, const char* what) {
  printf("%s: %s\n", name, what);
  fflush(stdout);  // the sanitizer may end the program at the very next load
  ++g_failures;
}

// the end of main: "<check>: N failures" or "<check> ok<note>", and the exit code
int finish(const char* check, const char* note = "") {
  printf("%s: %lld cases\n", check, (long long)g_cases);
  if (g_failures) {
    printf("%s: %d failures\n", check, g_failures);
    return 1;
  }
  printf("%s ok%s\n", check, note);
  return 0;
}

template <typename T>
T* exact(size_t n) {  // exactly n elements (n = 0: a one-byte block nothing may touch as a T)
  return static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
}

// base + i % m, i < count: the generated corpora (3001 documents of i % 13 -- every 13th empty --, i % 41, 1 + i % 2)
std::vector<int64_t> mod_lens(int64_t count, int64_t m, int64_t base = 0) {
  std::vector<int64_t> v;
  for (int64_t i = 0; i < count; ++i) v.push_back(base + i % m);
  return v;
}
// (i * mul + add) % m, i < n: the generated orders and index vectors
std::vector<int64_t> stride_order(int64_t n, int64_t mul, int64_t add, int64_t m) {
  std::vector<int64_t> v;
  for (int64_t i = 0; i < n; ++i) v.push_back((i * mul + add) % m);
  return v;
}

struct Lcg {
  uint64_t state;
  int64_t next() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<int64_t>(state >> 33);
  }
};

// the host plan (runtime/arena.cpp pack_plan): over-long sequences become S-chunks, a row breaks where the next
// segment does not fit
void host_pack_plan(const std::vector<int64_t>& offs, int64_t S, std::vector<int64_t>* rs, std::vector<int64_t>* re,
                    std::vector<int64_t>* so) {
  int64_t cur_s = -1, cur_e = -1, last = 0;
  auto add = [&](int64_t s, int64_t e) {
    so->push_back(s);
    last = e;
    if (cur_s < 0) {
      cur_s = s, cur_e = e;
    } else if (e - cur_s <= S && s == cur_e) {
      cur_e = e;
    } else {
      rs->push_back(cur_s), re->push_back(cur_e);
      cur_s = s, cur_e = e;
    }
  };
  for (size_t i = 0; i + 1 < offs.size(); ++i) {
    int64_t s = offs[i];
    const int64_t e = offs[i + 1];
    for (; e - s > S; s += S) add(s, s + S);
    if (e > s) add(s, e);
  }
  if (cur_s >= 0) rs->push_back(cur_s), re->push_back(cur_e);
  so->push_back(last);
}

}  // namespace
