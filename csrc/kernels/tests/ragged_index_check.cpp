// Host check of the ragged gather's index arithmetic (csrc/kernels/ragged_index.h), built with
// -fsanitize=address,undefined by tests/test_zerocopy_tokens.py. It runs the kernel's loops (ragged.hip)
// tile by tile, lane by lane, on the host: every 16-byte unit load is a memcpy out of a source buffer
// that is exactly the 16-byte aligned hull of the corpus, every store goes into a destination of exactly
// dst_offsets[n] elements, so a unit outside the hulls or an element outside the destination is a heap
// overflow. The result is compared with a plain per-sequence memcpy, and every destination element must
// be written exactly once.
#include <limits.h>
#include <string.h>

#include "../ragged_index.h"
#include "check_common.h"

namespace {

template <typename T>
void run_case(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& idx, int shift,
              int64_t max_blocks) {
  ++g_cases;
  constexpr int eb = static_cast<int>(sizeof(T));
  constexpr int per_unit = ddl::kRgUnitBytes / eb;
  std::vector<int64_t> offs(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) offs[i + 1] = offs[i] + lens[i];
  const int64_t total_src = offs.back();
  // the corpus starts `shift` elements into a 16-byte aligned allocation that ends with its hull
  const size_t hull_bytes = (static_cast<size_t>(shift + total_src) * eb + 15) / 16 * 16;
  uint8_t* raw = static_cast<uint8_t*>(aligned_alloc(16, hull_bytes ? hull_bytes : 16));
  for (size_t i = 0; i < hull_bytes; ++i) raw[i] = static_cast<uint8_t>(i * 131u + 7u);
  const uint64_t src = reinterpret_cast<uint64_t>(raw) + static_cast<uint64_t>(shift) * eb;

  const int64_t n = static_cast<int64_t>(idx.size());
  std::vector<int64_t> src_start(n ? n : 1), dst_offsets(n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    src_start[i] = offs[idx[i]];
    dst_offsets[i + 1] = dst_offsets[i] + lens[idx[i]];
  }
  std::vector<int32_t> tile_start(n + 1);
  const int64_t n_tiles = ddl::ragged_tile_plan(src, src_start.data(), dst_offsets.data(), n, eb, tile_start.data());
  const int64_t total = dst_offsets[n];
  T* dst = static_cast<T*>(malloc(total ? total * eb : 1));  // exact size: one element further is an overflow
  T* ref = static_cast<T*>(malloc(total ? total * eb : 1));
  std::vector<int> written(total, 0);
  for (int64_t i = 0; i < n; ++i)
    if (lens[idx[i]])
      memcpy(ref + dst_offsets[i], reinterpret_cast<const void*>(src + src_start[i] * eb), lens[idx[i]] * eb);

  const int64_t grid = (max_blocks > 0 && max_blocks < n_tiles) ? max_blocks : n_tiles;
  for (int64_t block = 0; block < grid; ++block) {
    for (int64_t tile = block; tile < n_tiles; tile += grid) {
      const int64_t seq = ddl::rg_find_seq([&](int64_t j) { return tile_start[j]; }, n, tile);
      if (seq < 0 || seq >= n || tile < tile_start[seq] || tile >= tile_start[seq + 1]) {
        printf("%s: tile %lld mapped to sequence %lld\n", name, (long long)tile, (long long)seq);
        ++g_failures;
        continue;
      }
      const int64_t chunk = tile - tile_start[seq];
      const int64_t d0 = dst_offsets[seq];
      const int64_t len = dst_offsets[seq + 1] - d0;
      const uint64_t a = src + static_cast<uint64_t>(src_start[seq]) * eb;
      const int64_t units = ddl::rg_units(a, len, eb);
      const int64_t head = ddl::rg_head_elems(a, eb);
      for (int tid = 0; tid < ddl::kRgThreads; ++tid) {
        T v[ddl::kRgUnroll][per_unit];
        for (int k = 0; k < ddl::kRgUnroll; ++k) {
          const int64_t u = ddl::rg_unit(chunk, k, tid);
          if (u < units) {
            const uint64_t ua = ddl::rg_unit_addr(a, u);
            if (ua % 16) fail(name, "unaligned unit");
            memcpy(v[k], reinterpret_cast<const void*>(ua), 16);  // the whole unit, as the lane's load
          }
        }
        for (int k = 0; k < ddl::kRgUnroll; ++k) {
          const int64_t u = ddl::rg_unit(chunk, k, tid);
          if (u < units) {
            for (int e = 0; e < per_unit; ++e) {
              const int64_t p = ddl::rg_elem_pos(u, e, head, eb);
              if (p >= 0 && p < len) {
                dst[d0 + p] = v[k][e];
                ++written[d0 + p];
              }
            }
          }
        }
      }
    }
  }
  bool ok = total == 0 || memcmp(dst, ref, total * eb) == 0;
  for (int64_t i = 0; i < total; ++i) ok = ok && written[i] == 1;
  if (!ok) {
    printf("%s (eb %d, shift %d, max_blocks %lld): mismatch\n", name, eb, shift, (long long)max_blocks);
    ++g_failures;
  }
  free(dst);
  free(ref);
  free(raw);
}

template <typename T>
void run_all() {
  // the wanted lengths, each behind a filler whose length walks the residues modulo 8 elements
  const std::vector<int64_t> wanted = {0, 1, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1000, 0, 5};
  std::vector<int64_t> lens, idx;
  lens.push_back(6);  // the corpus's first sequence
  int64_t at = 6;
  for (size_t i = 0; i < wanted.size(); ++i) {
    const int64_t fill = ((static_cast<int64_t>(i) - at) % 8 + 8) % 8;  // wanted sequence i starts at residue i % 8
    lens.push_back(fill);
    lens.push_back(wanted[i]);
    at += fill + wanted[i];
    idx.push_back(static_cast<int64_t>(lens.size()) - 1);
  }
  lens.push_back(11);  // the corpus's last sequence: its hull ends the allocation
  idx.push_back(0);
  idx.push_back(static_cast<int64_t>(lens.size()) - 1);
  idx.push_back(idx[9]);  // a repeated index
  idx.push_back(idx[12]);
  for (int shift : {0, 1, 3})
    for (int64_t mb : {0, 1, 4}) run_case<T>("shape list", lens, idx, shift, mb);
  // every start residue modulo 8 elements, for every short length
  for (int64_t len = 0; len <= 18; ++len)
    for (int64_t fill = 0; fill < 8; ++fill) run_case<T>("residues", {fill, len}, {1}, 0, 0);
  // sequences of several tiles (a tile is 16 KB of source)
  run_case<T>("long", {3, 20000, 5, 8192, 4096}, {1, 3, 4, 1}, 1, 4);
  // more sequences than the LDS cap of the tile map holds, short ones
  run_case<T>("many", mod_lens(5000, 13), stride_order(5000, 7, 0, 5000), 0, 4);
  run_case<T>("n = 0", {4, 5}, {}, 0, 0);
  run_case<T>("all empty", {0, 0, 3}, {0, 1, 0}, 0, 1);
}

// Far case: no memory behind the addresses, the index arithmetic alone, at a source address and sequence starts
// whose byte offsets pass 2^33. Every unit a lane would load must be 16-byte aligned and inside the sequence's hull,
// every surviving element must be the one at a + p * eb, and each position of each sequence must come exactly once.
template <typename T>
void far_case(const char* name, uint64_t src, const std::vector<int64_t>& src_start, const std::vector<int64_t>& lens) {
  ++g_cases;
  constexpr int eb = static_cast<int>(sizeof(T));
  constexpr int per_unit = ddl::kRgUnitBytes / eb;
  const int64_t n = static_cast<int64_t>(lens.size());
  std::vector<int64_t> dst_offsets(n + 1, 0);
  for (int64_t i = 0; i < n; ++i) dst_offsets[i + 1] = dst_offsets[i] + lens[i];
  std::vector<int32_t> tile_start(n + 1);
  const int64_t n_tiles = ddl::ragged_tile_plan(src, src_start.data(), dst_offsets.data(), n, eb, tile_start.data());
  if (n_tiles < 0) return fail(name, "a plan that fits int32 is refused");
  std::vector<int> written(dst_offsets[n], 0);
  for (int64_t tile = 0; tile < n_tiles; ++tile) {
    const int64_t seq = ddl::rg_find_seq([&](int64_t j) { return tile_start[j]; }, n, tile);
    if (seq < 0 || seq >= n || tile < tile_start[seq] || tile >= tile_start[seq + 1]) return fail(name, "tile map");
    const int64_t chunk = tile - tile_start[seq];
    const int64_t d0 = dst_offsets[seq], len = dst_offsets[seq + 1] - d0;
    const uint64_t a = src + static_cast<uint64_t>(src_start[seq]) * eb;
    if ((a - src) / eb != static_cast<uint64_t>(src_start[seq])) return fail(name, "sequence address wrapped");
    const int64_t units = ddl::rg_units(a, len, eb);
    const int64_t head = ddl::rg_head_elems(a, eb);
    const uint64_t hull_lo = a & ~uint64_t{15}, hull_hi = (a + static_cast<uint64_t>(len) * eb + 15) & ~uint64_t{15};
    for (int tid = 0; tid < ddl::kRgThreads; ++tid)
      for (int k = 0; k < ddl::kRgUnroll; ++k) {
        const int64_t u = ddl::rg_unit(chunk, k, tid);
        if (u >= units) continue;
        const uint64_t ua = ddl::rg_unit_addr(a, u);
        if (ua % 16 || ua < hull_lo || ua + 16 > hull_hi) return fail(name, "unit outside the hull");
        for (int e = 0; e < per_unit; ++e) {
          const int64_t p = ddl::rg_elem_pos(u, e, head, eb);
          if (p < 0 || p >= len) continue;
          if (ua + static_cast<uint64_t>(e) * eb != a + static_cast<uint64_t>(p) * eb) return fail(name, "element address");
          ++written[d0 + p];
        }
      }
  }
  for (int w : written)
    if (w != 1) return fail(name, "a position is not produced exactly once");
}

template <typename T>
void run_far() {
  constexpr int64_t eb = static_cast<int64_t>(sizeof(T));
  const int64_t far = (int64_t{1} << 33) / eb;  // the element at byte 2^33
  for (uint64_t shift : {0, 1, 3}) {
    const uint64_t src = (uint64_t{0x7f} << 40) + shift * eb;  // a plausible mapping address, element-aligned only
    far_case<T>("far starts", src, {far - 3, far + 5000, (int64_t{1} << 40) + 1, (int64_t{1} << 31) / eb - 1, 2 * far + 7},
                {5000, 0, 17, 9000, 1});
  }
  // ragged_tile_plan at its int32 limit: INT32_MAX tiles are accepted, one more is refused
  const int64_t per_tile = ddl::kRgTileUnits * (ddl::kRgUnitBytes / eb);  // elements per tile of an aligned sequence
  const uint64_t src = uint64_t{1} << 44;
  {
    ++g_cases;
    const std::vector<int64_t> start = {0, int64_t{INT32_MAX} * per_tile};
    std::vector<int64_t> dofs = {0, int64_t{INT32_MAX} * per_tile, int64_t{INT32_MAX} * per_tile};
    std::vector<int32_t> ts(3);
    if (ddl::ragged_tile_plan(src, start.data(), dofs.data(), 2, eb, ts.data()) != INT32_MAX || ts[1] != INT32_MAX ||
        ts[2] != INT32_MAX)
      fail("tile plan limit", "INT32_MAX tiles are not accepted");
    dofs[2] += 1;  // one more element: one more tile
    if (ddl::ragged_tile_plan(src, start.data(), dofs.data(), 2, eb, ts.data()) != -1)
      fail("tile plan limit", "2^31 tiles are not refused");
    dofs = {0, int64_t{INT32_MAX} * per_tile + 1, int64_t{INT32_MAX} * per_tile + 1};  // one sequence alone past it
    if (ddl::ragged_tile_plan(src, start.data(), dofs.data(), 1, eb, ts.data()) != -1)
      fail("tile plan limit", "a sequence of 2^31 tiles is not refused");
  }
}

}  // namespace

int main() {
  run_all<uint16_t>();
  run_all<uint32_t>();
  run_far<uint16_t>();
  run_far<uint32_t>();
  return finish("ragged index check");
}
