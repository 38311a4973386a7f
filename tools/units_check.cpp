// units_check — the fused budget trace's unit table on the host (csrc/budget.h:
// bd_host_units, the body of rt_budget_units_host, with bd_units_at, the text
// budget_units_kernel runs) built for the host under the sanitizers, over
// random plans and the edge cases of the packed fields.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -static-libasan -static-libubsan tools/units_check.cpp
//
// Every array is a heap block of exactly its size (the table: the sum of the
// multipliers), so a slot outside the table is a report.  Checked besides: per
// half the table is exactly {(tile, 2 j + h) : j < mult[tile]}, each once;
// block-major, in list order within a block; y >> 8 == 2 max_mult and y & 255
// <= 31; a single tile, all ones, all max_mult and max_mult = 16; bad
// arguments and lists out of order are refused with nothing written.  One JSON
// line; exit status 0 when everything held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <numeric>
#include <vector>

#include "../include/rt.h"
#include "../raytracing-clj_amd/csrc/budget.h"

using namespace rtclj;

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};

long g_bad = 0, g_calls = 0, g_entries = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    ++g_bad;
    std::fprintf(stderr, "units_check: %s\n", what);
  }
}

// the tiles by descending multiplier, equal multipliers shuffled
std::vector<int32_t> list_of(const std::vector<uint32_t>& mult, Rng& rng) {
  std::vector<int32_t> list(mult.size());
  std::iota(list.begin(), list.end(), 0);
  for (size_t i = list.size(); i > 1; --i) std::swap(list[i - 1], list[rng.next() % i]);
  std::stable_sort(list.begin(), list.end(), [&](int32_t a, int32_t b) { return mult[a] > mult[b]; });
  return list;
}

// one plan: both halves against the definition
void check_plan(const std::vector<uint32_t>& mult, int max_mult, Rng& rng) {
  const int n = static_cast<int>(mult.size());
  const std::vector<int32_t> list = list_of(mult, rng);
  size_t total = 0;
  for (uint32_t m : mult) total += m;
  // exactly n items on the heap (no slack behind them)
  std::unique_ptr<int32_t[]> lp(new int32_t[n]);
  std::unique_ptr<uint32_t[]> mp(new uint32_t[n]);
  std::copy(list.begin(), list.end(), lp.get());
  std::copy(mult.begin(), mult.end(), mp.get());
  for (int h = 0; h < 2; ++h) {
    std::unique_ptr<int32_t[]> out(new int32_t[2 * total]);
    const char* why = nullptr;
    const int got = bd_host_units(lp.get(), mp.get(), n, max_mult, h, out.get(), &why);
    ++g_calls;
    expect(got == static_cast<int>(total), "the table holds the sum of the multipliers");
    if (got != static_cast<int>(total)) continue;
    g_entries += got;
    size_t u = 0;
    std::vector<int> seen(static_cast<size_t>(n) * max_mult, 0);
    for (int j = 0; j < max_mult; ++j)        // block-major
      for (int i = 0; i < n; ++i) {           // in list order
        if (mult[list[i]] <= static_cast<uint32_t>(j)) continue;
        const int x = out[2 * u], y = out[2 * u + 1];
        expect(x == list[i] && (y & 255) == 2 * j + h, "slot order: pass by pass, the list's order within a pass");
        expect((y >> 8) == 2 * max_mult && (y & 255) <= 31, "the packed fields");
        if (x >= 0 && x < n && (y & 255) / 2 < max_mult) ++seen[static_cast<size_t>(x) * max_mult + (y & 255) / 2];
        ++u;
      }
    expect(u == total, "every slot accounted for");
    for (int t = 0; t < n; ++t)
      for (int j = 0; j < max_mult; ++j)
        expect(seen[static_cast<size_t>(t) * max_mult + j] == (static_cast<uint32_t>(j) < mult[t] ? 1 : 0),
               "exactly the set {(tile, 2 j + h) : j < mult[tile]}");
  }
}

void refusals() {
  const uint32_t mult[4] = {3, 1, 2, 3};
  const int32_t good[4] = {0, 3, 2, 1};
  int32_t out[18];
  const char* why = nullptr;
  auto refused = [&](const int32_t* l, const uint32_t* m, int n, int mm, int h, int32_t* o, const char* what) {
    std::fill(out, out + 18, 77);
    ++g_calls;
    expect(bd_host_units(l, m, n, mm, h, o, &why) == RT_E_ARG && why != nullptr &&
               std::all_of(out, out + 18, [](int32_t v) { return v == 77; }),
           what);
  };
  ++g_calls;
  expect(bd_host_units(good, mult, 4, 3, 0, out, &why) == 9 && why == nullptr, "the good call");
  refused(nullptr, mult, 4, 3, 0, out, "NULL list refused");
  refused(good, nullptr, 4, 3, 0, out, "NULL mult refused");
  refused(good, mult, 4, 3, 0, nullptr, "NULL output refused");
  refused(good, mult, 0, 3, 0, out, "n_tiles 0 refused");
  refused(good, mult, -4, 3, 0, out, "n_tiles < 0 refused");
  refused(good, mult, 4, 0, 0, out, "max_mult 0 refused");
  refused(good, mult, 4, 17, 0, out, "max_mult 17 refused");
  refused(good, mult, 4, 2, 0, out, "a multiplier above max_mult refused");
  refused(good, mult, 4, 3, 2, out, "half 2 refused");
  refused(good, mult, 4, 3, -1, out, "half -1 refused");
  const uint32_t zero[4] = {3, 0, 2, 3};
  refused(good, zero, 4, 3, 0, out, "a multiplier of 0 refused");
  const int32_t ascending[4] = {1, 2, 0, 3}, swapped[4] = {0, 2, 3, 1}, twice[4] = {0, 0, 2, 1}, outside[4] = {0, 3, 2, 4},
                negative[4] = {0, 3, 2, -1};
  refused(ascending, mult, 4, 3, 0, out, "an ascending list refused");
  refused(swapped, mult, 4, 3, 0, out, "a list out of order refused");
  refused(twice, mult, 4, 3, 0, out, "a tile listed twice refused");
  refused(outside, mult, 4, 3, 0, out, "a list entry past the tiles refused");
  refused(negative, mult, 4, 3, 0, out, "a negative list entry refused");
}

}  // namespace

int main() {
  Rng rng{97531};
  // random plans: tile grids of 9 x 12, 33 x 17, 64 x 40, 1200 x 675 pixels
  for (const int n : {4, 15, 40, 12750})
    for (const int max_mult : {1, 2, 4, 16})
      for (int rep = 0; rep < (n > 1000 ? 1 : 4); ++rep) {
        std::vector<uint32_t> mult(n);
        for (uint32_t& m : mult) m = 1u + static_cast<uint32_t>(rng.next() % max_mult);
        if (rep == 1) mult[rng.next() % n] = max_mult;   // (one tile at the cap among the rest)
        check_plan(mult, max_mult, rng);
      }
  // the edges: a single tile, all ones (U = n_tiles), all max_mult, one tile at 16 and the rest low
  for (const int max_mult : {1, 4, 16}) {
    check_plan(std::vector<uint32_t>(1, 1u), max_mult, rng);
    check_plan(std::vector<uint32_t>(1, static_cast<uint32_t>(max_mult)), max_mult, rng);
    check_plan(std::vector<uint32_t>(15, 1u), max_mult, rng);
    check_plan(std::vector<uint32_t>(15, static_cast<uint32_t>(max_mult)), max_mult, rng);
  }
  {
    std::vector<uint32_t> mult(15);
    for (size_t t = 0; t < mult.size(); ++t) mult[t] = 1u + static_cast<uint32_t>(t % 3);
    mult[7] = 16u;
    check_plan(mult, 16, rng);
  }
  refusals();
  std::printf("{\"calls\": %ld, \"bad\": %ld, \"entries\": %ld}\n", g_calls, g_bad, g_entries);
  return g_bad == 0 && g_entries > 0 ? 0 : 1;
}
