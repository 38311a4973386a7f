// variant_check — csrc/variant_policy.h, the text the library's launch code
// calls, built for the host and run over the cases of a JSON file
// (tests/test_variant_policy.py: tests/golden/variant_policy.json).
//
// The file's "groups" is an array of arrays of 18 integers:
//   table (0 product, 1 diagnostic), (n_nodes, depth, blob_f4) of the three
//   trees, n_pad, unit_albedo, width, height, rows, spp, RTCLJ_TH4's ratio, the
//   resident workgroups of variant 22
// Each group is crossed with the selectors 0..29; one line per case:
//   group selector rt_resolve_variant launch-variant dynamic-LDS-bytes
//   stack-entries-per-lane threads tile-rows feature-source feature-LDS-bytes
// with -1 throughout for a selector the table lacks (rt_set_variant refuses it).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../raytracing-clj_amd/csrc/variant_policy.h"

using namespace rtclj::policy;

static std::vector<std::vector<long long>> read_groups(const char* path) {
  std::ifstream f(path);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string s = ss.str();
  std::vector<std::vector<long long>> out;
  size_t i = s.find("\"groups\"");
  if (i == std::string::npos) return out;
  i = s.find('[', i);
  int depth = 0;
  for (; i < s.size(); ++i) {
    const char ch = s[i];
    if (ch == '[') {
      if (++depth == 2) out.emplace_back();
    } else if (ch == ']') {
      if (--depth == 0) break;
    } else if (depth == 2 && (ch == '-' || (ch >= '0' && ch <= '9'))) {
      char* end = nullptr;
      out.back().push_back(std::strtoll(s.c_str() + i, &end, 10));
      i = static_cast<size_t>(end - s.c_str()) - 1;
    }
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: variant_check cases.json\n");
    return 2;
  }
  const auto groups = read_groups(argv[1]);
  if (groups.empty()) {
    std::fprintf(stderr, "variant_check: no \"groups\" in %s\n", argv[1]);
    return 2;
  }
  for (size_t g = 0; g < groups.size(); ++g) {
    const auto& q = groups[g];
    if (q.size() != 18) {
      std::fprintf(stderr, "variant_check: group %zu has %zu fields, not 18\n", g, q.size());
      return 2;
    }
    const bool diag = q[0] != 0;
    Scene ds{};
    for (int k = 0; k < 3; ++k)
      ds.tree[k] = Tree{static_cast<int>(q[1 + 3 * k]), static_cast<int>(q[2 + 3 * k]), static_cast<int>(q[3 + 3 * k])};
    ds.n_pad = static_cast<int>(q[10]);
    ds.unit_albedo = q[11] != 0;
    const Frame p{static_cast<int>(q[12]), static_cast<int>(q[13]), static_cast<int>(q[14]), static_cast<int>(q[15])};
    const int ratio = static_cast<int>(q[16]), slots = static_cast<int>(q[17]);
    // (the selectors the file records, 0..29: variant 30, 22 without the tile
    // list, is explicit only and launches as 22 does -- tests/test_gpu_tile_list.py)
    for (int sel = 0; sel < 30; ++sel) {
      if (!has_variant(sel, diag)) {
        std::printf("%zu %d -1 -1 -1 -1 -1 -1 -1 -1\n", g, sel);
        continue;
      }
      const int vsel = launch_variant(ds, p, sel, diag, ratio, slots);
      const Traits& v = traits(vsel, diag);
      const int src = feat_source(ds, sel, diag);
      std::printf("%zu %d %d %d %zu %d %d %d %d %zu\n", g, sel, resolve_variant(ds, sel, diag), vsel,
                  launch_lds(ds, vsel, diag), launch_stack(ds, v), v.threads, variant_rows(v), src, feat_lds(ds, src));
    }
  }
  return 0;
}
