// bvh_check.cpp — host-side dump of bvh_build (raytracing-clj_amd/csrc/bvh.cpp)
// for tests/test_oracle_input_edges.py: for every file of n x 4 float32
// (centre, radius) on the command line and every leaf size (2, 4, 8), one
// JSON line with the tree's centre, radius and r_max, whether every node box
// is finite, and the bodies of every leaf (the tree's leaves, then the
// big-body leaves), so a test can see where a body went.
//
//   g++ -O2 -std=c++17 -Icsrc -o lib/bvh_check ../tools/bvh_check.cpp csrc/bvh.cpp
#include <cmath>
#include <cstdio>
#include <vector>

#include "bvh.h"

namespace {

void num(float v) {   // JSON has no NaN / Infinity: they go out as strings
  if (std::isfinite(v)) std::printf("%.9g", v);
  else std::printf("\"%s\"", std::isnan(v) ? "nan" : v > 0 ? "inf" : "-inf");
}

}  // namespace

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::fprintf(stderr, "bvh_check: cannot read %s\n", argv[a]);
      return 2;
    }
    std::vector<float> sph;
    float v[4];
    while (std::fread(v, sizeof(float), 4, f) == 4) sph.insert(sph.end(), v, v + 4);
    std::fclose(f);
    const int n = static_cast<int>(sph.size() / 4);
    for (int leaf : {2, 4, 8}) {
      rtclj::BvhHost h;
      rtclj::bvh_build(sph.data(), n, &h, leaf, true);
      bool boxes = true;
      for (const rtclj::BvhNode& nd : h.nodes)
        for (int k = 0; k < 6; ++k) boxes = boxes && std::isfinite(nd.x[k]) && std::isfinite(nd.y[k]) && std::isfinite(nd.z[k]);
      std::printf("{\"file\": \"%s\", \"n\": %d, \"leaf_size\": %d, \"center\": [", argv[a], n, leaf);
      for (int k = 0; k < 3; ++k) {
        if (k) std::printf(", ");
        num(h.center[k]);
      }
      std::printf("], \"radius\": ");
      num(h.radius);
      std::printf(", \"r_max\": ");
      num(h.r_max);
      std::printf(", \"boxes_finite\": %s, \"n_nodes\": %zu, \"depth\": %d, \"n_big_leaves\": %d, \"big_leaf0\": %d, \"leaves\": [",
                  boxes ? "true" : "false", h.nodes.size(), h.depth, h.n_big_leaves, h.big_pair0 / (leaf / 2));
      const size_t per = static_cast<size_t>(leaf);
      for (size_t i = 0; i < h.pidx.size(); i += per) {
        std::printf("%s[", i ? ", " : "");
        for (size_t j = 0; j < per && i + j < h.pidx.size(); ++j) std::printf("%s%d", j ? ", " : "", h.pidx[i + j]);
        std::printf("]");
      }
      std::printf("]}\n");
    }
  }
  return 0;
}
