// map_build_main.cpp — stand-alone driver of the host map builder (csrc/sit_map_build.h) for
// tests/test_map_build_host.py, which compiles it with ASan + UBSan and runs it as a child process.
//
//   map_build_main <map.txt> <out prefix>
//
// map.txt: n_poly, then n_poly + 1 vertex offsets, then (east, north) per vertex as C hex floats.
// For real sizes 4 and 8 it writes the image to <out prefix>.<real size>.bin and prints the
// MapMeta fields as one JSON line (doubles as %a strings).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "sit_map_build.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <map.txt> <out prefix>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  int n_poly = 0;
  if (!(in >> n_poly) || n_poly <= 0 || n_poly > sit::kMaxPolys) { std::fprintf(stderr, "bad n_poly\n"); return 2; }
  std::vector<int32_t> offs(n_poly + 1);
  for (int32_t& o : offs)
    if (!(in >> o)) { std::fprintf(stderr, "bad offsets\n"); return 2; }
  for (int p = 0; p < n_poly; ++p)
    if (offs[0] != 0 || offs[p + 1] - offs[p] < 3) { std::fprintf(stderr, "bad ring %d\n", p); return 2; }
  const int nv = offs[n_poly];
  if (nv > sit::kMaxPolyVerts) { std::fprintf(stderr, "too many vertices\n"); return 2; }
  std::vector<double> verts(2 * (size_t)nv);
  std::string tok;
  for (double& v : verts) {
    if (!(in >> tok)) { std::fprintf(stderr, "bad vertices\n"); return 2; }
    v = std::strtod(tok.c_str(), nullptr);
  }
  for (size_t rs : {size_t(4), size_t(8)}) {
    const sit::MapImage img = sit::build_map_image(n_poly, offs.data(), verts.data(), rs);
    const sit::MapMeta& m = img.meta;
    const std::string path = std::string(argv[2]) + "." + std::to_string(rs) + ".bin";
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(img.bytes.data(), 1, img.bytes.size(), f) != img.bytes.size() || std::fclose(f) != 0) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      return 1;
    }
    std::printf("{\"real_size\": %zu, \"size\": %zu, \"idx_off\": %zu, \"fine_off\": %zu, \"frank_off\": %zu, "
                "\"crec_off\": %zu, \"clive_off\": %zu, \"ring_off\": %zu, \"bbox_off\": %zu, \"map_bytes\": %zu, "
                "\"n_poly\": %d, \"n_vert\": %d, \"use_index\": %d, \"use_cells\": %d, \"n_idx\": %lld, "
                "\"n_mixed\": %lld, \"n_live\": %lld",
                rs, img.bytes.size(), m.idx_off, m.fine_off, m.frank_off, m.crec_off, m.clive_off, m.ring_off,
                m.bbox_off, m.map_bytes, m.n_poly, m.n_vert, m.use_index, m.use_cells, (long long)m.n_idx,
                (long long)m.n_mixed, (long long)m.n_live);
    const char* const names[14] = {"gx0", "gy0", "ginvx", "ginvy", "by0", "binv", "fx0", "fy0", "finvx", "finvy",
                                   "min_n", "max_n", "min_e", "max_e"};
    const double vals[14] = {m.gx0, m.gy0, m.ginvx, m.ginvy, m.by0, m.binv, m.fx0, m.fy0, m.finvx, m.finvy,
                             m.min_n, m.max_n, m.min_e, m.max_e};
    for (int i = 0; i < 14; ++i) std::printf(", \"%s\": \"%a\"", names[i], vals[i]);
    std::printf("}\n");
  }
  return 0;
}
