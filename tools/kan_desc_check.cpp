// Stand-alone host check of csrc/kan.h: the KAN descriptor validation (kan_validate) and the offset arithmetic
// of the flat trainable vector and the constants vector (KanLayout), over the envelope's corner descriptors and
// descriptors just outside it.  Plain host C++ (no HIP); build it with the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DDDR_KAN_HOST_ONLY \
//       tools/kan_desc_check.cpp -o kan_desc_check && ./kan_desc_check
// Every offset is used to write into buffers of exactly param_count / const_count floats, so an offset past the
// end is an AddressSanitizer report and a signed overflow an UndefinedBehaviorSanitizer one.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ddr_amd/csrc/kan.h"

using ddr::KanLayout;

static int g_fail = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                              \
    }                                                        \
  } while (0)

// fill [off, off + n) with `tag`, checking the range was untouched: the pieces tile the vector without overlap
static void fill(std::vector<float>& v, int off, int n, float tag) {
  CHECK(off >= 0 && n >= 0);
  for (int e = 0; e < n; ++e) {
    CHECK(v.data()[off + e] == 0.0f);
    v.data()[off + e] = tag;
  }
}

static void check_layout(const ddr_kan_desc& d) {
  CHECK(ddr::kan_validate(&d).empty());
  const KanLayout L(d);
  std::vector<float> p(L.total(), 0.0f), c(L.const_total(), 0.0f);
  float tag = 1.0f;
  fill(p, L.w_in(), L.H * L.F, tag++);
  fill(p, L.b_in(), L.H, tag++);
  for (int l = 0; l < L.L; ++l) {
    fill(p, L.coef(l), L.H * L.H * L.gk(), tag++);
    fill(p, L.scale_base(l), L.H * L.H, tag++);
    fill(p, L.scale_sp(l), L.H * L.H, tag++);
    fill(c, L.c_grid(l), L.H * L.nk(), tag++);
    fill(c, L.c_mask(l), L.H * L.H, tag++);
    fill(c, L.c_node_scale(l), L.H, tag++);
    fill(c, L.c_node_bias(l), L.H, tag++);
    fill(c, L.c_sub_scale(l), L.H, tag++);
    fill(c, L.c_sub_bias(l), L.H, tag++);
  }
  fill(p, L.w_out(), L.O * L.H, tag++);
  fill(p, L.b_out(), L.O, tag++);
  for (float v : p) CHECK(v != 0.0f);
  for (float v : c) CHECK(v != 0.0f);
}

int main() {
  // the published checkpoints' architecture: 47 925 trainable values
  const ddr_kan_desc ckpt{10, 21, 3, 2, 50, 2};
  check_layout(ckpt);
  CHECK(KanLayout(ckpt).total() == 47925);
  // the envelope's corners: every combination of the extreme F, H, O, L, k with the smallest and the largest grid
  // that H H (G + k) <= 32768 allows
  int corners = 0;
  for (int F : {1, 32})
    for (int H : {1, 2, 31, 32})
      for (int O : {1, 8})
        for (int L : {1, 4})
          for (int k : {1, 3}) {
            const int gmax = 32768 / (H * H) - k;
            for (int G : {1, gmax}) {
              check_layout(ddr_kan_desc{F, H, O, L, G, k});
              ++corners;
            }
            const ddr_kan_desc over{F, H, O, L, gmax + 1, k};
            CHECK(!ddr::kan_validate(&over).empty());
          }
  // just outside, and values that would overflow 32-bit products
  const int big = 2147483647;
  const ddr_kan_desc outside[] = {{0, 21, 3, 2, 50, 2},  {33, 21, 3, 2, 50, 2}, {10, 0, 3, 2, 50, 2},   {10, 33, 3, 2, 50, 2},
                                  {10, 21, 0, 2, 50, 2}, {10, 21, 9, 2, 50, 2}, {10, 21, 3, 0, 50, 2},  {10, 21, 3, 5, 50, 2},
                                  {10, 21, 3, 2, 0, 2},  {10, 21, 3, 2, 50, 0}, {10, 21, 3, 2, 50, 4},  {10, 21, 3, 2, big, 3},
                                  {big, big, big, big, big, big},               {-1, -1, -1, -1, -1, -1}, {10, 32, 3, 2, 30, 3},
                                  {10, 1, 3, 2, 32768, 1}};
  for (const ddr_kan_desc& d : outside) CHECK(!ddr::kan_validate(&d).empty());
  CHECK(!ddr::kan_validate(nullptr).empty());
  std::printf("kan_desc_check: %d corner descriptors, %d failures\n", corners, g_fail);
  return g_fail ? 1 : 0;
}
