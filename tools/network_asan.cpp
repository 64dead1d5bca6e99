// Address and undefined-behaviour check of the host network build (csrc/network_host.cpp), as a program of its own:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include tools/network_asan.cpp ddr_amd/csrc/network_host.cpp -o network_asan && ./network_asan
// It builds the cycle tables of tests/network_cases.py (self-loop, 2-cycle, cycles of 3, 5 and 7 with tails, a cycle
// with a tail of 5 and side reaches, two cycles, nothing but a cycle), a 4097-reach chain in reversed row order, the
// int64 extremes and a duplicate, checks the contract on each result and prints one line per table.  No GPU, no HIP
// call: the error plumbing of capi.cpp is replaced below.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../ddr_amd/csrc/internal.h"
#include "../ddr_amd/csrc/network.h"

namespace ddr {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
ddr_status fail(ddr_status code, const std::string& msg) {
  g_error = msg;
  return code;
}
}  // namespace ddr

namespace {

struct Table {
  std::string name;
  std::vector<int64_t> ids, to;
  int64_t dropped;
  void add(int64_t id, int64_t t) {
    ids.push_back(id);
    to.push_back(t);
  }
};

// a cycle of `length` reaches from `base`, a tail of `tail` reaches draining into its middle, optionally two side reaches
void add_cycle(Table& t, int64_t base, int length, int tail, bool branch) {
  for (int k = 0; k < length; ++k) t.add(base + k, base + (k + 1) % length);
  int64_t prev = base + length / 2;
  for (int k = 0; k < tail; ++k) {
    t.add(base + 500 + k, prev);
    prev = base + 500 + k;
  }
  if (branch) {
    t.add(base + 900, tail ? base + 500 + tail / 2 : base);
    t.add(base + 901, base);
  }
  t.dropped += length;
}
void add_reversed_chain(Table& t, int64_t base, int length) {
  for (int k = 0; k < length; ++k) t.add(base + k, k ? base + k - 1 : 0);
}

int check(const Table& t) {
  ddr::Network* nw = nullptr;
  const int64_t n = (int64_t)t.ids.size();
  const ddr_status st = ddr::network_build_host(n, t.ids.data(), t.to.data(), &nw);
  if (st != DDR_OK) {
    std::printf("%-24s FAILED: %s\n", t.name.c_str(), ddr::g_error.c_str());
    return 1;
  }
  int bad = 0;
  bad += nw->n_dropped != t.dropped || nw->kept != n - t.dropped;
  bad += (int64_t)nw->position.size() != nw->kept || (int64_t)nw->rows.size() != nw->nnz;
  bad += nw->n_basins != nw->kept - nw->nnz;
  for (int64_t e = 0; e < nw->nnz; ++e) bad += !(nw->rows[e] > nw->cols[e] && nw->rows[e] < nw->kept);
  for (int64_t k = 0; k < nw->kept; ++k) bad += nw->order[k] != t.ids[nw->position[k]];
  std::printf("%-24s rows %6lld kept %6lld edges %6lld basins %4lld depth %5lld dropped %3lld  %s\n", t.name.c_str(),
              (long long)n, (long long)nw->kept, (long long)nw->nnz, (long long)nw->n_basins,
              (long long)nw->max_depth, (long long)nw->n_dropped, bad ? "WRONG" : "ok");
  ddr::network_destroy(nw);
  return bad != 0;
}

}  // namespace

namespace ddr {
void network_destroy(Network* nw) { delete nw; }  // (network.hip's, without the device block)
}  // namespace ddr

int main() {
  std::vector<Table> tables;
  auto start = [&](const char* name) -> Table& {
    tables.push_back(Table{name, {}, {}, 0});
    return tables.back();
  };
  {
    Table& t = start("self-loop");
    add_reversed_chain(t, 10, 5);
    add_cycle(t, 1000, 1, 2, false);
  }
  {
    Table& t = start("two-cycle");
    add_cycle(t, 1000, 2, 1, false);
    add_reversed_chain(t, 10, 5);
  }
  for (int len : {3, 5, 7}) {
    Table& t = start("cycle");
    t.name += std::to_string(len);
    add_reversed_chain(t, 10, 5);
    add_cycle(t, 1000, len, 3, false);
  }
  {
    Table& t = start("cycle-tail5-branch");
    add_cycle(t, 1000, 4, 5, true);
    add_reversed_chain(t, 10, 5);
  }
  {
    Table& t = start("two-cycles");
    add_cycle(t, 1000, 3, 2, false);
    add_reversed_chain(t, 10, 5);
    add_cycle(t, 5000, 5, 1, true);
  }
  add_cycle(start("only-a-cycle"), 1000, 6, 0, false);
  add_reversed_chain(start("reversed-chain4097"), 10, 4097);
  {
    Table& t = start("int64-extremes");
    t.add(INT64_MIN, -1);
    t.add(-1, 0);
    t.add(0, INT64_MAX);
    t.add(INT64_MAX, 12345);
    t.add(7, INT64_MIN);
  }
  start("empty");
  int bad = 0;
  for (const Table& t : tables) bad += check(t);
  // refusals leave nothing behind
  ddr::Network* nw = nullptr;
  const int64_t dup[] = {5, 9, 7, 9, 5};
  bad += ddr::network_build_host(5, dup, dup, &nw) != DDR_ERR_ARG || nw != nullptr;
  std::printf("%-24s %s\n", "duplicate", ddr::g_error.c_str());
  int32_t pos[5];
  bad += ddr::network_lookup_host(3, dup, 5, dup, pos) != DDR_OK || pos[3] != 1 || pos[4] != 0;
  std::printf("%s\n", bad ? "FAILED" : "all ok");
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
