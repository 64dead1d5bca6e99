// kan.hip: the reference's parameter network (src/ddr/nn/kan.py:11-62: Linear -> pykan KAN([H, H]) layers ->
// Linear -> sigmoid).  This header holds what is plain host C++ -- the supported envelope and the offsets of
// the flat trainable vector and of the constants vector -- so that a stand-alone program can exercise it
// (tools/kan_desc_check.cpp, built with the host sanitizers); the launchers are declared for HIP callers.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/ddr_mc.h"

namespace ddr {

constexpr int kKanMaxF = 32, kKanMaxH = 32, kKanMaxO = 8, kKanMaxL = 4, kKanMaxK = 3;
constexpr int kKanMaxTable = 32768;  // H * H * (G + k) floats: one layer's coefficient table in LDS

// "" for a supported architecture, else a message naming the limit it breaks
inline std::string kan_validate(const ddr_kan_desc* d) {
  if (!d) return "kan: null descriptor";
  if (d->n_features < 1 || d->n_features > kKanMaxF) return "kan: 1 <= n_features <= 32";
  if (d->hidden < 1 || d->hidden > kKanMaxH) return "kan: 1 <= hidden <= 32";
  if (d->n_outputs < 1 || d->n_outputs > kKanMaxO) return "kan: 1 <= n_outputs <= 8";
  if (d->n_layers < 1 || d->n_layers > kKanMaxL) return "kan: 1 <= n_layers <= 4";
  if (d->k < 1 || d->k > kKanMaxK) return "kan: 1 <= k <= 3";
  if (d->grid < 1) return "kan: grid >= 1";
  // (grid + k) <= 32768 before the product: no overflow for any int32 grid
  if (d->grid > kKanMaxTable || (int64_t)d->hidden * d->hidden * ((int64_t)d->grid + d->k) > kKanMaxTable)
    return "kan: hidden * hidden * (grid + k) <= 32768 floats";
  return "";
}

// Offsets (in floats) of a validated descriptor.
//   flat trainable vector:  input.weight (H, F) | input.bias (H) | per layer: coef (H, H, G + k) [in, out, j] |
//                           scale_base (H, H) [in, out] | scale_sp (H, H) | ... | output.weight (O, H) | output.bias (O)
//   constants vector:       per layer: grid (H, G + 1 + 2k) | mask (H, H) [in, out] | node_scale (H) | node_bias (H) |
//                           subnode_scale (H) | subnode_bias (H)
struct KanLayout {
  int F, H, O, L, G, K;
  explicit KanLayout(const ddr_kan_desc& d)
      : F(d.n_features), H(d.hidden), O(d.n_outputs), L(d.n_layers), G(d.grid), K(d.k) {}
  int gk() const { return G + K; }           // bases per input
  int nk() const { return G + 1 + 2 * K; }   // knots per input
  int w_in() const { return 0; }
  int b_in() const { return H * F; }
  int layer_size() const { return H * H * gk() + 2 * H * H; }
  int coef(int l) const { return b_in() + H + l * layer_size(); }
  int scale_base(int l) const { return coef(l) + H * H * gk(); }
  int scale_sp(int l) const { return scale_base(l) + H * H; }
  int w_out() const { return coef(L); }
  int b_out() const { return w_out() + O * H; }
  int total() const { return b_out() + O; }
  int const_layer_size() const { return H * nk() + H * H + 4 * H; }
  int c_grid(int l) const { return l * const_layer_size(); }
  int c_mask(int l) const { return c_grid(l) + H * nk(); }
  int c_node_scale(int l) const { return c_mask(l) + H * H; }
  int c_node_bias(int l) const { return c_node_scale(l) + H; }
  int c_sub_scale(int l) const { return c_node_bias(l) + H; }
  int c_sub_bias(int l) const { return c_sub_scale(l) + H; }
  int const_total() const { return L * const_layer_size(); }
};

#ifndef DDR_KAN_HOST_ONLY
int kan_partial_groups();  // workgroups of the backward's persistent launches (one gradient partial each)
int64_t kan_work_bytes(const ddr_kan_desc& d, int64_t N, bool backward);
hipError_t launch_kan_forward(const ddr_kan_desc& d, int64_t N, const float* X, const float* P, const float* C,
                              float* h_save, float* U, void* work, hipStream_t stream);
hipError_t launch_kan_backward(const ddr_kan_desc& d, int64_t N, const float* X, const float* P, const float* C,
                               const float* h_save, const float* U, const float* gU, float* grad, void* work,
                               hipStream_t stream);
#endif

}  // namespace ddr
