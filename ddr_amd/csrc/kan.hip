// The reference's parameter network (src/ddr/nn/kan.py:11-62), forward and backward, for gfx950:
//   attributes (N, F) -> Linear(F, H) -> L x pykan KAN([H, H]) -> Linear(H, O) -> sigmoid -> u (N, O) in [0, 1].
// The KAN layer restates pykan 0.2.x (MultKAN with width [H, H], no multiplication nodes, symbolic branch off):
//   B^0_j(x) = [t_j <= x < t_{j+1}]                                   (half-open: x at the last knot gives 0)
//   B^k_j(x) = (x - t_j) / (t_{j+k} - t_j) B^{k-1}_j(x) + (t_{j+k+1} - x) / (t_{j+k+1} - t_{j+1}) B^{k-1}_{j+1}(x)
//   y_o = sum_i mask[i,o] (scale_base[i,o] silu(h_i) + scale_sp[i,o] sum_j coef[i,o,j] B^k_j(h_i))
//   y   = node_scale (subnode_scale y + subnode_bias) + node_bias
// with per-input knot rows t = grid[i] (G + 1 + 2k knots, G + k bases); outside [t_0, t_last) only the SiLU
// branch is live.  pykan materialises every basis, an (N, H, G + k) tensor; here a row finds its knot interval
// m by a binary search of the stored knots and evaluates the k + 1 bases j = m - k .. m that can be non-zero
// with the same recursion, in fp32 and in the recursion's operation order (the absent terms are exact zeros).
//
// Forward: one persistent launch per KAN layer (one workgroup per CU over 512-row tiles, a lane per row).  A
// workgroup stages the layer's mask scale_sp coef table once in LDS as [i][j][o] with an odd [o] stride (lanes
// of a wave read it at different j); the input Linear is fused into the first layer's load, the output Linear
// and the sigmoid into the last layer's epilogue.  Saved for the backward: h^0 .. h^L (N x H each) and u.
//
// Backward (gradient of the flat trainable vector only; no input gradient), bitwise reproducible, no atomics:
// thread (i, o) of the layer kernel owns row [i][o][.] of an LDS gradient table and the (i, o) entries of
// scale_base / scale_sp; it walks a chunk's rows in order, reading each row's interval and bases from an LDS
// image the chunk's first phase wrote (recomputed from h^l), and does plain read-modify-writes on the k + 1
// entries it owns.  dL/dh is summed over o in a fixed order by thread (row, i).  The two Linears' gradients
// use the same ownership (thread (a, b) owns dW[a][b]).  Every workgroup writes one partial in the flat
// layout; kan_reduce_kernel sums the partials in ascending order.
#include <algorithm>
#include <atomic>

#include "internal.h"
#include "kan.h"

namespace ddr {

namespace {

constexpr int kKanFwdThreads = 512;          // rows per forward tile (a lane per row)
constexpr int kKanLdsFloats = 160 * 1024 / 4;  // LDS a workgroup may declare
constexpr int kKanLinRows = 32;              // rows per tile of the Linear weight-gradient kernel
constexpr int kKanMaxChunk = 16;             // rows per chunk of the layer backward
constexpr int kKanAhead = 4;                 // rows whose coefficients a thread of it loads ahead

__device__ __forceinline__ float ksigm(float x) { return 1.0f / (1.0f + expf(-x)); }
// s += v with Kahan's compensation c (the build forms no FMA and reassociates nothing): the register sums of
// the backward run over every row a workgroup owns, thousands at C3's size
__device__ __forceinline__ void kan_add(float& s, float& c, float v) {
  const float y = v - c, t = s + y;
  c = (t - s) - y;
  s = t;
}

// Knot interval of x in a strictly increasing row t[0 .. NK): the m with t[m] <= x < t[m + 1], or -1 outside
// [t[0], t[NK - 1]) (and for NaN).  Always 0 <= m <= NK - 2, whatever the row holds.
__device__ __forceinline__ int kan_interval(const float* t, int NK, float x) {
  if (!(x >= t[0] && x < t[NK - 1])) return -1;
  int lo = 0, hi = NK - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (x >= t[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// b[jj] = B^K_j(x), and (D) db[jj] = d/dx B^K_j(x), for j = m - K + jj, jj = 0 .. K; a basis that does not exist
// (j < 0 or j >= G + K) is 0.  A basis of order d exists for 0 <= j and j + d + 1 <= NK - 1, and then so do the two
// of order d - 1 it is built from, so no knot outside the row is read.
// d/dx B^K_j = K / (t_{j+K} - t_j) B^{K-1}_j - K / (t_{j+K+1} - t_{j+1}) B^{K-1}_{j+1}.
template <int K, bool D>
__device__ __forceinline__ void kan_bases(const float* t, int NK, int m, float x, float (&b)[K + 1], float (&db)[K + 1]) {
#pragma unroll
  for (int jj = 0; jj < K; ++jj) b[jj] = 0.0f;
  b[K] = 1.0f;
#pragma unroll
  for (int d = 1; d <= K; ++d) {
    if (D && d == K) {
#pragma unroll
      for (int jj = 0; jj <= K; ++jj) {
        const int j = m - K + jj;
        float v = 0.0f;
        if (j >= 0 && j + K + 1 <= NK - 1) {
          const float right = jj < K ? b[jj + 1] : 0.0f;
          v = (float)K / (t[j + K] - t[j]) * b[jj] - (float)K / (t[j + K + 1] - t[j + 1]) * right;
        }
        db[jj] = v;
      }
    }
#pragma unroll
    for (int jj = K - d; jj <= K; ++jj) {  // ascending in place: b[jj + 1] is still the order d - 1 value
      const int j = m - K + jj;
      float v = 0.0f;
      if (j >= 0 && j + d + 1 <= NK - 1) {
        const float right = jj < K ? b[jj + 1] : 0.0f;
        v = (x - t[j]) / (t[j + d] - t[j]) * b[jj] + (t[j + d + 1] - x) / (t[j + d + 1] - t[j + 1]) * right;
      }
      b[jj] = v;
    }
  }
}

struct KanFwdArgs {
  int64_t N;
  int32_t ntiles, F, H, O, GK, NK, HP;
  int32_t first, last, knots_lds;
  const float* X;      // (N, F): the first layer's input
  const float* hin;    // (N, H): another layer's input
  float* h0;           // first layer: where h^0 is saved (or null)
  float* hout;         // (N, H): the layer's output (null: not stored)
  float* U;            // last layer: (N, O)
  const float *Win, *bin, *coef, *sbase, *ssp, *Wout, *bout;
  const float *grid, *mask, *nscale, *nbias, *sscale, *sbias;
};

template <int HT, int K>
__global__ void __launch_bounds__(kKanFwdThreads) kan_layer_fwd_kernel(KanFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ksm[];
  const int H = a.H, GK = a.GK, NK = a.NK, HP = a.HP, F = a.F, tid = threadIdx.x;
  float* tab = ksm;               // [i][j][o], stride HP: mask scale_sp coef
  float* mbase = tab + H * GK * HP;  // [i][o], stride HP: mask scale_base
  float* knl = mbase + H * HP;    // [i][NK]: the knots (when they fit)
  for (int e = tid; e < H * H * GK; e += kKanFwdThreads) {  // e = (i, o, j) of coef
    const int i = e / (H * GK), r = e - i * H * GK, o = r / GK, j = r - o * GK;
    tab[(i * GK + j) * HP + o] = a.mask[i * H + o] * a.ssp[i * H + o] * a.coef[e];
  }
  for (int e = tid; e < H * H; e += kKanFwdThreads) mbase[(e / H) * HP + e % H] = a.mask[e] * a.sbase[e];
  const float* kn = a.grid;
  if (a.knots_lds) {
    for (int e = tid; e < H * NK; e += kKanFwdThreads) knl[e] = a.grid[e];
    kn = knl;
  }
  __syncthreads();

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t row = (int64_t)tile * kKanFwdThreads + tid;
    if (row >= a.N) continue;  // no barrier below
    float acc[HT];
#pragma unroll
    for (int o = 0; o < HT; ++o) acc[o] = 0.0f;
    for (int i = 0; i < H; ++i) {
      float h;
      if (a.first) {
        h = 0.0f;
        for (int f = 0; f < F; ++f) h += a.X[row * F + f] * a.Win[i * F + f];
        h += a.bin[i];
        if (a.h0) a.h0[row * H + i] = h;
      } else {
        h = a.hin[row * H + i];
      }
      const float s = h * ksigm(h);
      const float* kt = kn + i * NK;
      const int m = kan_interval(kt, NK, h);
      const float* mb = mbase + i * HP;
      if (m < 0) {
#pragma unroll
        for (int o = 0; o < HT; ++o)
          if (o < H) acc[o] += mb[o] * s;
        continue;
      }
      float b[K + 1], db[K + 1];
      kan_bases<K, false>(kt, NK, m, h, b, db);
      const float* tp[K + 1];
#pragma unroll
      for (int jj = 0; jj <= K; ++jj) {
        const int j = m - K + jj;
        const bool ok = j >= 0 && j < GK;  // (b is 0 for a basis that does not exist)
        tp[jj] = tab + (i * GK + (ok ? j : 0)) * HP;
      }
#pragma unroll
      for (int o = 0; o < HT; ++o)
        if (o < H) {
          float sp = 0.0f;
#pragma unroll
          for (int jj = 0; jj <= K; ++jj) sp += tp[jj][o] * b[jj];
          acc[o] += mb[o] * s + sp;
        }
    }
    float zq[kKanMaxO];
#pragma unroll
    for (int q = 0; q < kKanMaxO; ++q) zq[q] = 0.0f;
#pragma unroll
    for (int o = 0; o < HT; ++o)
      if (o < H) {
        const float y = a.nscale[o] * (a.sscale[o] * acc[o] + a.sbias[o]) + a.nbias[o];
        if (a.hout) a.hout[row * H + o] = y;
        if (a.last) {
#pragma unroll
          for (int q = 0; q < kKanMaxO; ++q)
            if (q < a.O) zq[q] += y * a.Wout[q * H + o];
        }
      }
    if (a.last) {
#pragma unroll
      for (int q = 0; q < kKanMaxO; ++q)
        if (q < a.O) a.U[row * a.O + q] = ksigm(zq[q] + a.bout[q]);
    }
  }
}

// dz = dL/du u (1 - u) (N, O) and dL/dh^L = dz W_out (N, H), a thread per row
__global__ void __launch_bounds__(256) kan_out_rows_kernel(int64_t N, int H, int O, const float* U, const float* gU,
                                                           const float* Wout, float* dz, float* G) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < N; row += (int64_t)gridDim.x * blockDim.x) {
    float d[kKanMaxO];
#pragma unroll
    for (int q = 0; q < kKanMaxO; ++q) {
      d[q] = 0.0f;
      if (q < O) {
        const float u = U[row * O + q];
        d[q] = gU[row * O + q] * (u * (1.0f - u));
        dz[row * O + q] = d[q];
      }
    }
    for (int o = 0; o < H; ++o) {
      float s = 0.0f;
#pragma unroll
      for (int q = 0; q < kKanMaxO; ++q)
        if (q < O) s += d[q] * Wout[q * H + o];
      G[row * H + o] = s;
    }
  }
}

// A Linear's gradients: dW[a][b] = sum_r D[r][a] X[r][b], db[a] = sum_r D[r][a] for D (N, A), X (N, B); thread
// (a, b) owns dW[a][b] (and, for b = 0, db[a]) and adds its rows in ascending order (compensated).  Persistent over 32-row tiles.
__global__ void __launch_bounds__(1024) kan_linear_wgrad_kernel(int64_t N, int A, int B, const float* D, const float* X,
                                                                float* partial, int total, int woff, int boff) {
  __shared__ float Ds[kKanLinRows * kKanMaxH], Xs[kKanLinRows * kKanMaxH];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ta = tid / B, tb = tid - ta * B;
  const bool own = tid < A * B;
  float w = 0.0f, wc = 0.0f, bias = 0.0f, biasc = 0.0f;
  const int64_t ntiles = (N + kKanLinRows - 1) / kKanLinRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kKanLinRows;
    const int rc = (int)std::min<int64_t>(kKanLinRows, N - r0);
    for (int e = tid; e < rc * A; e += nt) Ds[e] = D[r0 * A + e];
    for (int e = tid; e < rc * B; e += nt) Xs[e] = X[r0 * B + e];
    __syncthreads();
    if (own) {
      for (int r = 0; r < rc; ++r) {
        const float d = Ds[r * A + ta];
        kan_add(w, wc, d * Xs[r * B + tb]);
        if (tb == 0) kan_add(bias, biasc, d);
      }
    }
    __syncthreads();
  }
  float* out = partial + (int64_t)blockIdx.x * total;
  if (own) {
    out[woff + tid] = w;
    if (tb == 0) out[boff + ta] = bias;
  }
}

struct KanBwdArgs {
  int64_t N;
  int32_t H, GK, NK, GKP, HP, R;
  const float* hin;   // (N, H): the layer's input h^l
  float* G;           // (N, H): dL/dy of the layer on entry, dL/dh^l on exit (in place, row by row)
  const float *coef, *sbase, *ssp, *grid, *mask, *nscale, *sscale;
  float* partial;
  int32_t total, off_coef, off_sbase, off_ssp;
};

template <int K>
__global__ void __launch_bounds__(1024) kan_layer_bwd_kernel(KanBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ksm[];
  const int H = a.H, GK = a.GK, NK = a.NK, GKP = a.GKP, HP = a.HP, R = a.R;
  const int tid = threadIdx.x, nt = blockDim.x;
  float* gt = ksm;                           // [i][o][j], stride GKP: the coef gradient
  int* IDX = reinterpret_cast<int*>(gt + H * H * GKP);  // [r][i] knot interval (-1 outside)
  float* SL = reinterpret_cast<float*>(IDX + R * H);    // [r][i] silu(h)
  float* DSL = SL + R * H;                   // [r][i] silu'(h)
  float* BV = DSL + R * H;                   // [r][i][K + 1] bases
  float* DBV = BV + R * H * (K + 1);         // [r][i][K + 1] their derivatives
  float* GS = DBV + R * H * (K + 1);         // [r][o] dL/dy node_scale subnode_scale
  float* T = GS + R * H;                     // [r][i][o], stride HP: dL/dh_i's term of output o
  for (int e = tid; e < H * H * GKP; e += nt) gt[e] = 0.0f;
  const bool own = tid < H * H;
  const int ti = own ? tid / H : 0, to = own ? tid - ti * H : 0;
  const float m = own ? a.mask[tid] : 0.0f, sb = own ? a.sbase[tid] : 0.0f, sp = own ? a.ssp[tid] : 0.0f;
  const float* crow = a.coef + (int64_t)(ti * H + to) * GK;
  float* grow = gt + (ti * H + to) * GKP;
  float dsb = 0.0f, dsbc = 0.0f, dsp = 0.0f, dspc = 0.0f;
  const int64_t nchunks = (a.N + R - 1) / R;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t r0 = chunk * R;
    const int rc = (int)std::min<int64_t>(R, a.N - r0);
    // phase 1: the chunk's image, item (r, i)
    for (int e = tid; e < rc * H; e += nt) {
      const int i = e % H;
      const float h = a.hin[r0 * H + e];
      const float s = ksigm(h);
      SL[e] = h * s;
      DSL[e] = s * (1.0f + h * (1.0f - s));
      GS[e] = a.G[r0 * H + e] * a.nscale[i] * a.sscale[i];  // (here i is the output index of G's column)
      const float* kt = a.grid + i * NK;
      const int mm = kan_interval(kt, NK, h);
      IDX[e] = mm;
      if (mm >= 0) {
        float b[K + 1], db[K + 1];
        kan_bases<K, true>(kt, NK, mm, h, b, db);
#pragma unroll
        for (int jj = 0; jj <= K; ++jj) {
          BV[e * (K + 1) + jj] = b[jj];
          DBV[e * (K + 1) + jj] = db[jj];
        }
      }
    }
    __syncthreads();
    // phase 2: thread (i, o) walks the rows in order
    if (own) {
      // kKanAhead rows at a time: their coefficients first (global memory, L2-resident), every load issued before
      // the first LDS store below, so they pay that latency once
      for (int rb = 0; rb < rc; rb += kKanAhead) {
        int mi[kKanAhead];
        float cc[kKanAhead][K + 1];
#pragma unroll
        for (int q = 0; q < kKanAhead; ++q) mi[q] = rb + q < rc ? IDX[(rb + q) * H + ti] : -1;
#pragma unroll
        for (int q = 0; q < kKanAhead; ++q)
#pragma unroll
          for (int jj = 0; jj <= K; ++jj) {
            const int j = mi[q] - K + jj;
            cc[q][jj] = (mi[q] >= 0 && j >= 0 && j < GK) ? crow[j] : 0.0f;
          }
#pragma unroll
        for (int q = 0; q < kKanAhead; ++q) {
          const int r = rb + q;
        if (r >= rc) continue;
        const int e = r * H + ti;
        const float g = m * GS[r * H + to];
        const int mm = mi[q];
        float t = sb * DSL[e];
        kan_add(dsb, dsbc, g * SL[e]);
        if (mm >= 0) {
          float S = 0.0f, dS = 0.0f;
          const float gs = g * sp;
#pragma unroll
          for (int jj = 0; jj <= K; ++jj) {
            const int j = mm - K + jj;
            if (j >= 0 && j < GK) {
              const float c = cc[q][jj], b = BV[e * (K + 1) + jj];
              S += c * b;
              dS += c * DBV[e * (K + 1) + jj];
              grow[j] += gs * b;
            }
          }
          kan_add(dsp, dspc, g * S);
          t += sp * dS;
        }
        T[e * HP + to] = g * t;
        }
      }
    }
    __syncthreads();
    // phase 3: dL/dh[r][i] = sum over o (ascending), item (r, i); the next chunk's phase 1 writes other arrays
    for (int e = tid; e < rc * H; e += nt) {
      float v = 0.0f;
      for (int o = 0; o < H; ++o) v += T[e * HP + o];
      a.G[r0 * H + e] = v;
    }
  }
  __syncthreads();
  float* out = a.partial + (int64_t)blockIdx.x * a.total;
  for (int e = tid; e < H * H * GK; e += nt) out[a.off_coef + e] = gt[(e / GK) * GKP + e % GK];
  if (own) {
    out[a.off_sbase + tid] = dsb;
    out[a.off_ssp + tid] = dsp;
  }
}

// grad[p] = sum over workgroups (ascending) of partial[wg][p]: a fixed order, so the result is deterministic
__global__ void kan_reduce_kernel(const float* partial, int nwg, int total, float* grad) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  float v = 0.0f;
  int g = 0;
  for (; g + 8 <= nwg; g += 8) {  // eight loads in flight, summed in ascending order
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = partial[(int64_t)(g + j) * total + p];
#pragma unroll
    for (int j = 0; j < 8; ++j) v += t[j];
  }
  for (; g < nwg; ++g) v += partial[(int64_t)g * total + p];
  grad[p] = v;
}

int kan_device_cus() {
  constexpr int kDevs = 64;
  static std::atomic<int> cache[kDevs] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevs) return 256;
  int cus = cache[dev].load(std::memory_order_relaxed);
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cache[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// the forward's LDS image: the odd [o] stride and the knots' LDS copy are kept when they fit
struct KanFwdLds {
  int HP, knots_lds, floats;
};
KanFwdLds kan_fwd_lds(const KanLayout& L) {
  KanFwdLds s{L.H | 1, 1, 0};
  auto need = [&] { return L.H * L.gk() * s.HP + L.H * s.HP + (s.knots_lds ? L.H * L.nk() : 0); };
  if (need() > kKanLdsFloats) s.knots_lds = 0;
  if (need() > kKanLdsFloats) s.HP = L.H;
  s.floats = need();
  return s;
}

// the layer backward's LDS image: odd row stride of the gradient table when it fits, then as many rows per chunk
// (up to 16) as fit beside it
struct KanBwdLds {
  int GKP, HP, R, floats;
};
KanBwdLds kan_bwd_lds(const KanLayout& L) {
  KanBwdLds s{L.gk() | 1, L.H | 1, 1, 0};
  auto per_row = [&] { return L.H * (4 + 2 * (L.K + 1) + s.HP); };
  if (L.H * L.H * s.GKP + per_row() > kKanLdsFloats) s.GKP = L.gk();
  if (L.H * L.H * s.GKP + per_row() > kKanLdsFloats) s.HP = L.H;
  s.R = std::max(1, std::min(kKanMaxChunk, (kKanLdsFloats - L.H * L.H * s.GKP) / per_row()));
  s.floats = L.H * L.H * s.GKP + s.R * per_row();
  return s;
}

template <int HT, int K>
hipError_t kan_launch_fwd(const KanFwdArgs& a, int grid, size_t lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute((const void*)kan_layer_fwd_kernel<HT, K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((kan_layer_fwd_kernel<HT, K>), dim3(grid), dim3(kKanFwdThreads), lds, stream, a);
  return hipGetLastError();
}
template <int K>
hipError_t kan_launch_fwd_h(const KanFwdArgs& a, int grid, size_t lds, hipStream_t stream) {
  if (a.H <= 8) return kan_launch_fwd<8, K>(a, grid, lds, stream);
  if (a.H <= 16) return kan_launch_fwd<16, K>(a, grid, lds, stream);
  if (a.H <= 24) return kan_launch_fwd<24, K>(a, grid, lds, stream);
  return kan_launch_fwd<32, K>(a, grid, lds, stream);
}
template <int K>
hipError_t kan_launch_bwd(const KanBwdArgs& a, int grid, int threads, size_t lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute((const void*)kan_layer_bwd_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((kan_layer_bwd_kernel<K>), dim3(grid), dim3(threads), lds, stream, a);
  return hipGetLastError();
}

int kan_groups(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>((N + 63) / 64, kan_device_cus())); }

}  // namespace

// work: forward -- two (N, H) activation buffers when nothing is saved; backward -- the per-workgroup
// partials, dL/dh (N, H) and dz (N, O)
int64_t kan_work_bytes(const ddr_kan_desc& d, int64_t N, bool backward) {
  const KanLayout L(d);
  if (!backward) return 2 * N * L.H * (int64_t)sizeof(float);
  return ((int64_t)kan_groups(N) * L.total() + N * L.H + N * L.O) * (int64_t)sizeof(float);
}

hipError_t launch_kan_forward(const ddr_kan_desc& d, int64_t N, const float* X, const float* P, const float* C,
                              float* h_save, float* U, void* work, hipStream_t stream) {
  const KanLayout L(d);
  const KanFwdLds lds = kan_fwd_lds(L);
  const int64_t NH = N * L.H;
  KanFwdArgs a{};
  a.N = N;
  a.ntiles = (int)((N + kKanFwdThreads - 1) / kKanFwdThreads);
  a.F = L.F, a.H = L.H, a.O = L.O, a.GK = L.gk(), a.NK = L.nk(), a.HP = lds.HP;
  a.knots_lds = lds.knots_lds;
  a.X = X;
  a.U = U;
  a.Win = P + L.w_in(), a.bin = P + L.b_in(), a.Wout = P + L.w_out(), a.bout = P + L.b_out();
  const int grid = (int)std::min<int64_t>(a.ntiles, kan_device_cus());
  float* ping = static_cast<float*>(work);
  for (int l = 0; l < L.L; ++l) {
    a.first = l == 0, a.last = l == L.L - 1;
    if (h_save) {
      a.hin = h_save + (int64_t)l * NH;
      a.h0 = a.first ? h_save : nullptr;
      a.hout = h_save + (int64_t)(l + 1) * NH;
    } else {
      a.hin = ping + (int64_t)((l + 1) & 1) * NH;  // what layer l - 1 wrote
      a.h0 = nullptr;
      a.hout = a.last ? nullptr : ping + (int64_t)(l & 1) * NH;
    }
    a.coef = P + L.coef(l), a.sbase = P + L.scale_base(l), a.ssp = P + L.scale_sp(l);
    a.grid = C + L.c_grid(l), a.mask = C + L.c_mask(l), a.nscale = C + L.c_node_scale(l);
    a.nbias = C + L.c_node_bias(l), a.sscale = C + L.c_sub_scale(l), a.sbias = C + L.c_sub_bias(l);
    const size_t bytes = sizeof(float) * (size_t)lds.floats;
    hipError_t e = L.K == 1   ? kan_launch_fwd_h<1>(a, grid, bytes, stream)
                   : L.K == 2 ? kan_launch_fwd_h<2>(a, grid, bytes, stream)
                              : kan_launch_fwd_h<3>(a, grid, bytes, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_kan_backward(const ddr_kan_desc& d, int64_t N, const float* X, const float* P, const float* C,
                               const float* h_save, const float* U, const float* gU, float* grad, void* work,
                               hipStream_t stream) {
  const KanLayout L(d);
  const KanBwdLds lds = kan_bwd_lds(L);
  const int64_t NH = N * L.H;
  const int nwg = kan_groups(N), total = L.total();
  float* partial = static_cast<float*>(work);
  float* G = partial + (int64_t)nwg * total;
  float* dz = G + NH;
  const int rows_grid = (int)std::min<int64_t>((N + 255) / 256, 8 * (int64_t)kan_device_cus());
  hipLaunchKernelGGL(kan_out_rows_kernel, dim3(rows_grid), dim3(256), 0, stream, N, L.H, L.O, U, gU, P + L.w_out(), dz, G);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  auto threads_for = [](int n) { return (n + 63) / 64 * 64; };
  hipLaunchKernelGGL(kan_linear_wgrad_kernel, dim3(nwg), dim3(threads_for(L.O * L.H)), 0, stream, N, L.O, L.H,
                     (const float*)dz, h_save + (int64_t)L.L * NH, partial, total, L.w_out(), L.b_out());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  KanBwdArgs a{};
  a.N = N;
  a.H = L.H, a.GK = L.gk(), a.NK = L.nk(), a.GKP = lds.GKP, a.HP = lds.HP, a.R = lds.R;
  a.G = G;
  a.partial = partial;
  a.total = total;
  for (int l = L.L - 1; l >= 0; --l) {
    a.hin = h_save + (int64_t)l * NH;
    a.coef = P + L.coef(l), a.sbase = P + L.scale_base(l), a.ssp = P + L.scale_sp(l);
    a.grid = C + L.c_grid(l), a.mask = C + L.c_mask(l), a.nscale = C + L.c_node_scale(l), a.sscale = C + L.c_sub_scale(l);
    a.off_coef = L.coef(l), a.off_sbase = L.scale_base(l), a.off_ssp = L.scale_sp(l);
    const size_t bytes = sizeof(float) * (size_t)lds.floats;
    const int threads = threads_for(L.H * L.H);
    e = L.K == 1   ? kan_launch_bwd<1>(a, nwg, threads, bytes, stream)
        : L.K == 2 ? kan_launch_bwd<2>(a, nwg, threads, bytes, stream)
                   : kan_launch_bwd<3>(a, nwg, threads, bytes, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kan_linear_wgrad_kernel, dim3(nwg), dim3(threads_for(L.H * L.F)), 0, stream, N, L.H, L.F,
                     (const float*)G, X, partial, total, L.w_in(), L.b_in());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(kan_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, (const float*)partial, nwg, total, grad);
  return hipGetLastError();
}

}  // namespace ddr
