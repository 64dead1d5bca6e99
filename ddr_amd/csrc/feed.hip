// The per-batch forcing feed: what the reference's StreamflowReader.forward (src/ddr/io/readers.py:461-531) and the
// observation selection of its training loop (io/builders.py:112-129, scripts/train.py:84-92) do on the host per
// batch, as two gathers from stores that were uploaded once.
//
// feed_qprime_kernel -- a tiled gather-transpose.  The store holds time on the inner axis, (n_rows, T_store); the
// router reads (T, N) with reaches on the inner axis.  A workgroup owns a tile of kTR = 64 batch reaches x kTC = 64
// store columns: it reads each reach's piece of the window along time (contiguous in the store), stages it in LDS,
// and writes it along reaches (contiguous in the output), each staged column to its `repeat` output rows (24 for a
// daily store expanded to hours, readers.py:513-519; the last one cut at T_out).
//   VEC    the tile starts at the window's first column rounded down to a multiple of 4, so every row piece is
//          read with 16-byte loads whatever t0 is; the columns in front of the window are staged and not emitted.
//          It needs a 16-byte aligned store and a row stride that is a multiple of 4 elements.  Eight lanes read
//          128 contiguous bytes of a row, a half-wave four rows: with the tile's leading dimension kTC + 1 its 32
//          ds_write_b32 of one component land on 32 banks, and so do the transposed reads (lane = reach).
//   dword  any other view: the tile starts at t0, a wave reads 64 consecutive columns of one row.
// The output's rows are N floats long, so a tile's 256-byte pieces of them share their first and last 128-byte line
// with the neighbouring tiles; the tiles are numbered so that neighbours run on one XCD, where the shared lines are
// completed in its L2 (at N = 939 409 the hourly (2136, N) tensor takes 2.6-3.0 ms, 3.8 ms with tiles in launch order).
// A row index outside [0, n_rows) is a divide the store lacks: its reach gets `fill` (readers.py:523-530) and
// valid = 0, and nothing is read for it.  Values move as 32-bit words: NaN payloads and -0.0 arrive unchanged.
// Addresses are 64-bit (row * row_stride passes 2^32 elements on a real store).  Plain vector stores only.
//
// feed_rows_kernel -- one workgroup per gauge copies the gauge's window without its first and last `trim` days
// (train.py:92) and reduces "any NaN in the whole window" (train.py:84-87); one lane stores the flag.
#include "feed.h"

#include <algorithm>
#include <string>

#include "internal.h"

namespace ddr {

namespace {

constexpr int kTR = 64;       // batch reaches per tile
constexpr int kTC = 64;       // store columns per tile
constexpr int kLD = kTC + 1;  // leading dimension of the staged tile (bank-conflict padding)
constexpr int kXcds = 8;      // accelerator dies, each with its own L2
constexpr uint32_t kQuietNaN = 0x7fc00000u;

struct FeedArgs {
  const uint32_t* store;
  int64_t row_stride;
  const int32_t* rows;
  int64_t N;
  int64_t n_tiles, tiles_per_xcd;  // reach tiles, and ceil(n_tiles / kXcds)
  int32_t n_rows, T_store;
  int32_t t0, tend;  // the window [t0, tend) in store columns
  int32_t abase;     // first column of tile 0
  int32_t repeat;
  int64_t T_out;
  uint32_t fill;
  uint32_t* out;
  uint8_t* valid;
};

// REP: the output rows per staged column when known at compile time (1, 24), 0 = a.repeat
template <bool VEC, int REP>
__global__ void __launch_bounds__(256) feed_qprime_kernel(FeedArgs a) {
  __shared__ uint32_t tile[kTR * kLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // (blockIdx.x -> reach tile: workgroups b and b + 8 have been observed to share an XCD, so each XCD gets a run of
  // neighbouring tiles, and the output lines that two tiles share at their edge meet in one L2)
  const int64_t tile_n = (int64_t)(blockIdx.x & (kXcds - 1)) * a.tiles_per_xcd + (blockIdx.x / kXcds);
  if (tile_n >= a.n_tiles) return;  // (the whole workgroup, before the barrier)
  const int64_t n0 = tile_n * kTR;
  const int a0 = a.abase + (int)blockIdx.y * kTC;

  if (blockIdx.y == 0 && tid < kTR && n0 + tid < a.N)
    a.valid[n0 + tid] = (uint32_t)a.rows[n0 + tid] < (uint32_t)a.n_rows;

  if constexpr (VEC) {
    const int f4 = (lane & 7) + 8 * (lane >> 5);
    const int col = a0 + 4 * f4;
    const bool wanted = col < a.tend && col + 4 > a.t0;
    uint4 v[4];
    bool have[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = k * 16 + w * 4 + ((lane >> 3) & 3);
      const int64_t n = n0 + row;
      have[k] = wanted && n < a.N;
      v[k] = make_uint4(a.fill, a.fill, a.fill, a.fill);
      if (!have[k]) continue;
      const int32_t r = a.rows[n];
      if ((uint32_t)r >= (uint32_t)a.n_rows) continue;
      const uint32_t* p = a.store + (int64_t)r * a.row_stride + col;
      if (col + 4 <= a.T_store) {
        v[k] = *reinterpret_cast<const uint4*>(p);
      } else {  // the row's last, partial quad (tend <= T_store: the columns past it are not emitted)
        v[k].x = p[0];
        if (col + 1 < a.T_store) v[k].y = p[1];
        if (col + 2 < a.T_store) v[k].z = p[2];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!have[k]) continue;
      uint32_t* t = tile + (k * 16 + w * 4 + ((lane >> 3) & 3)) * kLD + 4 * f4;
      t[0] = v[k].x;
      t[1] = v[k].y;
      t[2] = v[k].z;
      t[3] = v[k].w;
    }
  } else {
    const int col = a0 + lane;
    const bool wanted = col < a.tend;
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t n = n0 + w + 4 * k;
      v[k] = a.fill;
      if (!wanted || n >= a.N) continue;
      const int32_t r = a.rows[n];
      if ((uint32_t)r < (uint32_t)a.n_rows) v[k] = a.store[(int64_t)r * a.row_stride + col];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) tile[(w + 4 * k) * kLD + lane] = v[k];
  }
  __syncthreads();

  const int64_t n = n0 + lane;
  if (n >= a.N) return;
  const int rep = REP ? REP : a.repeat;
#pragma unroll 4
  for (int k = 0; k < kTC / 4; ++k) {
    const int c = w + 4 * k;
    const int col = a0 + c;
    if (col < a.t0 || col >= a.tend) continue;  // (wave-uniform)
    const uint32_t x = tile[lane * kLD + c];
    const int64_t first = (int64_t)(col - a.t0) * rep;
    uint32_t* o = a.out + first * a.N + n;
    if (REP && first + REP <= a.T_out) {
#pragma unroll
      for (int h = 0; h < REP; ++h) o[(int64_t)h * a.N] = x;
    } else {
      const int64_t left = a.T_out - first;
      const int64_t cnt = left < rep ? left : rep;
      for (int64_t h = 0; h < cnt; ++h) o[h * a.N] = x;
    }
  }
}

__global__ void __launch_bounds__(256) feed_rows_kernel(const uint32_t* store, int64_t row_stride, int32_t n_rows,
                                                        const int32_t* rows, int32_t t0, int32_t n_cols, int32_t trim,
                                                        uint32_t* out, int64_t out_stride, uint8_t* has_nan) {
  const int64_t g = blockIdx.x;
  const int32_t r = rows[g];
  const bool known = (uint32_t)r < (uint32_t)n_rows;
  const uint32_t* src = store + (known ? (int64_t)r * row_stride + t0 : 0);
  uint32_t* dst = out + g * out_stride;
  int nan = !known;  // an unknown gauge is an all-NaN row
  for (int c = threadIdx.x; c < n_cols; c += 256) {
    const uint32_t x = known ? src[c] : kQuietNaN;
    nan |= (x & 0x7fffffffu) > 0x7f800000u;
    if (c >= trim && c < n_cols - trim) dst[c - trim] = x;
  }
  const int any = __syncthreads_or(nan);
  if (threadIdx.x == 0) has_nan[g] = any != 0;
}

ddr_status check_store(const char* who, int64_t row_stride, int64_t n_rows, int64_t T_store, int64_t n, int64_t t0,
                       int64_t n_cols) {
  const std::string w(who);
  if (row_stride < 0 || n_rows < 0 || T_store < 0 || n < 0 || n_cols < 0)
    return fail(DDR_ERR_ARG, w + ": negative size");
  if (n_rows > INT32_MAX) return fail(DDR_ERR_ARG, w + ": n_rows exceeds the 32-bit row index");
  if (T_store > INT32_MAX - 4096) return fail(DDR_ERR_ARG, w + ": T_store exceeds the 32-bit in-row offset");
  if (row_stride < T_store) return fail(DDR_ERR_ARG, w + ": row_stride is shorter than a row");
  if (t0 < 0 || t0 > T_store || n_cols > T_store - t0)
    return fail(DDR_ERR_ARG, w + ": the window [" + std::to_string(t0) + ", " + std::to_string(t0) + " + " +
                                 std::to_string(n_cols) + ") leaves the store's [0, " + std::to_string(T_store) + ")");
  return DDR_OK;
}

}  // namespace

ddr_status feed_qprime(const float* store, int64_t row_stride, int64_t n_rows, int64_t T_store, const int32_t* rows,
                       int64_t N, int64_t t0, int64_t n_cols, int32_t repeat, int64_t T_out, float fill, float* out,
                       uint8_t* valid, hipStream_t stream) {
  if (ddr_status s = check_store("feed_qprime", row_stride, n_rows, T_store, N, t0, n_cols); s != DDR_OK) return s;
  if (repeat < 1)
    return fail(DDR_ERR_ARG, "feed_qprime: repeat must be at least 1 (got " + std::to_string(repeat) + ")");
  if (T_out < 0) return fail(DDR_ERR_ARG, "feed_qprime: negative size");
  if (n_cols != (T_out + repeat - 1) / repeat)
    return fail(DDR_ERR_ARG, "feed_qprime: T_out = " + std::to_string(T_out) + " with repeat = " +
                                 std::to_string(repeat) + " needs ceil(T_out / repeat) columns, not " +
                                 std::to_string(n_cols));
  if (N == 0) return DDR_OK;
  if (!rows || !valid || (T_out > 0 && !out) || (n_rows > 0 && n_cols > 0 && !store))
    return fail(DDR_ERR_ARG, "feed_qprime: null argument");
  const bool vec = (reinterpret_cast<uintptr_t>(store) & 15) == 0 && (row_stride & 3) == 0;
  const int64_t abase = vec ? (t0 & ~int64_t(3)) : t0;
  const int64_t n_tiles = (N + kTR - 1) / kTR, per_xcd = (n_tiles + kXcds - 1) / kXcds;
  const int64_t gx = per_xcd * kXcds;
  const int64_t gy = std::max<int64_t>(1, (t0 + n_cols - abase + kTC - 1) / kTC);
  if (gx > INT32_MAX || gy > 65535) return fail(DDR_ERR_ARG, "feed_qprime: too many tiles for one launch");

  uint32_t fill_bits;
  static_assert(sizeof fill_bits == sizeof fill, "fp32");
  __builtin_memcpy(&fill_bits, &fill, sizeof fill_bits);
  FeedArgs a{reinterpret_cast<const uint32_t*>(store), row_stride, rows, N, n_tiles, per_xcd, (int32_t)n_rows,
             (int32_t)T_store, (int32_t)t0, (int32_t)(t0 + n_cols), (int32_t)abase, repeat, T_out, fill_bits,
             reinterpret_cast<uint32_t*>(out), valid};
  const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
#define DDR_FEED_LAUNCH(V, R) hipLaunchKernelGGL((feed_qprime_kernel<V, R>), grid, block, 0, stream, a)
  if (vec) {
    if (repeat == 1) DDR_FEED_LAUNCH(true, 1);
    else if (repeat == 24) DDR_FEED_LAUNCH(true, 24);
    else DDR_FEED_LAUNCH(true, 0);
  } else {
    if (repeat == 1) DDR_FEED_LAUNCH(false, 1);
    else if (repeat == 24) DDR_FEED_LAUNCH(false, 24);
    else DDR_FEED_LAUNCH(false, 0);
  }
#undef DDR_FEED_LAUNCH
  DDR_HIP(hipGetLastError());
  return DDR_OK;
}

ddr_status feed_rows(const float* store, int64_t row_stride, int64_t n_rows, int64_t T_store, const int32_t* rows,
                     int64_t G, int64_t t0, int64_t n_cols, int32_t trim, float* out, int64_t out_stride,
                     uint8_t* has_nan, hipStream_t stream) {
  if (ddr_status s = check_store("feed_rows", row_stride, n_rows, T_store, G, t0, n_cols); s != DDR_OK) return s;
  if (trim < 0 || out_stride < 0) return fail(DDR_ERR_ARG, "feed_rows: negative size");
  if (n_cols < 2 * (int64_t)trim)
    return fail(DDR_ERR_ARG, "feed_rows: a window of " + std::to_string(n_cols) + " columns cannot lose " +
                                 std::to_string(trim) + " at each end");
  const int64_t kept = n_cols - 2 * (int64_t)trim;
  if (out_stride < kept) return fail(DDR_ERR_ARG, "feed_rows: out_stride is shorter than a row of the output");
  if (G > INT32_MAX) return fail(DDR_ERR_ARG, "feed_rows: too many rows for one launch");
  if (G == 0) return DDR_OK;
  if (!rows || !has_nan || (kept > 0 && !out) || (n_rows > 0 && n_cols > 0 && !store))
    return fail(DDR_ERR_ARG, "feed_rows: null argument");
  hipLaunchKernelGGL(feed_rows_kernel, dim3((unsigned)G), dim3(256), 0, stream,
                     reinterpret_cast<const uint32_t*>(store), row_stride, (int32_t)n_rows, rows, (int32_t)t0,
                     (int32_t)n_cols, trim, reinterpret_cast<uint32_t*>(out), out_stride, has_nan);
  DDR_HIP(hipGetLastError());
  return DDR_OK;
}

}  // namespace ddr
