// The unrouted baseline of the reference's evaluation (scripts/summed_q_prime.py:208-261, eval_q_prime): for every
// gauge the sum of the lateral inflow Q' of the divides upstream of it, per day,
//   daily[i, d] = (sum_{h < rho} qr[i, d rho + h]) / rho          rho = 24 (hourly store) or 1 (daily store)
//   pred[g, d]  = sum over the members i of g with daily[i, d] not NaN of daily[i, d]        (nansum)
// from the device-resident (n_rows, T) fp32 store into the (G, D) fp32 series that ddr_metrics_f32 reads.
//
// A segmented, NaN-skipping row gather.  The plan cuts every member list into *pieces* of at most `chunk` members,
// at multiples of `chunk` counted from the list's start, and sorts the pieces largest first.  One wave owns a
// (piece, day tile) task and walks the piece's members in list order, kMembers rows in flight:
//   rho = 1   a lane owns 4 consecutive days (one 16-byte load per member: the wave reads 1 KiB of the row), a tile
//             is 256 days
//   rho = 24  a lane owns one day = 96 contiguous bytes (six 16-byte loads: the wave reads 6 KiB), a tile is 64 days
// The 16-byte loads need a 16-byte aligned base and a row stride that is a multiple of 4 elements; any other view,
// and a lane whose days run past D, takes 4-byte loads of the same elements.  A row is addressed by a 64-bit base
// (index * row_stride) plus a 32-bit offset inside the row.
//
// Every lane adds its own days in fp64 -- the hours of a day in hour order, one IEEE division by rho, the members
// in list order, NaN days skipped -- so no value crosses lanes.  A one-piece list is rounded to fp32 and stored;
// the pieces of a longer list store fp64 partial rows, which a second launch adds in piece order and rounds.
// No atomics: a gauge's row depends on its own list, the chunk and the store alone, not on the grid, the other
// gauges of the call or the order the tasks run in.
#include "summedq.h"

#include <algorithm>
#include <numeric>
#include <vector>

#include "internal.h"

namespace ddr {

namespace {

constexpr int kWaves = 4;  // tasks (waves) per workgroup

struct SqArgs {
  const float* qr;
  int64_t row_stride;
  const int32_t* idx;
  const SummedQPiece* pieces;
  int64_t n_tasks;
  int32_t n_tiles, D;
  float* out;
  int64_t out_stride;
  double* part;  // (n_slots, D)
};

// the NF = DPL * RHO floats of one member that this lane owns (DPL days of RHO hours), `valid` of the days real
template <int RHO, int DPL, bool VEC>
__device__ __forceinline__ void load_member(const float* p, int valid, float (&f)[DPL * RHO]) {
  constexpr int NF = DPL * RHO;
  if (VEC && valid == DPL) {
#pragma unroll
    for (int k = 0; k < NF / 4; ++k) {
      const float4 v = reinterpret_cast<const float4*>(p)[k];
      f[4 * k] = v.x;
      f[4 * k + 1] = v.y;
      f[4 * k + 2] = v.z;
      f[4 * k + 3] = v.w;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < DPL; ++j) {
#pragma unroll
    for (int h = 0; h < RHO; ++h) f[j * RHO + h] = j < valid ? p[j * RHO + h] : 0.0f;
  }
}

template <int RHO, int DPL>
__device__ __forceinline__ void add_member(const float (&f)[DPL * RHO], double (&acc)[DPL]) {
#pragma unroll
  for (int j = 0; j < DPL; ++j) {
    double s = (double)f[j * RHO];
#pragma unroll
    for (int h = 1; h < RHO; ++h) s += (double)f[j * RHO + h];
    if constexpr (RHO > 1) s = s / (double)RHO;
    acc[j] += s == s ? s : 0.0;
  }
}

template <int RHO, bool VEC>
__global__ void __launch_bounds__(64 * kWaves) summedq_kernel(SqArgs a) {
  constexpr int DPL = RHO == 1 ? 4 : 1;         // days per lane
  constexpr int kMembers = RHO == 1 ? 8 : 4;    // member rows in flight per wave
  // (readfirstlane: the task, its piece and the member indices are wave-uniform, so they load as scalars)
  const int64_t task = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (task >= a.n_tasks) return;  // (the whole wave; no barrier in this kernel)
  const int lane = threadIdx.x & 63;
  const int64_t pi = task / a.n_tiles;
  const int tile = (int)(task - pi * a.n_tiles);
  const SummedQPiece pc = a.pieces[pi];
  const int d0 = (tile * 64 + lane) * DPL;  // this lane's first day
  const int valid = min(max(a.D - d0, 0), DPL);
  const int off = d0 * RHO;  // (< T whenever valid > 0, and below T + 64 * 24 always)
  const int32_t* ix = a.idx + pc.begin;

  double acc[DPL];
#pragma unroll
  for (int j = 0; j < DPL; ++j) acc[j] = 0.0;
  int m = 0;
  for (; m + kMembers <= pc.count; m += kMembers) {
    float f[kMembers][DPL * RHO];
#pragma unroll
    for (int u = 0; u < kMembers; ++u)
      load_member<RHO, DPL, VEC>(a.qr + (int64_t)ix[m + u] * a.row_stride + off, valid, f[u]);
#pragma unroll
    for (int u = 0; u < kMembers; ++u) add_member<RHO, DPL>(f[u], acc);
  }
  for (; m < pc.count; ++m) {
    float f[DPL * RHO];
    load_member<RHO, DPL, VEC>(a.qr + (int64_t)ix[m] * a.row_stride + off, valid, f);
    add_member<RHO, DPL>(f, acc);
  }

  if (pc.slot < 0) {
    float* o = a.out + (int64_t)pc.gauge * a.out_stride + d0;
#pragma unroll
    for (int j = 0; j < DPL; ++j)
      if (j < valid) o[j] = (float)acc[j];
  } else {
    double* o = a.part + pc.slot * a.D + d0;
#pragma unroll
    for (int j = 0; j < DPL; ++j)
      if (j < valid) o[j] = acc[j];
  }
}

// a split gauge's partial rows added in piece order, rounded once
__global__ void __launch_bounds__(256) summedq_combine_kernel(const SummedQSplit* splits, int64_t n_splits, int32_t D,
                                                              const double* part, float* out, int64_t out_stride) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_splits * D) return;
  const int64_t s = t / D;
  const int d = (int)(t - s * D);
  const SummedQSplit sp = splits[s];
  const double* p = part + sp.first_slot * D + d;
  double acc = p[0];
  for (int k = 1; k < sp.n_pieces; ++k) acc += p[(int64_t)k * D];
  out[(int64_t)sp.gauge * out_stride + d] = (float)acc;
}

template <typename T>
hipError_t upload(const std::vector<T>& v, T** dst, hipStream_t stream) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(v.size() * sizeof(T), 16));
  if (e != hipSuccess || v.empty()) return e;
  return hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream);
}

}  // namespace

ddr_status summedq_plan_create(int64_t G, const int64_t* member_off, const int32_t* member_idx, int64_t chunk,
                               hipStream_t stream, SummedQPlan** plan) {
  if (!plan) return fail(DDR_ERR_ARG, "summedq_plan_create: null plan pointer");
  *plan = nullptr;
  if (G < 0) return fail(DDR_ERR_ARG, "summedq_plan_create: negative size");
  if (G > INT32_MAX) return fail(DDR_ERR_ARG, "summedq_plan_create: too many gauges");
  if (chunk < 1 || chunk > (int64_t(1) << 30))
    return fail(DDR_ERR_ARG, "summedq_plan_create: chunk must be in [1, 2^30] (got " + std::to_string(chunk) + ")");
  if (!member_off) return fail(DDR_ERR_ARG, "summedq_plan_create: null member_off");
  if (member_off[0] != 0) return fail(DDR_ERR_ARG, "summedq_plan_create: member_off is not monotone from 0");
  for (int64_t g = 0; g < G; ++g)
    if (member_off[g + 1] < member_off[g])
      return fail(DDR_ERR_ARG, "summedq_plan_create: member_off is not monotone from 0 (at gauge " +
                                   std::to_string(g) + ")");
  const int64_t nnz = member_off[G];
  if (nnz > 0 && !member_idx) return fail(DDR_ERR_ARG, "summedq_plan_create: null member_idx");
  int32_t max_index = -1;
  for (int64_t k = 0; k < nnz; ++k) {
    if (member_idx[k] < 0)
      return fail(DDR_ERR_ARG, "summedq_plan_create: negative index at position " + std::to_string(k));
    max_index = std::max(max_index, member_idx[k]);
  }

  std::vector<SummedQPiece> pieces;
  std::vector<SummedQSplit> splits;
  int64_t n_slots = 0;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t b = member_off[g], M = member_off[g + 1] - b;
    if (M <= chunk) {  // (an empty list too: its piece stores the zeros)
      pieces.push_back({b, -1, (int32_t)M, (int32_t)g});
      continue;
    }
    const int64_t np = (M + chunk - 1) / chunk;
    if (np > INT32_MAX) return fail(DDR_ERR_ARG, "summedq_plan_create: too many pieces in one list");
    splits.push_back({n_slots, (int32_t)g, (int32_t)np});
    for (int64_t p = 0; p < np; ++p)
      pieces.push_back({b + p * chunk, n_slots + p, (int32_t)std::min(chunk, M - p * chunk), (int32_t)g});
    n_slots += np;
  }
  std::stable_sort(pieces.begin(), pieces.end(),
                   [](const SummedQPiece& x, const SummedQPiece& y) { return x.count > y.count; });

  auto* P = new SummedQPlan;
  P->G = G;
  P->nnz = nnz;
  P->chunk = chunk;
  P->n_pieces = (int64_t)pieces.size();
  P->n_splits = (int64_t)splits.size();
  P->n_slots = n_slots;
  P->max_index = max_index;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
    (void)hipGetLastError();
    *plan = P;  // no device: the plan still checks arguments
    return DDR_OK;
  }
  hipError_t e = hipGetDevice(&P->device);
  if (e == hipSuccess) e = upload(std::vector<int32_t>(member_idx, member_idx + nnz), &P->d_idx, stream);
  if (e == hipSuccess) e = upload(pieces, &P->d_pieces, stream);
  if (e == hipSuccess) e = upload(splits, &P->d_splits, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);  // (the uploads read this call's host arrays)
  if (e != hipSuccess) {
    summedq_plan_destroy(P);
    return hip_fail(e, "summedq_plan_create: upload");
  }
  *plan = P;
  return DDR_OK;
}

void summedq_plan_destroy(SummedQPlan* plan) {
  if (!plan) return;
  if (plan->d_idx) (void)hipFree(plan->d_idx);
  if (plan->d_pieces) (void)hipFree(plan->d_pieces);
  if (plan->d_splits) (void)hipFree(plan->d_splits);
  delete plan;
}

int64_t summedq_scratch_bytes(const SummedQPlan* plan, int64_t D) {
  if (!plan || D < 0) return -1;
  return plan->n_slots * D * (int64_t)sizeof(double);
}

ddr_status summedq_run(const SummedQPlan* plan, const float* qr, int64_t n_rows, int64_t row_stride, int64_t T,
                       int32_t rho, float* out, int64_t out_stride, void* scratch, int64_t scratch_bytes,
                       hipStream_t stream) {
  if (!plan) return fail(DDR_ERR_ARG, "summedq: null plan");
  if (n_rows < 0 || row_stride < 0 || T < 0 || out_stride < 0 || scratch_bytes < 0)
    return fail(DDR_ERR_ARG, "summedq: negative size");
  if (rho != 1 && rho != 24)
    return fail(DDR_ERR_ARG, "summedq: hours per step must be 1 or 24 (got " + std::to_string(rho) + ")");
  if (T < rho) return fail(DDR_ERR_ARG, "summedq: T is shorter than one step (T < rho)");
  if (T > INT32_MAX - 4096) return fail(DDR_ERR_ARG, "summedq: T exceeds the 32-bit in-row offset");
  const int64_t D = T / rho;
  if (row_stride < T) return fail(DDR_ERR_ARG, "summedq: row_stride is shorter than a row");
  if (out_stride < D) return fail(DDR_ERR_ARG, "summedq: out_stride is shorter than a row of days");
  if (n_rows <= plan->max_index)
    return fail(DDR_ERR_ARG, "summedq: n_rows (" + std::to_string(n_rows) + ") does not cover the plan's largest "
                                 "index (" + std::to_string(plan->max_index) + ")");
  const int64_t need = summedq_scratch_bytes(plan, D);
  if (scratch_bytes < need)
    return fail(DDR_ERR_ARG, "summedq: scratch_bytes " + std::to_string(scratch_bytes) + " is below the " +
                                 std::to_string(need) + " of ddr_summedq_scratch_bytes");
  if (plan->G == 0) return DDR_OK;
  if (!out || (plan->nnz > 0 && !qr) || (need > 0 && !scratch)) return fail(DDR_ERR_ARG, "summedq: null argument");
  const int64_t n_tiles = rho == 1 ? (D + 255) / 256 : (D + 63) / 64;
  const int64_t n_tasks = plan->n_pieces * n_tiles;
  const int64_t n_wg = (n_tasks + kWaves - 1) / kWaves;
  const int64_t n_cwg = (plan->n_splits * D + 255) / 256;
  if (n_wg > INT32_MAX || n_cwg > INT32_MAX) return fail(DDR_ERR_ARG, "summedq: too many tasks for one launch");
  if (plan->device < 0) return fail(DDR_ERR_HIP, "summedq: the plan was created without a HIP device");
  int cur = -1;
  DDR_HIP(hipGetDevice(&cur));
  if (cur != plan->device)
    return fail(DDR_ERR_ARG, "summedq: the plan lives on device " + std::to_string(plan->device) +
                                 ", the current device is " + std::to_string(cur));

  SqArgs a{qr, row_stride, plan->d_idx, plan->d_pieces, n_tasks, (int32_t)n_tiles, (int32_t)D, out, out_stride,
           static_cast<double*>(scratch)};
  const bool vec = (reinterpret_cast<uintptr_t>(qr) & 15) == 0 && (row_stride & 3) == 0;
  const dim3 grid((unsigned)n_wg), block(64 * kWaves);
  if (rho == 1) {
    if (vec) hipLaunchKernelGGL((summedq_kernel<1, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((summedq_kernel<1, false>), grid, block, 0, stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((summedq_kernel<24, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((summedq_kernel<24, false>), grid, block, 0, stream, a);
  }
  DDR_HIP(hipGetLastError());
  if (plan->n_splits > 0) {
    hipLaunchKernelGGL(summedq_combine_kernel, dim3((unsigned)n_cwg), dim3(256), 0, stream, plan->d_splits,
                       plan->n_splits, (int32_t)D, static_cast<const double*>(scratch), out, out_stride);
    DDR_HIP(hipGetLastError());
  }
  return DDR_OK;
}

}  // namespace ddr
