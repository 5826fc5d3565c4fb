// phnn_mppi.hip -- the two kernels of the batched sampling (MPPI) solve (phnn_solve_mppi).  Per iteration and problem b:
// k_mppi_sample writes K perturbed copies of the nominal control sequence, v_k = clamp(u_b + sigma o z_k) (z_0 = 0),
// as the (B*K, H, m) control tensor K1 reads, K1 costs all B*K rollouts in one launch, and k_mppi_update moves the
// nominal to the softmin-weighted mean  u_b = clamp(sum_k w_k v_k / sum_k w_k),  w_k = exp(-(S_k - min S) / lambda).
// DESIGN.md section 12.
//
// Noise: Philox4x32-10, counter-based (phnn_mppi.h gives the counter layout): no generator state in memory, and the
// normals of (seed, epoch, iteration, global problem id, sample, float4) do not depend on the batch they are drawn in.
// One Philox call gives the four normals of one float4: two Box-Muller pairs, uniforms (x >> 8 + 0.5) * 2^-24.
//
// k_mppi_update has k_lbfgs's geometry: 16 lanes (one DPP row) per problem, lane l owns float4 l + 16e of the row.
// Reductions over the K samples (min, weight sum, argmin): lane l takes k = l, l + 16, ... in order, then a DPP
// butterfly inside the row; every step combines a pair of equal-order partials, so all 16 lanes end with the same bits
// and the result depends on K only, never on the problem's position or on B.  The weighted sum streams the K sample
// rows once, k ascending; row k + 1 is loaded before row k is accumulated.
#include "phnn_mppi.h"

#include <math.h>

#include "phnn_rows.hip.h"

namespace {

using namespace phnn_rows;  // Philox, Box-Muller, the DPP row reductions, rload / rstore

// ---------------------------------------------------------------------------------------------- k_mppi_sample
// One thread per float4 of the sample tensor: thread t -> rollout r = t / nv4 = b * K + k, float4 j = t % nv4.
template <bool ALIGNED>
__global__ __launch_bounds__(kBlock) void k_mppi_sample(MppiSampleParams p) {
  const int nv4 = (p.N + 3) / 4;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long r = t / nv4;
  if (r >= p.B * p.K) return;
  const int j = (int)(t - r * nv4);
  const long long b = r / p.K;
  const int k = (int)(r - b * p.K);
  const int e = 4 * j;

  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (k != 0) {  // sample 0 is the nominal itself
    const unsigned long long gid = (unsigned long long)(p.problem_offset + b);
    const int epoch = p.epoch_dev ? *p.epoch_dev : p.epoch_host;
    U4 c;
    c.x = (unsigned)gid;
    c.y = (unsigned)(gid >> 32) | ((unsigned)p.iteration << 16);
    c.z = (unsigned)epoch;
    c.w = ((unsigned)k << 6) | (unsigned)j;
    const U4 o = philox4x32_10(c, p.key0, p.key1);
    box_muller(o.x, o.y, z[0], z[1]);
    box_muller(o.z, o.w, z[2], z[3]);
  }
  const float* urow = p.u + (size_t)b * p.N;
  float* vrow = p.v + (size_t)r * p.N;
  if (ALIGNED) {  // N % 4 == 0 and 16-byte aligned bases: one 16-byte load and store
    const float4 u4 = reinterpret_cast<const float4*>(urow)[j];
    const float un[4] = {u4.x, u4.y, u4.z, u4.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = clampf(un[i] + p.sigma[(e + i) % p.m] * z[i], p.u_min, p.u_max, p.has_u_bounds);
    reinterpret_cast<float4*>(vrow)[j] = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e + i < p.N) vrow[e + i] = clampf(urow[e + i] + p.sigma[(e + i) % p.m] * z[i], p.u_min, p.u_max, p.has_u_bounds);
  }
  if (j == 0 && p.x0_rep) {
    for (int i = 0; i < p.n; ++i) p.x0_rep[(size_t)r * p.n + i] = p.x0[(size_t)b * p.n + i];
  }
}

__global__ __launch_bounds__(kBlock) void k_mppi_clamp(float* u, long long count, float lo, float hi) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < count) u[i] = fminf(fmaxf(u[i], lo), hi);
}

// ---------------------------------------------------------------------------------------------- k_mppi_update
template <int E4, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void k_mppi_update(MppiUpdateParams p) {
  const int lane = threadIdx.x & (kLanes - 1);
  const long long b = (long long)blockIdx.x * kPerBlock + (threadIdx.x / kLanes);
  if (b >= p.B) return;  // whole 16-lane groups leave together
  const int K = p.K, N = p.N;
  const float* s = p.s + (size_t)b * K;
  const float* v = p.v + (size_t)b * K * N;

  // beta = min over the finite costs
  float mn = INFINITY;
  for (int k = lane; k < K; k += kLanes) {
    const float sk = s[k];
    if (finite(sk) && sk < mn) mn = sk;
  }
  const float beta = row_min(mn);
  const bool any = beta < INFINITY;

  // weight sum and argmin (lowest k of cost beta)
  float ws = 0.f;
  int kmin = 0x7fffffff;
  for (int k = lane; k < K; k += kLanes) {
    const float sk = s[k];
    if (finite(sk)) {
      ws = ws + expf(-((sk - beta) / p.lambda));
      if (sk == beta && k < kmin) kmin = k;
    }
  }
  const float W = row_sum(ws);
  kmin = row_min(kmin);

  if (p.costs_out && lane == 0) p.costs_out[b] = s[0];
  if (!any) return;  // every cost non-finite: the nominal is kept, nothing can be a new best

  // weighted sum of the K sample rows, k ascending; row k + 1 in flight while row k is accumulated
  Vec<E4> acc, cur, nxt;
#pragma unroll
  for (int q = 0; q < E4; ++q) acc.v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  rload<E4, ALIGNED>(cur, v, lane, N);
  for (int k = 0; k < K; ++k) {
    if (k + 1 < K) rload<E4, ALIGNED>(nxt, v + (size_t)(k + 1) * N, lane, N);
    const float sk = s[k];
    if (finite(sk)) {
      const float w = expf(-((sk - beta) / p.lambda));
#pragma unroll
      for (int q = 0; q < E4; ++q) {
        acc.v[q].x = acc.v[q].x + w * cur.v[q].x;
        acc.v[q].y = acc.v[q].y + w * cur.v[q].y;
        acc.v[q].z = acc.v[q].z + w * cur.v[q].z;
        acc.v[q].w = acc.v[q].w + w * cur.v[q].w;
      }
    }
    if (k + 1 < K) cur = nxt;
  }
#pragma unroll
  for (int q = 0; q < E4; ++q) {
    acc.v[q].x = clampf(acc.v[q].x / W, p.u_min, p.u_max, p.has_u_bounds);
    acc.v[q].y = clampf(acc.v[q].y / W, p.u_min, p.u_max, p.has_u_bounds);
    acc.v[q].z = clampf(acc.v[q].z / W, p.u_min, p.u_max, p.has_u_bounds);
    acc.v[q].w = clampf(acc.v[q].w / W, p.u_min, p.u_max, p.has_u_bounds);
  }
  rstore<E4, ALIGNED>(acc, p.u + (size_t)b * N, lane, N);

  if (p.best_cost) {
    const float prev = p.best_cost[b];  // read by all 16 lanes before lane 0 replaces it
    if (beta < prev) {
      rload<E4, ALIGNED>(cur, v + (size_t)kmin * N, lane, N);
      rstore<E4, ALIGNED>(cur, p.best_u + (size_t)b * N, lane, N);
      if (lane == 0) p.best_cost[b] = beta;
    }
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

MppiLayout mppi_layout(long long B, int N, int n, int K) {
  const size_t r = (size_t)(B > 0 ? B : 0) * (size_t)(K > 0 ? K : 0);
  MppiLayout l;
  l.v = 0;
  l.x0_rep = align256(l.v + r * (size_t)N * sizeof(float));
  l.s = align256(l.x0_rep + r * (size_t)n * sizeof(float));
  l.total = align256(l.s + r * sizeof(float));
  return l;
}

hipError_t mppi_sample_launch(const MppiSampleParams& p, hipStream_t st) {
  const long long threads = p.B * p.K * ((p.N + 3) / 4);
  const long long blocks = (threads + kBlock - 1) / kBlock;
  if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kBlock);
  if (p.N % 4 == 0 && aligned16(p.u) && aligned16(p.v)) hipLaunchKernelGGL(k_mppi_sample<true>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(k_mppi_sample<false>, grid, block, 0, st, p);
  return hipGetLastError();
}

template <bool ALIGNED>
static hipError_t update_launch(const MppiUpdateParams& p, hipStream_t st) {
  const int nv4 = (p.N + 3) / 4;
  const dim3 grid((unsigned)((p.B + kPerBlock - 1) / kPerBlock)), block(kBlock);
  if (nv4 <= 1 * kLanes) hipLaunchKernelGGL((k_mppi_update<1, ALIGNED>), grid, block, 0, st, p);
  else if (nv4 <= 2 * kLanes) hipLaunchKernelGGL((k_mppi_update<2, ALIGNED>), grid, block, 0, st, p);
  else if (nv4 <= 3 * kLanes) hipLaunchKernelGGL((k_mppi_update<3, ALIGNED>), grid, block, 0, st, p);
  else if (nv4 <= 4 * kLanes) hipLaunchKernelGGL((k_mppi_update<4, ALIGNED>), grid, block, 0, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t mppi_update_launch(const MppiUpdateParams& p, hipStream_t st) {
  const bool al = p.N % 4 == 0 && aligned16(p.u) && aligned16(p.v) && (!p.best_cost || aligned16(p.best_u));
  return al ? update_launch<true>(p, st) : update_launch<false>(p, st);
}

hipError_t mppi_clamp_launch(float* u, long long count, float u_min, float u_max, hipStream_t st) {
  if (count < 1) return hipSuccess;
  hipLaunchKernelGGL(k_mppi_clamp, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, u, count, u_min,
                     u_max);
  return hipGetLastError();
}
