// phnn_sampling.hip -- the kernels of the two batched sampling solves (phnn_solve_mppi, phnn_solve_cem).  Per iteration
// and problem b, k_sample writes K perturbed copies of the nominal (MPPI) or mean (CEM) control sequence,
// v_k = clamp(u_b + sigma o z_k) (z_0 = 0), as the (B*K, H, m) control tensor K1 reads; K1 costs all B*K rollouts in one
// launch; and the method's update kernel moves u_b:
//   k_mppi_update  to the softmin-weighted mean  u_b = clamp(sum_k w_k v_k / sum_k w_k),  w_k = exp(-(S_k - min S) / lambda);
//   k_cem_update   refits mean and standard deviation to the E samples of lowest finite cost (cost, then k ascending):
//     em = mean of the elite rows, ev = mean of their squared deviations from em (two passes, each k ascending),
//     u_b = clamp(alpha u_b + (1 - alpha) em),  sig_b = max(sigma_min, sqrt(alpha sig_b^2 + (1 - alpha) ev)).
// DESIGN.md sections 12 (MPPI, and everything the two share) and 13 (CEM).
//
// Noise: Philox4x32-10, counter-based (phnn_sampling.h gives the counter layout): no generator state in memory, and the
// normals of (seed, epoch, iteration, global problem id, sample, float4) do not depend on the batch they are drawn in.
// One Philox call gives the four normals of one float4: two Box-Muller pairs, uniforms (x >> 8 + 0.5) * 2^-24.
// The standard deviation is the only thing the two methods' samples differ in: MPPI's is a table per control
// component in the kernel arguments, CEM's a (B, N) tensor, and k_sample is instantiated for either source.
// k_shaped_sample is k_sample with time-correlated noise, z = L eps along the horizon (the *_shaped entry points,
// DESIGN.md section 15); k_sample itself, the update kernels and K1 are the same with and without it.
//
// The update kernels have k_lbfgs's geometry: 16 lanes (one DPP row) per problem, lane l owns float4 l + 16e of the row.
// Reductions over the K samples: lane l takes k = l, l + 16, ... in order, then a DPP butterfly inside the row; every
// step combines a pair of equal-order partials, so all 16 lanes end with the same bits and the result depends on K only,
// never on the problem's position or on B.  Sample rows are streamed k ascending, row k + 1 loaded before row k is
// accumulated.
//
// CEM's elite selection is exact: every cost maps to a 32-bit key that orders as the floats do (-0 and +0 share a key,
// non-finite costs get the key above all finite ones), the E-th smallest key T is found by a 32-step descent over the
// key's bits -- each step one count over the K costs and an integer row sum -- and a row is an elite when its key is
// below T, or equals T while fewer than E - #{key < T} such rows have been taken.  The 16 lanes of a problem walk k
// together, so that running count is the same in all of them.  Only elite rows are loaded.  No transcendental anywhere
// in k_cem_update: it is pinned bit for bit against a float32 model (tests/cem_model.py).
//
// k_plant_step_ex, the extended plant step of the device closed loop (phnn_plant_step_ex), is here
// as well: its disturbance and measurement noise are draws of this unit's generator at the sampler's counters.
#include "phnn_sampling.h"

#include <math.h>

#include "phnn_rows.hip.h"

namespace {

using namespace phnn_rows;  // Philox, Box-Muller, the DPP row reductions, rload / rstore

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }  // NULL counts as aligned

template <int E4>
__device__ __forceinline__ void vzero(Vec<E4>& a) {
#pragma unroll
  for (int q = 0; q < E4; ++q) a.v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------------------- k_sample
// One thread per float4 of the sample tensor: thread t -> rollout r = t / nv4 = b * K + k, float4 j = t % nv4.
// TENSOR: sigma of element e is sig[b, e] (CEM), else the table entry sigma[e % m] (MPPI).
template <bool TENSOR, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void k_sample(SampleParams p) {
  const int nv4 = (p.N + 3) / 4;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long r = t / nv4;
  if (r >= p.B * p.K) return;
  const int j = (int)(t - r * nv4);
  const long long b = r / p.K;
  const int k = (int)(r - b * p.K);
  const int e = 4 * j;

  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (k != 0) {  // sample 0 is the nominal / mean itself
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
  const float* srow = TENSOR ? p.sig + (size_t)b * p.N : nullptr;
  float* vrow = p.v + (size_t)r * p.N;
  if (ALIGNED) {  // N % 4 == 0 and 16-byte aligned bases: 16-byte loads and one 16-byte store
    const float4 u4 = reinterpret_cast<const float4*>(urow)[j];
    const float un[4] = {u4.x, u4.y, u4.z, u4.w};
    float sn[4], o[4];
    if (TENSOR) {
      const float4 s4 = reinterpret_cast<const float4*>(srow)[j];
      sn[0] = s4.x, sn[1] = s4.y, sn[2] = s4.z, sn[3] = s4.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) sn[i] = p.sigma[(e + i) % p.m];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = clampf(un[i] + sn[i] * z[i], p.u_min, p.u_max, p.has_u_bounds);
    reinterpret_cast<float4*>(vrow)[j] = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e + i < p.N) {
        const float sg = TENSOR ? srow[e + i] : p.sigma[(e + i) % p.m];
        vrow[e + i] = clampf(urow[e + i] + sg * z[i], p.u_min, p.u_max, p.has_u_bounds);
      }
  }
  if (j == 0 && p.x0_rep) {
    for (int i = 0; i < p.n; ++i) p.x0_rep[(size_t)r * p.n + i] = p.x0[(size_t)b * p.n + i];
  }
}

__global__ __launch_bounds__(kBlock) void k_clamp(float* u, long long count, float lo, float hi) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < count) u[i] = clampf(u[i], lo, hi, 1);
}

struct SigmaInit {
  float s[4];
};

__global__ __launch_bounds__(kBlock) void k_sigma_init(float* sig, long long count, int m, SigmaInit init) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int c = (int)(i % m);
  sig[i] = c == 0 ? init.s[0] : c == 1 ? init.s[1] : c == 2 ? init.s[2] : init.s[3];
}

// ---------------------------------------------------------------------------------------------- k_shaped_sample
// k_sample with time-correlated noise: z[t, c] = sum_{s < P} L[t, s] * eps[s, c], eps the white
// normals k_sample would draw for a row of length P*m (element s*m + c), summed s ascending from 0 as
// acc = acc + L * eps (a rounded product, then a rounded sum; the unit is built with -ffp-contract=off).
// One group of G lanes per rollout r = b * K + k, G = 16, 32 or 64: the smallest that has a lane per float4 of the row
// (a wave for N > 128; four rollouts to a wave for N <= 64, so that a short row does not leave most of a wave idle).
// The 256 / G groups of a block take rows base + group, base striding over the grid, so a block stages L once for all
// the rows it serves.  Per row, lane l of its group:
//   1. makes the one Philox call of float4 l of the eps row (at most 64 calls) and leaves it in LDS;
//   2. forms z of elements e = l, l + G, l + 2G, l + 3G (t = e / m, c = e % m) and leaves them in LDS: the lanes of one
//      read walk consecutive rows t of L at one s -- the LDS row stride is odd, so they fall on distinct banks (m lanes,
//      and the groups of a wave, share a word: a broadcast) -- and one word eps[s, c] per component (the rows' eps slots
//      are 4G + 1 floats apart, so the groups of a wave read theirs from different banks);
//   3. takes float4 l of z and writes float4 l of the sample row exactly as k_sample does.
// Sample 0 skips 1 and 2 (z = 0): it reads neither L nor eps.  STAGED: L sits in LDS (dynamic, H rows of stride
// ld = P | 1 floats), else it is read in place from global memory (shared by every rollout: it stays in L2).
constexpr int kShapedMaxBlocks = 2048;
constexpr size_t kShapedStageBytes = 48 * 1024;  // L (padded) at most this large is staged in LDS

template <bool TENSOR, bool ALIGNED, bool STAGED, int G>
__global__ __launch_bounds__(kBlock) void k_shaped_sample(SampleParams p, const float* __restrict__ Lg, int P) {
  constexpr int kShapedRows = kBlock / G;  // rollouts (lane groups) per block and pass
  constexpr int kSlot = 4 * G;             // floats of a row's eps / z: G float4, 4 * G >= 4 * ceil(N / 4)
  extern __shared__ float Ls[];            // STAGED: (H, ld)
  __shared__ float eps_s[kShapedRows * (kSlot + 1)];
  __shared__ __attribute__((aligned(16))) float z_s[kShapedRows * (kSlot + 4)];
  const int lane = threadIdx.x & (G - 1), wave = threadIdx.x / G;  // `wave`: the lane group's index in the block
  const int N = p.N, m = p.m, H = N / m;
  const int nv4 = (N + 3) / 4, nvp4 = (P * m + 3) / 4;
  const int ld = STAGED ? (P | 1) : P;
  if (STAGED) {
    for (int i = threadIdx.x; i < H * P; i += kBlock) Ls[(i / P) * ld + (i % P)] = Lg[i];
  }
  const float* L = STAGED ? Ls : Lg;
  const long long rows = p.B * p.K;
  float* eps = eps_s + wave * (kSlot + 1);
  float* zz = z_s + wave * (kSlot + 4);
  for (long long base = (long long)blockIdx.x * kShapedRows; base < rows; base += (long long)gridDim.x * kShapedRows) {
    const long long r = base + wave;
    const bool live = r < rows;  // whole groups; every group keeps to the block's barriers
    const long long b = live ? r / p.K : 0;
    const int k = live ? (int)(r - b * p.K) : 0;
    if (live && k != 0 && lane < nvp4) {
      const unsigned long long gid = (unsigned long long)(p.problem_offset + b);
      const int epoch = p.epoch_dev ? *p.epoch_dev : p.epoch_host;
      U4 c;
      c.x = (unsigned)gid;
      c.y = (unsigned)(gid >> 32) | ((unsigned)p.iteration << 16);
      c.z = (unsigned)epoch;
      c.w = ((unsigned)k << 6) | (unsigned)lane;
      const U4 o = philox4x32_10(c, p.key0, p.key1);
      float e0, e1, e2, e3;
      box_muller(o.x, o.y, e0, e1);
      box_muller(o.z, o.w, e2, e3);
      eps[4 * lane + 0] = e0, eps[4 * lane + 1] = e1, eps[4 * lane + 2] = e2, eps[4 * lane + 3] = e3;
    }
    __syncthreads();  // eps rows (and, first pass, L) are in LDS
    if (live) {
      for (int e = lane; e < 4 * nv4; e += G) {
        float acc = 0.f;
        if (k != 0 && e < N) {
          const int t = e / m, c = e - t * m;
          const float* Lrow = L + (size_t)t * ld;
#pragma unroll 4  // the loads of four steps in flight; the sum stays in order
          for (int s = 0; s < P; ++s) acc = acc + Lrow[s] * eps[s * m + c];
        }
        zz[e] = acc;
      }
    }
    __syncthreads();  // z rows are in LDS
    if (live && lane < nv4) {
      const int j = lane, e = 4 * j;
      const float z[4] = {zz[e], zz[e + 1], zz[e + 2], zz[e + 3]};
      const float* urow = p.u + (size_t)b * N;
      const float* srow = TENSOR ? p.sig + (size_t)b * N : nullptr;
      float* vrow = p.v + (size_t)r * N;
      if (ALIGNED) {  // as k_sample
        const float4 u4 = reinterpret_cast<const float4*>(urow)[j];
        const float un[4] = {u4.x, u4.y, u4.z, u4.w};
        float sn[4], o[4];
        if (TENSOR) {
          const float4 s4 = reinterpret_cast<const float4*>(srow)[j];
          sn[0] = s4.x, sn[1] = s4.y, sn[2] = s4.z, sn[3] = s4.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) sn[i] = p.sigma[(e + i) % m];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = clampf(un[i] + sn[i] * z[i], p.u_min, p.u_max, p.has_u_bounds);
        reinterpret_cast<float4*>(vrow)[j] = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (e + i < N) {
            const float sg = TENSOR ? srow[e + i] : p.sigma[(e + i) % m];
            vrow[e + i] = clampf(urow[e + i] + sg * z[i], p.u_min, p.u_max, p.has_u_bounds);
          }
      }
      if (j == 0 && p.x0_rep) {
        for (int i = 0; i < p.n; ++i) p.x0_rep[(size_t)r * p.n + i] = p.x0[(size_t)b * p.n + i];
      }
    }
  }
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
  vzero(acc);
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

// ---------------------------------------------------------------------------------------------- k_cem_update
constexpr unsigned kNoKey = 0xFFFFFFFFu;  // above every finite cost's key

// unsigned key that orders as the finite floats do; -0 -> +0's key; NaN, +inf, -inf -> kNoKey
__device__ __forceinline__ unsigned cost_key(float s) {
  if (!finite(s)) return kNoKey;
  unsigned b = __float_as_uint(s);
  if (s == 0.f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// row k (key `key`) of the stream k = 0, 1, ...: among the E lowest?  `taken` counts the rows of key T taken so far
__device__ __forceinline__ bool is_elite(unsigned key, unsigned T, int ties, int& taken) {
  if (key < T) return true;
  if (key == T && taken < ties) {
    ++taken;
    return true;
  }
  return false;
}

__device__ __forceinline__ float sqdev(float acc, float x, float mean) {
  const float d = x - mean;
  return acc + d * d;
}

__device__ __forceinline__ float refit_mean(float u, float em, const CemUpdateParams& p, float oma) {
  return clampf(p.alpha * u + oma * em, p.u_min, p.u_max, p.has_u_bounds);
}

__device__ __forceinline__ float refit_sigma(float sg, float ev, const CemUpdateParams& p, float oma) {
  const float r = sqrtf(p.alpha * (sg * sg) + oma * ev);
  return r == r ? fmaxf(p.sigma_min, r) : r;  // np.maximum: a NaN deviation stays NaN
}

template <int E4, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void k_cem_update(CemUpdateParams p) {
  const int lane = threadIdx.x & (kLanes - 1);
  const long long b = (long long)blockIdx.x * kPerBlock + (threadIdx.x / kLanes);
  if (b >= p.B) return;  // whole 16-lane groups leave together
  const int K = p.K, N = p.N;
  const float* s = p.s + (size_t)b * K;
  const float* v = p.v + (size_t)b * K * N;

  // number of finite costs and the lowest key
  int nf = 0;
  unsigned lo = kNoKey;
  for (int k = lane; k < K; k += kLanes) {
    const unsigned key = cost_key(s[k]);
    nf += key != kNoKey;
    lo = min(lo, key);
  }
  nf = row_sum(nf);
  lo = (unsigned)row_min((int)(lo ^ 0x80000000u)) ^ 0x80000000u;

  if (p.costs_out && lane == 0) p.costs_out[b] = s[0];
  if (nf == 0) return;  // every cost non-finite: mean and sigma are kept, nothing can be a new best

  // T = the E-th smallest key: the largest T with #{key < T} < E, one bit per step from the top
  const int E = min(p.elites, nf);
  unsigned T = 0u;
  int below = 0;  // #{key < T}
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned trial = T | (1u << bit);
    int c = 0;
    for (int k = lane; k < K; k += kLanes) c += cost_key(s[k]) < trial;
    c = row_sum(c);
    if (c < E) {
      T = trial;
      below = c;
    }
  }
  const int ties = E - below;  // rows of key T that are elites: the first `ties` of them, k ascending
  const float Ef = (float)E;

  // em: sum of the elite rows, k ascending; the next row's fetch is in flight while the current one is accumulated
  Vec<E4> acc, em, cur, nxt;
  vzero(acc);
  vzero(cur);
  vzero(nxt);
  int kmin = 0;  // lowest k of key lo: the best sample
  int taken = 0;
  bool found = false;
  unsigned key = cost_key(s[0]);
  if (key == lo) found = true;
  bool ecur = is_elite(key, T, ties, taken);
  if (ecur) rload<E4, ALIGNED>(cur, v, lane, N);
  for (int k = 0; k < K; ++k) {
    bool enxt = false;
    if (k + 1 < K) {
      key = cost_key(s[k + 1]);
      if (!found && key == lo) {
        found = true;
        kmin = k + 1;
      }
      enxt = is_elite(key, T, ties, taken);
      if (enxt) rload<E4, ALIGNED>(nxt, v + (size_t)(k + 1) * N, lane, N);
    }
    if (ecur) {
#pragma unroll
      for (int q = 0; q < E4; ++q) {
        acc.v[q].x = acc.v[q].x + cur.v[q].x;
        acc.v[q].y = acc.v[q].y + cur.v[q].y;
        acc.v[q].z = acc.v[q].z + cur.v[q].z;
        acc.v[q].w = acc.v[q].w + cur.v[q].w;
      }
    }
    cur = nxt;
    ecur = enxt;
  }
#pragma unroll
  for (int q = 0; q < E4; ++q) {
    em.v[q].x = acc.v[q].x / Ef;
    em.v[q].y = acc.v[q].y / Ef;
    em.v[q].z = acc.v[q].z / Ef;
    em.v[q].w = acc.v[q].w / Ef;
  }

  // ev: sum of the squared deviations of the same rows from em, k ascending
  vzero(acc);
  taken = 0;
  ecur = is_elite(cost_key(s[0]), T, ties, taken);
  if (ecur) rload<E4, ALIGNED>(cur, v, lane, N);
  for (int k = 0; k < K; ++k) {
    bool enxt = false;
    if (k + 1 < K) {
      enxt = is_elite(cost_key(s[k + 1]), T, ties, taken);
      if (enxt) rload<E4, ALIGNED>(nxt, v + (size_t)(k + 1) * N, lane, N);
    }
    if (ecur) {
#pragma unroll
      for (int q = 0; q < E4; ++q) {
        acc.v[q].x = sqdev(acc.v[q].x, cur.v[q].x, em.v[q].x);
        acc.v[q].y = sqdev(acc.v[q].y, cur.v[q].y, em.v[q].y);
        acc.v[q].z = sqdev(acc.v[q].z, cur.v[q].z, em.v[q].z);
        acc.v[q].w = sqdev(acc.v[q].w, cur.v[q].w, em.v[q].w);
      }
    }
    cur = nxt;
    ecur = enxt;
  }

  // refit, in place
  const float oma = 1.0f - p.alpha;
  rload<E4, ALIGNED>(cur, p.u + (size_t)b * N, lane, N);
  rload<E4, ALIGNED>(nxt, p.sig + (size_t)b * N, lane, N);
#pragma unroll
  for (int q = 0; q < E4; ++q) {
    cur.v[q].x = refit_mean(cur.v[q].x, em.v[q].x, p, oma);
    cur.v[q].y = refit_mean(cur.v[q].y, em.v[q].y, p, oma);
    cur.v[q].z = refit_mean(cur.v[q].z, em.v[q].z, p, oma);
    cur.v[q].w = refit_mean(cur.v[q].w, em.v[q].w, p, oma);
    nxt.v[q].x = refit_sigma(nxt.v[q].x, acc.v[q].x / Ef, p, oma);
    nxt.v[q].y = refit_sigma(nxt.v[q].y, acc.v[q].y / Ef, p, oma);
    nxt.v[q].z = refit_sigma(nxt.v[q].z, acc.v[q].z / Ef, p, oma);
    nxt.v[q].w = refit_sigma(nxt.v[q].w, acc.v[q].w / Ef, p, oma);
  }
  rstore<E4, ALIGNED>(cur, p.u + (size_t)b * N, lane, N);
  rstore<E4, ALIGNED>(nxt, p.sig + (size_t)b * N, lane, N);

  if (p.best_cost) {
    const float prev = p.best_cost[b];  // read by all 16 lanes before lane 0 replaces it
    const float beta = s[kmin];
    if (beta < prev) {
      rload<E4, ALIGNED>(cur, v + (size_t)kmin * N, lane, N);
      rstore<E4, ALIGNED>(cur, p.best_u + (size_t)b * N, lane, N);
      if (lane == 0) p.best_cost[b] = beta;
    }
  }
}

// ---------------------------------------------------------------------------------------------- k_plant_step_ex
// k_plant_step (phnn_kernels.hip.h) restated with the extensions of phnn_plant_step_ex: one thread per plant, float64
// dynamics in k_plant_step's operation order (tests pin the two bit for bit), no LDS, no atomics.  At most two Philox
// calls per plant, and only those whose sigma is non-zero.
__device__ __forceinline__ U4 plant_noise(const PlantExParams& p, long long b, int step, unsigned j) {
  const unsigned long long gid = (unsigned long long)(p.plant_offset + b);
  U4 c;
  c.x = (unsigned)gid;
  c.y = (unsigned)(gid >> 32);  // iteration 0
  c.z = (unsigned)step;
  c.w = (1u << 6) | j;  // sample 1, float4 j
  return philox4x32_10(c, p.key0, p.key1);
}

__global__ __launch_bounds__(kBlock) void k_plant_step_ex(PlantExParams p) {
  const long long b = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (b >= p.B) return;
  const int step = p.step_dev ? *p.step_dev : p.step_host;
  float uf = p.action[b * p.stride];
  if (p.has_u_bounds && uf == uf) uf = fminf(fmaxf(uf, p.u_min), p.u_max);  // a NaN command stays NaN
  double force = (double)uf;
  const bool disturbed = p.force_bias || p.force_sigma > 0.f;
  float w = p.force_bias ? p.force_bias[b] : 0.f;
  if (p.force_sigma > 0.f) {
    const U4 o = plant_noise(p, b, step, 0u);
    float z0, z1;
    box_muller(o.x, o.y, z0, z1);
    w = w + p.force_sigma * z0;
  }
  if (disturbed) force = (double)uf + (double)w;  // else nothing is added: a -0.0 command stays -0.0
  const bool frozen = p.freeze_done && p.done_step[b] >= 0;

  double x = p.state[4 * b + 0], theta = p.state[4 * b + 1], x_dot = p.state[4 * b + 2], theta_dot = p.state[4 * b + 3];
  if (!frozen) {
    double gravity = p.gravity, masscart = p.masscart, masspole = p.masspole, length = p.length;
    if (p.params) gravity = p.params[4 * b + 0], masscart = p.params[4 * b + 1], masspole = p.params[4 * b + 2], length = p.params[4 * b + 3];
    const double polemass_length = masspole * length, total_mass = masspole + masscart;
    const double costheta = cos(theta), sintheta = sin(theta);
    const double temp = (force + polemass_length * (theta_dot * theta_dot) * sintheta) / total_mass;
    const double thetaacc = (gravity * sintheta - costheta * temp) / (length * (4.0 / 3.0 - masspole * (costheta * costheta) / total_mass));
    const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
    x = x + p.dt * x_dot;
    theta = theta + p.dt * theta_dot;
    x_dot = x_dot + p.dt * xacc;
    theta_dot = theta_dot + p.dt * thetaacc;
    p.state[4 * b + 0] = x;
    p.state[4 * b + 1] = theta;
    p.state[4 * b + 2] = x_dot;
    p.state[4 * b + 3] = theta_dot;
  }
  if (p.state_f32) {
    float m[4] = {(float)x, (float)theta, (float)x_dot, (float)theta_dot};
    if (p.meas_sigma[0] > 0.f || p.meas_sigma[1] > 0.f || p.meas_sigma[2] > 0.f || p.meas_sigma[3] > 0.f) {
      const U4 o = plant_noise(p, b, step, 1u);
      float z[4];
      box_muller(o.x, o.y, z[0], z[1]);
      box_muller(o.z, o.w, z[2], z[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p.meas_sigma[i] > 0.f) m[i] = m[i] + p.meas_sigma[i] * z[i];
    }
    p.state_f32[4 * b + 0] = m[0];
    p.state_f32[4 * b + 1] = m[1];
    p.state_f32[4 * b + 2] = m[2];
    p.state_f32[4 * b + 3] = m[3];
  }
  if (!frozen) {
    const bool done = fabs(x) > p.x_limit || fabs(theta) > p.theta_limit;
    if (p.done_step && done && p.done_step[b] < 0) p.done_step[b] = step;
  }
  if (p.log_states) {
    double* row = p.log_states + ((long long)(step + 1) * p.B + b) * 4;
    row[0] = x;
    row[1] = theta;
    row[2] = x_dot;
    row[3] = theta_dot;
  }
  if (p.log_controls) p.log_controls[(long long)step * p.B + b] = uf;
  if (p.disturbance_log) p.disturbance_log[(long long)step * p.B + b] = w;
  if (p.has_metrics && !frozen) {
    const double e[4] = {x - p.target[0], theta - p.target[1], x_dot - p.target[2], theta_dot - p.target[3]};
    double c = 0.0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) c = c + (e[i] * p.Q[4 * i + j]) * e[j];
      ok = ok && fabs(e[i]) <= p.tol[i];  // false for a NaN
    }
    c = c + ((double)uf * p.R) * (double)uf;
    p.cost_acc[b] = p.cost_acc[b] + c;
    const int run = ok ? p.run[b] + 1 : 0;
    p.run[b] = run;
    if (run > p.best_run[b]) p.best_run[b] = run;
  }
}

// the update kernel of the row width: table[ALIGNED][E4 - 1], E4 = float4 per lane
template <class P>
hipError_t update_launch(void (*const table[2][4])(P), const P& p, bool aligned, hipStream_t st) {
  const int e4 = ((p.N + 3) / 4 + kLanes - 1) / kLanes;
  if (e4 < 1 || e4 > 4) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.B + kPerBlock - 1) / kPerBlock)), block(kBlock);
  hipLaunchKernelGGL(table[aligned][e4 - 1], grid, block, 0, st, p);
  return hipGetLastError();
}

void (*const kMppiUpdate[2][4])(MppiUpdateParams) = {
    {k_mppi_update<1, false>, k_mppi_update<2, false>, k_mppi_update<3, false>, k_mppi_update<4, false>},
    {k_mppi_update<1, true>, k_mppi_update<2, true>, k_mppi_update<3, true>, k_mppi_update<4, true>}};
void (*const kCemUpdate[2][4])(CemUpdateParams) = {
    {k_cem_update<1, false>, k_cem_update<2, false>, k_cem_update<3, false>, k_cem_update<4, false>},
    {k_cem_update<1, true>, k_cem_update<2, true>, k_cem_update<3, true>, k_cem_update<4, true>}};

}  // namespace

SamplingLayout sampling_layout(long long B, int N, int n, int K, bool sigma_state) {
  const size_t b = (size_t)(B > 0 ? B : 0), r = b * (size_t)(K > 0 ? K : 0);
  SamplingLayout l;
  l.v = 0;
  l.x0_rep = align256(l.v + r * (size_t)N * sizeof(float));
  l.s = align256(l.x0_rep + r * (size_t)n * sizeof(float));
  l.sig = l.total = align256(l.s + r * sizeof(float));
  if (sigma_state) l.total = align256(l.sig + b * (size_t)N * sizeof(float));
  return l;
}

hipError_t sample_launch(const SampleParams& p, hipStream_t st) {
  const long long threads = p.B * p.K * ((p.N + 3) / 4);
  const long long blocks = (threads + kBlock - 1) / kBlock;
  if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kBlock);
  const bool al = p.N % 4 == 0 && aligned16(p.u) && aligned16(p.sig) && aligned16(p.v);
  if (p.sig) hipLaunchKernelGGL((al ? k_sample<true, true> : k_sample<true, false>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((al ? k_sample<false, true> : k_sample<false, false>), grid, block, 0, st, p);
  return hipGetLastError();
}

size_t sample_shaped_lds_bytes(int H, int P) {
  const size_t bytes = (size_t)H * (size_t)(P | 1) * sizeof(float);
  return bytes <= kShapedStageBytes ? bytes : 0;
}

// the shaped sample kernel of the sigma source and the row's alignment; lds: the bytes of L to stage, 0 = L stays in global memory
template <bool TENSOR, bool ALIGNED, int G>
static void sample_shaped_pick_g(const SampleParams& p, const float* L, int P, size_t lds, hipStream_t st) {
  const long long want = (p.B * p.K + kBlock / G - 1) / (kBlock / G);
  const dim3 grid((unsigned)(want < kShapedMaxBlocks ? want : kShapedMaxBlocks));
  if (lds) hipLaunchKernelGGL((k_shaped_sample<TENSOR, ALIGNED, true, G>), grid, dim3(kBlock), lds, st, p, L, P);
  else hipLaunchKernelGGL((k_shaped_sample<TENSOR, ALIGNED, false, G>), grid, dim3(kBlock), 0, st, p, L, P);
}

// G: the smallest lane group with a lane per float4 of the sample row (P <= H: the eps row is no longer)
template <bool TENSOR, bool ALIGNED>
static void sample_shaped_pick(const SampleParams& p, const float* L, int P, size_t lds, hipStream_t st) {
  const int nv4 = (p.N + 3) / 4;
  if (nv4 <= 16) sample_shaped_pick_g<TENSOR, ALIGNED, 16>(p, L, P, lds, st);
  else if (nv4 <= 32) sample_shaped_pick_g<TENSOR, ALIGNED, 32>(p, L, P, lds, st);
  else sample_shaped_pick_g<TENSOR, ALIGNED, 64>(p, L, P, lds, st);
}

hipError_t sample_shaped_launch(const SampleParams& p, const float* L, int P, hipStream_t st) {
  const long long rows = p.B * p.K;
  if (rows < 1 || !L || p.m < 1 || p.N % p.m || P < 1 || P > p.N / p.m || p.N > kSamplingMaxN) return hipErrorInvalidValue;
  const size_t lds = sample_shaped_lds_bytes(p.N / p.m, P);
  const bool al = p.N % 4 == 0 && aligned16(p.u) && aligned16(p.sig) && aligned16(p.v);
  if (p.sig) al ? sample_shaped_pick<true, true>(p, L, P, lds, st) : sample_shaped_pick<true, false>(p, L, P, lds, st);
  else al ? sample_shaped_pick<false, true>(p, L, P, lds, st) : sample_shaped_pick<false, false>(p, L, P, lds, st);
  return hipGetLastError();
}

hipError_t mppi_update_launch(const MppiUpdateParams& p, hipStream_t st) {
  const bool al = p.N % 4 == 0 && aligned16(p.u) && aligned16(p.v) && (!p.best_cost || aligned16(p.best_u));
  return update_launch(kMppiUpdate, p, al, st);
}

hipError_t cem_update_launch(const CemUpdateParams& p, hipStream_t st) {
  const bool al = p.N % 4 == 0 && aligned16(p.u) && aligned16(p.sig) && aligned16(p.v) && (!p.best_cost || aligned16(p.best_u));
  return update_launch(kCemUpdate, p, al, st);
}

hipError_t clamp_launch(float* u, long long count, float u_min, float u_max, hipStream_t st) {
  if (count < 1) return hipSuccess;
  hipLaunchKernelGGL(k_clamp, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, u, count, u_min, u_max);
  return hipGetLastError();
}

hipError_t plant_step_ex_launch(const PlantExParams& p, hipStream_t st) {
  const long long blocks = (p.B + kBlock - 1) / kBlock;
  if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_plant_step_ex, dim3((unsigned)blocks), dim3(kBlock), 0, st, p);
  return hipGetLastError();
}

hipError_t sigma_init_launch(float* sig, long long count, int m, const float* sigma_init, hipStream_t st) {
  if (count < 1) return hipSuccess;
  SigmaInit init;
  for (int i = 0; i < 4; ++i) init.s[i] = i < m ? sigma_init[i] : 0.f;
  hipLaunchKernelGGL(k_sigma_init, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, sig, count, m, init);
  return hipGetLastError();
}
