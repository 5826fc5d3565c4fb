// phnn_rows.hip.h -- device helpers shared by the sampling solves (phnn_sampling.hip): the Philox4x32-10
// noise source with its uniforms and Box-Muller, and the 16-lane (one DPP row) per-problem geometry: butterfly
// reductions that leave identical bits in every lane, and loads / stores of a lane's float4s of an unpadded row.
// DESIGN.md sections 12 and 13.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace phnn_rows {

constexpr int kLanes = 16;  // lanes per problem
constexpr int kBlock = 256;
constexpr int kPerBlock = kBlock / kLanes;

// ---------------------------------------------------------------------------------------------- Philox4x32-10
struct U4 {
  unsigned x, y, z, w;
};

__host__ __device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
    U4 n;
    n.x = (unsigned)(p1 >> 32) ^ c.y ^ k0;
    n.y = (unsigned)p1;
    n.z = (unsigned)(p0 >> 32) ^ c.w ^ k1;
    n.w = (unsigned)p0;
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// top 24 bits -> (0, 1]: (n + 0.5) * 2^-24 (float32: exact below 2^23, rounded to even above; never 0)
__device__ __forceinline__ float unit(unsigned x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-08f; }

__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(unit(a)));
  float s, c;
  sincospif(2.0f * unit(b), &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// a NaN stays NaN, as in torch.clamp (fminf / fmaxf alone would turn it into lo)
__device__ __forceinline__ float clampf(float v, float lo, float hi, int on) { return on && v == v ? fminf(fmaxf(v, lo), hi) : v; }

// ---------------------------------------------------------------------------------------------- one DPP row
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, false);
}

// over the 16 lanes of a DPP row; identical bits in every lane
__device__ __forceinline__ float row_sum(float v) {
  v = v + dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v = v + dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v = v + dpp<0x141>(v);  // row_half_mirror
  v = v + dpp<0x140>(v);  // row_mirror
  return v;
}
__device__ __forceinline__ int row_sum(int v) {
  v = v + dppi<0xB1>(v);
  v = v + dppi<0x4E>(v);
  v = v + dppi<0x141>(v);
  v = v + dppi<0x140>(v);
  return v;
}
__device__ __forceinline__ float row_min(float v) {  // no NaN reaches it
  v = fminf(v, dpp<0xB1>(v));
  v = fminf(v, dpp<0x4E>(v));
  v = fminf(v, dpp<0x141>(v));
  v = fminf(v, dpp<0x140>(v));
  return v;
}
__device__ __forceinline__ int row_min(int v) {
  v = min(v, dppi<0xB1>(v));
  v = min(v, dppi<0x4E>(v));
  v = min(v, dppi<0x141>(v));
  v = min(v, dppi<0x140>(v));
  return v;
}

__device__ __forceinline__ bool finite(float s) { return fabsf(s) < INFINITY; }  // false for NaN

template <int E4>
struct Vec {
  float4 v[E4];
};

// lane's float4s of an unpadded length-N row: 16-byte loads where the row allows them, else element loads (zero past N)
template <int E4, bool ALIGNED>
__device__ __forceinline__ void rload(Vec<E4>& r, const float* row, int lane, int N) {
#pragma unroll
  for (int q = 0; q < E4; ++q) {
    const int e = 4 * (lane + kLanes * q);
    if (ALIGNED) {
      r.v[q] = e < N ? reinterpret_cast<const float4*>(row)[lane + kLanes * q] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      r.v[q].x = e + 0 < N ? row[e + 0] : 0.f;
      r.v[q].y = e + 1 < N ? row[e + 1] : 0.f;
      r.v[q].z = e + 2 < N ? row[e + 2] : 0.f;
      r.v[q].w = e + 3 < N ? row[e + 3] : 0.f;
    }
  }
}

template <int E4, bool ALIGNED>
__device__ __forceinline__ void rstore(const Vec<E4>& r, float* row, int lane, int N) {
#pragma unroll
  for (int q = 0; q < E4; ++q) {
    const int e = 4 * (lane + kLanes * q);
    if (ALIGNED) {
      if (e < N) reinterpret_cast<float4*>(row)[lane + kLanes * q] = r.v[q];
    } else {
      if (e + 0 < N) row[e + 0] = r.v[q].x;
      if (e + 1 < N) row[e + 1] = r.v[q].y;
      if (e + 2 < N) row[e + 2] = r.v[q].z;
      if (e + 3 < N) row[e + 3] = r.v[q].w;
    }
  }
}

}  // namespace phnn_rows
