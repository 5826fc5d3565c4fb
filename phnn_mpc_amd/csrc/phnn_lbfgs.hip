// phnn_lbfgs.hip -- k_lbfgs: one slot of the batched L-BFGS solve (phnn_solve_lbfgs).  Each of B problems is its own
// torch.optim.LBFGS (torch/optim/lbfgs.py, step(), no line search), mapped onto a fixed schedule: every slot is one
// K1 + K2 evaluation of all B problems followed by one k_lbfgs launch, which consumes that evaluation for the problems
// waiting on it (slot 0: step()'s orig_loss; later slots: the evaluation after u += t*d), runs torch's break checks
// and then the next iteration body (history update, two-loop recursion, step, u += t*d).  DESIGN.md section 11.
//
// Mapping: 16 lanes (one DPP row) per problem, 4 problems per wave; lane l holds float4 l + 16k of every length-N
// vector (N = H*m, rows padded to Np = 4*ceil(N/4) floats).  Dot products: per-lane partial sums in a fixed order,
// then a DPP butterfly inside the row (quad_perm, half-mirror, mirror); every step adds a pair of equal-order sums,
// so all 16 lanes end with the same bits, and the result depends on N only, never on the problem's position or B.
// The history pairs are streamed from HBM twice per iteration (newest -> oldest, then back); the loads of entry i +- 1
// are issued before the reductions of entry i, which do not depend on them.
#include "phnn_lbfgs.h"

#include <math.h>

namespace {

constexpr int kLanes = 16;          // lanes per problem
constexpr int kBlock = 256;         // threads per workgroup
constexpr int kPerBlock = kBlock / kLanes;

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}

// sum over the 16 lanes of a DPP row; identical bits in every lane
__device__ __forceinline__ float row_sum(float v) {
  v = v + dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v = v + dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v = v + dpp<0x141>(v);  // row_half_mirror
  v = v + dpp<0x140>(v);  // row_mirror
  return v;
}

// NaN-propagating max (torch's max() returns NaN if any element is NaN)
__device__ __forceinline__ float nmax(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

__device__ __forceinline__ float row_max(float v) {
  v = nmax(v, dpp<0xB1>(v));
  v = nmax(v, dpp<0x4E>(v));
  v = nmax(v, dpp<0x141>(v));
  v = nmax(v, dpp<0x140>(v));
  return v;
}

template <int E4>
struct Vec {
  float4 v[E4];
};

template <int E4>
__device__ __forceinline__ void vload(Vec<E4>& r, const float* row, int lane, int nv4) {
  const float4* p = reinterpret_cast<const float4*>(row);
#pragma unroll
  for (int k = 0; k < E4; ++k) {
    const int j = lane + kLanes * k;
    r.v[k] = j < nv4 ? p[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <int E4>
__device__ __forceinline__ void vstore(const Vec<E4>& r, float* row, int lane, int nv4) {
  float4* p = reinterpret_cast<float4*>(row);
#pragma unroll
  for (int k = 0; k < E4; ++k) {
    const int j = lane + kLanes * k;
    if (j < nv4) p[j] = r.v[k];
  }
}

// unpadded (B, N) rows (u, grad): element loads, zero past N
template <int E4>
__device__ __forceinline__ void eload(Vec<E4>& r, const float* row, int lane, int N) {
#pragma unroll
  for (int k = 0; k < E4; ++k) {
    const int e = 4 * (lane + kLanes * k);
    r.v[k].x = e + 0 < N ? row[e + 0] : 0.f;
    r.v[k].y = e + 1 < N ? row[e + 1] : 0.f;
    r.v[k].z = e + 2 < N ? row[e + 2] : 0.f;
    r.v[k].w = e + 3 < N ? row[e + 3] : 0.f;
  }
}

template <int E4>
__device__ __forceinline__ float dot(const Vec<E4>& a, const Vec<E4>& b) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < E4; ++k) {
    s = s + a.v[k].x * b.v[k].x;
    s = s + a.v[k].y * b.v[k].y;
    s = s + a.v[k].z * b.v[k].z;
    s = s + a.v[k].w * b.v[k].w;
  }
  return row_sum(s);
}

// a += alpha * b   (Tensor.add_(b, alpha=alpha))
template <int E4>
__device__ __forceinline__ void axpy(Vec<E4>& a, float alpha, const Vec<E4>& b) {
#pragma unroll
  for (int k = 0; k < E4; ++k) {
    a.v[k].x = a.v[k].x + alpha * b.v[k].x;
    a.v[k].y = a.v[k].y + alpha * b.v[k].y;
    a.v[k].z = a.v[k].z + alpha * b.v[k].z;
    a.v[k].w = a.v[k].w + alpha * b.v[k].w;
  }
}

template <int E4>
__device__ __forceinline__ void scale(Vec<E4>& r, const Vec<E4>& a, float c) {
#pragma unroll
  for (int k = 0; k < E4; ++k) {
    r.v[k].x = a.v[k].x * c;
    r.v[k].y = a.v[k].y * c;
    r.v[k].z = a.v[k].z * c;
    r.v[k].w = a.v[k].w * c;
  }
}

template <int E4>
__device__ __forceinline__ float abs_max(const Vec<E4>& a, float c) {  // max |a * c|
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < E4; ++k) {
    m = nmax(m, fabsf(a.v[k].x * c));
    m = nmax(m, fabsf(a.v[k].y * c));
    m = nmax(m, fabsf(a.v[k].z * c));
    m = nmax(m, fabsf(a.v[k].w * c));
  }
  return row_max(m);
}

template <int E4>
__global__ __launch_bounds__(kBlock) void k_lbfgs(LbfgsParams p) {
  const int lane = threadIdx.x & (kLanes - 1);
  const long long b = (long long)blockIdx.x * kPerBlock + (threadIdx.x / kLanes);
  if (b >= p.B) return;  // whole 16-lane groups leave together
  LbfgsState st = p.st[b];
  if (p.slot != 0 && st.status != 1) return;  // idle until the next step()

  const int N = p.N, nv4 = p.Np / 4, hs = p.hs;
  const size_t vrow = (size_t)p.Np;
  float* drow = p.d + (size_t)b * vrow;
  float* pgrow = p.pg + (size_t)b * vrow;
  float* hrow = p.hist + (size_t)b * hs * 2 * vrow;  // entry e: s at hrow + 2e*Np, y at hrow + (2e+1)*Np
  float* ro = p.ro + (size_t)b * hs;
  float* al = p.al + (size_t)b * hs;

  // ---- consume this slot's evaluation: loss = float(closure()), flat_grad, opt_cond
  Vec<E4> g;
  eload(g, p.grad + (size_t)b * N, lane, N);
  const float cost = p.cost[b];
  const double loss = (double)cost;
  st.func_evals += 1;
  const bool opt_cond = abs_max(g, 1.0f) <= p.tol_grad;
  Vec<E4> d;
  bool stop = false;
  if (p.slot == 0) {  // step(): orig_loss
    if (p.costs_out && lane == 0) p.costs_out[b] = cost;
    st.evals = 1;
    st.it = 0;
    stop = opt_cond;
    if (st.n_iter > 0) vload(d, drow, lane, nv4);
  } else {  // after u += t*d: the break checks of torch's loop, in its order
    st.evals += 1;
    vload(d, drow, lane, nv4);
    stop = st.evals >= p.max_eval || opt_cond || abs_max(d, st.t) <= p.tol_change ||
           fabs(loss - st.prev_loss) < p.tol_change_d;
  }

  if (!stop) {
    // ---- the next iteration body
    st.it += 1;
    st.n_iter += 1;
    if (st.n_iter == 1) {
      scale(d, g, -1.0f);  // d = -g
      st.hdiag = 1.0f;
      st.count = 0;
      st.head = 0;
    } else {
      Vec<E4> y, s;
      vload(y, pgrow, lane, nv4);
#pragma unroll
      for (int k = 0; k < E4; ++k) {
        y.v[k].x = g.v[k].x - y.v[k].x;
        y.v[k].y = g.v[k].y - y.v[k].y;
        y.v[k].z = g.v[k].z - y.v[k].z;
        y.v[k].w = g.v[k].w - y.v[k].w;
      }
      scale(s, d, st.t);
      const float ys = dot(y, s);
      if (ys > p.ys_min) {
        const int pos = st.head;
        vstore(s, hrow + (size_t)(2 * pos) * vrow, lane, nv4);
        vstore(y, hrow + (size_t)(2 * pos + 1) * vrow, lane, nv4);
        ro[pos] = 1.0f / ys;  // every lane stores the same value and reads back its own
        st.head = pos + 1 == hs ? 0 : pos + 1;
        st.count = st.count < hs ? st.count + 1 : hs;
        st.hdiag = ys / dot(y, y);
      }
      // two-loop recursion: q = -g; newest -> oldest al_i = s_i.q ro_i, q -= al_i y_i; r = q H_diag;
      // oldest -> newest be_i = y_i.r ro_i, r += (al_i - be_i) s_i.  Entry i (0 = oldest) sits at ring position
      // (head - count + i) mod hs.
      const int cnt = st.count;
      const int base = st.head - cnt + (st.head - cnt < 0 ? hs : 0);
      Vec<E4> q;
      scale(q, g, -1.0f);
      if (cnt > 0) {
        int i = cnt - 1;
        int pos = base + i >= hs ? base + i - hs : base + i;
        vload(s, hrow + (size_t)(2 * pos) * vrow, lane, nv4);
        vload(y, hrow + (size_t)(2 * pos + 1) * vrow, lane, nv4);
        float roi = ro[pos];
        for (; i >= 0; --i) {
          Vec<E4> sn, yn;
          float ron = 0.f;
          if (i > 0) {  // prefetch entry i - 1
            const int pn = pos == 0 ? hs - 1 : pos - 1;
            vload(sn, hrow + (size_t)(2 * pn) * vrow, lane, nv4);
            vload(yn, hrow + (size_t)(2 * pn + 1) * vrow, lane, nv4);
            ron = ro[pn];
            pos = pn;
          }
          const float a = dot(s, q) * roi;
          al[i] = a;
          axpy(q, -a, y);
          if (i > 0) {
            s = sn;
            y = yn;
            roi = ron;
          }
        }
      }
      scale(d, q, st.hdiag);  // d = r = q * H_diag
      if (cnt > 0) {
        int pos = base;
        vload(y, hrow + (size_t)(2 * pos + 1) * vrow, lane, nv4);
        vload(s, hrow + (size_t)(2 * pos) * vrow, lane, nv4);
        float roi = ro[pos], ali = al[0];
        for (int i = 0; i < cnt; ++i) {
          Vec<E4> sn, yn;
          float ron = 0.f, aln = 0.f;
          if (i + 1 < cnt) {  // prefetch entry i + 1
            const int pn = pos + 1 == hs ? 0 : pos + 1;
            vload(yn, hrow + (size_t)(2 * pn + 1) * vrow, lane, nv4);
            vload(sn, hrow + (size_t)(2 * pn) * vrow, lane, nv4);
            ron = ro[pn];
            aln = al[i + 1];
            pos = pn;
          }
          const float be = dot(y, d) * roi;
          axpy(d, ali - be, s);
          if (i + 1 < cnt) {
            s = sn;
            y = yn;
            roi = ron;
            ali = aln;
          }
        }
      }
    }
    vstore(g, pgrow, lane, nv4);  // prev_flat_grad.copy_(flat_grad)
    st.prev_loss = loss;
    float t = p.lr;
    if (st.n_iter == 1) {  // t = min(1., 1. / flat_grad.abs().sum()) * lr
      float sa = 0.f;
#pragma unroll
      for (int k = 0; k < E4; ++k) sa = sa + fabsf(g.v[k].x) + fabsf(g.v[k].y) + fabsf(g.v[k].z) + fabsf(g.v[k].w);
      const float r = 1.0f / row_sum(sa);
      t = (r < 1.0f ? r : 1.0f) * p.lr;
    }
    st.t = t;
    vstore(d, drow, lane, nv4);
    const float gtd = dot(g, d);
    if (gtd > -p.tol_change) {
      stop = true;  // directional derivative below tolerance: break before moving
    } else {
      float* urow = p.u + (size_t)b * N;  // u += t * d
#pragma unroll
      for (int k = 0; k < E4; ++k) {
        const int e = 4 * (lane + kLanes * k);
        if (e + 0 < N) urow[e + 0] = urow[e + 0] + t * d.v[k].x;
        if (e + 1 < N) urow[e + 1] = urow[e + 1] + t * d.v[k].y;
        if (e + 2 < N) urow[e + 2] = urow[e + 2] + t * d.v[k].z;
        if (e + 3 < N) urow[e + 3] = urow[e + 3] + t * d.v[k].w;
      }
      stop = st.it == p.max_iter;  // the max_iter-th iteration moves without an evaluation
    }
  }
  st.status = stop ? 0 : 1;
  if (lane == 0) {
    p.st[b] = st;
    if (p.n_iter_out) p.n_iter_out[b] = st.n_iter;
    if (p.func_evals_out) p.func_evals_out[b] = st.func_evals;
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

LbfgsLayout lbfgs_layout(long long B, int N, int hs) {
  const size_t b = (size_t)(B > 0 ? B : 0), np = (size_t)((N + 3) / 4 * 4), h = (size_t)(hs > 0 ? hs : 0);
  LbfgsLayout l;
  l.st = 0;
  l.ro = align256(l.st + b * sizeof(LbfgsState));
  l.al = align256(l.ro + b * h * sizeof(float));
  l.d = align256(l.al + b * h * sizeof(float));
  l.pg = align256(l.d + b * np * sizeof(float));
  l.hist = align256(l.pg + b * np * sizeof(float));
  l.total = align256(l.hist + b * h * 2 * np * sizeof(float));
  return l;
}

hipError_t lbfgs_launch(const LbfgsParams& p, hipStream_t st) {
  const int nv4 = p.Np / 4;
  const dim3 grid((unsigned)((p.B + kPerBlock - 1) / kPerBlock)), block(kBlock);
  if (nv4 <= 1 * kLanes) hipLaunchKernelGGL(k_lbfgs<1>, grid, block, 0, st, p);
  else if (nv4 <= 2 * kLanes) hipLaunchKernelGGL(k_lbfgs<2>, grid, block, 0, st, p);
  else if (nv4 <= 3 * kLanes) hipLaunchKernelGGL(k_lbfgs<3>, grid, block, 0, st, p);
  else if (nv4 <= 4 * kLanes) hipLaunchKernelGGL(k_lbfgs<4>, grid, block, 0, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
