// phnn_feedback.hip -- the kernel of the tracking law between two solves (phnn_feedback_control):
// per problem the control of row j of the last plan plus the time-varying LQR feedback on the deviation of the current
// state from that plan's nominal row, u = clamp(clamp(u_j) + K_j (x - x_j^nominal)).  tests/feedback_model.py states
// every operation in its order; the kernel equals it bit for bit.  The unit is built with -ffp-contract=off: every
// product is rounded before it is added.
#include "phnn_feedback.h"

#include "phnn_rows.hip.h"

namespace {

using phnn_rows::clampf;

constexpr int kCtlThreads = 64;

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite64(double v) { return ((unsigned)__double2hiint(v) & 0x7ff00000u) != 0x7ff00000u; }

// ------------------------------------------------------------------------------------------------ k_feedback_control
// One thread per problem, float64 in registers; no array is indexed by a run-time value.  The plan row j = step %
// solve_every is uniform over the launch (the step comes from a device counter or from the host), so one captured
// launch serves every tracking step.  Everything is computed for every problem and the outcome (feedback, gains not
// finite, deviation not finite) selects what is written, as tests/feedback_model.py does it.  The deviation is finite
// exactly when the two float32 values it is formed from are (their difference cannot overflow a double), so that
// test runs on the floats as loaded.
template <int N, int MI>
__global__ __launch_bounds__(kCtlThreads) void k_feedback_control(FeedbackControlParams p) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const int step = p.step_dev ? *p.step_dev : p.step_host;
  int j = step % p.solve_every;
  if (j < 0) j += p.solve_every;  // never a row outside the plan
  const float* xb = p.x + b * N;
  const float* ub = p.u + (b * p.H + j) * MI;
  const float* tb = p.traj + (b * (p.H + 1) + j) * N;
  const double* Kb = p.K + (b * p.H + j) * (MI * N);

  double dx[N];
  bool bad_dx = false;
  double dev = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float xf = xb[i], tf = tb[i];
    if (!finite32(xf) || !finite32(tf)) bad_dx = true;
    dx[i] = (double)xf - (double)tf;
    dev = fmax(dev, fabs(dx[i]));
  }
  float un[MI], uo[MI];
  bool bad_K = false;
#pragma unroll
  for (int k = 0; k < MI; ++k) {
    un[k] = clampf(ub[k], p.u_min, p.u_max, p.has_u_bounds);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double g = Kb[k * N + i];
      if (!finite64(g)) bad_K = true;
      s = s + g * dx[i];
    }
    const float v = clampf((float)((double)un[k] + s), p.u_min, p.u_max, p.has_u_bounds);
    uo[k] = s == 0.0 ? un[k] : v;  // no feedback: the plan's control, a -0.0 included
  }
  // the outcome selects what is written
  const int status = bad_dx ? 2 : (bad_K ? 1 : 0);
  if (bad_dx) dev = __builtin_nan("");
#pragma unroll
  for (int k = 0; k < MI; ++k) p.u_out[b * MI + k] = status ? un[k] : uo[k];
  if (p.status) p.status[b] = status;
  if (p.dev) p.dev[b] = dev;
  if (p.log_status) p.log_status[(long long)step * p.B + b] = status;
  if (p.log_dev) p.log_dev[(long long)step * p.B + b] = dev;
}

template <int N, int MI>
hipError_t control_launch(const FeedbackControlParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kCtlThreads - 1) / kCtlThreads);
  hipLaunchKernelGGL((k_feedback_control<N, MI>), dim3(grid), dim3(kCtlThreads), 0, st, p);
  return hipGetLastError();
}

template <int N>
hipError_t control_launch_m(int m, const FeedbackControlParams& p, hipStream_t st) {
  switch (m) {
    case 1: return control_launch<N, 1>(p, st);
    case 2: return control_launch<N, 2>(p, st);
    case 3: return control_launch<N, 3>(p, st);
    case 4: return control_launch<N, 4>(p, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

FeedbackLayout feedback_layout(long long B, int H, int n, int m) {
  FeedbackLayout l{};
  const size_t b = (size_t)B, h = (size_t)H, f = sizeof(float);
  size_t off = 0;
  const auto region = [&off](size_t bytes) {
    const size_t at = off;
    off = align256(off + bytes);
    return at;
  };
  l.A = region(b * h * n * n * f);
  l.Bm = region(b * h * n * m * f);
  l.cost = region(b * f);
  l.P0 = region(b * n * n * sizeof(double));
  l.total = off;
  return l;
}

hipError_t feedback_control_launch(int n, int m, const FeedbackControlParams& p, hipStream_t st) {
  switch (n) {
    case 2: return control_launch_m<2>(m, p, st);
    case 3: return control_launch_m<3>(m, p, st);
    case 4: return control_launch_m<4>(m, p, st);
    default: return hipErrorInvalidValue;
  }
}
