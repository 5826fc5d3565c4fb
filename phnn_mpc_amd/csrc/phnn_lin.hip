// phnn_lin.hip -- instantiates the linearisation kernels of every variant (k_model_jacobian, k_rollout_linearize) and the
// TV-LQR backward pass k_tvlqr<n, m>.  A translation unit of its own, built like phnn_grad.hip:
// the rows these kernels return are pinned bit for bit against the adjoint kernels of that unit.
#define PHNN_ADJOINT_UNIT
#include "phnn_variants.h"

template <class M>
static LinSet lin_set() {
  LinSet g;
  g.jac = k_model_jacobian<M>;
  g.lin[0] = k_rollout_linearize<M, PHNN_INTEG_EULER>;
  g.lin[1] = k_rollout_linearize<M, PHNN_INTEG_RK4>;
  return g;
}

bool phnn_lin_kernels(int variant, LinSet* g) {
  switch (variant) {
#define PHNN_CASE(V, M, NAME) \
  case V: *g = lin_set<M>(); return true;
    PHNN_FOR_EACH_VARIANT(PHNN_CASE)
#undef PHNN_CASE
    default: return false;
  }
}

constexpr int kTvlqrThreads = 64;

template <int N, int MI>
static hipError_t tvlqr_launch(const TvlqrParams& p, hipStream_t stream) {
  const unsigned grid = (unsigned)((p.B + kTvlqrThreads - 1) / kTvlqrThreads);
  hipLaunchKernelGGL((k_tvlqr<N, MI>), dim3(grid), dim3(kTvlqrThreads), 0, stream, p);
  return hipGetLastError();
}

hipError_t phnn_tvlqr_launch(int n, int m, const TvlqrParams& p, hipStream_t stream) {
  switch (n * 8 + m) {
#define PHNN_TVLQR_CASE(N, MI) \
  case N * 8 + MI: return tvlqr_launch<N, MI>(p, stream);
#define PHNN_TVLQR_ROW(N) PHNN_TVLQR_CASE(N, 1) PHNN_TVLQR_CASE(N, 2) PHNN_TVLQR_CASE(N, 3) PHNN_TVLQR_CASE(N, 4)
    PHNN_TVLQR_ROW(2)
    PHNN_TVLQR_ROW(3)
    PHNN_TVLQR_ROW(4)
#undef PHNN_TVLQR_ROW
#undef PHNN_TVLQR_CASE
    default: return hipErrorInvalidValue;
  }
}
