// phnn_filter_layout.h -- the caller-owned workspaces of the three filter steps (phnn_ekf_step, phnn_dekf_step,
// phnn_ukf_step) as byte offsets, every region 256-byte aligned.  Host code only: the one place that states these
// layouts, read by phnn_mpc.hip for the size queries and for the steps.  DESIGN.md section 25.
#pragma once
#include <stddef.h>

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Hands out consecutive 256-byte aligned regions: r(bytes) is the offset of the next one, r.off the bytes so far.
struct Regions {
  size_t off = 0;
  size_t operator()(size_t bytes) {
    const size_t at = off;
    off = align256(off + bytes);
    return at;
  }
};

// phnn_ekf_step and phnn_dekf_step: the control row (B,1,m), K1's trajectory (B,2,n) and cost (B), A (B,n,n), Bm (B,n,m).
struct FilterStepLayout {
  size_t ctrl, traj, cost, A, Bm, total;
};
inline FilterStepLayout filter_step_layout(long long B, int n, int m) {
  const size_t b = (size_t)B * sizeof(float);  // bytes of one float per problem
  Regions r;
  return {r(b * m), r(b * 2 * n), r(b), r(b * n * n), r(b * n * m), r.off};  // a braced list: evaluated left to right
}

// phnn_ukf_step: the sigma points (B,S,n), their control rows (B,S,1,m), K1's trajectory (B*S,2,n) and cost (B*S), the
// mean (B,n) and the identity (B,n,n); S = 2 n + 1.
struct UkfLayout {
  size_t chi, ctrl, traj, cost, xm, eye, total;
};
inline UkfLayout ukf_layout(long long B, int n, int m) {
  const size_t b = (size_t)B * sizeof(float), s = (size_t)(2 * n + 1);
  Regions r;
  return {r(b * s * n), r(b * s * m), r(b * s * 2 * n), r(b * s), r(b * n), r(b * n * n), r.off};
}
