// phnn_variants.h -- the kernel variants the library instantiates, shared by the two translation units:
// phnn_mpc.hip (host side, forward kernels) and phnn_grad.hip (adjoint kernels, compiled with another
// instruction-scheduling strategy).
#pragma once
#include "phnn_kernels.hip.h"

enum Variant {
  V_NONE = 0,
  V_PHNN_4_128_FIX,  // cart-pole pHNN (cartpole_mpc_config.yaml)
  V_PHNN_4_64_FIX,
  V_PHNN_2_64_GNET,  // pendulum pHNN with learned G (pendulum_config.yaml)
  V_PHNN_2_64_FIX,
  V_CANON_128,       // canonical cart-pole pHNN
  V_CANON_64,
  V_ODE_2_128,       // ODEFunc(2,1), hidden [128,128,128]
  V_ODE_2_64,
  V_ODE_3_128,
  V_PHNN_4_128_FIX_BF,  // same models, 128x128 products as bf16x3 on the matrix pipe
  V_CANON_128_BF,
  V_PHNN_4_128_FIX_H,   // same models, 128x128 products as f16x2 on the matrix pipe
  V_CANON_128_H,
  V_ODE_2_128_H,
  V_ODE_3_128_H,
  V_ODE_4_128,  // the reference's default ODEFunc(4,1): 5 inputs; f32 only (the f16x2 image would not fit LDS)
  V_PHNN_4_128_GNET_H,  // remaining (n, G) combinations at width 128, f16x2 only
  V_PHNN_2_128_GNET_H,
  V_PHNN_2_128_FIX_H,
  V_PHNN_4_64_FIX_H,  // f16x2 forms of the 64-wide models
  V_PHNN_2_64_GNET_H,
  V_PHNN_2_64_FIX_H,
  V_CANON_64_H,
  V_ODE_2_64_H,
  V_PHNN_4_128_FIX_H_M2,   // two controls per step (m = 2): G is (n, 2), u is (B, H, 2)
  V_PHNN_4_128_GNET_H_M2,
  V_CANON_128_H_M2,
  V_PHNN_4_128_FIX_H_M3,   // three and four controls per step
  V_PHNN_4_128_GNET_H_M3,
  V_CANON_128_H_M3,
  V_PHNN_4_128_FIX_H_M4,
  V_PHNN_4_128_GNET_H_M4,
  V_CANON_128_H_M4,
  V_CANON_128_H_MCONST,  // canonical pHNN with MassMatrixNetwork 'constant' / 'diagonal' / 'full' (src/mass_matrix.py:15-216)
  V_CANON_128_H_MDIAG,
  V_CANON_128_H_MFULL,
  V_PHNN_4_128_FIX_SILU,  // other activations than Tanh (src/NN.py:13 default nn.SiLU; src/baseline_node.py:49-50 relu): all-f32 kernels
  V_PHNN_4_128_FIX_RELU,
  V_CANON_128_SILU,
  V_CANON_128_RELU,
  V_ODE_2_128_RELU,
  V_ODE_4_128_RELU,
  V_PHNN_4_128_FIX_ELU,  // nn.ELU / nn.GELU (src/baseline_node.py:53-56; src/pHNN.py:41 by name)
  V_PHNN_4_128_FIX_GELU,
  V_CANON_128_ELU,
  V_CANON_128_GELU,
  V_ODE_2_128_ELU,
  V_ODE_2_128_GELU,
  V_ODE_4_128_ELU,
  V_ODE_4_128_GELU,
};

using M_PHNN_4_128_FIX = PhnnModel<4, 128, true>;
using M_PHNN_4_64_FIX = PhnnModel<4, 64, true>;
using M_PHNN_2_64_GNET = PhnnModel<2, 64, false>;
using M_PHNN_2_64_FIX = PhnnModel<2, 64, true>;
using M_CANON_128 = CanonModel<128>;
using M_CANON_64 = CanonModel<64>;
using M_ODE_2_128 = OdeModel<2, 128>;
using M_ODE_2_64 = OdeModel<2, 64>;
using M_ODE_3_128 = OdeModel<3, 128>;
using M_PHNN_4_128_FIX_BF = PhnnModel<4, 128, true, MM_BF16X3>;
using M_CANON_128_BF = CanonModel<128, MM_BF16X3>;
using M_PHNN_4_128_FIX_H = PhnnModel<4, 128, true, MM_F16X2>;
using M_CANON_128_H = CanonModel<128, MM_F16X2>;
using M_ODE_2_128_H = OdeModel<2, 128, MM_F16X2>;
using M_ODE_3_128_H = OdeModel<3, 128, MM_F16X2>;
using M_ODE_4_128 = OdeModel<4, 128>;
using M_PHNN_4_128_GNET_H = PhnnModel<4, 128, false, MM_F16X2>;
using M_PHNN_2_128_GNET_H = PhnnModel<2, 128, false, MM_F16X2>;
using M_PHNN_2_128_FIX_H = PhnnModel<2, 128, true, MM_F16X2>;
using M_PHNN_4_64_FIX_H = PhnnModel<4, 64, true, MM_F16X2>;
using M_PHNN_2_64_GNET_H = PhnnModel<2, 64, false, MM_F16X2>;
using M_PHNN_2_64_FIX_H = PhnnModel<2, 64, true, MM_F16X2>;
using M_CANON_64_H = CanonModel<64, MM_F16X2>;
using M_ODE_2_64_H = OdeModel<2, 64, MM_F16X2>;
using M_PHNN_4_128_FIX_H_M2 = PhnnModel<4, 128, true, MM_F16X2, 2>;
using M_PHNN_4_128_GNET_H_M2 = PhnnModel<4, 128, false, MM_F16X2, 2>;
using M_CANON_128_H_M2 = CanonModel<128, MM_F16X2, 2>;
using M_PHNN_4_128_FIX_H_M3 = PhnnModel<4, 128, true, MM_F16X2, 3>;
using M_PHNN_4_128_GNET_H_M3 = PhnnModel<4, 128, false, MM_F16X2, 3>;
using M_CANON_128_H_M3 = CanonModel<128, MM_F16X2, 3>;
using M_PHNN_4_128_FIX_H_M4 = PhnnModel<4, 128, true, MM_F16X2, 4>;
using M_PHNN_4_128_GNET_H_M4 = PhnnModel<4, 128, false, MM_F16X2, 4>;
using M_CANON_128_H_M4 = CanonModel<128, MM_F16X2, 4>;
using M_CANON_128_H_MCONST = CanonModel<128, MM_F16X2, 1, MASS_CONSTANT>;
using M_CANON_128_H_MDIAG = CanonModel<128, MM_F16X2, 1, MASS_DIAGONAL>;
using M_CANON_128_H_MFULL = CanonModel<128, MM_F16X2, 1, MASS_FULL>;
using M_PHNN_4_128_FIX_SILU = PhnnModel<4, 128, true, MM_F32, 1, ACT_SILU>;
using M_PHNN_4_128_FIX_RELU = PhnnModel<4, 128, true, MM_F32, 1, ACT_RELU>;
using M_CANON_128_SILU = CanonModel<128, MM_F32, 1, MASS_CARTPOLE, ACT_SILU>;
using M_CANON_128_RELU = CanonModel<128, MM_F32, 1, MASS_CARTPOLE, ACT_RELU>;
using M_ODE_2_128_RELU = OdeModel<2, 128, MM_F32, ACT_RELU>;
using M_ODE_4_128_RELU = OdeModel<4, 128, MM_F32, ACT_RELU>;
using M_PHNN_4_128_FIX_ELU = PhnnModel<4, 128, true, MM_F32, 1, ACT_ELU>;
using M_PHNN_4_128_FIX_GELU = PhnnModel<4, 128, true, MM_F32, 1, ACT_GELU>;
using M_CANON_128_ELU = CanonModel<128, MM_F32, 1, MASS_CARTPOLE, ACT_ELU>;
using M_CANON_128_GELU = CanonModel<128, MM_F32, 1, MASS_CARTPOLE, ACT_GELU>;
using M_ODE_2_128_ELU = OdeModel<2, 128, MM_F32, ACT_ELU>;
using M_ODE_2_128_GELU = OdeModel<2, 128, MM_F32, ACT_GELU>;
using M_ODE_4_128_ELU = OdeModel<4, 128, MM_F32, ACT_ELU>;
using M_ODE_4_128_GELU = OdeModel<4, 128, MM_F32, ACT_GELU>;

// The march kernels of one model, K1 (fwd) or K2 (grad), indexed [ref][stash][integrator]: ref = reference tracking
// (phnn_reference; the REF marches), stash = K1 keeps the tape(s) of every step and K2 reads them instead of recomputing
// them, integrator = Euler, RK4.
using RollKernel = void (*)(RollParams);
using RollTable = RollKernel[2][2][2];

// Each kernel set below visits its own kernel pointers (each_kernel: as const void*, null ones included), so that what
// is done once per kernel -- phnn_create_ex raises the dynamic-LDS limit -- keeps no list of its own.  The static_assert
// next to a visitor counts the struct's fields: a kernel pointer added without the visitor does not compile.
template <class K>
const void* kernel_ptr(K* kern) { return reinterpret_cast<const void*>(kern); }
template <class F>
void each_roll(const RollTable& t, F& f) {
  for (int ref = 0; ref < 2; ++ref)
    for (int stash = 0; stash < 2; ++stash)
      for (int integ = 0; integ < 2; ++integ) f(kernel_ptr(t[ref][stash][integ]));
}
constexpr size_t set_bytes(size_t pointers, size_t ints) {  // sizeof a struct of that many pointers, then ints
  return (pointers * sizeof(void*) + ints * sizeof(int) + sizeof(void*) - 1) / sizeof(void*) * sizeof(void*);
}

template <class M>
void fill_fwd(RollTable t) {
  t[0][0][0] = k_rollout_fwd<M, PHNN_INTEG_EULER, TAPE_NONE>;
  t[0][0][1] = k_rollout_fwd<M, PHNN_INTEG_RK4, TAPE_NONE>;
  t[0][1][0] = k_rollout_fwd<M, PHNN_INTEG_EULER, TAPE_MPC>;
  t[0][1][1] = k_rollout_fwd<M, PHNN_INTEG_RK4, TAPE_MPC>;
  t[1][0][0] = k_rollout_fwd<M, PHNN_INTEG_EULER, TAPE_NONE, true>;
  t[1][0][1] = k_rollout_fwd<M, PHNN_INTEG_RK4, TAPE_NONE, true>;
  t[1][1][0] = k_rollout_fwd<M, PHNN_INTEG_EULER, TAPE_MPC, true>;
  t[1][1][1] = k_rollout_fwd<M, PHNN_INTEG_RK4, TAPE_MPC, true>;
}

// K1 keeping the training tape (phnn_rollout_trajectory_ws with a weight-gradient workspace): Euler, RK4.  Null for
// models with one tape format (no M::CURV): they use the MPC kernels of the table above.
template <class M>
void fill_fwd_train(RollKernel (&t)[2]) {
  t[0] = t[1] = nullptr;
  if constexpr (M::CURV) {
    t[0] = k_rollout_fwd<M, PHNN_INTEG_EULER, TAPE_TRAIN>;
    t[1] = k_rollout_fwd<M, PHNN_INTEG_RK4, TAPE_TRAIN>;
  }
}

template <class M>
void fill_grad(RollTable t) {
  t[0][0][0] = k_rollout_grad<M, PHNN_INTEG_EULER, false>;
  t[0][0][1] = k_rollout_grad<M, PHNN_INTEG_RK4, false>;
  t[0][1][0] = k_rollout_grad<M, PHNN_INTEG_EULER, true>;
  t[0][1][1] = k_rollout_grad<M, PHNN_INTEG_RK4, true>;
  t[1][0][0] = k_rollout_grad<M, PHNN_INTEG_EULER, false, false, true>;
  t[1][0][1] = k_rollout_grad<M, PHNN_INTEG_RK4, false, false, true>;
  t[1][1][0] = k_rollout_grad<M, PHNN_INTEG_EULER, true, false, true>;
  t[1][1][1] = k_rollout_grad<M, PHNN_INTEG_RK4, true, false, true>;
}

struct GradSet {
  RollTable grad;
  void (*mvjp)(PointParams);
};

// defined in phnn_grad.hip
bool phnn_grad_kernels(int variant, GradSet* g);

// The whole-tile kernels of one variant: K1 here (phnn_mpc.hip, make_set), K2 and the VJP from the GradSet.
struct KernelSet {
  RollTable fwd, grad;  // K1, K2
  void (*mfwd)(PointParams);
  void (*mvjp)(PointParams);
  const char* name;
  int stash_floats[2];  // per wave (16 rollouts) per step: Euler, RK4
  int scr_floats;       // per-wave LDS scratch
  int img_floats;
  // dynamic LDS of a launch with that many waves per workgroup: the image and one scratch area per wave
  size_t lds_bytes(int waves) const { return sizeof(float) * ((size_t)img_floats + (size_t)waves * scr_floats); }
  template <class F>
  void each_kernel(F f) const {
    each_roll(fwd, f);
    each_roll(grad, f);
    f(kernel_ptr(mfwd));
    f(kernel_ptr(mvjp));
  }
};
static_assert(sizeof(KernelSet) == set_bytes(8 + 8 + 2 + /* name */ 1, 4), "KernelSet::each_kernel visits every kernel?");

// Split-tile kernels (small batches: four waves share one 16-rollout tile; phnn_kernels.hip.h "Split-tile models"),
// defined in phnn_split.hip for the 128-wide f16x2 pHNN (fixed G) and canonical variants.  Bitwise the same results
// and the same tape formats as the whole-tile kernels.
struct SplitSet {
  RollTable fwd, grad;
  RollKernel fwd_t[2];  // K1 keeping the training tape: Euler, RK4
  int lds_floats;  // image + 4 x per-wave scratch + exchange area
  template <class F>
  void each_kernel(F f) const {
    each_roll(fwd, f);
    each_roll(grad, f);
    for (RollKernel k : fwd_t) f(kernel_ptr(k));
  }
};
static_assert(sizeof(SplitSet) == set_bytes(8 + 8 + 2, 1), "SplitSet::each_kernel visits every kernel?");
bool phnn_split_kernels(int variant, SplitSet* g);  // false: no split-tile kernels for this variant

// Weight-gradient kernels (training side), defined in phnn_wgrad.hip for the pHNN and canonical
// variants: the adjoint kernels built with the record flag (recompute mode) and the record reduction.
struct WgradSet {
  void (*grad[2])(RollParams);  // K2 + records: Euler, RK4
  void (*grad_t[2])(RollParams);  // the same fed by K1's tapes (a2, q1 stay out of the record)
  RollKernel fwd_t[2];            // K1 writing those tapes (TAPE_TRAIN: they carry q1): Euler, RK4
  void (*mvjp)(PointParams);    // single-evaluation VJP + record
  void (*reduce)(WgradParams);
  void (*reduce_t)(WgradParams);  // reads a2, q1 from the tapes
  int tape_floats[2];  // floats per record slot of the tapes: Euler, RK4
  int rec_floats;     // floats per record
  int blob_floats;    // floats per slab row = size of the (width-padded) weight blob
  int reduce_waves;   // waves per workgroup of the reduce kernel (= hidden width / 16)
  int reduce_lds_bytes;
  template <class F>
  void each_kernel(F f) const {
    for (int i = 0; i < 2; ++i) {
      f(kernel_ptr(grad[i]));
      f(kernel_ptr(grad_t[i]));
      f(kernel_ptr(fwd_t[i]));
    }
    f(kernel_ptr(mvjp));
    f(kernel_ptr(reduce));
    f(kernel_ptr(reduce_t));
  }
};
static_assert(sizeof(WgradSet) == set_bytes(2 + 2 + 2 + 3, 2 + 4), "WgradSet::each_kernel visits every kernel?");
bool phnn_wgrad_kernels(int variant, WgradSet* g);  // false: no weight-gradient kernels for this variant
// launches k_wgrad_finish (phnn_wgrad.hip); returns the launch status
hipError_t phnn_wgrad_finish(const float* slab, int rows, int PP, const int* map, int P, float* out, int accumulate,
                             hipStream_t stream);

// Linearisation kernels, defined in phnn_lin.hip for every variant: the point Jacobian and the
// step Jacobians along a trajectory (Euler, RK4).
using LinKernel = void (*)(LinParams);
struct LinSet {
  LinKernel jac;
  LinKernel lin[2];
  template <class F>
  void each_kernel(F f) const {
    f(kernel_ptr(jac));
    for (LinKernel k : lin) f(kernel_ptr(k));
  }
};
static_assert(sizeof(LinSet) == set_bytes(1 + 2, 0), "LinSet::each_kernel visits every kernel?");
bool phnn_lin_kernels(int variant, LinSet* g);
// launches k_tvlqr<n, m> (phnn_lin.hip), one thread per problem; hipErrorInvalidValue: no kernel for (n, m)
hipError_t phnn_tvlqr_launch(int n, int m, const TvlqrParams& p, hipStream_t stream);

#define PHNN_FOR_EACH_VARIANT(X)                                                                                      \
  X(V_PHNN_4_128_FIX, M_PHNN_4_128_FIX, "phnn<n=4,hid=128,fixedG>") \
  X(V_PHNN_4_64_FIX, M_PHNN_4_64_FIX, "phnn<n=4,hid=64,fixedG>") \
  X(V_PHNN_2_64_GNET, M_PHNN_2_64_GNET, "phnn<n=2,hid=64,Gnet>") \
  X(V_PHNN_2_64_FIX, M_PHNN_2_64_FIX, "phnn<n=2,hid=64,fixedG>") \
  X(V_CANON_128, M_CANON_128, "canonical<hid=128>") \
  X(V_CANON_64, M_CANON_64, "canonical<hid=64>") \
  X(V_ODE_2_128, M_ODE_2_128, "odefunc<n=2,hid=128>") \
  X(V_ODE_2_64, M_ODE_2_64, "odefunc<n=2,hid=64>") \
  X(V_ODE_3_128, M_ODE_3_128, "odefunc<n=3,hid=128>") \
  X(V_PHNN_4_128_FIX_BF, M_PHNN_4_128_FIX_BF, "phnn<n=4,hid=128,fixedG,bf16x3>") \
  X(V_CANON_128_BF, M_CANON_128_BF, "canonical<hid=128,bf16x3>") \
  X(V_PHNN_4_128_FIX_H, M_PHNN_4_128_FIX_H, "phnn<n=4,hid=128,fixedG,f16x2>") \
  X(V_CANON_128_H, M_CANON_128_H, "canonical<hid=128,f16x2>") \
  X(V_ODE_2_128_H, M_ODE_2_128_H, "odefunc<n=2,hid=128,f16x2>") \
  X(V_ODE_3_128_H, M_ODE_3_128_H, "odefunc<n=3,hid=128,f16x2>") \
  X(V_ODE_4_128, M_ODE_4_128, "odefunc<n=4,hid=128>") \
  X(V_PHNN_4_128_GNET_H, M_PHNN_4_128_GNET_H, "phnn<n=4,hid=128,Gnet,f16x2>") \
  X(V_PHNN_2_128_GNET_H, M_PHNN_2_128_GNET_H, "phnn<n=2,hid=128,Gnet,f16x2>") \
  X(V_PHNN_2_128_FIX_H, M_PHNN_2_128_FIX_H, "phnn<n=2,hid=128,fixedG,f16x2>") \
  X(V_PHNN_4_64_FIX_H, M_PHNN_4_64_FIX_H, "phnn<n=4,hid=64,fixedG,f16x2>") \
  X(V_PHNN_2_64_GNET_H, M_PHNN_2_64_GNET_H, "phnn<n=2,hid=64,Gnet,f16x2>") \
  X(V_PHNN_2_64_FIX_H, M_PHNN_2_64_FIX_H, "phnn<n=2,hid=64,fixedG,f16x2>") \
  X(V_CANON_64_H, M_CANON_64_H, "canonical<hid=64,f16x2>") \
  X(V_ODE_2_64_H, M_ODE_2_64_H, "odefunc<n=2,hid=64,f16x2>") \
  X(V_PHNN_4_128_FIX_H_M2, M_PHNN_4_128_FIX_H_M2, "phnn<n=4,m=2,hid=128,fixedG,f16x2>") \
  X(V_PHNN_4_128_GNET_H_M2, M_PHNN_4_128_GNET_H_M2, "phnn<n=4,m=2,hid=128,Gnet,f16x2>") \
  X(V_CANON_128_H_M2, M_CANON_128_H_M2, "canonical<m=2,hid=128,f16x2>") \
  X(V_PHNN_4_128_FIX_H_M3, M_PHNN_4_128_FIX_H_M3, "phnn<n=4,m=3,hid=128,fixedG,f16x2>") \
  X(V_PHNN_4_128_GNET_H_M3, M_PHNN_4_128_GNET_H_M3, "phnn<n=4,m=3,hid=128,Gnet,f16x2>") \
  X(V_CANON_128_H_M3, M_CANON_128_H_M3, "canonical<m=3,hid=128,f16x2>") \
  X(V_PHNN_4_128_FIX_H_M4, M_PHNN_4_128_FIX_H_M4, "phnn<n=4,m=4,hid=128,fixedG,f16x2>") \
  X(V_PHNN_4_128_GNET_H_M4, M_PHNN_4_128_GNET_H_M4, "phnn<n=4,m=4,hid=128,Gnet,f16x2>") \
  X(V_CANON_128_H_M4, M_CANON_128_H_M4, "canonical<m=4,hid=128,f16x2>") \
  X(V_CANON_128_H_MCONST, M_CANON_128_H_MCONST, "canonical<hid=128,f16x2,mass=constant>") \
  X(V_CANON_128_H_MDIAG, M_CANON_128_H_MDIAG, "canonical<hid=128,f16x2,mass=diagonal>") \
  X(V_CANON_128_H_MFULL, M_CANON_128_H_MFULL, "canonical<hid=128,f16x2,mass=full>") \
  X(V_PHNN_4_128_FIX_SILU, M_PHNN_4_128_FIX_SILU, "phnn<n=4,hid=128,fixedG,silu>") \
  X(V_PHNN_4_128_FIX_RELU, M_PHNN_4_128_FIX_RELU, "phnn<n=4,hid=128,fixedG,relu>") \
  X(V_CANON_128_SILU, M_CANON_128_SILU, "canonical<hid=128,silu>") \
  X(V_CANON_128_RELU, M_CANON_128_RELU, "canonical<hid=128,relu>") \
  X(V_ODE_2_128_RELU, M_ODE_2_128_RELU, "odefunc<n=2,hid=128,relu>") \
  X(V_ODE_4_128_RELU, M_ODE_4_128_RELU, "odefunc<n=4,hid=128,relu>") \
  X(V_PHNN_4_128_FIX_ELU, M_PHNN_4_128_FIX_ELU, "phnn<n=4,hid=128,fixedG,elu>") \
  X(V_PHNN_4_128_FIX_GELU, M_PHNN_4_128_FIX_GELU, "phnn<n=4,hid=128,fixedG,gelu>") \
  X(V_CANON_128_ELU, M_CANON_128_ELU, "canonical<hid=128,elu>") \
  X(V_CANON_128_GELU, M_CANON_128_GELU, "canonical<hid=128,gelu>") \
  X(V_ODE_2_128_ELU, M_ODE_2_128_ELU, "odefunc<n=2,hid=128,elu>") \
  X(V_ODE_2_128_GELU, M_ODE_2_128_GELU, "odefunc<n=2,hid=128,gelu>") \
  X(V_ODE_4_128_ELU, M_ODE_4_128_ELU, "odefunc<n=4,hid=128,elu>") \
  X(V_ODE_4_128_GELU, M_ODE_4_128_GELU, "odefunc<n=4,hid=128,gelu>")
