/*
 * phnn_mpc.h -- C-ABI of the MI355X-native batched shooting-MPC rollout engine.
 *
 * Drop-in boundary for the hot path of Peilun-Tommy-Li/pHNN-MPC (reference paths below are relative
 * to the reference checkout).  The reference has no FFI of its own: the boundary it exposes is the
 * Python object protocol model(x,u) / euler_step / rollout / compute_cost / cost.backward().  Each
 * entry point here names the reference interface it replaces; INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no C++ types or exceptions cross the boundary; every function returns a phnn_status
 *     (0 = ok, negative = error) and records a message readable with phnn_last_error();
 *   - all tensors are contiguous row-major float32; *_dev pointers are device (HBM) addresses owned by
 *     the caller (e.g. torch tensor.data_ptr()); the library owns only the packed weights in a handle;
 *   - every launch is asynchronous on the hipStream_t passed as `void* stream` (NULL = default stream);
 *     no entry point synchronises the device or allocates on the hot path;
 *   - one handle per (model, device); calls on one handle are not re-entrant from several host threads;
 *   - a call leaves the calling thread's current HIP device as it found it (the handle's device is made current
 *     only for the duration of the call).
 *
 * Buffer contract (pinned by tests/test_gpu_footprint.py with guarded buffers of exactly the stated sizes)
 *   - sizes are exact: a tensor argument has the shape stated at its entry point and a workspace the bytes its
 *     phnn_*_workspace_bytes() returns (positive for valid arguments, 0 for invalid ones, non-decreasing in B, H, samples
 *     and history_size); no call needs a byte more, and none reads or writes a byte outside those extents -- not in front
 *     of a buffer, not behind it, not for the lanes of a partly filled 16-rollout tile.  Inputs are never written;
 *   - what outputs and workspaces hold on entry is ignored: every byte a call reads from them it has written itself in
 *     that call (or, for a workspace, in the call documented to fill it: phnn_rollout_fwd before phnn_rollout_grad /
 *     _vjp, phnn_rollout_trajectory_ws before phnn_rollout_wgrad with PHNN_WGRAD_TAPES).  The exceptions accumulate, so
 *     their contents on entry are data: grad_theta_dev with PHNN_WGRAD_ACCUMULATE / accumulate = 1; best_cost_dev and
 *     best_u_dev of phnn_adam_step, phnn_mppi_update and phnn_cem_update (the solves reset them first); done_step_dev of
 *     phnn_plant_step (initialise to -1); log_states_dev / log_controls_dev, of which a call writes one row (and of
 *     phnn_plant_step_ex: disturbance_log_dev likewise, cost_acc_dev / run_dev / best_run_dev of its metrics); cost_dev of
 *     phnn_terminal_cost, which adds to what K1 wrote, and its traj_bar_dev, of which it writes row H only; and the
 *     documented in-place states (u_dev of the solves and updates, sigma_dev, exp_avg / exp_avg_sq of phnn_adam_step,
 *     state_dev, *step_dev);
 *   - alignment: float32 / int32 tensors need 4-byte and float64 tensors 8-byte alignment, with two exceptions.
 *     Workspaces must be 16-byte aligned (their sub-regions sit at multiples of 256 bytes from the base, and the kernels
 *     access them with 16-byte vectors).  For a model with state_dim n = 4 every tensor of state rows -- x0, traj,
 *     traj_bar, dx / dx_bar, grad_x0, x, lam, xbar, x0_rep -- must be 16-byte aligned: K1, K2 and the point kernels load
 *     and store a state row as one 16-byte access (n = 2, 3 use element accesses).  Controls, costs and gradients
 *     w.r.t. controls are accessed by element; the MPPI / CEM row kernels use 16-byte accesses only where H*m is a
 *     multiple of 4 and the pointers they are given are 16-byte aligned, which the library tests itself.  A row slice
 *     t[1:] of a contiguous tensor that satisfies this still does.
 */
#ifndef PHNN_MPC_H
#define PHNN_MPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHNN_MAX_N 8      /* state dimension limit (array bound of the structs below)  */
#define PHNN_MAX_M 4      /* array bound for R in phnn_cost; see PHNN_SUPPORTED_M        */
#define PHNN_SUPPORTED_M 4 /* largest input dimension with gfx950 kernels (m = 2..4: pHNN n = 4 and canonical cart-pole pHNN); phnn_create refuses more */
#define PHNN_MAX_LAYERS 4 /* hidden layers per MLP  */

typedef enum {
  PHNN_OK = 0,
  PHNN_ERR_INVALID_ARG = -1,
  PHNN_ERR_UNSUPPORTED = -2, /* dims / options the HIP kernels are not instantiated for */
  PHNN_ERR_HIP = -3,
  PHNN_ERR_ALLOC = -4
} phnn_status;

/* Dynamics model family (which reference nn.Module the handle restates). */
typedef enum {
  PHNN_MODEL_PHNN = 0,      /* src/pHNN.py:12-100            dx = (J-J^T-R(x)) dH/dx + G u          */
  PHNN_MODEL_CANONICAL = 1, /* src/pHNN_canonical.py:40-273  [q,qdot] -> [q,p] -> back, cart-pole M */
  PHNN_MODEL_ODEFUNC = 2    /* src/baseline_node.py:19-116   dx = MLP_tanh([x,u])                   */
} phnn_model_kind;

typedef enum { PHNN_INTEG_EULER = 0, PHNN_INTEG_RK4 = 1 } phnn_integrator; /* src/integrators.py:13-84 */

/* Mass matrix M(q) of the canonical model (src/pHNN_canonical.py:67-86 selects it from config model.mass_matrix.type):
 *   CARTPOLE  src/mass_matrix.py:239-370  [[a, b cos th],[b cos th, c]], parameters constants to autograd, det + 1e-6
 *   CONSTANT  src/mass_matrix.py:52-57    M = L L^T, L = tril(L_tril) with softplus(diag) + 1e-3; M^-1 = L^-T L^-1
 *   DIAGONAL  src/mass_matrix.py:59-73    M = diag(exp(mlp(q)) + 1e-3)
 *   FULL      src/mass_matrix.py:75-98    M = L(q) L(q)^T, L from mlp(q) (n(n+1)/2 outputs, softplus(diag) + 1e-3),
 *                                         M^-1 = inverse of that 2x2 matrix.   q_dim = 2 (state_dim 4) only. */
typedef enum { PHNN_MASS_CARTPOLE = 0, PHNN_MASS_CONSTANT = 1, PHNN_MASS_DIAGONAL = 2, PHNN_MASS_FULL = 3 } phnn_mass_type;

/* Activation of every MLP in the model (src/NN.py:6-40 takes any nn.Module class -- its default is nn.SiLU;
 * src/pHNN.py:41 resolves it by name; src/baseline_node.py:49-58 offers relu / tanh / elu / gelu).  Tanh is what every
 * shipped config selects and what the fast kernels implement; SiLU, ReLU, ELU (alpha = 1) and GELU (exact, erf form) run
 * on the all-f32 kernels (their activations are unbounded, so the f16 / bf16 split products do not apply; rollouts and
 * VJPs only, no weight-gradient kernels); anything else (OTHER) is refused by phnn_create so that a checkpoint trained with another activation (same
 * keys, same shapes) cannot be run as the wrong network.  One activation per model: all its MLPs must agree. */
typedef enum { PHNN_ACT_TANH = 0, PHNN_ACT_OTHER = 1, PHNN_ACT_SILU = 2, PHNN_ACT_RELU = 3, PHNN_ACT_ELU = 4, PHNN_ACT_GELU = 5 } phnn_activation;

/* How the hidden x hidden products are evaluated.  DEFAULT: f16x2 for 128-wide models, f32 for
 * narrower ones (f16x2 on the 64-wide trained pendulum model is known to exceed the stated tolerance in long
 * rollouts: phnn_create_ex refuses it there unless force_matmul is set).
 * Input range: the f16x2 rollout kernels and phnn_model_forward split the raw state into float16 hi + lo in the
 * input layers, so they hold the stated tolerances for |x_i| < 65520 (the float16 range) and return NaN for a rollout
 * with a larger component -- never a finite wrong value; phnn_model_vjp and the f32 and bf16x3 kernels have no such
 * limit.  Cotangents and cost weights may have any float32 magnitude in every mode: they are normalised per rollout
 * by exact powers of two. */
typedef enum { PHNN_MATMUL_DEFAULT = 0, PHNN_MATMUL_F32 = 1, PHNN_MATMUL_BF16X3 = 2, PHNN_MATMUL_F16X2 = 3 } phnn_matmul_mode;

/* MLP shape: Linear(in,h[0]) tanh ... Linear(h[depth-1],out); src/NN.py:6-40 with activation nn.Tanh,
 * bias=True, dropout=0, layer_norm=False (the only variant any shipped config selects). */
typedef struct {
  int32_t depth;                   /* number of hidden layers (>=1)      */
  int32_t hidden[PHNN_MAX_LAYERS]; /* hidden sizes                       */
} phnn_mlp_shape;

/* Model description.  The float32 weight blob passed to phnn_create() is the concatenation below, each
 * Linear as weight (out,in) row-major followed by bias (out) -- i.e. the reference state_dict order:
 *   PHNN      : J (n*n) | G_fixed (n*m) if fixed_G | R_net layers | H_net layers | G_net layers if !fixed_G
 *               (src/pHNN.py:22-38; R_net out = n*n, H_net out = 1, G_net out = n*m)
 *   CANONICAL : R_diag_raw (n) | G (n*m) | mass block | H_net layers
 *               (src/pHNN_canonical.py:57-110; J is the fixed canonical one); mass block by mass_type:
 *               CARTPOLE log_a, b, log_c (src/mass_matrix.py:263-268) | CONSTANT L_tril (q_dim*q_dim) |
 *               DIAGONAL / FULL the layers of M_net.mlp (in q_dim, out q_dim / q_dim(q_dim+1)/2)
 *   ODEFUNC   : network layers, in = n+m, out = n (src/baseline_node.py:60-75)
 */
typedef struct {
  int32_t kind;    /* phnn_model_kind */
  int32_t n;       /* state_dim */
  int32_t m;       /* input_dim */
  int32_t fixed_G; /* PHNN only: 1 = G_fixed buffer, 0 = learned G_net */
  phnn_mlp_shape h_net; /* H_net, or the ODEFunc network */
  phnn_mlp_shape r_net; /* PHNN only */
  phnn_mlp_shape g_net; /* PHNN with fixed_G == 0 only */
  int32_t activation;   /* phnn_activation: TANH, SILU or RELU */
  int32_t mass_type;    /* CANONICAL only: phnn_mass_type */
  phnn_mlp_shape m_net; /* CANONICAL with mass_type DIAGONAL / FULL: hidden layers of M_net.mlp */
} phnn_desc;

/* Options of phnn_create_ex; zero-initialise for the defaults. */
typedef struct {
  int32_t matmul_mode;  /* phnn_matmul_mode */
  int32_t force_matmul; /* 1: accept matmul_mode even where it is known to miss the stated tolerance (64-wide + f16x2) */
  int32_t max_waves;    /* waves per workgroup cap, 1..8; 0 = default (8).  4 = one wave per SIMD (diagnostics) */
  int32_t split_tiles;  /* small-batch kernels (four waves share one 16-rollout tile; bitwise the same results):
                         * 0 = automatic (used while the batch has at most 2 tiles per CU), 1 = never, 2 = always
                         * (where the variant has them: 128-wide f16x2 pHNN with fixed G, canonical pHNN) */
  int32_t reserved[4];  /* must be zero */
} phnn_options;

/* Stage cost of both controllers:
 *   cost = sum_{t=0..H} (x_t-x*)^T Q (x_t-x*) + sum_{t<H} u_t^T R u_t
 *        + barrier_weight * sum_{t=0..H} sum_i relu(x_min_i - x_t,i)^2 + relu(x_t,i - x_max_i)^2
 * (src/mpc_controller.py:75-114 with Q = diag, R = scalar*I; src/mpc_controller_canonical.py:91-120 with
 * full Q, R).  Controls are clamped to [u_min,u_max] before use when has_u_bounds, and the returned
 * gradient is w.r.t. the UNclamped controls (torch.clamp backward: pass-through on u_min<=u<=u_max,
 * src/mpc_controller.py:180-181).  Every clamp of the library -- here, in the sampling kernels and updates, in
 * phnn_adam_step's best_u and in phnn_plant_step -- passes a NaN on as torch.clamp does (it never becomes u_min), and
 * CEM's floor max(sigma_min, .) passes a NaN deviation on as numpy.maximum does: a diverged problem shows as NaN. */
typedef struct {
  float Q[PHNN_MAX_N * PHNN_MAX_N]; /* row-major n x n (leading n*n entries used) */
  float R[PHNN_MAX_M * PHNN_MAX_M]; /* row-major m x m */
  float x_target[PHNN_MAX_N];
  float u_min, u_max;
  int32_t has_u_bounds;
  float x_min[PHNN_MAX_N], x_max[PHNN_MAX_N];
  int32_t has_x_min, has_x_max;
  float barrier_weight; /* reference constant: 1000 */
} phnn_cost;

/* Reference trajectories (the *_ref entry points): problem b tracks its own, possibly time-varying, target,
 *   cost_b = sum_{t=0..H} (x_t - r_{b,row(t)})^T Q (x_t - r_{b,row(t)}) + sum_{t<H} u_t^T R u_t + barrier,
 *   r_{b,row} = x_ref[b * batch_stride + row * time_stride + 0 .. n-1],   row(t) = min(offset + t, rows - 1)
 * (past its end a reference holds its last row).  Everything else is phnn_cost's: Q, R (shared by the batch), the
 * u clamp, the barrier, the gradient w.r.t. the unclamped u; x_target is not read.  The difference x - r is formed
 * as x - x_target is, so a reference equal to x_target everywhere gives the non-tracking results bit for bit.
 * offset: *offset_dev when offset_dev != NULL -- read by each launch, so a captured HIP graph walks along the
 * reference when it is the counter phnn_plant_step / phnn_shift_controls advance -- else offset_host (>= 0).
 * A device offset outside [0, rows - 1] is clamped to it.  x_ref must hold every row it addresses for the B problems. */
typedef struct {
  const float* x_ref;        /* device */
  int64_t batch_stride;      /* floats between problems; 0 = shared by all */
  int64_t time_stride;       /* floats between rows;     0 = constant setpoint */
  int32_t rows;              /* >= 1 */
  const int32_t* offset_dev; /* device step counter added to the row index (graph replay), or NULL */
  int32_t offset_host;       /* used when offset_dev == NULL */
} phnn_reference;

typedef struct phnn_handle phnn_handle;

/* Build a handle: validates the description, packs the weights into the MFMA fragment order the
 * kernels stage into LDS, and uploads them to `device` once.  Replaces model construction +
 * load_state_dict (src/pHNN.py:13-38, scripts/run_cartpole_mpc.py:27-54). */
int phnn_create(const phnn_desc* desc, const float* weights_host, size_t n_floats, int device,
                phnn_handle** out);
/* Same with explicit options (NULL = defaults).  The library reads no environment variable: the Python host maps
 * PHNN_MATMUL / PHNN_MAX_WAVES to this struct as its own default (phnn_mpc_amd/engine.py). */
int phnn_create_ex(const phnn_desc* desc, const float* weights_host, size_t n_floats, int device,
                   const phnn_options* opt, phnn_handle** out);
/* Replace the weights of an existing handle (same description): re-packs and re-uploads the LDS image on `stream`
 * order.  What load_state_dict / an optimizer step on the reference module amounts to for the engine. */
int phnn_update_weights(phnn_handle* h, const float* weights_host, size_t n_floats, void* stream);
/* The same from a blob that already lives on the handle's device (e.g. the parameters of a module trained there, laid
 * out as for phnn_create): zero-padding to the kernel width and packing run as ONE small kernel in stream order -- no
 * device-to-host copy, host packing or upload, nothing to wait for on the host, and the call may be captured into a HIP
 * graph.  Same image as phnn_update_weights bit for bit, except the constants of CANONICAL models that go through
 * exp / log1p (softplus(R_diag_raw), the mass-matrix constants), where host and device math libraries may differ in the
 * last bit.  Kernels launched later on `stream` see the new weights; work on other streams must be ordered by the caller. */
int phnn_update_weights_dev(phnn_handle* h, const float* weights_dev, size_t n_floats, void* stream);
int phnn_destroy(phnn_handle* h);
/* Message of the last failing call on this handle (or of the last failing phnn_create if h == NULL). */
const char* phnn_last_error(const phnn_handle* h);
/* Number of float32 the weight blob for `desc` must hold; 0 if the description is invalid. */
size_t phnn_weight_count(const phnn_desc* desc);

/* model(x,u) -> (dx, H): src/pHNN.py:52-100, src/pHNN_canonical.py:172-273, src/baseline_node.py:88-116.
 * x_dev (B,n), u_dev (B,m) -> dx_dev (B,n), H_dev (B) (H_dev may be NULL; ODEFUNC writes 0). */
int phnn_model_forward(phnn_handle* h, const float* x_dev, const float* u_dev, int64_t B, float* dx_dev,
                       float* H_dev, void* stream);

/* Vector-Jacobian product of the dynamics, what autograd does for one model call inside
 * cost.backward(): xbar = (df/dx)^T lam, ubar = (df/du)^T lam.  lam_dev (B,n) -> xbar_dev (B,n),
 * ubar_dev (B,m). */
int phnn_model_vjp(phnn_handle* h, const float* x_dev, const float* u_dev, const float* lam_dev, int64_t B,
                   float* xbar_dev, float* ubar_dev, void* stream);

/* K1 -- fused forward march: clamp, dynamics, integrator step and stage cost over the whole horizon.
 * Replaces rollout_dynamics + compute_cost (src/mpc_controller.py:75-141), rollout + compute_cost
 * (src/mpc_controller_canonical.py:91-161) and rollout_trajectory_differentiable (src/integrators.py:192-258).
 *   x0_dev (B,n), u_dev (B,H,m) -> cost_dev (B), traj_dev (B,H+1,n) (may be NULL when neither the
 *   trajectory nor a later phnn_rollout_grad is wanted). */
int phnn_rollout_fwd(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                     const phnn_cost* cost, int32_t integrator, float dt, float* cost_dev, float* traj_dev,
                     void* workspace_dev, void* stream);

/* Optional K1 -> K2 workspace.  With workspace_dev != NULL (at least phnn_workspace_bytes() bytes) K1 also streams
 * the H_net / network activations of every dynamics evaluation to it and K2, given the same pointer, reads them back
 * instead of re-evaluating the forward pass: about half of K2's matrix work for 0.66 KB per rollout-step of extra HBM
 * traffic each way (cart-pole, Euler, default f16x2 kernels; 1.1 KB with the all-f32 / bf16x3 ones).  RK4 keeps four
 * stage slots per step (tape + stage state: 2.7 KB per rollout-step), so that K2 runs no forward evaluation at all; pass
 * NULL to trade that memory for recomputation.
 * The workspace passed to phnn_rollout_grad / phnn_rollout_vjp must have been filled by phnn_rollout_fwd with the
 * same (x0, u, B, H, cost, integrator, dt). */
size_t phnn_workspace_bytes(const phnn_handle* h, int64_t B, int32_t H, int32_t integrator);

/* K2 -- adjoint march: replaces cost.backward() (src/mpc_controller.py:192,
 * src/mpc_controller_canonical.py:205).  Reads the states K1 wrote to traj_dev, re-evaluates the
 * dynamics at each of them, and marches the costate backwards (explicit Hessian-vector product of
 * H_net).  -> grad_u_dev (B,H,m) = d cost_b / d u_b (unclamped), grad_x0_dev (B,n) or NULL. */
int phnn_rollout_grad(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                      const phnn_cost* cost, int32_t integrator, float dt, const float* traj_dev,
                      const void* workspace_dev, float* grad_u_dev, float* grad_x0_dev, void* stream);

/* General reverse pass of the rollout, what autograd does when a loss is built on BOTH outputs of
 * rollout_trajectory_differentiable + compute_cost (src/integrators.py:192-258): given cotangents
 * traj_bar_dev (B,H+1,n) on the trajectory (may be NULL = 0) and cost_bar_dev (B) on the cost (may be NULL = 1),
 * returns grad_u_dev (B,H,m) and grad_x0_dev (B,n) (may be NULL).  phnn_rollout_grad is the special case
 * traj_bar = 0, cost_bar = 1. */
int phnn_rollout_vjp(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                     const phnn_cost* cost, int32_t integrator, float dt, const float* traj_dev,
                     const void* workspace_dev, const float* traj_bar_dev, const float* cost_bar_dev,
                     float* grad_u_dev, float* grad_x0_dev, void* stream);

/* K1 / K2 tracking a reference (phnn_reference above): the same as phnn_rollout_fwd / phnn_rollout_grad with the
 * stage cost of problem b taken about its reference rows instead of cost->x_target (same workspace and stash
 * format; the workspace a phnn_rollout_fwd_ref filled serves the phnn_rollout_grad_ref of the same reference).
 * PHNN_ERR_INVALID_ARG for ref == NULL, x_ref == NULL (B > 0), rows < 1, negative strides or offset_host < 0. */
int phnn_rollout_fwd_ref(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                         const phnn_cost* cost, const phnn_reference* ref, int32_t integrator, float dt, float* cost_dev,
                         float* traj_dev, void* workspace_dev, void* stream);
int phnn_rollout_grad_ref(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                          const phnn_cost* cost, const phnn_reference* ref, int32_t integrator, float dt,
                          const float* traj_dev, const void* workspace_dev, float* grad_u_dev, float* grad_x0_dev,
                          void* stream);

/* phnn_rollout_vjp tracking a reference: the stage cost's part of the gradient is taken about the reference rows, as in
 * phnn_rollout_grad_ref; traj_bar_dev and cost_bar_dev as in phnn_rollout_vjp.  The same K2 launch as
 * phnn_rollout_grad_ref, which is the special case traj_bar = 0, cost_bar = 1 (the solve with a terminal weight hands the
 * terminal term's gradient in through traj_bar_dev). */
int phnn_rollout_vjp_ref(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                         const phnn_cost* cost, const phnn_reference* ref, int32_t integrator, float dt,
                         const float* traj_dev, const void* workspace_dev, const float* traj_bar_dev,
                         const float* cost_bar_dev, float* grad_u_dev, float* grad_x0_dev, void* stream);

/* ---- training side: rollouts with gradients w.r.t. the MODEL PARAMETERS ----------------------
 * What loss.backward() does in the reference's training loops (scripts/train_cartpole_phnn.py:112-178,
 * scripts/train_cartpole_phnn_canonical.py:83-196, main.py:93-148): an Euler (or RK4) rollout from x_batch[:,0] with
 * the dataset's controls, a loss built on the predicted states X_pred and/or the per-step derivatives dX_pred, and the
 * gradient of that loss w.r.t. every parameter.  The loss itself stays with the caller (torch): these entry points take
 * its cotangents on the two outputs and return the parameter gradient as a blob laid out exactly like the weight blob
 * of phnn_create (buffers of the reference modules -- G_fixed, the canonical G -- and the CartPoleMassMatrix
 * parameters, which are constants to autograd through .item(), src/mass_matrix.py:299-301, stay zero).
 * Available for the variants with weight-gradient kernels: the tanh PHNN and CANONICAL ones.  PHNN_ERR_UNSUPPORTED for
 * every other handle -- ODEFUNC, and the all-f32 kernels of the other activations -- whose
 * phnn_wgrad_workspace_bytes() is 0. */

/* Forward of a training rollout: no clamp, no cost.  -> traj_dev (B,H+1,n) = X_pred, dx_dev (B,H,n) = dX_pred
 * (f(x_t,u_t) at the first stage of each step; may be NULL). */
int phnn_rollout_trajectory(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                            int32_t integrator, float dt, float* traj_dev, float* dx_dev, void* stream);

/* The same, and with wgrad_workspace_dev != NULL (phnn_wgrad_workspace_bytes() bytes, the buffer later handed to
 * phnn_rollout_wgrad) it also keeps the tapes of every dynamics evaluation in that workspace, so that
 * phnn_rollout_wgrad(..., flags | PHNN_WGRAD_TAPES) neither re-evaluates the forward pass nor copies the tapes into
 * its records (training pass 6.6 -> 5.x ms at B = 65536, H = 50). */
int phnn_rollout_trajectory_ws(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H,
                               int32_t integrator, float dt, float* traj_dev, float* dx_dev, void* wgrad_workspace_dev,
                               void* stream);

/* Bytes of workspace phnn_rollout_wgrad (H >= 1) / phnn_model_wgrad (H = 0, B = number of points) need. */
size_t phnn_wgrad_workspace_bytes(const phnn_handle* h, int64_t B, int32_t H, int32_t integrator);

/* flags of phnn_rollout_wgrad / phnn_model_wgrad */
#define PHNN_WGRAD_ACCUMULATE 1 /* add to grad_theta_dev instead of overwriting it */
#define PHNN_WGRAD_TAPES 2      /* the workspace holds the tapes phnn_rollout_trajectory_ws wrote for the SAME
                                   (x0, u, B, H, integrator, dt) and weights; anything else gives wrong gradients */

/* Layout of the records phnn_rollout_wgrad / phnn_model_wgrad leave at the start of the workspace: record r (one per
 * 16-point tile and evaluation: tile-major, then step, then RK4 stage) starts at float r * record_floats; its
 * per-point block starts small_offset floats in and holds small_stride floats for each of the tile's 16 points.  For
 * CANONICAL handles with a MassMatrixNetwork (mass_type != PHNN_MASS_CARTPOLE) floats 20..23 of a point's block are the
 * cotangent of the 2 x 2 matrix M(q) (row-major) of that evaluation and floats 24, 25 its q: the gradient of the mass
 * network's parameters -- which the kernels leave at zero in grad_theta -- is one autograd pass of the caller's
 * MassMatrixNetwork over those points (phnn_mpc_amd/models.py does exactly that); points beyond B carry zero cotangents. */
int phnn_wgrad_record_info(const phnn_handle* h, int32_t* record_floats, int32_t* small_offset, int32_t* small_stride);

/* Reverse pass of the training rollout.  traj_dev: the states phnn_rollout_trajectory wrote; traj_bar_dev (B,H+1,n) and
 * dx_bar_dev (B,H,n): cotangents of the loss on X_pred and dX_pred (either may be NULL = 0).
 * -> grad_theta_dev (phnn_weight_count floats; overwritten, or added to with PHNN_WGRAD_ACCUMULATE), grad_u_dev (B,H,m)
 * and grad_x0_dev (B,n) (both may be NULL).  Two kernels: the adjoint march, which also streams one record per
 * (16-rollout tile, step, stage) to the workspace, and a reduction of the records into the gradient (GEMMs over the
 * evaluation points; fixed summation order, bitwise reproducible). */
int phnn_rollout_wgrad(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H, int32_t integrator,
                       float dt, const float* traj_dev, const float* traj_bar_dev, const float* dx_bar_dev,
                       void* workspace_dev, float* grad_theta_dev, int32_t flags, float* grad_u_dev,
                       float* grad_x0_dev, void* stream);

/* Single evaluations: gradient of sum_p lam_p . f(x_p,u_p) + Hbar_p H(x_p) w.r.t. the parameters (what backward() does
 * for model(x,u) calls outside a rollout, e.g. the energy anchor H(0)^2 of scripts/train_cartpole_phnn.py:166-170),
 * plus xbar_dev (N,n) and ubar_dev (N,m) as phnn_model_vjp (with Hbar dH/dx added).  Hbar_dev (N) may be NULL. */
int phnn_model_wgrad(phnn_handle* h, const float* x_dev, const float* u_dev, const float* lam_dev, const float* Hbar_dev,
                     int64_t N, void* workspace_dev, float* grad_theta_dev, int32_t accumulate, float* xbar_dev,
                     float* ubar_dev, void* stream);

/* K3 -- Adam step on the controls, arithmetic order of torch.optim.Adam (single-tensor, defaults:
 * no weight decay / amsgrad) as used by src/mpc_controller.py:168,200 and
 * src/mpc_controller_canonical.py:186,206.  `step` is the 1-based step count after the increment.
 * Optionally fuses the best-iterate tracking of src/mpc_controller_canonical.py:208-214: when
 * best_cost_dev != NULL, rollouts whose cost_dev[b] < best_cost_dev[b] copy clamp(u_b) (the pre-step
 * iterate that produced cost_dev) into best_u_dev and update best_cost_dev.  count = B*H*m, per = H*m.
 * Known deviation: lr, beta1, beta2 and eps arrive as C floats and are widened back, so the defaults are 0.9f and 0.999f,
 * not torch's doubles 0.9 and 0.999 (1 - beta2 is 1.3e-5 relative off). */
int phnn_adam_step(phnn_handle* h, float* u_dev, const float* grad_dev, float* exp_avg_dev,
                   float* exp_avg_sq_dev, int64_t count, float lr, float beta1, float beta2, float eps,
                   int32_t step, const float* cost_dev, float* best_cost_dev, float* best_u_dev, int64_t per,
                   float u_min, float u_max, int32_t has_u_bounds, void* stream);

/* The whole shooting solve behind MPCController.compute_control (src/mpc_controller.py:164-209) and
 * MPCControllerCanonical.optimize_control (src/mpc_controller_canonical.py:163-228) for B independent problems:
 * `iters` times { cost and gradient of the current iterate (K1, K2); Adam step (K3) }, a fresh optimizer state per call.
 *   u_dev (B,H,m): in = initial iterate (zeros for a cold start, the shifted previous solution for a warm start),
 *                  out = the LAST iterate, unclamped (compute_control returns clamp(u[0]) of it);
 *   track_best: best_u_dev (B,H,m) / best_cost_dev (B) receive the clamped iterate of lowest cost, the cost of iterate k
 *               being measured before step k is applied, strict '<' (what optimize_control returns);
 *   costs_dev (iters,B) or NULL: the cost history (info['costs'] of the canonical controller);
 *   exp_avg_dev, exp_avg_sq_dev, grad_dev (B,H,m), cost_dev (B), traj_dev (B,H+1,n): caller-owned scratch, overwritten;
 *   workspace_dev: phnn_workspace_bytes() bytes (K1 -> K2 tape) or NULL (the adjoint recomputes).
 * The call enqueues the 3 x iters launches on `stream` (stream-ordered, no host synchronisation; small batches run on the
 * split-tile kernels).  A fused one-launch form was measured and dropped: back-to-back launches are already pipelined, a
 * single-plant solve is the serial chain of its time steps. */
typedef struct {
  int32_t iters;
  float lr, beta1, beta2, eps; /* torch.optim.Adam: lr, betas (0.9, 0.999), eps 1e-8 */
  int32_t track_best;
} phnn_solve_options;
int phnn_solve(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
               int32_t integrator, float dt, const phnn_solve_options* opt, float* exp_avg_dev, float* exp_avg_sq_dev,
               float* grad_dev, float* cost_dev, float* traj_dev, void* workspace_dev, float* costs_dev,
               float* best_cost_dev, float* best_u_dev, void* stream);
/* phnn_solve with every K1 / K2 of the solve tracking `ref` (phnn_rollout_fwd_ref / phnn_rollout_grad_ref); with
 * ref->offset_dev the offset is read by every launch, so a captured closed-loop step advances along the reference. */
int phnn_solve_ref(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                   const phnn_reference* ref, int32_t integrator, float dt, const phnn_solve_options* opt,
                   float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_dev, float* cost_dev, float* traj_dev,
                   void* workspace_dev, float* costs_dev, float* best_cost_dev, float* best_u_dev, void* stream);

/* ---- batched L-BFGS solve (src/mpc_controller.py:169-170,196-197: optimizer 'LBFGS') ---------------------------
 * Problem b is its own torch.optim.LBFGS([u_b], lr, max_iter, max_eval, tolerance_grad, tolerance_change,
 * history_size, line_search_fn=None), created fresh per call and stepped outer_steps times; its closure is the K1 cost
 * and the K2 gradient (w.r.t. the unclamped u) of that problem.  The data-dependent loop of step() runs on a fixed
 * schedule: per outer step, max_iter slots of (K1, K2, k_lbfgs) for all B problems; k_lbfgs consumes the slot's
 * evaluation for the problems waiting on one and leaves the others idle (their K1 / K2 results are ignored).
 * Arithmetic: vectors and the scalars ys, ro, H_diag, al, be, t, gtd in float32 with a fixed reduction order per
 * problem (results do not depend on B or on a problem's position); the loss is the float32 cost widened to double.
 * DESIGN.md 11. */
typedef struct {
  int32_t outer_steps;      /* optimizer.step(closure) calls */
  int32_t max_iter;         /* >= 1 (torch default 20) */
  int32_t max_eval;         /* 0: torch's default max_iter * 5 / 4 */
  int32_t history_size;     /* >= 1 (torch default 100) */
  double lr;                /* finite (torch default 1) */
  double tolerance_grad;    /* torch default 1e-7 */
  double tolerance_change;  /* torch default 1e-9 */
  int32_t reserved[4];      /* zero */
} phnn_lbfgs_options;
/* Bytes of the L-BFGS workspace for B problems of horizon H and this handle's m: per-problem scalars, the (s, y)
 * history ring [B][history_size][2][H*m] (rows padded to 16 bytes), direction, previous gradient and two-loop scratch.
 * 0 for invalid arguments. */
size_t phnn_lbfgs_workspace_bytes(const phnn_handle* h, int64_t B, int32_t H, int32_t history_size);
/* u_dev (B,H,m) holds the initial iterate on entry and the last one on return (unclamped).  grad_dev (B,H,m),
 * cost_dev (B), traj_dev (B,H+1,n) and stash_workspace (phnn_workspace_bytes, or NULL) serve K1 / K2 as in phnn_solve;
 * lbfgs_workspace (lbfgs_workspace_size >= phnn_lbfgs_workspace_bytes) holds the optimizer state.  Optional outputs:
 * costs_dev (outer_steps,B) the orig_loss of every step() call, n_iter_dev / func_evals_dev (B) int32 state['n_iter'] /
 * state['func_evals'].  ref: NULL = the cost's x_target, else every K1 / K2 tracks it (phnn_solve_ref; offset_dev is
 * read by every launch).  Enqueues the state reset (zero counters), then outer_steps x max_iter x (K1, K2, k_lbfgs);
 * stream-ordered, capturable.  outer_steps == 0 or B == 0 returns PHNN_OK after the reset.  PHNN_ERR_INVALID_ARG for
 * history_size < 1, max_iter < 1, max_eval < 0, outer_steps < 0, a non-finite lr, NULL required buffers or a too
 * small workspace; PHNN_ERR_UNSUPPORTED for H*m > 256. */
int phnn_solve_lbfgs(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                     const phnn_reference* ref, int32_t integrator, float dt, const phnn_lbfgs_options* opt,
                     float* grad_dev, float* cost_dev, float* traj_dev, void* stash_workspace, void* lbfgs_workspace,
                     size_t lbfgs_workspace_size, float* costs_dev, int32_t* n_iter_dev, int32_t* func_evals_dev,
                     void* stream);

/* ---- batched sampling (MPPI) solve: gradient-free, K1 only -----------------------------------------------------
 * Per problem b, `iters` times: sample  v_{b,k} = clamp(u_b + sigma o z_{b,k}), k = 0 .. samples-1, z standard normal
 * and z_{b,0} = 0 (the nominal itself is always evaluated); cost S_{b,k} of all B * samples rollouts in ONE K1 launch
 * (no K2, no stash); update  u_b = sum_k w_k v_{b,k} / sum_k w_k,  w_k = exp(-(S_k - min_k S) / lambda).  A non-finite
 * S_k has weight 0; where all are non-finite u_b is kept.  The control effort u^T R u of a sample is inside S; there is
 * no separate control-cost term.  DESIGN.md 12.
 * Noise: Philox4x32-10, one call per float4 of a sample row, key = seed, counter = (gid low 32 bits,
 * gid high 16 bits | iteration << 16, epoch, sample << 6 | float4 index) with gid = problem_offset + b; two Box-Muller
 * pairs per call, uniforms ((x >> 8) + 0.5) * 2^-24.  Problem b's samples therefore depend on (seed, epoch, iteration,
 * gid) only -- not on B, on its position in the batch, or on how the batch is split over calls.  Ranges: iters <= 65536,
 * samples <= 2^26, 0 <= problem_offset, problem_offset + B <= 2^48.
 * epoch: *epoch_dev when epoch_dev != NULL -- read by every launch, so a captured graph whose counter
 * phnn_shift_controls advances draws fresh noise at every replay -- else epoch_host. */
typedef struct {
  int32_t iters;             /* >= 0 */
  int32_t samples;           /* K >= 2, sample 0 included */
  float lambda;              /* temperature, > 0 and finite */
  float sigma[PHNN_MAX_M];   /* noise standard deviation per control component (leading m used), >= 0 and finite */
  uint64_t seed;
  int64_t problem_offset;    /* global id of problem 0 of this call */
  const int32_t* epoch_dev;  /* device, or NULL */
  int32_t epoch_host;        /* used when epoch_dev == NULL */
  int32_t reserved[4];       /* zero */
} phnn_mppi_options;
/* Bytes of the MPPI workspace: the sample tensor (B*samples, H, m), the replicated x0 (B*samples, n) and K1's cost
 * vector (B*samples), each region 256-byte aligned.  0 for invalid arguments. */
size_t phnn_mppi_workspace_bytes(const phnn_handle* h, int64_t B, int32_t H, int32_t samples);
/* The two kernels of one iteration, as phnn_adam_step stands next to phnn_solve.
 * phnn_mppi_sample: u_dev (B,H,m) nominal, x0_dev (B,n) -> samples_dev (B*samples,H,m), x0_rep_dev (B*samples,n) (may be
 *   NULL); clamps to the cost's bounds when has_u_bounds; `iteration` is the counter field (opt->iters is not read).
 * phnn_mppi_update: samples_dev and their K1 costs sample_cost_dev (B*samples) -> u_dev (B,H,m) replaced by the weighted
 *   mean, clamped to the cost's bounds when has_u_bounds (in exact arithmetic a convex combination of in-bound samples is
 *   in bounds; float32 rounding can leave it one ulp outside); optional costs_row_dev (B) = S_{b,0}; optional best_cost_dev (B) / best_u_dev (B,H,m), updated where the lowest
 *   finite sample cost is < best_cost (strict; lowest k on ties) with that cost and that sample's row. */
int phnn_mppi_sample(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                     const phnn_mppi_options* opt, int32_t iteration, float* samples_dev, float* x0_rep_dev, void* stream);
int phnn_mppi_update(phnn_handle* h, float* u_dev, const float* samples_dev, const float* sample_cost_dev, int64_t B,
                     int32_t H, const phnn_cost* cost, const phnn_mppi_options* opt, float* costs_row_dev,
                     float* best_cost_dev, float* best_u_dev, void* stream);
/* The whole solve.  u_dev (B,H,m): in = initial nominal, out = the last nominal (in bounds: clamped on entry when
 * has_u_bounds, and every update is a clamped convex combination of in-bound samples).  best_cost_dev (B) / best_u_dev (B,H,m):
 * the best sample over all iterations, reset to +inf / 0 first -- also when iters == 0.  costs_dev (iters,B) or NULL: the
 * nominal's cost S_{b,0} at every iteration.  workspace: workspace_size >= phnn_mppi_workspace_bytes.  ref: NULL = the
 * cost's x_target, else K1 tracks it; its batch_stride indexes the B*samples ROLLOUTS (rollout b*samples + k belongs to
 * problem b), so a per-problem reference is passed with one row set per rollout and a shared one with batch_stride 0.
 * Enqueues the clamp and the resets, then iters x (k_sample, K1, k_mppi_update); stream-ordered, capturable.
 * PHNN_ERR_INVALID_ARG for samples < 2, lambda <= 0 or non-finite, a negative or non-finite sigma, iters < 0, values
 * outside the ranges above, NULL required buffers or a too small workspace; PHNN_ERR_UNSUPPORTED for H*m > 256. */
int phnn_solve_mppi(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                    const phnn_reference* ref, int32_t integrator, float dt, const phnn_mppi_options* opt, void* workspace,
                    size_t workspace_size, float* costs_dev, float* best_cost_dev, float* best_u_dev, void* stream);

/* ---- batched cross-entropy (CEM) solve: gradient-free, K1 only, adaptive per-element noise ------------------------
 * Per problem b a mean u_b (H,m), started at clamp(u_init_b), and a standard deviation sig_b (H,m), element (t,c) started
 * at sigma_init[c] (fresh at every solve).  `iters` times: sample  v_{b,k} = clamp(u_b + sig_b o z_{b,k}), k = 0 ..
 * samples-1, z standard normal and z_{b,0} = 0 (the mean itself is always evaluated and is an ordinary candidate); cost
 * S_{b,k} of all B * samples rollouts in ONE K1 launch (no K2, no stash); elites: of the samples with finite cost the
 * `elites` lowest in the order (cost as floats, -0 == +0, then k ascending) -- all of them when fewer are finite; refit
 *   em = mean of the elite rows,  ev = mean of their squared deviations from em (two passes, each k ascending),
 *   u_b = clamp(alpha u_b + (1 - alpha) em),  sig_b = max(sigma_min, sqrt(alpha sig_b^2 + (1 - alpha) ev)),
 * float32 with separate multiplications and additions and correctly rounded division and square root.  Where no cost is
 * finite u_b and sig_b are kept bit for bit.  The only cost-related parameter is the count `elites`: the solve is
 * invariant to any monotone rescaling of the cost.  DESIGN.md 13.
 * Noise: the MPPI counter layout above (key = seed, counter = (gid, iteration, epoch, sample, float4)), so problem b's
 * samples depend on (seed, epoch, iteration, gid = problem_offset + b) only; same ranges; epoch as in phnn_mppi_options. */
typedef struct {
  int32_t iters;                  /* >= 0 */
  int32_t samples;                /* K >= 2, sample 0 (the mean) included */
  int32_t elites;                 /* E, 1 <= E <= samples */
  float alpha;                    /* smoothing in [0, 1): 0 = plain refit */
  float sigma_init[PHNN_MAX_M];   /* initial standard deviation per control component (leading m used), >= 0 and finite */
  float sigma_min;                /* floor of the refitted standard deviation, >= 0 and finite */
  uint64_t seed;
  int64_t problem_offset;         /* global id of problem 0 of this call */
  const int32_t* epoch_dev;       /* device, or NULL */
  int32_t epoch_host;             /* used when epoch_dev == NULL */
  int32_t reserved[4];            /* zero */
} phnn_cem_options;
/* Bytes of the CEM workspace: the MPPI layout (sample tensor, replicated x0, K1's cost vector) plus the sigma state
 * (B, H, m), each region 256-byte aligned.  0 for invalid arguments. */
size_t phnn_cem_workspace_bytes(const phnn_handle* h, int64_t B, int32_t H, int32_t samples);
/* The two kernels of one iteration.
 * phnn_cem_sample: mean u_dev (B,H,m), sigma_dev (B,H,m), x0_dev (B,n) -> samples_dev (B*samples,H,m), x0_rep_dev
 *   (B*samples,n) (may be NULL); clamps to the cost's bounds when has_u_bounds; `iteration` is the counter field.
 * phnn_cem_update: samples_dev and their K1 costs sample_cost_dev (B*samples) -> u_dev and sigma_dev refitted in place;
 *   optional costs_row_dev (B) = S_{b,0}; optional best_cost_dev (B) / best_u_dev (B,H,m), updated where the lowest finite
 *   sample cost is < best_cost (strict; lowest k on ties) with that cost and that sample's row. */
int phnn_cem_sample(phnn_handle* h, const float* x0_dev, const float* u_dev, const float* sigma_dev, int64_t B, int32_t H,
                    const phnn_cost* cost, const phnn_cem_options* opt, int32_t iteration, float* samples_dev,
                    float* x0_rep_dev, void* stream);
int phnn_cem_update(phnn_handle* h, float* u_dev, float* sigma_dev, const float* samples_dev, const float* sample_cost_dev,
                    int64_t B, int32_t H, const phnn_cost* cost, const phnn_cem_options* opt, float* costs_row_dev,
                    float* best_cost_dev, float* best_u_dev, void* stream);
/* The whole solve.  u_dev (B,H,m): in = initial mean, out = the last mean (in bounds when has_u_bounds).  best_cost_dev
 * (B) / best_u_dev (B,H,m): the best sample over all iterations, reset to +inf / 0 first -- also when iters == 0.
 * costs_dev (iters,B) or NULL: the mean's cost S_{b,0} at every iteration.  sigma_out_dev (B,H,m) or NULL: the last
 * standard deviation (sigma_init when iters == 0).  workspace: workspace_size >= phnn_cem_workspace_bytes.  ref: as in
 * phnn_solve_mppi -- its batch_stride indexes the B*samples ROLLOUTS.
 * Enqueues the clamp and the resets, then iters x (k_sample, K1, k_cem_update); stream-ordered, capturable.  B == 0
 * or iters == 0 returns PHNN_OK after the resets.  PHNN_ERR_INVALID_ARG for samples < 2, elites outside 1 .. samples,
 * alpha outside [0, 1), a negative or non-finite sigma_init / sigma_min, iters < 0, counter fields outside their ranges,
 * NULL required buffers or a too small workspace; PHNN_ERR_UNSUPPORTED for H*m > 256. */
int phnn_solve_cem(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                   const phnn_reference* ref, int32_t integrator, float dt, const phnn_cem_options* opt, void* workspace,
                   size_t workspace_size, float* costs_dev, float* best_cost_dev, float* best_u_dev, float* sigma_out_dev,
                   void* stream);

/* ---- time-correlated (shaped) sampling noise for the MPPI and CEM solves -----------------------------------------
 * A noise shape is a matrix L with rows = H rows and cols = P columns, 1 <= P <= H: float32, row-major, on the device,
 * shared by the whole batch, never written.  For problem b, sample k >= 1, control component c and step t
 *   z[t, c] = sum_{s = 0 .. P-1} L[t, s] * eps[s, c]     float32: acc = 0, then acc = acc + L[t, s] * eps[s, c] for s
 *                                                         ascending, the product rounded, then the sum (no fused
 *                                                         multiply-add)
 *   v[t, c] = clamp(u[t, c] + sigma[t, c] * z[t, c])      sigma: MPPI's table entry sigma[c], or CEM's tensor
 * where eps[s, c] is the white normal the unshaped sampler draws for element s*m + c of a row of length P*m with the
 * same (seed, epoch, iteration, gid = problem_offset + b, k): component (s*m + c) % 4 of the Philox call with counter
 * word 3 = k << 6 | (s*m + c) / 4.  Each normal is drawn once per rollout.  Sample 0 stays the nominal / mean itself
 * (z = 0; L is not read for it).  Shaping acts along time for each control component separately.
 *   - rows = cols = H and L = I returns the values of the unshaped sampler.
 *   - Problem b's samples depend on (seed, epoch, iteration, gid, L) only: not on B, on its position in the batch, on how
 *     the batch is split over calls, or on graph vs eager.
 *   - When L's rows have unit Euclidean norm every z[t, c] has unit variance, and sigma, CEM's refit of it and sigma_min
 *     keep their meaning.  The library does NOT normalise (phnn_mpc_amd/noise.py's builders do).
 * Buffers: L_dev holds exactly rows * cols floats and is only read; it is caller-owned and must stay alive and unchanged
 * until the work enqueued with it has run (a captured graph reads it through this pointer at every replay).  Every
 * other buffer is as documented for the unshaped entry point; the workspace sizes do not change
 * (phnn_mppi_workspace_bytes / phnn_cem_workspace_bytes), and the update entry points are shared.
 * The *_shaped entry points take the arguments of their unshaped counterparts plus `shape`.  shape == NULL is the
 * unshaped call: same launches, same bits.  Else k_shaped_sample replaces k_sample (one group of 16, 32 or 64 lanes per
 * rollout; L staged in LDS when rows * (cols | 1) * 4 bytes <= 48 KiB, read from global memory above that), K1 and the update kernels are
 * launched exactly as in the unshaped solve; stream-ordered, capturable, epoch_dev read by every launch.
 * Every check of the unshaped entry point runs in its order; then PHNN_ERR_INVALID_ARG, with nothing launched, for
 * rows != H, cols < 1, cols > rows or L_dev == NULL (B > 0); PHNN_ERR_UNSUPPORTED for H*m > 256 stays the last check
 * of the options.  DESIGN.md 15. */
typedef struct {
  const float* L_dev;   /* device, (rows, cols) row-major, never written */
  int32_t rows;         /* must equal H */
  int32_t cols;         /* P, 1 <= P <= rows */
  int32_t reserved[4];  /* zero */
} phnn_noise_shape;
int phnn_mppi_sample_shaped(phnn_handle* h, const float* x0_dev, const float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                            const phnn_mppi_options* opt, int32_t iteration, const phnn_noise_shape* shape, float* samples_dev,
                            float* x0_rep_dev, void* stream);
int phnn_cem_sample_shaped(phnn_handle* h, const float* x0_dev, const float* u_dev, const float* sigma_dev, int64_t B, int32_t H,
                           const phnn_cost* cost, const phnn_cem_options* opt, int32_t iteration, const phnn_noise_shape* shape,
                           float* samples_dev, float* x0_rep_dev, void* stream);
int phnn_solve_mppi_shaped(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                           const phnn_reference* ref, int32_t integrator, float dt, const phnn_mppi_options* opt,
                           const phnn_noise_shape* shape, void* workspace, size_t workspace_size, float* costs_dev,
                           float* best_cost_dev, float* best_u_dev, void* stream);
int phnn_solve_cem_shaped(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                          const phnn_reference* ref, int32_t integrator, float dt, const phnn_cem_options* opt,
                          const phnn_noise_shape* shape, void* workspace, size_t workspace_size, float* costs_dev,
                          float* best_cost_dev, float* best_u_dev, float* sigma_out_dev, void* stream);

/* ---- the plant on the other side of the path ------------------------------------------
 * Ground-truth cart-pole of src/cartpole_simulator.py:63-112: float64, explicit Euler, the standard cart-pole
 * equations in the reference's operation order; termination |x| > x_limit or |theta| > theta_limit.  Defaults of
 * the reference: gravity 9.8, masscart 1.0, masspole 0.1, length 0.5 (half-length), dt 0.02, limits 10.0 / 0.5. */
typedef struct {
  double gravity, masscart, masspole, length, dt, x_limit, theta_limit;
} phnn_plant;

/* One plant step for B plants, everything resident on the device (no host round trip in a closed loop):
 *   state_dev (B,4) float64, updated in place;  action: action_dev[b * action_stride] (float32 force; the first
 *   control of rollout b's sequence when action_stride = H*m), clamped to [u_min,u_max] first when has_u_bounds
 *   (src/mpc_controller.py:203-209 returns clamp(u_seq[0])); a NaN force is not clamped: it reaches the state, its
 *   float32 copy and both logs as NaN, and a NaN state never terminates (done_step stays as it is).
 * Optional outputs (NULL = skip): state_f32_dev (B,4) = float32 of the new state (what the next solve consumes:
 * torch.tensor(state, dtype=float32) in scripts/run_cartpole_mpc.py:129); done_step_dev (B) int32, set to the step
 * index the first time a plant terminates (initialise to -1); log_states_dev (T+1,B,4) float64 and
 * log_controls_dev (T,B) float32 receive row step+1 / row step.  The step index is *step_dev when step_dev != NULL
 * (a device counter, so that a captured HIP graph can be replayed), else step_host. */
int phnn_plant_step(phnn_handle* h, const phnn_plant* plant, double* state_dev, const float* action_dev,
                    int64_t action_stride, int64_t B, int32_t has_u_bounds, float u_min, float u_max,
                    float* state_f32_dev, int32_t* done_step_dev, const int32_t* step_dev, int32_t step_host,
                    double* log_states_dev, float* log_controls_dev, void* stream);

/* ---- plant scenarios: per-plant parameters, disturbances, freeze at termination, metrics ------
 * phnn_plant_step_ex is phnn_plant_step with two optional structs; ex == NULL && metrics == NULL IS phnn_plant_step
 * (same kernel, same bits), and a zero-initialised ex with metrics == NULL gives its bits too.  Everything is float64
 * unless stated, without fused multiply-adds.  Per plant b, gid = plant_offset + b:
 *   1. step index, force uf and its clamp: as phnn_plant_step (a NaN command stays NaN; log_controls holds uf).
 *   2. disturbance w, float32: w = force_bias_dev ? force_bias_dev[b] : 0; if force_sigma > 0, w = w + force_sigma * z0
 *      (the product rounded, then the sum).  force = (double)uf + (double)w; with neither a bias nor a sigma nothing is
 *      added at all, force = (double)uf (a -0.0 command stays -0.0).  disturbance_log_dev row `step` receives w.
 *   3. noise: the library's sampling generator (Philox4x32-10, Box-Muller; key = seed).  z0 is component 0 of the call
 *      with counter (gid & 0xffffffff, gid >> 32, step, 1 << 6 | 0), the four measurement normals z_0..z_3 are the four
 *      components of the call with last word 1 << 6 | 1.  CONTRACT: these are the values the white sampler
 *      (phnn_mppi_sample, sigma 1, u 0, no bounds) draws for elements 0 and 4..7 of sample 1 of problem gid at (seed,
 *      epoch = step, iteration = 0).  The noise of plant gid at step s depends on (seed, gid, s) only: not on B, on the
 *      position in the batch, on how a batch is split over calls, or on graph replay vs eager launches.  Use a seed
 *      other than the controller's sampling seed, or the disturbance equals one of the controller's own perturbations.
 *      A call is made only where its sigma is non-zero.
 *   4. parameters: params_dev[4b .. 4b+3] = gravity, masscart, masspole, length when given, else the phnn_plant's; dt
 *      and the limits are always the phnn_plant's.  The dynamics are phnn_plant_step's, operation for operation.
 *   5. freeze_done: a plant whose done_step_dev[b] >= 0 ON ENTRY is not stepped: state_dev keeps its bits, the log_states
 *      row repeats them, log_controls and disturbance_log are still written (the computed w is logged, not applied),
 *      state_f32 is the measurement (6) of the kept state, done_step and the metrics are not touched.
 *   6. measurement: state_f32[i] = (float)x_i, and for every i with meas_sigma[i] > 0 additionally + meas_sigma[i] * z_i
 *      in float32 (product rounded, then the sum).  State, logs and the termination test never see this noise.
 *   7. termination: on the true new state, strict, written once; a NaN state never terminates.
 *   8. metrics (metrics != NULL, plant stepped): e_i = x_i - target[i] on the new state;
 *      c = sum_i sum_j (e_i * Q[4i+j]) * e_j + ((double)uf * R) * (double)uf, i outer, j inner, ascending, added one
 *      by one to an accumulator that starts at 0; cost_acc[b] += c; ok = all_i |e_i| <= tol[i] (false for a NaN);
 *      run[b] = ok ? run[b] + 1 : 0; best_run[b] = max(best_run[b], run[b]).  To count the initial state as
 *      closed_loop.stability_report does, initialise run / best_run to 1 where it is in the band, else 0.
 * Buffer contract as at the top of this file: params_dev, force_bias_dev and action_dev are inputs and are never
 * written; cost_acc_dev, run_dev, best_run_dev accumulate (their contents on entry are data, the caller initialises
 * them), disturbance_log_dev receives one row per call like the other logs.  Stream-ordered and capturable; *step_dev
 * is read by the launch, so a replayed graph draws fresh noise at every control step.
 * PHNN_ERR_INVALID_ARG, nothing launched: what phnn_plant_step refuses, in its order; then a negative or non-finite
 * force_sigma / meas_sigma; plant_offset < 0 or plant_offset + B > 2^48; freeze_done without done_step_dev;
 * disturbance_log_dev with neither step_dev nor step_host >= 0; non-zero reserved; metrics with a NULL array or a
 * negative or NaN tol. */
typedef struct {
  const double* params_dev;     /* (B,4) float64 per plant: gravity, masscart, masspole, length; NULL = the phnn_plant's.
                                   dt, x_limit, theta_limit stay shared */
  const float*  force_bias_dev; /* (B) constant force offset per plant, or NULL */
  float   force_sigma;          /* std of additive Gaussian force noise, >= 0, finite */
  float   meas_sigma[4];        /* std of Gaussian noise on state_f32 only (what the controller sees), >= 0, finite */
  uint64_t seed;                /* noise key; use a seed other than the controller's sampling seed */
  int64_t plant_offset;         /* global id of plant 0: gid = plant_offset + b, 0 <= .., plant_offset + B <= 2^48 */
  int32_t freeze_done;          /* 1: a plant whose done_step is >= 0 ON ENTRY is not stepped any more */
  float*  disturbance_log_dev;  /* (T,B) float32, row `step` receives w_b, or NULL */
  int32_t reserved[4];          /* zero */
} phnn_plant_ex;

typedef struct {
  double Q[16], R, target[4], tol[4]; /* closed-loop stage cost and the stability band, float64 */
  double*  cost_acc_dev;  /* (B) += cost of this step            (caller zeroes)            */
  int32_t* run_dev;       /* (B) current in-band run length      (caller initialises)       */
  int32_t* best_run_dev;  /* (B) longest in-band run so far      (caller initialises)       */
} phnn_plant_metrics;

int phnn_plant_step_ex(phnn_handle* h, const phnn_plant* plant, const phnn_plant_ex* ex, const phnn_plant_metrics* metrics,
                       double* state_dev, const float* action_dev, int64_t action_stride, int64_t B, int32_t has_u_bounds,
                       float u_min, float u_max, float* state_f32_dev, int32_t* done_step_dev, const int32_t* step_dev,
                       int32_t step_host, double* log_states_dev, float* log_controls_dev, void* stream);

/* Warm start of the next solve, src/mpc_controller_canonical.py:252-255: dst[b,t] = src[b,t+1] for t < H-1,
 * dst[b,H-1] = 0 (u (B,H,m), shift by one step).  Also advances *step_dev by one when step_dev != NULL; B == 0 with a
 * step_dev only advances the counter (src_dev / dst_dev may be NULL).  Not an in-place operation: src_dev and dst_dev
 * must not overlap, in whole or in part -- PHNN_ERR_INVALID_ARG, nothing is launched and the counter stays. */
int phnn_shift_controls(phnn_handle* h, const float* src_dev, float* dst_dev, int64_t B, int32_t H, int32_t m,
                        int32_t* step_dev, void* stream);

/* ---- linearisation and time-varying LQR gains ----------------------------------------------------
 * The local model  delta x_{t+1} = A_t delta x_t + B_t delta u_t  of a rollout, and the LQ backward pass on it.
 * All three calls are stream-ordered and capturable, allocate nothing and do not synchronise; B == 0 returns PHNN_OK
 * with nothing launched; H >= 1.  PHNN_ERR_INVALID_ARG, nothing launched and no output touched: NULL required buffers,
 * B < 0, H < 1, an unknown integrator, a non-finite dt, u_min > u_max with has_u_bounds, a negative or non-finite mu, a
 * non-zero reserved.  Buffer contract as at the top of this file: sizes are exact, inputs are never written, outputs
 * are fully written for b < B and nothing else is touched.  For n = 4, A_dev and traj_dev (and x_dev of the point
 * Jacobian) are tensors of state rows and must be 16-byte aligned; Bm_dev, u_dev and the float64 tensors are accessed
 * by element.
 *
 * Point Jacobian: x_dev (B,n), u_dev (B,m) -> A[b,i,j] = d f_i / d x_j, Bm[b,i,k] = d f_i / d u_k at (x_b, u_b).
 * Row i is, bit for bit, what the single-call VJP above returns for the cotangent e_i (one launch instead of n, the
 * inputs not replicated). */
int phnn_model_jacobian(phnn_handle* h, const float* x_dev, const float* u_dev, int64_t B,
                        float* A_dev /* (B,n,n) */, float* Bm_dev /* (B,n,m) */, void* stream);

/* A[b,t] = d x_{t+1} / d x_t, Bm[b,t] = d x_{t+1} / d u_t (unclamped u) of the integrator step K1 takes at
 * (traj[b,t], u[b,t]).  cost: read for has_u_bounds / u_min / u_max only; NULL = no clamp.  With bounds, column k of
 * Bm[b,t] is 0 where u[b,t,k] lies outside [u_min, u_max] or is NaN (the adjoint's mask).
 * traj_dev: the states K1 wrote, (B,H+1,n) (rows 0 .. H-1 are read).  u_dev (B,H,m).
 * Row i is, bit for bit, grad_x0 / grad_u of the general reverse pass above on the one-step rollout from traj[b,t] with
 * traj_bar = (0, e_i) and cost_bar = 0 (the step adjoint of K2 in recompute mode, operation for operation). */
int phnn_rollout_linearize(phnn_handle* h, const float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                           int32_t integrator, float dt, const float* traj_dev,
                           float* A_dev /* (B,H,n,n) */, float* Bm_dev /* (B,H,n,m) */, void* stream);

/* LQ backward pass (Riccati recursion) per problem, float64 without fused multiply-adds, for the stage cost x^T Q x
 * (also at t = H) + u^T R u of `cost` (Q, R only; target, bounds and barrier do not enter):
 *   Lxx = Q + Q^T, Luu = R + R^T (widened first), P_H = Lxx; for t = H-1 .. 0:  S = P A_t, T = P B_t,
 *   Qxx = Lxx + A^T S, Qux = B^T S, Quu = Luu + B^T T + mu I (lower triangle read), Quu = L D L^T without square roots,
 *   X = Quu^-1 Qux, K_t = -X, P_t = Qxx - Qux^T X, symmetrised as 0.5 (P + P^T).
 * Every inner product runs with its index ascending from an accumulator 0, each product rounded, then added;
 * tests/tvlqr_model.py states the remaining order and the kernel equals it bit for bit.  The feedback law is
 * delta u_t = K_t delta x_t.
 * Failure: a pivot d with !(d > 0) or d = +inf.  On the first failure, going backwards, at step t: K_s and P_s for every
 * s <= t (P0 included) are quiet NaN, status[b] = t + 1, the steps after t keep their values; else status[b] = 0.  A NaN
 * in A_t or B_t reaches a pivot one step further down (B_t: the same step) and is reported this way; a NaN in A_0 can
 * only show as NaN in K_0 and P0.  A diverged problem is NaN plus a status, never a finite wrong gain.
 * A_dev (B,H,n,n), Bm_dev (B,H,n,m) float32 -> K_dev (B,H,m,n), P0_dev (B,n,n), status_dev (B) int32 and, when not
 * NULL, P_all_dev (B,H+1,n,n) = P_0 .. P_H. */
typedef struct { double mu; int32_t reserved[4]; } phnn_tvlqr_options;   /* mu >= 0, finite; NULL = {0} */
int phnn_tvlqr(phnn_handle* h, const float* A_dev, const float* Bm_dev, int64_t B, int32_t H,
               const phnn_cost* cost, const phnn_tvlqr_options* opt,
               double* K_dev /* (B,H,m,n) */, double* P0_dev /* (B,n,n) */,
               double* P_all_dev /* (B,H+1,n,n) or NULL */, int32_t* status_dev /* (B) */, void* stream);

/* ---- batched Gauss-Newton solve on the linearisation and the LQ pass --------------------------------
 * Projected Gauss-Newton shooting with Levenberg-Marquardt regularisation and a parallel backtracking line search, per
 * problem b of B independent ones.  State: the iterate u_b (H,m), kept inside the cost's bounds, its cost_b and
 * trajectory traj_b (H+1,n), and mu_b (float64).  Set-up: u <- clamp(u) when has_u_bounds (a NaN stays NaN),
 * mu_b <- mu_init, accepts_b <- 0, one K1 gives cost_b and traj_b.  Then `iters` times, five launches:
 *   1 linearise   phnn_rollout_linearize(u, traj) -> A (B,H,n,n), Bm (B,H,n,m), with the cost's bounds
 *   2 direction   k_gn_direction<n,m>: float64, no fused multiply-adds, one thread per problem, (n, m) in {2,3,4} x
 *                 {1,2,3,4}.  With e_t = x_t - r_t (r: x_target or the reference row) and act_t,i = 1 where the barrier
 *                 of component i is active at x_t (x_min_i - x > 0 or x - x_max_i > 0):
 *                   Lxx_t = (Q+Q^T) + diag(2 w act_t),  lx_t = (Q+Q^T) e_t - 2w (x_min - x) [below] + 2w (x - x_max) [above],
 *                   lu_t = (R+R^T) u_t,  Luu = R+R^T;   P_H = Lxx_H, p_H = lx_H;  for t = H-1 .. 0:
 *                   S, T, Qxx (with Lxx_t), Qux, Quu = Luu + B^T T + mu_b I and its L D L^T exactly as phnn_tvlqr forms them,
 *                   qx = lx_t + A^T p, qu = lu_t + B^T p, X = Quu^-1 Qux, d = Quu^-1 qu (the same factors), K_t = -X,
 *                   k_t = -d, P_t as in phnn_tvlqr (symmetrised), p_t = qx - Qux^T d, dV_b += qu^T d;
 *                 then forward on the linear model: dx_0 = 0, du_t = k_t + K_t dx_t, dx_{t+1} = A_t dx_t + B_t du_t.
 *                 -> du (B,H,m) float32 (the float64 value rounded once), dV (B) float64 (>= 0 in exact arithmetic; the
 *                 predicted change of the cost at step length 1 is -dV/2 and its slope at 0 is -dV), status (B) int32
 *                 with phnn_tvlqr's rule: t + 1 at the first pivot with !(d > 0) or +inf, else 0.  Where status != 0, or
 *                 dV_b or an element of du_b is not finite, du_b is all zeros and dV_b quiet NaN: never a finite wrong
 *                 step.  u is read as given (the solve keeps it in bounds).  tests/gn_model.py states the order.
 *   3 candidates  k_gn_candidates: v_{b,j} = clamp(u_b + alpha_j du_b), alpha_j = 2^-j, j = 0 .. L-1 (float32, the product
 *                 rounded, then the sum; the library's NaN-preserving clamp) -> cand (B*L,H,m), row b*L + j; and x0
 *                 replicated -> x0_rep (B*L,n)
 *   4 evaluate    ONE K1 launch over the B*L candidates with their trajectories (no K2, no stash)
 *   5 select      k_gn_select: j* = the lowest finite candidate cost (as floats, lowest j on ties).  Accept iff
 *                 status_b == 0 and S_{b,j*} < cost_b (strict): u_b, traj_b, cost_b take candidate j*'s row, trajectory
 *                 and cost, mu_b <- max(mu_min, mu_b mu_down), accepts_b += 1.  Else u_b, traj_b, cost_b keep their bits
 *                 and mu_b <- min(mu_max, mu_b mu_up).  costs_row[b] = cost_b BEFORE the update, alpha_row[b] =
 *                 alpha_{j*} or 0 on reject.
 * cost_b is therefore non-increasing bit for bit; a diverged problem shows as NaN or status plus rejections.  Not part
 * of this solve: a closed-loop forward pass inside K1 (true iLQR), a box-QP at the bounds (a control on a bound that is
 * pushed outwards loses that component to the clamp and the line search decides; phnn_solve_gn_ex with PHNN_GN_BOX, below,
 * is the solve with it), early termination per problem.
 * All calls are stream-ordered and capturable, allocate nothing and do not synchronise; inputs are never written. */
typedef struct {
  int32_t iters;      /* >= 0 */
  int32_t line_steps; /* L, 1 .. 32 */
  double mu_init;     /* the mu fields: >= 0 and finite, mu_min <= mu_max */
  double mu_min;
  double mu_max;
  double mu_up;       /* >= 1, finite */
  double mu_down;     /* in (0, 1] */
  int32_t reserved[4]; /* zero */
} phnn_gn_options;
/* Bytes of the workspace of phnn_solve_gn: A, Bm, traj_b, du, dV, status, the direction's scratch, the candidates,
 * their x0, costs and trajectories, each region 256-byte aligned.  0 for invalid arguments (B < 0, H < 1, L outside
 * 1 .. 32, a model without a direction kernel); non-decreasing in B, H and line_steps. */
size_t phnn_gn_workspace_bytes(const phnn_handle* h, int64_t B, int32_t H, int32_t line_steps);
/* The three kernels, as phnn_mppi_sample / phnn_mppi_update stand next to their solve.  B == 0: PHNN_OK, nothing
 * launched.  ref: NULL = the cost's x_target, else problem b's reference (batch_stride indexes PROBLEMS here).
 * scratch_dev: B*H*(m*n + m) float64, private layout.  mu_dev (B) float64 is read only. */
int phnn_gn_direction(phnn_handle* h, const float* A_dev, const float* Bm_dev, const float* traj_dev, const float* u_dev,
                      int64_t B, int32_t H, const phnn_cost* cost, const phnn_reference* ref, const double* mu_dev,
                      float* du_dev /* (B,H,m) */, double* dV_dev /* (B) */, int32_t* status_dev /* (B) */,
                      double* scratch_dev, void* stream);
int phnn_gn_candidates(phnn_handle* h, const float* x0_dev, const float* u_dev, const float* du_dev, int64_t B, int32_t H,
                       const phnn_cost* cost, int32_t line_steps, float* cand_dev /* (B*L,H,m) */,
                       float* x0_rep_dev /* (B*L,n) or NULL */, void* stream);
/* In place on u_dev (B,H,m), traj_dev (B,H+1,n), cost_dev (B), mu_dev (B) float64, accepts_dev (B) int32 from the
 * candidates cand_dev (B*L,H,m), their K1 costs cand_cost_dev (B*L) and trajectories cand_traj_dev (B*L,H+1,n) and the
 * direction's status_dev (B); costs_row_dev (B) / alpha_row_dev (B) float32 or NULL.  opt: line_steps and the mu fields
 * are read (iters and mu_init are checked like the rest). */
int phnn_gn_select(phnn_handle* h, float* u_dev, float* traj_dev, float* cost_dev, double* mu_dev, int32_t* accepts_dev,
                   const float* cand_dev, const float* cand_cost_dev, const float* cand_traj_dev, const int32_t* status_dev,
                   int64_t B, int32_t H, const phnn_gn_options* opt, float* costs_row_dev, float* alpha_row_dev, void* stream);
/* The whole solve.  u_dev (B,H,m): in = initial iterate, out = the last one (in bounds).  cost_out (B) float32: its
 * cost; mu_out (B) float64: the last mu; accepts_dev (B) int32: accepted iterations -- all three required, they are the
 * solve's state and are defined after the set-up also when iters == 0.  costs_dev (iters,B) or NULL: the cost of the
 * iterate at the START of every iteration; alpha_hist_dev (iters,B) float32 or NULL: the accepted step length, 0 on
 * reject.  workspace: workspace_size >= phnn_gn_workspace_bytes, required when B > 0.  ref: as in phnn_solve_mppi -- its
 * batch_stride indexes the B*L ROLLOUTS (rollout b*L + j belongs to problem b); the set-up K1 and the direction address
 * problem b as rollout b*L, i.e. with stride batch_stride * L; offset_dev is read by every launch, the direction
 * included.  B == 0: PHNN_OK, nothing launched.  PHNN_ERR_INVALID_ARG, nothing launched: NULL required buffers, a too
 * small workspace, line_steps outside 1 .. 32, iters < 0, a non-finite or negative mu field, mu_min > mu_max, mu_up < 1,
 * mu_down outside (0, 1], non-zero reserved, B < 0, H < 1, the reference checks of phnn_solve_mppi;
 * PHNN_ERR_UNSUPPORTED: no direction kernel for the model's (n, m). */
int phnn_solve_gn(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                  const phnn_reference* ref, int32_t integrator, float dt, const phnn_gn_options* opt, void* workspace,
                  size_t workspace_size, float* cost_out, float* costs_dev, double* mu_out, int32_t* accepts_dev,
                  float* alpha_hist_dev, void* stream);

/* ---- box-constrained LQ step for the Gauss-Newton solve ------------------------------------------------
 * Control-limited DDP (Tassa, Mansard, Todorov 2014) on the Gauss-Newton model of the solve above: launch 2 with the
 * cost's control bounds inside the LQ step instead of only in the candidates' clamp.  k_gn_direction_box<n,m>, float64,
 * no fused multiply-adds, one thread per problem, the same (n, m) and the same scratch as k_gn_direction.  Step t of the
 * backward sweep:
 *   lx, lu, S, T, Qxx, Qux, Quu = Luu + B^T T + mu_b I, its L D L^T, qx, qu and the pivot rule: exactly phnn_gn_direction's.
 *   lo_i = (double)u_min - (double)u_t,i, hi_i = (double)u_max - (double)u_t,i (without has_u_bounds: -inf, +inf).  A nominal
 *   with !(lo_i <= 0 <= hi_i) -- a NaN control with bounds is one -- fails like a pivot: status = t + 1.
 *   d = Quu^-1 qu.  Where no component has -d_i < lo_i or -d_i > hi_i the step is phnn_gn_direction's, operation for
 *   operation (K = -X, k = -d, P = Qxx - Qux^T X, p = qx - Qux^T d, dV += qu^T d).  Otherwise the box-QP
 *   min 1/2 x^T Quu x + qu^T x, lo <= x <= hi, is solved by enumerating the active sets in the order of their codes
 *   c = 1 .. 3^m - 1 (digit i of c in base 3: 0 free, 1 at lo_i, 2 at hi_i): the free block is solved with the same
 *   L D L^T routine (on Quu with the fixed rows and columns replaced by the identity), the right-hand side corrected for
 *   the fixed components; the first code with lo <= x_free <= hi and g = qu + Quu x >= 0 at lo, <= 0 at hi is taken; if
 *   none passes (borderline rounding) the step fails like a pivot and the solve raises mu.  Then k_t = x, the rows of K_t
 *   are -(Quu_FF)^-1 Qux_F for the free and 0 for the fixed components, and the value function takes the general form
 *     P_t = Qxx + K^T Quu K + K^T Qux + Qux^T K (symmetrised),  p_t = qx + K^T Quu k + K^T qu + Qux^T k,
 *     dV_b += -(2 qu^T k + k^T Quu k)        (= qu^T d when nothing is fixed; the predicted change stays -dV/2).
 * Forward: dx_0 = 0, du_t = min(max(k_t + K_t dx_t, lo), hi), dx_{t+1} = A_t dx_t + B_t du_t; du is rounded once to float32,
 * so u + du lies inside the bounds up to that one rounding (the candidates' clamp stays).  Failure (status != 0, dV or a
 * du element not finite): du_b = 0, dV_b = quiet NaN as in phnn_gn_direction, nclamp_b = 0.  nclamp (B) int32: the
 * (t, component) pairs the backward sweep held on a bound.  Where nothing is clamped in either sweep every output equals
 * phnn_gn_direction's bit for bit.  tests/gn_box_model.py states every operation in its order.
 * Arguments, checks (in the same order) and scratch size: phnn_gn_direction's; nclamp_dev may be NULL. */
int phnn_gn_direction_box(phnn_handle* h, const float* A_dev, const float* Bm_dev, const float* traj_dev, const float* u_dev,
                          int64_t B, int32_t H, const phnn_cost* cost, const phnn_reference* ref, const double* mu_dev,
                          float* du_dev /* (B,H,m) */, double* dV_dev /* (B) */, int32_t* status_dev /* (B) */,
                          int32_t* nclamp_dev /* (B) int32 or NULL */, double* scratch_dev, void* stream);
#define PHNN_GN_BOX 1 /* flags of phnn_solve_gn_ex: launch 2 of every iteration is phnn_gn_direction_box */
/* phnn_solve_gn with flags.  flags == 0 and nclamp_hist_dev == NULL: phnn_solve_gn itself, the same launches and the
 * same bits.  PHNN_GN_BOX: the direction of every iteration is phnn_gn_direction_box; linearise, candidates, K1 and
 * select are unchanged.  nclamp_hist_dev (iters,B) int32 or NULL: row `it` is the direction's nclamp, written by the
 * kernel itself (the workspace, and phnn_gn_workspace_bytes, are those of phnn_solve_gn).  PHNN_ERR_INVALID_ARG, nothing
 * launched: unknown flag bits, nclamp_hist_dev without PHNN_GN_BOX, and whatever phnn_solve_gn refuses.  Stream-ordered
 * and capturable; the reference conventions are phnn_solve_gn's. */
int phnn_solve_gn_ex(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                     const phnn_reference* ref, int32_t integrator, float dt, const phnn_gn_options* opt, void* workspace,
                     size_t workspace_size, float* cost_out, float* costs_dev, double* mu_out, int32_t* accepts_dev,
                     float* alpha_hist_dev, int32_t flags, int32_t* nclamp_hist_dev /* (iters,B) or NULL */, void* stream);

/* ---- batched extended Kalman filter on the learned model --------------------------------------------------
 * The estimator between a noisy or partial measurement and the solve, per problem b of B independent ones.  The
 * measurement is a selection of state components: bit i of meas_mask set means component i is measured, p = popcount,
 * 0 <= p <= n.  k_ekf_update<n>, n in {2, 3, 4}: one thread per problem, float64, no fused multiply-adds, every inner
 * product with its index ascending from an accumulator 0, each product rounded, then added; tests/ekf_model.py states the
 * remaining order and the kernel equals it bit for bit.  With x- the predicted state (float32, widened), A the Jacobian
 * of the prediction step (float32, widened), P the covariance (float64, in/out), y the measurement row (float32; ONLY
 * the measured components are read):
 *   predict     M = A P,  P- = M A^T + Qn,  symmetrised as 0.5 (P- + P-^T)
 *   innovation  nu_a = (double)y[i_a] - (double)x-[i_a] over the measured components i_a;  S = P-[idx, idx] with Rn[i_a]
 *               added on the diagonal;  S = L D L^T without square roots, with phnn_tvlqr's pivot rule (a pivot d with
 *               !(d > 0) or d = +inf is a failure)
 *   gain        K = P-[:, idx] S^-1 by column solves with those factors
 *   state       xhat_i = (double)x-_i + sum_a K[i][a] nu_a, rounded once to float32
 *   covariance  Joseph form: G = I - K C,  P = G P- G^T + K diag(Rn[idx]) K^T,  symmetrised
 *   nis         sum_a nu_a (S^-1 nu)_a   (chi-square with p degrees of freedom for a consistent filter)
 * status (B) int32 and the special cases:
 *   0  updated; or p = 0: no update, xhat = x- as floats, P = P-, nis = quiet NaN
 *   1  a measured component of y is not finite (a dropped measurement): no update, as for p = 0
 *   2  a pivot failure, or an x- or A that is not finite: xhat and P are all quiet NaN, nis too -- never a finite wrong
 *      estimate
 * Qn (n x n, row-major in the leading n*n entries) is read as given; Rn[i] is read for measured components only.
 * Optional outputs (NULL = skip): nis_dev (B) float64; innov_dev (B,n) float64, 0 at unmeasured components; and through
 * a phnn_ekf_log one row each of log_xhat_dev (T+1,B,n) float32 at row step + 1 and log_nis_dev (T,B) float64 at row
 * step, the step index being *step_dev when step_dev != NULL (a device counter, so that a captured graph can be
 * replayed), else step_host -- as in the plant step.
 * All calls are stream-ordered and capturable, allocate nothing and do not synchronise; B == 0 returns PHNN_OK with
 * nothing launched; sizes are exact and inputs are never written.  For n = 4 the float32 state rows (xhat, y, x-) are
 * 16-byte aligned and A follows the rule of the linearisation above.
 * PHNN_ERR_INVALID_ARG, nothing launched and no output touched: NULL required buffers, B < 0, mask bits at or above n, a
 * non-finite Qn entry, a non-positive or non-finite Rn at a measured component, non-zero reserved, a log without a step
 * source (step_dev == NULL and step_host < 0), and for the step an unknown integrator, a non-finite dt or u_min > u_max;
 * PHNN_ERR_UNSUPPORTED for n outside {2, 3, 4}. */
typedef struct {
  uint32_t meas_mask;                  /* bit i: component i is measured */
  double Qn[PHNN_MAX_N * PHNN_MAX_N];  /* process noise covariance, (n,n) row-major in the leading entries, finite */
  double Rn[PHNN_MAX_N];               /* measurement noise variances, > 0 and finite where measured */
  int32_t reserved[4];                 /* zero */
} phnn_ekf_options;
typedef struct {
  float* log_xhat_dev;      /* (T+1,B,n) float32, row step + 1 receives xhat, or NULL */
  double* log_nis_dev;      /* (T,B) float64, row step receives nis, or NULL */
  const int32_t* step_dev;  /* device step counter, or NULL */
  int32_t step_host;        /* used when step_dev == NULL */
} phnn_ekf_log;
/* Bytes of the workspace of the step below: the control row (B,1,m), K1's trajectory (B,2,n) and cost (B), A (B,n,n)
 * and Bm (B,n,m), each region 256-byte aligned.  0 for invalid arguments (B < 0, n outside {2, 3, 4}). */
size_t phnn_ekf_workspace_bytes(const phnn_handle* h, int64_t B);
/* The kernel on its own; A and x- may come from anywhere.  Problem b's prediction is xpred_dev[b * xpred_stride + i] (so
 * that row 1 of a (B,2,n) trajectory is read in place with stride 2n) and its measurement y_dev[b * y_stride + i].
 * A_dev (B,n,n), P_dev (B,n,n) float64 in/out, xhat_dev (B,n), status_dev (B) int32; nis_dev, innov_dev, log may be
 * NULL. */
int phnn_ekf_update(phnn_handle* h, const float* xpred_dev, int64_t xpred_stride, const float* A_dev, const float* y_dev,
                    int64_t y_stride, int64_t B, const phnn_ekf_options* opt, double* P_dev, float* xhat_dev, double* nis_dev,
                    double* innov_dev, int32_t* status_dev, const phnn_ekf_log* log, void* stream);
/* One filter step through the learned model: xhat_dev (B,n) and P_dev (B,n,n) in/out.  u_dev[b * u_stride + k], k < m,
 * is the control applied during the step (stride H*m: the first control of a solve's sequence, in place); cost is read
 * for has_u_bounds / u_min / u_max only, NULL = no clamp -- the clamp of the control is K1's and the plant's.  Four
 * launches in stream order: k_ekf_controls (the control row), K1 with H = 1 from xhat on the path of the forward
 * rollout above (its trajectory into the workspace), the linearisation above with H = 1, k_ekf_update on row 1 of that
 * trajectory.  workspace_dev: the bytes of the size query above, required when B > 0. */
int phnn_ekf_step(phnn_handle* h, float* xhat_dev, double* P_dev, const float* u_dev, int64_t u_stride, const float* y_dev,
                  int64_t y_stride, int64_t B, const phnn_cost* cost, int32_t integrator, float dt,
                  const phnn_ekf_options* opt, double* nis_dev, double* innov_dev, int32_t* status_dev,
                  const phnn_ekf_log* log, void* workspace_dev, void* stream);

/* ---- tracking the plan between two solves with its TV-LQR feedback ---------------------------------------
 * A loop that solves every k-th control step applies, in between, row j of the last plan plus the time-varying LQR
 * feedback around it:  u = clamp(clamp(u_j) + K_j (x - x_j^nominal)),  j = step % k.  phnn_feedback_plan makes the
 * nominal trajectory and the gains of a plan, phnn_feedback_control applies the law, per problem b of B independent ones.
 * k_feedback_control<n,m>, (n, m) in {2,3,4} x {1,2,3,4}: one thread per problem, float64, no fused multiply-adds;
 * tests/feedback_model.py states the order and the kernel equals it bit for bit.  With clampf the library's
 * NaN-preserving float32 clamp, applied only when the cost has bounds:
 *   un_k = clampf(u[b,j,k])
 *   dx_i = (double)x[b,i] - (double)traj[b,j,i]
 *   s_k  = sum_i K[b,j,k,i] dx_i        index ascending from an accumulator 0.0, each product rounded, then added
 *   v_k  = clampf((float)((double)un_k + s_k)), the sum rounded once to float32; where s_k == 0.0 the output keeps un_k's
 *          bits (a -0.0 included): at j = 0, where x is the state the plan started from, the control is the plan's
 * status (B) int32 and the special cases:
 *   0  u_out[b,k] = v_k
 *   1  an entry of K[b,j] is not finite (the rows phnn_tvlqr marked): u_out[b,k] = un_k
 *   2  a dx_i is not finite (a NaN estimate or a NaN nominal row): u_out[b,k] = un_k, dev = quiet NaN
 * -- open-loop tracking of the plan, never a finite control built from a NaN.  dev (B) float64 = max_i |dx_i|.
 * Both calls are stream-ordered and capturable, allocate nothing, do not synchronise and never write their inputs;
 * B == 0 returns PHNN_OK with nothing launched; sizes are exact. */
/* Bytes of the workspace of phnn_feedback_plan: A (B,H,n,n) and Bm (B,H,n,m) float32, K1's cost vector (B) float32 and
 * P0 (B,n,n) float64, each region 256-byte aligned.  0 for invalid arguments (B < 0, H < 1) or a model whose (n, m) has
 * no TV-LQR kernel; non-decreasing in B and H. */
size_t phnn_feedback_workspace_bytes(const phnn_handle* h, int64_t B, int32_t H);
/* The plan's nominal trajectory and gains.  Exactly three launches in stream order and nothing else: K1 from x0 with
 * trajectories on phnn_rollout_fwd's path (the caller's cost, so the control clamp is K1's), phnn_rollout_linearize's
 * launch on that trajectory with the cost's bounds, phnn_tvlqr's launch (opt NULL = {0}).  traj_dev (B,H+1,n) float32,
 * K_dev (B,H,m,n) float64 and status_dev (B) int32 are bit for bit what those three public calls give when issued by
 * hand.  Reference rows enter neither A, B nor K, so the call takes none.  PHNN_ERR_INVALID_ARG, nothing launched and
 * no output touched: NULL required buffers (cost included), B < 0, H < 1, an unknown integrator, a non-finite dt,
 * u_min > u_max, a negative or non-finite mu, non-zero reserved, workspace_size below the size query;
 * PHNN_ERR_UNSUPPORTED for an (n, m) without a TV-LQR kernel. */
int phnn_feedback_plan(phnn_handle* h, const float* x0_dev /* (B,n) */, const float* u_dev /* (B,H,m) */, int64_t B, int32_t H,
                       const phnn_cost* cost, int32_t integrator, float dt, const phnn_tvlqr_options* opt, void* workspace,
                       size_t workspace_size, float* traj_dev /* (B,H+1,n) */, double* K_dev /* (B,H,m,n) */,
                       int32_t* status_dev /* (B) */, void* stream);
/* The law above, one launch.  The plan row is j = step % solve_every with step = *step_dev when step_dev != NULL (a
 * device counter >= 0, so that ONE captured launch serves every tracking step), else step_host; 1 <= solve_every <= H,
 * so j is always a row of the plan.  cost is read for has_u_bounds / u_min / u_max only, NULL = no clamp.  x_dev (B,n)
 * float32, u_dev (B,H,m), traj_dev and K_dev as phnn_feedback_plan wrote them, u_out (B,m) float32; status_out (B) int32
 * and dev_out (B) float64 may be NULL; log_status_dev (T,B) int32 and log_dev_dev (T,B) float64 (NULL = skip) receive
 * row `step`, as the plant step's logs do.  PHNN_ERR_INVALID_ARG, nothing launched and no output touched: NULL required
 * buffers, B < 0, H < 1, solve_every outside 1 .. H, neither step_dev nor step_host >= 0, u_min > u_max;
 * PHNN_ERR_UNSUPPORTED for an (n, m) without a kernel. */
int phnn_feedback_control(phnn_handle* h, const float* x_dev, const float* u_dev, const float* traj_dev, const double* K_dev,
                          int64_t B, int32_t H, const phnn_cost* cost, int32_t solve_every, const int32_t* step_dev,
                          int32_t step_host, float* u_out, int32_t* status_out, double* dev_out, int32_t* log_status_dev,
                          double* log_dev_dev, void* stream);

/* ---- terminal cost and its LQR weight for the Adam and Gauss-Newton solves -------------------------------
 * Every solve above weights the last state like every other one.  A terminal weight adds, per rollout b,
 *   cost_b += e_H^T W e_H,   e_H = x_H - r_{b,row(H)},
 * with row(H) exactly K1's rule min(offset + H, rows - 1) -- the device offset when the reference has one -- and the
 * cost's x_target without a reference.  W is n x n float32, row-major, on the device, never written: ONE matrix for the
 * batch (batch_stride 0) or one per problem; row i of a batch uses the W of problem i / group, so group is 1 for a plain
 * batch and L for the L line-search candidates per problem of the Gauss-Newton solve.  The usual W is the cost-to-go of
 * the infinite-horizon LQR of the model linearised at the target, which phnn_dare computes.  A NULL phnn_terminal means
 * no terminal term: the entry points below then issue the launches of their plain counterparts and return their bits.
 * L-BFGS, MPPI and CEM take no terminal weight; the TV-LQR of phnn_feedback_plan stays on the stage cost. */
typedef struct {
  const float* W_dev;   /* device, (n,n) row-major per problem */
  int64_t batch_stride; /* floats between problems; 0 = one W shared by all */
  int32_t group;        /* rows per problem, >= 1 */
} phnn_terminal;

/* k_terminal_cost<n>, n in {2, 3, 4}: one thread per rollout, float32, behind the K1 launch that wrote traj_dev (B,H+1,n)
 * and cost_dev (B).  Operation order (tests/terminal_model.py; the kernel equals it bit for bit), the fused
 * multiply-adds below being the only ones:
 *   e_i = x_H,i - r_i                         formed as the stage cost forms it
 *   s_j = fma(e_i, W[i][j], s_j)              i ascending, from 0
 *   c   = fma(s_j, e_j, c)                    j ascending, from 0
 *   cost_dev[b] = cost_dev[b] + c
 *   traj_bar_dev[b,H,i] = g_i, g_i = fma(W[i][j] + W[j][i], e_j, g_i)   j ascending from 0, the sum of the two weights
 *                                             rounded once in float32 -- only when traj_bar_dev != NULL
 * Rows t < H of traj_bar_dev (B,H+1,n) are never written: the caller zeroes them once, and phnn_rollout_vjp with that
 * cotangent returns the gradient of the total cost.  A NaN state gives a NaN cost and a NaN row.  ref: NULL = the cost's
 * x_target, else K1's reference (batch_stride indexes the B rows).  B == 0: PHNN_OK, nothing launched.
 * PHNN_ERR_INVALID_ARG, nothing launched: NULL handle, cost or term, B < 0, H < 1, W_dev == NULL (B > 0), group < 1, a
 * negative batch_stride, NULL traj_dev / cost_dev (B > 0), the reference checks of phnn_rollout_fwd_ref;
 * PHNN_ERR_UNSUPPORTED for n outside {2, 3, 4}. */
int phnn_terminal_cost(phnn_handle* h, const float* traj_dev, int64_t B, int32_t H, const phnn_cost* cost,
                       const phnn_reference* ref, const phnn_terminal* term, float* cost_dev, float* traj_bar_dev,
                       void* stream);

/* k_dare<n,m>, the (n, m) of phnn_tvlqr: one thread per problem, float64, no fused multiply-adds.  The Riccati step of
 * phnn_tvlqr -- ONE device function both kernels call, operation order in tests/tvlqr_model.py -- with the constant
 * A_dev (B,n,n), Bm_dev (B,n,m) float32 of problem b, from P_0 = Lxx = Q + Q^T:  step k = 1, 2, ... gives P_k and the
 * gain K_k = -X_k, so after N steps the kernel holds what phnn_tvlqr returns as P0 and K[0] on N copies of (A, B), bit
 * for bit.  After each step d = max |P_k - P_{k-1}| and s = max |P_k| over the entries:
 *   status 1  a pivot failure, or an s that is NaN or +inf, or a W entry that is not finite: P, K, W all quiet NaN
 *   status 0  d <= tol * s: converged
 *   status 2  k == max_iters: the outputs are the last iterate
 * Outputs: P_dev (B,n,n) float64 = P_k (in the cost's units the cost-to-go of a deviation e is e^T (P/2) e), K_dev
 * (B,m,n) float64, W_dev (B,n,n) float32 = (float)(0.5 * (P_k - Lxx)) -- the stage cost already charges Q at t = H --,
 * iters_dev (B) int32 = k, status_dev (B) int32.  mu >= 0 is added to the diagonal of Quu as in phnn_tvlqr.
 * opt NULL = {200000, 1e-12, 0}: untrained models of this family need some 62 000 steps at tol 1e-12.
 * PHNN_ERR_INVALID_ARG, nothing launched: NULL handle or cost, B < 0, max_iters < 1, a negative or non-finite tol or mu,
 * non-zero reserved, NULL tensors (B > 0); PHNN_ERR_UNSUPPORTED for an (n, m) without a TV-LQR kernel. */
typedef struct {
  int32_t max_iters;   /* >= 1 */
  double tol;          /* >= 0, finite; relative to max |P| */
  double mu;           /* >= 0, finite */
  int32_t reserved[4]; /* zero */
} phnn_dare_options;
int phnn_dare(phnn_handle* h, const float* A_dev, const float* Bm_dev, int64_t B, const phnn_cost* cost,
              const phnn_dare_options* opt, double* P_dev, double* K_dev, float* W_dev, int32_t* iters_dev,
              int32_t* status_dev, void* stream);

/* The Gauss-Newton direction with a terminal weight: phnn_gn_direction (flags 0) or phnn_gn_direction_box (PHNN_GN_BOX;
 * nclamp_dev as there, NULL without the flag) with the backward sweep started from
 *   Tf[i][j] = (double)W[i][j] + (double)W[j][i],   P_H = Lxx_H + Tf,
 *   p_H[i] = lx_H[i] + sum_k Tf[i][k] e_k           k ascending from 0.0, each product rounded, then added,
 * e = (double)x_H - (double)r_H, W the matrix of problem b / group.  term == NULL: those additions are not executed at
 * all and the call is the plain one, bit for bit.  Checks: the plain call's, then the terminal's of phnn_terminal_cost. */
int phnn_gn_direction_term(phnn_handle* h, const float* A_dev, const float* Bm_dev, const float* traj_dev, const float* u_dev,
                           int64_t B, int32_t H, const phnn_cost* cost, const phnn_reference* ref, const phnn_terminal* term,
                           const double* mu_dev, float* du_dev /* (B,H,m) */, double* dV_dev /* (B) */,
                           int32_t* status_dev /* (B) */, int32_t flags, int32_t* nclamp_dev /* (B) or NULL */,
                           double* scratch_dev, void* stream);

/* phnn_solve / phnn_solve_ref with an optional terminal weight: ref may be NULL and term may be NULL in the same call.
 * Per iteration: K1 -> k_terminal_cost (cost and row H of traj_bar_dev) -> K2 with that cotangent -> K3, so the cost
 * history and the best-iterate tracking see the total cost.  traj_bar_dev (B,H+1,n): caller-owned scratch, required
 * with a terminal weight (B > 0, iters > 0); the call zeroes it once, before the first iteration.  term == NULL:
 * traj_bar_dev is not touched and the launches and bits are phnn_solve's / phnn_solve_ref's.  term->group applies to the
 * B rows (1 for a plain batch). */
int phnn_solve_term(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                    const phnn_reference* ref, const phnn_terminal* term, int32_t integrator, float dt,
                    const phnn_solve_options* opt, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_dev,
                    float* cost_dev, float* traj_dev, void* workspace_dev, float* costs_dev, float* best_cost_dev,
                    float* best_u_dev, float* traj_bar_dev, void* stream);

/* phnn_solve_gn_ex with an optional terminal weight.  The set-up K1 and the candidates' K1 are each followed by
 * k_terminal_cost (cost only; the candidates with group * L rows per W), the direction of every iteration takes the
 * terminal as phnn_gn_direction_term does, k_gn_select is unchanged: it compares total costs.  term->batch_stride and
 * term->group index the B PROBLEMS (group 1: problem b uses W_dev + b * batch_stride).  The workspace is
 * phnn_solve_gn's (phnn_gn_workspace_bytes; the terminal needs none of its own).  term == NULL: phnn_solve_gn_ex
 * itself, the same launches and the same bits. */
int phnn_solve_gn_term(phnn_handle* h, const float* x0_dev, float* u_dev, int64_t B, int32_t H, const phnn_cost* cost,
                       const phnn_reference* ref, const phnn_terminal* term, int32_t integrator, float dt,
                       const phnn_gn_options* opt, void* workspace, size_t workspace_size, float* cost_out, float* costs_dev,
                       double* mu_out, int32_t* accepts_dev, float* alpha_hist_dev, int32_t flags,
                       int32_t* nclamp_hist_dev /* (iters,B) or NULL */, void* stream);

/* ---- input-disturbance estimation and offset-free control ------------------------------------------------
 * The filter above on the augmented state z = (x in R^n, d in R^m), nz = n + m, with the model x+ = F(x, c(u) + d),
 * d+ = d: d is an input disturbance that enters where the control enters, F is K1's integrator step WITHOUT a control
 * clamp, and c is the library's float32 clamp to the cost's bounds (a NaN stays NaN), applied to the command only.  The
 * measurement is a selection of STATE components (bit i of meas_mask, i < n).  xhat (B,n) and dhat (B,m) are float32,
 * Pz (B,nz,nz) is float64, in/out.  The Jacobian of the augmented step is A_z = [[A, Bm], [0, I]] with A (B,n,n) and
 * Bm (B,n,m) the float32 outputs of the linearisation of that step taken with no bounds (cost = NULL), so that Bm is
 * d x+ / d d with no clamp mask.  k_dekf_update<n, m>, (n, m) in {(2,1), (3,1), (4,1), (4,2)}: one thread per problem,
 * the operations of k_ekf_update above at size nz on the prediction (x-, dhat), A_z (read from A and Bm, never
 * assembled in memory, its d rows the exact constants 0 and 1), Qz and Rn, with the rows of S of every unmeasured
 * component -- all of d included -- held as the identity; (xhat, dhat) are rounded once to float32.
 * tests/dekf_model.py states it around tests/ekf_model.py's update and the kernel equals it bit for bit.  With the d
 * rows and columns of Pz and Qz zero the x part equals phnn_ekf_update's bit for bit, dhat keeps its bits and the d
 * rows of Pz stay exactly 0.
 * status (B) int32 and the special cases are the filter's above:
 *   0  updated; or nothing measured: xhat = x- and dhat keep their float bits, Pz = Pz-, nis = quiet NaN
 *   1  a dropped measurement: no update, as for nothing measured
 *   2  a pivot failure, or an x-, dhat, A or Bm that is not finite: xhat, dhat, Pz and nis all quiet NaN
 * Two small kernels go with it: k_dekf_controls, row[b,k] = c(u[b * u_stride + k]) + dhat[b,k], and k_dist_compensate,
 * u_cmd[b,k] = c(c(v[b * v_stride + k]) - dhat[b,k]), both float32 with the sum / difference rounded once.
 * Conventions as above: stream-ordered, capturable, no allocation, no synchronisation; B == 0 returns PHNN_OK with
 * nothing launched; sizes are exact and inputs are never written.  PHNN_ERR_INVALID_ARG, nothing launched and no output
 * touched: NULL required buffers, B < 0, mask bits at or above n, a non-finite Qz entry, a non-positive or non-finite
 * Rn at a measured component, non-zero reserved, a log without a step source, and for the step an unknown integrator,
 * a non-finite dt or u_min > u_max; PHNN_ERR_UNSUPPORTED for an (n, m) without a kernel ((4,3), (4,4), n outside
 * {2, 3, 4}). */
#define PHNN_DEKF_MAX_Z 6 /* largest n + m with a k_dekf_update */
typedef struct {
  uint32_t meas_mask;    /* bit i < n: state component i is measured */
  double Qz[36];         /* process noise covariance of (x, d), (nz,nz) row-major in the leading entries, finite */
  double Rn[PHNN_MAX_N]; /* measurement noise variances, > 0 and finite where measured */
  int32_t reserved[4];   /* zero */
} phnn_dekf_options;
typedef struct {
  float* log_xhat_dev;      /* (T+1,B,n) float32, row step + 1 receives xhat, or NULL */
  double* log_nis_dev;      /* (T,B) float64, row step receives nis, or NULL */
  const int32_t* step_dev;  /* device step counter, or NULL */
  int32_t step_host;        /* used when step_dev == NULL */
  float* log_dhat_dev;      /* (T+1,B,m) float32, row step + 1 receives dhat, or NULL */
} phnn_dekf_log;
/* Bytes of the workspace of the step below: the control row (B,1,m), K1's trajectory (B,2,n) and cost (B), A (B,n,n)
 * and Bm (B,n,m), each region 256-byte aligned.  0 for invalid arguments (B < 0, an (n, m) without a kernel). */
size_t phnn_dekf_workspace_bytes(const phnn_handle* h, int64_t B);
/* The kernel on its own; x-, A and Bm may come from anywhere.  Problem b's prediction is xpred_dev[b * xpred_stride + i]
 * and its measurement y_dev[b * y_stride + i], i < n.  A_dev (B,n,n), Bm_dev (B,n,m), Pz_dev (B,nz,nz) float64 in/out,
 * xhat_dev (B,n), dhat_dev (B,m) in/out (the predicted disturbance is the one held), status_dev (B) int32; nis_dev (B),
 * innov_dev (B,n) and log may be NULL. */
int phnn_dekf_update(phnn_handle* h, const float* xpred_dev, int64_t xpred_stride, const float* A_dev, const float* Bm_dev,
                     const float* y_dev, int64_t y_stride, int64_t B, const phnn_dekf_options* opt, double* Pz_dev,
                     float* xhat_dev, float* dhat_dev, double* nis_dev, double* innov_dev, int32_t* status_dev,
                     const phnn_dekf_log* log, void* stream);
/* One filter step through the learned model: xhat_dev (B,n), dhat_dev (B,m) and Pz_dev (B,nz,nz) in/out.
 * u_dev[b * u_stride + k], k < m, is the command applied during the step; cost is read for has_u_bounds / u_min /
 * u_max only and clamps the COMMAND only, NULL = no clamp.  Four launches in stream order and nothing else:
 * k_dekf_controls (the control row c(u) + dhat), K1 with H = 1 from xhat on the path of the forward rollout above with a
 * zero cost and no bounds (its trajectory into the workspace), the linearisation above with H = 1 and cost = NULL,
 * k_dekf_update on row 1 of that trajectory.  workspace_dev: the bytes of the size query above, required when B > 0. */
int phnn_dekf_step(phnn_handle* h, float* xhat_dev, float* dhat_dev, double* Pz_dev, const float* u_dev, int64_t u_stride,
                   const float* y_dev, int64_t y_stride, int64_t B, const phnn_cost* cost, int32_t integrator, float dt,
                   const phnn_dekf_options* opt, double* nis_dev, double* innov_dev, int32_t* status_dev,
                   const phnn_dekf_log* log, void* workspace_dev, void* stream);
/* The compensated command u_cmd_dev (B,m): c(c(v) - dhat) per component, v_dev[b * v_stride + k] the controller's
 * command (stride H*m: the first control of a solve's sequence, in place), cost read for its bounds as above (NULL: no
 * clamp).  Where dhat[b,k] is not finite the component is c(v) and status_dev[b] (B, int32, may be NULL) is 1, else 0:
 * never a finite command built from a NaN estimate.  A NaN v stays NaN.  One launch.  Any m the handle has. */
int phnn_dist_compensate(phnn_handle* h, const float* v_dev, int64_t v_stride, const float* dhat_dev, int64_t B,
                         const phnn_cost* cost, float* u_cmd_dev, int32_t* status_dev, void* stream);

/* ---- batched unscented Kalman filter -----------------------------------------------------------------------
 * The filter of phnn_ekf_* without a Jacobian: per problem the S = 2 n + 1 sigma points of (xhat, P) go through the real
 * integrator step -- its activations and its control clamp included -- as B * S rollouts of K1 with H = 1, and the
 * prediction is the weighted mean and covariance of their images.  n in {2, 3, 4}; xhat (B,n) float32, P (B,n,n) float64.
 * The caller computes the weights of the scaled unscented transform in float64 and passes them; the library never sees
 * alpha, beta or kappa:  lambda = alpha^2 (n + kappa) - n,  gamma = sqrt(n + lambda),  wm0 = lambda / (n + lambda),
 * wc0 = wm0 + (1 - alpha^2 + beta),  wi = 1 / (2 (n + lambda)).  (alpha, beta, kappa) = (1, 0, 1) is the default of the
 * Python layer: the sigma points are float32, and a small alpha sinks their spread into the rounding of xhat.
 * Float64, no fused multiply-adds, sums in ascending index order (tests/ukf_model.py states both kernels):
 *   k_ukf_sigma<n>    P = L L^T by columns from the LOWER triangle of P: d_j = P[j][j] - L[j][0]^2 - ..., L[j][j] =
 *                     sqrt(d_j), L[i][j] = (P[i][j] - L[i][0] L[j][0] - ...) / L[j][j];  chi_0 = xhat (its own bits),
 *                     chi_{1+c} = (float)(xhat + gamma L[:,c]),  chi_{1+n+c} = (float)(xhat - gamma L[:,c]), the product
 *                     first, then the sum, one rounding.  A pivot with !(d > 0) or d = +inf, or an xhat that is not
 *                     finite: every chi of the problem is a quiet NaN (K1 keeps it NaN, the update below reports status
 *                     2).  P must be positive definite; an exactly singular P is such a failure.  The control rows
 *                     (B,S,1,m) are u[b * u_stride + k] for every sigma point of problem b, unclamped: the clamp is K1's.
 *   k_ukf_moments<n>  Y_k the image of sigma point k, widened:  x-_i = wm0 Y_0i + wi Y_1i + ... + wi Y_{S-1,i};
 *                     e_k = Y_k - x- (the float64 mean);  Pm[i][j] = Pm[j][i] = wc0 (e_0i e_0j) + sum_{k>=1} wi (e_ki e_kj)
 *                     (i <= j; the product of the deviations rounded first, then the weight times it, then the sum);
 *                     xm = (float)x-.  It also writes the float32 identity (B,n,n).
 *   then k_ekf_update above on (xm, A = that identity, P = Pm): it adds Qn, symmetrises, and updates with the measured
 *   components; nis, innov, status, the dropped measurement and the empty mask are phnn_ekf_update's.
 * Conventions as above: stream-ordered, capturable, no allocation, no synchronisation; B == 0 returns PHNN_OK with
 * nothing launched; sizes are exact and inputs are never written.  PHNN_ERR_INVALID_ARG, nothing launched and no output
 * touched: the refusals of phnn_ekf_step, and a gamma or wi that is not finite and positive, a wm0 or wc0 that is not
 * finite; PHNN_ERR_UNSUPPORTED for n outside {2, 3, 4}. */
#define PHNN_UKF_MAX_N 4 /* largest n with a k_ukf_sigma / k_ukf_moments */
typedef struct {
  uint32_t meas_mask;              /* bit i < n: state component i is measured */
  double Qn[PHNN_UKF_MAX_N * PHNN_UKF_MAX_N]; /* additive process noise covariance, (n,n) row-major in the leading entries, finite */
  double Rn[PHNN_UKF_MAX_N];       /* measurement noise variances, > 0 and finite where measured */
  double gamma;                    /* sqrt(n + lambda): the spread of the sigma points, > 0 and finite */
  double wm0;                      /* weight of sigma point 0 in the mean, finite */
  double wc0;                      /* weight of sigma point 0 in the covariance, finite */
  double wi;                       /* weight of every other sigma point, > 0 and finite */
  int32_t reserved[4];             /* zero */
} phnn_ukf_options;
/* Bytes of the workspace of the step below: the sigma points (B,S,n), their control rows (B,S,1,m), K1's trajectory
 * (B*S,2,n) and cost (B*S), xm (B,n) and the identity (B,n,n), each region 256-byte aligned.  0 for invalid arguments
 * (B < 0, n outside {2, 3, 4}). */
size_t phnn_ukf_workspace_bytes(const phnn_handle* h, int64_t B);
/* k_ukf_sigma on its own: chi_dev (B,S,n) float32 and, when ctrl_dev is given, the control rows ctrl_dev (B,S,1,m) from
 * u_dev[b * u_stride + k] (ctrl_dev == NULL: u_dev is not read and may be NULL).  Of opt, gamma is used. */
int phnn_ukf_sigma(phnn_handle* h, const float* xhat_dev, const double* P_dev, const float* u_dev, int64_t u_stride,
                   int64_t B, const phnn_ukf_options* opt, float* chi_dev, float* ctrl_dev, void* stream);
/* k_ukf_moments on its own: image k of problem b is Y_dev[(b * S + k) * Y_stride + i], i < n (Y_stride = 2 n and
 * Y_dev = traj + n read row 1 of a (B*S,2,n) trajectory in place).  xm_dev (B,n) float32, Pm_dev (B,n,n) float64,
 * eye_dev (B,n,n) float32 or NULL.  Of opt, wm0, wc0 and wi are used. */
int phnn_ukf_moments(phnn_handle* h, const float* Y_dev, int64_t Y_stride, int64_t B, const phnn_ukf_options* opt,
                     float* xm_dev, double* Pm_dev, float* eye_dev, void* stream);
/* One filter step through the learned model: xhat_dev (B,n) and P_dev (B,n,n) in/out; u, y, cost, integrator, dt, nis,
 * innov, status and log as in phnn_ekf_step (cost is read for has_u_bounds / u_min / u_max only, NULL = no clamp).  Four
 * launches in stream order and nothing else: k_ukf_sigma, K1 with H = 1 on the B * S sigma points on the path of the
 * forward rollout above (its trajectory into the workspace), k_ukf_moments on row 1 of that trajectory (Pm into P_dev),
 * k_ekf_update with the identity.  workspace_dev: the bytes of the size query above, required when B > 0. */
int phnn_ukf_step(phnn_handle* h, float* xhat_dev, double* P_dev, const float* u_dev, int64_t u_stride, const float* y_dev,
                  int64_t y_stride, int64_t B, const phnn_cost* cost, int32_t integrator, float dt,
                  const phnn_ukf_options* opt, double* nis_dev, double* innov_dev, int32_t* status_dev,
                  const phnn_ekf_log* log, void* workspace_dev, void* stream);

/* Introspection for tests: copies the packed weight image the kernels stage into LDS (phnn_kernels.hip.h layouts; a
 * device-resident private format) to image_host after the work queued on `stream`, and waits for the copy.
 * *image_floats (may be NULL) receives its size; image_host == NULL only queries the size. */
int phnn_read_image(phnn_handle* h, float* image_host, size_t n_floats, size_t* image_floats, void* stream);

/* Introspection for benches/tests: name of the kernel variant selected for this handle, rollouts per
 * workgroup, LDS bytes staged per workgroup. */
int phnn_kernel_info(const phnn_handle* h, int32_t integrator, int32_t* rollouts_per_wg,
                     int32_t* lds_bytes, int32_t* n_workgroups_for_B, int64_t B);

/* Name of the kernel variant serving this handle, e.g. "phnn<n=4,hid=128,fixedG,f16x2>".  The hidden x hidden
 * products run as all-f32 MFMAs ("f32"), as an exact 3-way bf16 split ("bf16x3") or 2-way f16 split ("f16x2",
 * default for 128-wide models) on the matrix pipe; phnn_options.matmul_mode selects one at phnn_create_ex time. */
const char* phnn_variant_name(const phnn_handle* h);

/* Library version (major*10000 + minor*100 + patch). */
int phnn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PHNN_MPC_H */
