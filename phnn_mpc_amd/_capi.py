"""ctypes view of include/phnn_mpc.h: the structs, and the loader of the HIP shared library.

The product path has no CPU fallback: if libphnn_mpc.so is missing or a symbol is absent the import of the
engine raises, loudly.
"""
import ctypes as C
import os

PHNN_MAX_N = 8
PHNN_MAX_M = 4
PHNN_MAX_LAYERS = 4

MODEL_PHNN, MODEL_CANONICAL, MODEL_ODEFUNC = 0, 1, 2
INTEG_EULER, INTEG_RK4 = 0, 1
INTEGRATORS = {"euler": INTEG_EULER, "rk4": INTEG_RK4}

ACT_TANH, ACT_OTHER, ACT_SILU, ACT_RELU, ACT_ELU, ACT_GELU = 0, 1, 2, 3, 4, 5
ACTIVATIONS = {"tanh": ACT_TANH, "silu": ACT_SILU, "relu": ACT_RELU, "elu": ACT_ELU, "gelu": ACT_GELU}  # activations with kernels (others: ACT_OTHER, refused)
MASS_CARTPOLE, MASS_CONSTANT, MASS_DIAGONAL, MASS_FULL = 0, 1, 2, 3
WGRAD_ACCUMULATE, WGRAD_TAPES = 1, 2  # flags of phnn_rollout_wgrad / phnn_model_wgrad (include/phnn_mpc.h)
MATMUL_MODES = {"default": 0, "f32": 1, "bf16x3": 2, "f16x2": 3}
SPLIT_MODES = {"auto": 0, "never": 1, "always": 2}

_HERE = os.path.dirname(os.path.abspath(__file__))
# PHNN_LIB_PATH: load another build of the library (A/B comparisons, tools/ab_bench.sh) without touching the product file
LIB_PATH = os.environ.get("PHNN_LIB_PATH") or os.path.join(_HERE, "csrc", "libphnn_mpc.so")

# every symbol include/phnn_mpc.h declares
EXPORTED = [
    "phnn_create", "phnn_create_ex", "phnn_update_weights", "phnn_update_weights_dev", "phnn_read_image", "phnn_destroy", "phnn_last_error", "phnn_weight_count", "phnn_model_forward",
    "phnn_model_vjp", "phnn_rollout_fwd", "phnn_workspace_bytes", "phnn_rollout_grad", "phnn_rollout_vjp",
    "phnn_rollout_trajectory", "phnn_rollout_trajectory_ws", "phnn_wgrad_workspace_bytes", "phnn_wgrad_record_info", "phnn_rollout_wgrad", "phnn_model_wgrad",
    "phnn_adam_step", "phnn_solve", "phnn_plant_step", "phnn_shift_controls", "phnn_kernel_info", "phnn_variant_name",
    "phnn_version", "phnn_rollout_fwd_ref", "phnn_rollout_grad_ref", "phnn_solve_ref", "phnn_lbfgs_workspace_bytes",
    "phnn_solve_lbfgs", "phnn_mppi_workspace_bytes", "phnn_mppi_sample", "phnn_mppi_update", "phnn_solve_mppi",
    "phnn_cem_workspace_bytes", "phnn_cem_sample", "phnn_cem_update", "phnn_solve_cem",
    "phnn_mppi_sample_shaped", "phnn_cem_sample_shaped", "phnn_solve_mppi_shaped", "phnn_solve_cem_shaped",
    "phnn_plant_step_ex", "phnn_model_jacobian", "phnn_rollout_linearize", "phnn_tvlqr",
    "phnn_gn_workspace_bytes", "phnn_gn_direction", "phnn_gn_candidates", "phnn_gn_select", "phnn_solve_gn",
    "phnn_gn_direction_box", "phnn_solve_gn_ex",
    "phnn_ekf_workspace_bytes", "phnn_ekf_update", "phnn_ekf_step",
    "phnn_dekf_workspace_bytes", "phnn_dekf_update", "phnn_dekf_step", "phnn_dist_compensate",
    "phnn_ukf_workspace_bytes", "phnn_ukf_sigma", "phnn_ukf_moments", "phnn_ukf_step",
    "phnn_feedback_workspace_bytes", "phnn_feedback_plan", "phnn_feedback_control",
    "phnn_rollout_vjp_ref", "phnn_terminal_cost", "phnn_dare", "phnn_gn_direction_term", "phnn_solve_term",
    "phnn_solve_gn_term",
]

PHNN_GN_BOX = 1  # flags of phnn_solve_gn_ex


class MlpShape(C.Structure):
    _fields_ = [("depth", C.c_int32), ("hidden", C.c_int32 * PHNN_MAX_LAYERS)]

    @classmethod
    def of(cls, hidden):
        hidden = list(hidden)
        if len(hidden) > PHNN_MAX_LAYERS:
            raise ValueError(f"at most {PHNN_MAX_LAYERS} hidden layers are supported, got {len(hidden)}")
        s = cls()
        s.depth = len(hidden)
        for i, h in enumerate(hidden):
            s.hidden[i] = int(h)
        return s


class Desc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("fixed_G", C.c_int32),
                ("h_net", MlpShape), ("r_net", MlpShape), ("g_net", MlpShape), ("activation", C.c_int32),
                ("mass_type", C.c_int32), ("m_net", MlpShape)]


class SolveOptions(C.Structure):
    """phnn_solve_options"""
    _fields_ = [("iters", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("track_best", C.c_int32)]


class LbfgsOptions(C.Structure):
    """phnn_lbfgs_options: torch.optim.LBFGS(lr, max_iter, max_eval, tolerance_grad, tolerance_change, history_size)
    stepped outer_steps times; max_eval 0 = torch's default max_iter * 5 // 4."""
    _fields_ = [("outer_steps", C.c_int32), ("max_iter", C.c_int32), ("max_eval", C.c_int32), ("history_size", C.c_int32),
                ("lr", C.c_double), ("tolerance_grad", C.c_double), ("tolerance_change", C.c_double),
                ("reserved", C.c_int32 * 4)]


class MppiOptions(C.Structure):
    """phnn_mppi_options: K = samples perturbations of the nominal per iteration (sample 0 is the nominal), noise
    sigma per control component, softmin temperature lambda; Philox counter fields seed / problem_offset / epoch."""
    _fields_ = [("iters", C.c_int32), ("samples", C.c_int32), ("lambda", C.c_float), ("sigma", C.c_float * PHNN_MAX_M),
                ("seed", C.c_uint64), ("problem_offset", C.c_int64), ("epoch_dev", C.c_void_p), ("epoch_host", C.c_int32),
                ("reserved", C.c_int32 * 4)]  # 'lambda' is a Python keyword: setattr(opt, "lambda", v)


class CemOptions(C.Structure):
    """phnn_cem_options: K = samples perturbations of the mean per iteration (sample 0 is the mean), refit of mean and
    per-element standard deviation to the `elites` lowest-cost samples with smoothing alpha, initial sigma per control
    component and its floor sigma_min; Philox counter fields seed / problem_offset / epoch as in MppiOptions."""
    _fields_ = [("iters", C.c_int32), ("samples", C.c_int32), ("elites", C.c_int32), ("alpha", C.c_float),
                ("sigma_init", C.c_float * PHNN_MAX_M), ("sigma_min", C.c_float), ("seed", C.c_uint64),
                ("problem_offset", C.c_int64), ("epoch_dev", C.c_void_p), ("epoch_host", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class NoiseShape(C.Structure):
    """phnn_noise_shape: the (rows = H, cols = P) float32 row-major device matrix L that turns the white normals of a
    sampling solve into time-correlated ones, z[t, c] = sum_s L[t, s] eps[s, c] (phnn_mpc_amd/noise.py builds them)."""
    _fields_ = [("L_dev", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32 * 4)]


class TvlqrOptions(C.Structure):
    """phnn_tvlqr_options: mu >= 0 is added to the diagonal of Quu (a Levenberg-Marquardt style regularisation)."""
    _fields_ = [("mu", C.c_double), ("reserved", C.c_int32 * 4)]


class GnOptions(C.Structure):
    """phnn_gn_options: iters Gauss-Newton iterations with line_steps = L candidates u + 2^-j du each; mu is the
    Levenberg-Marquardt term on Quu: started at mu_init, times mu_down (floor mu_min) after an accepted iteration, times
    mu_up (cap mu_max) after a rejected one."""
    _fields_ = [("iters", C.c_int32), ("line_steps", C.c_int32), ("mu_init", C.c_double), ("mu_min", C.c_double),
                ("mu_max", C.c_double), ("mu_up", C.c_double), ("mu_down", C.c_double), ("reserved", C.c_int32 * 4)]


class Terminal(C.Structure):
    """phnn_terminal: row i of a batch adds e_H^T W e_H with W = W_dev + (i // group) * batch_stride, (n,n) row-major."""
    _fields_ = [("W_dev", C.c_void_p), ("batch_stride", C.c_int64), ("group", C.c_int32)]


class DareOptions(C.Structure):
    """phnn_dare_options: at most max_iters Riccati steps, stopped where max|P_k - P_{k-1}| <= tol * max|P_k|; mu >= 0
    on the diagonal of Quu."""
    _fields_ = [("max_iters", C.c_int32), ("tol", C.c_double), ("mu", C.c_double), ("reserved", C.c_int32 * 4)]


class EkfOptions(C.Structure):
    """phnn_ekf_options: bit i of meas_mask set = state component i is measured; Qn (n,n) row-major process noise
    covariance in the leading entries; Rn the measurement noise variances (read where measured)."""
    _fields_ = [("meas_mask", C.c_uint32), ("Qn", C.c_double * (PHNN_MAX_N * PHNN_MAX_N)), ("Rn", C.c_double * PHNN_MAX_N),
                ("reserved", C.c_int32 * 4)]


PHNN_DEKF_MAX_Z = 6  # largest n + m with a k_dekf_update


class DekfOptions(C.Structure):
    """phnn_dekf_options: bit i < n of meas_mask set = state component i is measured; Qz (nz,nz) row-major process noise
    covariance of (x, d) in the leading entries; Rn the measurement noise variances (read where measured)."""
    _fields_ = [("meas_mask", C.c_uint32), ("Qz", C.c_double * (PHNN_DEKF_MAX_Z * PHNN_DEKF_MAX_Z)), ("Rn", C.c_double * PHNN_MAX_N),
                ("reserved", C.c_int32 * 4)]


class DekfLog(C.Structure):
    """phnn_dekf_log: phnn_ekf_log's fields, then log_dhat (T+1,B,m) float32, row step + 1."""
    _fields_ = [("log_xhat_dev", C.c_void_p), ("log_nis_dev", C.c_void_p), ("step_dev", C.c_void_p), ("step_host", C.c_int32),
                ("log_dhat_dev", C.c_void_p)]


PHNN_UKF_MAX_N = 4  # largest n with a k_ukf_sigma / k_ukf_moments


class UkfOptions(C.Structure):
    """phnn_ukf_options: meas_mask, Qn and Rn as in EkfOptions (at most 4 state components); gamma = sqrt(n + lambda) the
    spread of the sigma points, wm0 / wc0 the weights of sigma point 0 in the mean / the covariance, wi the weight of
    every other one -- computed by the caller in float64 (estimation.UKF.options)."""
    _fields_ = [("meas_mask", C.c_uint32), ("Qn", C.c_double * (PHNN_UKF_MAX_N * PHNN_UKF_MAX_N)), ("Rn", C.c_double * PHNN_UKF_MAX_N),
                ("gamma", C.c_double), ("wm0", C.c_double), ("wc0", C.c_double), ("wi", C.c_double), ("reserved", C.c_int32 * 4)]


class EkfLog(C.Structure):
    """phnn_ekf_log: row step + 1 of log_xhat (T+1,B,n) float32 and row step of log_nis (T,B) float64; the step is
    *step_dev (device int32) when given, else step_host."""
    _fields_ = [("log_xhat_dev", C.c_void_p), ("log_nis_dev", C.c_void_p), ("step_dev", C.c_void_p), ("step_host", C.c_int32)]


class Plant(C.Structure):
    """phnn_plant: the reference's cart-pole constants (src/cartpole_simulator.py:26-36, 107-110)."""
    _fields_ = [("gravity", C.c_double), ("masscart", C.c_double), ("masspole", C.c_double), ("length", C.c_double),
                ("dt", C.c_double), ("x_limit", C.c_double), ("theta_limit", C.c_double)]

    @classmethod
    def default(cls, dt=0.02):
        return cls(9.8, 1.0, 0.1, 0.5, float(dt), 10.0, 0.5)


class PlantEx(C.Structure):
    """phnn_plant_ex: per-plant parameters (B,4) float64, force bias (B) float32, force / measurement noise, the noise
    counter fields seed / plant_offset, freeze at termination, and the disturbance log (T,B) float32."""
    _fields_ = [("params_dev", C.c_void_p), ("force_bias_dev", C.c_void_p), ("force_sigma", C.c_float),
                ("meas_sigma", C.c_float * 4), ("seed", C.c_uint64), ("plant_offset", C.c_int64), ("freeze_done", C.c_int32),
                ("disturbance_log_dev", C.c_void_p), ("reserved", C.c_int32 * 4)]


class PlantMetrics(C.Structure):
    """phnn_plant_metrics: the closed-loop stage cost (Q row-major, R), the stability band (target, tol) and the three
    accumulating device arrays: cost (B) float64, current and longest in-band run (B) int32."""
    _fields_ = [("Q", C.c_double * 16), ("R", C.c_double), ("target", C.c_double * 4), ("tol", C.c_double * 4),
                ("cost_acc_dev", C.c_void_p), ("run_dev", C.c_void_p), ("best_run_dev", C.c_void_p)]


class Options(C.Structure):
    _fields_ = [("matmul_mode", C.c_int32), ("force_matmul", C.c_int32), ("max_waves", C.c_int32),
                ("split_tiles", C.c_int32), ("reserved", C.c_int32 * 4)]


class Cost(C.Structure):
    _fields_ = [("Q", C.c_float * (PHNN_MAX_N * PHNN_MAX_N)), ("R", C.c_float * (PHNN_MAX_M * PHNN_MAX_M)),
                ("x_target", C.c_float * PHNN_MAX_N), ("u_min", C.c_float), ("u_max", C.c_float),
                ("has_u_bounds", C.c_int32), ("x_min", C.c_float * PHNN_MAX_N), ("x_max", C.c_float * PHNN_MAX_N),
                ("has_x_min", C.c_int32), ("has_x_max", C.c_int32), ("barrier_weight", C.c_float)]


class Reference(C.Structure):
    """phnn_reference: problem b tracks x_ref[b * batch_stride + min(offset + t, rows - 1) * time_stride + i]."""
    _fields_ = [("x_ref", C.c_void_p), ("batch_stride", C.c_int64), ("time_stride", C.c_int64), ("rows", C.c_int32),
                ("offset_dev", C.c_void_p), ("offset_host", C.c_int32)]


def make_cost(n, m, Q, R, x_target=None, u_min=None, u_max=None, x_min=None, x_max=None, barrier_weight=1000.0):
    """Fill a phnn_cost.  Q: (n,n) matrix or length-n diagonal; R: (m,m) matrix, length-m diagonal or scalar."""
    import numpy as np

    c = Cost()
    Q = np.asarray(Q, dtype=np.float64)
    if Q.ndim == 1:
        Q = np.diag(Q)
    if Q.shape != (n, n):
        raise ValueError(f"Q must be ({n},{n}) or ({n},), got {Q.shape}")
    R = np.asarray(R, dtype=np.float64)
    if R.ndim == 0:
        R = np.eye(m) * float(R)
    elif R.ndim == 1:
        R = np.diag(R)
    if R.shape != (m, m):
        raise ValueError(f"R must be ({m},{m}), ({m},) or scalar, got {R.shape}")
    for i in range(n):
        for j in range(n):
            c.Q[i * n + j] = Q[i, j]
    for i in range(m):
        for j in range(m):
            c.R[i * m + j] = R[i, j]
    xt = np.zeros(n) if x_target is None else np.asarray(x_target, dtype=np.float64).reshape(n)
    for i in range(n):
        c.x_target[i] = xt[i]
    if (u_min is None) != (u_max is None):
        # the reference only clamps when both bounds are given (src/mpc_controller.py:180-183)
        u_min = u_max = None
    c.has_u_bounds = int(u_min is not None)
    c.u_min = float(u_min) if u_min is not None else 0.0
    c.u_max = float(u_max) if u_max is not None else 0.0
    c.has_x_min = int(x_min is not None)
    c.has_x_max = int(x_max is not None)
    if x_min is not None:
        for i, v in enumerate(np.asarray(x_min, dtype=np.float64).reshape(n)):
            c.x_min[i] = v
    if x_max is not None:
        for i, v in enumerate(np.asarray(x_max, dtype=np.float64).reshape(n)):
            c.x_max[i] = v
    c.barrier_weight = float(barrier_weight)
    return c


_lib = None


def load_library():
    """Load csrc/libphnn_mpc.so and declare the signatures of include/phnn_mpc.h.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C phnn_mpc_amd/csrc`). "
            "There is no CPU fallback for the rollout engine.")
    # torch first: it brings its own HIP runtime (same soname as the system one the library is linked against);
    # the runtime that is loaded first serves both, and only torch's matches the rest of torch's ROCm libraries.
    # Loading this library before torch leaves the process with a mixed set and no visible device.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, f32p, i64, i32 = C.c_void_p, C.c_void_p, C.c_int64, C.c_int32
    lib.phnn_create.argtypes = [C.POINTER(Desc), C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(vp)]
    lib.phnn_create.restype = C.c_int
    lib.phnn_create_ex.argtypes = [C.POINTER(Desc), C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(Options),
                                   C.POINTER(vp)]
    lib.phnn_create_ex.restype = C.c_int
    lib.phnn_update_weights.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, vp]
    lib.phnn_update_weights.restype = C.c_int
    lib.phnn_update_weights_dev.argtypes = [vp, f32p, C.c_size_t, vp]
    lib.phnn_update_weights_dev.restype = C.c_int
    lib.phnn_read_image.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_size_t), vp]
    lib.phnn_read_image.restype = C.c_int
    lib.phnn_destroy.argtypes = [vp]
    lib.phnn_destroy.restype = C.c_int
    lib.phnn_last_error.argtypes = [vp]
    lib.phnn_last_error.restype = C.c_char_p
    lib.phnn_weight_count.argtypes = [C.POINTER(Desc)]
    lib.phnn_weight_count.restype = C.c_size_t
    lib.phnn_model_forward.argtypes = [vp, f32p, f32p, i64, f32p, f32p, vp]
    lib.phnn_model_forward.restype = C.c_int
    lib.phnn_model_vjp.argtypes = [vp, f32p, f32p, f32p, i64, f32p, f32p, vp]
    lib.phnn_model_vjp.restype = C.c_int
    lib.phnn_model_jacobian.argtypes = [vp, f32p, f32p, i64, f32p, f32p, vp]
    lib.phnn_model_jacobian.restype = C.c_int
    lib.phnn_rollout_linearize.argtypes = [vp, f32p, i64, i32, C.POINTER(Cost), i32, C.c_float, f32p, f32p, f32p, vp]
    lib.phnn_rollout_linearize.restype = C.c_int
    lib.phnn_tvlqr.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(TvlqrOptions), vp, vp, vp, vp, vp]
    lib.phnn_tvlqr.restype = C.c_int
    lib.phnn_rollout_fwd.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), i32, C.c_float, f32p, f32p, vp, vp]
    lib.phnn_rollout_fwd.restype = C.c_int
    lib.phnn_workspace_bytes.argtypes = [vp, i64, i32, i32]
    lib.phnn_workspace_bytes.restype = C.c_size_t
    lib.phnn_rollout_grad.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), i32, C.c_float, f32p, vp, f32p, f32p,
                                      vp]
    lib.phnn_rollout_grad.restype = C.c_int
    lib.phnn_rollout_vjp.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), i32, C.c_float, f32p, vp, f32p, f32p,
                                     f32p, f32p, vp]
    lib.phnn_rollout_vjp.restype = C.c_int
    lib.phnn_rollout_trajectory.argtypes = [vp, f32p, f32p, i64, i32, i32, C.c_float, f32p, f32p, vp]
    lib.phnn_rollout_trajectory.restype = C.c_int
    lib.phnn_rollout_trajectory_ws.argtypes = [vp, f32p, f32p, i64, i32, i32, C.c_float, f32p, f32p, vp, vp]
    lib.phnn_rollout_trajectory_ws.restype = C.c_int
    lib.phnn_wgrad_record_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.phnn_wgrad_record_info.restype = C.c_int
    lib.phnn_wgrad_workspace_bytes.argtypes = [vp, i64, i32, i32]
    lib.phnn_wgrad_workspace_bytes.restype = C.c_size_t
    lib.phnn_rollout_wgrad.argtypes = [vp, f32p, f32p, i64, i32, i32, C.c_float, f32p, f32p, f32p, vp, f32p, i32, f32p,
                                       f32p, vp]
    lib.phnn_rollout_wgrad.restype = C.c_int
    lib.phnn_model_wgrad.argtypes = [vp, f32p, f32p, f32p, f32p, i64, vp, f32p, i32, f32p, f32p, vp]
    lib.phnn_model_wgrad.restype = C.c_int
    lib.phnn_adam_step.argtypes = [vp, f32p, f32p, f32p, f32p, i64, C.c_float, C.c_float, C.c_float, C.c_float, i32,
                                   f32p, f32p, f32p, i64, C.c_float, C.c_float, i32, vp]
    lib.phnn_adam_step.restype = C.c_int
    lib.phnn_solve.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), i32, C.c_float, C.POINTER(SolveOptions), f32p, f32p,
                               f32p, f32p, f32p, vp, f32p, f32p, f32p, vp]
    lib.phnn_solve.restype = C.c_int
    lib.phnn_rollout_fwd_ref.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float,
                                         f32p, f32p, vp, vp]
    lib.phnn_rollout_fwd_ref.restype = C.c_int
    lib.phnn_rollout_grad_ref.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float,
                                          f32p, vp, f32p, f32p, vp]
    lib.phnn_rollout_grad_ref.restype = C.c_int
    lib.phnn_solve_ref.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float,
                                   C.POINTER(SolveOptions), f32p, f32p, f32p, f32p, f32p, vp, f32p, f32p, f32p, vp]
    lib.phnn_solve_ref.restype = C.c_int
    lib.phnn_lbfgs_workspace_bytes.argtypes = [vp, i64, i32, i32]
    lib.phnn_lbfgs_workspace_bytes.restype = C.c_size_t
    lib.phnn_solve_lbfgs.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float,
                                     C.POINTER(LbfgsOptions), f32p, f32p, f32p, vp, vp, C.c_size_t, f32p, vp, vp, vp]
    lib.phnn_solve_lbfgs.restype = C.c_int
    lib.phnn_mppi_workspace_bytes.argtypes = [vp, i64, i32, i32]
    lib.phnn_mppi_workspace_bytes.restype = C.c_size_t
    lib.phnn_mppi_sample.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(MppiOptions), i32, f32p, f32p, vp]
    lib.phnn_mppi_sample.restype = C.c_int
    lib.phnn_mppi_update.argtypes = [vp, f32p, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(MppiOptions), f32p, f32p, f32p,
                                     vp]
    lib.phnn_mppi_update.restype = C.c_int
    lib.phnn_solve_mppi.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float,
                                    C.POINTER(MppiOptions), vp, C.c_size_t, f32p, f32p, f32p, vp]
    lib.phnn_solve_mppi.restype = C.c_int
    lib.phnn_cem_workspace_bytes.argtypes = [vp, i64, i32, i32]
    lib.phnn_cem_workspace_bytes.restype = C.c_size_t
    lib.phnn_cem_sample.argtypes = [vp, f32p, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(CemOptions), i32, f32p, f32p, vp]
    lib.phnn_cem_sample.restype = C.c_int
    lib.phnn_cem_update.argtypes = [vp, f32p, f32p, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(CemOptions), f32p, f32p,
                                    f32p, vp]
    lib.phnn_cem_update.restype = C.c_int
    lib.phnn_solve_cem.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float,
                                   C.POINTER(CemOptions), vp, C.c_size_t, f32p, f32p, f32p, f32p, vp]
    lib.phnn_solve_cem.restype = C.c_int
    # the *_shaped entry points: the unshaped argument lists with a phnn_noise_shape* after `iteration` / `opt`
    shp = C.POINTER(NoiseShape)
    for name, at in (("mppi_sample", 8), ("cem_sample", 9), ("solve_mppi", 10), ("solve_cem", 10)):
        fn, base = getattr(lib, f"phnn_{name}_shaped"), getattr(lib, f"phnn_{name}")
        fn.argtypes = base.argtypes[:at] + [shp] + base.argtypes[at:]
        fn.restype = C.c_int
    lib.phnn_plant_step.argtypes = [vp, C.POINTER(Plant), vp, f32p, i64, i64, i32, C.c_float, C.c_float, f32p, vp, vp, i32,
                                    vp, f32p, vp]
    lib.phnn_plant_step.restype = C.c_int
    # the arguments of phnn_plant_step with a phnn_plant_ex* and a phnn_plant_metrics* after the plant
    lib.phnn_plant_step_ex.argtypes = (lib.phnn_plant_step.argtypes[:2] + [C.POINTER(PlantEx), C.POINTER(PlantMetrics)] +
                                       lib.phnn_plant_step.argtypes[2:])
    lib.phnn_plant_step_ex.restype = C.c_int
    lib.phnn_shift_controls.argtypes = [vp, f32p, f32p, i64, i32, i32, vp, vp]
    lib.phnn_shift_controls.restype = C.c_int
    gno = C.POINTER(GnOptions)
    lib.phnn_gn_workspace_bytes.argtypes = [vp, i64, i32, i32]
    lib.phnn_gn_workspace_bytes.restype = C.c_size_t
    lib.phnn_gn_direction.argtypes = [vp, f32p, f32p, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), vp, f32p, vp,
                                      vp, vp, vp]
    lib.phnn_gn_direction.restype = C.c_int
    lib.phnn_gn_candidates.argtypes = [vp, f32p, f32p, f32p, i64, i32, C.POINTER(Cost), i32, f32p, f32p, vp]
    lib.phnn_gn_candidates.restype = C.c_int
    lib.phnn_gn_select.argtypes = [vp, f32p, f32p, f32p, vp, vp, f32p, f32p, f32p, vp, i64, i32, gno, f32p, f32p, vp]
    lib.phnn_gn_select.restype = C.c_int
    lib.phnn_solve_gn.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float, gno, vp,
                                  C.c_size_t, f32p, f32p, vp, vp, f32p, vp]
    lib.phnn_solve_gn.restype = C.c_int
    # phnn_gn_direction's arguments with nclamp before the scratch; phnn_solve_gn's with flags and nclamp_hist before the stream
    lib.phnn_gn_direction_box.argtypes = lib.phnn_gn_direction.argtypes[:13] + [vp] + lib.phnn_gn_direction.argtypes[13:]
    lib.phnn_gn_direction_box.restype = C.c_int
    lib.phnn_solve_gn_ex.argtypes = lib.phnn_solve_gn.argtypes[:-1] + [i32, vp, vp]
    lib.phnn_solve_gn_ex.restype = C.c_int
    eko, ekl = C.POINTER(EkfOptions), C.POINTER(EkfLog)
    lib.phnn_ekf_workspace_bytes.argtypes = [vp, i64]
    lib.phnn_ekf_workspace_bytes.restype = C.c_size_t
    lib.phnn_ekf_update.argtypes = [vp, f32p, i64, f32p, f32p, i64, i64, eko, vp, f32p, vp, vp, vp, ekl, vp]
    lib.phnn_ekf_update.restype = C.c_int
    lib.phnn_ekf_step.argtypes = [vp, f32p, vp, f32p, i64, f32p, i64, i64, C.POINTER(Cost), i32, C.c_float, eko, vp, vp, vp,
                                  ekl, vp, vp]
    lib.phnn_ekf_step.restype = C.c_int
    dko, dkl = C.POINTER(DekfOptions), C.POINTER(DekfLog)
    lib.phnn_dekf_workspace_bytes.argtypes = [vp, i64]
    lib.phnn_dekf_workspace_bytes.restype = C.c_size_t
    lib.phnn_dekf_update.argtypes = [vp, f32p, i64, f32p, f32p, f32p, i64, i64, dko, vp, f32p, f32p, vp, vp, vp, dkl, vp]
    lib.phnn_dekf_update.restype = C.c_int
    lib.phnn_dekf_step.argtypes = [vp, f32p, f32p, vp, f32p, i64, f32p, i64, i64, C.POINTER(Cost), i32, C.c_float, dko, vp, vp,
                                   vp, dkl, vp, vp]
    lib.phnn_dekf_step.restype = C.c_int
    lib.phnn_dist_compensate.argtypes = [vp, f32p, i64, f32p, i64, C.POINTER(Cost), f32p, vp, vp]
    lib.phnn_dist_compensate.restype = C.c_int
    uko = C.POINTER(UkfOptions)
    lib.phnn_ukf_workspace_bytes.argtypes = [vp, i64]
    lib.phnn_ukf_workspace_bytes.restype = C.c_size_t
    lib.phnn_ukf_sigma.argtypes = [vp, f32p, vp, f32p, i64, i64, uko, f32p, f32p, vp]
    lib.phnn_ukf_sigma.restype = C.c_int
    lib.phnn_ukf_moments.argtypes = [vp, f32p, i64, i64, uko, f32p, vp, f32p, vp]
    lib.phnn_ukf_moments.restype = C.c_int
    lib.phnn_ukf_step.argtypes = [vp, f32p, vp, f32p, i64, f32p, i64, i64, C.POINTER(Cost), i32, C.c_float, uko, vp, vp, vp,
                                  ekl, vp, vp]
    lib.phnn_ukf_step.restype = C.c_int
    lib.phnn_feedback_workspace_bytes.argtypes = [vp, i64, i32]
    lib.phnn_feedback_workspace_bytes.restype = C.c_size_t
    lib.phnn_feedback_plan.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), i32, C.c_float, C.POINTER(TvlqrOptions), vp,
                                       C.c_size_t, f32p, vp, vp, vp]
    lib.phnn_feedback_plan.restype = C.c_int
    lib.phnn_feedback_control.argtypes = [vp, f32p, f32p, f32p, vp, i64, i32, C.POINTER(Cost), i32, vp, i32, f32p, vp, vp, vp, vp,
                                          vp]
    lib.phnn_feedback_control.restype = C.c_int
    # the terminal cost
    trm = C.POINTER(Terminal)
    lib.phnn_rollout_vjp_ref.argtypes = [vp, f32p, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), i32, C.c_float, f32p,
                                         vp, f32p, f32p, f32p, f32p, vp]
    lib.phnn_rollout_vjp_ref.restype = C.c_int
    lib.phnn_terminal_cost.argtypes = [vp, f32p, i64, i32, C.POINTER(Cost), C.POINTER(Reference), trm, f32p, f32p, vp]
    lib.phnn_terminal_cost.restype = C.c_int
    lib.phnn_dare.argtypes = [vp, f32p, f32p, i64, C.POINTER(Cost), C.POINTER(DareOptions), vp, vp, f32p, vp, vp, vp]
    lib.phnn_dare.restype = C.c_int
    # phnn_gn_direction's arguments with the terminal after the reference and flags, nclamp before the scratch
    gd = lib.phnn_gn_direction.argtypes
    lib.phnn_gn_direction_term.argtypes = gd[:9] + [trm] + gd[9:13] + [i32, vp] + gd[13:]
    lib.phnn_gn_direction_term.restype = C.c_int
    # phnn_solve_ref's arguments with the terminal after the reference and traj_bar before the stream
    sr = lib.phnn_solve_ref.argtypes
    lib.phnn_solve_term.argtypes = sr[:7] + [trm] + sr[7:-1] + [f32p, vp]
    lib.phnn_solve_term.restype = C.c_int
    # phnn_solve_gn_ex's arguments with the terminal after the reference
    sg = lib.phnn_solve_gn_ex.argtypes
    lib.phnn_solve_gn_term.argtypes = sg[:7] + [trm] + sg[7:]
    lib.phnn_solve_gn_term.restype = C.c_int
    lib.phnn_kernel_info.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i64]
    lib.phnn_kernel_info.restype = C.c_int
    lib.phnn_variant_name.argtypes = [vp]
    lib.phnn_variant_name.restype = C.c_char_p
    lib.phnn_version.argtypes = []
    lib.phnn_version.restype = C.c_int
    _lib = lib
    return lib
