"""ctypes binding of libsubspace_hip.so -- the same C ABI the Julia `ccall` wrapper binds
(include/subspace_hip.h; julia/SubspaceInferenceHIP.jl).  No arithmetic happens in this file.

Errors follow the reference's convention (`throw(::String)`, e.g. src/space_inference.jl:42,103,162):
a non-zero status raises `SubspaceError(message)`.
"""
import ctypes
import os
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_int, c_int32, c_int64, c_uint64,
                    c_void_p)

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsubspace_hip.so")

SI_OK, SI_ERR_INVALID, SI_ERR_STATE, SI_ERR_HIP, SI_ERR_NOMEM, SI_ERR_BOUNDS, SI_ERR_NODEVICE = 0, -1, -2, -3, -4, -5, -6
SI_ERR_COMM = -7
SI_COMM_ID_BYTES, SI_COMM_SUM, SI_COMM_MAX = 128, 0, 1
SI_F32, SI_F64 = 0, 1
SI_DTYPE_OF_DATA = -1
SI_LIK_GAUSSIAN, SI_LIK_CATEGORICAL, SI_LIK_BERNOULLI = 0, 1, 2
LIKELIHOODS = {"gaussian": SI_LIK_GAUSSIAN, "categorical": SI_LIK_CATEGORICAL, "bernoulli": SI_LIK_BERNOULLI}
ACT_IDENTITY, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
ACT_LEAKYRELU, ACT_ELU, ACT_SOFTPLUS, ACT_SELU = 4, 5, 6, 7
K_NAMES = ["push", "gram", "gram_reduce", "project", "reconstruct", "dense", "sse", "rwmh", "dense_main", "eig_host", "backward",
           "conv", "conv_aux"]
LAYER_DENSE, LAYER_CONV, LAYER_MAXPOOL, LAYER_FLATTEN = 0, 1, 2, 3
K_COUNT = len(K_NAMES)


class SubspaceError(RuntimeError):
    """The host-side image of the reference's `throw("...")`."""

    def __init__(self, msg, code=SI_ERR_INVALID):
        super().__init__(msg)
        self.code = code


class BoundsError(SubspaceError, IndexError):
    """Julia's BoundsError at `U[:,1:M]` (src/subspace_construction.jl:65) when rank(A) < M."""


class SiLayer(Structure):
    _fields_ = [("kind", c_int32), ("in_", c_int32), ("out", c_int32), ("act", c_int32),
                ("w_off", c_int64), ("b_off", c_int64),
                ("kw", c_int32), ("kh", c_int32), ("cin", c_int32), ("cout", c_int32), ("wi", c_int32), ("hi", c_int32),
                ("sw", c_int32), ("sh", c_int32), ("pw", c_int32), ("ph", c_int32), ("dw", c_int32), ("dh", c_int32)]


class SiStats(Structure):
    _fields_ = [("ms", c_double * K_COUNT), ("launches", c_int64 * K_COUNT),
                ("flops", c_double * K_COUNT), ("bytes", c_double * K_COUNT)]


class SiNodeOpts(Structure):
    _fields_ = [("t0", c_double), ("reltol", c_double), ("abstol", c_double), ("dt", c_double),
                ("adaptive", c_int32), ("max_steps", c_int32), ("pre_power", c_int32)]


# every symbol include/subspace_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "si_version": (c_int32, []),
    "si_create": (c_int32, [POINTER(c_void_p), c_int32]),
    "si_destroy": (c_int32, [c_void_p]),
    "si_last_error": (c_char_p, [c_void_p]),
    "si_set_stream": (c_int32, [c_void_p, c_void_p]),
    "si_synchronize": (c_int32, [c_void_p]),
    "si_set_profiling": (c_int32, [c_void_p, c_int32]),
    "si_set_profiling_classes": (c_int32, [c_void_p, ctypes.c_uint32]),
    "si_get_stats": (c_int32, [c_void_p, POINTER(SiStats)]),
    "si_reset_stats": (c_int32, [c_void_p]),
    "si_device_name": (c_int32, [c_void_p, c_char_p, c_int32]),
    "si_construct_begin": (c_int32, [c_void_p, c_int64, c_int64, c_int32]),
    "si_construct_set_mean": (c_int32, [c_void_p, c_void_p, c_int32]),
    "si_construct_push": (c_int32, [c_void_p, c_void_p, c_int32, c_double]),
    "si_construct_push_dev": (c_int32, [c_void_p, c_void_p, c_int32, c_double]),
    "si_construct_push_batch_dev": (c_int32, [c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p]),
    "si_construct_gram": (c_int32, [c_void_p]),
    "si_construct_gram_get": (c_int32, [c_void_p, c_void_p, POINTER(c_int64)]),
    "si_construct_gram_set": (c_int32, [c_void_p, c_void_p]),
    "si_construct_gram_ptr": (c_int32, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    "si_construct_result_ptr": (c_int32, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int64),
                                          POINTER(c_int32)]),
    "si_construct_needs_refine": (c_int32, [c_void_p, c_int32, POINTER(c_int32)]),
    "si_construct_refine": (c_int32, [c_void_p]),
    "si_construct_finish": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    "si_construct_get_A": (c_int32, [c_void_p, c_int64, c_int64, c_void_p]),
    "si_construct_finish_diffmap": (c_int32, [c_void_p, c_int32, c_double, c_double, c_int32, c_int32, c_double, c_int32, c_void_p,
                                              c_void_p, c_void_p, POINTER(c_int64)]),
    "si_diffmap_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_double)]),
    "si_diffmap_get_kernel": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "si_construct_get_result": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int32)]),
    "si_infer_setup": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_int32, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_int32, c_int32, c_int64, c_double, c_int32]),
    "si_infer_setup_dev": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_int32, c_void_p, c_void_p, c_int64,
                                     c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_double, c_int32]),
    "si_infer_set_prior": (c_int32, [c_void_p, c_double]),
    "si_infer_set_likelihood": (c_int32, [c_void_p, c_int32]),
    "si_infer_likelihood_info": (c_int32, [c_void_p, POINTER(c_int32)]),
    "si_infer_set_decoder": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_void_p, c_int32]),
    "si_infer_decoder_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "si_decode": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "si_decode_vjp": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_infer_setup_node": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int32, c_int32, c_int64, c_void_p, c_void_p]),
    "si_node_solve": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_node_tableau": (c_int32, [c_void_p]),
    "si_node_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int64), POINTER(c_int32)]),
    "si_node_set_grad": (c_int32, [c_void_p, c_int32]),
    "si_node_grad_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32)]),
    "si_node_grad": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "si_logdensity": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p]),
    "si_logdensity_grad": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_logdensity_grad_batch": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "si_grad_kernel_info": (c_int32, [c_void_p, POINTER(c_int32)]),
    "si_forward": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "si_predict": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
    "si_sample_rwmh": (c_int32, [c_void_p, c_int64, c_double, c_uint64, c_int32, c_int32, c_void_p, c_void_p,
                                 c_void_p]),
    "si_sample_rwmh_weights": (c_int32, [c_void_p, c_int64, c_double, c_uint64, c_int32, c_int32, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "si_sample_mala": (c_int32, [c_void_p, c_int64, c_double, c_uint64, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                 c_void_p]),
    "si_mala_kernel_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32)]),
    "si_sample_hmc": (c_int32, [c_void_p, c_int64, c_int64, c_double, c_double, c_uint64, c_int32, c_int32, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_hmc_kernel_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "si_sample_nuts": (c_int32, [c_void_p, c_int64, c_int64, c_double, c_double, c_int32, c_double, c_uint64, c_int32, c_int32,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int64]),
    "si_nuts_kernel_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int64),
                                      POINTER(c_int64)]),
    "si_sample_ess": (c_int32, [c_void_p, c_int64, c_double, c_int32, c_uint64, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "si_ess_kernel_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int64), POINTER(c_int64)]),
    "si_fit_advi": (c_int32, [c_void_p, c_int64, c_int32, c_double, c_double, c_double, c_int32, c_uint64, c_int32, c_int32, c_int64,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_advi_kernel_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32)]),
    "si_rwmh_begin": (c_int32, [c_void_p, c_int64, c_double, c_uint64, c_int32, c_int32, c_int64]),
    "si_rwmh_step_eval": (c_int32, [c_void_p, c_void_p]),
    "si_rwmh_step_accept": (c_int32, [c_void_p, c_void_p]),
    "si_rwmh_sse_ptr": (c_int32, [c_void_p, POINTER(c_void_p), POINTER(c_int32)]),
    "si_rwmh_end": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_rwmh_abort": (c_int32, [c_void_p]),
    "si_reconstruct": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "si_train_setup": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_int32,
                                 c_int32, c_int64, c_int64, c_int32, c_double, c_double, c_double]),
    "si_train_setup_ex": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                    c_int32, c_int64, c_int64, c_int32, c_double, c_double, c_double, c_int32]),
    "si_train_compute_dtype": (c_int32, [c_void_p, c_void_p]),
    "si_train_set_cost": (c_int32, [c_void_p, c_int32, c_double]),
    "si_train_cost_info": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "si_train_step": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "si_train_push": (c_int32, [c_void_p, c_double]),
    "si_train_get_weights": (c_int32, [c_void_p, c_void_p]),
    "si_train_get_opt_state": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_train_grad": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "si_train_grad_ptr": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "si_train_grad_get": (c_int32, [c_void_p, c_void_p]),
    "si_train_grad_set": (c_int32, [c_void_p, c_void_p]),
    "si_train_apply": (c_int32, [c_void_p]),
    "si_train_setup_node": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64,
                                      c_void_p, c_void_p, c_int64, c_int32, c_double, c_double, c_double, c_double]),
    "si_train_node_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int64), POINTER(c_int64), POINTER(c_int32)]),
    "si_ae_train_setup": (c_int32, [c_void_p, POINTER(SiLayer), c_int32, c_int64, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int32,
                                    c_int32, c_double, c_double, c_double, c_int32]),
    "si_ae_train_step": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "si_ae_train_loss": (c_int32, [c_void_p, c_void_p]),
    "si_ae_train_get_params": (c_int32, [c_void_p, c_void_p]),
    "si_ae_train_get_opt_state": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "si_ae_train_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int32)]),
    "si_ae_train_free": (c_int32, [c_void_p]),
    "si_comm_unique_id": (c_int32, [c_void_p]),
    "si_comm_init_rank": (c_int32, [c_void_p, c_int32, c_int32, c_void_p]),
    "si_comm_destroy": (c_int32, [c_void_p]),
    "si_comm_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "si_comm_allreduce_host": (c_int32, [c_void_p, c_void_p, c_int64, c_int32]),
    "si_comm_allgather_host": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "si_comm_barrier": (c_int32, [c_void_p]),
    "si_row_shard": (c_int32, [c_int64, c_int32, c_int32, POINTER(c_int64), POINTER(c_int64)]),
    "si_construct_allreduce_gram": (c_int32, [c_void_p]),
    "si_construct_allgather": (c_int32, [c_void_p, c_int64]),
    "si_bcast_subspace": (c_int32, [c_void_p, c_int32, c_int64, c_int32]),
    "si_rwmh_allreduce_sse": (c_int32, [c_void_p]),
    "si_sample_rwmh_sharded": (c_int32, [c_void_p, c_int64, c_double, c_uint64, c_int32, c_int32, c_int64, c_void_p, c_void_p,
                                         c_void_p]),
    "si_train_allreduce_grad": (c_int32, [c_void_p, c_void_p]),
    "si_train_step_dp": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "si_host_sym_eig": (c_int, [c_int, c_void_p, c_void_p]),
    "si_host_sym_eig_top": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "si_host_jacobi_eig_psd": (c_int, [c_int, c_void_p, c_void_p, c_void_p]),
    "si_set_chain_loop": (c_int32, [c_void_p, c_int32]),
    "si_chain_kernel_info": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32)]),
    "si_chain_spec_message": (c_char_p, [c_void_p]),
    "si_construct_set_storage": (c_int32, [c_void_p, c_int32]),
    "si_host_hmc_windows": (c_int32, [c_int64, POINTER(c_int64), POINTER(c_int64), c_void_p, c_int32]),
    "si_host_cpu_budget": (c_int, []),
    "si_host_parse_cpu_max": (c_double, [c_char_p]),
    "si_host_copy_plan": (c_int, [c_int, c_int, c_char_p]),
}

_lib = None

# What si_fit_advi refuses with SI_ERR_INVALID (include/subspace_hip.h), mirrored: (the refusal, its test).  The comparisons are
# written so that a NaN refuses, as the library's are.
ADVI_REFUSALS = (
    ("max_iters < 1", lambda a: not a["T"] >= 1),
    ("samples_per_step < 1", lambda a: not a["S"] >= 1),
    ("samples_per_step * ceil(M / 2) >= 2^24", lambda a: a["S"] * ((a["M"] + 1) // 2) >= 2 ** 24),
    ("window outside 1 .. 1024", lambda a: not 1 <= a["W"] <= 1024),
    ("nruns < 1", lambda a: not a["R"] >= 1),
    ("chain_id0 < 0", lambda a: not a["chain_id0"] >= 0),
    ("sigma_z <= 0", lambda a: not a["sigma_z"] > 0.0),
    ("tau <= 0", lambda a: not a["tau"] > 0.0),
    ("eta <= 0", lambda a: not a["eta"] > 0.0),
    ("ndraws < 0", lambda a: not a["D"] >= 0),
)


def advi_refusal(m, max_iters, samples_per_step, sigma_z, eta, tau, window, chain_id0, nruns, ndraws):
    """the first refusal of ADVI_REFUSALS that holds, or None"""
    a = dict(M=m, T=max_iters, S=samples_per_step, sigma_z=sigma_z, eta=eta, tau=tau, W=window, chain_id0=chain_id0, R=nruns, D=ndraws)
    return next((what for what, bad in ADVI_REFUSALS if bad(a)), None)


def load():
    """dlopen the in-tree library.  Fails loudly when it has not been built: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SubspaceError(
            "libsubspace_hip.so is missing (%s): build it with `python __graft_entry__.py` -- "
            "this package has no CPU or PyTorch fallback" % LIB_PATH, SI_ERR_NODEVICE)
    if os.environ.get("SI_PRELOAD_TORCH", "1") != "0":
        # torch wheels bundle their own libamdhip64.so.7; when both live in one process the HIP runtime
        # must be loaded once.  Importing torch first makes the library bind to the already loaded runtime.
        try:
            import torch  # noqa: F401
        except Exception:  # torch is plumbing only; the library itself does not need it
            pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and the header disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    # (a.ctypes builds a helper object per call -- a quarter of a millisecond in a loop of training steps)
    return None if a is None else c_void_p(a.__array_interface__["data"][0])


def conv_out_size(wi, k, s, p, d):
    return (wi + 2 * p - d * (k - 1) - 1) // s + 1


def _layer_array(table):
    """table rows: Dense (in, out, act, w_off, b_off), or
         ("conv", (kw, kh, cin, cout), (wi, hi), (sw, sh), (pw, ph), (dw, dh), act, w_off, b_off)
         ("maxpool", (pw, ph), c, (wi, hi), (sw, sh))        ("flatten", c, (wi, hi))"""
    arr = (SiLayer * len(table))()
    for i, row in enumerate(table):
        if row[0] == "conv":
            _, (kw, kh, cin, cout), (wi, hi), (sw, sh), (pw, ph), (dw, dh), act, w_off, b_off = row
            wo, ho = conv_out_size(wi, kw, sw, pw, dw), conv_out_size(hi, kh, sh, ph, dh)
            arr[i] = SiLayer(LAYER_CONV, wi * hi * cin, wo * ho * cout, int(act), int(w_off), int(b_off), kw, kh, cin, cout,
                             wi, hi, sw, sh, pw, ph, dw, dh)
        elif row[0] == "maxpool":
            _, (kw, kh), c, (wi, hi), (sw, sh) = row
            wo, ho = (wi - kw) // sw + 1, (hi - kh) // sh + 1
            arr[i] = SiLayer(LAYER_MAXPOOL, wi * hi * c, wo * ho * c, 0, 0, 0, kw, kh, c, c, wi, hi, sw, sh, 0, 0, 1, 1)
        elif row[0] == "flatten":
            _, c, (wi, hi) = row
            arr[i] = SiLayer(LAYER_FLATTEN, wi * hi * c, wi * hi * c, 0, 0, 0, 0, 0, c, c, wi, hi, 1, 1, 0, 0, 1, 1)
        else:
            fin, fout, act, w_off, b_off = row[:5]
            arr[i] = SiLayer(LAYER_DENSE, int(fin), int(fout), int(act), int(w_off), int(b_off))
    return arr


def _f64(a, order="F"):
    return np.require(a, dtype=np.float64, requirements=[order, "A"])


class Context:
    """Owns one `si_ctx` (one GPU).  Thin: argument marshalling + status -> exception."""

    def __init__(self, device=0):
        self.lib = load()
        h = c_void_p()
        rc = self.lib.si_create(byref(h), int(device))
        if rc != SI_OK:
            msg = self.lib.si_last_error(None).decode()
            raise SubspaceError(msg, rc)
        self.h = h
        self.device = int(device)

    # -- plumbing
    def _check(self, rc):
        if rc == SI_OK:
            return
        msg = self.lib.si_last_error(self.h).decode()
        if rc == SI_ERR_BOUNDS:
            raise BoundsError(msg, rc)
        raise SubspaceError(msg, rc)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.si_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.si_device_name(self.h, buf, 256))
        return buf.value.decode()

    def set_stream(self, stream_handle):
        self._check(self.lib.si_set_stream(self.h, c_void_p(stream_handle) if stream_handle else None))

    def synchronize(self):
        self._check(self.lib.si_synchronize(self.h))

    def set_profiling(self, on, classes=None):
        """classes: iterable of class names (K_NAMES) that get event pairs; None = all."""
        self._check(self.lib.si_set_profiling(self.h, 1 if on else 0))
        mask = 0xFFFFFFFF if classes is None else sum(1 << K_NAMES.index(k) for k in classes)
        self._check(self.lib.si_set_profiling_classes(self.h, mask))

    def reset_stats(self):
        self._check(self.lib.si_reset_stats(self.h))

    def stats(self):
        st = SiStats()
        self._check(self.lib.si_get_stats(self.h, byref(st)))
        return {K_NAMES[i]: {"ms": st.ms[i], "launches": st.launches[i], "flops": st.flops[i], "bytes": st.bytes[i]}
                for i in range(K_COUNT)}

    # -- R1: the RCCL communicator of this ctx (one rank per ctx / GPU / process)
    def comm_init_rank(self, world, rank, uid):
        if len(uid) != SI_COMM_ID_BYTES:
            raise SubspaceError("comm_init_rank: the id must be %d bytes" % SI_COMM_ID_BYTES)
        buf = ctypes.create_string_buffer(bytes(uid), SI_COMM_ID_BYTES)
        self._check(self.lib.si_comm_init_rank(self.h, int(world), int(rank), buf))

    def comm_destroy(self):
        self._check(self.lib.si_comm_destroy(self.h))

    def comm_info(self):
        """(world, rank, rccl_version); world = 0 without a communicator"""
        w, r, v = c_int32(), c_int32(), c_int32()
        self._check(self.lib.si_comm_info(self.h, byref(w), byref(r), byref(v)))
        return int(w.value), int(r.value), int(v.value)

    def comm_world(self):
        return self.comm_info()[0]

    def comm_allreduce_host(self, values, op="sum"):
        a = np.array(values, dtype=np.float64, order="C").reshape(-1)
        self._check(self.lib.si_comm_allreduce_host(self.h, _ptr(a), a.size, SI_COMM_SUM if op == "sum" else SI_COMM_MAX))
        return a.reshape(np.shape(values))

    def comm_allgather_host(self, values):
        """(world, n) array: row r = rank r's `values`"""
        a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        out = np.empty((self.comm_world(), a.size), dtype=np.float64)
        self._check(self.lib.si_comm_allgather_host(self.h, _ptr(a), a.size, _ptr(out)))
        return out

    def comm_barrier(self):
        self._check(self.lib.si_comm_barrier(self.h))

    def construct_allreduce_gram(self):
        self._check(self.lib.si_construct_allreduce_gram(self.h))

    def construct_allgather(self, n_total):
        """full (W_swa, P) on every rank, device to device; the ctx then holds a finished construction of n_total rows"""
        self._check(self.lib.si_construct_allgather(self.h, int(n_total)))
        self._n = int(n_total)

    def bcast_subspace(self, root, n, m):
        self._check(self.lib.si_bcast_subspace(self.h, int(root), int(n), int(m)))
        self._n = int(n)

    def rwmh_allreduce_sse(self):
        self._check(self.lib.si_rwmh_allreduce_sse(self.h))

    def sample_rwmh_sharded(self, itr, sigma_z, seed, d_total, chain_id0=0, nchains=1):
        z = np.empty((self._m, int(itr), int(nchains)), dtype=np.float64, order="F")
        lp = np.empty((int(itr), int(nchains)), dtype=np.float64, order="F")
        acc = np.empty(int(nchains), dtype=np.float64)
        self._check(self.lib.si_sample_rwmh_sharded(self.h, int(itr), float(sigma_z), int(seed), int(chain_id0), int(nchains),
                                                    int(d_total), _ptr(z), _ptr(lp), _ptr(acc)))
        return z, lp, acc

    def train_allreduce_grad(self, want_sse=True):
        sse = np.empty(1, dtype=np.float64) if want_sse else None
        self._check(self.lib.si_train_allreduce_grad(self.h, _ptr(sse)))
        return float(sse[0]) if want_sse else None

    def train_step_dp(self, idx, nb_total, want_loss=True):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        loss = np.empty(1, dtype=np.float64) if want_loss else None
        self._check(self.lib.si_train_step_dp(self.h, _ptr(idx) if idx.size else None, idx.size, int(nb_total), _ptr(loss)))
        return float(loss[0]) if want_loss else None

    def construct_get_result(self, want_p=True):
        """(W_swa, P, s) of the FINISHED construction the ctx holds -- its own, or one received through bcast_subspace /
        construct_allgather -- copied to the host."""
        n, m = c_int64(), c_int32()
        self._check(self.lib.si_construct_get_result(self.h, None, None, None, byref(n), byref(m)))
        w = np.empty(n.value, dtype=np.float64)
        p = np.empty((n.value, m.value), dtype=np.float64, order="F") if want_p else None
        s = np.empty(m.value, dtype=np.float64)
        self._check(self.lib.si_construct_get_result(self.h, _ptr(w), _ptr(p), _ptr(s), byref(n), byref(m)))
        return w, p, s

    # -- construction
    def construct_begin(self, n, k_capacity, max_cols=0):
        self._check(self.lib.si_construct_begin(self.h, int(n), int(k_capacity), int(max_cols)))
        self._n = int(n)

    def construct_set_storage(self, a_dtype):
        """SI_F32: keep the deviation matrix in fp32 (opt-in); right after construct_begin."""
        self._check(self.lib.si_construct_set_storage(self.h, int(a_dtype)))

    def construct_set_mean(self, w):
        """non-default init = :pretrained (Q1): W_swa starts at w instead of zeros"""
        w = np.ascontiguousarray(w)
        if w.dtype not in (np.float32, np.float64) or w.size != self._n:
            raise SubspaceError("DimensionMismatch / dtype: initial mean needs %d Float32 or Float64 values" % self._n)
        self._check(self.lib.si_construct_set_mean(self.h, _ptr(w), SI_F32 if w.dtype == np.float32 else SI_F64))

    def construct_push(self, w, n):
        w = np.ascontiguousarray(w)
        if w.dtype == np.float32:
            dt = SI_F32
        elif w.dtype == np.float64:
            dt = SI_F64
        else:
            raise SubspaceError("weights must be Float32 or Float64, got %s" % w.dtype)
        if w.size != self._n:
            raise SubspaceError("DimensionMismatch: snapshot has %d elements, expected %d" % (w.size, self._n))
        self._check(self.lib.si_construct_push(self.h, _ptr(w), dt, float(n)))

    def construct_push_dev(self, dev_ptr, dtype, n):
        self._check(self.lib.si_construct_push_dev(self.h, c_void_p(int(dev_ptr)), int(dtype), float(n)))

    def construct_push_batch_dev(self, dev_ptr, dtype, ld, ns):
        ns = np.ascontiguousarray(ns, dtype=np.float64)
        self._check(self.lib.si_construct_push_batch_dev(self.h, c_void_p(int(dev_ptr)), int(dtype), int(ld), ns.size,
                                                         _ptr(ns)))

    def construct_gram(self):
        self._check(self.lib.si_construct_gram(self.h))

    def construct_gram_get(self):
        k = c_int64()
        self._check(self.lib.si_construct_gram_get(self.h, None, byref(k)))
        g = np.empty((k.value, k.value), dtype=np.float64, order="F")
        self._check(self.lib.si_construct_gram_get(self.h, _ptr(g), byref(k)))
        return g

    def construct_gram_set(self, g):
        g = _f64(g)
        self._check(self.lib.si_construct_gram_set(self.h, _ptr(g)))

    def construct_needs_refine(self, m):
        """True when the Gram route cannot resolve s_M (ill-conditioned A): the two-stage route is needed."""
        flag = c_int32()
        self._check(self.lib.si_construct_needs_refine(self.h, int(m), byref(flag)))
        return bool(flag.value)

    def construct_refine(self):
        self._check(self.lib.si_construct_refine(self.h))

    def construct_gram_ptr(self):
        """(device address, K) of the K x K fp64 Gram matrix, for an in-place RCCL all-reduce."""
        ptr, k = c_void_p(), c_int64()
        self._check(self.lib.si_construct_gram_ptr(self.h, byref(ptr), byref(k)))
        return int(ptr.value), int(k.value)

    def construct_result_ptr(self):
        """(W_swa device address, P device address, ld, M) of the finished construction."""
        ws, pp, ld, m = c_void_p(), c_void_p(), c_int64(), c_int32()
        self._check(self.lib.si_construct_result_ptr(self.h, byref(ws), byref(pp), byref(ld), byref(m)))
        return int(ws.value), int(pp.value), int(ld.value), int(m.value)

    def construct_finish(self, m, want_swa=True, want_p=True):
        k = c_int64()
        w_swa = np.empty(self._n, dtype=np.float64) if want_swa else None
        p = np.empty((self._n, int(m)), dtype=np.float64, order="F") if want_p else None
        s = np.empty(int(m), dtype=np.float64)
        self._check(self.lib.si_construct_finish(self.h, int(m), _ptr(w_swa), _ptr(p), _ptr(s), byref(k)))
        return w_swa, p, s, k.value

    def construct_finish_diffmap(self, m, eps=1.0, alpha=1.0, kernel_sign=-1, rescale=True, tol=0.0, max_iters=0, want_swa=True,
                                 want_p=True):
        """method = :diffusion (reference src/subspace_construction.jl:202-206; the definition is diffmap.py's): (W_swa, P, lam, K)
        with lam the M + 1 leading eigenvalues by |.| descending, lam[0] = 1.  tol <= 0: 1e-12; max_iters <= 0: 500."""
        k = c_int64()
        w_swa = np.empty(self._n, dtype=np.float64) if want_swa else None
        p = np.empty((self._n, max(int(m), 0)), dtype=np.float64, order="F") if want_p else None
        lam = np.empty(max(int(m), 0) + 1, dtype=np.float64)
        self._check(self.lib.si_construct_finish_diffmap(self.h, int(m), float(eps), float(alpha), int(kernel_sign), 1 if rescale else 0,
                                                         float(tol), int(max_iters), _ptr(w_swa), _ptr(p), _ptr(lam), byref(k)))
        return w_swa, p, lam, k.value

    def diffmap_info(self):
        """(iterations, largest leading residual) of the last construct_finish_diffmap"""
        it, res = c_int32(), c_double()
        self._check(self.lib.si_diffmap_info(self.h, byref(it), byref(res)))
        return it.value, res.value

    def diffmap_get_kernel(self, want_kn=True):
        """audit read-back of the last construct_finish_diffmap: (Kn (N x N) or None, u_1)"""
        kn = np.empty((self._n, self._n), dtype=np.float64, order="F") if want_kn else None
        u1 = np.empty(self._n, dtype=np.float64)
        self._check(self.lib.si_diffmap_get_kernel(self.h, _ptr(kn), _ptr(u1)))
        return kn, u1

    def construct_get_A(self, k0, nk):
        a = np.empty((self._n, int(nk)), dtype=np.float64, order="F")
        self._check(self.lib.si_construct_get_A(self.h, int(k0), int(nk), _ptr(a)))
        return a

    # -- on-device training (f1)
    def train_setup(self, table, n, w0, x, y, batch_max, opt_kind, eta, p1=0.0, p2=0.0, compute_dtype=None):
        """si_train_setup_ex.  compute_dtype None: the reference's own arithmetic for the data handed in -- Float32 (x, y) give
        the all-Float32 pass (SI_F32), anything else is promoted to Float64 as Julia would; SI_F32 / SI_F64 override."""
        arr = _layer_array(table)
        x, y = np.asarray(x), np.asarray(y)
        data_f32 = x.dtype == np.float32 and y.dtype == np.float32
        dt = np.float32 if data_f32 else np.float64
        x, y = np.asfortranarray(x, dtype=dt), np.asfortranarray(y, dtype=dt)
        w0 = np.ascontiguousarray(w0, dtype=np.float32)
        if w0.size != n or x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
            raise SubspaceError("DimensionMismatch: w0 %s, X %s, Y %s" % (w0.shape, x.shape, y.shape))
        self._check(self.lib.si_train_setup_ex(self.h, arr, len(table), int(n), _ptr(w0), _ptr(x), _ptr(y),
                                               SI_F32 if data_f32 else SI_F64, x.shape[0], y.shape[0], x.shape[1], int(batch_max),
                                               int(opt_kind), float(eta), float(p1), float(p2),
                                               SI_DTYPE_OF_DATA if compute_dtype is None else int(compute_dtype)))
        self._tn = int(n)
        self._tout = int(y.shape[0])

    def train_setup_node(self, table, n, w0, u0, y, ts, batch_max, opt_kind, eta, p1=0.0, p2=0.0, penalty_div=100.0, t0=0.0,
                         reltol=1e-3, abstol=1e-6, dt=0.0, adaptive=True, max_steps=100000, pre_power=1):
        """si_train_setup_node, in place of train_setup, for a NeuralODE (node.train_value_and_grad is the definition of a step):
        `table`, u0 (d x f), y (d*S x f), ts and the options as infer_setup_node takes them; penalty_div None or 0: no penalty."""
        arr = _layer_array(table)
        u0, y, ts = _f64(u0), _f64(y), np.ascontiguousarray(ts, dtype=np.float64).reshape(-1)
        w0 = np.ascontiguousarray(w0, dtype=np.float32)
        if w0.size != n or u0.ndim != 2 or y.ndim != 2 or u0.shape[1] != y.shape[1] or y.shape[0] != u0.shape[0] * ts.size:
            raise SubspaceError("DimensionMismatch: w0 %s, U0 is %s, Y is %s, %d save times: Y must be (d*S, f)"
                                % (w0.shape, u0.shape, y.shape, ts.size))
        opts = SiNodeOpts(float(t0), float(reltol), float(abstol), float(dt), 1 if adaptive else 0, int(max_steps), int(pre_power))
        self._check(self.lib.si_train_setup_node(self.h, arr, len(table), int(n), _ptr(w0), _ptr(u0), _ptr(y), u0.shape[0], ts.size,
                                                 u0.shape[1], _ptr(ts), byref(opts), int(batch_max), int(opt_kind), float(eta), float(p1),
                                                 float(p2), 0.0 if penalty_div is None else float(penalty_div)))
        self._tn = int(n)
        self._tout = int(y.shape[0])

    def train_node_info(self):
        """(active, G, failed step or -1, the failed trajectory's position in its batch or -1, its status): si_train_node_info"""
        on, g, st = c_int32(0), c_int32(0), c_int32(0)
        step, traj = c_int64(-1), c_int64(-1)
        self._check(self.lib.si_train_node_info(self.h, byref(on), byref(g), byref(step), byref(traj), byref(st)))
        return bool(on.value), int(g.value), int(step.value), int(traj.value), int(st.value)

    def train_compute_dtype(self):
        out = np.zeros(1, dtype=np.int32)
        self._check(self.lib.si_train_compute_dtype(self.h, _ptr(out)))
        return int(out[0])

    def train_set_cost(self, cost, param=0.0):
        """si_train_set_cost: the cost of the steps that follow (costs.py: MSE .. LOGITBCE; param = Huber's delta).  It follows
        train_setup, which starts with mse again."""
        self._check(self.lib.si_train_set_cost(self.h, int(cost), float(param)))

    def train_cost_info(self):
        """(cost id, param) of the training state: si_train_cost_info"""
        cost, param = c_int32(0), c_double(0.0)
        self._check(self.lib.si_train_cost_info(self.h, byref(cost), byref(param)))
        return int(cost.value), float(param.value)

    def train_step(self, idx, want_loss=True):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        loss = np.empty(1, dtype=np.float64) if want_loss else None
        self._check(self.lib.si_train_step(self.h, _ptr(idx), idx.size, _ptr(loss)))
        return float(loss[0]) if want_loss else None

    # data-parallel form: grad -> (caller's all-reduce) -> apply
    def train_grad(self, idx, nb_total):
        """Gradient of the cost (mse by default) over the WHOLE batch (nb_total observations) restricted to this rank's idx;
        returns the local numerator of the cost (mse: the local SSE)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        sse = np.empty(1, dtype=np.float64)
        self._check(self.lib.si_train_grad(self.h, _ptr(idx), idx.size, int(nb_total), _ptr(sse)))
        return float(sse[0])

    def train_grad_ptr(self):
        """(device address, element count) of the fp64 gradient buffer, for an in-place RCCL all-reduce."""
        ptr, n = c_void_p(), c_int64()
        self._check(self.lib.si_train_grad_ptr(self.h, byref(ptr), byref(n)))
        return int(ptr.value), int(n.value)

    def train_grad_get(self):
        g = np.empty(self._tn, dtype=np.float64)
        self._check(self.lib.si_train_grad_get(self.h, _ptr(g)))
        return g

    def train_grad_set(self, g):
        g = np.ascontiguousarray(g, dtype=np.float64)
        if g.size != self._tn:
            raise SubspaceError("DimensionMismatch: gradient of %d elements for %d weights" % (g.size, self._tn))
        self._check(self.lib.si_train_grad_set(self.h, _ptr(g)))

    def train_apply(self):
        self._check(self.lib.si_train_apply(self.h))

    def train_out_dim(self):
        return self._tout

    def train_push(self, n):
        self._check(self.lib.si_train_push(self.h, float(n)))

    def train_get_weights(self):
        w = np.empty(self._tn, dtype=np.float32)
        self._check(self.lib.si_train_get_weights(self.h, _ptr(w)))
        return w

    def train_get_opt_state(self):
        """(m, v, (beta1^t, beta2^t)) -- Float32 flat state of the device optimiser."""
        m = np.empty(self._tn, dtype=np.float32)
        v = np.empty(self._tn, dtype=np.float32)
        bp = np.empty(2, dtype=np.float64)
        self._check(self.lib.si_train_get_opt_state(self.h, _ptr(m), _ptr(v), _ptr(bp)))
        return m, v, (float(bp[0]), float(bp[1]))

    # -- the autoencoder of auto_encoder_subspace trained on the device (autoencoder.py: train_step is the definition)
    def ae_train_setup(self, table, w0, x, n, batch_max, opt_kind, eta, p1=0.0, p2=0.0, penalty=False):
        """si_ae_train_setup.  `table` is the Dense layer table of Chain(encoder, decoder), `w0` its flat Float32 or Float64
        parameters (they and the optimiser state stay on the device in that type).  x None: the open construction's deviation
        matrix, read in place; else the N x K matrix, uploaded once."""
        w0 = np.ascontiguousarray(w0)
        if w0.dtype not in (np.float32, np.float64) or w0.ndim != 1:
            raise SubspaceError("autoencoder parameters must be a flat Float32 or Float64 vector, got %s %s" % (w0.dtype, w0.shape))
        k = 0
        if x is not None:
            x = _f64(x)
            if x.ndim != 2 or x.shape[0] != n:
                raise SubspaceError("DimensionMismatch: X is %s, expected %d rows" % (x.shape, n))
            k = x.shape[1]
        arr = _layer_array(table)
        self._check(self.lib.si_ae_train_setup(self.h, arr, len(table), w0.size, _ptr(w0), SI_F32 if w0.dtype == np.float32 else SI_F64,
                                               _ptr(x), int(n), int(k), int(batch_max), int(opt_kind), float(eta), float(p1), float(p2),
                                               1 if penalty else 0))
        self._ae_n, self._ae_dtype = w0.size, w0.dtype

    def ae_train_step(self, idx, want_loss=True):
        """one step on the columns idx; the loss of the batch before the update, or None (queued: no host synchronisation)"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        loss = c_double(0.0)
        self._check(self.lib.si_ae_train_step(self.h, _ptr(idx), idx.size, byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def ae_train_loss(self):
        """the loss over all K columns (the reference's callback `autoloss(re_weight)`)"""
        loss = c_double(0.0)
        self._check(self.lib.si_ae_train_loss(self.h, byref(loss)))
        return float(loss.value)

    def ae_train_get_params(self):
        w = np.empty(self._ae_n, dtype=self._ae_dtype)
        self._check(self.lib.si_ae_train_get_params(self.h, _ptr(w)))
        return w

    def ae_train_get_opt_state(self):
        """(m, v, (beta1^t, beta2^t)) in the parameters' element type"""
        m, v = np.empty(self._ae_n, dtype=self._ae_dtype), np.empty(self._ae_n, dtype=self._ae_dtype)
        bp = np.empty(2, dtype=np.float64)
        self._check(self.lib.si_ae_train_get_opt_state(self.h, _ptr(m), _ptr(v), _ptr(bp)))
        return m, v, (float(bp[0]), float(bp[1]))

    def ae_train_info(self):
        """(active, N, K, n_params, whether the last layer's update is fused into the pass over W_D)"""
        a, f = c_int32(0), c_int32(0)
        n, k, p = c_int64(0), c_int64(0), c_int64(0)
        self._check(self.lib.si_ae_train_info(self.h, byref(a), byref(n), byref(k), byref(p), byref(f)))
        return bool(a.value), int(n.value), int(k.value), int(p.value), bool(f.value)

    def ae_train_free(self):
        self._check(self.lib.si_ae_train_free(self.h))

    # -- density + sampling
    def infer_setup(self, table, n, m, w_swa, p, x, y, sigma_m, compute_dtype=SI_F64):
        """table: list of (in, out, act, w_off, b_off); w_swa/p None => reuse the finished construction.
        compute_dtype: SI_F64 (the reference's arithmetic) or SI_F32 (Dense chains: fp32 X / weights / activations on the
        fp32 matrix instruction, head + SSE in fp64; the measured option of SURVEY section 0 Q6)."""
        arr = _layer_array(table)
        x = _f64(x)
        y = _f64(y)
        if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
            raise SubspaceError("DimensionMismatch: X is %s, Y is %s" % (x.shape, y.shape))
        if w_swa is not None:
            w_swa = _f64(w_swa)
            p = _f64(p)
            if w_swa.shape != (n,) or p.shape != (n, m):
                raise SubspaceError("DimensionMismatch: W_swa %s, P %s, expected (%d,), (%d, %d)"
                                    % (w_swa.shape, p.shape, n, n, m))
        self._check(self.lib.si_infer_setup(self.h, arr, len(table), int(n), int(m), _ptr(w_swa), _ptr(p), _ptr(x),
                                            _ptr(y), x.shape[0], y.shape[0], x.shape[1], float(sigma_m), int(compute_dtype)))
        self._m, self._in, self._out, self._b, self._ni = int(m), x.shape[0], y.shape[0], x.shape[1], int(n)

    def infer_setup_dev(self, table, n, m, w_swa_ptr, p_ptr, ld_p, x_ptr, y_ptr, in_dim, out_dim, b, sigma_m, borrow=False,
                        compute_dtype=SI_F64):
        """si_infer_setup with device addresses (ints); w_swa_ptr / p_ptr 0 or None => the finished construction."""
        arr = _layer_array(table)
        self._check(self.lib.si_infer_setup_dev(
            self.h, arr, len(table), int(n), int(m), c_void_p(int(w_swa_ptr)) if w_swa_ptr else None,
            c_void_p(int(p_ptr)) if p_ptr else None, int(ld_p), 1 if borrow else 0, c_void_p(int(x_ptr)), c_void_p(int(y_ptr)),
            int(in_dim), int(out_dim), int(b), float(sigma_m), int(compute_dtype)))
        self._m, self._in, self._out, self._b, self._ni = int(m), int(in_dim), int(out_dim), int(b), int(n)

    def set_prior(self, sigma_p):
        """non-default include_prior (Q4): sigma_p > 0 adds logpdf(MvNormal(zeros(N), sigma_p), W_swa + P z); 0 = off"""
        self._check(self.lib.si_infer_set_prior(self.h, float(sigma_p)))

    def infer_set_likelihood(self, kind):
        """si_infer_set_likelihood, after infer_setup: SI_LIK_GAUSSIAN (0, the reference and every set-up's start), SI_LIK_CATEGORICAL
        (1: lp = -costs.numerator(LOGITCE, yhat, Y)) or SI_LIK_BERNOULLI (2: lp = -costs.numerator(LOGITBCE, yhat, Y)) on the model's
        outputs; sigma_m is unused then, the prior term stays as set_prior set it"""
        self._check(self.lib.si_infer_set_likelihood(self.h, int(kind)))

    def infer_likelihood_info(self):
        """the likelihood set: 0 gaussian, 1 categorical, 2 bernoulli"""
        k = c_int32(0)
        self._check(self.lib.si_infer_likelihood_info(self.h, byref(k)))
        return int(k.value)

    def set_decoder(self, table, wdec):
        """si_infer_set_decoder, after infer_setup: the density at W_swa + decoder(z) (autoencoder.py is the definition).  `table` is
        the decoder's Dense layer table (flux.layer_table), `wdec` its flat Float32 or Float64 parameter vector; it stays on the
        device in that element type.  table=None clears the decoder: the P route returns bit for bit."""
        if table is None:
            self._check(self.lib.si_infer_set_decoder(self.h, None, 0, 0, None, SI_F64))
            return
        wdec = np.ascontiguousarray(wdec)
        if wdec.dtype not in (np.float32, np.float64) or wdec.ndim != 1:
            raise SubspaceError("decoder parameters must be a flat Float32 or Float64 vector, got %s %s" % (wdec.dtype, wdec.shape))
        arr = _layer_array(table)
        self._check(self.lib.si_infer_set_decoder(self.h, arr, len(table), wdec.size, _ptr(wdec),
                                                  SI_F32 if wdec.dtype == np.float32 else SI_F64))

    def decoder_info(self):
        """(D, H, storage dtype) of the decoder set: layers (0: none), the last layer's input width, SI_F32 / SI_F64"""
        d, h, t = c_int32(0), c_int32(0), c_int32(0)
        self._check(self.lib.si_infer_decoder_info(self.h, byref(d), byref(h), byref(t)))
        return int(d.value), int(h.value), int(t.value)

    def decode(self, z):
        """decoder(z) alone for every column of the M x C matrix z: the N x C matrix (si_decode)"""
        z = _f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, 1, order="F")
        if z.ndim != 2 or z.shape[0] != self._m:
            raise SubspaceError("DimensionMismatch: z has %d rows, M = %d" % (z.shape[0], self._m))
        y = np.empty((self._ni, z.shape[1]), dtype=np.float64, order="F")
        self._check(self.lib.si_decode(self.h, _ptr(z), z.shape[1], _ptr(y)))
        return y

    def decode_vjp(self, z, gy):
        """J_decoder(z)' gy at the point z (M) for the cotangent gy (N): the M-vector (si_decode_vjp).  It runs the decoder's
        forward with its outputs kept and then the reverse kernels, launch for launch as logdensity_grad does."""
        z, gy = _f64(z).reshape(-1), _f64(gy).reshape(-1)
        if z.size != self._m or gy.size != self._ni:
            raise SubspaceError("DimensionMismatch: z has %d entries (M = %d), gy has %d (N = %d)" % (z.size, self._m, gy.size, self._ni))
        gz = np.empty(self._m, dtype=np.float64)
        self._check(self.lib.si_decode_vjp(self.h, _ptr(z), _ptr(gy), _ptr(gz)))
        return gz

    def infer_setup_node(self, table, n, m, w_swa, p, u0, y, ts, t0=0.0, reltol=1e-3, abstol=1e-6, dt=0.0, adaptive=True,
                         max_steps=100000, pre_power=1):
        """si_infer_setup_node, in place of infer_setup, for a NeuralODE (node.py is the definition): `table` is the Dense layer table
        of the right-hand side d -> ... -> d, u0 the initial states (d x f), y the observed trajectories (d*S x f, row i*S + s: state i
        at ts[s]), ts the S save times.  w_swa / p None => the finished construction."""
        arr = _layer_array(table)
        u0, y, ts = _f64(u0), _f64(y), np.ascontiguousarray(ts, dtype=np.float64).reshape(-1)
        if u0.ndim != 2 or y.ndim != 2 or u0.shape[1] != y.shape[1] or y.shape[0] != u0.shape[0] * ts.size:
            raise SubspaceError("DimensionMismatch: U0 is %s, Y is %s, %d save times: Y must be (d*S, f)" % (u0.shape, y.shape, ts.size))
        if w_swa is not None:
            w_swa = _f64(w_swa)
            p = _f64(p)
            if w_swa.shape != (n,) or p.shape != (n, m):
                raise SubspaceError("DimensionMismatch: W_swa %s, P %s, expected (%d,), (%d, %d)" % (w_swa.shape, p.shape, n, n, m))
        opts = SiNodeOpts(float(t0), float(reltol), float(abstol), float(dt), 1 if adaptive else 0, int(max_steps), int(pre_power))
        self._check(self.lib.si_infer_setup_node(self.h, arr, len(table), int(n), int(m), _ptr(w_swa), _ptr(p), _ptr(u0), _ptr(y),
                                                 u0.shape[0], ts.size, u0.shape[1], _ptr(ts), byref(opts)))
        self._m, self._in, self._out, self._b, self._ni = int(m), u0.shape[0], y.shape[0], u0.shape[1], int(n)

    def node_info(self):
        """(active, d, S, f, G): whether a NeuralODE set-up is active, its sizes and the lanes that share one trajectory"""
        on, d, s, g, f = c_int32(0), c_int32(0), c_int32(0), c_int32(0), c_int64(0)
        self._check(self.lib.si_node_info(self.h, byref(on), byref(d), byref(s), byref(f), byref(g)))
        return bool(on.value), int(d.value), int(s.value), int(f.value), int(g.value)

    def node_solve(self, z, want_u=True):
        """the trajectories at every column of z (M x C): (U (d*S, f, C) or None, sse (f, C), naccept, nreject, status (f, C) int32)"""
        z = _f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, 1, order="F")
        if z.ndim != 2 or z.shape[0] != self._m:
            raise SubspaceError("DimensionMismatch: z has %d rows, M = %d" % (z.shape[0], self._m))
        c = z.shape[1]
        u = np.empty((self._out, self._b, c), dtype=np.float64, order="F") if want_u else None
        sse = np.empty((self._b, c), dtype=np.float64, order="F")
        na, nr, st = (np.empty((self._b, c), dtype=np.int32, order="F") for _ in range(3))
        self._check(self.lib.si_node_solve(self.h, _ptr(z), c, _ptr(u), _ptr(sse), _ptr(na), _ptr(nr), _ptr(st)))
        return u, sse, na, nr, st

    def node_set_grad(self, on=True):
        """si_node_set_grad: the gradient through the solver (the discrete adjoint over the frozen accepted steps, node.logdensity_grad)
        for the NeuralODE set up; off after every infer_setup_node"""
        self._check(self.lib.si_node_set_grad(self.h, 1 if on else 0))

    def node_grad_info(self):
        """(on, chains per pass of launches under the workspace budget)"""
        on, cpp = c_int32(0), c_int32(0)
        self._check(self.lib.si_node_grad_info(self.h, byref(on), byref(cpp)))
        return bool(on.value), int(cpp.value)

    def node_grad(self, z):
        """si_node_grad at every column of z (M x C): (lp (C), d lp / dW with the prior term (N, C), its pull-back to z (M, C))"""
        z = _f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, 1, order="F")
        if z.ndim != 2 or z.shape[0] != self._m:
            raise SubspaceError("DimensionMismatch: z has %d rows, M = %d" % (z.shape[0], self._m))
        c = z.shape[1]
        lp = np.empty(c, dtype=np.float64)
        gw = np.empty((self._ni, c), dtype=np.float64, order="F")
        gz = np.empty((self._m, c), dtype=np.float64, order="F")
        self._check(self.lib.si_node_grad(self.h, _ptr(z), c, _ptr(lp), _ptr(gw), _ptr(gz)))
        return lp, gw, gz

    def node_tableau(self):
        """c, a, b~ and the interpolant's constants as the kernel holds them (node.TABLEAU's order)"""
        out = np.empty(57, dtype=np.float64)
        self._check(self.lib.si_node_tableau(_ptr(out)))
        return out

    def logdensity(self, z):
        z = _f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, 1, order="F")
        if z.shape[0] != self._m:
            raise SubspaceError("DimensionMismatch: z has %d rows, M = %d" % (z.shape[0], self._m))
        lp = np.empty(z.shape[1], dtype=np.float64)
        self._check(self.lib.si_logdensity(self.h, _ptr(z), z.shape[1], _ptr(lp)))
        return lp

    def logdensity_grad(self, z):
        z = _f64(z).reshape(-1)
        if z.size != self._m:
            raise SubspaceError("DimensionMismatch: z has %d elements, M = %d" % (z.size, self._m))
        lp = np.empty(1, dtype=np.float64)
        g = np.empty(self._m, dtype=np.float64)
        self._check(self.lib.si_logdensity_grad(self.h, _ptr(z), _ptr(lp), _ptr(g)))
        return float(lp[0]), g

    def logdensity_grad_batch(self, z):
        """(lp[C], G[M, C]): value and gradient at every column of the M x C matrix z in ONE call (si_logdensity_grad_batch)"""
        z = _f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, 1, order="F")
        if z.ndim != 2 or z.shape[0] != self._m:
            raise SubspaceError("DimensionMismatch: z has %d rows, M = %d" % (z.shape[0], self._m))
        lp = np.empty(z.shape[1], dtype=np.float64)
        g = np.empty((self._m, z.shape[1]), dtype=np.float64, order="F")
        self._check(self.lib.si_logdensity_grad_batch(self.h, _ptr(z), z.shape[1], _ptr(lp), _ptr(g)))
        return lp, g

    def grad_kernel_info(self):
        """1 when the last logdensity_grad_batch ran the fused narrow-chain kernel, 0 when it walked the per-point path"""
        f = c_int32(0)
        self._check(self.lib.si_grad_kernel_info(self.h, byref(f)))
        return int(f.value)

    def forward(self, z):
        z = _f64(z).reshape(-1)
        yhat = np.empty((self._out, self._b), dtype=np.float64, order="F")
        self._check(self.lib.si_forward(self.h, _ptr(z), _ptr(yhat)))
        return yhat

    def predict(self, z, xnew):
        z = _f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, 1, order="F")
        xnew = _f64(xnew)
        if z.shape[0] != self._m or xnew.ndim != 2 or xnew.shape[0] != self._in:
            raise SubspaceError("DimensionMismatch: Z %s, Xnew %s" % (z.shape, xnew.shape))
        out = np.empty((self._out, xnew.shape[1], z.shape[1]), dtype=np.float64, order="F")
        self._check(self.lib.si_predict(self.h, _ptr(z), z.shape[1], _ptr(xnew), xnew.shape[1], _ptr(out)))
        return out

    def sample_rwmh(self, itr, sigma_z, seed, chain_id0=0, nchains=1, want_z=True):
        z = np.empty((self._m, int(itr), int(nchains)), dtype=np.float64, order="F") if want_z else None
        lp = np.empty((int(itr), int(nchains)), dtype=np.float64, order="F")
        acc = np.empty(int(nchains), dtype=np.float64)
        self._check(self.lib.si_sample_rwmh(self.h, int(itr), float(sigma_z), int(seed), int(chain_id0), int(nchains),
                                            _ptr(z), _ptr(lp), _ptr(acc)))
        return z, lp, acc

    def sample_rwmh_weights(self, itr, sigma_z, seed, chain_id0=0, nchains=1, out=None):
        """si_sample_rwmh + the output map (:125) streamed while the chain runs: returns (z, lp, acc, W) with
        W of shape (N, itr, nchains), Fortran order -- W[:, t, c] == W_swa + P z[:, t, c]."""
        z = np.empty((self._m, int(itr), int(nchains)), dtype=np.float64, order="F")
        lp = np.empty((int(itr), int(nchains)), dtype=np.float64, order="F")
        acc = np.empty(int(nchains), dtype=np.float64)
        if out is None:
            w = np.empty((self._ni, int(itr), int(nchains)), dtype=np.float64, order="F")
        else:
            w = out
            if w.dtype != np.float64 or w.shape != (self._ni, int(itr), int(nchains)) or not w.flags.f_contiguous:
                raise ValueError("sample_rwmh_weights: `out` must be a Fortran-ordered float64 array of shape (N, itr, nchains)")
        self._check(self.lib.si_sample_rwmh_weights(self.h, int(itr), float(sigma_z), int(seed), int(chain_id0), int(nchains),
                                                    _ptr(z), _ptr(lp), _ptr(acc), _ptr(w)))
        return z, lp, acc, w

    def sample_mala(self, itr, sigma_z, seed, chain_id0=0, nchains=1, grad=False):
        """si_sample_mala: MALA with the chain state on the device, on the library's Philox streams.  Returns (z, lp, acc), and
        with grad=True (z, lp, acc, G) where G[:, t, c] = d lp / d z at z[:, t, c]."""
        z = np.empty((self._m, int(itr), int(nchains)), dtype=np.float64, order="F")
        lp = np.empty((int(itr), int(nchains)), dtype=np.float64, order="F")
        acc = np.empty(int(nchains), dtype=np.float64)
        g = np.empty((self._m, int(itr), int(nchains)), dtype=np.float64, order="F") if grad else None
        self._check(self.lib.si_sample_mala(self.h, int(itr), float(sigma_z), int(seed), int(chain_id0), int(nchains),
                                            _ptr(z), _ptr(lp), _ptr(acc), _ptr(g)))
        return (z, lp, acc, g) if grad else (z, lp, acc)

    def mala_kernel_info(self):
        """(fused, passes) of the last sample_mala: did it take the device-resident route, gradient passes per transition"""
        f, p = c_int32(0), c_int32(0)
        self._check(self.lib.si_mala_kernel_info(self.h, byref(f), byref(p)))
        return int(f.value), int(p.value)

    def sample_hmc(self, itr, sigma_z, seed, chain_id0=0, nchains=1, n_adapts=None, delta=0.8, grad=False, metric=False):
        """si_sample_hmc: the reference's one-step HMC under the Stan adaptor with position, momentum, step size, metric and adaptor
        state on the device, on the library's Philox streams.  n_adapts=None is the reference's Int(round(itr / 2)) (ties to even,
        like Python's round).  Returns (z, lp, alpha, eps) with itr + 1 columns -- column 0 is the initial state, alpha[t] the
        acceptance probability of transition t and eps[t] the step size it used -- then G (grad=True: d lp / d z at every state)
        and Minv (metric=True: the diagonal metric transition t used), each of z's shape."""
        itr, c = int(itr), int(nchains)
        na = int(round(itr / 2)) if n_adapts is None else int(n_adapts)
        cols = max(itr, 0) + 1
        z = np.empty((self._m, cols, max(c, 0)), dtype=np.float64, order="F")
        lp, alpha, eps = (np.empty((cols, max(c, 0)), dtype=np.float64, order="F") for _ in range(3))
        g = np.empty_like(z, order="F") if grad else None
        mi = np.empty_like(z, order="F") if metric else None
        self._check(self.lib.si_sample_hmc(self.h, itr, na, float(sigma_z), float(delta), int(seed), int(chain_id0), c, _ptr(z),
                                           _ptr(lp), _ptr(alpha), _ptr(eps), _ptr(g), _ptr(mi)))
        return (z, lp, alpha, eps) + ((g,) if grad else ()) + ((mi,) if metric else ())

    def hmc_kernel_info(self):
        """(fused, passes, search_rounds) of the last sample_hmc: did it take the device-resident route, gradient passes per
        transition, rounds of the synchronising step-size search (the evaluation at z_0 included)"""
        f, p, r = c_int32(0), c_int32(0), c_int32(0)
        self._check(self.lib.si_hmc_kernel_info(self.h, byref(f), byref(p), byref(r)))
        return int(f.value), int(p.value), int(r.value)

    def sample_nuts(self, itr, sigma_z, seed, chain_id0=0, nchains=1, n_adapts=None, delta=0.8, max_depth=10, max_dh=1000.0,
                    tree=True, grad=False, metric=False, leaf_cap=0):
        """si_sample_nuts: the reference's NUTS (multinomial sampling, generalised no-U-turn criterion) under the Stan adaptor with
        the trajectory tree, step size, metric and adaptor state on the device, on the library's Philox streams -- the transition
        of `samplers.nuts_iter`.  n_adapts=None is the reference's Int(round(itr / 2)).  Returns (z, lp, alpha, eps) with itr + 1
        columns as sample_hmc (alpha[t] = the mean acceptance over the leaves of transition t), then with tree=True (depth, nleaf,
        sel) -- doublings started, leapfrog steps, the leaf (1-based) that became the state or 0 -- then G (grad=True), Minv
        (metric=True) and, with leaf_cap > 0, the leaf log [3M+1, leaf_cap, C]: chain c's leaves in build order as (z, r, lp, g),
        NaN where nothing was logged."""
        itr, c = int(itr), int(nchains)
        na = int(round(itr / 2)) if n_adapts is None else int(n_adapts)
        cols = max(itr, 0) + 1
        z = np.empty((self._m, cols, max(c, 0)), dtype=np.float64, order="F")
        lp, alpha, eps = (np.empty((cols, max(c, 0)), dtype=np.float64, order="F") for _ in range(3))
        depth, nleaf, sel = (np.zeros((cols, max(c, 0)), dtype=np.int32, order="F") if tree else None for _ in range(3))
        g = np.empty_like(z, order="F") if grad else None
        mi = np.empty_like(z, order="F") if metric else None
        leaf = np.full((3 * self._m + 1, int(leaf_cap), max(c, 0)), np.nan, dtype=np.float64, order="F") if leaf_cap else None
        self._check(self.lib.si_sample_nuts(self.h, itr, na, float(sigma_z), float(delta), int(max_depth), float(max_dh), int(seed),
                                            int(chain_id0), c, _ptr(z), _ptr(lp), _ptr(alpha), _ptr(eps), _ptr(depth), _ptr(nleaf),
                                            _ptr(sel), _ptr(g), _ptr(mi), _ptr(leaf), int(leaf_cap)))
        return ((z, lp, alpha, eps) + ((depth, nleaf, sel) if tree else ()) + ((g,) if grad else ()) + ((mi,) if metric else ())
                + ((leaf,) if leaf_cap else ()))

    def nuts_kernel_info(self):
        """(fused, passes, search_rounds, rounds, leaves) of the last sample_nuts: route and passes as hmc_kernel_info, the rounds
        of all transitions and the leapfrog steps of all chains -- rounds * nchains - leaves is the lock-step waste"""
        f, p, r = c_int32(0), c_int32(0), c_int32(0)
        n, lv = c_int64(0), c_int64(0)
        self._check(self.lib.si_nuts_kernel_info(self.h, byref(f), byref(p), byref(r), byref(n), byref(lv)))
        return int(f.value), int(p.value), int(r.value), int(n.value), int(lv.value)

    def sample_ess(self, itr, sigma_z, seed, chain_id0=0, nchains=1, max_evals=128, trace=False):
        """si_sample_ess (not in the reference): elliptical slice sampling with the chain state on the device, on the library's
        Philox streams -- the transition of `samplers.ess_iter`.  The target is exp(logdensity(z)) N(z; 0, sigma_z^2 I): sigma_z is
        here the PRIOR's standard deviation on z, not a step size; lp[t] = logdensity(z[:, t]), the prior on z is not added.  `itr`
        counts the initial state.  Returns (z [M, itr, C], lp [itr, C]) and with trace=True also (nev, theta) [itr, C]: the
        evaluations transition t took (-max_evals: the cap was reached and the state kept) and the angle of the kept point."""
        itr, c = int(itr), int(nchains)
        z = np.empty((self._m, max(itr, 0), max(c, 0)), dtype=np.float64, order="F")
        lp = np.empty((max(itr, 0), max(c, 0)), dtype=np.float64, order="F")
        nev = np.zeros(lp.shape, dtype=np.int32, order="F") if trace else None
        theta = np.empty_like(lp, order="F") if trace else None
        self._check(self.lib.si_sample_ess(self.h, itr, float(sigma_z), int(max_evals), int(seed), int(chain_id0), c, _ptr(z), _ptr(lp),
                                           _ptr(nev), _ptr(theta)))
        return (z, lp, nev, theta) if trace else (z, lp)

    def ess_kernel_info(self):
        """(passes, rounds, evals) of the last sample_ess: passes of launches per evaluation, the synchronised rounds of all
        transitions and the density evaluations of all chains -- rounds * nchains - evals is the lock-step waste"""
        p, r, n = c_int32(0), c_int64(0), c_int64(0)
        self._check(self.lib.si_ess_kernel_info(self.h, byref(p), byref(r), byref(n)))
        return int(p.value), int(r.value), int(n.value)

    def fit_advi(self, max_iters, sigma_z, seed, samples_per_step=10, eta=0.1, tau=1.0, window=100, chain_id0=0, nruns=1,
                 ndraws=None, trace=False):
        """si_fit_advi: the reference's ADVI (src/space_inference.jl:126-138) with its state on the device, on the library's Philox
        streams; the defaults are the reference's ADVI(10, itr) and AdvancedVI's TruncatedADAGrad(0.1, 1.0, 100).  ndraws=None
        draws max_iters points from the fitted q, as the reference's rand(q, itr).  Returns (theta [2M, R], Z [M, D, R],
        elbo [T, R]), and with trace=True also (theta_trace [2M, T+1, R], points [M, S, T, R])."""
        t, s, w, r = int(max_iters), int(samples_per_step), int(window), int(nruns)
        d = t if ndraws is None else int(ndraws)
        why = advi_refusal(self._m, t, s, float(sigma_z), float(eta), float(tau), w, int(chain_id0), r, d)
        if why is not None:   # (before any array is sized by a refused value; the library refuses the same arguments)
            raise SubspaceError("si_fit_advi: bad argument (%s)" % why, SI_ERR_INVALID)
        m = self._m
        theta = np.empty((2 * m, r), dtype=np.float64, order="F")
        z = np.empty((m, d, r), dtype=np.float64, order="F")
        elbo = np.empty((t, r), dtype=np.float64, order="F")
        tr = np.empty((2 * m, t + 1, r), dtype=np.float64, order="F") if trace else None
        pts = np.empty((m, s, t, r), dtype=np.float64, order="F") if trace else None
        self._check(self.lib.si_fit_advi(self.h, t, s, float(sigma_z), float(eta), float(tau), w, int(seed), int(chain_id0), r, d,
                                         _ptr(theta), _ptr(z) if d > 0 else None, _ptr(elbo), _ptr(tr), _ptr(pts)))
        return (theta, z, elbo, tr, pts) if trace else (theta, z, elbo)

    def advi_kernel_info(self):
        """(fused, passes) of the last fit_advi: did it take the device-resident route, gradient passes per step"""
        f, p = c_int32(0), c_int32(0)
        self._check(self.lib.si_advi_kernel_info(self.h, byref(f), byref(p)))
        return int(f.value), int(p.value)

    def set_chain_loop(self, on):
        """False / 0: one launch per layer and per step of si_sample_rwmh; True / 1 (default): small and narrow Dense chains run
        fused and device-resident; 2: the one-launch density for narrow chains, but no device-resident loop; 3 / 4: as 1 / 2 with
        the generic kernels only (no run-time specialisation to the chain's shapes)."""
        self._check(self.lib.si_set_chain_loop(self.h, int(on)))

    def chain_kernel_info(self):
        """(density_specialised, loop_specialised, message): did the last density evaluation / si_sample_rwmh* call run the kernels
        compiled for this chain's shapes at run time (hiprtc), and if not, why"""
        d, l = c_int32(0), c_int32(0)
        self._check(self.lib.si_chain_kernel_info(self.h, byref(d), byref(l)))
        return bool(d.value), bool(l.value), (self.lib.si_chain_spec_message(self.h) or b"").decode()

    def rwmh_begin(self, itr, sigma_z, seed, chain_id0=0, nchains=1, d_total=0):
        self._check(self.lib.si_rwmh_begin(self.h, int(itr), float(sigma_z), int(seed), int(chain_id0), int(nchains),
                                           int(d_total)))
        self._sw = (int(itr), int(nchains))

    def rwmh_step_eval(self, on_device=False):
        """on_device: leave the partial sums in the library's device buffer (rwmh_sse_ptr) -- no copy, no sync."""
        if on_device:
            self._check(self.lib.si_rwmh_step_eval(self.h, None))
            return None
        sse = np.empty(self._sw[1], dtype=np.float64)
        self._check(self.lib.si_rwmh_step_eval(self.h, _ptr(sse)))
        return sse

    def rwmh_step_accept(self, sse_total=None):
        """sse_total None: the device buffer already holds the totals (all-reduced in place)."""
        if sse_total is None:
            self._check(self.lib.si_rwmh_step_accept(self.h, None))
            return
        sse_total = np.ascontiguousarray(sse_total, dtype=np.float64)
        self._check(self.lib.si_rwmh_step_accept(self.h, _ptr(sse_total)))

    def rwmh_sse_ptr(self):
        ptr, c = c_void_p(), c_int32()
        self._check(self.lib.si_rwmh_sse_ptr(self.h, byref(ptr), byref(c)))
        return int(ptr.value), int(c.value)

    def rwmh_abort(self):
        self._check(self.lib.si_rwmh_abort(self.h))

    def rwmh_end(self):
        itr, c = self._sw
        z = np.empty((self._m, itr, c), dtype=np.float64, order="F")
        lp = np.empty((itr, c), dtype=np.float64, order="F")
        acc = np.empty(c, dtype=np.float64)
        self._check(self.lib.si_rwmh_end(self.h, _ptr(z), _ptr(lp), _ptr(acc)))
        return z, lp, acc

    def reconstruct(self, z, out=None):
        """W_swa + P z for every column of z (space_inference.jl:125); `out` (N x C, Fortran order, float64) is filled in
        place when given (e.g. a buffer the caller reuses), else a new array is returned."""
        z = _f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, 1, order="F")
        if out is None:
            w = np.empty((self._ni, z.shape[1]), dtype=np.float64, order="F")
        else:
            w = out
            if w.dtype != np.float64 or w.shape != (self._ni, z.shape[1]) or not w.flags.f_contiguous:
                raise ValueError("reconstruct: `out` must be a Fortran-ordered float64 array of shape (N, C)")
        self._check(self.lib.si_reconstruct(self.h, _ptr(z), z.shape[1], _ptr(w)))
        return w


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it and ships it to the other ranks; needs no ctx)."""
    lib = load()
    buf = ctypes.create_string_buffer(SI_COMM_ID_BYTES)
    rc = lib.si_comm_unique_id(buf)
    if rc != SI_OK:
        raise SubspaceError(lib.si_last_error(None).decode(), rc)
    return buf.raw


def row_shard(n_total, rank, world):
    """si_row_shard: rows [r0, r1) of rank `rank` (32-element aligned boundaries) -- the partition the library assumes."""
    r0, r1 = c_int64(), c_int64()
    if load().si_row_shard(int(n_total), int(rank), int(world), byref(r0), byref(r1)) != SI_OK:
        raise SubspaceError("si_row_shard: bad argument")
    return int(r0.value), int(r1.value)


def host_hmc_windows(n_adapts):
    """si_host_hmc_windows: (window_start, window_end, [steps that close a window]) of si_sample_hmc's metric adaptation -- the
    schedule of samplers.StanAdaptor (needs no GPU)."""
    lib = load()
    ws, we = c_int64(), c_int64()
    n = lib.si_host_hmc_windows(int(n_adapts), byref(ws), byref(we), None, 0)
    splits = np.zeros(max(1, n), dtype=np.int64)
    lib.si_host_hmc_windows(int(n_adapts), byref(ws), byref(we), _ptr(splits), n)
    return int(ws.value), int(we.value), [int(v) for v in splits[:n]]


def host_sym_eig(g):
    """The host eigensolver of si_construct_finish (needs no GPU)."""
    lib = load()
    a = np.array(g, dtype=np.float64, order="F")
    n = a.shape[0]
    w = np.empty(n, dtype=np.float64)
    rc = lib.si_host_sym_eig(n, _ptr(a), _ptr(w))
    if rc != 0:
        raise SubspaceError("eigensolver did not converge")
    return w, a


def host_sym_eig_top(g, m):
    """The m largest eigenpairs by the fast host route of si_construct_finish (needs no GPU).  Returns
    (w_top descending, V n x m), or None when the route declines / fails its own verification."""
    lib = load()
    a = np.array(g, dtype=np.float64, order="F")
    n = a.shape[0]
    w = np.empty(int(m), dtype=np.float64)
    v = np.empty((n, int(m)), dtype=np.float64, order="F")
    rc = lib.si_host_sym_eig_top(n, _ptr(a), int(m), _ptr(w), _ptr(v))
    return (w, v) if rc == 0 else None


def host_jacobi_eig_psd(g):
    """Scaled-criterion Jacobi of the ill-conditioned route (needs no GPU): (w descending, V)."""
    lib = load()
    a = np.array(g, dtype=np.float64, order="F")
    n = a.shape[0]
    w = np.empty(n, dtype=np.float64)
    v = np.empty((n, n), dtype=np.float64, order="F")
    lib.si_host_jacobi_eig_psd(n, _ptr(a), _ptr(w), _ptr(v))
    return w, v
