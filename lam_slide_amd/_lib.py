"""ctypes binding of liblamslide_hip.so (include/lsl_api.h).

The HIP library is the only compute path of this package: importing works without it (so CPU-only
tooling can read shapes and pack weights), but every call that would run the network raises
``RuntimeError`` if the library is missing or the tensors are not on an AMD GPU.  There is no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from collections import OrderedDict
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblamslide_hip.so")
SRC_DIR = os.path.join(_HERE, "csrc")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

ABI_VERSION = 6  # LSL_VERSION of include/lsl_api.h this binding was written against
RK_SCRATCH_BYTES = 8192  # LSL_RK_SCRATCH_BYTES
GEOM_MAX_A, GEOM_MAX_D = 2048, 4  # the native form of lsl_geom_loss_sums (csrc/k_geomloss.hip.h)
DISP_MAX_D, DISP_MAX_UNITS = 4, 16777215  # the native form of lsl_disp_error_rows (csrc/k_disperr.hip.h): coordinates, K * B
TORS_MAX_A, TORS_MAX_Q, HIST_MAX_BINS, HIST2_MAX_BINS = 2044, 65536, 2048, 90  # the native forms of lsl_dihedral_angles / lsl_histogram (csrc/k_torsstat.hip.h)
LAG_CHUNK, LAG_MAX_LAGS, LAG_MAX_ROWS = 448, 1 << 21, 65535  # lsl_lag_products: the fp32 chain m, nlag + 1, S * C of one call
MOM_SEG = 1024  # lsl_lagged_moments (csrc/k_tica.hip.h): segment g holds the time steps [g * MOM_SEG, (g + 1) * MOM_SEG) below n - lag
MOM_CHAIN = MOM_SEG  # the longest fp64 addition chain inside a segment
MOM_MAX_F, PROJ_MAX_D = 128, 16  # the native forms of lsl_lagged_moments / lsl_project: features, output columns
ASG_MAX_K, ASG_MAX_D, ASG_CELLS, ASG_MAX_STATES, TR_MAX_STATES = 1024, 64, 8192, 1024, 128  # lsl_assign_centers, lsl_transition_counts
KM_SEG, KM_MAX_S = 2048, 65535  # lsl_kmeans_step (csrc/k_kmeans.hip.h): segment g holds the rows [g * KM_SEG, (g + 1) * KM_SEG); series of one call.  Its centres' limits are ASG_*
WMOM_MIN_F, WMOM_MAX_F, WPROJ_MAX_D = 129, 2048, 64  # the native form of lsl_weighted_moments / lsl_project_wide (csrc/k_wtica.hip.h): features, output columns
WMOM_SEG, WMOM_CHAIN = 1024, 4130  # lsl_weighted_moments: the rows of a segment, the roundings on the longest path to one entry
PAIR_MAX_P, CA_MAX_R = 65536, 146  # lsl_pair_distances / lsl_ca_frame_stats (csrc/k_structstat.hip.h): pairs of one call, selected atoms of a frame
SI_SLAB = 4096  # LSL_SI_SLAB: elements of one trajectory per partial sum of lsl_si_reduce
CLS_MAX_K, CLS_IGNORE = 128, -100  # lsl_class_loss_sums (csrc/k_classloss.hip.h): the classes of one call, the target of an ignored row

EXPORTED = (
    "lsl_version", "lsl_build_info", "lsl_last_error", "lsl_model_create", "lsl_model_set_weights", "lsl_model_destroy",
    "lsl_model_set_chunk", "lsl_model_set_attention_mode", "lsl_model_set_tail", "lsl_model_tail", "lsl_model_set_ln_fuse", "lsl_model_ln_fuse", "lsl_profile_kernel_name", "lsl_pass_size", "lsl_sampler_path", "lsl_workspace_bytes", "lsl_forward", "lsl_sample", "lsl_sample_ex", "lsl_debug_block", "lsl_debug_block_ex", "lsl_debug_taps", "lsl_debug_mods",
    "lsl_debug_mods_ex", "lsl_debug_mods_steps", "lsl_debug_embed", "lsl_debug_head",
    "lsl_si_loss_workspace_bytes", "lsl_si_loss", "lsl_si_reduce", "lsl_geom_loss_sums", "lsl_geom_loss_final",
    "lsl_peptide_loss_sums", "lsl_peptide_loss_final", "lsl_disp_error_rows", "lsl_disp_error_final",
    "lsl_dihedral_angles", "lsl_histogram", "lsl_lag_products_workspace_bytes", "lsl_lag_products", "lsl_js_distance",
    "lsl_pair_distances", "lsl_ca_frame_stats", "lsl_histogram_columns", "lsl_js_distance_density",
    "lsl_lagged_moments_workspace_bytes", "lsl_lagged_moments", "lsl_project", "lsl_assign_centers", "lsl_transition_counts",
    "lsl_kmeans_workspace_bytes", "lsl_kmeans_step", "lsl_kmeans_nearest_rows",
    "lsl_weighted_moments_workspace_bytes", "lsl_weighted_moments", "lsl_affine_weights", "lsl_project_wide",
    "lsl_msm_active_set", "lsl_msm_reversible_step", "lsl_msm_transition_matrix",
    "lsl_superpose", "lsl_atom_rmsf_workspace_bytes", "lsl_atom_rmsf",
    "lsl_profile_enable", "lsl_profile_read", "lsl_randn", "lsl_rk_lincomb", "lsl_rk_dense", "lsl_rk_error_ratio",
    "lsl_dopri_workspace_bytes", "lsl_dopri_begin", "lsl_dopri_advance", "lsl_debug_dopri_coeffs",
    "lsl_dopri_each_workspace_bytes", "lsl_dopri_each_begin", "lsl_dopri_each_advance",
    "lsl_dopri_logp_workspace_bytes", "lsl_dopri_logp_begin", "lsl_dopri_logp_advance", "lsl_rademacher",
    "lsl_forward_jvp_workspace_bytes", "lsl_forward_jvp", "lsl_dot_rows",
    "lsl_decoder_create", "lsl_decoder_destroy", "lsl_decode_workspace_bytes", "lsl_decode",
    "lsl_encoder_create", "lsl_encoder_destroy", "lsl_encode_workspace_bytes", "lsl_encode",
    "lsl_decode_heads", "lsl_class_loss_sums", "lsl_class_loss_final",
)


def mom_segments(n: int, lag: int) -> int:
    """The segment rule of lsl_lagged_moments: the number of segments of a series of n steps at this lag."""
    return -(-(int(n) - int(lag)) // MOM_SEG)


class ModelDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_dim", "hidden", "heads", "head_dim", "head_dim_pad", "mlp_dim", "depth",
                                         "vec_in_dim", "normalize")] + [("theta", C.c_float)]


class BlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "qs", "ks", "w2", "b2")]


class Weights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "x_in_w", "x_in_b", "cond_w", "cond_b", "mask_emb", "time_freqs", "time_w1", "time_b1", "time_w2", "time_b2",
        "vec_w1", "vec_b1", "vec_w2", "vec_b2", "mod_w", "mod_b", "out_w", "out_b")] + [("blocks", C.POINTER(BlockWeights))]


class IO(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_cond", C.c_void_p), ("mask", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p),
                ("out", C.c_void_p), ("B", C.c_int32), ("T", C.c_int32), ("L", C.c_int32)]


class DecBlock(C.Structure):  # lsl_dec_block
    _fields_ = [(n, C.c_void_p) for n in ("ln_w", "ln_b", "lnc_w", "lnc_b", "w_q", "w_kv", "w_out", "b_out", "q_scale", "k_scale",
                                          "ff_ln_w", "ff_ln_b", "ff_w1", "ff_b1", "ff_w2", "ff_b2")]


class DecoderDesc(C.Structure):  # lsl_decoder_desc
    _fields_ = [(n, C.c_int32) for n in ("in_dim", "dim_latent", "dim_query", "dim_emb", "n_entities", "heads_latent", "dim_head_latent",
                                         "heads_cross", "dim_head_cross", "num_block_attn", "num_block_cross", "act", "out_dim", "num_split")]


class DecoderWeights(C.Structure):  # lsl_decoder_weights
    _fields_ = [("pq_w", C.c_void_p), ("pq_b", C.c_void_p), ("table", C.c_void_p), ("qm_w", C.c_void_p), ("qm_b", C.c_void_p),
                ("self_blocks", C.POINTER(DecBlock)), ("cross_blocks", C.POINTER(DecBlock)), ("out_block", DecBlock),
                ("ext_w", C.c_void_p), ("ext_b", C.c_void_p), ("head_w1", C.c_void_p), ("head_b1", C.c_void_p), ("head_w2", C.c_void_p), ("head_b2", C.c_void_p)]


class DecoderHead(C.Structure):  # lsl_decoder_head
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("out_dim", C.c_int32)]


class EncoderDesc(C.Structure):  # lsl_encoder_desc
    _fields_ = [(n, C.c_int32) for n in ("dim_input", "dim_emb", "n_entities", "dim_latent", "num_latents", "heads_cross", "dim_head_cross",
                                         "heads_latent", "dim_head_latent", "num_block_cross", "num_block_attn", "act")]


class EncoderWeights(C.Structure):  # lsl_encoder_weights
    _fields_ = [("table", C.c_void_p), ("mlp_w1", C.c_void_p), ("mlp_b1", C.c_void_p), ("mlp_w2", C.c_void_p), ("mlp_b2", C.c_void_p),
                ("latents", C.c_void_p), ("cross_blocks", C.POINTER(DecBlock)), ("self_blocks", C.POINTER(DecBlock)),
                ("quant_w", C.c_void_p), ("quant_b", C.c_void_p)]


class Step(C.Structure):
    _fields_ = [("t", C.c_float), ("ax", C.c_float), ("am", C.c_float), ("aw", C.c_float)]


class StepEx(C.Structure):  # lsl_step_ex
    _fields_ = [("t", C.c_float), ("ax", C.c_float), ("am", C.c_float), ("aw", C.c_float), ("as_", C.c_float), ("flags", C.c_int32),
                ("noise_index", C.c_int32), ("trace_index", C.c_int32)]


class SiRow(C.Structure):  # lsl_si_row
    _fields_ = [(n, C.c_float) for n in ("alpha", "sigma", "p", "q1", "q0", "w")]


STEP_NO_NETWORK, STEP_SAVE = 1, 2


class DopriDesc(C.Structure):  # lsl_dopri_desc
    _fields_ = [(n, C.c_int32) for n in ("path_type", "model_type", "reverse", "max_steps")] + [("rtol", C.c_double), ("atol", C.c_double)]


class DopriCtl(C.Structure):  # lsl_dopri_ctl
    _fields_ = [(n, C.c_double) for n in ("t", "dt", "t_lo", "ratio", "t_new", "dt_next", "rtol", "atol")] + [("out", C.c_void_p)] + [
        (n, C.c_int32) for n in ("accept", "out_end", "accepted", "rejected", "nfe", "next_out", "done", "status", "n_out", "max_steps", "path_type",
                                 "model_type", "reverse")]


class DopriEachSummary(C.Structure):  # lsl_dopri_each_summary
    _fields_ = [(n, C.c_int32) for n in ("B", "n_done", "n_failed", "max_attempts", "done")]


class Dopri:
    """The constants of lsl_dopri_* (include/lsl_api.h; tests/test_dopri5_controller.py holds them against the header)."""
    MAX_ATTEMPTS = 100000  # LSL_DOPRI_MAX_ATTEMPTS
    CTL_OFFSET, LOG_OFFSET, STATE_OFFSET = 0, 256, 256 + 32 * MAX_ATTEMPTS  # LSL_DOPRI_*_OFFSET
    PATHS = {"LINEAR": 0, "GVP": 1, "VP": 2}  # LSL_PATH_*
    PREDICTIONS = {"VELOCITY": 0, "DATA": 1, "NOISE": 2, "SCORE": 3}  # LSL_PRED_*
    STATUS_MAX_STEPS, STATUS_NON_FINITE = 1, 2  # lsl_dopri_ctl.status
    # lsl_dopri_each_*: the head of the workspace (tests/test_dopri5_each.py holds these against the header's macros)
    EACH_SUMMARY_OFFSET, EACH_CTL_OFFSET, EACH_CTL_STRIDE, EACH_MAX_B = 0, 256, 128, 65535

    @staticmethod
    def each_log_offset(B: int) -> int:  # LSL_DOPRI_EACH_LOG_OFFSET
        return 256 + 256 * ((128 * int(B) + 255) // 256)

    @staticmethod
    def each_state_offset(B: int, log_rows: int) -> int:  # LSL_DOPRI_EACH_STATE_OFFSET
        return Dopri.each_log_offset(B) + 256 * ((32 * int(B) * int(log_rows) + 255) // 256)

    NEGATED = 2  # LSL_DOPRI_NEGATED: the bit of lsl_dopri_ctl.reverse an augmented solve (lsl_dopri_logp_*) sets

    @staticmethod
    def logp_side_offset(state_offset: int, n_state: int) -> int:  # LSL_DOPRI_LOGP_SIDE_OFFSET
        return int(state_offset) + 256 * ((4 * int(n_state) + 255) // 256)


# The translation units of the library and the compile options each adds to BASE_FLAGS: a unit per family of entry points (the sampling
# path, the losses, the evaluation statistics, the frozen stage 1), plus a unit where a kernel's best options differ (csrc/unit_lin1.hip:
# profiles/lin1_unit.txt).  The families share no state and no kernel; no device call crosses units (no -fgpu-rdc).
BASE_FLAGS = ("-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wno-unused-value")
UNITS = (("lsl_api.hip", ()), ("unit_lin1.hip", ("-fno-slp-vectorize",)), ("unit_loss.hip", ()), ("unit_stat.hip", ()), ("unit_stage1.hip", ()))
BUILD_DIR = os.path.join(_HERE, "build")  # the units' object files


def unit_options(extra) -> str:
    """What lsl_build_info() reports for a unit: the options of every unit, then its own."""
    return " ".join(BASE_FLAGS[:1] + tuple(extra))


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 into the in-tree shared library (hipcc cross-compiles without a GPU): one object per unit of UNITS,
    compiled side by side (at most 16 compiler jobs), linked into one library."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(SRC_DIR, f) for f in sorted(os.listdir(SRC_DIR))] + [os.path.join(INCLUDE_DIR, "lsl_api.h"), os.path.abspath(__file__)]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(BUILD_DIR, exist_ok=True)

    def run(cmd):
        res = subprocess.run(cmd, capture_output=True, text=True)
        if verbose or res.returncode != 0:
            print(" ".join(cmd))
            print(res.stdout + res.stderr)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed building liblamslide_hip.so")

    objs = [os.path.join(BUILD_DIR, os.path.splitext(name)[0] + ".o") for name, _ in UNITS]
    cmds = [[hipcc, *BASE_FLAGS, *extra, f'-DLSL_UNIT_OPTIONS="{unit_options(extra)}"', "-c", os.path.join(SRC_DIR, name), "-o", obj]
            for (name, extra), obj in zip(UNITS, objs)]
    with ThreadPoolExecutor(max_workers=min(16, len(cmds))) as pool:
        list(pool.map(run, cmds))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(SRC_DIR, "exports.map"), "-o", LIB_PATH, *objs])
    return LIB_PATH


class LibraryMissing(RuntimeError):
    """liblamslide_hip.so has not been built (the only failure a caller may treat as "no library": anything else - a HIP error, an
    out-of-memory condition - propagates)."""


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the library or fail loudly: the HIP path is the product, there is nothing to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP extension is the only compute path of lam_slide_amd)")
    lib = C.CDLL(LIB_PATH)
    # LSL_VERSION stayed 6 when entry points were added without changing a signature: a library built before them is found by the symbols
    missing = [s for s in EXPORTED if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"{LIB_PATH} is stale: it lacks {', '.join(missing)}; rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
    lib.lsl_version.restype = C.c_int
    lib.lsl_build_info.restype = C.c_char_p
    lib.lsl_last_error.restype = C.c_char_p
    lib.lsl_model_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]
    lib.lsl_model_set_weights.argtypes = [C.c_void_p, C.POINTER(Weights)]
    lib.lsl_model_destroy.argtypes = [C.c_void_p]
    lib.lsl_model_destroy.restype = None
    lib.lsl_model_set_chunk.argtypes = [C.c_void_p, C.c_int32]
    lib.lsl_model_set_attention_mode.argtypes = [C.c_void_p, C.c_int32]
    lib.lsl_model_set_tail.argtypes = [C.c_void_p, C.c_int32]
    lib.lsl_model_tail.argtypes = [C.c_void_p]
    lib.lsl_model_set_ln_fuse.argtypes = [C.c_void_p, C.c_int32]
    lib.lsl_model_ln_fuse.argtypes = [C.c_void_p]
    lib.lsl_profile_kernel_name.argtypes = [C.c_void_p]
    lib.lsl_profile_kernel_name.restype = C.c_char_p
    lib.lsl_pass_size.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.lsl_sampler_path.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.lsl_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.lsl_workspace_bytes.restype = C.c_size_t
    lib.lsl_forward.argtypes = [C.c_void_p, C.POINTER(IO), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_sample.argtypes = [C.c_void_p, C.POINTER(IO), C.POINTER(Step), C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64,
                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_sample_ex.argtypes = [C.c_void_p, C.POINTER(IO), C.POINTER(StepEx), C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint64,
                                  C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_debug_block.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_debug_block_ex.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_debug_taps.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_debug_mods.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]
    lib.lsl_debug_mods_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_debug_mods_steps.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_debug_embed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [
        C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_debug_head.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(StepEx), C.c_void_p, C.c_uint64,
                                   C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.lsl_forward_jvp_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.lsl_forward_jvp_workspace_bytes.restype = C.c_size_t
    lib.lsl_forward_jvp.argtypes = [C.c_void_p, C.POINTER(IO), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_dot_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_si_loss_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.lsl_si_loss_workspace_bytes.restype = C.c_size_t
    lib.lsl_si_loss.argtypes = [C.c_void_p, C.POINTER(IO), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_si_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_void_p]
    lib.lsl_geom_loss_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_geom_loss_final.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_peptide_loss_sums.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_peptide_loss_final.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_disp_error_rows.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 9 + [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lsl_disp_error_final.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lsl_dihedral_angles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_histogram.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_lag_products_workspace_bytes.argtypes = [C.c_int32] * 4
    lib.lsl_lag_products_workspace_bytes.restype = C.c_size_t
    lib.lsl_lag_products.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_js_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_pair_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_ca_frame_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float] + [C.c_void_p] * 5
    lib.lsl_histogram_columns.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_js_distance_density.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
    lib.lsl_lagged_moments_workspace_bytes.argtypes = [C.c_int32] * 4
    lib.lsl_lagged_moments_workspace_bytes.restype = C.c_size_t
    lib.lsl_lagged_moments.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_project.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lsl_assign_centers.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lsl_transition_counts.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]
    lib.lsl_weighted_moments_workspace_bytes.argtypes = [C.c_int32] * 3
    lib.lsl_weighted_moments_workspace_bytes.restype = C.c_size_t
    lib.lsl_weighted_moments.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_affine_weights.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.lsl_project_wide.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lsl_kmeans_workspace_bytes.argtypes = [C.c_int32] * 4
    lib.lsl_kmeans_workspace_bytes.restype = C.c_size_t
    lib.lsl_kmeans_step.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_double, C.c_double,
                                    C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_kmeans_nearest_rows.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_msm_active_set.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lsl_msm_reversible_step.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_double, C.c_int32] + [C.c_void_p] * 5
    lib.lsl_msm_transition_matrix.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lsl_superpose.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    lib.lsl_atom_rmsf_workspace_bytes.argtypes = [C.c_int64, C.c_int32]
    lib.lsl_atom_rmsf_workspace_bytes.restype = C.c_size_t
    lib.lsl_atom_rmsf.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_randn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.lsl_rk_lincomb.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.c_int32, C.c_uint64, C.c_void_p]
    lib.lsl_rk_dense.argtypes = [C.c_void_p] * 6 + [C.c_float, C.c_uint64, C.c_void_p]
    lib.lsl_rk_error_ratio.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_float,
                                       C.c_uint64, C.c_void_p, C.c_void_p]
    lib.lsl_dopri_workspace_bytes.argtypes = [C.c_void_p] + [C.c_int32] * 4
    lib.lsl_dopri_workspace_bytes.restype = C.c_size_t
    lib.lsl_dopri_begin.argtypes = [C.c_void_p, C.POINTER(IO), C.POINTER(DopriDesc), C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p]
    lib.lsl_dopri_advance.argtypes = [C.c_void_p, C.POINTER(IO), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_dopri_each_workspace_bytes.argtypes = [C.c_void_p] + [C.c_int32] * 5
    lib.lsl_dopri_each_workspace_bytes.restype = C.c_size_t
    lib.lsl_dopri_each_begin.argtypes = [C.c_void_p, C.POINTER(IO), C.POINTER(DopriDesc), C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_size_t, C.c_void_p]
    lib.lsl_dopri_each_advance.argtypes = [C.c_void_p, C.POINTER(IO), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_dopri_logp_workspace_bytes.argtypes = [C.c_void_p] + [C.c_int32] * 6
    lib.lsl_dopri_logp_workspace_bytes.restype = C.c_size_t
    lib.lsl_dopri_logp_begin.argtypes = [C.c_void_p, C.POINTER(IO), C.POINTER(DopriDesc), C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_dopri_logp_advance.argtypes = [C.c_void_p, C.POINTER(IO), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_rademacher.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.lsl_debug_dopri_coeffs.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_profile_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.lsl_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.lsl_decoder_create.argtypes = [C.POINTER(DecoderDesc), C.POINTER(DecoderWeights), C.POINTER(C.c_void_p)]
    lib.lsl_decoder_destroy.argtypes = [C.c_void_p]
    lib.lsl_decoder_destroy.restype = None
    lib.lsl_decode_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.lsl_decode_workspace_bytes.restype = C.c_size_t
    lib.lsl_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p]
    lib.lsl_decode_heads.argtypes = [C.c_void_p, C.POINTER(DecoderHead), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]
    lib.lsl_class_loss_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    lib.lsl_class_loss_final.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lsl_encoder_create.argtypes = [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), C.POINTER(C.c_void_p)]
    lib.lsl_encoder_destroy.argtypes = [C.c_void_p]
    lib.lsl_encoder_destroy.restype = None
    lib.lsl_encode_workspace_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.lsl_encode_workspace_bytes.restype = C.c_size_t
    lib.lsl_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p]
    if lib.lsl_version() != ABI_VERSION:
        raise RuntimeError(f"liblamslide_hip.so reports ABI version {lib.lsl_version()}, this package binds version {ABI_VERSION}: rebuild it "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    _lib = lib
    return lib


def last_error() -> str:
    return load().lsl_last_error().decode()


def check(rc: int):
    if rc == 0:
        return
    msg = last_error()
    if rc in (-3, -20, -21):
        raise ValueError(msg)
    raise RuntimeError(f"lamslide_hip error {rc}: {msg}")


def call(dev, name: str, *args) -> None:
    """Run the compute entry point ``name`` of the library on ``dev``: inside that device's context, on its current stream (every such
    entry point takes the stream last), the return code through :func:`check`.  Handle calls without a stream (create, destroy, ``set_*``,
    ``*_workspace_bytes``) stay ``check(load().f(...))``."""
    fn = getattr(load(), name)
    with torch.cuda.device(dev):
        check(fn(*args, torch.cuda.current_stream(dev).cuda_stream))


def to_host(t: "torch.Tensor"):
    """A device tensor as a numpy array.  One of the documented synchronising copies of a fit: allowed under
    ``torch.cuda.set_sync_debug_mode("error")`` by switching to "default" around this copy alone."""
    if not t.is_cuda:
        return t.numpy()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("default")
    try:
        return t.cpu().numpy()
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def to_device(a, dev) -> "torch.Tensor":
    """A host array on ``dev``: the way back of :func:`to_host`, with the same exception."""
    import numpy as np
    t = torch.from_numpy(np.ascontiguousarray(a))
    if torch.device(dev).type != "cuda":
        return t
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("default")
    try:
        return t.to(dev)
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def device_form(*tensors, dtype=torch.float32, same_device: bool = True) -> bool:
    """The dispatch rule of every device form: all tensors on one GPU, all of ``dtype`` (the torch paths promote as the reference does),
    none requiring grad under grad mode (a library result carries no grad_fn).  The callers add their own shape or module clause.
    ``same_device=False`` leaves the comparison of the devices to a caller whose argument check raises the reference's "Expected all
    tensors to be on the same device" instead."""
    dev, grad = tensors[0].device, torch.is_grad_enabled()
    return all(t.is_cuda and t.dtype == dtype and (t.device == dev or not same_device) and not (grad and t.requires_grad) for t in tensors)


def flat(x, lead: tuple, trailing: tuple, dtype, dev, shape_error, device_error) -> "torch.Tensor":
    """One input of a loss entry point made canonical: ``ValueError(shape_error())`` unless x is [*lead, *trailing],
    ``RuntimeError(device_error())`` unless it is on ``dev``; then detached, the leading axes flattened into one, cast to ``dtype``
    (uint8: nonzero -> 1) and contiguous - these inputs come out of rearranges and slices, and the library reads dense rows."""
    if tuple(x.shape) != tuple(lead) + tuple(trailing):
        raise ValueError(shape_error())
    if x.device != dev:
        raise RuntimeError(device_error())
    x = x.detach().reshape(-1, *trailing)
    return (x != 0 if dtype == torch.uint8 else x).to(dtype).contiguous()


def loss_from_sums(fn: str, entry: str, widths: tuple, n_out: int, sums, required: tuple, optional: tuple, compute, needs: str,
                   takes: Optional[str] = None) -> "torch.Tensor":
    """The ``sums=`` bracket of geom_losses / class_losses / peptide_losses: either the tensors (none of ``required`` is ``None``; then
    ``compute()`` makes the sums) or ``sums=``, never both; the per-frame sums - one float32 [F, w] table per width, all on one GPU -
    finished by one call of ``entry``.  Returns its float32 [n_out] output."""
    if sums is None:
        if any(x is None for x in required):
            raise TypeError(f"{fn} needs {needs} or sums=")
        sums = compute()
    elif any(x is not None for x in required + optional):
        raise TypeError(f"{fn} takes {takes or needs} or sums=, not both")
    tables = sums if isinstance(sums, (tuple, list)) else (sums,)
    ok = len(tables) == len(widths) and all(t.dim() == 2 and t.shape[1] == w and t.shape[0] == tables[0].shape[0] > 0 and t.dtype == torch.float32
                                            and t.device == tables[0].device for t, w in zip(tables, widths))
    if not ok:
        one = len(widths) == 1
        raise ValueError(f"sums must be float32 {'' if one else '('}{', '.join(f'[F, {w}]' for w in widths)}{'' if one else ')'} with F > 0"
                         f"{'' if one else ' on one device'}, got " + " and ".join(f"{t.dtype} {tuple(t.shape)}" for t in tables))
    if not tables[0].is_cuda:
        raise RuntimeError(f"{fn} runs on the GPU (HIP kernel); there is no CPU fallback")
    tables = [t.contiguous() for t in tables]
    out = torch.empty(n_out, dtype=torch.float32, device=tables[0].device)
    call(out.device, entry, *(t.data_ptr() for t in tables), tables[0].shape[0], out.data_ptr())
    return out


class Scratch:
    """The scratch buffers of one owner object (a model, a stage-1 handle): one uint8 buffer per (device, current stream), so two calls
    of the owner in flight on different streams never share scratch (calls on ONE stream are ordered by the stream).  A buffer is replaced
    when a call needs more; the ``keep`` most recently used are kept."""

    def __init__(self, keep: int = 4):
        self.keep = keep
        self.buffers: "OrderedDict[tuple, torch.Tensor]" = OrderedDict()

    def get(self, device, need: int) -> "torch.Tensor":
        device = torch.device(device)
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        ws = self.buffers.get(key)
        if ws is None or ws.numel() < need:
            ws = self.buffers[key] = torch.empty(need, dtype=torch.uint8, device=device)
        self.buffers.move_to_end(key)
        while len(self.buffers) > self.keep:
            self.buffers.popitem(last=False)
        return ws
