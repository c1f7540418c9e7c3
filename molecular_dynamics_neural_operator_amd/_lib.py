"""ctypes binding of libmdno.so (include/mdno.h).  No CPU fallback exists: if the library is
missing, or a tensor is not on the GPU, the call raises."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MDNO_LIB", _HERE / "libmdno.so"))

OK, EINVAL, ELAUNCH, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -4
AGGR = {"add": 0, "mean": 1, "max": 2}      # "max": mdno_nnconv_fwd (stand-alone conv) and mdno_nnconv_msg_grad
STATUS_EDGE_OVERFLOW, STATUS_BAD_AMINOACID = 1, 2
ABI_VERSION = 15
GEMM_MODES = {"split_bf16": 0, "f32": 1, "split_f16": 2}
CONV_MODES = {"materialized": 0, "factored": 1, "auto": 2}
STATUS_BAD_EDGE_INDEX = 16


class MdnoError(RuntimeError):
    pass


class MdnoIndexError(MdnoError, IndexError):
    """An index the reference's nn.Embedding / index_select / scatter would reject with IndexError."""


class KernelNNParams(C.Structure):
    """struct mdno_kernelnn_params"""
    _INTS = ["width", "ker_width", "depth", "ker_in", "in_width", "out_width",
             "num_embeddings", "embedding_dim", "x_position_dim", "gemm_mode", "conv_mode", "reserved0"]
    _PTRS = ["lstm_w_ih", "lstm_w_hh", "lstm_b_ih", "lstm_b_hh", "lstm_fc_w", "lstm_fc_b", "emb_w",
             "fc1_w", "fc1_b", "k_w0", "k_b0", "k_w1", "k_b1", "k_w2", "k_b2",
             "k2_w0", "k2_b0", "k2_w1", "k2_b1", "k2_w2", "k2_b2",
             "conv1_root", "conv1_bias", "conv2_root", "conv2_bias", "fc2_w", "fc2_b"]
    _fields_ = [(n, C.c_int32) for n in _INTS] + [(n, C.c_void_p) for n in _PTRS]


_P = C.c_void_p
_I = C.c_int
_L = C.c_int64
_SZ = C.c_size_t
_D = C.c_double

# One table per public header, name -> (restype, argtypes); TABLES below pairs each with its header and states the
# contract they all keep.  Beside a table stands only what is particular to it.

# include/mdno.h
SIGNATURES = {
    "mdno_abi_version": (_I, []),
    "mdno_last_error": (C.c_char_p, []),
    "mdno_build_id": (C.c_char_p, []),
    "mdno_radius_graph_csr": (_I, [_P, _I, _I, _D, _P, _P, _P, _L, _P, _P, _P]),
    "mdno_radius_graph_workspace_bytes": (_SZ, [_I, _I]),
    "mdno_radius_graph_csr_ws": (_I, [_P, _I, _I, _D, _P, _P, _P, _L, _P, _P, _P, _SZ, _P]),
    "mdno_coo_to_csr_workspace_bytes": (_SZ, [_L, _I]),
    "mdno_coo_to_csr": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "mdno_csr_by_source": (_I, [_P, _P, _L, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "mdno_permute_rows": (_I, [_P, _P, _L, _I, _P, _P]),
    "mdno_edge_mlp_workspace_bytes": (_SZ, [_I, _I, _L, _I]),
    "mdno_edge_mlp_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _SZ,
                               _P]),
    "mdno_nnconv_fwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "mdno_node_prologue_fwd": (_I, [C.POINTER(KernelNNParams), _P, _I, _I, _I, _P, _I, _P, _P, _P]),
    "mdno_fc_out_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    "mdno_kernelnn_workspace_bytes": (_SZ, [C.POINTER(KernelNNParams), _I, _I, _L]),
    "mdno_resolve_conv_mode": (_I, [C.POINTER(KernelNNParams), _I, _L]),
    "mdno_conv_mode_for_graph": (_I, [C.POINTER(KernelNNParams), _I, _I, _L]),
    "mdno_kernelnn_fwd": (_I, [C.POINTER(KernelNNParams), _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _L,
                               _P, _P, _P, _P, _P, _P, _SZ, _P, _P]),
    "mdno_rollout_workspace_bytes": (_SZ, [C.POINTER(KernelNNParams), _I, _I, _L]),
    "mdno_rollout": (_I, [C.POINTER(KernelNNParams), _P, _I, _I, _I, _I, _P, _I, _D, _L, _P, _SZ, _P, _P, _I, _P]),
    "mdno_rollout_plan_create": (_I, [C.POINTER(_P), C.POINTER(KernelNNParams), _P, _I, _I, _I, _I, _P, _I, _D, _L,
                                      _P, _SZ, _P, _P, _I, _P]),
    "mdno_rollout_plan_run": (_I, [_P, _I, _I, _P]),
    "mdno_rollout_plan_steps_per_launch": (_I, [_P]),
    "mdno_rollout_plan_destroy": (_I, [_P]),
    "mdno_rollout_plan_timer_attach": (_I, [_P, _I]),
    "mdno_rollout_plan_timer_read": (_I, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mdno_rollout_plan_timer_detach": (_I, [_P]),
    "mdno_rollout_plan_fallback_counts": (_I, [_P, _P, _P]),
    "mdno_kernelnn_fallback_counts": (_I, [C.POINTER(KernelNNParams), _I, _I, _L, _I, _P, _P, _P]),
    "mdno_adam_step": (_I, [_I, _P, _D, _D, _D, _D, _D, _L, _P]),
    "mdno_pack_tensors": (_I, [_I, _P, _P, _P]),
    "mdno_unpack_tensors": (_I, [_I, _P, _P, _P]),
    "mdno_linear_fwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P]),
    "mdno_linear_split_workspace_bytes": (_SZ, [_L, _I, _I]),
    "mdno_linear_split_fwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P, _SZ, _P]),
    "mdno_gemm_atb_split_f16_supported": (_I, [_L, _I, _I]),
    "mdno_gemm_atb_split_f16_workspace_bytes": (_SZ, [_L, _I, _I]),
    "mdno_gemm_atb_split_f16": (_I, [_P, _P, _L, _I, _I, _P, _I, _P, _SZ, _P]),
    "mdno_linear_split_f16_workspace_bytes": (_SZ, [_L, _I, _I]),
    "mdno_linear_split_f16_fwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P, _SZ, _P]),
    "mdno_reduce_workspace_bytes": (_SZ, [_I, _I]),
    "mdno_gemm_atb": (_I, [_P, _P, _L, _I, _I, _P, _I, _P, _SZ, _P]),
    "mdno_colsum": (_I, [_P, _L, _I, _P, _I, _P, _SZ, _P]),
    "mdno_relu_bwd": (_I, [_P, _P, _P, _L, _I, _P, _P]),
    "mdno_relu_bwd2": (_I, [_P, _P, _P, _L, _I, _P, _P, _P]),
    "mdno_transpose": (_I, [_P, _I, _I, _P, _P]),
    "mdno_inv_degree": (_I, [_P, _I, _I, _P, _P]),
    "mdno_nnconv_bwd_x": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P]),
    "mdno_nnconv_bwd_root_workspace_bytes": (_SZ, [_L]),
    "mdno_nnconv_bwd_root": (_I, [_P, _P, _L, _I, _I, _P, _P, _I, _P, _SZ, _P]),
    "mdno_nnconv_bwd_root_pair_workspace_bytes": (_SZ, [_L]),
    "mdno_nnconv_bwd_root_pair": (_I, [_P, _P, _L, _P, _P, _P, _P, _P, _SZ, _P]),
    "mdno_nnconv_bwd_we": (_I, [_P, _P, _P, _P, _L, _I, _L, _I, _I, _P, _I, _P]),
    "mdno_cast_bf16": (_I, [_P, _L, _P, _P]),
    "mdno_linear_smallk_bf16_fwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P]),
    "mdno_linear_bf16_workspace_bytes": (_SZ, [_I, _I]),
    "mdno_linear_bf16_fwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    "mdno_linear_bf16_masked_supported": (_I, [_L, _I, _I]),
    "mdno_linear_bf16_masked": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _SZ, _P]),
    "mdno_gemm_atb_bf16_workspace_bytes": (_SZ, [_I, _I]),
    "mdno_gemm_atb_bf16": (_I, [_P, _P, _L, _I, _I, _P, _P, _SZ, _P]),
    "mdno_nnconv_bf16w_fwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _P]),
    "mdno_nnconv_bwd_x_bf16w": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mdno_nnconv_bwd_we_bf16": (_I, [_P, _P, _P, _P, _L, _I, _L, _P, _P]),
    "mdno_nnconv_bwd_we_bf16_colsum_workspace_bytes": (_SZ, []),
    "mdno_nnconv_bwd_we_colsum_workspace_bytes": (_SZ, []),
    "mdno_nnconv_bwd_we_colsum": (_I, [_P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _SZ, _P]),
    "mdno_nnconv_bwd_we_bf16_colsum": (_I, [_P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _SZ, _P]),
    "mdno_relu_bwd_bf16": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "mdno_colsum_bf16_workspace_bytes": (_SZ, [_I]),
    "mdno_colsum_bf16": (_I, [_P, _L, _I, _P, _P, _SZ, _P]),
    "mdno_nnconv_chain_fwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _P]),
    "mdno_nnconv_chain_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mdno_nnconv_chain_bf16w_fwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _P]),
    "mdno_nnconv_chain_bf16w_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mdno_colsum_atb_bf16_workspace_bytes": (_SZ, [_I, _I]),
    "mdno_colsum_atb_bf16": (_I, [_P, _P, _L, _I, _I, _P, _P, _P, _SZ, _P]),
    "mdno_node_prologue_bwd_workspace_bytes": (_SZ, [C.POINTER(KernelNNParams), _I]),
    "mdno_node_prologue_bwd": (_I, [C.POINTER(KernelNNParams), _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _SZ,
                                    _P]),
    "mdno_fc_out_bwd_workspace_bytes": (_SZ, [_I, _I, _I]),
    "mdno_fc_out_bwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "mdno_collate_samples": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "mdno_lploss_rel_fwd": (_I, [_P, _P, _L, _I, _I, _P, _P, _P]),
    "mdno_lploss_rel_bwd": (_I, [_P, _P, _P, _P, _L, _I, _I, _P, _P]),
    "mdno_nnconv_msg_grad": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P]),
    "mdno_nnconv_bwd_x_edges": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _P]),
    "mdno_nnconv_bwd_we_edges": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "mdno_scale_rows": (_I, [_P, _P, _L, _I, _P, _P]),
    "mdno_relu_mask_bwd": (_I, [_P, _P, _L, _P, _P]),
    "mdno_scatter_rows": (_I, [_P, _P, _L, _I, _P, _P]),
    "mdno_forecast_score_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "mdno_forecast_score": (_I, [_P, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P, _I, _P, _SZ, _P]),
    "mdno_contact_maps": (_I, [_P, _L, _I, _D, _P, _P]),
}

# include/mdno_train.h: training on dense graphs, with a version number of its own
TRAIN_ABI_VERSION = 1
TRAIN_SIGNATURES = {
    "mdno_train_abi_version": (_I, []),
    "mdno_train_moment_h_floats": (_SZ, [_L, _I]),
    "mdno_train_moment_fwd_workspace_bytes": (_SZ, [_I, _I, _L, _I]),
    "mdno_train_moment_fwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I,
                                   _P, _P, _P, _SZ, _P]),
    "mdno_train_moment_bwd_workspace_bytes": (_SZ, [_I, _I, _L]),
    "mdno_train_moment_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                   _SZ, _P]),
}

# include/mdno_noise.h: seeded Gaussian noise on the device
_U64 = C.c_uint64
_F = C.c_float
NOISE_PURPOSES = {"rollout": 0, "train_window": 1, "train_motion": 2}
NOISE_SIGNATURES = {
    "mdno_noise_fill": (_I, [_U64, _P, _I, _L, _I, _I, _I, _F, _P, _P, _P]),
    "mdno_noise_add_window": (_I, [_U64, _P, _P, _I, _I, _L, _I, _L, _F, _P, _P, _P]),
    "mdno_rollout_plan_set_noise": (_I, [_P, _F, _U64, _P]),
}

# include/mdno_augment.h: random rigid motions of training samples (the generator's third purpose, "train_motion")
AUGMENT_LAST_ELEMENT = 65
AUGMENT_SIGNATURES = {
    "mdnoaug_motions": (_I, [_U64, _P, _I, _L, _I, _D, _I, _P, _I, _P, _P, _P, _P, _P]),
    "mdnoaug_apply": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "mdnoaug_edge_attr": (_I, [_P, _P, _L, _L, _P, _P]),
}

# include/mdno_unroll.h: gradients w.r.t. the model's inputs, targets of an unrolled step
UNROLL_SIGNATURES = {
    "mdno_edge_mlp_input_bwd": (_I, [_P, _P, _P, _L, _I, _I, _P, _P]),
    "mdno_edge_attr_from_pos": (_I, [_P, _P, _P, _P, _L, _I, _P, _P]),
    "mdno_edge_attr_pos_bwd": (_I, [_P, _P, _P, _P, _I, _P, _P]),
    "mdno_node_prologue_bwd_frames": (_I, [C.POINTER(KernelNNParams), _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P,
                                           _P, _SZ, _P]),
    "mdno_collate_targets": (_I, [_P, _L, _P, _I, _I, _I, _I, _I, _P, _P]),
}

# include/mdno_pbc.h: orthorhombic periodic boundary conditions.  `box` is a HOST pointer to three doubles
# (ops.box_arg).
PBC_SIGNATURES = {
    "mdno_radius_graph_pbc": (_I, [_P, _I, _I, _D, _P, _P, _P, _P, _P, _L, _P, _P, _P]),
    "mdno_rollout_plan_set_box": (_I, [_P, _P, _P]),
    "mdno_forecast_score_pbc": (_I, [_P, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P, _I, _P, _SZ, _P]),
    "mdno_contact_maps_pbc": (_I, [_P, _L, _I, _D, _P, _P, _P]),
}

# include/mdno_observe.h: pair-distance histograms and the radius of gyration of frames on the device.  `box` is a HOST
# pointer to three doubles or NULL.
OBSERVE_SIGNATURES = {
    "mdno_pair_histogram_workspace_bytes": (_SZ, [_L, _I, _I, _I]),
    "mdno_pair_histogram": (_I, [_P, _L, _I, _D, _I, _P, _P, _I, _P, _SZ, _P]),
    "mdno_radius_of_gyration": (_I, [_P, _L, _I, _P, _P]),
}

# include/mdno_dynamics.h: displacement statistics, velocity autocorrelation and unwrapping of a trajectory on the
# device.  `lags` is a HOST pointer to n_lags int32, `box` a HOST pointer to three doubles.
DYNAMICS_SIGNATURES = {
    "mdno_displacement_stats_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "mdno_displacement_stats": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _D, _I, _P, _P, _P, _P, _SZ, _P]),
    "mdno_velocity_autocorrelation_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "mdno_velocity_autocorrelation": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _SZ, _P]),
    "mdno_unwrap_frames": (_I, [_P, _I, _I, _I, _P, _P, _P]),
}

# include/mdno_ensemble.h: ensemble verification (error of the mean, spread, CRPS sums and the rank histogram per step).
# Prefix mdnoens_.
ENSEMBLE_FORMS = {"auto": 0, "registers": 1, "lds": 2}
ENSEMBLE_SIGNATURES = {
    "mdnoens_score_workspace_bytes": (_SZ, [_I, _I, _I]),
    "mdnoens_score": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _SZ, _P]),
}

# include/mdno_conformations.h: structural coverage (the superposed RMSD of every frame against every reference frame, its
# row and per-member column minima).  Prefix mdnoconf_.
CONFORMATIONS_SIGNATURES = {
    "mdnoconf_cross_rmsd_workspace_bytes": (_SZ, [_I, _I, _I, _L, _I]),
    "mdnoconf_cross_rmsd": (_I, [_P, _I, _I, _P, _L, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
}

# include/mdno_essential.h: essential dynamics (superposition onto one reference with the rotated frames handed back,
# column sums, the feature x feature second-moment matrix at a time lag, projection).  Prefix mdnopca_.
ESSENTIAL_SIGNATURES = {
    "mdnopca_superpose": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "mdnopca_feature_sums": (_I, [_P, _L, _I, _P, _P, _P]),
    "mdnopca_covariance_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "mdnopca_covariance": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _SZ, _P]),
    "mdnopca_project": (_I, [_P, _L, _I, _P, _P, _I, _P, _P]),
}

# include/mdno_markov.h: Markov state models (nearest-centre assignment, k-centres seeding, per-state row sums, transition
# counts at a set of lags).  Prefix mdnomsm_.  `lags` is a HOST pointer to n_lags int32.
MARKOV_DTYPES = {"float32": 0, "float64": 1}
MARKOV_SIGNATURES = {
    "mdnomsm_assign_workspace_bytes": (_SZ, [_L, _I, _I]),
    "mdnomsm_assign": (_I, [_P, _L, _I, _I, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    "mdnomsm_kcenters_workspace_bytes": (_SZ, [_L, _I]),
    "mdnomsm_kcenters": (_I, [_P, _L, _I, _I, _I, _L, _P, _P, _P, _SZ, _P]),
    "mdnomsm_centroid_sums": (_I, [_P, _L, _I, _I, _P, _I, _P, _P, _P]),
    "mdnomsm_transition_counts": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P, _P]),
}

# include/mdno_internal.h: internal coordinates (pair distances, angle cosines and dihedral (cos, sin) per frame as a feature
# matrix, and a per-column histogram of one).  Prefix mdnoic_.  `box`, `lo` and `hi` are HOST pointers to doubles.
INTERNAL_DTYPES = {"float32": 0, "float64": 1}
INTERNAL_FORMS = {"auto": 0, "lds": 1, "global": 2}
INTERNAL_RADIANS = 1
INTERNAL_SIGNATURES = {
    "mdnoic_features": (_I, [_P, _L, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _P, _I, _P]),
    "mdnoic_column_histogram": (_I, [_P, _L, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P]),
}

# include/mdno_internal_grad.h: the adjoint of mdnoic_features in its default mode (the gradient with respect to the
# features -> the gradient with respect to the positions).  Prefix mdnoicg_.  `box` is a HOST pointer to doubles; the
# element types and forms are INTERNAL_DTYPES and INTERNAL_FORMS.
INTERNAL_GRAD_MAX_ITEMS = 1 << 29
INTERNAL_GRAD_SIGNATURES = {
    "mdnoicg_features_bwd": (_I, [_P, _L, _I, _P, _I, _P, _I, _P, _I, _P, _P, _L, _P, _I, _P, _I, _P, _I, _I, _P]),
}

# include/mdno_constrain.h: distance-constraint projection of frames, and of the frame a rollout step produces.  Prefix
# mdnocst_, the plan's setter included.  `box` is a HOST pointer to three doubles; the table (pairs, lo, hi, colour_ptr,
# weights) lies on the device.
CONSTRAIN_MAX_ATOMS = 6144          # MDNOCST_MAX_ATOMS: the largest N (the state of a frame lies in LDS as fp64)
CONSTRAIN_MAX_CONSTRAINTS = 1 << 26  # MDNOCST_MAX_CONSTRAINTS
CONSTRAIN_SIGNATURES = {
    "mdnocst_project": (_I, [_P, _P, _L, _I, _P, _P, _P, _L, _P, _I, _P, _P, _I, _D, _P, _P, _P, _P]),
    "mdnocst_rollout_plan_set_constraints": (_I, [_P, _P, _P, _P, _L, _P, _I, _P, _I, _D, _P, _P, _P]),
}

# include/mdno_pbc_train.h: training under a periodic box (edge attributes as a function of positions on the minimum
# image).  Prefix mdnopbt_.  `box` is a HOST pointer to three doubles.
PBC_TRAIN_SIGNATURES = {
    "mdnopbt_edge_attr_from_pos": (_I, [_P, _P, _P, _P, _L, _I, _D, _P, _P, _P]),
}

# include/mdno_contacts.h: contact statistics over time (per-pair counts and distance sums per time block, the contact bits
# of a pair list, their autocorrelation).  Prefix mdnocm_.  `box` is a HOST pointer to three doubles, `lags` a HOST pointer
# to L int32; `pairs` and `cut` lie on the device.
CONTACTS_TILE = 64                  # MDNOCM_TILE
CONTACTS_MAX_LAGS = 1024            # MDNOCM_MAX_LAGS
CONTACTS_SIGNATURES = {
    "mdnocm_pair_statistics": (_I, [_P, _I, _I, _I, _D, _P, _I, _P, _P, _P, _P]),
    "mdnocm_contact_bits": (_I, [_P, _I, _I, _I, _P, _P, _I, _D, _P, _P, _P, _P]),
    "mdnocm_contact_correlation": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _P]),
}

# include/mdno_surface.h: Shrake-Rupley counts of exposed sphere points per atom and frame (the solvent-accessible surface).
# Prefix mdnosa_.  `box` is a HOST pointer to three doubles; `R` and the point table `U` lie on the device.  The forms are
# those of mdno.h (ops.FORECAST_FORMS).
SURFACE_MAX_POINTS = 1024           # MDNOSA_MAX_POINTS
SURFACE_STAGED_ATOMS = 2048         # MDNOSA_STAGED_ATOMS: the largest N whose frame is staged in LDS
SURFACE_TILE = 256                  # MDNOSA_TILE
SURFACE_CHUNK = 64                  # MDNOSA_CHUNK
SURFACE_SIGNATURES = {
    "mdnosa_workspace_bytes": (_SZ, [_L, _I, _I, _I]),
    "mdnosa_exposed_points": (_I, [_P, _L, _I, _P, _P, _I, _P, _D, _P, _I, _P, _SZ, _P]),
}

# THE REGISTRY of the C ABI: every header under include/ with its table.  The contract, for all of them alike:
#   * a header's declarations are its table's names, with the table's arities, and every one is exported by libmdno.so;
#     the library exports no other name that starts with mdno;
#   * a name stands in ONE table (the merge below raises otherwise), so a new header may use any free name: mdno_ is
#     fine.  The prefixes mdnoens_ ... mdnopbt_ of the later tables are kept because they are ABI, not because
#     anything still asks for them;
#   * mdno.h and mdno_train.h carry a version number each (ABI_VERSION, TRAIN_ABI_VERSION); the others are additive
#     and carry none;
#   * every header here is part of the library's build id (source_build_id), and include/ holds no other header.
# tests/test_cabi_tables.py checks all of it, per header and once over the whole.  A new header is: the header, its table,
# one line here.
TABLES = (
    ("mdno.h", SIGNATURES),
    ("mdno_train.h", TRAIN_SIGNATURES),
    ("mdno_noise.h", NOISE_SIGNATURES),
    ("mdno_unroll.h", UNROLL_SIGNATURES),
    ("mdno_pbc.h", PBC_SIGNATURES),
    ("mdno_observe.h", OBSERVE_SIGNATURES),
    ("mdno_dynamics.h", DYNAMICS_SIGNATURES),
    ("mdno_ensemble.h", ENSEMBLE_SIGNATURES),
    ("mdno_conformations.h", CONFORMATIONS_SIGNATURES),
    ("mdno_essential.h", ESSENTIAL_SIGNATURES),
    ("mdno_markov.h", MARKOV_SIGNATURES),
    ("mdno_internal.h", INTERNAL_SIGNATURES),
    ("mdno_internal_grad.h", INTERNAL_GRAD_SIGNATURES),
    ("mdno_constrain.h", CONSTRAIN_SIGNATURES),
    ("mdno_pbc_train.h", PBC_TRAIN_SIGNATURES),
    ("mdno_contacts.h", CONTACTS_SIGNATURES),
    ("mdno_augment.h", AUGMENT_SIGNATURES),
    ("mdno_surface.h", SURFACE_SIGNATURES),
)


def merge_tables(tables=TABLES) -> dict:
    """name -> (header, restype, argtypes) over all tables; a name in two of them is an error."""
    merged = {}
    for header, table in tables:
        for name, (res, args) in table.items():
            if name in merged:
                raise MdnoError(f"{name} stands in the tables of {merged[name][0]} and of {header}")
            merged[name] = (header, res, args)
    return merged


BINDINGS = merge_tables()

_lib = None


def source_build_id(root: Path | None = None) -> str | None:
    """The id csrc/build.sh compiles into the library, recomputed from the tree (or from a copy of it at `root`): sha256
    over csrc/*.{hip,h,sh}, then over every header of TABLES under include/ (bytes, C-locale name order each), first 16
    hex digits.  None where any of them is not beside the package (a binary-only install)."""
    import hashlib
    root = _HERE.parent if root is None else Path(root)
    csrc = root / _HERE.name / "csrc"
    headers = [root / "include" / name for name in sorted((h for h, _ in TABLES), key=str.encode)]
    if not csrc.is_dir() or not all(f.exists() for f in headers):
        return None
    files = sorted([f for f in csrc.iterdir() if f.suffix in (".hip", ".h", ".sh")], key=lambda f: str(f).encode())
    h = hashlib.sha256()
    for f in files + headers:
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def load() -> C.CDLL:
    """Load libmdno.so once; raise (never fall back) if it is absent or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise MdnoError(
            f"{LIB_PATH} not found: the HIP library is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or molecular_dynamics_neural_operator_amd/csrc/build.sh). There is no CPU fallback.")
    lib = C.CDLL(str(LIB_PATH))
    for name, (_, res, args) in BINDINGS.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    ver = lib.mdno_abi_version()
    if ver != ABI_VERSION:
        raise MdnoError(f"libmdno ABI {ver} != binding {ABI_VERSION}; rebuild the library")
    if lib.mdno_train_abi_version() != TRAIN_ABI_VERSION:
        raise MdnoError(f"libmdno training ABI {lib.mdno_train_abi_version()} != binding {TRAIN_ABI_VERSION}; rebuild the library")
    want, have = source_build_id(), lib.mdno_build_id().decode()
    # (an experimental build — scripts/micro/build_exp.sh, loaded through MDNO_LIB — says so in its build id; MDNO_LIB
    # pointing at any other library, the in-tree one included, does not switch the check off)
    if want is not None and have != want and have != "experimental":
        raise MdnoError(f"{LIB_PATH} was built from other sources (build id {have}; csrc/ and include/ of the tree give {want}): run "
                        f"molecular_dynamics_neural_operator_amd/csrc/build.sh — a stale library is never used")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        msg = load().mdno_last_error().decode(errors="replace")
        raise MdnoError(f"{what or 'libmdno'} failed (code {rc}): {msg}")


def ptr(t) -> int | None:
    """Device pointer of a CUDA(HIP) tensor, None for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MdnoError("libmdno kernels run on the GPU only: got a CPU tensor (no CPU fallback exists)")
    if not t.is_contiguous():
        raise MdnoError("libmdno needs contiguous tensors")
    return t.data_ptr()


def f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t.contiguous()


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise MdnoError("no HIP device visible: this package only runs on an MI355X-class GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def raise_on_status(status_word: int, what: str = "") -> None:
    """Turn the device status bits (include/mdno.h MDNO_STATUS_*) into the exception the reference
    would have raised at that point (IndexError from nn.Embedding / index_select) or an MdnoError."""
    st = int(status_word)
    if not st:
        return
    pre = (what + ": ") if what else ""
    if st & STATUS_BAD_AMINOACID:
        raise MdnoIndexError(pre + "x_aminoacid outside [0, num_embeddings) (index out of range in self)")
    if st & STATUS_BAD_EDGE_INDEX:
        raise MdnoIndexError(pre + "edge_index holds a node id outside [0, num_nodes)")
    if st & STATUS_EDGE_OVERFLOW:
        raise MdnoError(pre + "radius graph exceeded edge_cap; use a larger capacity")
    raise MdnoError(pre + f"device status {st:#x}")
