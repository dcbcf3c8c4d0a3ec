"""ctypes binding of libbyzagg.so (include/byzagg.h).  No fallback: a missing library is an error."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BYZ_LIBRARY: another build of the same ABI (the sanitized one, build_native.py --sanitize)
LIB_PATH = os.environ.get('BYZ_LIBRARY') or os.path.join(_HERE, 'libbyzagg.so')

OK, E_INVALID, E_PRECONDITION, E_HIP, E_UNSUPPORTED, E_NO_WINNER, E_COLLECTIVE = 0, -1, -2, -3, -4, -5, -6

KERNELS = ('column_stats', 'gram_tile', 'gram_reduce', 'distances', 'row_sort', 'krum_argmin',
           'bulyan_loop', 'trimmed_mean', 'misc', 'plane_split')

c_i64, c_i32, c_int, c_f32, c_vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_P = ctypes.POINTER



class GeomedParams(ctypes.Structure):
    """byz_geomed_params: the geometric median's smoothing, update budget and stopping tolerance."""
    _fields_ = [('nu', ctypes.c_double), ('max_iter', c_i64), ('ftol', ctypes.c_double)]


class CclipParams(ctypes.Structure):
    """byz_cclip_params: centered clipping's radius and iteration count."""
    _fields_ = [('tau', ctypes.c_double), ('iters', c_i64)]


SIGNGUARD_MAX_SAMPLES = 1024      # BYZ_SIGNGUARD_MAX_SAMPLES


class SignGuardParams(ctypes.Structure):
    """byz_signguard_params: SignGuard's census window, norm bounds, bandwidth (0: estimated) and sample size."""
    _fields_ = [('window_start', c_i64), ('window_len', c_i64), ('lower', ctypes.c_double), ('upper', ctypes.c_double),
                ('bandwidth', ctypes.c_double), ('n_sample', c_i64)]


class SparsefedParams(ctypes.Structure):
    """byz_sparsefed_params: SparseFed's clipping norm and the coordinates applied per round."""
    _fields_ = [('clip', ctypes.c_double), ('k', c_i64)]


class NoiseParams(ctypes.Structure):
    """byz_noise_params: the noise's standard deviation and where in the Philox stream the vector lies."""
    _fields_ = [('sigma', ctypes.c_double), ('seed', ctypes.c_uint64), ('round', ctypes.c_uint64), ('column_offset', c_i64)]


class WeakDpParams(ctypes.Structure):
    """byz_weak_dp_params: the norm bound (or adaptive: the median norm), the noise and its place in the stream."""
    _fields_ = [('clip', ctypes.c_double), ('sigma', ctypes.c_double), ('adaptive', c_i64), ('seed', ctypes.c_uint64),
                ('round', ctypes.c_uint64), ('column_offset', c_i64)]


class FlameParams(ctypes.Structure):
    """byz_flame_params: FLAME's noise level, HDBSCAN's two parameters (min_cluster_size 0: n / 2 + 1) and the noise's place."""
    _fields_ = [('lam', ctypes.c_double), ('min_samples', c_i64), ('min_cluster_size', c_i64), ('seed', ctypes.c_uint64),
                ('round', ctypes.c_uint64), ('column_offset', c_i64)]


class FangParams(ctypes.Structure):
    """byz_fang_params: the full-knowledge factor b, the partial-knowledge multiples of sigma, the mode and the draw's place."""
    _fields_ = [('b', ctypes.c_double), ('k_lo', ctypes.c_double), ('k_hi', ctypes.c_double), ('partial', ctypes.c_int),
                ('seed', ctypes.c_uint64), ('round', ctypes.c_uint64), ('column_offset', ctypes.c_uint64)]


MANHATTAN_CHAIN = 128            # BYZ_MANHATTAN_CHAIN: the Manhattan matrix's relative error is at most (this + 2) * 2^-24


class ClippedClusteringParams(ctypes.Structure):
    """byz_clipped_clustering_params: the fixed clip, the adaptive switch (the median norm), the linkage and its fill."""
    _fields_ = [('clip', ctypes.c_double), ('adaptive', ctypes.c_int32), ('method', ctypes.c_int32), ('fill', ctypes.c_double)]


class AfaParams(ctypes.Structure):
    """byz_afa_params: AFA's first xi, its growth per removing round and the cap on the rounds (0: none)."""
    _fields_ = [('xi0', ctypes.c_double), ('delta_xi', ctypes.c_double), ('max_rounds', c_i64)]


class MinmaxParams(ctypes.Structure):
    """byz_minmax_params: the kind (0 Min-Max, 1 Min-Sum), the perturbation (0 unit, 1 std, 2 sign, 3 custom), partial knowledge,
    and whether the caller supplies the distance matrix."""
    _fields_ = [('kind', ctypes.c_int), ('perturbation', ctypes.c_int), ('partial', ctypes.c_int), ('dist_given', ctypes.c_int)]


class FoolsgoldParams(ctypes.Structure):
    """byz_foolsgold_params: FoolsGold's confidence and the divisor of its sum (0: the usable count, 1: the weights' sum)."""
    _fields_ = [('kappa', ctypes.c_double), ('normalise', c_i64)]


class AurorParams(ctypes.Structure):
    """byz_auror_params: the indicative gap, the share of votes that removes a row, the sweeps' cap and the accumulate switch."""
    _fields_ = [('alpha', ctypes.c_double), ('tau', ctypes.c_double), ('max_iter', c_i64), ('accumulate', c_i64)]


class DncParams(ctypes.Structure):
    """byz_dnc_params: DnC's iterations, sampled columns per iteration, power iterations and rows removed per iteration."""
    _fields_ = [('n_iters', c_i64), ('sub_dim', c_i64), ('power_iters', c_i64), ('remove_count', c_i64)]


# name -> argument types (everything returns int unless listed in _RESTYPES)
_PROTOTYPES = {
    'byz_abi_version': [],
    'byz_last_error': [],
    'byz_ctx_create': [c_int, _P(c_vp)],
    'byz_ctx_destroy': [c_vp],
    'byz_ctx_reserve': [c_vp, c_i64, c_i64],
    'byz_ctx_device': [c_vp],
    'byz_limits': [_P(c_i64), _P(c_i64)],
    'byz_malloc': [c_vp, c_i64, _P(c_vp)],
    'byz_free': [c_vp, c_vp],
    'byz_upload': [c_vp, c_vp, c_vp, c_i64, c_vp],
    'byz_download': [c_vp, c_vp, c_vp, c_i64, c_vp],
    'byz_upload_2d': [c_vp, c_vp, c_i64, c_vp, c_i64, c_i64, c_i64, c_vp],
    'byz_stream_sync': [c_vp, c_vp],
    'byz_no_defense_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_pairwise_distances_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_gram_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_gram_share_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_vp, c_vp],
    'byz_gram_share_add_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_int, c_int, c_vp, c_vp],
    'byz_distances_from_gram_dev': [c_vp, c_vp, c_i64, c_vp, c_vp],
    'byz_near_pairs_count': [c_vp, _P(c_i64), c_vp],
    'byz_near_pairs_sqdist_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_near_pairs_apply_dev': [c_vp, c_vp, c_i64, c_vp, c_vp],
    'byz_ctx_check': [c_vp, c_vp],
    'byz_bulyan_rescored': [c_vp, _P(c_i64)],
    'byz_krum_select_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(c_i32), c_vp, c_vp],
    'byz_krum_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_vp, _P(c_i32), c_vp],
    'byz_trimmed_mean_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp],
    'byz_coordinate_median_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_rank_trimmed_mean_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp],
    'byz_window_mean_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp],
    'byz_phocas_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_trimmed_mean_redone': [c_vp, _P(c_i64), c_vp],
    'byz_bulyan_select_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_krum_bulyan_select_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(c_i32), c_vp, c_vp],
    'byz_bulyan_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_mean_rows_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp],
    'byz_multi_krum_select_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_multi_krum_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_vp, c_vp, c_vp],
    # (the byz_allreduce_f64_fn callback and its `user` word are passed as plain pointers: ALLREDUCE_F64_FN builds the callback)
    'byz_pairwise_distances_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_krum_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_vp, c_vp, c_vp, _P(c_i32), c_vp],
    'byz_bulyan_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_multi_krum_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_vp, c_vp, c_vp, c_vp,
                                   c_vp],
    'byz_drift_attack_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_f32, c_vp, c_vp, c_vp, c_int, c_vp],
    'byz_column_chain_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_column_finish_dev': [c_vp, c_vp, c_vp, c_i64, c_f32, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_drift_axpy_dev': [c_vp, c_vp, c_vp, c_i64, c_f32, c_vp],
    'byz_server_update_dev': [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_vp],
    'byz_backdoor_initial_params_dev': [c_vp, c_vp, c_vp, c_i64, c_f32, c_vp, c_vp],
    'byz_backdoor_clip_dev': [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_vp, c_vp],
    'byz_assemble_row_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_assemble_rows_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_assemble_rows_again_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp],
    'byz_assemble_columns_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_assemble_row_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_defend_host': [c_vp, c_int, c_vp, c_i64, c_i64, c_i64, c_i64, c_int, c_vp, c_vp],
    'byz_pairwise_distances_host': [c_vp, c_vp, c_i64, c_i64, c_vp],
    'byz_krum_select_host': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(c_i32)],
    'byz_drift_attack_host': [c_vp, c_vp, c_i64, c_i64, c_f32, c_vp, c_vp, c_vp],
    'byz_multi_krum_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_coordinate_median_host': [c_vp, c_vp, c_i64, c_i64, c_vp],
    'byz_rank_trimmed_mean_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp],
    'byz_window_mean_host': [c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp],
    'byz_phocas_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_row_sqdist_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_weighted_mean_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_geometric_median_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(GeomedParams), c_vp, c_vp, c_vp],
    'byz_geometric_median_info': [c_vp, _P(c_i64), _P(c_i64), _P(ctypes.c_double)],
    'byz_geometric_median_host': [c_vp, c_vp, c_i64, c_i64, _P(GeomedParams), c_vp, c_vp],
    'byz_geometric_median_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(GeomedParams), c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_clip_update_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_centered_clip_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(CclipParams), c_vp, c_vp, c_vp, c_vp],
    'byz_centered_clip_info': [c_vp, _P(c_i64), _P(c_i64)],
    'byz_centered_clip_host': [c_vp, c_vp, c_i64, c_i64, _P(CclipParams), c_vp, c_vp, c_vp],
    'byz_centered_clip_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(CclipParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_row_dots_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_scaled_rows_sum_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_fltrust_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_fltrust_info': [c_vp, _P(c_i64), _P(c_i64), _P(c_i32), _P(ctypes.c_double)],
    'byz_fltrust_host': [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_fltrust_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_row_signs_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_signguard_select_dev': [c_vp, c_vp, c_vp, c_i64, _P(SignGuardParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_signguard_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(SignGuardParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_signguard_info': [c_vp, _P(c_i64), _P(c_i64), _P(c_i64), _P(c_i64), _P(c_i64), _P(ctypes.c_double),
                           _P(ctypes.c_double)],
    'byz_signguard_host': [c_vp, c_vp, c_i64, c_i64, _P(SignGuardParams), c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_signguard_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(SignGuardParams), c_i64, c_i64, c_vp, c_vp, c_vp, c_vp,
                                  c_vp, c_vp, c_vp, c_vp],
    'byz_nnm_neighbours_dev': [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_nnm_mix_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp],
    'byz_nnm_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp],
    'byz_nnm_info': [c_vp, _P(c_i64), _P(c_i64)],
    'byz_nnm_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_nnm_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp],
    'byz_sign_votes_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_sign_flip_dev': [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp],
    'byz_robust_lr_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_robust_lr_info': [c_vp, _P(c_i64)],
    'byz_robust_lr_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_bucket_means_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp],
    'byz_bucket_means_host': [c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp],
    'byz_topk_sparsify_dev': [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_topk_info': [c_vp, _P(c_i64), _P(ctypes.c_uint32), _P(c_i64), _P(c_i64)],
    'byz_topk_sparsify_host': [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp],
    'byz_sparsefed_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(SparsefedParams), c_vp, c_vp, c_vp],
    'byz_sparsefed_host': [c_vp, c_vp, c_i64, c_i64, _P(SparsefedParams), c_vp, c_vp],
    'byz_gaussian_noise_dev': [c_vp, c_vp, c_i64, _P(NoiseParams), c_vp, c_vp, c_vp],
    'byz_noise_words_dev': [c_vp, _P(NoiseParams), c_i64, c_vp, c_vp],
    'byz_gaussian_noise_host': [c_vp, c_vp, c_i64, _P(NoiseParams), c_vp],
    'byz_clip_scales_dev': [c_vp, c_vp, c_i64, _P(WeakDpParams), c_vp, c_vp, c_vp],
    'byz_weak_dp_info': [c_vp, _P(c_i64), _P(c_i64), _P(ctypes.c_double)],
    'byz_weak_dp_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(WeakDpParams), c_vp, c_vp],
    'byz_weak_dp_host': [c_vp, c_vp, c_i64, c_i64, _P(WeakDpParams), c_vp],
    'byz_cosine_distances_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_cosine_from_gram_dev': [c_vp, c_vp, c_i64, c_vp, c_vp],
    'byz_flame_core_distances_dev': [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp],
    'byz_flame_select_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_flame_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(FlameParams), c_vp, c_vp, c_vp, c_vp],
    'byz_flame_info': [c_vp, _P(c_i64), _P(c_i64), _P(ctypes.c_double), _P(ctypes.c_double)],
    'byz_flame_host': [c_vp, c_vp, c_i64, c_i64, _P(FlameParams), c_vp, c_vp, c_vp],
    'byz_flame_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(FlameParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_manhattan_distances_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_manhattan_sums_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_manhattan_from_sums_dev': [c_vp, c_vp, c_i64, c_vp, c_vp],
    'byz_multi_metrics_features_dev': [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp],
    'byz_multi_metrics_select_dev': [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_multi_metrics_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp],
    'byz_multi_metrics_info': [c_vp, _P(c_i64), _P(c_i64), _P(ctypes.c_int32), _P(ctypes.c_double)],
    'byz_multi_metrics_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp],
    'byz_linkage_dev': [c_vp, c_vp, c_i64, c_int, _P(ctypes.c_double), c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_linkage_info': [c_vp, _P(c_i64), _P(c_i64), _P(c_i64)],
    'byz_linkage_cut_dev': [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp],
    'byz_clipped_clustering_select_dev': [c_vp, c_vp, c_i64, c_int, _P(ctypes.c_double), c_vp, c_vp],
    'byz_clipped_clustering_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(ClippedClusteringParams), c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_clipped_clustering_info': [c_vp, _P(c_i64), _P(c_i64), _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double)],
    'byz_clipped_clustering_host': [c_vp, c_vp, c_i64, c_i64, _P(ClippedClusteringParams), c_vp, c_vp, c_vp, c_vp],
    'byz_clipped_clustering_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(ClippedClusteringParams), c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_vp],
    'byz_faba_select_dev': [c_vp, c_vp, c_i64, c_i64, c_int, c_vp, c_vp, c_vp],
    'byz_faba_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_faba_info': [c_vp, _P(c_i64), _P(c_i64), _P(c_i64), _P(ctypes.c_double), _P(ctypes.c_double)],
    'byz_faba_host': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_afa_select_dev': [c_vp, c_vp, c_i64, c_vp, _P(AfaParams), c_vp, c_vp, c_vp, c_vp],
    'byz_afa_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, _P(AfaParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_afa_info': [c_vp, _P(c_i64), _P(ctypes.c_double), _P(ctypes.c_double)],
    'byz_afa_host': [c_vp, c_vp, c_i64, c_i64, c_vp, _P(AfaParams), c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_auror_votes_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(AurorParams), c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_auror_select_dev': [c_vp, c_vp, c_vp, c_vp, c_i64, _P(AurorParams), c_vp, c_vp],
    'byz_auror_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(AurorParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_auror_info': [c_vp, _P(c_i64), _P(c_i64), _P(c_i64), _P(c_i64), _P(c_i64)],
    'byz_auror_host': [c_vp, c_vp, c_i64, c_i64, _P(AurorParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_rows_add_dev': [c_vp, c_vp, c_i64, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp],
    'byz_foolsgold_weights_dev': [c_vp, c_vp, c_i64, _P(FoolsgoldParams), c_vp, c_vp, c_vp, c_vp],
    'byz_foolsgold_trace_dev': [c_vp, c_i64, c_vp, c_vp, c_vp],
    'byz_foolsgold_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, _P(FoolsgoldParams), c_vp, c_vp, c_vp, c_vp],
    'byz_foolsgold_info': [c_vp, _P(c_i64), _P(ctypes.c_double)],
    'byz_foolsgold_host': [c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, _P(FoolsgoldParams), c_vp, c_vp, c_vp],
    'byz_multi_metrics_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_topk_sparsify_sharded_dev': [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_dnc_scores_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp],
    'byz_dnc_select_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(DncParams), c_vp, c_vp, c_vp, c_vp],
    'byz_dnc_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(DncParams), c_vp, c_vp, c_vp, c_vp],
    'byz_dnc_info': [c_vp, _P(c_i64), _P(c_i64)],
    'byz_dnc_host': [c_vp, c_vp, c_i64, c_i64, _P(DncParams), c_vp, c_vp, c_vp, _P(c_i64)],
    'byz_dnc_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(DncParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_column_extremes_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp],
    'byz_fang_fill_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(FangParams), c_vp, c_vp, c_vp, c_vp],
    'byz_fang_trmean_attack_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, _P(FangParams), c_vp],
    'byz_fang_trmean_attack_host': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(FangParams), c_vp],
    'byz_fang_krum_attack_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, _P(ctypes.c_double), c_vp, c_vp, c_vp, c_vp],
    'byz_row_moments_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_minmax_attack_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, _P(MinmaxParams), c_vp, c_vp, c_vp],
    'byz_minmax_attack_sharded_dev': [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, _P(MinmaxParams), c_vp, c_vp, c_vp, c_vp, c_vp],
    'byz_minmax_info': [c_vp, _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double), _P(c_i64), _P(c_i64), _P(c_i32), _P(c_i32)],
    'byz_minmax_attack_host': [c_vp, c_vp, c_i64, c_i64, c_i64, _P(MinmaxParams), c_vp, c_vp],
    'byz_fang_krum_info': [c_vp, _P(ctypes.c_double), _P(ctypes.c_double), _P(c_i64), _P(c_i64), _P(c_i32)],
    'byz_timing_enable': [c_vp, c_int],
    'byz_timing_reset': [c_vp],
    'byz_timing_read': [c_vp, c_int, _P(ctypes.c_double), _P(c_i64)],
    'byz_kernel_name': [c_int],
    'byz_selftest_lane_exchange_dev': [c_vp, c_vp, _P(c_i32), c_vp],
    'byz_selftest_owner_loop_dev': [c_vp, c_vp, _P(c_i32), c_vp],
    'byz_gram_unit_table': [c_i64, _P(c_i32), c_i64, _P(c_i64)],
}
_RESTYPES = {'byz_last_error': ctypes.c_char_p, 'byz_kernel_name': ctypes.c_char_p, 'byz_ctx_destroy': None}

# int (*byz_allreduce_f64_fn)(void* user, double* buf_dev, int64_t count, void* stream)
ALLREDUCE_F64_FN = ctypes.CFUNCTYPE(c_int, c_vp, c_vp, c_i64, c_vp)

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.

    PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 (same SONAMEs as /opt/rocm's).  If
    libbyzagg pulled in /opt/rocm's copies first, a later `import torch` would mix the two sets and find no
    GPU.  So when torch is installed its copies are loaded first (without importing torch), and both torch
    and libbyzagg bind to them; device pointers and streams are then interchangeable.
    """
    if os.environ.get('BYZ_SYSTEM_HIP') == '1':
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], 'lib')
    for name in ('libhsa-runtime64.so', 'libamd_comgr.so', 'libamdhip64.so'):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                pass


def load():
    """Load libbyzagg.so; raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            'libbyzagg.so is not built (%s).  Run `python -m attacking_federate_learning_amd.build_native` '
            '(needs hipcc); this package has no CPU fallback.' % LIB_PATH)
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in _PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here means the library and the header disagree
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)
    if lib.byz_abi_version() != 1:
        raise RuntimeError('libbyzagg ABI version mismatch')
    _lib = lib
    return lib


def last_error():
    msg = load().byz_last_error()
    return msg.decode('utf-8', 'replace') if msg else ''
