"""ctypes binding of librangeldm_hip.so (include/rangeldm_hip.h).  The product path has NO fallback: if the HIP
library is missing or a call fails, a RuntimeError carrying rldm_last_error() is raised."""
import ctypes as C
import enum
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RLDM_LIB selects another build of the same library (tools/: the -DRLDM_ABLATE timeline build); never a fallback
LIB_PATH = os.environ.get("RLDM_LIB") or os.path.join(_HERE, "librangeldm_hip.so")
RLDM_MAX_LEVELS = 8
# rldm_sampler_config::mode (RLDM_SAMPLER_*)
RLDM_SAMPLER_DDIM, RLDM_SAMPLER_DDPM, RLDM_SAMPLER_DPMSOLVER, RLDM_SAMPLER_UNIPC = 0, 1, 2, 3
# rldm_emd_matrix: the `symmetric` argument, and the return value that reports a pair at the bid cap
RLDM_EMD_RECT, RLDM_EMD_SYMMETRIC, RLDM_EMD_DIAGONAL = 0, 1, 2
RLDM_EMD_BID_CAP = 2
# rldm_voxel_counts: the return value that reports a point out of range, and the workspace bound in hash slots
RLDM_VOXEL_RANGE, RLDM_VOXEL_MAX_SLOTS = 4, 1 << 25
# rldm_hough_*: the largest accumulator (rows, bins per row) and the most candidate beams
RLDM_HOUGH_MAX_THETA, RLDM_HOUGH_MAX_H, RLDM_HOUGH_MAX_BEAMS = 65536, 4096, 256
# rldm_singular_values_f64 / rldm_frechet_distance: the return values that are not the ordinary error
RLDM_FRECHET_SWEEP_CAP, RLDM_FRECHET_NONFINITE, RLDM_FRECHET_MAX_SWEEPS = 2, 3, 60
# rldm_feature_scan_f64: the largest k (a row keeps k + 1 squared distances); non-finite input returns RLDM_FRECHET_NONFINITE
RLDM_FEATURE_MAX_K = 16
RLDM_TRAIN_PAD_END = 4  # rldm_train_conv_desc.mode flag: end-only padding
# rldm_rangenet_layer_desc::kind (enum rldm_rangenet_kind)
RLDM_RN_CONV1X1, RLDM_RN_CONV3X3, RLDM_RN_CONV3X3_S2, RLDM_RN_UPCONV = 0, 1, 2, 3


class Flag(enum.IntFlag):
    """Routing switches of rldm_debug_set_flags / plan_flags (enum rldm_flag: Flag.X is RLDM_FLAG_X)."""
    ATTN_PROJ_LAUNCH = 1 << 7
    NO_CONV_SMALL = 1 << 8
    SMALL_128PX = 1 << 10
    NO_STREAM_REGW = 1 << 11
    STREAM_ANY_GRID = 1 << 12
    GRAPH_TRACE = 1 << 13
    SMALL_64PX_32X2 = 1 << 19
    CONSUMER_GN = 1 << 20
    NO_WIDE_SPLIT = 1 << 21
    OWN_IMAGE_COPIES = 1 << 22
    SCHED_LAUNCH = 1 << 23
    NO_PERSISTENT = 1 << 24
    NO_CLUSTERS = 1 << 26


class Flag2(enum.IntFlag):
    """Routing switches of rldm_debug_set_flags2 (enum rldm_flag2: Flag2.X is RLDM_FLAG2_X)."""
    STREAM_8WAVE_FULL = 1
    STREAM_8WAVE_128X8 = 2
    STREAM_8WAVE_C64 = 4
    STREAM_SPEC_WAVES = 32
    STREAM_64PX = 64
    NO_REGW = 1 << 24
    REGW_CAP8 = 1 << 25
    FP32_OUT = 1 << 26
    HALO_RING = 1 << 29


class UNetConfigC(C.Structure):
    _fields_ = [("sample_w", C.c_int32), ("sample_h", C.c_int32), ("in_channels", C.c_int32),
                ("out_channels", C.c_int32), ("layers_per_block", C.c_int32), ("num_levels", C.c_int32),
                ("block_out_channels", C.c_int32 * RLDM_MAX_LEVELS), ("down_attn", C.c_int32 * RLDM_MAX_LEVELS),
                ("up_attn", C.c_int32 * RLDM_MAX_LEVELS), ("attention_head_dim", C.c_int32),
                ("norm_num_groups", C.c_int32), ("norm_eps", C.c_float), ("mid_attention", C.c_int32),
                ("flip_sin_to_cos", C.c_int32), ("freq_shift", C.c_int32)]


class VAEConfigC(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("ch", C.c_int32), ("num_levels", C.c_int32),
                ("ch_mult", C.c_int32 * RLDM_MAX_LEVELS), ("num_res_blocks", C.c_int32), ("z_channels", C.c_int32),
                ("double_z", C.c_int32), ("norm_num_groups", C.c_int32), ("norm_eps", C.c_float),
                ("scaling_factor", C.c_float)]


class SamplerConfigC(C.Structure):
    _fields_ = [("batch", C.c_int32), ("num_steps", C.c_int32), ("mode", C.c_int32), ("pos_encoding", C.c_int32),
                ("cond_channels", C.c_int32), ("guided", C.c_int32), ("coef", C.POINTER(C.c_float)),
                ("timesteps", C.POINTER(C.c_int64)),
                ("plan_flags", C.c_int32), ("prediction_type", C.c_int32)]


class ConvDescC(C.Structure):
    _fields_ = [("B", C.c_int32), ("Cin0", C.c_int32), ("Cin1", C.c_int32), ("Win", C.c_int32), ("Hin", C.c_int32),
                ("Cout", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("pad_mode", C.c_int32),
                ("upsample", C.c_int32), ("gn", C.c_int32), ("silu", C.c_int32), ("eps", C.c_float)]


class ConvSchedDescC(C.Structure):
    """rldm_conv_sched_desc: the scheduler block of rldm_test_conv_sched (device pointers)."""
    _fields_ = [("sampler_mode", C.c_int32), ("prediction_type", C.c_int32), ("coef_table", C.c_void_p), ("step", C.c_void_p),
                ("x", C.c_void_p), ("noise", C.c_void_p), ("noise_step_stride", C.c_int64), ("x_prev", C.c_void_p),
                ("pack", C.c_void_p), ("pack_ld", C.c_int32)]


class LidarConfigC(C.Structure):
    _fields_ = [("beams", C.c_int32), ("width", C.c_int32), ("mode", C.c_int32), ("mean", C.c_float), ("std", C.c_float),
                ("range_fill", C.c_float), ("intensity_fill", C.c_float), ("grid", C.c_int32 * 3),
                ("pc_range", C.c_float * 6), ("normalize_volume_densities", C.c_int32)]


class RangeNetLayerDescC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
                ("Cout", C.c_int32), ("leaky", C.c_int32)]


class RangeNetConfigC(C.Structure):
    _fields_ = [("layers", C.c_int32), ("in_channels", C.c_int32), ("num_classes", C.c_int32)]


class TrainConvDescC(C.Structure):
    _fields_ = [("B", C.c_int32), ("Win", C.c_int32), ("Hin", C.c_int32), ("Cin", C.c_int32), ("N", C.c_int32),
                ("taps", C.c_int32), ("stride", C.c_int32), ("mode", C.c_int32)]


class TrainMetaDescC(C.Structure):
    """rldm_train_meta_desc: one Meta-Kernel layer (4x4 window, padding 1, W wraps) over an input (B, Win, Hin, C)."""
    _fields_ = [("B", C.c_int32), ("Win", C.c_int32), ("Hin", C.c_int32), ("C", C.c_int32), ("N", C.c_int32), ("stride", C.c_int32)]


class TrainDiscConvDescC(C.Structure):
    """rldm_train_disc_conv_desc: the discriminator's 4x4 conv, zero-padded 1 on both axes (W does not wrap)."""
    _fields_ = [("B", C.c_int32), ("Win", C.c_int32), ("Hin", C.c_int32), ("Cin", C.c_int32), ("N", C.c_int32), ("stride", C.c_int32)]


class TrainFuseC(C.Structure):
    """rldm_train_fuse (include/rangeldm_hip.h): what a fused conv / weight-gradient launch folds in."""
    _fields_ = [("x1", C.c_void_p), ("C0", C.c_int32), ("cs0", C.c_void_p), ("cs1", C.c_void_p), ("gamma", C.c_void_p),
                ("beta", C.c_void_p), ("silu", C.c_int32), ("groups", C.c_int32), ("eps", C.c_float), ("cs_out", C.c_void_p),
                ("g0", C.c_void_p), ("g1", C.c_void_p), ("G0", C.c_int32), ("gcs0", C.c_void_p), ("gcs1", C.c_void_p),
                ("ggamma", C.c_void_p), ("gbeta", C.c_void_p), ("gsilu", C.c_int32), ("ggroups", C.c_int32), ("geps", C.c_float),
                ("gs_out", C.c_void_p)]


class PackDescC(C.Structure):
    _fields_ = [("first", C.c_int64), ("param_offset", C.c_int64), ("w_forward", C.c_void_p), ("w_transposed", C.c_void_p),
                ("N", C.c_int32), ("Cin", C.c_int32), ("taps", C.c_int32), ("pad_", C.c_int32)]


class HyperConfigC(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("ema_max_decay", C.c_float),
                ("ema_inv_gamma", C.c_float), ("ema_power", C.c_float), ("lr_warmup_steps", C.c_int64), ("total_steps", C.c_int64)]


class AdamWConfigC(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("max_grad_norm", C.c_float), ("ema_decay", C.c_float), ("step", C.c_int32)]


_P = C.c_void_p
# every symbol declared in include/rangeldm_hip.h: name -> (restype, argtypes)
PROTOTYPES = {
    "rldm_last_error": (C.c_char_p, []),
    "rldm_device_info": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    "rldm_unet_create": (C.c_int, [C.POINTER(UNetConfigC), C.POINTER(_P)]),
    "rldm_unet_destroy": (None, [_P]),
    "rldm_unet_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "rldm_unet_finalize": (C.c_int, [_P]),
    "rldm_unet_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "rldm_vae_create": (C.c_int, [C.POINTER(VAEConfigC), C.POINTER(_P)]),
    "rldm_vae_destroy": (None, [_P]),
    "rldm_vae_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "rldm_vae_finalize": (C.c_int, [_P]),
    "rldm_vae_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_vae_encode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_diag_gaussian_sample": (C.c_int, [_P, _P, C.c_float, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_sched_ddim_step": (C.c_int, [C.POINTER(C.c_float), _P, _P, _P, _P, C.c_int64, _P]),
    "rldm_sched_ddpm_step": (C.c_int, [C.POINTER(C.c_float), _P, _P, _P, _P, C.c_int64, _P]),
    "rldm_sched_step": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float), _P, _P, _P, _P, C.c_int64, _P]),
    "rldm_sched_dpmsolver_step": (C.c_int, [C.c_int, C.POINTER(C.c_float), _P, _P, _P, _P, C.c_int64, _P]),
    "rldm_sched_unipc_step": (C.c_int, [C.c_int, C.POINTER(C.c_float), _P, _P, _P, _P, _P, C.c_int64, _P]),
    # rldm_sched_step + known-region blend + re-noise (the row of a guided sampler)
    "rldm_sched_guided_step": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int,
                                         C.c_int64, _P]),
    "rldm_sched_add_noise": (C.c_int, [_P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int64, _P, _P]),
    "rldm_sampler_create": (C.c_int, [_P, _P, C.POINTER(SamplerConfigC), C.POINTER(_P)]),
    "rldm_sampler_destroy": (None, [_P]),
    "rldm_sample": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "rldm_sample_guided": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rldm_sampler_status": (C.c_int, [_P]),
    # counter-based normals (csrc/rng.hip; rng.py): the fill, its two test entry points, the samplers that draw inside their graphs
    "rldm_randn": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, _P]),
    "rldm_rng_philox": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_int64, _P, _P]),
    "rldm_rng_normals_from_bits": (C.c_int, [_P, C.c_int64, _P, _P]),
    "rldm_sample_rng": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint64, _P, _P, _P, _P]),
    "rldm_sample_guided_rng": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint64, _P, _P, _P, _P, _P]),
    "rldm_debug_sampler_captures": (C.c_int, [_P]),
    "rldm_unet_set_plan_flags": (C.c_int, [_P, C.c_int]),
    "rldm_debug_inject_trunk_error": (C.c_int, [_P, C.c_int]),
    "rldm_comm_bind": (C.c_int, []),
    "rldm_comm_unique_id": (C.c_int, [_P, C.c_size_t]),
    "rldm_comm_create": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "rldm_comm_destroy": (None, [_P]),
    "rldm_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "rldm_allgather_images": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "rldm_allreduce_grads": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "rldm_lidar_create": (C.c_int, [C.POINTER(LidarConfigC), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(_P)]),
    "rldm_lidar_destroy": (None, [_P]),
    "rldm_lidar_to_points": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_lidar_to_voxel": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_lidar_to_voxel_train": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_lidar_to_voxel_ordered": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_lidar_to_voxel_backward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "rldm_lidar_filter_points": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P]),
    "rldm_render_u8": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_lidar_project": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_float, _P, _P, _P, _P]),
    "rldm_bev_histogram": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, _P, _P]),
    "rldm_hist_jsd": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_double), _P]),
    "rldm_hist_spectral_sq": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_hist_mmd": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_double), _P]),
    # pytorch3d.loss.chamfer_distance as ldm/convert_vae.py:262-271 calls it (nearest squared distances, then per-pair means)
    "rldm_chamfer_nn": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_chamfer_mean": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P]),
    # nearest neighbour with its index and the hit counts (csrc/nn_index.hip): packed as rldm_chamfer_nn; d2, idx per side, hits
    "rldm_nn_index": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    # K nearest neighbours, one direction (csrc/knn.hip): d2 and idx [queries][K]; PCA normals and eigenvalues from such indices
    "rldm_knn": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_knn_normals": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    # all-pairs Chamfer matrix of two sets of clouds, and the lowest-index row argmin the set metrics count with
    "rldm_chamfer_matrix": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_matrix_row_argmin": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    # voxel-occupancy counts {a, b, c} per pair (csrc/voxel.hip): packed as rldm_chamfer_nn, voxel size, int32 [pairs][3]
    "rldm_voxel_counts": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_float, _P, _P]),
    # sensor tables by Hough voting (csrc/hough.hip): (d, z) pairs, the vote, row maxima, beam assignment, per-beam moments
    "rldm_hough_pack": (C.c_int, [_P, C.c_int64, C.c_int, C.c_float, C.c_float, _P, _P]),
    "rldm_hough_vote": (C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P]),
    "rldm_hough_vote_shape": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "rldm_hough_row_max": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_hough_assign": (C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_float, _P, _P]),
    "rldm_hough_moments": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    # all-pairs Earth Mover's Distance (epsilon-scaling auction) between equal-size clouds: emd, assignment, prices, bids
    "rldm_emd_matrix": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, _P, _P]),
    # farthest point sampling of a ragged batch of clouds: k local indices per cloud, in selection order
    "rldm_farthest_point_sample": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    # Frechet distance over dumped activations: fp64 Gram product (MFMA), one-sided Jacobi singular values, the distance
    "rldm_gram_f64": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "rldm_singular_values_f64": (C.c_int, [_P, C.c_int, C.c_int, C.c_double, C.c_int, _P, C.POINTER(C.c_int), _P]),
    "rldm_frechet_distance": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_double), _P]),
    "rldm_frechet_last_sweeps": (C.c_int, []),
    # kernel distance and precision / recall / density / coverage: one row scan of a against b, per-row outputs only
    "rldm_feature_scan_f64": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_longlong,
                                        _P, _P, _P, _P, _P, _P]),
    "rldm_feature_scan_column_chunk": (C.c_int, [C.c_int]),
    # RangeNet++ inference (csrc/rangenet.hip): weight packing, one layer, the architecture's layer list, the network
    "rldm_rangenet_packed_elems": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "rldm_rangenet_pack_weights": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_rangenet_layer": (C.c_int, [C.POINTER(RangeNetLayerDescC), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P]),
    "rldm_rangenet_num_layers": (C.c_int, [C.POINTER(RangeNetConfigC)]),
    "rldm_rangenet_layer_info": (C.c_int, [C.POINTER(RangeNetConfigC), C.c_int, C.POINTER(RangeNetLayerDescC)]),
    "rldm_rangenet_create": (C.c_int, [C.POINTER(RangeNetConfigC), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    "rldm_rangenet_destroy": (None, [_P]),
    "rldm_rangenet_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P]),
    # around the forward (csrc/rangenet_post.hip): a ragged batch of scans -> the network's input; argmax -> per-point labels
    "rldm_rangenet_project": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_float),
                                        C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rldm_rangenet_unproject": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_float,
                                          C.c_int, _P, _P]),
    # MAE / PSNR of ldm/convert_vae.py:236-247 and the range MAE of metrics/metrics/mae.py:45-117
    "rldm_range_errors": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.c_int, C.c_int, _P, _P, _P]),
    # cv2.resize(target[::rate], fx=1, fy=rate, INTER_NEAREST / INTER_CUBIC) baselines, metrics/metrics/mae.py:61-81
    "rldm_beam_upsample": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_train_conv": (C.c_int, [C.POINTER(TrainConvDescC), _P, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "rldm_train_conv_splits": (C.c_int, [C.POINTER(TrainConvDescC), C.c_int]),
    "rldm_train_wgrad": (C.c_int, [C.POINTER(TrainConvDescC), _P, _P, _P, _P]),
    "rldm_train_wgrad_bias": (C.c_int, [C.POINTER(TrainConvDescC), _P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "rldm_train_colsum": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "rldm_train_gn_forward": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, C.c_int, _P, _P, _P]),
    "rldm_train_gn_backward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, C.c_int,
                                         _P, _P, _P]),
    "rldm_train_conv_fused_ok": (C.c_int, [C.POINTER(TrainConvDescC), C.POINTER(TrainFuseC), C.c_int]),
    "rldm_train_conv_fused": (C.c_int, [C.POINTER(TrainConvDescC), C.POINTER(TrainFuseC), _P, _P, _P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "rldm_train_wgrad_fused_ok": (C.c_int, [C.POINTER(TrainConvDescC), C.POINTER(TrainFuseC)]),
    "rldm_train_wgrad_fused": (C.c_int, [C.POINTER(TrainConvDescC), C.POINTER(TrainFuseC), _P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "rldm_train_defer_reduce": (C.c_int, [C.c_int]),
    "rldm_train_flush_reduce": (C.c_int, []),
    "rldm_calibrate": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "rldm_calib_clock_stamp": (C.c_int, [_P, _P]),
    "rldm_train_wgrad_group": (C.c_int, [C.c_int]),
    "rldm_train_wgrad_group_flush": (C.c_int, []),
    "rldm_train_wgrad_group_pending": (C.c_int, []),
    "rldm_train_deterministic": (C.c_int, [C.c_int]),
    "rldm_train_deterministic_enabled": (C.c_int, []),
    "rldm_train_reduce_pending": (C.c_int, []),
    "rldm_train_chan_stats": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_train_gn_backward_apply": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P,
                                               _P, C.c_int, _P, C.c_int, _P, _P, _P]),
    "rldm_train_linear_rows": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rldm_train_linear_rows_wgrad": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_attention_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_attention_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "rldm_train_attention_qkv_forward": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_attention_qkv_backward": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_add": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "rldm_train_copy_channels": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, _P]),
    "rldm_train_sum2x2": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_train_silu": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "rldm_train_timestep_embedding": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "rldm_train_pack_input": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_train_unpack_output": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_train_mse": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_l1": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_gaussian": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_gaussian_backward": (C.c_int, [_P, _P, _P, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_train_sqnorm": (C.c_int, [_P, C.c_int64, _P, _P]),
    # decoder-guided sampling (csrc/guide.hip): masked residual + its fixed-order fp64 sum, the decoder's input, the update of the
    # clean-latent estimate, the correction of the plain DDIM step
    "rldm_guide_residual": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_guide_latent": (C.c_int, [_P, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_guide_update": (C.c_int, [_P, _P, C.c_double, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_guide_correct": (C.c_int, [_P, _P, C.c_float, C.c_int64, _P, _P]),
    "rldm_train_adamw": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(AdamWConfigC), _P]),
    "rldm_train_adamw_dyn": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(AdamWConfigC), _P, C.c_int, _P]),
    "rldm_train_hyper_step": (C.c_int, [_P, C.POINTER(HyperConfigC), _P, _P]),
    "rldm_train_pack_weights": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rldm_train_pack_weights_all": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P]),
    "rldm_train_pack_weights_tiled": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P]),
    # the PatchGAN discriminator (csrc/train_disc.hip): 4x4 zero-padded convs, BatchNorm + LeakyReLU, the adversarial losses
    "rldm_train_disc_conv_ok": (C.c_int, [C.POINTER(TrainDiscConvDescC)]),
    "rldm_train_disc_conv": (C.c_int, [C.POINTER(TrainDiscConvDescC), _P, _P, _P, _P, _P]),
    "rldm_train_disc_conv_dgrad": (C.c_int, [C.POINTER(TrainDiscConvDescC), _P, _P, _P, _P]),
    "rldm_train_disc_wgrad_workspace": (C.c_int64, [C.POINTER(TrainDiscConvDescC)]),
    "rldm_train_disc_wgrad": (C.c_int, [C.POINTER(TrainDiscConvDescC), _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rldm_train_disc_bn_workspace": (C.c_int64, [C.c_int64, C.c_int]),
    "rldm_train_disc_bn_forward": (C.c_int, [_P, C.c_int64, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int64, _P]),
    "rldm_train_disc_bn_backward": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "rldm_train_disc_lrelu": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P]),
    "rldm_train_disc_hinge": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P, _P, _P, _P, _P]),
    "rldm_train_disc_generator": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P]),
    "rldm_train_disc_adaptive_mix": (C.c_int, [_P, _P, _P, _P, C.c_float, C.c_float, _P, _P, C.c_int64, _P]),
    # the Meta-Kernel discriminator layer (csrc/train_meta.hip)
    "rldm_train_meta_ok": (C.c_int, [C.POINTER(TrainMetaDescC)]),
    "rldm_train_meta_workspace": (C.c_int64, [C.POINTER(TrainMetaDescC)]),
    "rldm_train_meta_range": (C.c_int, [_P, C.c_int64, C.c_int, C.c_float, C.c_float, _P, _P]),
    "rldm_train_meta_range_grad": (C.c_int, [_P, C.c_int64, C.c_int, C.c_float, _P, _P]),
    "rldm_train_meta_forward": (C.c_int, [C.POINTER(TrainMetaDescC)] + [_P] * 15 + [C.c_int64, _P]),
    "rldm_train_meta_backward": (C.c_int, [C.POINTER(TrainMetaDescC)] + [_P] * 20 + [C.c_int64, _P]),
    "rldm_unet_flops": (C.c_double, [_P, C.c_int]),
    "rldm_vae_decode_flops": (C.c_double, [_P, C.c_int, C.c_int, C.c_int]),
    "rldm_unet_num_launches": (C.c_int, [_P, C.c_int]),
    "rldm_unet_trunk_status": (C.c_int, [_P, C.c_int]),
    "rldm_sampler_profile": (C.c_int, [_P, _P, C.c_char_p, C.c_size_t]),
    "rldm_test_conv": (C.c_int, [C.POINTER(ConvDescC), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rldm_bench_conv": (C.c_int, [C.POINTER(ConvDescC), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                  C.c_char_p, C.c_size_t, _P]),
    "rldm_debug_force_tile": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "rldm_test_conv_stats": (C.c_int, [C.POINTER(ConvDescC), _P, _P, _P, _P, _P]),
    "rldm_test_conv_sched": (C.c_int, [C.POINTER(ConvDescC), _P, _P, _P, _P, _P, C.POINTER(ConvSchedDescC), _P, C.c_char_p, C.c_size_t,
                                       _P]),
    # the time-embedding table of n timesteps on its own, and its layout (row length; a resnet's first column)
    "rldm_test_temb": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "rldm_test_temb_layout": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int)]),
    "rldm_debug_set_flags": (C.c_int, [C.c_int]),
    "rldm_debug_set_flags2": (C.c_int, [C.c_int]),
    "rldm_debug_graph_trace": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_size_t]),
    "rldm_debug_timestamps": (C.c_int, [_P]),
    "rldm_debug_block_times": (C.c_int, [_P, C.c_int]),
    "rldm_test_attention": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rldm_test_attention_qkv": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P]),
    "rldm_test_attention_route": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "rldm_test_attention_block": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P,
                                            _P]),
    "rldm_bench_attention_qkv": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _P]),
}

_lib = None


def lib():
    """Load (once) and return the bound library; raises if it has not been built (`__graft_entry__.build()`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               f"(hipcc --offload-arch=gfx950).  rangeldm_amd has no CPU fallback.")
        # PyTorch first: its wheel carries its own libamdhip64, and the library's dependency on that soname must resolve to the copy
        # torch loads -- loaded the other way round the process holds two HIP runtimes, and this one then finds "no ROCm-capable
        # device" (seen with build() and smoke() in one process on a GPU box)
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)           # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().rldm_last_error()
        raise RuntimeError(f"librangeldm_hip: {what} failed: {msg.decode() if msg else 'unknown error'}")


def ptr(t):
    """The device pointer of a tensor as the C ABI takes it; None stays None (a null argument)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr(device=None):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("rangeldm_amd needs an MI355X (gfx950) visible to PyTorch-ROCm; there is no CPU fallback")
    name = C.create_string_buffer(64)
    cus = C.c_int(0)
    check(lib().rldm_device_info(name, 64, C.byref(cus)), "rldm_device_info")
    return name.value.decode(), cus.value
