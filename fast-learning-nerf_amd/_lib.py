"""ctypes binding of libfastnerf.so (the C ABI declared in include/fastnerf.h).

The product path has NO CPU fallback: if the library is missing or a call
fails, a RuntimeError is raised."""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('FASTNERF_LIB') or os.path.join(HERE, 'libfastnerf.so')   # FASTNERF_LIB: tuning builds

P = C.c_void_p
I = C.c_int
L = C.c_int64
F = C.c_float
D = C.c_double
U64 = C.c_uint64



class StepArgs(C.Structure):
    """fn_step_args of include/fastnerf.h, field for field."""
    _fields_ = (
        [('n', L)] + [(k, P) for k in ('rays_o', 'rays_d', 'target', 't_rand', 'u', 'noise0', 'noise1')]
        + [('seed0', U64), ('seed1', U64), ('leaf_tag', P), ('table', P), ('net_floats', L)]
        + [(k, P) for k in ('params', 'grads', 'adam_m', 'adam_v', 'packed_fwd_c', 'packed_bwd_c', 'packed_fwd_f', 'packed_bwd_f',
                            'rays11', 'z0', 'raw0', 'act0', 'rgb0', 'disp0', 'acc0', 'w0', 'depth0',
                            'z1', 'z_samples', 'z_std', 'raw1', 'act1', 'rgb1', 'disp1', 'acc1', 'w1', 'depth1',
                            'g_rgb', 'g_rgb0', 'loss2', 'draw_ws', 'act_ws', 'dact_ws', 'partial_ws', 'live_ws', 'counts')]
        + [(k, D) for k in ('focal', 'lr', 'beta1', 'beta2', 'eps')]
        + [(k, F) for k in ('near_plane', 'far_plane', 'grad_scale')]
        + [(k, I) for k in ('math_mode', 'N_samples', 'N_importance', 'lindisp', 'perturb', 'white_bkgd', 'ndc', 'H', 'W', 'live',
                            'fwd_flags', 'max_leaves', 'adam_t')]
        + [('occ', P), ('occ_counts', P)])


class MapGrads(C.Structure):
    """fn_map_grads of include/fastnerf.h, field for field."""
    _fields_ = [(k, P) for k in ('g_disp1', 'g_acc1', 'g_depth1', 'g_disp0', 'g_acc0', 'g_depth0')]


class StepAux(C.Structure):
    """fn_step_aux of include/fastnerf.h, field for field."""
    _fields_ = ([(k, P) for k in ('depth_target', 'depth_weight', 'acc_target', 'acc_weight', 'g_depth1', 'g_acc1', 'g_depth0',
                                  'g_acc0', 'loss4')]
                + [('lambda_depth', F), ('lambda_acc', F)])


class StepMarch(C.Structure):
    """fn_step_march of include/fastnerf.h, field for field."""
    _fields_ = [('K', C.c_int32), ('C', C.c_int32), ('which', C.c_int32), ('u', P), ('seed', U64), ('kidx', P), ('overflow', P),
                ('list_ws', P), ('counts', P)]


class StepBkgd(C.Structure):
    """fn_step_bkgd of include/fastnerf.h, field for field."""
    _fields_ = [('bkgd', P), ('seed', U64), ('alpha', P), ('bkgd_used', P), ('target_ws', P), ('g_acc1', P), ('g_acc0', P)]


class WeightGrads(C.Structure):
    """fn_weight_grads of include/fastnerf.h, field for field."""
    _fields_ = [('g_w1', P), ('g_w0', P)]


class StepDist(C.Structure):
    """fn_step_dist of include/fastnerf.h, field for field."""
    _fields_ = [('lambda_dist', F)] + [(k, P) for k in ('ell1', 'ell0', 'g_w1', 'g_w0', 'loss2d')]


class StepExpo(C.Structure):
    """fn_step_expo of include/fastnerf.h, field for field ('lambda' is set by name: setattr / _term_struct)."""
    _fields_ = ([('img', P), ('ab', P), ('n_img', I), ('lambda', F)]
                + [(k, P) for k in ('e1', 'e0', 'ws', 'd_ab', 'counts', 'loss_reg')])


class OccGrid(C.Structure):
    """fn_occ_grid of include/fastnerf.h, field for field."""
    _fields_ = [('words', P), ('lo', F * 3), ('inv', F * 3), ('n', C.c_int32 * 3), ('outside_occupied', C.c_int32)]


OCC_MAX_LEVELS = 8      # FN_OCC_MAX_LEVELS


class OccCascade(C.Structure):
    """fn_occ_cascade of include/fastnerf.h, field for field."""
    _fields_ = [('levels', C.c_int32), ('reserved', C.c_int32), ('level', OccGrid * OCC_MAX_LEVELS)]


STEP_FORWARD, STEP_BWD_FINE, STEP_BWD_COARSE, STEP_UPDATE = 1, 2, 4, 8
STEP_TIGHTEN = 2      # FN_STEP_TIGHTEN: a bit of StepArgs.fwd_flags

# name -> (restype, argtypes); mirrors include/fastnerf.h one to one
SIGNATURES = {
    'fastnerf_version': (I, []),
    'fastnerf_last_error': (C.c_char_p, []),
    'fastnerf_device_cus': (I, []),
    'fastnerf_x6_pair_launches': (L, []),
    'fastnerf_side_rebuild_passes': (L, []),
    'fastnerf_gen_rays': (I, [I, I, F, F, F, F, P, P, P, P]),
    'fastnerf_gen_rays_pixels': (I, [L, P, P, F, F, F, F, P, P, P]),
    'fastnerf_ndc_rays': (I, [L, I, I, D, F, P, P, P, P, P]),
    'fastnerf_pack_rays': (I, [L, P, P, F, F, I, I, I, D, P, P]),
    'fastnerf_sample_coarse': (I, [L, I, P, I, I, P, U64, P, P]),
    'fastnerf_posenc': (I, [L, I, P, P, P]),
    'fastnerf_mlp_pack': (I, [P, P, P, P]),
    'fastnerf_mlp_fwd': (I, [L, I, P, P, P, P, P, P, P]),
    'fastnerf_mlp_bwd_partial_floats': (L, []),
    'fastnerf_mlp_bwd': (I, [L, I, P, P, P, P, P, P, P, P]),
    'fastnerf_raw2outputs_fwd': (I, [L, I, P, P, P, P, I, P, P, P, P, P, P]),
    'fastnerf_raw2outputs_bwd': (I, [L, I, P, P, P, P, I, P, P, P]),
    'fastnerf_raw2outputs_bwd_full': (I, [L, I, P, P, P, P, I, P, P, P, P, P, P, P, P, P]),
    'fastnerf_sample_pdf_merge': (I, [L, I, I, P, P, I, P, U64, P, P, P, P]),
    'fastnerf_sample_pdf': (I, [L, I, I, P, P, I, P, U64, P, P]),
    'fastnerf_mse_leafmax': (I, [L, P, P, P, F, P, P, P, P, I, P, P]),
    'fastnerf_aux_loss': (I, [L] + [P] * 8 + [F, F, F] + [P] * 5 + [P]),
    'fastnerf_adam_step': (I, [L, P, P, P, P, D, D, D, D, I, P]),
    'fastnerf_net_floats': (L, [I, I]),
    'fastnerf_mlp_act_floats': (L, [I, L]),
    'fastnerf_mlp_pack_ex': (I, [I, P, P, P, P]),
    'fastnerf_mlp_fwd_ex': (I, [I, L, I, P, P, P, P, P, P, P]),
    'fastnerf_mlp_bwd_ex': (I, [I, L, I, P, P, P, P, P, P, P, P]),
    'fastnerf_mlp_bf16_floats': (L, [I, I, L]),
    'fastnerf_mlp_bf16_partial_floats': (L, []),
    'fastnerf_mlp_bf16_pack': (I, [I, P, P, P, P]),
    'fastnerf_mlp_bf16_fwd': (I, [I, L, I, P, P, P, P, P, P, P]),
    'fastnerf_mlp_bf16_bwd': (I, [I, L, I, P, P, P, P, P, P, P, P]),
    'fastnerf_render_rays_fwd': (I, [I, L, I, I, P, I, I, I, I, P, P, P, P, U64, U64, P, P, P, P] + [P] * 18 + [P]),
    'fastnerf_render_rays_fwd_ex': (I, [I, L, I, I, P, I, I, I, I, P, P, P, P, U64, U64, P, P, P, P] + [P] * 18 + [I, P]),
    'fastnerf_mlp_bf16_fwd_flags': (I, [I, L, I, P, P, P, P, P, I, P]),
    'fastnerf_mlp_fwd_flags_ex': (I, [I, L, I, P, P, P, P, P, I, P]),
    'fastnerf_render_rays_bwd': (I, [I, L, I, I, P, I] + [P] * 20),
    'fastnerf_render_rays_bwd_maps': (I, [I, L, I, I, P, I] + [P] * 19 + [P] * 4 + [C.POINTER(MapGrads), P]),
    'fastnerf_pp_intersect_sphere': (I, [L, P, P, P, P]),
    'fastnerf_pp_fg_depths': (I, [L, I, F, P, I, P, U64, P, P]),
    'fastnerf_pp_sample_pdf_merge': (I, [L, I, I, P, P, I, P, U64, P, P, P]),
    'fastnerf_pp_perturb_samples': (I, [L, I, P, P, U64, P, P]),
    'fastnerf_pp_sample_pdf': (I, [L, I, I, P, P, I, P, U64, P, P]),
    'fastnerf_pp_depth2pts_outside': (I, [L, I, P, P, P, P, P, P]),
    'fastnerf_pp_composite_fwd': (I, [L, I, I, P, P, P, P, P, P, P, P, P]),
    'fastnerf_pp_composite_bwd': (I, [L, I, I, P, P, P, P, P, P, P, P]),
    'fastnerf_pp_gen_rays': (I, [I, I, P, P, P, P, P]),
    'fastnerf_leaf_sumcount': (I, [L, P, P, P, I, P, P, P]),
    'fastnerf_tree_adjust_mean': (L, [P, P, P, I, D]),
    'fastnerf_tree_create': (P, [I, I, I, I]),
    'fastnerf_tree_destroy': (None, [P]),
    'fastnerf_tree_num_leaves': (I, [P, I]),
    'fastnerf_tree_max_leaves': (I, [P]),
    'fastnerf_tree_min_area': (D, [P, I]),
    'fastnerf_tree_get_leaves': (I, [P, I, P]),
    'fastnerf_tree_set_leaves': (I, [P, I, I, P, D]),
    'fastnerf_tree_leaf_plan': (I, [P, I, D, I, P]),
    'fastnerf_tree_adjust': (L, [P, P, I, D]),
    'fastnerf_tree_epoch_plan': (L, [P, D, I, P, P]),
    'fastnerf_epoch_rays': (I, [L, I, P, P, P, P, I, I, I, F, F, F, F, U64, I] + [P] * 10 + [P]),
    'fastnerf_epoch_rays_shard': (I, [L, I, P, P, P, P, I, I, I, F, F, F, F, U64, I] + [P] * 5 + [L, I, I] + [P] * 5 + [P]),
    'fastnerf_epoch_shard_rows': (L, [L, L, I, I]),
    'fastnerf_gauss_noise': (I, [L, F, U64, P, P]),
    'fastnerf_compact_ws_ints': (L, [L]),
    'fastnerf_compact_live': (I, [L, P, P, P, P, P]),
    'fastnerf_mlp_bf16_fwd_live': (I, [I, L, I, P, P, P, P, P, P, P, P]),
    'fastnerf_mlp_bf16_bwd_live': (I, [I, L, I, P, P, P, P, P, P, P, P, P, P]),
    'fastnerf_mlp_fwd_live_ex': (I, [I, L, I, P, P, P, P, P, P, P, P]),
    'fastnerf_mlp_bwd_live_ex': (I, [I, L, I, P, P, P, P, P, P, P, P, P, P]),
    'fastnerf_render_rays_bwd_live': (I, [I, L, I, I, P, I] + [P] * 22 + [P]),
    'fastnerf_render_rays_bwd_live_maps': (I, [I, L, I, I, P, I] + [P] * 22 + [P] * 4 + [C.POINTER(MapGrads), P]),
    'fastnerf_mlp_x6_packed_floats': (L, [I, I]),
    'fastnerf_mlp_x6_pack': (I, [I, P, P, P, P]),
    'fastnerf_mlp_fold_offset': (L, [I, I]),
    'fastnerf_mlp_x6_fwd': (I, [I, L, I, P, P, P, P, P, P, I, P]),
    'fastnerf_mlp_x6_bwd': (I, [I, L, I, P, P, P, P, P, P, P, P]),
    'fastnerf_mlp_x6_fwd_live': (I, [I, L, I, P, P, P, P, P, P, P, P]),
    'fastnerf_mlp_x6_bwd_live': (I, [I, L, I, P, P, P, P, P, P, P, P, P, P]),
    'fastnerf_step_args_size': (L, []),
    'fastnerf_train_step': (I, [C.POINTER(StepArgs), I, P]),
    'fastnerf_step_aux_size': (L, []),
    'fastnerf_train_step_aux': (I, [C.POINTER(StepArgs), C.POINTER(StepAux), I, P]),
    'fastnerf_comm_unique_id': (I, [C.c_char_p]),
    'fastnerf_comm_init': (I, [C.POINTER(P), C.c_char_p, I, I]),
    'fastnerf_comm_destroy': (I, [P]),
    'fastnerf_allreduce_grads': (I, [P, P, L, C.c_float, P]),
    'fastnerf_allreduce_leaf_table': (I, [P, P, L, P]),
    'fastnerf_allreduce_leaf_sumcount': (I, [P, P, P, L, P]),
    'fastnerf_leaf_table_reset': (I, [P, L, P]),
    'fastnerf_leaf_table_read': (I, [P, P, L, P]),
    'fastnerf_grid_points': (I, [L, L, P, L, P, L, P, L, P, P]),
    'fastnerf_grid_sigma': (I, [L, P, P, P]),
    'fastnerf_mc_ws_bytes': (L, [L, L, L]),
    'fastnerf_mc_count': (I, [P, L, L, L, F, P, P, P]),
    'fastnerf_mc_emit': (I, [P, L, L, L, F, P, P, P, P]),
    'fastnerf_mc_tables': (I, [P, P]),
    'fastnerf_occ_words': (L, [L, L, L]),
    'fastnerf_occ_build': (I, [P, L, L, L, F, I, P, P, P]),
    'fastnerf_occ_from_mask': (I, [P, L, L, L, P, P]),
    'fastnerf_occ_query': (I, [C.POINTER(OccGrid), L, P, P, P]),
    'fastnerf_occ_classify': (I, [C.POINTER(OccGrid), L, I, P, P, P, P, P, P, P]),
    'fastnerf_occ_query_cascade': (I, [C.POINTER(OccCascade), L, P, P, P]),
    'fastnerf_occ_classify_cascade': (I, [C.POINTER(OccCascade), L, I, P, P, P, P, P, P, P]),
    'fastnerf_occ_cell_points': (I, [C.POINTER(OccGrid), L, L, U64, P, P]),
    'fastnerf_occ_update': (I, [P, P, L, L, L, L, L, F, F, I, P, P, P, P]),
    'fastnerf_mlp_fwd_list_ex': (I, [I, L, I, P, P, P, P, P, P, P, I, P]),
    'fastnerf_mlp_bf16_fwd_list': (I, [I, L, I, P, P, P, P, P, P, P, I, P]),
    'fastnerf_mlp_x6_fwd_list': (I, [I, L, I, P, P, P, P, P, P, P, I, P]),
    'fastnerf_render_rays_fwd_occ': (I, [I, L, I, I, P, I, I, I, I, P, P, U64, U64, P, P, P, P, C.POINTER(OccGrid), P, P] + [P] * 16 + [I, P]),
    'fastnerf_render_rays_fwd_occ_cascade': (I, [I, L, I, I, P, I, I, I, I, P, P, U64, U64, P, P, P, P, C.POINTER(OccCascade), P, P] + [P] * 16 + [I, P]),
    'fastnerf_ert_classify': (I, [C.POINTER(OccGrid), C.POINTER(OccCascade), L, I, I, I, P, P, P, F, P, P, P, P, P]),
    'fastnerf_ert_advance': (I, [L, I, I, I, P, P, P, I, P, P, P, P]),
    'fastnerf_render_rays_fwd_ert': (I, [I, L, I, I, P, I, I, I, I, P, P, U64, U64, P, P, P, P, C.POINTER(OccGrid), C.POINTER(OccCascade), F, I,
                                         P, P, P] + [P] * 16 + [I, P]),
    'fastnerf_occ_ray_bounds': (I, [C.POINTER(OccGrid), C.POINTER(OccCascade), L, P, I, P, P, P]),
    'fastnerf_occ_march': (I, [C.POINTER(OccGrid), C.POINTER(OccCascade), L, I, I, P, I, I, I, I, P, F, P, P, P, P, P]),
    'fastnerf_march_list': (I, [L, I, I, I, P, P, P, P, P, P, C.c_int32, P]),
    'fastnerf_render_rays_fwd_march': (I, [I, L, I, I, P, I, I, P, P, C.POINTER(OccGrid), C.POINTER(OccCascade), F, I] + [P] * 10 + [I, P]),
    'fastnerf_occ_march_jitter': (I, [C.POINTER(OccGrid), C.POINTER(OccCascade), L, I, I, P, I, I, I, I, P, F, P, U64, P, P, P, P, P]),
    'fastnerf_march_mask': (I, [L, P, P, P]),
    'fastnerf_step_march_size': (L, []),
    'fastnerf_step_march_ws_ints': (L, [L, I]),
    'fastnerf_train_step_march': (I, [C.POINTER(StepArgs), C.POINTER(StepMarch), I, P]),
    'fastnerf_step_bkgd_size': (L, []),
    'fastnerf_bkgd_blend': (I, [L, P, U64, P, P, P, P, P, P, P, P, P]),
    'fastnerf_bkgd_grad': (I, [L, P, P, P, P, P, P, P, P]),
    'fastnerf_train_step_bkgd': (I, [C.POINTER(StepArgs), C.POINTER(StepAux), C.POINTER(StepBkgd), I, P]),
    'fastnerf_train_step_march_bkgd': (I, [C.POINTER(StepArgs), C.POINTER(StepMarch), C.POINTER(StepBkgd), I, P]),
    'fastnerf_step_dist_size': (L, []),
    'fastnerf_distortion': (I, [L, I, P, P, P, I, P, F, P, P, P, P]),
    'fastnerf_distortion_mean': (I, [L, P, P, P, P]),
    'fastnerf_render_rays_bwd_w': (I, [I, L, I, I, P, I] + [P] * 19 + [P] * 4 + [C.POINTER(MapGrads), C.POINTER(WeightGrads), P]),
    'fastnerf_render_rays_bwd_live_w': (I, [I, L, I, I, P, I] + [P] * 22 + [P] * 4 + [C.POINTER(MapGrads), C.POINTER(WeightGrads), P]),
    'fastnerf_train_step_dist': (I, [C.POINTER(StepArgs), C.POINTER(StepAux), C.POINTER(StepBkgd), C.POINTER(StepDist), I, P]),
    'fastnerf_train_step_march_dist': (I, [C.POINTER(StepArgs), C.POINTER(StepMarch), C.POINTER(StepBkgd), C.POINTER(StepDist), I, P]),
    'fastnerf_mlp_sigma_grad_ws_floats': (L, [I, L]),
    'fastnerf_mlp_sigma_grad': (I, [I, I, L, I, P, P, P, P, P, P, P, P, P]),
    'fastnerf_ray_grad_ws_floats': (L, [I, L, I]),
    'fastnerf_ray_grad': (I, [I, I, L, I, P, P, P, P, P, P, P, P, P, I, P, P]),
    'fastnerf_pose_exp': (I, [I, P, P, P, P]),
    'fastnerf_pose_exp_bwd': (I, [I, P, P, P, P, P]),
    'fastnerf_pose_grad_ws_floats': (L, [L, I]),
    'fastnerf_pose_grad': (I, [L, I, P, P, F, F, F, F, P, P, P, P]),
    'fastnerf_step_expo_size': (L, []),
    'fastnerf_expo_apply': (I, [L, I, P, P, P, P, P, P, P]),
    'fastnerf_expo_grad_ws_floats': (L, [L, I]),
    'fastnerf_expo_grad': (I, [L, I, P, P, F, F, P, P, P, P, P, P, P, P, P]),
    'fastnerf_train_step_expo': (I, [C.POINTER(StepArgs), C.POINTER(StepAux), C.POINTER(StepBkgd), C.POINTER(StepDist), C.POINTER(StepExpo), I, P]),
    'fastnerf_train_step_march_expo': (I, [C.POINTER(StepArgs), C.POINTER(StepMarch), C.POINTER(StepBkgd), C.POINTER(StepDist),
                                           C.POINTER(StepExpo), I, P]),
    'fastnerf_occ_cascade_own': (I, [C.POINTER(OccCascade), I, I, P, P, P, P]),
    'fastnerf_occ_cascade_points': (I, [C.POINTER(OccCascade), P, C.POINTER(L), L, L, U64, P, P]),
    'fastnerf_occ_cascade_update': (I, [C.POINTER(OccCascade), P, P, P, C.POINTER(L), L, L, C.POINTER(F), C.POINTER(P), P]),
    'fastnerf_train_step_cascade': (I, [C.POINTER(StepArgs), C.POINTER(StepAux), C.POINTER(StepBkgd), C.POINTER(StepDist), C.POINTER(StepExpo),
                                        C.POINTER(OccCascade), I, P]),
    'fastnerf_train_step_march_cascade': (I, [C.POINTER(StepArgs), C.POINTER(StepMarch), C.POINTER(StepBkgd), C.POINTER(StepDist),
                                              C.POINTER(StepExpo), C.POINTER(OccCascade), I, P]),
    'fastnerf_env_lookup': (I, [L, P, L, P, I, P, P]),
    'fastnerf_env_grad_ws_bytes': (L, [I]),
    'fastnerf_env_grad': (I, [L, P, L, I, P, P, P, P, P, P, P]),
    'fastnerf_band_apply': (I, [I, P, P, P, P, P]),
    'fastnerf_band_grad': (I, [I, P, P, P, P]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes library; raise loudly when absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(the HIP path has no CPU fallback)')
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if l.fastnerf_step_args_size() != C.sizeof(StepArgs):
            raise RuntimeError('fn_step_args: the ctypes mirror does not match the library (stale libfastnerf.so?)')
        if l.fastnerf_step_aux_size() != C.sizeof(StepAux):
            raise RuntimeError('fn_step_aux: the ctypes mirror does not match the library (stale libfastnerf.so?)')
        if l.fastnerf_step_march_size() != C.sizeof(StepMarch):
            raise RuntimeError('fn_step_march: the ctypes mirror does not match the library (stale libfastnerf.so?)')
        if l.fastnerf_step_bkgd_size() != C.sizeof(StepBkgd):
            raise RuntimeError('fn_step_bkgd: the ctypes mirror does not match the library (stale libfastnerf.so?)')
        if l.fastnerf_step_dist_size() != C.sizeof(StepDist):
            raise RuntimeError('fn_step_dist: the ctypes mirror does not match the library (stale libfastnerf.so?)')
        if l.fastnerf_step_expo_size() != C.sizeof(StepExpo):
            raise RuntimeError('fn_step_expo: the ctypes mirror does not match the library (stale libfastnerf.so?)')
        _lib = l
    return _lib


def check(rc, what):
    if rc is None or rc < 0:
        msg = lib().fastnerf_last_error()
        raise RuntimeError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')
    return rc


def ptr(t):
    """Device (or host) pointer of a contiguous fp32/int32 tensor, or NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), 'tensor must be contiguous'
    return t.data_ptr()


def stream():
    """The HIP stream torch is currently enqueueing on."""
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a CPU tensor')
