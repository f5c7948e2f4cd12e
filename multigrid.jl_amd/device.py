"""ctypes binding of libmgvcycle.so (include/mgvcycle.h) and the device-side hierarchy handle.

This is the Python stand-in for the Julia glue a maintainer would add: it passes
the arrays exactly as Julia's ``SparseMatrixCSC`` holds them - 1-based Int64 ``colptr``/``rowval``,
Float64 ``nzval`` - following the reference's ccall idiom (src/Multigrid/parRelax.jl:61-64).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible, every entry point
raises.

Import order note: PyTorch wheels bundle their own libamdhip64; a process that wants to use torch.cuda as
well must ``import torch`` BEFORE this library is loaded (bench.py and tests/conftest.py do), otherwise the
system HIP runtime this library pulls in shadows torch's and torch.cuda fails to initialise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGVCYCLE_LIB") or os.path.join(_HERE, "csrc", "libmgvcycle.so")   # override: experiment builds

MG_OP_A, MG_OP_P, MG_OP_R = 0, 1, 2
(MG_K_SPMV, MG_K_RESIDUAL, MG_K_SMOOTH, MG_K_RESTRICT, MG_K_PROLONG, MG_K_DSCALE, MG_K_COARSE,
 MG_K_NORM, MG_K_SMOOTH_PROLONG, MG_K_SMOOTH_RESIDUAL, MG_K_SMOOTH_RESIDUAL_NORM, MG_K_FOUR_STAGE, MG_K_GHOST, MG_K_COUNT) = range(14)
KERNEL_NAMES = ["spmv", "residual", "smooth", "restrict", "prolong", "dscale", "coarse", "norm", "smooth+prolong", "smooth+residual",
                "smooth+residual+norm", "four-stage", "ghost-exchange"]

_ll = C.c_longlong
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_lp = C.POINTER(C.c_longlong)
_up = C.POINTER(C.c_uint)
_vp = C.c_void_p

# name -> (restype, argtypes); exactly the symbols include/mgvcycle.h declares
SIGNATURES = {
    "mg_create": (C.c_int, [_ll, _ll, _ll, C.POINTER(_vp)]),
    "mg_set_operator_FP64_INT64": (C.c_int, [_vp, _ll, _ll, _ll, _ll, _lp, _lp, _dp]),
    "mg_set_relax_FP64": (C.c_int, [_vp, _ll, _dp, _ll, _ll, _ll]),
    "mg_set_cycle_type": (C.c_int, [_vp, _ll]),
    "mg_set_relax_type": (C.c_int, [_vp, _ll]),
    "mg_set_grid_hint": (C.c_int, [_vp, _ll, _ll, _ll, _ll]),
    "mg_set_option": (C.c_int, [_vp, C.c_char_p, C.c_double]),
    "mg_set_coarse_dense_inverse_FP64": (C.c_int, [_vp, _ll, _dp]),
    "mg_build_coarse_dense_inverse_FP64": (C.c_int, [_vp]),
    "mg_build_coarse_dense_inverse_CF64": (C.c_int, [_vp]),
    "mg_get_coarse_dense_inverse_FP64": (C.c_int, [_vp, _ll, _dp]),
    "mg_get_coarse_dense_inverse_CF64": (C.c_int, [_vp, _ll, _dp]),
    "mg_dense_inverse_FP64": (C.c_int, [_ll, _ll, _dp, _dp]),
    "mg_dense_inverse_CF64": (C.c_int, [_ll, _ll, _dp, _dp]),
    "mg_graph_launches": (C.c_int, [_vp, _lp, _lp]),
    "mg_set_coarse_lu_FP64_INT64": (C.c_int, [_vp, _ll, _lp, _lp, _dp, _lp, _lp, _dp, _lp, _lp]),
    "mg_set_coarse_gmres_FP64": (C.c_int, [_vp, _ll, _dp]),
    "mg_finalize": (C.c_int, [_vp]),
    "mg_set_nrhs": (C.c_int, [_vp, _ll]),
    "mg_band_form": (C.c_int, [_vp, _ll, C.POINTER(C.c_longlong)]),
    "mg_operator_stream_kernel": (C.c_int, [_vp, _ll, _ll, C.POINTER(C.c_longlong)]),
    "mg_replace_values_FP64": (C.c_int, [_vp, _ll, _ll, _dp, _ll]),
    "mg_rap_FP64": (C.c_int, [_vp, _dp, _ll, _ll, _dp, _lp]),
    "mg_get_values_FP64": (C.c_int, [_vp, _ll, _ll, _dp, _ll]),
    "mg_get_relax_FP64": (C.c_int, [_vp, _ll, _dp, _ll]),
    "mg_destroy": (C.c_int, [_vp]),
    "mg_cycle_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_solve_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _dp]),
    "mg_pcg_FP64": (C.c_int, [_vp, _dp, _dp, _ll, C.c_double, _ll, _lp, _lp, _dp]),
    "mg_pcg_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, C.c_double, _ll, _lp, _lp, _dp]),
    "mg_bicgstab_FP64": (C.c_int, [_vp, _dp, _dp, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_bicgstab_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_fgmres_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_fgmres_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_block_pcg_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp]),
    "mg_block_pcg_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp]),
    "mg_block_bicgstab_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_block_bicgstab_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_block_fgmres_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_block_fgmres_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_kry_dot_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _dp]),
    "mg_kry_norm_dev_FP64": (C.c_int, [_vp, _vp, _ll, _dp]),
    "mg_kry_axpby_dev_FP64": (C.c_int, [_vp, C.c_double, _vp, C.c_double, _vp, _ll]),
    "mg_kry_cg_update_dev_FP64": (C.c_int, [_vp, C.c_double, _vp, _vp, _vp, _vp, _ll, _dp]),
    "mg_kry_cg_p_dev_FP64": (C.c_int, [_vp, C.c_double, _vp, _vp, _ll]),
    "mg_kry_mgs_step_dev_FP64": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "mg_kry_mgs_chain_dev_FP64": (C.c_int, [_vp, _vp, _ll, _ll, _dp]),
    "mg_kry_blk_gram_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _dp]),
    "mg_kry_blk_comb_dev_FP64": (C.c_int, [_vp, _vp, _vp, C.c_double, _vp, _dp, _ll, _ll]),
    "mg_cycle_mixed_FP32": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _ll, _ll]),
    "mg_host_register": (C.c_int, [_vp, _ll]),
    "mg_host_unregister": (C.c_int, [_vp]),
    "mg_spmv_FP64": (C.c_int, [_vp, _ll, _ll, C.c_double, _dp, C.c_double, _dp, _ll]),
    "mg_cycle_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_solve_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, C.c_double, _ll, _lp, _dp]),
    "mg_spmv_dev_FP64": (C.c_int, [_vp, _ll, _ll, C.c_double, _vp, C.c_double, _vp, _ll]),
    "mg_fused_dev_FP64": (C.c_int, [_vp, _ll, _ll, _vp, _vp, _vp, _ll]),
    "mg_sweep_residual_dev_FP64": (C.c_int, [_vp, _ll, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "mg_four_stage_dev_FP64": (C.c_int, [_vp, _ll, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "mg_four_stage_form": (C.c_int, [_vp, _ll, _lp, _lp]),
    "mg_transpose_hierarchy": (C.c_int, [_vp]),
    "mg_operator_shape": (C.c_int, [_vp, _ll, _ll, _lp]),
    "mg_time_op_dev_FP64": (C.c_int, [_vp, _ll, _ll, _ll, _ll, _dp, _dp]),
    "mg_profile_enable": (C.c_int, [_vp, _ll]),
    "mg_profile_get": (C.c_int, [_vp, _ll, _ll, _dp, _lp, _dp]),
    "mg_profile_reset": (C.c_int, [_vp]),
    "mg_profile_get_moved": (C.c_int, [_vp, _ll, _ll, _dp]),
    "mg_operator_format": (C.c_int, [_vp, _ll, _ll, _lp, _lp, _dp]),
    "mg_operator_rowclasses": (C.c_int, [_vp, _ll, _ll, _lp, _lp, _dp]),
    "mg_operator_rowclass_flags": (C.c_int, [_vp, _ll, _ll, _lp, _lp, _lp, _lp]),
    "mg_sweep_residual_form": (C.c_int, [_vp, _ll, _lp, _lp]),
    "mg_cycle_bytes": (C.c_int, [_vp, _dp]),
    "mg_device_bytes": (C.c_int, [_vp, _dp]),
    "mg_op_create_FP64_INT64": (C.c_int, [_ll, _ll, _ll, _lp, _lp, _dp, C.POINTER(_vp)]),
    "mg_op_create_box_FP64_INT64": (C.c_int, [_ll, _ll, _ll, _lp, _lp, _dp, _ll, _ll, _ll, _ll, C.POINTER(_vp)]),
    "mg_op_create_grid_FP64_INT64": (C.c_int, [_ll, _ll, _ll, _lp, _lp, _dp, _ll, _ll, _ll, _ll, _ll, _ll, _ll,
                                               C.POINTER(_vp)]),
    "mg_op_bind_relax_dev_FP64": (C.c_int, [_vp, _vp, _ll]),
    "mg_op_kernel_variant": (C.c_int, [_vp, _lp, _lp]),
    "mg_op_apply_phase_dev_FP64": (C.c_int, [_vp, _ll, C.c_double, _vp, C.c_double, _vp, _vp, _vp, _ll, _ll, _ll, _vp]),
    "mg_dist_set_level_box": (C.c_int, [_vp, _ll, _ll]),
    "mg_dist_set_relax_type": (C.c_int, [_vp, _ll]),
    "mg_kcycle_step_async_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll]),
    "mg_op_residual_fused_dev_FP64": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _lp, _vp]),
    "mg_op_can_fuse_next": (C.c_int, [_vp, _vp, _lp]),
    "mg_op_can_sweep_residual": (C.c_int, [_vp, _vp, _vp, _lp, _lp, _lp]),
    "mg_op_sweep_residual_dev_FP64": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _lp, _vp]),
    "mg_op_apply_list_dev_FP64": (C.c_int, [_vp, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _lp, _vp]),
    "mg_op_destroy": (C.c_int, [_vp]),
    "mg_op_apply_dev_FP64": (C.c_int, [_vp, _ll, C.c_double, _vp, C.c_double, _vp, _vp, _vp, _ll, _vp]),
    "mg_op_apply_rows_dev_FP64": (C.c_int, [_vp, _ll, C.c_double, _vp, C.c_double, _vp, _vp, _vp, _ll, _ll, _vp]),
    "mg_op_info": (C.c_int, [_vp, _lp, _lp, _lp, _dp]),
    "mg_vec_dscale_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _vp]),
    "mg_vec_xpdr_dev_FP64": (C.c_int, [_vp, _vp, _vp, _vp, _ll, _ll, _vp]),
    "mg_vec_sumsq_dev_FP64": (C.c_int, [_vp, _ll, _vp, _vp, _vp]),
    "mg_set_stream": (C.c_int, [_vp, _vp]),
    "mg_cycle_async_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_lu_create_FP64_INT64": (C.c_int, [_ll, _ll, _lp, _lp, _dp, _lp, _lp, _dp, _lp, _lp, C.POINTER(_vp)]),
    "mg_lu_solve_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_lu_solve_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_lu_create_CFP64_INT64": (C.c_int, [_ll, _ll, _lp, _lp, _dp, _lp, _lp, _dp, _lp, _lp, C.POINTER(_vp)]),
    "mg_lu_solve_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_lu_solve_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_lu_create_FP32_UINT32": (C.c_int, [_ll, _ll, _lp, _up, _fp, _lp, _up, _fp, _up, _up, C.POINTER(_vp)]),
    "mg_lu_create_CFP32_UINT32": (C.c_int, [_ll, _ll, _lp, _up, _fp, _lp, _up, _fp, _up, _up, C.POINTER(_vp)]),
    "mg_lu_create_CFP32_INT64": (C.c_int, [_ll, _ll, _lp, _lp, _fp, _lp, _lp, _fp, _lp, _lp, C.POINTER(_vp)]),
    "mg_lu_solve_FP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, _ll]),
    "mg_lu_solve_dev_FP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_lu_solve_CFP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, _ll]),
    "mg_lu_solve_dev_CFP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_lu_form": (C.c_int, [_vp, _ll, _lp]),
    "mg_lu_time_dev": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _ll, _dp]),
    "mg_lu_destroy": (C.c_int, [_vp]),
    "mg_dd_create_FP64_INT64": (C.c_int, [_ll, _ll, _lp, _lp, _dp, _ll, _lp, C.POINTER(C.c_uint), _lp, C.POINTER(_vp)]),
    "mg_dd_create_CFP64_INT64": (C.c_int, [_ll, _ll, _lp, _lp, _dp, _ll, _lp, C.POINTER(C.c_uint), _lp, C.POINTER(_vp)]),
    "mg_dd_set_factor_FP64_INT64": (C.c_int, [_vp, _ll, _ll, _lp, _lp, _dp, _lp, _lp, _dp, _lp, _lp]),
    "mg_dd_set_factor_CFP64_INT64": (C.c_int, [_vp, _ll, _ll, _lp, _lp, _dp, _lp, _lp, _dp, _lp, _lp]),
    "mg_dd_finalize": (C.c_int, [_vp]),
    "mg_dd_apply_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_dd_apply_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_dd_apply_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_dd_apply_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_dd0_apply_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll]),
    "mg_dd0_apply_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_dd0_apply_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll]),
    "mg_dd0_apply_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_dd_create_FP32_INT64": (C.c_int, [_ll, _ll, _lp, _lp, _fp, _ll, _lp, C.POINTER(C.c_uint), _lp, C.POINTER(_vp)]),
    "mg_dd_create_CFP32_INT64": (C.c_int, [_ll, _ll, _lp, _lp, _fp, _ll, _lp, C.POINTER(C.c_uint), _lp, C.POINTER(_vp)]),
    "mg_dd_set_factor_FP32_UINT32": (C.c_int, [_vp, _ll, _ll, _lp, _up, _fp, _lp, _up, _fp, _up, _up]),
    "mg_dd_set_factor_CFP32_UINT32": (C.c_int, [_vp, _ll, _ll, _lp, _up, _fp, _lp, _up, _fp, _up, _up]),
    "mg_dd_set_factor_CFP32_INT64": (C.c_int, [_vp, _ll, _ll, _lp, _lp, _fp, _lp, _lp, _fp, _lp, _lp]),
    "mg_dd_apply_FP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, _ll]),
    "mg_dd_apply_dev_FP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_dd_apply_CFP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, _ll]),
    "mg_dd_apply_dev_CFP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_dd0_apply_FP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll]),
    "mg_dd0_apply_dev_FP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_dd0_apply_CFP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll]),
    "mg_dd0_apply_dev_CFP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_set_coarse_dd": (C.c_int, [_vp, _vp]),
    "mg_coarse_form": (C.c_int, [_vp, _lp]),
    "mg_dd_info": (C.c_int, [_vp, _lp]),
    "mg_dd_time_dev": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _dp]),
    "mg_dd_destroy": (C.c_int, [_vp]),
    "mg_kaczmarz_create_FP64_INT64": (C.c_int, [_ll, _ll, _lp, _dp, _lp, _ll, _ll, C.POINTER(C.c_uint), _dp, C.POINTER(_vp)]),
    "mg_kaczmarz_apply_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_kaczmarz_apply_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_kaczmarz_create_CFP64_INT64": (C.c_int, [_ll, _ll, _lp, _dp, _lp, _ll, _ll, C.POINTER(C.c_uint), _dp, C.POINTER(_vp)]),
    "mg_kaczmarz_apply_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_kaczmarz_apply_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_kaczmarz_create_FP32_INT64": (C.c_int, [_ll, _ll, _lp, _fp, _lp, _ll, _ll, C.POINTER(C.c_uint), _fp, C.POINTER(_vp)]),
    "mg_kaczmarz_apply_FP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, _ll]),
    "mg_kaczmarz_apply_dev_FP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_kaczmarz_create_CFP32_INT64": (C.c_int, [_ll, _ll, _lp, _fp, _lp, _ll, _ll, C.POINTER(C.c_uint), _fp, C.POINTER(_vp)]),
    "mg_kaczmarz_apply_CFP32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, _ll]),
    "mg_kaczmarz_apply_dev_CFP32": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_kaczmarz_destroy": (C.c_int, [_vp]),
    "mg_set_vanka_FP64": (C.c_int, [_vp, _ll, _ll, _lp, _ll, _ll, C.POINTER(C.c_float)]),
    "mg_vanka_create_FP64_INT64": (C.c_int, [_ll, _ll, _lp, _ll, _ll, _lp, _lp, _dp, C.POINTER(C.c_float), C.POINTER(_vp)]),
    "mg_vanka_create_CFP64_INT64": (C.c_int, [_ll, _ll, _lp, _ll, _ll, _lp, _lp, _dp, C.POINTER(C.c_float), C.POINTER(_vp)]),
    "mg_vanka_apply_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll]),
    "mg_vanka_apply_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_vanka_apply_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll]),
    "mg_vanka_apply_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_vanka_apply_block_FP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_vanka_apply_block_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_vanka_apply_block_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_vanka_apply_block_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_vanka_time_block_dev": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _dp]),
    "mg_vanka_info": (C.c_int, [_vp, _lp]),
    "mg_vanka_time_dev": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll, _dp]),
    "mg_vanka_create_built_FP64_INT64": (C.c_int, [_ll, _ll, _lp, _ll, _ll, _lp, _lp, _dp, _ll, _dp, _ll, C.POINTER(_vp)]),
    "mg_vanka_create_built_CFP64_INT64": (C.c_int, [_ll, _ll, _lp, _ll, _ll, _lp, _lp, _dp, _ll, _dp, _ll, C.POINTER(_vp)]),
    "mg_vanka_build_blocks_FP64": (C.c_int, [_vp, _ll, _dp, _ll]),
    "mg_vanka_build_blocks_CFP64": (C.c_int, [_vp, _ll, _dp, _ll]),
    "mg_vanka_replace_values_FP64": (C.c_int, [_vp, _dp, _ll]),
    "mg_vanka_replace_values_CFP64": (C.c_int, [_vp, _dp, _ll]),
    "mg_vanka_get_blocks": (C.c_int, [_vp, C.POINTER(C.c_float), _ll]),
    "mg_vanka_time_build": (C.c_int, [_vp, _ll, _dp, _ll, _ll, _ll, _dp]),
    "mg_vanka_destroy": (C.c_int, [_vp]),
    "mg_dist_unique_id": (C.c_int, [C.c_char_p]),
    "mg_dist_create": (C.c_int, [_ll, _ll, _ll, C.c_char_p, _ll, _ll, _ll, C.POINTER(_vp)]),
    "mg_dist_set_exchange_plugin": (C.c_int, [_vp, _vp, _vp]),
    "mg_dist_set_level": (C.c_int, [_vp, _ll, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _ll, _ll]),
    "mg_dist_set_plan_INT64": (C.c_int, [_vp, _ll, _ll, _ll, _ll, _ll, _lp, _lp, _lp, _ll]),
    "mg_dist_set_tail_INT64": (C.c_int, [_vp, _vp, _ll, _ll, _ll, _lp]),
    "mg_dist_finalize": (C.c_int, [_vp]),
    "mg_dist_cycle_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_dist_solve_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, C.c_double, _ll, _lp, _dp]),
    "mg_dist_set_nrhs": (C.c_int, [_vp, _ll]),
    "mg_dist_release_tail": (C.c_int, [_vp]),
    "mg_dist_comm_count": (C.c_int, [_vp, _lp]),
    "mg_dist_pcg_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, C.c_double, _ll, _lp, _lp, _dp]),
    "mg_dist_bicgstab_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_dist_fgmres_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_dist_stats": (C.c_int, [_vp, _lp, _lp]),
    "mg_vec_dots_dev_FP64": (C.c_int, [_ll, C.POINTER(_vp), C.POINTER(_vp), _ll, _vp, _vp, _vp]),
    "mg_vec_pcg_dots_dev_FP64": (C.c_int, [_vp, _vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_vec_pcg_update_dev_FP64": (C.c_int, [C.c_double, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_vec_xpby_dev_FP64": (C.c_int, [_vp, C.c_double, _vp, _ll, _vp]),
    "mg_vec_scale_dev_FP64": (C.c_int, [C.c_double, _vp, _vp, _ll, _vp]),
    "mg_vec_bicg_p_dev_FP64": (C.c_int, [C.c_double, C.c_double, _vp, _vp, _vp, _ll, _vp]),
    "mg_vec_bicg_s_dev_FP64": (C.c_int, [C.c_double, _vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_vec_bicg_ts_dev_FP64": (C.c_int, [_vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_vec_bicg_xr_dev_FP64": (C.c_int, [C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_vec_gs_update_dev_FP64": (C.c_int, [_ll, _dp, C.POINTER(_vp), _vp, _ll, _vp, _vp, _vp]),
    "mg_dist_destroy": (C.c_int, [_vp]),
    "mg_ghost_attach": (C.c_int, [_vp, _ll, _ll, _ll, C.c_char_p]),
    "mg_ghost_set_exchange_plugin": (C.c_int, [_vp, _vp, _vp]),
    "mg_ghost_set_side_comm": (C.c_int, [_vp, C.c_char_p]),
    "mg_ghost_set_level_INT64": (C.c_int, [_vp, _ll, _lp, _lp, _lp, _ll, _ll, _lp, _lp, _ll, _lp, _lp]),
    "mg_ghost_finalize": (C.c_int, [_vp]),
    "mg_ghost_set_dry": (C.c_int, [_vp, _ll]),
    "mg_ghost_stats": (C.c_int, [_vp, _lp, _lp]),
    "mg_ghost_comm_count": (C.c_int, [_vp, _lp]),
    "mg_ghost_allreduce_count": (C.c_int, [_vp, _lp]),
    "mg_create_CF64": (C.c_int, [_ll, _ll, _ll, C.POINTER(_vp)]),
    "mg_set_operator_CF64_INT64": (C.c_int, [_vp, _ll, _ll, _ll, _ll, _lp, _lp, _dp]),
    "mg_set_relax_CF64": (C.c_int, [_vp, _ll, _dp, _ll, _ll, _ll]),
    "mg_set_schedule_CF64": (C.c_int, [_vp, _ll, _ll]),
    "mg_set_vanka_CF64": (C.c_int, [_vp, _ll, _ll, _lp, _ll, _ll, C.POINTER(C.c_float)]),
    "mg_set_vanka_CF32": (C.c_int, [_vp, _ll, _ll, _lp, _ll, _ll, C.POINTER(C.c_float)]),
    "mg_build_vanka_CF64": (C.c_int, [_vp, _ll, _ll, _lp, _ll, _ll, _dp, _ll]),
    "mg_build_vanka_CF32": (C.c_int, [_vp, _ll, _ll, _lp, _ll, _ll, _dp, _ll]),
    "mg_get_vanka_blocks_CF64": (C.c_int, [_vp, _ll, C.POINTER(C.c_float), _ll]),
    "mg_get_vanka_blocks_CF32": (C.c_int, [_vp, _ll, C.POINTER(C.c_float), _ll]),
    "mg_set_vanka_relax_CF64": (C.c_int, [_vp, _ll]),
    "mg_set_vanka_relax_CF32": (C.c_int, [_vp, _ll]),
    "mg_fgmres_relax_CF64": (C.c_int, [_vp, _ll, _dp, _dp, _ll, _ll, C.c_double, _dp, _dp, _dp, _lp]),
    "mg_set_schedule_CF32": (C.c_int, [_vp, _ll, _ll]),
    "mg_fgmres_relax_CF32": (C.c_int, [_vp, _ll, _fp, _fp, _ll, _ll, C.c_double, _dp, _dp, _dp, _lp, _fp, _fp]),
    "mg_set_coarse_dense_inverse_CF64": (C.c_int, [_vp, _ll, _dp]),
    "mg_set_coarse_lu_CF64_INT64": (C.c_int, [_vp, _ll, _lp, _lp, _dp, _lp, _lp, _dp, _lp, _lp]),
    "mg_set_coarse_lu_CF32_INT64": (C.c_int, [_vp, _ll, _lp, _lp, _fp, _lp, _lp, _fp, _lp, _lp]),
    "mg_set_coarse_gmres_CF64": (C.c_int, [_vp, _ll, _dp]),
    "mg_coarse_gmres_CF64": (C.c_int, [_vp, _dp, _dp, _ll, _lp, _lp, _dp]),
    "mg_block_coarse_gmres_CF64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _lp, _lp, _dp]),
    "mg_block_coarse_form": (C.c_int, [_vp, _ll, _lp]),
    "mg_cycle_CF64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_solve_CF64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _dp]),
    "mg_spmv_CF64": (C.c_int, [_vp, _ll, _ll, _dp, _dp, _dp, _dp, _ll]),
    "mg_set_krylov_operator_CFP64_INT64": (C.c_int, [_vp, _ll, _lp, _lp, _dp]),
    "mg_replace_krylov_values_CFP64": (C.c_int, [_vp, _dp, _ll]),
    "mg_rap_CF64": (C.c_int, [_vp, _dp, _ll, _ll, _dp, _lp]),
    "mg_rap_level_ms_CF64": (C.c_int, [_vp, _dp, _ll]),
    "mg_get_values_CF64": (C.c_int, [_vp, _ll, _ll, _dp, _ll]),
    "mg_get_relax_CF64": (C.c_int, [_vp, _ll, _dp, _ll]),
    "mg_replace_values_CF64": (C.c_int, [_vp, _ll, _ll, _dp, _ll]),
    "mg_rap_CF32": (C.c_int, [_vp, _fp, _ll, _ll, _dp, _lp]),
    "mg_rap_level_ms_CF32": (C.c_int, [_vp, _dp, _ll]),
    "mg_get_values_CF32": (C.c_int, [_vp, _ll, _ll, _fp, _ll]),
    "mg_get_relax_CF32": (C.c_int, [_vp, _ll, _fp, _ll]),
    "mg_replace_values_CF32": (C.c_int, [_vp, _ll, _ll, _fp, _ll]),
    "mg_adjoint_hierarchy_CF64": (C.c_int, [_vp]),
    "mg_adjoint_hierarchy_CF32": (C.c_int, [_vp]),
    "mg_bicgstab_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_bicgstab_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_fgmres_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_fgmres_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_cycle_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll]),
    "mg_block_spmv_CF64": (C.c_int, [_vp, _ll, _ll, _dp, _dp, _dp, _dp, _ll]),
    "mg_block_cycle_CF64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll]),
    "mg_block_fgmres_relax_CF64": (C.c_int, [_vp, _ll, _dp, _dp, _ll, _ll, _ll, C.c_double, _dp, _dp, _dp, _lp, _dp, _dp]),
    "mg_block_fgmres_relax_CF32": (C.c_int, [_vp, _ll, _dp, _dp, _ll, _ll, _ll, C.c_double, _dp, _dp, _dp, _lp, _dp, _dp]),
    "mg_block_solve_CF64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _dp]),
    "mg_block_cycle_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll]),
    "mg_block_bicgstab_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_block_bicgstab_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_block_fgmres_CFP64": (C.c_int, [_vp, _dp, _dp, _ll, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_block_fgmres_dev_CFP64": (C.c_int, [_vp, _vp, _vp, _ll, _ll, _ll, C.c_double, _ll, _lp, _lp, _dp, _lp]),
    "mg_cblk_gram_dev_CFP64": (C.c_int, [_vp, _vp, _ll, _ll, _vp, _vp, _vp]),
    "mg_create_CF32": (C.c_int, [_ll, _ll, _ll, C.POINTER(_vp)]),
    "mg_set_operator_CF32_INT64": (C.c_int, [_vp, _ll, _ll, _ll, _ll, _lp, _lp, _fp]),
    "mg_set_relax_CF32": (C.c_int, [_vp, _ll, _fp, _ll, _ll, _ll]),
    "mg_cycle_CF32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, _ll]),
    "mg_solve_CF32": (C.c_int, [_vp, _fp, _fp, _ll, _ll, C.c_double, _ll, _lp, _dp]),
    "mg_spmv_CF32": (C.c_int, [_vp, _ll, _ll, _fp, _fp, _fp, _fp, _ll]),
    "mg_cvec_dots_dev_CFP64": (C.c_int, [_ll, C.POINTER(_vp), C.POINTER(_vp), _ll, _vp, _vp, _vp]),
    "mg_cvec_scale_dev_CFP64": (C.c_int, [_dp, _vp, _vp, _ll, _vp]),
    "mg_cvec_bicg_p_dev_CFP64": (C.c_int, [_dp, _dp, _vp, _vp, _vp, _ll, _vp]),
    "mg_cvec_bicg_s_dev_CFP64": (C.c_int, [_dp, _vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_cvec_bicg_ts_dev_CFP64": (C.c_int, [_vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_cvec_bicg_xr_dev_CFP64": (C.c_int, [_dp, _dp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp]),
    "mg_cvec_gs_update_dev_CFP64": (C.c_int, [_ll, _dp, C.POINTER(_vp), _vp, _ll, _vp, _vp, _vp]),
    "mg_last_error": (C.c_char_p, []),
    "mg_version": (C.c_char_p, []),
}

_lib = None


class MGDeviceError(RuntimeError):
    pass


def load_library(path: Optional[str] = None):
    """dlopen libmgvcycle.so and bind every symbol of the header.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise MGDeviceError(
            f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the multigrid cycle.")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export the symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.mg_last_error()
        raise MGDeviceError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")


def _f64(a):
    return a.ctypes.data_as(_dp)


def _i64(a):
    return a.ctypes.data_as(_lp)


def _f32(a):
    return a.ctypes.data_as(_fp)


def _u32(a):
    return a.ctypes.data_as(_up)


def _julia_arrays(M):
    """scipy CSR -> the (colptr, rowval, nzval) triple Julia holds for the transposed CSC (1-based Int64)."""
    colptr = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
    rowval = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
    nzval = np.ascontiguousarray(M.data, dtype=np.float64)
    return colptr, rowval, nzval


def _ptr(t) -> int:
    """Device address of a torch tensor / raw int."""
    if isinstance(t, int):
        return t
    if hasattr(t, "data_ptr"):
        if not t.is_cuda:
            raise MGDeviceError("device API called with a CPU tensor")
        if not t.is_contiguous():
            raise MGDeviceError("device API needs contiguous tensors")
        return int(t.data_ptr())
    raise TypeError("expected a torch CUDA tensor or an integer device address")


def _sync_torch(*tensors):
    """The library enqueues on its OWN non-blocking stream, which does not order against torch's: whatever torch still has in
    flight for these tensors (a fill, a copy, the kernel that produced them) must have landed before the library touches them."""
    for t in tensors:
        if t is not None and hasattr(t, "is_cuda") and t.is_cuda:
            import torch
            torch.cuda.current_stream(t.device).synchronize()
            return


DENSE_COARSE_MAX = 16384
MG_ERR_INVALID = 1
MG_ERR_STATE = 3
MG_ERR_UNSUPPORTED = 4


def dense_inverse(A, device: int = 0) -> np.ndarray:
    """inv(A) of a dense float64 or complex128 matrix of order <= 8192 on the device (mg_dense_inverse_FP64 / _CF64): partial
    pivoting, one host synchronisation, the same bits on every run.  A singular matrix (a zero or non-finite pivot) raises
    ``np.linalg.LinAlgError``, as ``np.linalg.inv`` does; every other refusal is an MGDeviceError."""
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("dense_inverse takes a square matrix")
    cx = np.iscomplexobj(A)
    Af = np.asfortranarray(A, dtype=np.complex128 if cx else np.float64)
    out = np.zeros_like(Af, order="F")
    lib = load_library()
    what = "mg_dense_inverse_CF64" if cx else "mg_dense_inverse_FP64"
    rc = getattr(lib, what)(int(device), Af.shape[0], Af.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    if rc == MG_ERR_INVALID and Af.shape[0] >= 1:
        msg = lib.mg_last_error()
        raise np.linalg.LinAlgError(f"{what}: {msg.decode() if msg else 'singular matrix'}")
    _check(lib, rc, what)
    return out
BLOCK_KMAX = 16                  # columns of a complex block of right-hand sides (mgk::BLK_KMAX)


def _relax_type_code(param) -> int:
    """mg_set_relax_type: 0 pointwise (Jac / SPAI), 1 Jac-GMRES, 2 the Vanka smoothers."""
    from .vanka import getVankaRelaxType
    if getVankaRelaxType(param.relaxType)[0]:
        return 2
    return 1 if param.relaxType == "Jac-GMRES" else 0


def _vanka_guard(param, nrhs: int):
    """What a Vanka hierarchy does not serve, refused before the device is touched."""
    from .vanka import getVankaRelaxType, FULL_VANKA_LEX
    isVanka, vtype = getVankaRelaxType(param.relaxType)
    if not isVanka:
        return
    if vtype == FULL_VANKA_LEX:
        raise NotImplementedError("FULL_VANKA_LEX is a sequential sweep over the cells; the package keeps no CPU fallback")
    if int(nrhs) != 1:
        raise NotImplementedError("Vanka hierarchies serve one right-hand side (blocks of right-hand sides are out of scope)")
    val = np.dtype(getattr(param, "VAL", np.float64))
    if val.kind == "c":
        if not getattr(param, "complexVanka", False):
            raise NotImplementedError("complex Vanka hierarchies are asked for with getMGparam(np.complex128, ..., complexVanka=True)")
        from .mgdef import _solver_object
        if _solver_object(param.LU) == "dd":
            raise NotImplementedError("complex Vanka hierarchies: a Schwarz coarsest solve is out of scope")
    if param.cycleType == "K" and val != np.complex128 and not (val == np.complex64 and getattr(param, "singleKcycle", False)):
        raise NotImplementedError("Vanka hierarchies serve the V, W and F cycles (cycleType='K': ComplexF64 hierarchies only)")
    if param.transferOperatorType not in ("SystemsFacesLinear", "SystemsFacesMixedLinear") or not param.Meshes:
        raise NotImplementedError("Vanka hierarchies need the staggered meshes of MGsetup with a Systems transfer operator")


class DeviceHierarchy:
    """Owns one ``mg_hierarchy`` handle (HBM copy of As/Ps/Rs/relaxPrecs + coarse inverse).

    Dtype-aware: a param with VAL = ComplexF64 gets a ComplexDeviceHierarchy (the _CF64 entry points), one with VAL = ComplexF32
    (singlePrecision=True) a ComplexSingleDeviceHierarchy (the _CF32 entry points)."""

    def __new__(cls, param=None, *args, **kwargs):
        val = np.dtype(getattr(param, "VAL", np.float64)) if param is not None else None
        if cls is DeviceHierarchy and val == np.complex128:
            cls = ComplexDeviceHierarchy
        elif cls is DeviceHierarchy and val == np.complex64:
            cls = ComplexSingleDeviceHierarchy
        return super().__new__(cls)

    def __init__(self, param, device_id: int = 0, nrhs: Optional[int] = None, options: Optional[dict] = None):
        """options: per-handle format switches (mg_set_option), e.g. {"no_rowclass": 1} forces the streaming formats."""
        self.lib = load_library()
        self.handle = _vp()
        self.nlevels = len(param.As)
        self.n = int(param.As[0].shape[0])
        self.nrhs = int(nrhs if nrhs is not None else max(1, param.nrhs))
        lib = self.lib
        _check(lib, lib.mg_create(self.nlevels, self.nrhs, int(device_id), C.byref(self.handle)), "mg_create")
        try:
            for key, val in (options or {}).items():
                _check(lib, lib.mg_set_option(self.handle, key.encode(), float(val)), f"mg_set_option({key})")
            self._upload(param)
        except Exception:
            self.close()
            raise

    # -- setup ------------------------------------------------------------------------------------
    def _set_op(self, level, which, M):
        colptr, rowval, nzval = _julia_arrays(M)
        rc = self.lib.mg_set_operator_FP64_INT64(self.handle, level, which, M.shape[0], M.shape[1],
                                                 _i64(colptr), _i64(rowval), _f64(nzval))
        _check(self.lib, rc, f"mg_set_operator(level={level}, which={which})")

    def _set_relax_level(self, param, l, pre, post):
        """relaxPrecs[l]: the pointwise vector, or (Vanka) the cells' blocks - then the pointwise slot holds zeros, which
        nothing reads, and carries the sweep counts."""
        lib = self.lib
        if self._vanka:
            from .vanka import getVankaRelaxType
            blk = np.asfortranarray(param.relaxPrecs[l - 1], dtype=np.float32)
            nn = np.ascontiguousarray(param.Meshes[l - 1].n, dtype=np.int64)
            mixed = param.transferOperatorType == "SystemsFacesMixedLinear"
            _check(lib, lib.mg_set_vanka_FP64(self.handle, l, nn.size, _i64(nn), 1 if mixed else 0,
                                              getVankaRelaxType(param.relaxType)[1], blk.ctypes.data_as(C.POINTER(C.c_float))),
                   f"mg_set_vanka(level={l})")
            d = np.zeros(param.As[l - 1].shape[0], dtype=np.float64)
        else:
            d = np.ascontiguousarray(param.relaxPrecs[l - 1], dtype=np.float64)
        _check(lib, lib.mg_set_relax_FP64(self.handle, l, _f64(d), d.size, int(pre), int(post)), f"mg_set_relax(level={l})")

    def _upload(self, param):
        lib = self.lib
        nl = self.nlevels
        _vanka_guard(param, self.nrhs)
        self._vanka = _relax_type_code(param) == 2
        for l in range(1, nl + 1):
            self._set_op(l, MG_OP_A, param.As[l - 1])
            if l < nl:
                self._set_op(l, MG_OP_P, param.Ps[l - 1])
                self._set_op(l, MG_OP_R, param.Rs[l - 1])
                self._set_relax_level(param, l, param.relaxPre(l), param.relaxPost(l))
        # performance hint only: GMG levels are regular nodal grids (param.Meshes, MGsetup.jl:54)
        for l, mesh in enumerate(getattr(param, "Meshes", []) or []):
            if l < nl and mesh is not None:
                nn = [int(k) + 1 for k in mesh.n] + [1]
                if int(np.prod(nn)) == param.As[l].shape[0] and not self._vanka:
                    _check(lib, lib.mg_set_grid_hint(self.handle, l + 1, nn[0], nn[1], nn[2]), "mg_set_grid_hint")
        _check(lib, lib.mg_set_relax_type(self.handle, _relax_type_code(param)), "mg_set_relax_type")
        _check(lib, lib.mg_set_cycle_type(self.handle, ord(param.cycleType)), "mg_set_cycle_type")
        if param.LU is None:
            raise MGDeviceError("param.LU is empty: run MGsetup / SA_AMGsetup first")
        self._set_coarse(param)
        _check(lib, lib.mg_finalize(self.handle), "mg_finalize")
        self._schedule = self._schedule_of(param)

    def _schedule_of(self, param):
        nl = self.nlevels
        return (param.cycleType, param.relaxType, tuple(int(param.relaxPre(l)) for l in range(1, nl)),
                tuple(int(param.relaxPost(l)) for l in range(1, nl)))

    def sync_schedule(self, param):
        """Push cycleType / relaxType / sweep counts to the device when they were changed on ``param`` after the upload."""
        sig = self._schedule_of(param)
        if sig == getattr(self, "_schedule", sig):
            self._schedule = sig
            return
        lib = self.lib
        old = self._schedule
        refinalize = False
        _vanka_guard(param, self.nrhs)
        if (_relax_type_code(param) == 2) != self._vanka or (self._vanka and sig[1] != old[1]):
            raise NotImplementedError("relaxType changed to or from a Vanka smoother after the setup: relaxPrecs hold the other "
                                      "smoother's data - run MGsetup again")
        if sig[1] != old[1]:
            _check(lib, lib.mg_set_relax_type(self.handle, _relax_type_code(param)), "mg_set_relax_type")
            refinalize = True
        if sig[2] != old[2] or sig[3] != old[3]:
            for l in range(1, self.nlevels):
                self._set_relax_level(param, l, sig[2][l - 1], sig[3][l - 1])
            refinalize = True
        if sig[0] != old[0]:
            _check(lib, lib.mg_set_cycle_type(self.handle, ord(param.cycleType)), "mg_set_cycle_type")
            refinalize = refinalize or "K" in (sig[0], old[0])
        if refinalize:
            _check(lib, lib.mg_finalize(self.handle), "mg_finalize")
        self._schedule = sig

    def _set_coarse(self, param, force_sparse: bool = False):
        """`z = param.LU\\b` (MGcycle.jl:177) on the device: the explicit inverse for small coarsest levels, the sparse
        L/U factors in the reference's parLU layout (mg_set_coarse_lu_FP64_INT64) above DENSE_COARSE_MAX rows."""
        import scipy.sparse as sp
        lib = self.lib
        nc = int(param.As[-1].shape[0])
        self._coarse_device_inverse = False
        if self._set_coarse_solver(param):
            return
        if param.coarseSolveType == "GMRES":                            # param.LU = relaxParam ./ diag(A_c)
            d = np.ascontiguousarray(param.LU, dtype=np.float64)
            _check(lib, lib.mg_set_coarse_gmres_FP64(self.handle, nc, _f64(d)), "mg_set_coarse_gmres")
            return
        if nc <= DENSE_COARSE_MAX and not force_sparse:
            if self._build_coarse_inverse(param):                       # coarseDeviceInverse: inv(As[end]) built in HBM
                return
            Ainv = np.asfortranarray(param.LU.solve(np.eye(nc)))        # LU \ I, column-major
            _check(lib, lib.mg_set_coarse_dense_inverse_FP64(self.handle, nc, _f64(Ainv)), "mg_set_coarse_dense_inverse")
            return
        lu = param.LU
        L = sp.csr_matrix(lu.L)
        U = sp.csr_matrix(lu.U)
        L.sort_indices()
        U.sort_indices()                                                # lower: diagonal last; upper: diagonal first
        a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        Lp, Lc, Lv = a64(L.indptr) + 1, a64(L.indices) + 1, np.ascontiguousarray(L.data, dtype=np.float64)
        Up, Uc, Uv = a64(U.indptr) + 1, a64(U.indices) + 1, np.ascontiguousarray(U.data, dtype=np.float64)
        p = a64(np.argsort(lu.perm_r)) + 1                              # A[p, q] = L U
        q = a64(np.argsort(lu.perm_c)) + 1
        _check(lib, lib.mg_set_coarse_lu_FP64_INT64(self.handle, nc, _i64(Lp), _i64(Lc), _f64(Lv), _i64(Up), _i64(Uc),
                                                    _f64(Uv), _i64(p), _i64(q)), "mg_set_coarse_lu")

    _coarse_dd = None        # the DomainDecompositionParam whose device handle this hierarchy borrows as its coarsest solve
    _coarse_device_inverse = False     # the installed dense inverse was built on the device (a param with coarseDeviceInverse=True)
    _inverse_sfx = "FP64"

    def _build_coarse_inverse(self, param) -> bool:
        """A param with ``coarseDeviceInverse=True`` whose coarsest solve is a dense inverse: set the handle's option
        coarse_device_inverse (mg_rap_* then rebuild the inverse in HBM) and build inv(As[end]) from the resident operator
        (mg_build_coarse_dense_inverse_*).  False - and the option cleared - where the param did not ask or the library does not
        serve the operator (MG_ERR_UNSUPPORTED: more than coarse_device_inverse_max rows, 64-bit row pointers): the caller takes
        the host route.  ``_coarse_device_inverse`` records which route ran."""
        lib = self.lib
        self._coarse_device_inverse = False
        if not getattr(param, "coarseDeviceInverse", False):
            return False
        _check(lib, lib.mg_set_option(self.handle, b"coarse_device_inverse", 1.0), "mg_set_option(coarse_device_inverse)")
        what = f"mg_build_coarse_dense_inverse_{self._inverse_sfx}"
        rc = getattr(lib, what)(self.handle)
        if rc == MG_ERR_UNSUPPORTED:
            _check(lib, lib.mg_set_option(self.handle, b"coarse_device_inverse", 0.0), "mg_set_option(coarse_device_inverse)")
            return False
        _check(lib, rc, what)
        self._coarse_device_inverse = True
        return True

    def coarse_dense_inverse(self) -> np.ndarray:
        """The installed explicit inverse of the coarsest operator (mg_get_coarse_dense_inverse_*), n_c x n_c, whichever route
        installed it; MGDeviceError when the coarsest solve is not a dense inverse."""
        cx = self._inverse_sfx == "CF64"
        nc = int(self.coarse_form()["order"])
        out = np.zeros((nc, nc), dtype=np.complex128 if cx else np.float64, order="F")
        what = f"mg_get_coarse_dense_inverse_{self._inverse_sfx}"
        _check(self.lib, getattr(self.lib, what)(self.handle, nc, out.ctypes.data_as(_dp)), what)
        return out

    def _set_coarse_solver(self, param) -> bool:
        """param.LU a solver object (MGsetup.jl:323-331, MGcycle.jl:138-148): a DomainDecompositionParam is attached as one
        Schwarz sweep (mg_set_coarse_dd), a parallelJuliaSolver hands over its sparse factors (never an explicit inverse).
        False: param.LU is a plain factorisation."""
        from . import domain_decomposition as DD
        from . import parallel_julia_solver as PJS
        LU, lib = param.LU, self.lib
        if isinstance(LU, DD.DomainDecompositionParam):
            if self.nrhs != 1:
                raise NotImplementedError("a DomainDecompositionParam as coarsest solver serves one right-hand side "
                                          "(the reference's sweep indexes b[Idxs])")
            if np.dtype(param.VAL) == np.complex64 and np.dtype(LU.VAL) != np.complex64:
                raise NotImplementedError("a Schwarz coarsest solve is not served for ComplexF32 hierarchies "
                                          "(a DomainDecompositionParam of ComplexF32, singleValues=True, is)")
            if np.dtype(LU.VAL) != np.dtype(param.VAL):
                raise TypeError("param.LU holds %s values, the hierarchy %s" % (np.dtype(LU.VAL), np.dtype(param.VAL)))
            h = DD._device_handle(LU, param.As[-1])
            self._detach_dd()
            _check(lib, lib.mg_set_coarse_dd(self.handle, h), "mg_set_coarse_dd")
            self._coarse_dd = LU
            LU._borrowers.append(self)
            return True
        if isinstance(LU, PJS.parallelJuliaSolver):
            if LU.L is None:
                raise MGDeviceError("param.LU is a parallelJuliaSolver without factors: run MGsetup / SA_AMGsetup first")
            from .mgdef import factor_vals
            if np.dtype(LU.VAL) not in factor_vals(param):
                raise TypeError("param.LU holds %s factors, the hierarchy %s values" % (np.dtype(LU.VAL), np.dtype(param.VAL)))
            # (a ComplexF32 hierarchy keeps ComplexF64 factors, or applies the ComplexF32 ones of a single solver object to its own bc)
            VAL = np.dtype(LU.VAL)
            a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
            L, U = LU.L, LU.U
            Lp, Lc, Lv = a64(L.indptr) + 1, a64(L.indices) + 1, np.ascontiguousarray(L.data, dtype=VAL)
            Up, Uc, Uv = a64(U.indptr) + 1, a64(U.indices) + 1, np.ascontiguousarray(U.data, dtype=VAL)
            fn, what, val = {np.dtype(np.complex64): (lib.mg_set_coarse_lu_CF32_INT64, "mg_set_coarse_lu_CF32", _f32),
                             np.dtype(np.complex128): (lib.mg_set_coarse_lu_CF64_INT64, "mg_set_coarse_lu_CF64", _f64),
                             np.dtype(np.float64): (lib.mg_set_coarse_lu_FP64_INT64, "mg_set_coarse_lu", _f64)}[VAL]
            self._detach_dd()
            _check(lib, fn(self.handle, L.shape[0], _i64(Lp), _i64(Lc), val(Lv), _i64(Up), _i64(Uc), val(Uv), _i64(a64(LU.p)), _i64(a64(LU.q))), what)
            return True
        self._detach_dd()
        return False

    def _detach_dd(self):
        """Give a borrowed Schwarz handle back (before it is destroyed, or before another coarsest solve is set)."""
        p = self._coarse_dd
        if p is not None:
            self._coarse_dd = None
            if self in p._borrowers:
                p._borrowers.remove(self)
            if self.handle:
                self.lib.mg_set_coarse_dd(self.handle, None)

    def coarse_form(self) -> dict:
        """What ``mg_coarse_form`` reports: kind (0 dense inverse, 1 sparse LU in one workgroup, 2 sparse LU chip-wide, 3 GMRES,
        4 Schwarz sweep), order, kernel launches per solve."""
        info = (C.c_longlong * 3)()
        _check(self.lib, self.lib.mg_coarse_form(self.handle, info), "mg_coarse_form")
        return dict(kind=int(info[0]), order=int(info[1]), launches=int(info[2]))

    def set_nrhs(self, nrhs: int):
        if getattr(self, "_vanka", False) and int(nrhs) != 1:
            raise NotImplementedError("Vanka hierarchies serve one right-hand side (blocks of right-hand sides are out of scope)")
        if self._coarse_dd is not None and int(nrhs) != 1:
            raise NotImplementedError("a DomainDecompositionParam as coarsest solver serves one right-hand side "
                                      "(the reference's sweep indexes b[Idxs])")
        _check(self.lib, self.lib.mg_set_nrhs(self.handle, int(nrhs)), "mg_set_nrhs")
        self.nrhs = int(nrhs)

    def replace_values(self, level: int, which: int, M):
        nz = np.ascontiguousarray(M.data, dtype=np.float64)
        _check(self.lib, self.lib.mg_replace_values_FP64(self.handle, level, which, _f64(nz), nz.size),
               "mg_replace_values")

    def replace_matrix(self, param, A_new) -> None:
        """replaceMatrixInHierarchy on the device: numeric Galerkin products + relaxPrecs on the fixed patterns
        (mg_rap_FP64), host copies of the hierarchy refreshed from HBM, coarsest level re-factored on the host (a param with
        ``coarseDeviceInverse=True``: its explicit inverse is rebuilt in HBM by mg_rap_FP64; the host keeps its splu)."""
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        lib = self.lib
        nz = np.ascontiguousarray(A_new.data, dtype=np.float64)
        rp = param.relaxParam
        omega = np.ascontiguousarray([float(rp[l]) if isinstance(rp, (list, tuple, np.ndarray)) else float(rp)
                                      for l in range(self.nlevels)], dtype=np.float64)
        kind = 1 if param.relaxType == "SPAI" else 0
        done = C.c_longlong(0)
        _check(lib, lib.mg_rap_FP64(self.handle, _f64(nz), nz.size, kind, _f64(omega), C.byref(done)), "mg_rap")
        param.As[0] = A_new
        for l in range(2, self.nlevels + 1):                       # refresh the host copies (same patterns)
            M = param.As[l - 1]
            vals = np.empty(M.nnz, dtype=np.float64)
            _check(lib, lib.mg_get_values_FP64(self.handle, l, MG_OP_A, _f64(vals), vals.size), "mg_get_values")
            M.data[:] = vals
        for l in range(1, self.nlevels):
            d = np.empty(param.As[l - 1].shape[0], dtype=np.float64)
            _check(lib, lib.mg_get_relax_FP64(self.handle, l, _f64(d), d.size), "mg_get_relax")
            param.relaxPrecs[l - 1] = d
        from .mgsetup import defineCoarsestAinv
        defineCoarsestAinv(param, param.As[-1])                      # (MGsetup.jl:323-355; param.LU stays the host's factorisation)
        if not self._coarse_device_inverse:
            self._set_coarse(param)
            _check(lib, lib.mg_finalize(self.handle), "mg_finalize")
        # (coarseDeviceInverse: mg_rap_FP64 has rebuilt the inverse in HBM behind its last Galerkin product - nothing uploaded)

    def close(self):
        if self.handle:
            self._detach_dd()
            self.lib.mg_destroy(self.handle)
            self.handle = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-buffer hot path ------------------------------------------------------------------
    @staticmethod
    def _host_block(a, writable=False):
        if not isinstance(a, np.ndarray) or a.dtype != np.float64:
            raise TypeError("expected a float64 numpy array")
        if a.ndim == 2 and a.shape[1] > 1 and not a.flags.f_contiguous:
            raise ValueError("2-D blocks must be column-major (Julia layout): use np.asfortranarray")
        if a.ndim == 1 and not a.flags.c_contiguous:
            raise ValueError("vectors must be contiguous")
        if writable and not a.flags.writeable:
            raise ValueError("x must be writable (it is updated in place)")
        return a

    def cycle(self, b, x, x_is_zero: int = -1):
        b = self._host_block(b)
        x = self._host_block(x, True)
        nrhs = 1 if b.ndim == 1 else b.shape[1]
        _check(self.lib, self.lib.mg_cycle_FP64(self.handle, _f64(b), _f64(x), b.shape[0], nrhs, int(x_is_zero)),
               "mg_cycle")
        return x

    def solve(self, b, x, tol: float, maxIter: int):
        b = self._host_block(b)
        x = self._host_block(x, True)
        nrhs = 1 if b.ndim == 1 else b.shape[1]
        iters = C.c_longlong(0)
        resvec = np.zeros(int(maxIter) + 1)
        _check(self.lib, self.lib.mg_solve_FP64(self.handle, _f64(b), _f64(x), b.shape[0], nrhs, float(tol),
                                                int(maxIter), C.byref(iters), _f64(resvec)), "mg_solve")
        return x, int(iters.value), resvec[: iters.value + 1]

    def _krylov(self, name, res, b, x, *args, nres=True):
        """Call mg_<name>_FP64(handle, b, x, *args, &iters, &flag, res[, &nres]); returns (flag, iters, res cut to nres, or to
        iters for the drivers without nres)."""
        iters, flag, count = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        tail = (C.byref(count),) if nres else ()
        fn = getattr(self.lib, f"mg_{name}_FP64")
        _check(self.lib, fn(self.handle, b, x, *args, C.byref(iters), C.byref(flag), _f64(res), *tail), f"mg_{name}")
        return int(flag.value), int(iters.value), res[: (count if nres else iters).value]

    def pcg(self, b, x, tol: float, maxIter: int):
        """KrylovMethods.cg / blockCG with the MG cycle as preconditioner; returns (x, flag, iters, resvec)
        (resvec: ||r||/||b|| per iteration; for a block the maximum over the columns)."""
        b = self._host_block(b)
        x = self._host_block(x, True)
        if b.ndim != 1 and b.shape[1] > 1:
            flag, iters, self.last_resmat = self._krylov("block_pcg", np.zeros((max(int(maxIter), 1), b.shape[1])), _f64(b), _f64(x),
                                                         b.shape[0], b.shape[1], float(tol), int(maxIter), nres=False)
            return x, flag, iters, self.last_resmat.max(axis=1) if iters else np.zeros(0)
        if b.ndim != 1:
            b, x = b[:, 0], x[:, 0]
        return (x,) + self._krylov("pcg", np.zeros(max(int(maxIter), 1)), _f64(b), _f64(x), b.shape[0], float(tol), int(maxIter),
                                   nres=False)

    def bicgstab(self, b, x, tol: float, maxIter: int):
        """KrylovMethods.bicgstb with the MG cycle as M1; returns (x, flag, iters, resvec)."""
        b = self._host_block(b)
        x = self._host_block(x, True)
        resvec = np.zeros(2 * int(maxIter) + 1)
        if b.ndim != 1 and b.shape[1] > 1:
            return (x,) + self._krylov("block_bicgstab", resvec, _f64(b), _f64(x), b.shape[0], b.shape[1], float(tol), int(maxIter))
        if b.ndim != 1:
            b, x = b[:, 0], x[:, 0]
        return (x,) + self._krylov("bicgstab", resvec, _f64(b), _f64(x), b.shape[0], float(tol), int(maxIter))

    def fgmres(self, b, x, inner: int, tol: float, maxIter: int):
        """KrylovMethods.fgmres (flexible) with the MG cycle as preconditioner; returns (x, flag, iters, resvec)."""
        b = self._host_block(b)
        x = self._host_block(x, True)
        resvec = np.zeros(max(1, int(inner) * int(maxIter)))
        if b.ndim != 1 and b.shape[1] > 1:
            return (x,) + self._krylov("block_fgmres", resvec, _f64(b), _f64(x), b.shape[0], b.shape[1], int(inner), float(tol),
                                       int(maxIter))
        if b.ndim != 1:
            b, x = b[:, 0], x[:, 0]
        return (x,) + self._krylov("fgmres", resvec, _f64(b), _f64(x), b.shape[0], int(inner), float(tol), int(maxIter))

    def cycle_mixed_f32(self, b32, z32):
        """getMultigridPreconditioner's mixed-precision branch (SolveFuncs.jl:52-58): Float32 block, Float64 hierarchy."""
        if b32.dtype != np.float32 or z32.dtype != np.float32:
            raise TypeError("expected float32 arrays")
        nrhs = 1 if b32.ndim == 1 else b32.shape[1]
        if b32.ndim == 2 and nrhs > 1 and not (b32.flags.f_contiguous and z32.flags.f_contiguous):
            raise ValueError("2-D blocks must be column-major (Julia layout)")
        fp = C.POINTER(C.c_float)
        _check(self.lib, self.lib.mg_cycle_mixed_FP32(self.handle, b32.ctypes.data_as(fp), z32.ctypes.data_as(fp), b32.shape[0], nrhs),
               "mg_cycle_mixed_FP32")
        return z32

    def pcg_dev(self, b, x, tol: float, maxIter: int):
        _sync_torch(b, x)
        return self._krylov("pcg_dev", np.zeros(max(int(maxIter), 1)), _ptr(b), _ptr(x), self.n, float(tol), int(maxIter),
                            nres=False)

    # -- block Krylov drivers on device tensors (row-major [n][nrhs]); KrylovMethods.blockCG / blockBiCGSTB / blockFGMRES ----------
    def block_pcg_dev(self, b, x, tol: float, maxIter: int):
        """returns (flag, iterations, resmat[iterations][nrhs] of ||r_j|| / ||b_j||)"""
        _sync_torch(b, x)
        return self._krylov("block_pcg_dev", np.zeros((max(int(maxIter), 1), self.nrhs)), _ptr(b), _ptr(x), self.n, self.nrhs,
                            float(tol), int(maxIter), nres=False)

    def block_bicgstab_dev(self, b, x, tol: float, maxIter: int):
        _sync_torch(b, x)
        return self._krylov("block_bicgstab_dev", np.zeros(2 * max(int(maxIter), 1) + 1), _ptr(b), _ptr(x), self.n, self.nrhs,
                            float(tol), int(maxIter))

    def block_fgmres_dev(self, b, x, inner: int, tol: float, maxIter: int):
        _sync_torch(b, x)
        return self._krylov("block_fgmres_dev", np.zeros(max(int(inner) * int(maxIter), 1)), _ptr(b), _ptr(x), self.n, self.nrhs,
                            int(inner), float(tol), int(maxIter))

    def bicgstab_dev(self, b, x, tol: float, maxIter: int):
        """solveBiCGSTAB_MG on device tensors (one right-hand side); returns (flag, iterations, resvec: the entry at the start, then
        two per iteration)."""
        _sync_torch(b, x)
        return self._krylov("bicgstab_dev", np.zeros(2 * max(int(maxIter), 1) + 1), _ptr(b), _ptr(x), self.n, float(tol),
                            int(maxIter))

    def fgmres_dev(self, b, x, inner: int, tol: float, maxIter: int):
        """solveGMRES_MG on device tensors (one right-hand side); returns (flag, inner steps, resvec)."""
        _sync_torch(b, x)
        return self._krylov("fgmres_dev", np.zeros(max(int(inner) * int(maxIter), 1)), _ptr(b), _ptr(x), self.n, int(inner),
                            float(tol), int(maxIter))

    # -- the real drivers' passes on their own (mg_kry_*_dev_FP64): float64 device tensors of the caller's length n; the ones that
    #    return a host value have drained the library's stream, the others only enqueue on it (``sync()`` before reading) -----------
    def _kry(self, name, *args):
        _check(self.lib, getattr(self.lib, f"mg_kry_{name}_dev_FP64")(self.handle, *args), f"mg_kry_{name}_dev")

    def kry_dot(self, x, y, n: int) -> float:
        _sync_torch(x, y)
        out = C.c_double(0.0)
        self._kry("dot", _ptr(x), _ptr(y), int(n), C.byref(out))
        return out.value

    def kry_norm(self, x, n: int) -> float:
        _sync_torch(x)
        out = C.c_double(0.0)
        self._kry("norm", _ptr(x), int(n), C.byref(out))
        return out.value

    def kry_axpby(self, a: float, x, b: float, y, n: int):
        """y = a x + b y (b == 0: y is not read)."""
        _sync_torch(x, y)
        self._kry("axpby", float(a), _ptr(x), float(b), _ptr(y), int(n))

    def kry_cg_update(self, alpha: float, p, Ap, x, r, n: int, norm: bool = False):
        """x += alpha p ; r -= alpha Ap ; with ``norm`` returns ||r|| of the new r from the same pass."""
        _sync_torch(p, Ap, x, r)
        out = C.c_double(0.0)
        self._kry("cg_update", float(alpha), _ptr(p), _ptr(Ap), _ptr(x), _ptr(r), int(n), C.byref(out) if norm else None)
        return out.value if norm else None

    def kry_cg_p(self, beta: float, z, p, n: int):
        """p = z + beta p."""
        _sync_torch(z, p)
        self._kry("cg_p", float(beta), _ptr(z), _ptr(p), int(n))

    def kry_mgs_step(self, hk, v, w, u, n: int, out):
        """w -= hk[0] v ; out[0] = w'u of the new w (u None: w'w); hk and out are device scalars."""
        _sync_torch(hk, v, w, u, out)
        self._kry("mgs_step", _ptr(hk), _ptr(v), _ptr(w), _ptr(u) if u is not None else None, int(n), _ptr(out))

    def kry_mgs_chain(self, V, n: int, i: int):
        """V: i + 2 vectors n apart, the last one orthogonalised against the others and normalised; returns (h_0 .. h_i, ||w||^2)."""
        _sync_torch(V)
        hh = np.zeros(int(i) + 2)
        self._kry("mgs_chain", _ptr(V), int(n), int(i), _f64(hh))
        return hh

    def kry_blk_gram(self, X, Y, n: int, k: int):
        """X'Y (k x k) of two row-major [n][k] device blocks."""
        _sync_torch(X, Y)
        G = np.zeros((int(k), int(k)))
        self._kry("blk_gram", _ptr(X), _ptr(Y), int(n), int(k), _f64(G))
        return G

    def kry_blk_comb(self, out, add, s: float, inp, Cm, n: int, k: int):
        """out = s add + inp Cm (row-major [n][k] device blocks, Cm a k x k numpy array); add may be None, out may be inp or add."""
        _sync_torch(out, add, inp)
        Cc = np.ascontiguousarray(Cm, dtype=np.float64)
        if Cc.shape != (int(k), int(k)):
            raise ValueError("Cm must be k x k")
        self._kry("blk_comb", _ptr(out), _ptr(add) if add is not None else None, float(s), _ptr(inp), _f64(Cc), int(n), int(k))

    def spmv(self, level: int, which: int, alpha: float, x, beta: float, y):
        x = self._host_block(x)
        y = self._host_block(y, True)
        nrhs = 1 if x.ndim == 1 else x.shape[1]
        _check(self.lib, self.lib.mg_spmv_FP64(self.handle, level, which, float(alpha), _f64(x), float(beta),
                                               _f64(y), nrhs), "mg_spmv")
        return y

    # -- device-resident hot path (torch CUDA tensors, row-major [n][nrhs]) ---------------------
    def cycle_dev(self, b, x, x_is_zero: int = -1, nrhs: Optional[int] = None):
        _sync_torch(b, x)
        nrhs = self.nrhs if nrhs is None else nrhs
        _check(self.lib, self.lib.mg_cycle_dev_FP64(self.handle, _ptr(b), _ptr(x), self.n, nrhs, int(x_is_zero)),
               "mg_cycle_dev")

    def solve_dev(self, b, x, tol: float, maxIter: int, nrhs: Optional[int] = None):
        _sync_torch(b, x)
        nrhs = self.nrhs if nrhs is None else nrhs
        iters = C.c_longlong(0)
        resvec = np.zeros(int(maxIter) + 1)
        _check(self.lib, self.lib.mg_solve_dev_FP64(self.handle, _ptr(b), _ptr(x), self.n, nrhs, float(tol),
                                                    int(maxIter), C.byref(iters), _f64(resvec)), "mg_solve_dev")
        return int(iters.value), resvec[: iters.value + 1]

    def spmv_dev(self, level, which, alpha, x, beta, y, nrhs: Optional[int] = None):
        _sync_torch(x, y)
        nrhs = self.nrhs if nrhs is None else nrhs
        _check(self.lib, self.lib.mg_spmv_dev_FP64(self.handle, level, which, float(alpha), _ptr(x), float(beta),
                                                   _ptr(y), nrhs), "mg_spmv_dev")

    def fused_dev(self, level, kernel, b, x, out, nrhs: Optional[int] = None):
        _sync_torch(b, x, out)
        nrhs = self.nrhs if nrhs is None else nrhs
        _check(self.lib, self.lib.mg_fused_dev_FP64(self.handle, level, kernel, _ptr(b), _ptr(x), _ptr(out), nrhs),
               "mg_fused_dev")

    def sweep_residual_dev(self, level, b, x, t, r=None, xn=None, want_norm=False):
        """t = x + d.*(b - A x), r = b - A t [, xn = t + d.*r, ||r||] in one pass (two-stage marching kernel)."""
        _sync_torch(b, x, t, r, xn)
        ss = C.c_double(0.0)
        _check(self.lib, self.lib.mg_sweep_residual_dev_FP64(
            self.handle, level, _ptr(b), _ptr(x), _ptr(t), _ptr(r) if r is not None else None,
            _ptr(xn) if xn is not None else None, C.byref(ss) if want_norm else None), "mg_sweep_residual_dev")
        return float(ss.value)

    def four_stage_dev(self, level, b, x, tp, rp, want_norm=True):
        """The solve loop's two fine-level passes across the stopping test as one pass: t = x + d.*(b - A x), r = b - A t (||r||
        returned), xn = t + d.*r, tp = xn + d.*(b - A xn), rp = b - A tp (csr_rowclass_march4_spmv)."""
        _sync_torch(b, x, tp, rp)
        ss = C.c_double(0.0)
        _check(self.lib, self.lib.mg_four_stage_dev_FP64(self.handle, level, _ptr(b), _ptr(x), _ptr(tp), _ptr(rp),
                                                         C.byref(ss) if want_norm else None), "mg_four_stage_dev")
        return float(ss.value)

    def get_values(self, level: int, which: int) -> np.ndarray:
        """nzval of operator `which` of `level` as the device holds it (stored CSR order)."""
        nnz = C.c_longlong(0)
        info = (C.c_longlong * 3)()
        _check(self.lib, self.lib.mg_operator_shape(self.handle, level, which, info), "mg_operator_shape")
        vals = np.zeros(int(info[2]), dtype=np.float64)
        _check(self.lib, self.lib.mg_get_values_FP64(self.handle, level, which, _f64(vals), vals.size), "mg_get_values")
        return vals

    def transpose_hierarchy(self):
        """transposeHierarchy (MGsetup.jl:274-318) on the resident hierarchy; raises MGDeviceError (status MG_ERR_UNSUPPORTED)
        when the library cannot (sparse coarsest factors): the caller then re-uploads."""
        _check(self.lib, self.lib.mg_transpose_hierarchy(self.handle), "mg_transpose_hierarchy")

    def four_stage_form(self, level: int):
        """(available, geometry as sweep_residual_form's)."""
        f = C.c_longlong(0)
        g = (C.c_longlong * 12)()
        _check(self.lib, self.lib.mg_four_stage_form(self.handle, level, C.byref(f), g), "mg_four_stage_form")
        return bool(f.value), [int(v) for v in g]

    def set_stream(self, stream: int):
        """Enqueue on the caller's HIP stream (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        _check(self.lib, self.lib.mg_set_stream(self.handle, _vp(stream)), "mg_set_stream")

    def cycle_async_dev(self, b, x, x_is_zero: int, nrhs: Optional[int] = None):
        nrhs = self.nrhs if nrhs is None else nrhs
        _check(self.lib, self.lib.mg_cycle_async_dev_FP64(self.handle, _ptr(b), _ptr(x), self.n, nrhs, int(x_is_zero)),
               "mg_cycle_async_dev")

    # -- measurement --------------------------------------------------------------------------------
    def time_op(self, level: int, kernel: int, reps: int = 20):
        ms = C.c_double(0.0)
        bts = C.c_double(0.0)
        _check(self.lib, self.lib.mg_time_op_dev_FP64(self.handle, level, kernel, self.nrhs, int(reps),
                                                      C.byref(ms), C.byref(bts)), "mg_time_op_dev")
        return ms.value, bts.value

    def profile_enable(self, on: bool):
        _check(self.lib, self.lib.mg_profile_enable(self.handle, 1 if on else 0), "mg_profile_enable")

    def profile_reset(self):
        _check(self.lib, self.lib.mg_profile_reset(self.handle), "mg_profile_reset")

    def profile(self):
        """{(level, kernel_name): (total_ms, launches, bytes_per_launch)} for every kernel that ran."""
        out = {}
        for l in range(1, self.nlevels + 1):
            for k in range(MG_K_COUNT):
                ms, n, bts = C.c_double(0), C.c_longlong(0), C.c_double(0)
                _check(self.lib, self.lib.mg_profile_get(self.handle, l, k, C.byref(ms), C.byref(n), C.byref(bts)),
                       "mg_profile_get")
                if n.value:
                    out[(l, KERNEL_NAMES[k])] = (ms.value, int(n.value), bts.value)
        return out

    def profile_moved(self):
        """{(level, kernel_name): bytes one launch of the kernel in use has to move} (device format + each vector once)."""
        out = {}
        for (l, name) in self.profile():
            mv = C.c_double(0)
            _check(self.lib, self.lib.mg_profile_get_moved(self.handle, l, KERNEL_NAMES.index(name), C.byref(mv)),
                   "mg_profile_get_moved")
            out[(l, name)] = mv.value
        return out

    def operator_format(self, level: int, which: int):
        """(number of row patterns [0 = plain CSR], dictionary entries, index-side bytes per nrhs=1 launch)."""
        npat, nd, ib = C.c_longlong(0), C.c_longlong(0), C.c_double(0)
        _check(self.lib, self.lib.mg_operator_format(self.handle, level, which, C.byref(npat), C.byref(nd), C.byref(ib)),
               "mg_operator_format")
        return int(npat.value), int(nd.value), ib.value

    def operator_rowclasses(self, level: int, which: int):
        """(number of row classes [0 = not stored that way], dictionary entries, matrix-side bytes one nrhs=1 launch of
        the kernel in use streams)."""
        nc, nd, mb = C.c_longlong(0), C.c_longlong(0), C.c_double(0)
        _check(self.lib, self.lib.mg_operator_rowclasses(self.handle, level, which, C.byref(nc), C.byref(nd), C.byref(mb)),
               "mg_operator_rowclasses")
        return int(nc.value), int(nd.value), mb.value

    def operator_rowclass_flags(self, level: int, which: int):
        """(implicit first column, relaxPrec read from the class dictionary) of a row-class operator."""
        a, b, c, e = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _check(self.lib, self.lib.mg_operator_rowclass_flags(self.handle, level, which, C.byref(a), C.byref(b), C.byref(c),
                                                             C.byref(e)), "mg_operator_rowclass_flags")
        return bool(a.value), bool(b.value)

    def sweep_residual_form(self, level: int):
        """(form, geometry): 0 two launches, 2 csr_rowclass_march2_spmv, 5 csr_rowclass_march27_spmv (27-point levels; geometry of
        the pair, [7] = workgroups of its single-product geometry), 3 (4: band form) csr_rowclass_march3_spmv with its tile geometry
        [tiles per line, tiles per column, TX, TY, rows per lane, workgroups, LDS bytes, est. fill bytes per row x 100,
        threads per workgroup, lockstep segments (0: balanced ranges), planes per segment, class-table entries]."""
        f = C.c_longlong(0)
        g = (C.c_longlong * 12)()
        _check(self.lib, self.lib.mg_sweep_residual_form(self.handle, level, C.byref(f), g), "mg_sweep_residual_form")
        return int(f.value), [int(v) for v in g]

    def band_form(self, level: int):
        """[held, canonical slots, symmetric reads, value planes streamed per pass] of the level's band form (mg_band_form)."""
        g = (C.c_longlong * 4)()
        _check(self.lib, self.lib.mg_band_form(self.handle, level, g), "mg_band_form")
        return [int(v) for v in g]

    def operator_stream_kernel(self, level: int, which: int):
        """[kernel, NT / rows per lane, 16-bit column offsets, longest row] (mg_operator_stream_kernel): 0 a row-class or grid kernel,
        1 csr_pattern_spmv, 2 csr_stream_spmv, 3 csr_longrow_spmv, 4 csr_stream_spmm, 5 csr_rowclass_lane_spmm, 6 csr_rowclass_lane_spmm2."""
        g = (C.c_longlong * 4)()
        _check(self.lib, self.lib.mg_operator_stream_kernel(self.handle, level, which, g), "mg_operator_stream_kernel")
        return [int(v) for v in g]

    def operator_kernel_variant(self, level: int, which: int) -> int:
        """-1 streaming formats, 0 csr_rowclass_spmv, 1 csr_rowclass_window_spmv, 2 csr_rowclass_tile_spmv, 3 csr_rowclass_march_spmv,
        4 csr_rowclass_lane_spmv, 7 csr_rowclass_marchr_spmv (marching restriction), 8 the small-grid-level kernels (mg_small.hpp)."""
        return self.operator_kernel_info(level, which)[0]

    def operator_kernel_info(self, level: int, which: int):
        """(kernel variant as above, number of exception rows)."""
        a, b, c, e = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _check(self.lib, self.lib.mg_operator_rowclass_flags(self.handle, level, which, C.byref(a), C.byref(b), C.byref(c),
                                                             C.byref(e)), "mg_operator_rowclass_flags")
        return int(c.value), int(e.value)

    def graph_launches(self):
        """(replays so far, graphs cached) of the HIP graphs the launch-bound coarse sub-cycles run as."""
        a, b = C.c_longlong(0), C.c_longlong(0)
        _check(self.lib, self.lib.mg_graph_launches(self.handle, C.byref(a), C.byref(b)), "mg_graph_launches")
        return int(a.value), int(b.value)

    def cycle_bytes(self) -> float:
        v = C.c_double(0)
        _check(self.lib, self.lib.mg_cycle_bytes(self.handle, C.byref(v)), "mg_cycle_bytes")
        return v.value

    def device_bytes(self) -> float:
        v = C.c_double(0)
        _check(self.lib, self.lib.mg_device_bytes(self.handle, C.byref(v)), "mg_device_bytes")
        return v.value


def _c128(a):
    return a.ctypes.data_as(_dp)


class ComplexDeviceHierarchy(DeviceHierarchy):
    """A ComplexF64 hierarchy on the device (mg_create_CF64): generic CSR, V / W / F / K cycles, Jac / SPAI / Jac-GMRES relaxation
    or (a param with ``complexVanka=True``) the Vanka cell-block smoothers (blocks only for a param with ``vankaBlocks=True``),
    dense-inverse, sparse-LU or GMRES coarsest solve (the last adds one host synchronisation per coarsest solve and serves blocks only for a param with ``blockCoarseGMRES=True``: ``block_coarse_gmres``).  The handle serves one right-hand side; blocks of up to 16 go through the ``block_*``
    methods, which take the column count with each call (on a K-cycle / Jac-GMRES hierarchy only for a param with ``blockKcycle=True``: the block is then one long vector, its columns coupled).  ``param.As[l]`` is the applied operator A (= the reference's AT^H): it is
    uploaded as the reference's AT arrays, colptr = indptr+1, rowval = indices+1, nzval = conj(A.data), which the library
    conjugates back.  P and R are real."""

    _cdtype = np.complex128       # what As, relaxPrecs and the vectors of cycle / solve / spmv hold
    _rdtype = np.float64          # what Ps / Rs hold
    _sfx = "CF64"                 # the entry points of create / set_operator / set_relax / cycle / solve / spmv

    def _fn(self, stem):
        return getattr(self.lib, f"mg_{stem}_{self._sfx}")

    def __init__(self, param, device_id: int = 0, nrhs: Optional[int] = None, options: Optional[dict] = None):
        self.lib = load_library()
        self.handle = _vp()
        self.nlevels = len(param.As)
        self.n = int(param.As[0].shape[0])
        self.nrhs = int(nrhs if nrhs is not None else max(1, param.nrhs))
        if self.nrhs != 1:
            raise NotImplementedError("ComplexF64 hierarchies serve one right-hand side on the device")
        self._op_nnz = {}
        lib = self.lib
        _check(lib, self._fn("create")(self.nlevels, 1, int(device_id), C.byref(self.handle)), f"mg_create_{self._sfx}")
        try:
            for key, val in (options or {}).items():
                _check(lib, lib.mg_set_option(self.handle, key.encode(), float(val)), f"mg_set_option({key})")
            self._upload(param)
        except Exception:
            self.close()
            raise

    def _set_op(self, level, which, M):
        self._op_nnz[(int(level), int(which))] = int(M.nnz)     # (get_values sizes its array by it; adjoint_hierarchy updates P's)
        if which != MG_OP_A:
            if np.iscomplexobj(M.data):
                raise TypeError("P and R of a ComplexF64 hierarchy are real")
            return super()._set_op(level, which, M)
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
        nzval = np.ascontiguousarray(np.conj(M.data), dtype=np.complex128)     # the reference's AT values
        rc = self.lib.mg_set_operator_CF64_INT64(self.handle, level, which, M.shape[0], M.shape[1], _i64(colptr), _i64(rowval),
                                                 _c128(nzval))
        _check(self.lib, rc, f"mg_set_operator_CF64(level={level})")

    def _set_relax(self, level, d, pre, post):
        d = np.ascontiguousarray(d, dtype=np.complex128)
        _check(self.lib, self.lib.mg_set_relax_CF64(self.handle, level, _c128(d), d.size, int(pre), int(post)),
               f"mg_set_relax_CF64(level={level})")

    def _set_relax_level(self, param, l, pre, post, blocks=True):
        """relaxPrecs[l]: the pointwise vector, or (a complex Vanka hierarchy) the cells' complex64 blocks - then the pointwise
        slot holds zeros, which nothing reads, and carries the sweep counts (blocks=False: new sweep counts only)."""
        if not self._vanka:
            return self._set_relax(l, param.relaxPrecs[l - 1], pre, post)
        if not blocks:
            return self._set_relax(l, np.zeros(param.As[l - 1].shape[0], dtype=self._cdtype), pre, post)
        from .vanka import getVankaRelaxType
        blk = param.relaxPrecs[l - 1]
        if not isinstance(blk, np.ndarray) or blk.dtype != np.complex64 or blk.ndim != 2:
            raise TypeError("relaxPrecs of a complex Vanka hierarchy are the complex64 blocks of setupVankaFacesPreconditioner")
        nn = np.ascontiguousarray(param.Meshes[l - 1].n, dtype=np.int64)
        mixed = param.transferOperatorType == "SystemsFacesMixedLinear"
        self.__dict__.setdefault("_vanka_shape", {})[int(l)] = tuple(blk.shape)     # (vanka_blocks sizes its array by it)
        if getattr(param, "vankaDeviceSetup", False):
            # the level's blocks built in HBM from the operator just uploaded (mg_build_vanka_*): nothing of relaxPrecs[l] is sent
            from .mgsetup import _relax_param_arr
            from .vanka import _w_pair, _check_build
            wv, nw = _w_pair(_relax_param_arr(param)[l - 1])
            _check_build(self.lib, self._fn("build_vanka")(self.handle, l, nn.size, _i64(nn), 1 if mixed else 0,
                                                           getVankaRelaxType(param.relaxType)[1], _f64(wv), nw),
                         f"mg_build_vanka_{self._sfx}(level={l})")
        else:
            blk = np.asfortranarray(blk)
            _check(self.lib, self._fn("set_vanka")(self.handle, l, nn.size, _i64(nn), 1 if mixed else 0,
                                                   getVankaRelaxType(param.relaxType)[1], blk.ctypes.data_as(_fp)),
                   f"mg_set_vanka_{self._sfx}(level={l})")
        self._set_relax(l, np.zeros(param.As[l - 1].shape[0], dtype=self._cdtype), pre, post)

    def vanka_blocks(self, level: int) -> np.ndarray:
        """The Vanka blocks of ``level`` as the handle holds them (mg_get_vanka_blocks_*): (bs^2, cells) complex64, column-major."""
        if int(level) not in getattr(self, "_vanka_shape", {}):
            raise MGDeviceError(f"vanka_blocks: level {level} holds no Vanka blocks")
        out = np.zeros(self._vanka_shape[int(level)], dtype=np.complex64, order="F")
        _check(self.lib, self._fn("get_vanka_blocks")(self.handle, int(level), out.ctypes.data_as(_fp), out.size),
               f"mg_get_vanka_blocks_{self._sfx}(level={level})")
        return out

    def _upload(self, param):
        lib = self.lib
        nl = self.nlevels
        _vanka_guard(param, self.nrhs)
        self._vanka = _relax_type_code(param) == 2
        self._refuse_schedule(param)
        for l in range(1, nl + 1):
            self._set_op(l, MG_OP_A, param.As[l - 1])
            if l < nl:
                self._set_op(l, MG_OP_P, param.Ps[l - 1])
                self._set_op(l, MG_OP_R, param.Rs[l - 1])
                self._set_relax_level(param, l, param.relaxPre(l), param.relaxPost(l))
        self._set_schedule(param)
        if param.LU is None:
            raise MGDeviceError("param.LU is empty: run MGsetup first")
        self._block_coarse_gmres = bool(getattr(param, "blockCoarseGMRES", False))
        if self._block_coarse_gmres:      # blocks on the GMRES coarsest solve: the block form of that solve (opt-in, read at every call)
            _check(lib, lib.mg_set_option(self.handle, b"coarse_gmres_blocks", 1.0), "mg_set_option(coarse_gmres_blocks)")
        self._vanka_blocks = self._vanka and bool(getattr(param, "vankaBlocks", False))
        if self._vanka_blocks:            # blocks on a Vanka hierarchy: the block form of the smoother (opt-in, read at every call)
            _check(lib, lib.mg_set_option(self.handle, b"vanka_blocks", 1.0), "mg_set_option(vanka_blocks)")
        self._kcycle_blocks = bool(getattr(param, "blockKcycle", False))
        if self._kcycle_blocks:           # blocks on a K-cycle / Jac-GMRES hierarchy: the long-vector form (opt-in, ahead of mg_finalize)
            _check(lib, lib.mg_set_option(self.handle, b"kcycle_blocks", 1.0), "mg_set_option(kcycle_blocks)")
        self._vanka_device_setup = self._vanka and bool(getattr(param, "vankaDeviceSetup", False))
        if self._vanka_device_setup:      # mg_rap_CF64 serves the Vanka handle: operators and blocks refreshed in HBM (opt-in, read at every call)
            _check(lib, lib.mg_set_option(self.handle, b"vanka_device_setup", 1.0), "mg_set_option(vanka_device_setup)")
        self._set_coarse(param)
        _check(lib, lib.mg_finalize(self.handle), "mg_finalize")
        self._schedule = self._schedule_of(param)

    def _refuse_schedule(self, param):
        """The K-cycle and Jac-GMRES smoothing are served for ComplexF64 values, and for ComplexF32 ones where the param uploaded
        carried ``singleKcycle=True`` (the handle's option single_kcycle)."""
        if self._sfx != "CF64" and not getattr(self, "_single_kcycle", False) and (param.cycleType == "K" or param.relaxType == "Jac-GMRES"):
            raise NotImplementedError("ComplexF32 hierarchies: cycles V, W, F with the Jac / SPAI smoothers")

    def _set_schedule(self, param):
        lib = self.lib
        if self._vanka:       # relaxation type 2 with its cycle type: a setter of its own (the shared ones refuse type 2 on complex handles)
            _check(lib, self._fn("set_vanka_relax")(self.handle, ord(param.cycleType)), f"mg_set_vanka_relax_{self._sfx}")
        elif self._sfx == "CF64":
            _check(lib, lib.mg_set_schedule_CF64(self.handle, ord(param.cycleType), _relax_type_code(param)), "mg_set_schedule_CF64")
        elif getattr(self, "_single_kcycle", False):
            _check(lib, lib.mg_set_schedule_CF32(self.handle, ord(param.cycleType), _relax_type_code(param)), "mg_set_schedule_CF32")
        else:
            _check(lib, lib.mg_set_relax_type(self.handle, 0), "mg_set_relax_type")
            _check(lib, lib.mg_set_cycle_type(self.handle, ord(param.cycleType)), "mg_set_cycle_type")

    def _block_guard(self):
        """The reference runs its FGMRES relaxation on a block as one long vector (FGMRES.jl:51); that form runs where the param asked
        for it (``blockKcycle=True``: the handle's option kcycle_blocks; never for Vanka with 'K') and is refused otherwise."""
        self._vanka_block_guard()
        sched = getattr(self, "_schedule", None)
        if sched is not None and (sched[0] == "K" or sched[1] == "Jac-GMRES") and (
                not getattr(self, "_kcycle_blocks", False) or getattr(self, "_vanka", False)):
            raise NotImplementedError("blocks of right-hand sides are not served on a K-cycle / Jac-GMRES complex hierarchy "
                                      "(solve the columns one after the other)")

    def _vanka_block_guard(self):
        """Blocks on a complex Vanka hierarchy run where the param asked for them (``vankaBlocks=True``: the handle's option
        vanka_blocks) and are refused otherwise."""
        if getattr(self, "_vanka", False) and not getattr(self, "_vanka_blocks", False):
            raise NotImplementedError("blocks of right-hand sides are not served on a complex Vanka hierarchy (out of scope)")

    def _block_coarse_guard(self, k: int):
        """The reference calls blockFGMRES for a block on the GMRES coarsest solve (MGcycle.jl:166-167); that form runs where the
        param asked for it (``blockCoarseGMRES=True``: the handle's option coarse_gmres_blocks) and is refused otherwise."""
        if getattr(self, "_coarse_gmres", False) and int(k) > 1 and not getattr(self, "_block_coarse_gmres", False):
            raise NotImplementedError("blocks of right-hand sides are not served on a complex hierarchy with coarseSolveType='GMRES' "
                                      "(solve the columns one after the other)")

    def sync_schedule(self, param):
        sig = self._schedule_of(param)
        if sig == getattr(self, "_schedule", sig):
            self._schedule = sig
            return
        self._refuse_schedule(param)
        _vanka_guard(param, self.nrhs)
        old = self._schedule
        if (_relax_type_code(param) == 2) != self._vanka or (self._vanka and sig[1] != old[1]):
            raise NotImplementedError("relaxType changed to or from a Vanka smoother after the setup: relaxPrecs hold the other "
                                      "smoother's data - run MGsetup again")
        lib = self.lib
        for l in range(1, self.nlevels):
            self._set_relax_level(param, l, sig[2][l - 1], sig[3][l - 1], blocks=False)
        self._set_schedule(param)
        _check(lib, lib.mg_finalize(self.handle), "mg_finalize")
        self._schedule = sig

    def fgmres_relax(self, level: int, r0, x, inner: int, tol: float = 1e-5, want_bases: bool = False):
        """One FGMRES_relaxation (FGMRES.jl:48-126) with the diagonal preconditioner on As[level] and relaxPrecs[level]
        (mg_fgmres_relax_CF64 / _CF32): ``x += Z t`` in place for the residual ``r0``, both in the hierarchy's own precision.  Returns
        (rnorms, H, xi): the residual estimates of the directions used (``len(rnorms)`` is the reference's ``used``), and the summed
        Gram scalars H = (AZ)'(AZ) (inner x inner) and xi = (AZ)'r0 of all ``inner`` directions, formed in double.  On a
        ``singleKcycle`` ComplexF32 hierarchy Z and AZ are complex64 and the product is formed in single; there ``want_bases`` adds
        (Z, AZ), the n x inner complex64 bases of all ``inner`` directions."""
        single = self._sfx == "CF32"
        if want_bases and not single:
            raise TypeError("want_bases is served on ComplexF32 hierarchies (mg_fgmres_relax_CF32 takes the two arrays)")
        r0 = self._host_block(r0, dtype=self._cdtype)
        x = self._host_block(x, True, dtype=self._cdtype)
        k = int(inner)
        H = np.zeros((max(k, 1), max(k, 1)), dtype=np.complex128)
        xi = np.zeros(max(k, 1), dtype=np.complex128)
        rn = np.zeros(max(k, 1))
        used = C.c_longlong(0)
        Z = AZ = None
        if want_bases:
            Z = np.zeros((r0.shape[0], max(k, 1)), dtype=np.complex64, order="F")
            AZ = np.zeros_like(Z)
        bases = (Z.ctypes.data_as(_fp) if want_bases else None, AZ.ctypes.data_as(_fp) if want_bases else None) if single else ()
        _check(self.lib, self._fn("fgmres_relax")(self.handle, int(level), self._vp_of(r0), self._vp_of(x), r0.shape[0], k, float(tol),
                                                  _c128(H), _c128(xi), _f64(rn), C.byref(used), *bases), f"mg_fgmres_relax_{self._sfx}")
        return (rn[: used.value], H, xi) + ((Z, AZ) if want_bases else ())

    def block_fgmres_relax(self, level: int, R0, X, inner: int, tol: float = 1e-5, want_bases: bool = False):
        """One FGMRES_relaxation on the n x k complex128 block ``R0`` taken as ONE long vector of length n*k (FGMRES.jl:51-53;
        mg_block_fgmres_relax_CF64 / _CF32; a param with ``blockKcycle=True``): ``X += sum_j t_j Z_j`` in place, one H, xi, t and break
        test for the whole block - its columns are coupled.  Returns (rnorms, H, xi) as ``fgmres_relax`` does; ``want_bases`` adds
        (Z, AZ), complex128 arrays of shape (n, k, inner) holding all ``inner`` direction blocks (on a ComplexF32 hierarchy the
        device's complex64 values widened, which is exact)."""
        if not getattr(self, "_kcycle_blocks", False):
            raise NotImplementedError("blocks of right-hand sides are not served on a K-cycle / Jac-GMRES complex hierarchy "
                                      "(solve the columns one after the other)")
        Bf, k = self._blk(R0)
        Xf, kx = self._blk(X, True)
        if kx != k or Xf.shape[0] != Bf.shape[0]:
            raise ValueError("R0 and X must hold the same number of rows and columns")
        m = max(int(inner), 1)
        H = np.zeros((m, m), dtype=np.complex128)
        xi = np.zeros(m, dtype=np.complex128)
        rn = np.zeros(m)
        used = C.c_longlong(0)
        Z = AZ = None
        if want_bases:
            Z = np.zeros((Bf.shape[0], k, m), dtype=np.complex128, order="F")
            AZ = np.zeros_like(Z)
        _check(self.lib, self._fn("block_fgmres_relax")(self.handle, int(level), _c128(Bf), _c128(Xf), Bf.shape[0], k, int(inner), float(tol),
                                                        _c128(H), _c128(xi), _f64(rn), C.byref(used),
                                                        _c128(Z) if want_bases else None, _c128(AZ) if want_bases else None),
               f"mg_block_fgmres_relax_{self._sfx}")
        self._blk_back(X, Xf)
        return (rn[: used.value], H, xi) + ((Z, AZ) if want_bases else ())

    def _set_coarse(self, param, force_sparse: bool = False):
        """`z = param.LU\\b` (MGcycle.jl:177) from the complex splu: the explicit inverse up to DENSE_COARSE_MAX rows, else the
        sparse factors in the parLU layout (mg_set_coarse_lu_CF64_INT64)."""
        import scipy.sparse as sp
        lib = self.lib
        nc = int(param.As[-1].shape[0])
        self._coarse_gmres = False
        self._coarse_device_inverse = False
        if self._set_coarse_solver(param):
            return
        if param.coarseSolveType == "GMRES":                            # param.LU = relaxParam ./ diag(A_c)  (MGsetup.jl:335-336)
            d = param.LU
            if not isinstance(d, np.ndarray) or d.shape != (nc,):
                raise MGDeviceError(f"param.LU is not the coarsest Jacobi vector of {nc} values: run MGsetup first")
            d = np.ascontiguousarray(d, dtype=np.complex128)            # (complex128 for ComplexF32 hierarchies too)
            _check(lib, lib.mg_set_coarse_gmres_CF64(self.handle, nc, _c128(d)), "mg_set_coarse_gmres_CF64")
            self._coarse_gmres = True
            return
        if nc <= DENSE_COARSE_MAX and not force_sparse:
            if self._build_coarse_inverse(param):                       # coarseDeviceInverse: inv(As[end]) built in HBM
                return
            Ainv = np.asfortranarray(param.LU.solve(np.eye(nc, dtype=np.complex128)), dtype=np.complex128)
            _check(lib, lib.mg_set_coarse_dense_inverse_CF64(self.handle, nc, _c128(Ainv)), "mg_set_coarse_dense_inverse_CF64")
            return
        Lp, Lc, Lv, Up, Uc, Uv, p, q = complex_lu_arrays(param.LU)
        _check(lib, lib.mg_set_coarse_lu_CF64_INT64(self.handle, nc, _i64(Lp), _i64(Lc), _c128(Lv), _i64(Up), _i64(Uc), _c128(Uv),
                                                    _i64(p), _i64(q)), "mg_set_coarse_lu_CF64")

    def coarse_gmres(self, b):
        """The GMRES coarsest solve alone (mg_coarse_gmres_CF64): one restart of Jacobi-preconditioned FGMRES(10) from zero on the
        coarsest operator for the complex128 right-hand side ``b``.  Returns (x, flag, resvec): flag 0 (the estimate met 0.01), -1
        (it did not) or -9 (b = 0, x = 0); ``resvec`` holds err_i / ||b|| of the steps used."""
        b = self._host_block(b)
        x = np.zeros(b.shape[0], dtype=np.complex128)
        steps, flag = C.c_longlong(0), C.c_longlong(0)
        res = np.zeros(10)
        _check(self.lib, self.lib.mg_coarse_gmres_CF64(self.handle, _c128(b), _c128(x), b.shape[0], C.byref(steps), C.byref(flag),
                                                       _f64(res)), "mg_coarse_gmres_CF64")
        return x, int(flag.value), res[: steps.value]

    def block_coarse_gmres(self, B):
        """The block GMRES coarsest solve alone (mg_block_coarse_gmres_CF64; a param with ``blockCoarseGMRES=True``): one restart of
        Jacobi-preconditioned blockFGMRES(10) from zero on the coarsest operator for the complex128 block ``B`` (n_c x k, k <= 16).
        Returns (X, flag, resvec): flag 0 / -1 / -9 and the estimates ||xi - H Y||_F / ||B||_F of the steps used, of the whole block."""
        Bf, k = self._blk(B)
        if k > 1:
            self._vanka_block_guard()
        self._block_coarse_guard(k)
        X = np.zeros(Bf.shape, dtype=np.complex128, order="F")
        steps, flag = C.c_longlong(0), C.c_longlong(0)
        res = np.zeros(10)
        _check(self.lib, self.lib.mg_block_coarse_gmres_CF64(self.handle, _c128(Bf), _c128(X), Bf.shape[0], k, C.byref(steps), C.byref(flag),
                                                             _f64(res)), "mg_block_coarse_gmres_CF64")
        return X, int(flag.value), res[: steps.value]

    def block_coarse_form(self, k: int = 2) -> dict:
        """What ``mg_block_coarse_form`` reports for blocks of ``k`` columns: served (blocks run on this handle's GMRES coarsest
        solve), the kernel launches of one block solve, the path in use (0: the chain of grid-wide passes, 1: the one-workgroup form)."""
        info = (C.c_longlong * 3)()
        _check(self.lib, self.lib.mg_block_coarse_form(self.handle, int(k), info), "mg_block_coarse_form")
        return dict(served=bool(info[0]), launches=int(info[1]), path=int(info[2]))

    def set_nrhs(self, nrhs: int):
        if int(nrhs) != 1:
            raise NotImplementedError("ComplexF64 hierarchies serve one right-hand side on the device")
        _check(self.lib, self.lib.mg_set_nrhs(self.handle, 1), "mg_set_nrhs")

    @staticmethod
    def _host_block(a, writable=False, dtype=np.complex128):
        if not isinstance(a, np.ndarray) or a.dtype != dtype:
            raise TypeError(f"expected a {np.dtype(dtype)} numpy array here")
        if a.ndim == 2 and a.shape[1] != 1:
            raise NotImplementedError("ComplexF64 hierarchies serve one right-hand side on the device")
        if not a.flags.c_contiguous and not a.flags.f_contiguous:
            raise ValueError("vectors must be contiguous")
        if writable and not a.flags.writeable:
            raise ValueError("x must be writable (it is updated in place)")
        return a

    def _vp_of(self, a):
        """The vector's address in the handle's own precision (complex128 -> double*, complex64 -> float*)."""
        return a.ctypes.data_as(_dp if self._cdtype == np.complex128 else _fp)

    def cycle(self, b, x, x_is_zero: int = -1):
        b = self._host_block(b, dtype=self._cdtype)
        x = self._host_block(x, True, dtype=self._cdtype)
        _check(self.lib, self._fn("cycle")(self.handle, self._vp_of(b), self._vp_of(x), b.shape[0], 1, int(x_is_zero)),
               f"mg_cycle_{self._sfx}")
        return x

    def solve(self, b, x, tol: float, maxIter: int):
        b = self._host_block(b, dtype=self._cdtype)
        x = self._host_block(x, True, dtype=self._cdtype)
        iters = C.c_longlong(0)
        resvec = np.zeros(int(maxIter) + 1)
        _check(self.lib, self._fn("solve")(self.handle, self._vp_of(b), self._vp_of(x), b.shape[0], 1, float(tol), int(maxIter),
                                           C.byref(iters), _f64(resvec)), f"mg_solve_{self._sfx}")
        return x, int(iters.value), resvec[: iters.value + 1]

    def spmv(self, level: int, which: int, alpha, x, beta, y):
        x = self._host_block(x, dtype=self._cdtype)
        y = self._host_block(y, True, dtype=self._cdtype)
        a = np.array([complex(alpha).real, complex(alpha).imag], dtype=self._rdtype)
        bt = np.array([complex(beta).real, complex(beta).imag], dtype=self._rdtype)
        _check(self.lib, self._fn("spmv")(self.handle, int(level), int(which), self._vp_of(a), self._vp_of(x), self._vp_of(bt),
                                          self._vp_of(y), 1), f"mg_spmv_{self._sfx}")
        return y

    # -- the ComplexF64 Krylov drivers (mg_*_CFP64): BiCGSTAB / FGMRES on a system operator of their own ------------------------
    def set_krylov_operator(self, A):
        """The operator the Krylov drivers apply: a scipy sparse matrix (the APPLIED operator, as ``param.As``; real or complex),
        or None for the hierarchy's own fine level.  The cycle stays the preconditioner.  ``krylov_operator`` is the object
        uploaded last; a refused upload (wrong order) leaves the operator that was there."""
        if A is None:
            self._krylov_operator = None        # (whatever happens below, the object recorded is never one that is not uploaded)
            self._krylov_pattern = None
            _check(self.lib, self.lib.mg_set_krylov_operator_CFP64_INT64(self.handle, self.n, None, None, None),
                   "mg_set_krylov_operator_CFP64")
            return
        import scipy.sparse as sp
        M = sp.csr_matrix(A, dtype=np.complex128, copy=True)
        M.sum_duplicates()
        M.sort_indices()
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
        nzval = np.ascontiguousarray(np.conj(M.data), dtype=np.complex128)     # the reference's AT values
        if M.shape[0] != M.shape[1]:
            raise ValueError("the Krylov operator must be square")
        self._krylov_pattern = None             # (refused or not, the next update_krylov_operator uploads whole)
        _check(self.lib, self.lib.mg_set_krylov_operator_CFP64_INT64(self.handle, M.shape[0], _i64(colptr), _i64(rowval), _c128(nzval)),
               "mg_set_krylov_operator_CFP64")
        self._krylov_operator = A               # the object uploaded last (None: the fine level), whoever asked for it
        self._krylov_pattern = (M.shape, M.indptr, M.indices)

    def update_krylov_operator(self, A):
        """``set_krylov_operator`` for an operator that usually changes its values only (a new medium on the same grid): when A
        has - after the same sum_duplicates / sort_indices - the pattern uploaded last, its values replace the resident ones
        (mg_replace_krylov_values_CFP64: a copy, nothing re-blocked); any other A, None included, is uploaded whole.  Either way
        ``krylov_operator`` becomes A; a refused call leaves what was there."""
        pat = self._krylov_pattern
        if A is None or pat is None or self._krylov_operator is None:
            return self.set_krylov_operator(A)
        import scipy.sparse as sp
        M = sp.csr_matrix(A, dtype=np.complex128, copy=True)
        M.sum_duplicates()
        M.sort_indices()
        if M.shape != pat[0] or M.nnz != pat[2].size or not (np.array_equal(M.indptr, pat[1]) and np.array_equal(M.indices, pat[2])):
            return self.set_krylov_operator(A)
        nzval = np.ascontiguousarray(np.conj(M.data), dtype=np.complex128)     # the reference's AT values
        _check(self.lib, self.lib.mg_replace_krylov_values_CFP64(self.handle, _c128(nzval), nzval.size), "mg_replace_krylov_values_CFP64")
        self._krylov_operator = A

    _krylov_operator = None
    _krylov_pattern = None                      # (shape, indptr, indices) of the operator uploaded last
    _inverse_sfx = "CF64"                       # (mg_build / mg_get_coarse_dense_inverse_CF64 serve CF32 handles too)

    @property
    def krylov_operator(self):
        """The object handed to ``set_krylov_operator`` last (None: the drivers apply the hierarchy's fine level)."""
        return self._krylov_operator

    def _cfp64_driver(self, name, res, b, x, *args):
        """mg_<name>_CFP64(handle, b, x, n, *args, iters, flag, res, count) -> (flag, iters, res[:count]); the caller sizes ``res`` for
        the longest history its driver may write."""
        iters, flag, count = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        fn = getattr(self.lib, f"mg_{name}_CFP64")
        _check(self.lib, fn(self.handle, b, x, self.n, *args, C.byref(iters), C.byref(flag), _f64(res), C.byref(count)), f"mg_{name}_CFP64")
        return int(flag.value), int(iters.value), res[: count.value]

    def _host_pair(self, b, x):
        b = self._host_block(b)
        x = self._host_block(x, True)
        if b.shape[0] != self.n or x.shape[0] != self.n:
            raise ValueError(f"vectors of {self.n} complex values expected")
        return b, x

    @staticmethod
    def _dev_pair(b, x):
        for t in (b, x):
            if hasattr(t, "dtype") and hasattr(t, "data_ptr"):
                import torch
                if t.dtype != torch.complex128:
                    raise TypeError("expected torch.complex128 tensors (the Krylov vectors of a ComplexF32 hierarchy are ComplexF64 too)")
        _sync_torch(b, x)
        return _ptr(b), _ptr(x)

    def bicgstab(self, b, x, tol: float, maxIter: int):
        """KrylovMethods.bicgstb on the Krylov operator with the cycle as M1; returns (x, flag, iters, resvec)."""
        b, x = self._host_pair(b, x)
        return (x,) + self._cfp64_driver("bicgstab", np.zeros(2 * max(int(maxIter), 0) + 1), _c128(b), _c128(x), float(tol), int(maxIter))

    def fgmres(self, b, x, inner: int, tol: float, maxIter: int):
        """KrylovMethods.fgmres (flexible, restarted) on the Krylov operator with the cycle as preconditioner; returns
        (x, flag, inner steps, resvec)."""
        b, x = self._host_pair(b, x)
        return (x,) + self._cfp64_driver("fgmres", np.zeros(max(1, int(inner) * int(maxIter))), _c128(b), _c128(x), int(inner), float(tol),
                                         int(maxIter))

    def bicgstab_dev(self, b, x, tol: float, maxIter: int):
        """The same on torch.complex128 device tensors; returns (flag, iters, resvec)."""
        pb, px = self._dev_pair(b, x)
        return self._cfp64_driver("bicgstab_dev", np.zeros(2 * max(int(maxIter), 0) + 1), pb, px, float(tol), int(maxIter))

    def fgmres_dev(self, b, x, inner: int, tol: float, maxIter: int):
        pb, px = self._dev_pair(b, x)
        return self._cfp64_driver("fgmres_dev", np.zeros(max(1, int(inner) * int(maxIter))), pb, px, int(inner), float(tol), int(maxIter))

    def cycle_dev(self, b, x, x_is_zero: int):
        """One cycle on torch.complex128 device tensors (x_is_zero 0 or 1), enqueued on the library's stream without a
        synchronisation: synchronise the device before reading x."""
        pb, px = self._dev_pair(b, x)
        _check(self.lib, self.lib.mg_cycle_dev_CFP64(self.handle, pb, px, self.n, int(x_is_zero)), "mg_cycle_dev_CFP64")

    # -- blocks of right-hand sides (mg_block_*): the column count travels with each call, the handle's own nrhs stays 1 --------
    @staticmethod
    def _blk(a, writable=False):
        """A complex128 block (n x k; a vector counts as n x 1) as the Fortran-ordered array the host entry points take.
        Returns (f, k): f is `a` itself when it is Fortran-contiguous, else a copy (written back by ``_blk_back``)."""
        if not isinstance(a, np.ndarray) or a.dtype != np.complex128:
            raise TypeError("expected a complex128 numpy array here (blocks of a ComplexF32 hierarchy are ComplexF64 too)")
        a2 = a.reshape(-1, 1) if a.ndim == 1 else a
        if a2.ndim != 2:
            raise ValueError("a block is an n x k array")
        if writable and not a.flags.writeable:
            raise ValueError("X must be writable (it is updated in place)")
        return np.asfortranarray(a2), int(a2.shape[1])

    @staticmethod
    def _blk_back(a, f):
        if not np.shares_memory(a, f):
            a[...] = f.reshape(a.shape)
        return a

    def _block_pair(self, B, X, mismatch: str, need_n: bool = False):
        """What every host block method opens with: the guards, both blocks Fortran-ordered (X writable), the same column count - and,
        with ``need_n``, the fine level's rows - or ValueError(mismatch).  Returns (Bf, Xf, k)."""
        self._block_guard()
        Bf, k = self._blk(B)
        Xf, kx = self._blk(X, True)
        if kx != k or (need_n and (Bf.shape[0] != self.n or Xf.shape[0] != self.n)):
            raise ValueError(mismatch)
        self._block_coarse_guard(k)
        return Bf, Xf, k

    def block_spmv(self, level: int, which: int, alpha, X, beta, Y):
        """``Y = beta*Y + alpha*Op*X`` on one level for n x k complex128 blocks (mg_block_spmv_CF64); Y in place."""
        Xf, Yf, k = self._block_pair(X, Y, "X and Y must hold the same number of columns")
        a = np.array([complex(alpha).real, complex(alpha).imag])
        bt = np.array([complex(beta).real, complex(beta).imag])
        _check(self.lib, self.lib.mg_block_spmv_CF64(self.handle, int(level), int(which), _f64(a), _c128(Xf), _f64(bt), _c128(Yf), k),
               "mg_block_spmv_CF64")
        return self._blk_back(Y, Yf)

    def block_cycle(self, B, X, x_is_zero: int = -1):
        """One cycle on the whole n x k block (mg_block_cycle_CF64); X in place.  x_is_zero is a property of the whole block."""
        Bf, Xf, k = self._block_pair(B, X, "B and X must hold the same number of columns")
        _check(self.lib, self.lib.mg_block_cycle_CF64(self.handle, _c128(Bf), _c128(Xf), Bf.shape[0], k, int(x_is_zero)), "mg_block_cycle_CF64")
        return self._blk_back(X, Xf)

    def block_solve(self, B, X, tol: float, maxIter: int):
        """solveMG on the block with Frobenius norms (mg_block_solve_CF64); returns (X, iters, resvec)."""
        Bf, Xf, k = self._block_pair(B, X, "B and X must hold the same number of columns")
        iters = C.c_longlong(0)
        resvec = np.zeros(int(maxIter) + 1)
        _check(self.lib, self.lib.mg_block_solve_CF64(self.handle, _c128(Bf), _c128(Xf), Bf.shape[0], k, float(tol), int(maxIter),
                                                      C.byref(iters), _f64(resvec)), "mg_block_solve_CF64")
        return self._blk_back(X, Xf), int(iters.value), resvec[: iters.value + 1]

    def _dev_block(self, B, X):
        """Addresses and column count of two torch.complex128 device blocks [n][k], row-major (contiguous)."""
        self._block_guard()
        for t in (B, X):
            if not (hasattr(t, "dtype") and hasattr(t, "data_ptr")):
                raise TypeError("expected torch.complex128 device tensors of shape [n, k]")
            import torch
            if t.dtype != torch.complex128:
                raise TypeError("expected torch.complex128 tensors (the blocks of a ComplexF32 hierarchy are ComplexF64 too)")
            if t.dim() != 2 or not t.is_contiguous() or t.shape[0] != self.n:
                raise ValueError(f"device blocks are contiguous [n, k] tensors with n = {self.n} (row-major)")
        if tuple(B.shape) != tuple(X.shape):
            raise ValueError("B and X must have the same shape")
        self._block_coarse_guard(int(B.shape[1]))
        _sync_torch(B, X)
        return _ptr(B), _ptr(X), int(B.shape[1])

    def block_cycle_dev(self, B, X, x_is_zero: int):
        """One cycle on torch.complex128 device blocks [n, k] (mg_block_cycle_dev_CFP64), enqueued on the library's stream without
        a synchronisation.  On a ComplexF32 hierarchy: the mixed closure on the whole block, from zero."""
        pb, px, k = self._dev_block(B, X)
        _check(self.lib, self.lib.mg_block_cycle_dev_CFP64(self.handle, pb, px, self.n, k, int(x_is_zero)), "mg_block_cycle_dev_CFP64")

    def block_bicgstab(self, B, X, tol: float, maxIter: int):
        """KrylovMethods.blockBiCGSTB on the Krylov operator with the block cycle as M1 (mg_block_bicgstab_CFP64); X in place;
        returns (X, flag, iters, resvec)."""
        Bf, Xf, k = self._block_pair(B, X, f"blocks of {self.n} x k complex values expected, the same k for B and X", need_n=True)
        out = self._cfp64_driver("block_bicgstab", np.zeros(2 * max(int(maxIter), 0) + 1), _c128(Bf), _c128(Xf), k, float(tol), int(maxIter))
        return (self._blk_back(X, Xf),) + out

    def block_bicgstab_dev_CFP64(self, B, X, tol: float, maxIter: int):
        """The same on torch.complex128 device blocks [n, k]; returns (flag, iters, resvec).  (Named after its entry point:
        ``block_bicgstab_dev`` is the FP64 hierarchies' method and stays refused here, as tests/test_complex_krylov_host.py pins.)"""
        pb, px, k = self._dev_block(B, X)
        return self._cfp64_driver("block_bicgstab_dev", np.zeros(2 * max(int(maxIter), 0) + 1), pb, px, k, float(tol), int(maxIter))

    def block_fgmres(self, B, X, inner: int, tol: float, maxIter: int):
        """KrylovMethods.blockFGMRES(inner) on the Krylov operator with the block cycle as preconditioner (mg_block_fgmres_CFP64);
        X in place; returns (X, flag, inner steps in all, resvec with one entry per inner step)."""
        Bf, Xf, k = self._block_pair(B, X, f"blocks of {self.n} x k complex values expected, the same k for B and X", need_n=True)
        out = self._cfp64_driver("block_fgmres", np.zeros(max(int(maxIter), 0) * max(int(inner), 1) + 1), _c128(Bf), _c128(Xf), k, int(inner),
                                 float(tol), int(maxIter))
        return (self._blk_back(X, Xf),) + out

    def block_fgmres_dev_CFP64(self, B, X, inner: int, tol: float, maxIter: int):
        """The same on torch.complex128 device blocks [n, k]; returns (flag, inner steps, resvec).  (``block_fgmres_dev`` is the FP64
        hierarchies' method and stays refused here.)"""
        pb, px, k = self._dev_block(B, X)
        return self._cfp64_driver("block_fgmres_dev", np.zeros(max(int(maxIter), 0) * max(int(inner), 1) + 1), pb, px, k, int(inner), float(tol),
                                  int(maxIter))

    def cblk_gram(self, X, Y):
        """``X^H Y`` (k x k complex128 numpy array) of two torch.complex128 device blocks [n, k] by the one-pass Gram kernel of block
        FGMRES on its own (mg_cblk_gram_dev_CFP64); ``Y is X`` reads the block once.  Synchronises."""
        import torch
        for t in (X, Y):
            if not (hasattr(t, "dtype") and hasattr(t, "data_ptr")) or t.dtype != torch.complex128:
                raise TypeError("expected torch.complex128 device tensors of shape [n, k]")
            if t.dim() != 2 or not t.is_contiguous():
                raise ValueError("device blocks are contiguous [n, k] tensors (row-major)")
        if tuple(X.shape) != tuple(Y.shape):
            raise ValueError("X and Y must have the same shape")
        n, k = int(X.shape[0]), int(X.shape[1])
        work = torch.zeros(2048 * max(k, 1) * max(k, 1), dtype=torch.float64, device=X.device)
        out = torch.zeros((max(k, 1), max(k, 1)), dtype=torch.complex128, device=X.device)
        _sync_torch(X, Y)
        torch.cuda.synchronize()
        _check(self.lib, self.lib.mg_cblk_gram_dev_CFP64(_ptr(X), _ptr(Y), n, k, _ptr(work), _ptr(out), _vp(0)), "mg_cblk_gram_dev_CFP64")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    # -- replaceMatrixInHierarchy on the device (mg_rap_CF64 and the value replacements) ---------------------------------------
    def replace_values(self, level: int, which: int, M):
        """New values of one operator on its unchanged pattern: M.data complex (the applied A) for MG_OP_A, real for P and R."""
        if which == MG_OP_A:
            nz = np.ascontiguousarray(np.conj(M.data), dtype=self._cdtype)      # the reference's AT values
        else:
            if np.iscomplexobj(M.data):
                raise TypeError("P and R of a complex hierarchy are real")
            nz = np.ascontiguousarray(M.data, dtype=self._rdtype)
        _check(self.lib, self._fn("replace_values")(self.handle, int(level), int(which), self._vp_of(nz), M.data.size),
               f"mg_replace_values_{self._sfx}")

    def get_values(self, level: int, which: int) -> np.ndarray:
        """Values of operator `which` of `level` as applied (stored CSR order): complex128 for A, float64 for P and R (a ComplexF32
        hierarchy: complex64 and float32)."""
        if (int(level), int(which)) not in self._op_nnz:
            raise MGDeviceError(f"get_values: level {level} holds no operator {which}")
        vals = np.zeros(self._op_nnz[(int(level), int(which))], dtype=self._cdtype if which == MG_OP_A else self._rdtype)
        _check(self.lib, self._fn("get_values")(self.handle, int(level), int(which), self._vp_of(vals), vals.size),
               f"mg_get_values_{self._sfx}")
        return np.conjugate(vals, out=vals) if which == MG_OP_A else vals

    def replace_matrix(self, param, A_new, timings: Optional[dict] = None) -> None:
        """replaceMatrixInHierarchy on the device, the complex twin of DeviceHierarchy.replace_matrix: numeric Galerkin products
        and relaxPrecs on the fixed patterns (mg_rap_CF64), host copies of the hierarchy refreshed from HBM, coarsest level
        re-factored on the host (with coarseSolveType='GMRES' there is nothing to factor: its Jacobi vector is recomputed in HBM;
        a param with ``coarseDeviceInverse=True``: the explicit inverse is rebuilt in HBM by mg_rap_CF64 and ``coarsest`` is the
        host's splu alone).  ``timings`` (a dict) receives the seconds of the three parts.  A ComplexF32 hierarchy whose param
        carries ``singleDeviceSetup`` runs the same steps through the _CF32 entry points, its values complex64."""
        import time
        lib = self.lib
        t0 = time.perf_counter()
        nz = np.ascontiguousarray(np.conj(A_new.data), dtype=self._cdtype)      # the reference's AT values
        rp = param.relaxParam
        vanka = getattr(self, "_vanka", False)
        if vanka and not getattr(self, "_vanka_device_setup", False):
            raise MGDeviceError("replace_matrix of a complex Vanka hierarchy needs the device set-up of its blocks "
                                "(getMGparam(..., complexVanka=True, vankaDeviceSetup=True))")
        if vanka:     # (the levels remember their own (VankaType, w): omega is validated and not used)
            omega = np.ones(self.nlevels, dtype=np.float64)
        else:
            omega = np.ascontiguousarray([float(rp[l]) if isinstance(rp, (list, tuple, np.ndarray)) else float(rp)
                                          for l in range(self.nlevels)], dtype=np.float64)
        kind = 1 if param.relaxType == "SPAI" else 0
        done = C.c_longlong(0)
        _check(lib, self._fn("rap")(self.handle, self._vp_of(nz), nz.size, kind, _f64(omega), C.byref(done)), f"mg_rap_{self._sfx}")
        t1 = time.perf_counter()
        param.As[0] = A_new
        for l in range(2, self.nlevels + 1):                       # refresh the host copies (same patterns)
            M = param.As[l - 1]
            vals = np.empty(M.nnz, dtype=self._cdtype)
            _check(lib, self._fn("get_values")(self.handle, l, MG_OP_A, self._vp_of(vals), vals.size), f"mg_get_values_{self._sfx}")
            np.conjugate(vals, out=M.data)
        tb = time.perf_counter()
        for l in range(1, self.nlevels):
            if vanka:                                              # the cells' blocks, rebuilt in HBM (mg_get_vanka_blocks_CF64)
                param.relaxPrecs[l - 1] = self.vanka_blocks(l)
                continue
            d = np.empty(param.As[l - 1].shape[0], dtype=self._cdtype)
            _check(lib, self._fn("get_relax")(self.handle, l, self._vp_of(d), d.size), f"mg_get_relax_{self._sfx}")
            param.relaxPrecs[l - 1] = d
        t2 = time.perf_counter()
        from .mgsetup import defineCoarsestAinv
        defineCoarsestAinv(param, param.As[-1])                      # (MGsetup.jl:323-355)
        if not getattr(self, "_coarse_gmres", False) and not self._coarse_device_inverse:
            self._set_coarse(param)
            _check(lib, lib.mg_finalize(self.handle), "mg_finalize")
        # (coarseDeviceInverse: mg_rap_CF64 has rebuilt the explicit inverse in HBM behind its last Galerkin product; param.LU above
        #  stays the host's splu - nothing uploaded)
        # (GMRES coarsest solve: param.LU = relaxParam ./ diag(As[-1]) above is the host's copy; mg_rap_CF64 has recomputed the device's
        #  in HBM - no inverse, no factorisation, nothing uploaded)
        if timings is not None:
            timings.update(rap=t1 - t0, readback=t2 - t1, coarsest=time.perf_counter() - t2)
            if vanka:     # (the part of `readback` spent on the blocks)
                timings.update(blocks_readback=t2 - tb)

    def adjoint_hierarchy(self, param) -> None:
        """adjointHierarchy on the resident hierarchy (mg_adjoint_hierarchy_CF64 / _CF32): every operator replaced by its conjugate
        transpose in HBM, relaxPrecs conjugated, Ps[l] <- Rs[l]', the dense coarsest inverse or the GMRES coarsest vector flipped
        in place.  ``param`` is the host mirror ALREADY flipped (mgsetup.adjointHierarchy calls this last): its Ps give the sizes
        ``get_values`` needs.  Raises MGDeviceError where the library refuses (sparse coarsest factors, a Schwarz coarsest solve,
        64-bit row pointers, a column of more than 4096 entries); the handle then cycles with its old bits."""
        _check(self.lib, self._fn("adjoint_hierarchy")(self.handle), f"mg_adjoint_hierarchy_{self._sfx}")
        for l in range(1, self.nlevels):
            self._op_nnz[(l, MG_OP_P)] = int(param.Ps[l - 1].nnz)

    def rap_level_ms(self) -> np.ndarray:
        """Device milliseconds of the last replace_matrix per level (relaxPrecs[l] and As[l+1] together; mg_rap_level_ms_*)."""
        out = np.zeros(self.nlevels - 1)
        _check(self.lib, self._fn("rap_level_ms")(self.handle, _f64(out), out.size), f"mg_rap_level_ms_{self._sfx}")
        return out

    def _refuse(self, *args, **kwargs):
        raise NotImplementedError("PCG, block PCG / FGMRES, transposeHierarchy and the other device-pointer entry points serve "
                                  "FP64 hierarchies only (ComplexF64: adjoint_hierarchy; bicgstab, fgmres, cycle_dev and their _dev forms; block_spmv, "
                                  "block_cycle, block_solve, block_cycle_dev, block_bicgstab, block_bicgstab_dev_CFP64, block_fgmres, "
                                  "block_fgmres_dev_CFP64; replace_matrix, "
                                  "replace_values, get_values)")

    pcg = cycle_mixed_f32 = pcg_dev = block_pcg_dev = block_bicgstab_dev = block_fgmres_dev = _refuse
    solve_dev = spmv_dev = fused_dev = sweep_residual_dev = four_stage_dev = _refuse
    transpose_hierarchy = cycle_async_dev = _refuse


class ComplexSingleDeviceHierarchy(ComplexDeviceHierarchy):
    """A ComplexF32 hierarchy on the device (mg_create_CF32; ``getMGparam(np.complex128, ..., singlePrecision=True)``): As and
    relaxPrecs complex64, Ps / Rs float32, the cycle in single precision by the same kernels; the coarsest solve stays
    ComplexF64.  ``cycle``, ``solve``, ``spmv`` take complex64 arrays.  ``bicgstab``, ``fgmres``, their ``_dev`` forms,
    ``cycle_dev``, ``set_krylov_operator`` and ``update_krylov_operator`` take complex128 arrays and tensors: the Krylov method
    runs in ComplexF64 and is preconditioned by the single cycle (narrowed in, widened out; SolveFuncs.jl:52-58).  A param with
    ``singleKcycle=True`` adds the K-cycle and Jac-GMRES smoothing (option single_kcycle, mg_set_schedule_CF32; Gram sums and least
    squares in double) and ``fgmres_relax`` on complex64 vectors; without it both are refused."""

    _cdtype = np.complex64
    _rdtype = np.float32
    _sfx = "CF32"

    def _set_op(self, level, which, M):
        self._op_nnz[(int(level), int(which))] = int(M.nnz)
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
        if which == MG_OP_A:
            if M.dtype != np.complex64:
                raise TypeError("As of a ComplexF32 hierarchy are complex64")
            nzval = np.ascontiguousarray(np.conj(M.data), dtype=np.complex64)     # the reference's AT values
        else:
            if M.dtype != np.float32:
                raise TypeError("Ps and Rs of a ComplexF32 hierarchy are float32")
            nzval = np.ascontiguousarray(M.data, dtype=np.float32)
        rc = self.lib.mg_set_operator_CF32_INT64(self.handle, level, which, M.shape[0], M.shape[1], _i64(colptr), _i64(rowval),
                                                 nzval.ctypes.data_as(_fp))
        _check(self.lib, rc, f"mg_set_operator_CF32(level={level}, which={which})")

    def _set_relax(self, level, d, pre, post):
        if np.asarray(d).dtype != np.complex64:
            raise TypeError("relaxPrecs of a ComplexF32 hierarchy are complex64")
        d = np.ascontiguousarray(d, dtype=np.complex64)
        _check(self.lib, self.lib.mg_set_relax_CF32(self.handle, level, d.ctypes.data_as(_fp), d.size, int(pre), int(post)),
               f"mg_set_relax_CF32(level={level})")

    _single_device_setup = False      # the param uploaded last carried singleDeviceSetup: the four methods below are served

    _single_kcycle = False            # the param uploaded last carried singleKcycle: 'K' and Jac-GMRES are served (option single_kcycle)

    def _upload(self, param):
        self._single_device_setup = bool(getattr(param, "singleDeviceSetup", False))
        self._single_kcycle = bool(getattr(param, "singleKcycle", False))
        if self._single_kcycle:           # (ahead of the schedule: mg_set_schedule_CF32 and mg_finalize read it)
            _check(self.lib, self.lib.mg_set_option(self.handle, b"single_kcycle", 1.0), "mg_set_option(single_kcycle)")
        super()._upload(param)

    def _refuse_single(self, *args, **kwargs):
        raise NotImplementedError("ComplexF32 hierarchies: replace_matrix, replace_values, get_values and rap_level_ms on the device are "
                                  "served for a param with singleDeviceSetup=True (without it replaceMatrixInHierarchy recomputes on "
                                  "the host and uploads again)")

    def _served_single(name):
        """The ComplexF64 method of that name, by the _CF32 entry points, where the param asked for it; the refusal otherwise."""
        def method(self, *args, **kwargs):
            if not self._single_device_setup:
                return self._refuse_single()
            return getattr(ComplexDeviceHierarchy, name)(self, *args, **kwargs)
        method.__name__ = name
        method.__doc__ = getattr(ComplexDeviceHierarchy, name).__doc__
        return method

    replace_matrix = _served_single("replace_matrix")
    replace_values = _served_single("replace_values")
    get_values = _served_single("get_values")
    rap_level_ms = _served_single("rap_level_ms")
    del _served_single


def complex_lu_arrays(lu):
    """A complex scipy splu in the parLU layout (deps/src/parLU.cpp:120-190): CSR L with the diagonal last, CSR U with the
    diagonal first, 1-based Int64 pointers / indices, complex values, p and q with A[p, q] = L U."""
    import scipy.sparse as sp
    L = sp.csr_matrix(lu.L)
    U = sp.csr_matrix(lu.U)
    L.sort_indices()
    U.sort_indices()
    a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    c128 = lambda a: np.ascontiguousarray(a, dtype=np.complex128)
    p = a64(np.argsort(lu.perm_r)) + 1
    q = a64(np.argsort(lu.perm_c)) + 1
    return (a64(L.indptr) + 1, a64(L.indices) + 1, c128(L.data), a64(U.indptr) + 1, a64(U.indices) + 1, c128(U.data), p, q)


class DeviceOperator:
    """One CSR operator resident in HBM on its own (``mg_operator``): the building block of the multi-GPU
    cycle, where a rank holds its rows of A/P/R with halo columns appended.  Asynchronous on `stream`."""

    def __init__(self, M, device_id: int = 0, box=None, regular_cols=None, coarse_box=None):
        """box=(n1,n2,n3), regular_cols: the BOX form of a sharded level's local A (mg_op_create_box_FP64_INT64): M is
        square [owned box in natural order | halo] with empty halo rows.  With coarse_box=(c1,c2,c3) as well: the grid form
        of a local P (mg_op_create_grid_FP64_INT64): rows = the owned fine box `box`, columns = [owned coarse box | halo]."""
        self.lib = load_library()
        self.handle = _vp()
        colptr, rowval, nzval = _julia_arrays(M)
        if M.nnz == 0:                                   # keep the arrays non-empty for ctypes
            rowval = np.zeros(1, dtype=np.int64)
            nzval = np.zeros(1)
        self.shape = M.shape
        self.nnz = int(M.nnz)
        self.box = box is not None
        if regular_cols is not None and box is None and coarse_box is None:
            # only the owned | halo column split (a local restriction): rows reading a halo column go to phase 2
            _check(self.lib, self.lib.mg_op_create_grid_FP64_INT64(int(device_id), M.shape[0], M.shape[1], _i64(colptr),
                                                                   _i64(rowval), _f64(nzval), int(regular_cols),
                                                                   0, 0, 0, 0, 0, 0, C.byref(self.handle)), "mg_op_create_grid")
        elif box is not None and coarse_box is not None:
            f = (list(box) + [1, 1])[:3]
            c = (list(coarse_box) + [1, 1])[:3]
            _check(self.lib, self.lib.mg_op_create_grid_FP64_INT64(int(device_id), M.shape[0], M.shape[1], _i64(colptr),
                                                                   _i64(rowval), _f64(nzval), int(regular_cols),
                                                                   int(f[0]), int(f[1]), int(f[2]), int(c[0]), int(c[1]),
                                                                   int(c[2]), C.byref(self.handle)), "mg_op_create_grid")
        elif box is not None:
            n1, n2, n3 = (list(box) + [1, 1])[:3]
            _check(self.lib, self.lib.mg_op_create_box_FP64_INT64(int(device_id), M.shape[0], M.shape[1], _i64(colptr),
                                                                  _i64(rowval), _f64(nzval), int(n1), int(n2), int(n3),
                                                                  int(regular_cols), C.byref(self.handle)), "mg_op_create_box")
        else:
            _check(self.lib, self.lib.mg_op_create_FP64_INT64(int(device_id), M.shape[0], M.shape[1], _i64(colptr),
                                                              _i64(rowval), _f64(nzval), C.byref(self.handle)),
                   "mg_op_create")

    def bind_relax(self, d, n: int):
        """The relaxPrec vector (CUDA tensor) this operator is swept with: read from the class dictionary where possible."""
        _check(self.lib, self.lib.mg_op_bind_relax_dev_FP64(self.handle, _ptr(d), int(n)), "mg_op_bind_relax_dev")

    def kernel_variant(self):
        """(kernel variant as DeviceHierarchy.operator_kernel_variant, number of exception rows)."""
        a, b = C.c_longlong(0), C.c_longlong(0)
        _check(self.lib, self.lib.mg_op_kernel_variant(self.handle, C.byref(a), C.byref(b)), "mg_op_kernel_variant")
        return int(a.value), int(b.value)

    def apply(self, kernel, x, y, b=None, d=None, alpha=1.0, beta=0.0, nrhs=1, stream=0, row_offset=0, phase=0):
        _check(self.lib, self.lib.mg_op_apply_phase_dev_FP64(self.handle, int(kernel), float(alpha), _ptr(x), float(beta),
                                                             _ptr(y), _ptr(b) if b is not None else None,
                                                             _ptr(d) if d is not None else None, int(nrhs),
                                                             int(row_offset), int(phase), _vp(stream)),
               "mg_op_apply_phase_dev")

    def can_sweep_residual(self, x, d):
        """(yes, rows of list 1, rows of list 2): can the two-stage pass serve this operator with these vectors, and how
        many rows does it leave to ``apply_list``?"""
        y, a, b = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _check(self.lib, self.lib.mg_op_can_sweep_residual(self.handle, _ptr(x), _ptr(d), C.byref(y), C.byref(a), C.byref(b)),
               "mg_op_can_sweep_residual")
        return bool(y.value), int(a.value), int(b.value)

    def sweep_residual(self, x, b, d, t=None, r=None, xn=None, partials=None, stream=0):
        """t = x + d.*(b - M x) and r = b - M t [xn = t + d.*r, ||r||^2 partials] in one pass; returns the number of partials."""
        n = C.c_longlong(0)
        opt = lambda v: _ptr(v) if v is not None else None
        _check(self.lib, self.lib.mg_op_sweep_residual_dev_FP64(self.handle, _ptr(x), _ptr(b), _ptr(d), opt(t), opt(r), opt(xn),
                                                                opt(partials), C.byref(n), _vp(stream)), "mg_op_sweep_residual_dev")
        return int(n.value)

    def apply_list(self, which, kernel, x, y, b, d=None, y2=None, partials=None, stream=0):
        """The rows the two-stage pass leaves out (list 1: rows without a class; list 2: rows next to them), from the CSR arrays."""
        n = C.c_longlong(0)
        opt = lambda v: _ptr(v) if v is not None else None
        _check(self.lib, self.lib.mg_op_apply_list_dev_FP64(self.handle, int(which), int(kernel), _ptr(x), opt(y), _ptr(b), opt(d),
                                                            opt(y2), opt(partials), C.byref(n), _vp(stream)), "mg_op_apply_list_dev")
        return int(n.value)

    def close(self):
        if self.handle:
            self.lib.mg_op_destroy(self.handle)
            self.handle = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_register(a: np.ndarray):
    """Page-lock a long-lived numpy array (mg_host_register); the caller unregisters it before it is freed."""
    lib = load_library()
    _check(lib, lib.mg_host_register(_vp(a.ctypes.data), a.nbytes), "mg_host_register")


def host_unregister(a: np.ndarray):
    lib = load_library()
    _check(lib, lib.mg_host_unregister(_vp(a.ctypes.data)), "mg_host_unregister")


def vec_dscale(d, b, x, n, nrhs=1, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_dscale_dev_FP64(_ptr(d), _ptr(b), _ptr(x), int(n), int(nrhs), _vp(stream)), "mg_vec_dscale_dev")


def vec_xpdr(x, d, r, xout, n, nrhs=1, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_xpdr_dev_FP64(_ptr(x), _ptr(d), _ptr(r), _ptr(xout), int(n), int(nrhs), _vp(stream)),
           "mg_vec_xpdr_dev")


def vec_sumsq(x, length, workspace, out, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_sumsq_dev_FP64(_ptr(x), int(length), _ptr(workspace), _ptr(out), _vp(stream)),
           "mg_vec_sumsq_dev")


# ---- the fused vector passes of the sharded Krylov drivers (csrc/mg_krvec.hpp): device tensors, asynchronous on `stream`;
#      workspace: KRV_WORKSPACE doubles, out: the pass's sums (device) --------------------------------------------------------
KRV_WORKSPACE = 8192


def _ptr_array(tensors):
    return (_vp * len(tensors))(*[_ptr(t) for t in tensors])


def vec_dots(xs, ys, n, workspace, out, stream=0):
    """out[c] = xs[c]'ys[c] over n elements, c < len(xs) <= 8, in one pass."""
    lib = load_library()
    _check(lib, lib.mg_vec_dots_dev_FP64(len(xs), _ptr_array(xs), _ptr_array(ys), int(n), _ptr(workspace), _ptr(out), _vp(stream)),
           "mg_vec_dots_dev")


def vec_pcg_dots(p, q, r, n, workspace, out, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_pcg_dots_dev_FP64(_ptr(p), _ptr(q), _ptr(r), int(n), _ptr(workspace), _ptr(out), _vp(stream)), "mg_vec_pcg_dots_dev")


def vec_pcg_update(alpha, p, q, x, r, n, workspace, out, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_pcg_update_dev_FP64(float(alpha), _ptr(p), _ptr(q), _ptr(x), _ptr(r), int(n), _ptr(workspace), _ptr(out),
                                               _vp(stream)), "mg_vec_pcg_update_dev")


def vec_xpby(x, beta, y, n, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_xpby_dev_FP64(_ptr(x), float(beta), _ptr(y), int(n), _vp(stream)), "mg_vec_xpby_dev")


def vec_scale(a, x, y, n, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_scale_dev_FP64(float(a), _ptr(x), _ptr(y), int(n), _vp(stream)), "mg_vec_scale_dev")


def vec_bicg_p(beta, omega, r, v, p, n, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_bicg_p_dev_FP64(float(beta), float(omega), _ptr(r), _ptr(v), _ptr(p), int(n), _vp(stream)), "mg_vec_bicg_p_dev")


def vec_bicg_s(alpha, v, r, n, workspace, out, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_bicg_s_dev_FP64(float(alpha), _ptr(v), _ptr(r), int(n), _ptr(workspace), _ptr(out), _vp(stream)), "mg_vec_bicg_s_dev")


def vec_bicg_ts(t, s, n, workspace, out, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_bicg_ts_dev_FP64(_ptr(t), _ptr(s), int(n), _ptr(workspace), _ptr(out), _vp(stream)), "mg_vec_bicg_ts_dev")


def vec_bicg_xr(alpha, omega, phat, shat, t, rtld, x, r, n, workspace, out, stream=0):
    lib = load_library()
    _check(lib, lib.mg_vec_bicg_xr_dev_FP64(float(alpha), float(omega), _ptr(phat), _ptr(shat), _ptr(t), _ptr(rtld), _ptr(x), _ptr(r), int(n),
                                            _ptr(workspace), _ptr(out), _vp(stream)), "mg_vec_bicg_xr_dev")


def vec_gs_update(h, vs, w, n, workspace, out=None, stream=0):
    """w -= sum_j h[j] vs[j]; out (optional, device) = w'w."""
    lib = load_library()
    hh = np.ascontiguousarray(h, dtype=np.float64)
    _check(lib, lib.mg_vec_gs_update_dev_FP64(len(vs), _f64(hh), _ptr_array(vs), _ptr(w), int(n), _ptr(workspace),
                                              _ptr(out) if out is not None else None, _vp(stream)), "mg_vec_gs_update_dev")


# ---- the fused ComplexF64 vector passes of the complex Krylov drivers (csrc/mg_cxvec.hpp): torch.complex128 device tensors on a
#      16-byte boundary, asynchronous on `stream`; workspace: KRV_WORKSPACE doubles, out: the pass's sums (device doubles) ----------
def _cpair(a):
    a = complex(a)
    return _f64(np.array([a.real, a.imag]))


def cvec_dots(xs, ys, n, workspace, out, stream=0):
    """out[2c], out[2c+1] = re, im of dot(xs[c], ys[c]) = sum conj(xs[c]) ys[c] over n elements, c < len(xs) <= 4, in one pass."""
    lib = load_library()
    _check(lib, lib.mg_cvec_dots_dev_CFP64(len(xs), _ptr_array(xs), _ptr_array(ys), int(n), _ptr(workspace), _ptr(out), _vp(stream)),
           "mg_cvec_dots_dev")


def cvec_scale(a, x, y, n, stream=0):
    lib = load_library()
    _check(lib, lib.mg_cvec_scale_dev_CFP64(_cpair(a), _ptr(x), _ptr(y), int(n), _vp(stream)), "mg_cvec_scale_dev")


def cvec_bicg_p(beta, omega, r, v, p, n, stream=0):
    lib = load_library()
    _check(lib, lib.mg_cvec_bicg_p_dev_CFP64(_cpair(beta), _cpair(omega), _ptr(r), _ptr(v), _ptr(p), int(n), _vp(stream)), "mg_cvec_bicg_p_dev")


def cvec_bicg_s(alpha, v, r, n, workspace, out, stream=0):
    lib = load_library()
    _check(lib, lib.mg_cvec_bicg_s_dev_CFP64(_cpair(alpha), _ptr(v), _ptr(r), int(n), _ptr(workspace), _ptr(out), _vp(stream)), "mg_cvec_bicg_s_dev")


def cvec_bicg_ts(t, s, n, workspace, out, stream=0):
    """out = (re, im of dot(t, s), dot(t, t))."""
    lib = load_library()
    _check(lib, lib.mg_cvec_bicg_ts_dev_CFP64(_ptr(t), _ptr(s), int(n), _ptr(workspace), _ptr(out), _vp(stream)), "mg_cvec_bicg_ts_dev")


def cvec_bicg_xr(alpha, omega, phat, shat, t, rtld, x, r, n, workspace, out, stream=0):
    """x += alpha phat + omega shat ; r -= omega t ; out = (||r||^2, re, im of dot(rtld, r))."""
    lib = load_library()
    _check(lib, lib.mg_cvec_bicg_xr_dev_CFP64(_cpair(alpha), _cpair(omega), _ptr(phat), _ptr(shat), _ptr(t), _ptr(rtld), _ptr(x), _ptr(r),
                                              int(n), _ptr(workspace), _ptr(out), _vp(stream)), "mg_cvec_bicg_xr_dev")


def cvec_gs_update(h, vs, w, n, workspace, out=None, stream=0):
    """w -= sum_j h[j] vs[j] (complex h, one vs[j] after the other); out (optional, device) = ||w||^2."""
    lib = load_library()
    hh = np.ascontiguousarray(h, dtype=np.complex128)
    _check(lib, lib.mg_cvec_gs_update_dev_CFP64(len(vs), _c128(hh), _ptr_array(vs), _ptr(w), int(n), _ptr(workspace),
                                                _ptr(out) if out is not None else None, _vp(stream)), "mg_cvec_gs_update_dev")
