"""ctypes binding of libace_sfno.so (include/ace_sfno.h).

The product path has no CPU or eager-torch fallback: if the HIP library is
missing this module raises, loudly, at first use."""

import contextlib
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACE_SFNO_LIB") or os.path.join(HERE, "libace_sfno.so")   # ACE_SFNO_LIB: A/B a variant build

ACE_OK, ACE_ERR_INVALID, ACE_ERR_RUNTIME, ACE_ERR_STATE = 0, -1, -2, -3


class AceSfnoConfig(ctypes.Structure):
    """struct ace_sfno_config (include/ace_sfno.h)."""

    _fields_ = [
        ("in_chans", c_int), ("out_chans", c_int), ("nlat", c_int), ("nlon", c_int),
        ("embed_dim", c_int), ("num_layers", c_int), ("scale_factor", c_int),
        ("hard_thresholding_fraction", c_float), ("operator_type", c_int),
        ("normalization_layer", c_int), ("activation_function", c_int), ("use_mlp", c_int),
        ("mlp_ratio", c_float), ("encoder_layers", c_int), ("pos_embed", c_int), ("big_skip", c_int),
        ("data_grid", c_int), ("max_batch", c_int), ("precision", c_int),
        ("noise_embed_dim", c_int), ("affine_norms", c_int), ("normalize_big_skip", c_int), ("filter_num_groups", c_int),
        ("residual_filter_factor", c_int),
    ]


# ---- post-step physics (ace_physics_*): struct ace_phys_plane / ace_phys_config / ace_phys_fields
MAX_LEVELS, MAX_POSITIVE, MAX_PRESCRIBED = 16, 32, 8


class Plane(ctypes.Structure):
    _fields_ = [("p", c_void_p), ("stride", c_long)]


def bind_plane(dst: Plane, t, batch: int, shape, device, who: str, name: str) -> None:
    """Point ``dst`` at the (batch, H, W) fp32 planes of ``t`` ((batch, 1, H, W) is squeezed): rows contiguous, any sample stride."""
    import torch

    B, (H, W) = batch, shape
    if t.dtype != torch.float32 or t.device != device:
        raise TypeError(f"{who}: '{name}' must be float32 on {device}, got {t.dtype} on {t.device}")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or tuple(t.shape) != (B, H, W) or t.stride(-1) != 1 or t.stride(-2) != W:
        raise ValueError(f"{who}: '{name}' must be ({B}, {H}, {W}) with contiguous rows, got shape "
                         f"{tuple(t.shape)} strides {t.stride()}")
    dst.p, dst.stride = t.data_ptr(), (t.stride(0) if B > 1 else H * W)


class PhysConfig(ctypes.Structure):
    """struct ace_phys_config"""
    _fields_ = [("nlat", c_int), ("nlon", c_int), ("nlev", c_int), ("timestep_seconds", c_double),
                ("conserve_dry_air", c_int), ("zero_global_mean_moisture_advection", c_int), ("moisture_budget", c_int),
                ("clip_frozen_precipitation", c_int), ("energy_budget", c_int), ("unaccounted_heating", c_double),
                ("ocean", c_int), ("max_batch", c_int)]


class PhysFields(ctypes.Structure):
    """struct ace_phys_fields"""
    _fields_ = [("ps", Plane), ("wat", Plane * MAX_LEVELS), ("T", Plane * MAX_LEVELS), ("adv", Plane), ("precip", Plane),
                ("lhf", Plane), ("shf", Plane), ("dswsfc", Plane), ("uswsfc", Plane), ("dlwsfc", Plane), ("ulwsfc", Plane),
                ("ulwtoa", Plane), ("uswtoa", Plane), ("frozen", Plane), ("frozen_parts", Plane * 3),
                ("positive", Plane * MAX_POSITIVE), ("npositive", c_int),
                ("ps_in", Plane), ("wat_in", Plane * MAX_LEVELS), ("T_in", Plane * MAX_LEVELS), ("hgt_in", Plane),
                ("hgt_next", Plane), ("dswtoa_next", Plane), ("hgt_in_scale", c_float), ("hgt_next_scale", c_float),
                ("sst", Plane), ("sst_target", Plane), ("ocean_fraction", Plane),
                ("prescribed_dst", Plane * MAX_PRESCRIBED), ("prescribed_src", Plane * MAX_PRESCRIBED), ("nprescribed", c_int)]


# ---- ocean corrector (ace_ocean_phys_*): struct ace_ocean_config / ace_ocean_fields
OCEAN_MAX_LEVELS, OCEAN_MAX_POSITIVE, OCEAN_MAX_ZERO = 64, 40, 8


class OceanConfig(ctypes.Structure):
    """struct ace_ocean_config"""
    _fields_ = [("nlat", c_int), ("nlon", c_int), ("nlev", c_int), ("max_batch", c_int), ("sea_ice", c_int),
                ("remove_negative_ocean_fraction", c_int), ("hfds", c_int), ("ohc", c_int), ("timestep_seconds", c_double),
                ("unaccounted_heating", c_double)]


class OceanFields(ctypes.Structure):
    """struct ace_ocean_fields"""
    _fields_ = [("positive", Plane * OCEAN_MAX_POSITIVE), ("npositive", c_int), ("sif", Plane), ("zero", Plane * OCEAN_MAX_ZERO),
                ("nzero", c_int), ("hfds", Plane), ("hfds_total_area", c_int), ("thetao", Plane * OCEAN_MAX_LEVELS), ("sst", Plane),
                ("reb_land", Plane), ("in_land", Plane), ("in_sif", Plane), ("in_sst", Plane), ("in_sif_is_ocean_sif", c_int),
                ("thetao_in", Plane * OCEAN_MAX_LEVELS), ("in_flux", Plane), ("in_ssf", Plane), ("in_ssf_is_land", c_int),
                ("flux_source", c_int), ("dlw", Plane), ("ulw", Plane), ("dsw", Plane), ("usw", Plane), ("lhf", Plane), ("shf", Plane),
                ("precip", Plane), ("frozen", Plane), ("frozen_parts", Plane * 3), ("f_ssf", Plane), ("f_ssf_is_land", c_int),
                ("hfgeou", Plane)]


# ---- sea-ice budget corrector (ace_ice_budget_*): struct ace_ice_var / ace_ice_fields
ICE_MAX_VARS, ICE_FLAG_BYTES = 3, 64


class IceVar(ctypes.Structure):
    """struct ace_ice_var"""
    _fields_ = [("old_mass", Plane), ("source", Plane), ("sink", Plane), ("transport", Plane), ("mass", Plane), ("area_mode", c_int),
                ("masked", c_int)]


class IceFields(ctypes.Structure):
    """struct ace_ice_fields"""
    _fields_ = [("var", IceVar * ICE_MAX_VARS), ("nvars", c_int)]


# ---- the ocean's derived variables (ace_ocean_derive_window): struct ace_ocean_derive_field / _level / _desc
OCEAN_DERIVE_OUTPUTS = ("ocean_heat_content", "ocean_heat_content_tendency", "implied_tendency_of_ocean_heat_content_due_to_advection",
                        "net_energy_flux_into_ocean_column", "sea_ice_fraction", "HI", "hfds")      # bit i of `want`, slot i of `out`


class OceanDeriveField(ctypes.Structure):
    """struct ace_ocean_derive_field"""
    _fields_ = [("base", c_void_p), ("bstride", c_long), ("tstride", c_long)]


class OceanDeriveLevel(ctypes.Structure):
    """struct ace_ocean_derive_level"""
    _fields_ = [("f", OceanDeriveField), ("head", c_void_p), ("head_bstride", c_long)]


class OceanDeriveDesc(ctypes.Structure):
    """struct ace_ocean_derive_desc"""
    _fields_ = [("nlev", c_int), ("thetao", OceanDeriveLevel * OCEAN_MAX_LEVELS), ("dz", c_void_p), ("mask0", c_void_p),
                ("area_m2", c_void_p), ("hfds", OceanDeriveField), ("hfds_total_area", OceanDeriveField), ("hfgeou", OceanDeriveField),
                ("sea_surface_fraction", OceanDeriveField), ("land_fraction", OceanDeriveField),
                ("ocean_sea_ice_fraction", OceanDeriveField), ("sea_ice_fraction", OceanDeriveField), ("sea_ice_volume", OceanDeriveField),
                ("out", c_void_p * len(OCEAN_DERIVE_OUTPUTS)), ("out_bstride", c_long), ("out_tstride", c_long),
                ("want", ctypes.c_uint), ("has_head", c_int), ("dt_seconds", c_double), ("batch", c_int), ("steps", c_int),
                ("hw", c_long), ("t_chunk", c_int)]


class GemmRoute(ctypes.Structure):
    """struct ace_gemm_route"""
    _fields_ = [("family", c_int), ("tile", c_int)]


class Conv1x1FusedDesc(ctypes.Structure):
    """struct ace_conv1x1_fused_desc"""
    _fields_ = [("x", c_void_p), ("x2", c_void_p), ("weight", c_void_p), ("bias", c_void_p), ("in_scale", c_void_p),
                ("in_shift", c_void_p), ("res", c_void_p), ("res_scale", c_void_p), ("res_shift", c_void_p),
                ("out_scale", c_void_p), ("out_shift", c_void_p), ("y", c_void_p), ("out_absmax", c_void_p),
                ("n", c_int), ("cin", c_int), ("cin2", c_int), ("cout", c_int),
                ("hw", c_long), ("in_pitch", c_long), ("out_pitch", c_long),
                ("act", c_int), ("cap", c_float), ("engine", c_int)]


class DftRoute(ctypes.Structure):
    """struct ace_dft_route"""
    _fields_ = [("form", c_int), ("rows", c_int), ("units", c_int), ("rode", c_int)]


class DftStageDesc(ctypes.Structure):
    """struct ace_dft_stage_desc"""
    _fields_ = [("inverse", c_int), ("engine", c_int), ("bt", c_int), ("c", c_int),
                ("x", c_void_p), ("xhi", c_void_p), ("xlo", c_void_p), ("sxp", c_long), ("xslot", c_void_p),
                ("in_scale", c_void_p), ("in_shift", c_void_p), ("spec_out", c_void_p),
                ("spec", c_void_p), ("bias", c_void_p), ("y", c_void_p), ("mcut", c_void_p), ("out_absmax", c_void_p),
                ("ride_weight", c_void_p), ("ride_o", c_int), ("ride_i", c_int), ("ride_order", c_int), ("ride_scale", c_float),
                ("ride_dst", c_void_p), ("ride_dst_alone", c_void_p)]


class DhconvRoute(ctypes.Structure):
    """struct ace_dhconv_route"""
    _fields_ = [("storage", c_int), ("kspan", c_int), ("units", c_int * 3), ("max_chunks", c_int), ("units_per_xcd", c_int)]


class DhconvDesc(ctypes.Structure):
    """struct ace_dhconv_desc"""
    _fields_ = [("coeffs", c_void_p), ("weight", c_void_p), ("out", c_void_p), ("out_absmax", c_void_p),
                ("n", c_int), ("c", c_int), ("L", c_int), ("Mm", c_int), ("groups", c_int), ("storage", c_int),
                ("e_fill", c_float)]


# every symbol include/ace_sfno.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "ace_last_error": (c_char_p, []),
    "ace_version": (c_int, []),
    "ace_sht_plan_create": (c_int, [c_int, c_int, c_int, c_int, c_char_p, POINTER(c_void_p)]),
    "ace_sht_plan_create_ex": (c_int, [c_int, c_int, c_int, c_int, c_char_p, c_int, POINTER(c_void_p)]),
    "ace_sht_plan_destroy": (None, [c_void_p]),
    "ace_sht_plan_dims": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "ace_sht_plan_route": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "ace_sht_plan_cut": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int)]),
    "ace_sht_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ace_sht_inverse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ace_sht_tables_host": (c_int, [c_int, c_int, c_int, c_int, c_char_p, c_int, c_void_p]),
    "ace_conv1x1": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_int, c_void_p]),
    "ace_conv1x1_f16x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_int, c_void_p]),
    "ace_conv1x1_fused": (c_int, [POINTER(Conv1x1FusedDesc), POINTER(GemmRoute), c_void_p]),
    "ace_dft_stage": (c_int, [c_void_p, POINTER(DftStageDesc), POINTER(DftRoute), c_void_p]),
    "ace_mlp_f16x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_long, c_int, c_void_p]),
    "ace_dhconv_f16x3": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ace_dhconv_strip_op": (c_int, [POINTER(DhconvDesc), POINTER(DhconvRoute), c_void_p]),
    "ace_instance_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_long, c_void_p]),
    "ace_conditional_layer_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                           c_int, c_int, c_int, c_long, c_void_p]),
    "ace_conditional_layer_norm_f16x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                                 c_int, c_int, c_int, c_long, c_void_p]),
    "ace_sfno_create": (c_int, [POINTER(AceSfnoConfig), POINTER(c_void_p)]),
    "ace_sfno_destroy": (None, [c_void_p]),
    "ace_sfno_set_weight": (c_int, [c_void_p, c_char_p, c_void_p, c_long, c_void_p]),
    "ace_sfno_weights_generation": (c_long, [c_void_p]),
    "ace_sfno_workspace_size": (c_long, [c_void_p, c_int]),
    "ace_sfno_num_weights": (c_int, [c_void_p]),
    "ace_sfno_weight_name": (c_char_p, [c_void_p, c_int]),
    "ace_sfno_weight_numel": (c_long, [c_void_p, c_int]),
    "ace_sfno_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ace_sfno_forward_conditioned": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ace_sfno_forward_conditioned_timed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "ace_sfno_sht_route": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "ace_sfno_sht_cut": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int)]),
    "ace_sfno_norm_affine": (c_int, [c_void_p, c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "ace_sfno_num_stages": (c_int, []),
    "ace_sfno_stage_name": (c_char_p, [c_int]),
    "ace_sfno_forward_timed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, POINTER(c_float), POINTER(c_int)]),
    "ace_sfno_set_taps": (c_int, [c_void_p, c_int]),
    "ace_sfno_get_tap": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "ace_sfno_forward_graph": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ace_pack_normalize": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p]),
    "ace_unpack_denormalize": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p]),
    "ace_hpx_last_error": (c_char_p, []),
    "ace_hpx_pad_table_host": (c_int, [c_int, c_int, c_void_p, c_void_p]),
    "ace_hpx_pad": (c_int, [c_void_p, c_long, c_long, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                            c_void_p, c_void_p]),
    "ace_hpx_absmax": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "ace_hpx_weight_create": (c_int, [c_void_p, c_int, c_int, c_void_p, POINTER(c_void_p)]),
    "ace_hpx_weight_destroy": (None, [c_void_p]),
    # x, x2, cin, cin2, w, row_off, bias, R, y, imgs, cout, H, W, pitch, k, dil, act, cap, xmax, x2max, ymax, stream
    "ace_hpx_conv": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ace_hpx_pad_planes": (c_int, [c_void_p, c_long, c_long, c_int, c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ace_hpx_conv_packed": (c_int, [c_void_p, c_void_p, c_int, c_long, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_long, c_int,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "ace_hpx_halo_planes": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ace_hpx_conv1_packed": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p, c_void_p]),
    "ace_hpx_pool2": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_long, c_int, c_long, c_int, c_void_p]),
    "ace_hpx_upsample2": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_long, c_int, c_long, c_int, c_int, c_void_p]),
    # x, w, bias, tmp, y, imgs, cin, cout, H, W, pitch_in, pitch_out, plane_stride_out, act, cap, xmax, ymax, stream
    "ace_hpx_tconv2": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_long,
                               c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "ace_ll_last_error": (c_char_p, []),
    # x, x_img_stride, x_chan_stride, x_pitch, c, H, W, p, circular, hi, lo, pitch_p, imgs, ss, ss_img_stride, act, cap, xmax, bscale, boff,
    # pmax, stream
    "ace_ll_pad_planes": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                  c_void_p, c_long, c_int, c_float, c_void_p, c_float, c_float, c_void_p, c_void_p]),
    # x, img_stride, chan_stride, pitch, imgs, c, H, W, eps, gamma, beta, ss, mean_var, amax, stream
    "ace_ll_norm_stats": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "ace_ll_pool2": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_long, c_int, c_long, c_void_p, c_void_p]),
    # x, planes, h, w, pitch_x, plane_stride_x, skip, pitch_skip, plane_stride_skip, y, H, W, pitch_y, plane_stride_y, circular, periodic,
    # amax, stream
    "ace_ll_upsample2_add": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_long, c_void_p, c_int, c_long, c_void_p, c_int, c_int, c_int,
                                     c_long, c_int, c_int, c_void_p, c_void_p]),
    "ace_physics_last_error": (c_char_p, []),
    "ace_physics_create": (c_int, [POINTER(PhysConfig), c_void_p, c_void_p, c_void_p, POINTER(c_void_p)]),
    "ace_physics_destroy": (None, [c_void_p]),
    "ace_physics_reset": (c_int, [c_void_p, c_void_p]),
    "ace_physics_set_reference": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "ace_physics_get_reference": (c_int, [c_void_p, c_void_p, POINTER(c_int), c_int, c_void_p]),
    "ace_physics_apply": (c_int, [c_void_p, POINTER(PhysFields), c_int, c_void_p]),
    "ace_ocean_phys_last_error": (c_char_p, []),
    "ace_ocean_phys_create": (c_int, [POINTER(OceanConfig), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p)]),
    "ace_ocean_phys_destroy": (None, [c_void_p]),
    "ace_ocean_phys_apply": (c_int, [c_void_p, POINTER(OceanFields), c_int, c_void_p]),
    "ace_ocean_phys_launches": (c_int, [c_void_p, POINTER(c_long), POINTER(c_long)]),
    "ace_ocean_derive_last_error": (c_char_p, []),
    "ace_ocean_derive_window": (c_int, [POINTER(OceanDeriveDesc), c_void_p]),
    "ace_ice_budget_last_error": (c_char_p, []),
    "ace_ice_budget_scratch_bytes": (c_long, [c_int, c_long]),
    # fields, timestep, batch, H, W, scratch, stream
    "ace_ice_budget_apply": (c_int, [POINTER(IceFields), c_double, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ace_ice_budget_launches": (c_int, [POINTER(c_long), POINTER(c_long), POINTER(c_long)]),
    "ace_mask_last_error": (c_char_p, []),
    # srcs, src_strides, dsts, dst_strides, mask_idx, hits, nmask, fill, nplanes, batch, hw, stream
    "ace_mask_planes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_long,
                                c_void_p]),
    # srcs, src_strides, mask_idx, hits, nmask, fill, stage, stage_strides, mean, std, dst, npack, nplanes, batch, hw, stream
    "ace_mask_pack_normalize": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_int, c_int, c_int, c_long, c_void_p]),
    "ace_pixel_mlp_last_error": (c_char_p, []),
    # n_layers, dims, w_dev, bias_dev, act, embed_layer, stream, handle
    "ace_pixel_mlp_create": (c_int, [c_int, POINTER(c_int), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int), c_int, c_void_p,
                                     POINTER(c_void_p)]),
    "ace_pixel_mlp_destroy": (None, [c_void_p]),
    # handle, x, embed, y, batch, hw, stream
    "ace_pixel_mlp_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_void_p]),
    # ... embed_layer, embed_before_act, stream, handle
    "ace_pixel_mlp_create2": (c_int, [c_int, POINTER(c_int), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int), c_int, c_int, c_void_p,
                                      POINTER(c_void_p)]),
    "ace_disco_last_error": (c_char_p, []),
    # H, W, K, row_off (host), hi (host), wi (host), vals (host), w_dev, in_chans, out_chans, groups, act, has_embed, stream, handle
    "ace_disco_create": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                 c_int, c_void_p, POINTER(c_void_p)]),
    "ace_disco_destroy": (None, [c_void_p]),
    # handle, x, embed, y, batch, stream
    "ace_disco_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ace_disco_info": (c_int, [c_void_p, POINTER(c_long)]),
    "ace_gmr_chunks": (c_long, [c_long]),
    # srcs, strides, plane_idx, nsrc, partials, batch, K, hw, stream
    "ace_gmr_partials": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_long, c_void_p]),
    # srcs, strides, plane_idx, nsrc, partials, means, batch, K, hw, stream
    "ace_gmr_sample_means": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p]),
    # srcs, strides, mean, std, shift_idx, partials, clim_mean, extra_idx, extra_std, dst, shift, batch, nin, nextra, K, hw, stream
    "ace_gmr_pack_normalize": (c_int, [c_void_p] * 11 + [c_int] * 4 + [c_long, c_void_p]),
    # src, mean, std, dsts, strides, shift_idx, shift, batch, nch, K, hw, stream
    "ace_gmr_unpack_denormalize": (c_int, [c_void_p] * 7 + [c_int] * 3 + [c_long, c_void_p]),
    "ace_couple_last_error": (c_char_p, []),
    # srcs, src_strides, dsts, dst_strides, masks, npass, mode, interpolate, n_inner, batch, hw, stream
    "ace_couple_ocean_to_atmosphere": (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_long, c_void_p]),
    "ace_couple_ocean_to_atmosphere_window": (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_long, c_void_p]),      # the same arguments
    # srcs, src_strides, dsts, dst_strides, slot, nnames, n_inner, batch, hw, stream
    "ace_couple_atmosphere_to_ocean": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_long, c_void_p]),
    "ace_diag_last_error": (c_char_p, []),
    "ace_diag_partial_doubles": (c_long, [c_int, c_int, c_int, c_long]),
    # srcs, strides, rows, wrows, weights, nw, partial, tsum, series, nrows, n_time, t0, t_begin, do_tsum, nplanes, batch, steps,
    # hw, stream
    "ace_diag_window": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                c_int, c_int, c_int, c_int, c_int, c_int, c_long, c_void_p]),
    # coeffs, rows, spec, nrows, nnames, planes, lmax, mmax, stream
    "ace_diag_spectrum": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_long, c_int, c_int, c_void_p]),
    "ace_diag_paired_partial_doubles": (c_long, [c_int, c_int, c_int, c_int, c_int]),
    # gen, gen_strides, target, target_strides, rows, wrows, weights, nw, partial, tsum, zonal, series, nrows, n_time, t0, t_begin,
    # do_maps, zt0, factor, nslots, nplanes, batch, steps, nlat, nlon, stream
    "ace_diag_paired_window": (c_int, [c_void_p] * 7 + [c_int] + [c_void_p] * 4 + [c_int] * 13 + [c_void_p]),
    "ace_diag_hist_scratch_bytes": (c_long, [c_int, c_int, c_int, c_long]),
    # gen, gen_strides, target, target_strides, rows, masks, scratch, range, counts, dropped, nrows, n_bins, nplanes, batch, steps,
    # hw, stream
    "ace_diag_hist_window": (c_int, [c_void_p] * 10 + [c_int] * 5 + [c_long, c_void_p]),
    "ace_diag_regress_partial_doubles": (c_long, [c_int, c_int, c_int, c_long]),
    # gen, gen_strides, target, target_strides, rows, coef, slot, maps, eps, wrows, weights, nw, partial, below_count, below_frac,
    # nrows, nterms, nmaps, t_begin, nplanes, batch, steps, hw, stream
    "ace_diag_regress_window": (c_int, [c_void_p] * 11 + [c_int] + [c_void_p] * 3 + [c_int] * 7 + [c_long, c_void_p]),
    "ace_diag_calendar_partial_doubles": (c_long, [c_int, c_int, c_int, c_int, c_long]),
    # gen, gen_strides, target, target_strides, rows, bin, bins, regions, srow, mode, wrows, weights, nw, partial, series, nrows,
    # nbins, nreg, nsrows, n_time, t0, t_begin, nplanes, batch, steps, hw, stream
    "ace_diag_calendar_window": (c_int, [c_void_p] * 12 + [c_int] + [c_void_p] * 2 + [c_int] * 10 + [c_long, c_void_p]),
    # gen, gen_strides, target, target_strides, rows, maps, seen, nrows, slot, nslots, pair_weight, t, nplanes, n_ic, n_members, steps,
    # hw, stream
    "ace_diag_ensemble_step": (c_int, [c_void_p] * 7 + [c_int] * 3 + [c_double] + [c_int] * 5 + [c_long, c_void_p]),
    "ace_diag_fill_scratch_doubles": (c_long, [c_int, c_int, c_int, c_int, c_int]),
    # srcs, strides, tab, layers, blurred, nmasks, scratch, dst, nnames, batch, steps, nlat, nlon, stream
    "ace_diag_fill_planes": (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 2 + [c_int] * 5 + [c_void_p]),
    # srcs, strides, rows, edges, sums, means, nrows, nseg, nplanes, batch, steps, hw, stream
    "ace_diag_time_segments": (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_long, c_void_p]),
    # srcs, strides, rows, bounds, sums, means, nrows, nseg, nplanes, batch, steps, nlat, nlon, lat0, nlat_r, lon0, nlon_r, stream
    "ace_diag_region_segments": (c_int, [c_void_p] * 6 + [c_int] * 11 + [c_void_p]),
    # gen, gen_strides, target, target_strides, rows, mean, sq, err, nrows, n_time, t0, assign, nplanes, batch, steps, hw, stream
    "ace_diag_video_window": (c_int, [c_void_p] * 8 + [c_int] * 7 + [c_long, c_void_p]),
    # srcs, src_strides, dsts, dst_strides, nplanes, batch, hw, stream
    "ace_stepdiag_snapshot": (c_int, [c_void_p] * 4 + [c_int] * 2 + [c_long, c_void_p]),
    # outs, out_strides, snaps, snap_strides, nplanes, batch, steps, hw, stream
    "ace_stepdiag_delta_window": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_long, c_void_p]),
    "ace_diag_correction_partial_doubles": (c_long, [c_int, c_int, c_int, c_long]),
    # deltas, strides, stds, rows, wrows, weights, nw, partial, signed_sum, magnitude_sum, series, nrows, n_time, t0, nplanes, batch,
    # steps, hw, stream
    "ace_diag_correction_window": (c_int, [c_void_p] * 6 + [c_int] + [c_void_p] * 4 + [c_int] * 6 + [c_long, c_void_p]),
}

_lib = None
TEST_INSTRUMENTATION = ("ace_sht_plan_route", "ace_sht_plan_cut", "ace_sfno_sht_route", "ace_sfno_sht_cut", "ace_sfno_norm_affine", "ace_ocean_phys_launches")   # queries of the parity tests, not used by the product path


class AceLibraryMissing(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """The loaded library; raises AceLibraryMissing if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AceLibraryMissing(
                f"{LIB_PATH} not found: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `python -m ace_amd.build`). "
                "ace_amd has no CPU fallback."
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if name in TEST_INSTRUMENTATION and os.environ.get("ACE_SFNO_LIB") and not hasattr(handle, name):
                continue   # a variant build of an older round (same-box A/Bs through ACE_SFNO_LIB) may predate the route queries
            fn = getattr(handle, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def check(rc: int, family: str = None) -> None:
    """Map the C status to the exception the reference would raise at this boundary.  The message is read through the getter of
    the call's family (``ace_<family>_last_error``; None: ``ace_last_error``), looked up on ``lib()`` now: the library answers
    every getter from one string, an emulation standing in for ``lib()`` in a test has its own family's getter only."""
    if rc == ACE_OK:
        return
    msg = getattr(lib(), f"ace_{family}_last_error" if family else "ace_last_error")().decode()
    if rc == ACE_ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


def ptr(t) -> int:
    """Device pointer of a contiguous CUDA/HIP float32 tensor (or None)."""
    if t is None:
        return None
    import torch

    if not t.is_cuda:
        raise RuntimeError("ace_amd kernels need tensors on an MI355X (got a CPU tensor); there is no CPU fallback")
    if t.dtype != torch.float32 and t.dtype != torch.complex64:
        raise TypeError(f"expected float32/complex64 tensor, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")
    return t.data_ptr()


@contextlib.contextmanager
def capture_without_gc():
    """Around a ``torch.cuda.graph`` capture: collect the dead Python cycles first and keep the collector off until the capture
    ends.  ``torch.cuda.graph`` no longer collects on entry, and a cycle that dies inside the capture may own device resources whose
    release (a ``hipFree`` behind a native handle's ``__del__``, the graph of an engine no longer in use) invalidates the capture:
    the next launch then fails with hipErrorStreamCaptureInvalidated.  When the collector runs depends on the allocation count,
    i.e. on unrelated host code."""
    import gc
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def current_stream() -> int:
    import torch

    return torch.cuda.current_stream().cuda_stream
