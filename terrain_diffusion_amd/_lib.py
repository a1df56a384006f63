"""ctypes binding of libtd_engine.so (C-ABI declared in include/td_engine.h).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible, calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


class TdError(RuntimeError):
    pass


class Library:
    """One ctypes library of the package: loaded on first use, with restype / argtypes set for every entry of `sigs` ({name: (restype, argtypes)};
    a name the library lacks raises AttributeError).  `last_error` names its const char* f(void) entry point, `label` is what messages call it."""

    def __init__(self, file_name, sigs, last_error, label, missing="There is no CPU fallback."):
        self.path = os.path.join(_HERE, file_name)
        self.sigs, self.last_error, self.label, self.missing = sigs, last_error, label, missing
        self.handle = None

    def lib(self):
        """The loaded library; raises if it has not been built."""
        if self.handle is None:
            if not os.path.exists(self.path):
                raise TdError(f"{self.path} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()'). {self.missing}")
            l = C.CDLL(self.path)
            for name, (res, args) in self.sigs.items():
                fn = getattr(l, name)
                fn.restype = res
                fn.argtypes = args
            self.handle = l
        return self.handle

    def error_text(self):
        return getattr(self.lib(), self.last_error)().decode()

    def check(self, rc):
        if rc != 0:
            raise TdError(f"{self.label} error {rc}: {self.error_text()}")


class UnetConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("in_channels", C.c_int32), ("out_channels", C.c_int32),
                ("model_channels", C.c_int32), ("n_levels", C.c_int32), ("channel_mults", C.c_int32 * 8),
                ("layers_per_block", C.c_int32 * 8), ("n_attn_resolutions", C.c_int32),
                ("attn_resolutions", C.c_int32 * 8), ("midblock_attention", C.c_int32), ("concat_balance", C.c_float),
                ("noise_emb_dims", C.c_int32), ("emb_channels", C.c_int32), ("n_cond", C.c_int32),
                ("cond_type", C.c_int32 * 8), ("cond_dims", C.c_int32 * 8), ("cond_weights", C.c_float * 8)]


class AeConfig(C.Structure):
    """td_ae_config (include/td_ae.h): the EDMAutoencoder constructor arguments that shape its two graphs"""
    _fields_ = [("image_size", C.c_int32), ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("model_channels", C.c_int32), ("n_levels", C.c_int32),
                ("channel_mults", C.c_int32 * 8), ("layers_per_block", C.c_int32 * 8), ("layers_per_block_decoder", C.c_int32 * 8),
                ("n_attn_resolutions", C.c_int32), ("attn_resolutions", C.c_int32 * 8), ("midblock_attention", C.c_int32), ("latent_channels", C.c_int32),
                ("n_direct_skips", C.c_int32), ("direct_skips", C.c_int32 * 8)]


_P = C.c_void_p


class GridBatch(C.Structure):
    """td_grid_batch (include/td_engine.h): one window batch of the tiled sampler for td_sample_grid_batch"""
    _fields_ = [("noise_seed", C.c_uint64), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("tile_h", C.c_int32), ("tile_w", C.c_int32),
                ("noise_scale", C.c_float), ("origins_host", _P), ("cond_rows", _P), ("cond_grid", _P), ("grid_rows", C.c_int32), ("grid_cols", C.c_int32),
                ("cond_pos_host", _P), ("cond_means_host", _P), ("cond_stds_host", _P), ("hist_host", _P), ("n_hist", C.c_int32), ("noise_level", C.c_float),
                ("n_steps", C.c_int32), ("sigma_data", C.c_float), ("sigmas_host", _P), ("canvas", _P), ("Hc", C.c_int32), ("Wc", C.c_int32),
                ("size", C.c_int32), ("n_rows", C.c_int32), ("n_cols", C.c_int32), ("accumulate", C.c_int32), ("row_starts_host", _P),
                ("col_starts_host", _P), ("wi_host", _P), ("wj_host", _P), ("windows_out", _P)]


class EdmExt(C.Structure):
    """td_edm_ext (include/td_engine.h): the arguments of td_sample_edm_ext"""
    _fields_ = [("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_steps", C.c_int32), ("sigmas_host", _P), ("sigma_data", C.c_float), ("cond", _P),
                ("x", _P), ("cond_img", _P), ("cimg_channels", C.c_int32), ("guide", _P), ("guidance_scale", C.c_float), ("score_scaling", C.c_float),
                ("score_cs_host", _P)]


_SIGS = {
    "td_last_error": (C.c_char_p, []),
    "td_version": (C.c_int, []),
    "td_build_id": (C.c_char_p, []),
    "td_engine_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "td_engine_destroy": (None, [_P]),
    "td_engine_synchronize": (C.c_int, [_P]),
    "td_engine_stream": (_P, [_P]),
    "td_engine_set_stream": (C.c_int, [_P, _P]),
    "td_engine_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "td_engine_get_option": (C.c_int64, [_P, C.c_char_p, C.c_int64]),
    "td_engine_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "td_engine_profile_read_glds": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "td_engine_profile_dump": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "td_unet_create": (C.c_int, [_P, C.POINTER(UnetConfig), C.c_int, C.POINTER(_P)]),
    "td_unet_destroy": (None, [_P]),
    "td_unet_num_params": (C.c_int, [_P]),
    "td_unet_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64 * 4)]),
    "td_unet_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "td_unet_set_prefolded": (C.c_int, [_P, C.c_int]),
    "td_unet_finalize": (C.c_int, [_P]),
    "td_unet_cond_row_len": (C.c_int, [_P]),
    "td_unet_forward": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "td_unet_read_activation": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int32 * 4)]),
    "td_dpm_coefs": (C.c_int, [_P, C.c_int, C.c_float, C.c_int, C.c_int, _P]),
    "td_tile_seed": (C.c_uint64, [C.c_uint64, C.c_int64, C.c_int64]),
    "td_standard_normal": (C.c_int, [_P, C.c_uint64, C.c_int64, _P]),
    "td_noise_patches": (C.c_int, [_P, C.c_uint64, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "td_cond_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_float, _P]),
    "td_sample_grid_batch": (C.c_int, [_P, C.POINTER(GridBatch)]),
    "td_sample_edm": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_float, _P, _P]),
    "td_sample_edm_guided": (C.c_int, [_P, _P, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_float, _P, _P]),
    "td_sample_consistency": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P]),
    "td_sample_edm_img": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_float, _P, _P, C.c_int, _P]),
    "td_sample_edm_ext": (C.c_int, [_P, C.POINTER(EdmExt)]),
    "td_sample_consistency_img": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, C.c_int, _P]),
    "td_blend_windows": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int]),
    "td_blend_windows_w": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "td_gather_regions": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "td_blend_normalize": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "td_linear_weight_window": (C.c_int, [_P, C.c_int, _P]),
    "td_attention": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "td_perlin_map": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, _P, _P, C.c_int, _P]),
    "td_resample2d": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, C.c_int, _P]),
    "td_residual_plus": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_float, _P]),
    "td_elev_finish": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P]),
    "td_ddim_cfg_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, _P]),
    "td_climate_finish": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _P]),
}
EXPORTS = tuple(_SIGS)

_LIB = Library("libtd_engine.so", _SIGS, "td_last_error", "td_engine")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

# the autoencoder entry points of the same library, declared in include/td_ae.h (EXPORTS stays the list of include/td_engine.h's own declarations)
_AE_SIGS = {
    "td_last_error": (C.c_char_p, []),
    "td_ae_create": (C.c_int, [_P, C.POINTER(AeConfig), C.c_int, C.POINTER(_P)]),
    "td_ae_destroy": (None, [_P]),
    "td_ae_num_params": (C.c_int, [_P]),
    "td_ae_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64 * 4)]),
    "td_ae_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "td_ae_set_prefolded": (C.c_int, [_P, C.c_int]),
    "td_ae_finalize": (C.c_int, [_P]),
    "td_ae_preencode": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_float, C.c_int, _P, _P, _P]),
    "td_ae_postencode": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P]),
    "td_ae_decode": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_float, _P]),
    "td_ae_read_activation": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int32 * 4)]),
}
AE_EXPORTS = tuple(k for k in _AE_SIGS if k.startswith("td_ae_"))
_AE_LIB = Library("libtd_engine.so", _AE_SIGS, "td_last_error", "td_engine")
ae_lib, ae_check = _AE_LIB.lib, _AE_LIB.check
