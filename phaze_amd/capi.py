"""ctypes binding of include/phaze_amd.h (the same entry points the N-API addon binds).

Mirrors the reference surface: `PhaseVocoder.process(inputs, outputs, parameters)` has the argument
meaning of OLAProcessor.process (/root/reference/src/ola-processor.js:159-171).  There is NO fallback:
if libphaze_amd.so cannot be loaded, or no HIP device exists, construction raises.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("PHAZE_LIB") or os.path.join(_HERE, "lib", "libphaze_amd.so")   # PHAZE_LIB: A/B builds of the same ABI
_lib = None

PV_OK, PV_ERR_FFT_SIZE, PV_ERR_ARGUMENT, PV_ERR_UNSUPPORTED, PV_ERR_CAPACITY, PV_ERR_DEVICE, PV_ERR_DESTROYED = range(7)

EXPORTS = [
    "pv_create", "pv_destroy", "pv_last_error", "pv_status_string", "pv_get_info", "pv_reset", "pv_reset_channels",
    "pv_get_time_cursor", "pv_set_time_cursor", "pv_process", "pv_process_batch", "pv_process_batch_device",
    "pv_set_stream", "pv_synchronize", "pv_debug_frame", "pv_export_state", "pv_import_state", "pv_abi_version",
    "pv_process_begin", "pv_process_end", "pv_device_count", "pv_host_alloc", "pv_host_free", "pv_reset_channels_part",
    "pv_forward_stats",
    "pv_stretch_create", "pv_stretch_destroy", "pv_stretch_reset", "pv_stretch_last_error", "pv_stretch_process", "pv_stretch_process_device",
    "pv_stretch_set_stream", "pv_stretch_synchronize", "pv_stretch_export_state", "pv_stretch_import_state",
    "pv_tempo_process", "pv_tempo_process_device",
    "pv_link_channels",
    "pv_transient_process", "pv_transient_process_device", "pv_onset_strength", "pv_onset_strength_device", "pv_transient_plan",
    "pv_onsets_from_strength", "pv_transient_chain_layout", "pv_onset_chain_layout",
    "pv_resample_create", "pv_resample_destroy", "pv_resample_reset", "pv_resample_last_error", "pv_resample_set_stream", "pv_resample_synchronize",
    "pv_resample_process", "pv_resample_process_device", "pv_resample_out_count", "pv_resample_export_state", "pv_resample_import_state",
    "pv_resample_design", "pv_resample_count",
    "pv_pitch_create", "pv_pitch_destroy", "pv_pitch_reset", "pv_pitch_last_error", "pv_pitch_set_stream", "pv_pitch_synchronize",
    "pv_pitch_process", "pv_pitch_process_device", "pv_pitch_stretch", "pv_pitch_resampler",
    "pv_vari_create", "pv_vari_destroy", "pv_vari_reset", "pv_vari_last_error", "pv_vari_set_stream", "pv_vari_synchronize",
    "pv_vari_process", "pv_vari_process_device", "pv_vari_export_state", "pv_vari_import_state", "pv_vari_prototype", "pv_vari_half_width",
    "pv_glide_create", "pv_glide_destroy", "pv_glide_reset", "pv_glide_last_error", "pv_glide_set_stream", "pv_glide_synchronize",
    "pv_glide_process", "pv_glide_process_device", "pv_glide_stretch", "pv_glide_resampler",
    "pv_f0_create", "pv_f0_destroy", "pv_f0_last_error", "pv_f0_set_stream", "pv_f0_synchronize", "pv_f0_track", "pv_f0_track_device", "pv_f0_period",
    "pv_tune_plan",
    "pv_psola_create", "pv_psola_destroy", "pv_psola_last_error", "pv_psola_set_stream", "pv_psola_synchronize", "pv_psola_process",
    "pv_psola_process_device", "pv_psola_window", "pv_psola_ratios", "pv_psola_plan",
    "pv_epoch_create", "pv_epoch_destroy", "pv_epoch_last_error", "pv_epoch_set_stream", "pv_epoch_synchronize", "pv_epoch_track", "pv_epoch_track_device",
    "pv_epoch_periods", "pv_epoch_plan",
    "pv_tsm_create", "pv_tsm_destroy", "pv_tsm_last_error", "pv_tsm_set_stream", "pv_tsm_synchronize", "pv_tsm_process", "pv_tsm_process_device", "pv_tsm_plan",
    "pv_harmony_create", "pv_harmony_destroy", "pv_harmony_last_error", "pv_harmony_set_stream", "pv_harmony_synchronize", "pv_harmony_process",
    "pv_harmony_process_device", "pv_harmony_ratios",
    "pv_takes_create", "pv_takes_destroy", "pv_takes_last_error", "pv_takes_set_stream", "pv_takes_synchronize", "pv_takes_process", "pv_takes_process_device",
    "pv_takes_tiles",
    "pv_mirror_create", "pv_mirror_destroy", "pv_mirror_last_error", "pv_mirror_set_stream", "pv_mirror_synchronize", "pv_mirror_process",
    "pv_mirror_process_device", "pv_mirror_plan",
    "pv_formant_create", "pv_formant_destroy", "pv_formant_last_error", "pv_formant_set_stream", "pv_formant_synchronize", "pv_formant_process",
    "pv_formant_process_device", "pv_formant_plan",
    "pv_contour_create", "pv_contour_destroy", "pv_contour_last_error", "pv_contour_set_stream", "pv_contour_synchronize", "pv_contour_track",
    "pv_contour_track_device", "pv_contour_path",
    "pv_choir_create", "pv_choir_destroy", "pv_choir_last_error", "pv_choir_set_stream", "pv_choir_synchronize", "pv_choir_process", "pv_choir_process_device",
    "pv_choir_plan",
]


class PvError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


class _Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "fft_size", "hop_size", "max_channels", "max_hops", "device_id", "frames_per_chunk", "flags")]


class _StretchConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "fft_size", "analysis_hop", "synthesis_hop", "max_channels", "max_frames", "device_id", "flags")]


class _ResampleConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "up", "down", "max_channels", "max_samples", "device_id", "flags")]


class _PitchConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "fft_size", "analysis_hop", "synthesis_hop", "up", "down", "max_channels", "max_frames", "device_id",
                                          "flags")]


class _VariConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "block", "min_count", "max_count", "max_channels", "max_blocks", "device_id", "flags")]


class _GlideConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "fft_size", "synthesis_hop", "min_hop", "max_hop", "max_channels", "max_frames", "device_id", "flags")]


class _F0Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "window", "hop", "min_lag", "max_lag", "max_channels", "max_frames", "device_id", "flags")]


class _ContourConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "window", "hop", "min_lag", "max_lag", "candidates", "max_channels", "max_frames", "device_id", "flags")]


class _ContourParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "candidates", "max_lag", "bias", "unvoiced_cost", "voicing_cost", "jump_cost", "reserved")]


class _TuneParams(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("struct_size", "f0_hop", "f0_center", "scale_mask", "synthesis_hop", "min_hop", "max_hop", "reserved")]
                + [(n, C.c_double) for n in ("sample_rate", "a4", "strength", "retune")] + [(n, C.c_int64) for n in ("input_len", "shift")])


class _PsolaConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_period", "max_channels", "max_outputs", "device_id", "flags")]


class _PsolaParams(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("struct_size", "f0_hop", "f0_center", "min_period", "max_period", "reserved")]
                + [("unvoiced_period", C.c_double), ("input_len", C.c_int64)])


class _EpochConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "window", "hop", "max_period", "max_channels", "max_frames", "device_id", "flags")]


class _EpochParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("min_strength", C.c_int32), ("lock", C.c_double)]


class _TsmConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_period", "max_rate", "max_channels", "max_outputs", "device_id", "flags")]


class _HarmonyConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_period", "max_rate", "max_voices", "max_channels", "max_outputs", "device_id", "flags")]


class _TakesConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_period", "max_rate", "max_channels", "max_outputs", "device_id", "flags")]


class _MirrorConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_period", "max_rate", "max_channels", "max_outputs", "device_id", "flags")]


def make_mirror_config(max_period, max_rate=1, max_channels=1, max_outputs=0, device_id=0, flags=0):
    """pv_mirror_config with struct_size filled in (the C side's PV_MIRROR_CONFIG_INIT)."""
    return _MirrorConfig(C.sizeof(_MirrorConfig), max_period, max_rate, max_channels, max_outputs, device_id, flags)


class _FormantConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_period", "max_rate", "max_channels", "max_outputs", "device_id", "flags")]


def make_formant_config(max_period, max_rate=1, max_channels=1, max_outputs=0, device_id=0, flags=0):
    """pv_formant_config with struct_size filled in (the C side's PV_FORMANT_CONFIG_INIT)."""
    return _FormantConfig(C.sizeof(_FormantConfig), max_period, max_rate, max_channels, max_outputs, device_id, flags)


class _ChoirConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_period", "max_rate", "max_voices", "max_channels", "max_outputs", "device_id", "flags")]


def make_choir_config(max_period, max_rate=1, max_voices=0, max_channels=1, max_outputs=0, device_id=0, flags=0):
    """pv_choir_config with struct_size filled in (the C side's PV_CHOIR_CONFIG_INIT)."""
    return _ChoirConfig(C.sizeof(_ChoirConfig), max_period, max_rate, max_voices, max_channels, max_outputs, device_id, flags)


class _Take(C.Structure):
    """pv_take: in and out are addresses (host or device, as the entry point says)."""
    _fields_ = [("in_", C.c_void_p), ("nin", C.c_int64), ("in_stride", C.c_int64), ("grains", C.POINTER(C.c_int32)), ("ngrains", C.c_int64), ("out", C.c_void_p),
                ("out_first", C.c_int64), ("nout", C.c_int64), ("out_stride", C.c_int64)]


def make_takes_config(max_period, max_rate=1, max_channels=1, max_outputs=0, device_id=0, flags=0):
    """pv_takes_config with struct_size filled in (the C side's PV_TAKES_CONFIG_INIT)."""
    return _TakesConfig(C.sizeof(_TakesConfig), max_period, max_rate, max_channels, max_outputs, device_id, flags)


def make_harmony_config(max_period, max_rate=1, max_voices=0, max_channels=1, max_outputs=0, device_id=0, flags=0):
    """pv_harmony_config with struct_size filled in (the C side's PV_HARMONY_CONFIG_INIT)."""
    return _HarmonyConfig(C.sizeof(_HarmonyConfig), max_period, max_rate, max_voices, max_channels, max_outputs, device_id, flags)


def make_tsm_config(max_period, max_rate=1, max_channels=1, max_outputs=0, device_id=0, flags=0):
    """pv_tsm_config with struct_size filled in (the C side's PV_TSM_CONFIG_INIT)."""
    return _TsmConfig(C.sizeof(_TsmConfig), max_period, max_rate, max_channels, max_outputs, device_id, flags)


def make_epoch_config(window, hop, max_period, max_channels=1, max_frames=0, device_id=0, flags=0):
    """pv_epoch_config with struct_size filled in (the C side's PV_EPOCH_CONFIG_INIT)."""
    return _EpochConfig(C.sizeof(_EpochConfig), window, hop, max_period, max_channels, max_frames, device_id, flags)


def make_epoch_params(min_strength=0, lock=0.125):
    """pv_epoch_params with struct_size filled in (the C side's PV_EPOCH_PARAMS_INIT)."""
    return _EpochParams(C.sizeof(_EpochParams), min_strength, lock)


def make_psola_config(max_period, max_channels=1, max_outputs=0, device_id=0, flags=0):
    """pv_psola_config with struct_size filled in (the C side's PV_PSOLA_CONFIG_INIT)."""
    return _PsolaConfig(C.sizeof(_PsolaConfig), max_period, max_channels, max_outputs, device_id, flags)


def make_psola_params(f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period):
    """pv_psola_params with struct_size filled in (the C side's PV_PSOLA_PARAMS_INIT)."""
    return _PsolaParams(C.sizeof(_PsolaParams), f0_hop, f0_center, min_period, max_period, 0, unvoiced_period, input_len)


def make_f0_config(window, hop, min_lag, max_lag, max_channels=1, max_frames=0, device_id=0, flags=0):
    """pv_f0_config with struct_size filled in (the C side's PV_F0_CONFIG_INIT)."""
    return _F0Config(C.sizeof(_F0Config), window, hop, min_lag, max_lag, max_channels, max_frames, device_id, flags)


def make_contour_config(window, hop, min_lag, max_lag, candidates=8, max_channels=1, max_frames=0, device_id=0, flags=0):
    """pv_contour_config with struct_size filled in (the C side's PV_CONTOUR_CONFIG_INIT)."""
    return _ContourConfig(C.sizeof(_ContourConfig), window, hop, min_lag, max_lag, candidates, max_channels, max_frames, device_id, flags)


def make_contour_params(candidates, max_lag, bias=1024, unvoiced_cost=2458, voicing_cost=2458, jump_cost=16384):
    """pv_contour_params with struct_size filled in (the C side's PV_CONTOUR_PARAMS_INIT)."""
    return _ContourParams(C.sizeof(_ContourParams), candidates, max_lag, bias, unvoiced_cost, voicing_cost, jump_cost, 0)


def make_tune_params(f0_hop, f0_center, sample_rate, synthesis_hop, min_hop, max_hop, input_len, scale_mask=0xFFF, strength=1.0, retune=1.0, a4=440.0, shift=0):
    """pv_tune_params with struct_size filled in (the C side's PV_TUNE_PARAMS_INIT)."""
    return _TuneParams(C.sizeof(_TuneParams), f0_hop, f0_center, scale_mask, synthesis_hop, min_hop, max_hop, 0, sample_rate, a4, strength, retune, input_len, shift)


def make_vari_config(block, min_count, max_count, max_channels=1, max_blocks=0, device_id=0, flags=0):
    """pv_vari_config with struct_size filled in (the C side's PV_VARI_CONFIG_INIT)."""
    return _VariConfig(C.sizeof(_VariConfig), block, min_count, max_count, max_channels, max_blocks, device_id, flags)


def make_glide_config(fft_size, synthesis_hop, min_hop, max_hop, max_channels=1, max_frames=1, device_id=0, flags=0):
    """pv_glide_config with struct_size filled in (the C side's PV_GLIDE_CONFIG_INIT)."""
    return _GlideConfig(C.sizeof(_GlideConfig), fft_size, synthesis_hop, min_hop, max_hop, max_channels, max_frames, device_id, flags)


def make_resample_config(up, down, max_channels=1, max_samples=0, device_id=0, flags=0):
    """pv_resample_config with struct_size filled in (the C side's PV_RESAMPLE_CONFIG_INIT)."""
    return _ResampleConfig(C.sizeof(_ResampleConfig), up, down, max_channels, max_samples, device_id, flags)


def make_pitch_config(fft_size, analysis_hop, synthesis_hop, up=0, down=0, max_channels=1, max_frames=1, device_id=0, flags=0):
    """pv_pitch_config with struct_size filled in (the C side's PV_PITCH_CONFIG_INIT)."""
    return _PitchConfig(C.sizeof(_PitchConfig), fft_size, analysis_hop, synthesis_hop, up, down, max_channels, max_frames, device_id, flags)


def make_stretch_config(fft_size, analysis_hop, synthesis_hop, max_channels=1, max_frames=1, device_id=0, flags=0):
    """pv_stretch_config with struct_size filled in (the C side's PV_STRETCH_CONFIG_INIT)."""
    return _StretchConfig(C.sizeof(_StretchConfig), fft_size, analysis_hop, synthesis_hop, max_channels, max_frames, device_id, flags)


def make_config(fft_size, hop_size, max_channels=1, max_hops=1, device_id=0, frames_per_chunk=0, flags=0):
    """pv_config with struct_size filled in (the C side's PV_CONFIG_INIT)."""
    return _Config(C.sizeof(_Config), fft_size, hop_size, max_channels, max_hops, device_id, frames_per_chunk, flags)


ABI_VERSION = 6          # PV_ABI_VERSION of include/phaze_amd.h this binding was written against (checked at load time)


# pv_config.flags (include/phaze_amd.h): explicit A/B switches; the library reads no environment variables
FLAG_GENERIC_KERNEL, FLAG_STREAM_COPY, FLAG_WORKGROUP_KERNEL, FLAG_STREAM_EVENT_WAIT, FLAG_STREAM_PINNED_INPUT, FLAG_PERSISTENT_STREAM = 1, 2, 4, 8, 16, 32
FLAG_TEST_NO_HDP_FLUSH = 64      # test hook (tests/test_gpu_stream_forms.py)
FLAG_HOST_CHANNEL_BOOKKEEPING = 128
FLAG_TEST_FAIL_SECOND_PIECE = 512   # test hook (tests/test_gpu_batch_pipeline.py): a pipelined host-buffer batch fails behind its second piece
FLAG_FP64_FORWARD = 256          # every forward transform in fp64 (the round-4 kernels); default: fp32 first, fp64 only where a peak decision is in doubt
STATE_HISTORY, STATE_ACCUMULATOR = 1, 2


class _Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("fft_size", "hop_size", "overlaps", "max_channels", "max_hops", "threads_per_workgroup",
                                          "lds_bytes_per_workgroup", "frames_per_chunk", "compute_units", "device_id")] + [("device_name", C.c_char * 64),
                                                                                                       ("kernel_name", C.c_char * 32)]


def library_path() -> str:
    return _LIB_PATH


def build_library(force: bool = False) -> str:
    """Compile the gfx950 library in-tree with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    args = ["make", "-C", csrc]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return _LIB_PATH


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels bundle their own libamdhip64; two HIP runtimes in one process cannot both open the GPU ("no ROCm-capable
    # device").  If torch is installed, load it FIRST so that this library binds to the runtime torch already mapped (same SONAME).
    if "torch" not in sys.modules and not os.environ.get("PHAZE_NO_TORCH_PRELOAD"):
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(_LIB_PATH):
        raise PvError(PV_ERR_DEVICE, f"{_LIB_PATH} is missing: build it with phaze_amd.build_library() / __graft_entry__.build(); "
                                     "there is no CPU fallback")
    L = C.CDLL(_LIB_PATH)
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    L.pv_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    L.pv_destroy.argtypes = [vp]
    L.pv_last_error.argtypes = [vp]
    L.pv_last_error.restype = C.c_char_p
    L.pv_status_string.argtypes = [C.c_int]
    L.pv_status_string.restype = C.c_char_p
    L.pv_get_info.argtypes = [vp, C.POINTER(_Info)]
    L.pv_reset.argtypes = [vp]
    L.pv_reset_channels.argtypes = [vp, C.c_int32, C.c_int32]
    L.pv_reset_channels_part.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.pv_get_time_cursor.argtypes = [vp, C.POINTER(C.c_int64)]
    L.pv_set_time_cursor.argtypes = [vp, C.c_int64]
    L.pv_process.argtypes = [vp, C.POINTER(fp), C.POINTER(fp), C.c_int32, C.c_int32, C.c_float]
    L.pv_process_batch.argtypes = [vp, fp, fp, C.c_int32, C.c_int32, C.c_int64, fp, C.c_int32, C.c_int32]
    L.pv_process_batch_device.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, C.c_int32]
    L.pv_set_stream.argtypes = [vp, vp]
    L.pv_synchronize.argtypes = [vp]
    L.pv_debug_frame.argtypes = [vp, C.c_int32, fp, C.c_float, C.POINTER(C.c_double), fp, C.POINTER(C.c_int32), fp]
    L.pv_export_state.argtypes = [vp, C.c_int32, fp, fp, C.POINTER(C.c_int64)]
    L.pv_import_state.argtypes = [vp, C.c_int32, fp, fp, C.c_int64]
    up = C.POINTER(C.c_uint32)
    L.pv_stretch_create.argtypes = [C.POINTER(_StretchConfig), C.POINTER(vp)]
    L.pv_stretch_destroy.argtypes = [vp]
    L.pv_stretch_reset.argtypes = [vp]
    L.pv_stretch_last_error.argtypes = [vp]
    L.pv_stretch_last_error.restype = C.c_char_p
    L.pv_stretch_process.argtypes = [vp, fp, fp, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    L.pv_stretch_process_device.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64]
    L.pv_stretch_set_stream.argtypes = [vp, vp]
    L.pv_stretch_synchronize.argtypes = [vp]
    L.pv_stretch_export_state.argtypes = [vp, C.c_int32, fp, fp, up, up]
    L.pv_stretch_import_state.argtypes = [vp, C.c_int32, fp, fp, up, up]
    ip = C.POINTER(C.c_int32)
    L.pv_tempo_process.argtypes = [vp, fp, fp, C.c_int32, C.c_int32, ip, C.c_int64, C.c_int64, C.c_int64]
    L.pv_tempo_process_device.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, ip, C.c_int64, C.c_int64, C.c_int64]
    L.pv_link_channels.argtypes = [vp, C.c_int32]
    bp, lp = C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    L.pv_transient_process.argtypes = [vp, fp, fp, C.c_int32, C.c_int32, ip, C.c_int64, bp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_transient_process_device.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, ip, C.c_int64, bp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_onset_strength.argtypes = [vp, fp, C.c_int32, C.c_int32, C.c_int64, ip, C.c_int64]
    L.pv_onset_strength_device.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int64]
    L.pv_onsets_from_strength.argtypes = [ip, C.c_int64, C.c_int32, C.c_int32, C.c_double, lp, C.c_int64]
    L.pv_transient_plan.argtypes = [lp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, bp, C.c_int64]
    L.pv_transient_chain_layout.argtypes = [vp, C.c_int32, C.c_int32, ip, ip]
    L.pv_onset_chain_layout.argtypes = [vp, C.c_int32, C.c_int32, ip]
    L.pv_resample_create.argtypes = [C.POINTER(_ResampleConfig), C.POINTER(vp)]
    L.pv_resample_destroy.argtypes = [vp]
    L.pv_resample_reset.argtypes = [vp]
    L.pv_resample_last_error.argtypes = [vp]
    L.pv_resample_set_stream.argtypes = [vp, vp]
    L.pv_resample_synchronize.argtypes = [vp]
    L.pv_resample_process.argtypes = [vp, fp, C.c_int32, C.c_int64, C.c_int64, fp, C.c_int64, C.c_int64, lp]
    L.pv_resample_process_device.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, lp]
    L.pv_resample_out_count.argtypes = [vp, C.c_int64, lp]
    L.pv_resample_export_state.argtypes = [vp, C.c_int32, fp, lp, lp]
    L.pv_resample_import_state.argtypes = [vp, C.c_int32, fp, C.c_int64, C.c_int64]
    L.pv_resample_design.argtypes = [C.c_int32, C.c_int32, fp, C.c_int64, ip, ip, ip]
    L.pv_resample_count.argtypes = [C.c_int32, C.c_int32, C.c_int64]
    L.pv_pitch_create.argtypes = [C.POINTER(_PitchConfig), C.POINTER(vp)]
    L.pv_pitch_destroy.argtypes = [vp]
    L.pv_pitch_reset.argtypes = [vp]
    L.pv_pitch_last_error.argtypes = [vp]
    L.pv_pitch_set_stream.argtypes = [vp, vp]
    L.pv_pitch_synchronize.argtypes = [vp]
    L.pv_pitch_process.argtypes = [vp, fp, fp, C.c_int32, C.c_int32, ip, C.c_int64, bp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, lp]
    L.pv_pitch_process_device.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, ip, C.c_int64, bp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, lp]
    L.pv_pitch_stretch.argtypes = [vp]
    L.pv_pitch_resampler.argtypes = [vp]
    L.pv_vari_create.argtypes = [C.POINTER(_VariConfig), C.POINTER(vp)]
    L.pv_vari_destroy.argtypes = [vp]
    L.pv_vari_reset.argtypes = [vp]
    L.pv_vari_last_error.argtypes = [vp]
    L.pv_vari_set_stream.argtypes = [vp, vp]
    L.pv_vari_synchronize.argtypes = [vp]
    L.pv_vari_process.argtypes = [vp, fp, C.c_int32, C.c_int64, ip, C.c_int64, fp, C.c_int64, C.c_int64, lp]
    L.pv_vari_process_device.argtypes = [vp, vp, C.c_int32, C.c_int64, ip, C.c_int64, vp, C.c_int64, C.c_int64, lp]
    L.pv_vari_export_state.argtypes = [vp, C.c_int32, fp, lp, lp]
    L.pv_vari_import_state.argtypes = [vp, C.c_int32, fp, C.c_int64, C.c_int64]
    L.pv_vari_prototype.argtypes = [fp, C.c_int64]
    L.pv_vari_half_width.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.pv_glide_create.argtypes = [C.POINTER(_GlideConfig), C.POINTER(vp)]
    L.pv_glide_destroy.argtypes = [vp]
    L.pv_glide_reset.argtypes = [vp]
    L.pv_glide_last_error.argtypes = [vp]
    L.pv_glide_set_stream.argtypes = [vp, vp]
    L.pv_glide_synchronize.argtypes = [vp]
    L.pv_glide_process.argtypes = [vp, fp, fp, C.c_int32, C.c_int32, ip, bp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_glide_process_device.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, ip, bp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_glide_stretch.argtypes = [vp]
    L.pv_glide_resampler.argtypes = [vp]
    L.pv_f0_create.argtypes = [C.POINTER(_F0Config), C.POINTER(vp)]
    L.pv_f0_destroy.argtypes = [vp]
    L.pv_f0_last_error.argtypes = [vp]
    L.pv_f0_set_stream.argtypes = [vp, vp]
    L.pv_f0_synchronize.argtypes = [vp]
    L.pv_f0_track.argtypes = [vp, fp, C.c_int32, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64]
    L.pv_f0_track_device.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, C.c_int32, vp, C.c_int64]
    L.pv_f0_period.argtypes = [ip]
    L.pv_tune_plan.argtypes = [C.POINTER(_TuneParams), ip, C.c_int64, ip, C.POINTER(C.c_double), C.c_int64]
    L.pv_psola_create.argtypes = [C.POINTER(_PsolaConfig), C.POINTER(vp)]
    L.pv_psola_destroy.argtypes = [vp]
    L.pv_psola_last_error.argtypes = [vp]
    L.pv_psola_set_stream.argtypes = [vp, vp]
    L.pv_psola_synchronize.argtypes = [vp]
    L.pv_psola_process.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, fp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_psola_process_device.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_psola_window.argtypes = [fp, C.c_int64]
    L.pv_psola_ratios.argtypes = [C.POINTER(_TuneParams), ip, C.c_int64, C.POINTER(C.c_double), C.c_int64]
    L.pv_psola_plan.argtypes = [C.POINTER(_PsolaParams), ip, C.c_int64, C.POINTER(C.c_double), ip, C.c_int64]
    L.pv_epoch_create.argtypes = [C.POINTER(_EpochConfig), C.POINTER(vp)]
    L.pv_epoch_destroy.argtypes = [vp]
    L.pv_epoch_last_error.argtypes = [vp]
    L.pv_epoch_set_stream.argtypes = [vp, vp]
    L.pv_epoch_synchronize.argtypes = [vp]
    L.pv_epoch_track.argtypes = [vp, fp, C.c_int32, C.c_int64, C.c_int64, ip, ip, C.c_int64]
    L.pv_epoch_track_device.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, vp, vp, C.c_int64]
    L.pv_epoch_periods.argtypes = [ip, C.c_int64, ip, C.c_int64]
    L.pv_epoch_plan.argtypes = [C.POINTER(_PsolaParams), C.POINTER(_EpochParams), ip, C.c_int64, C.POINTER(C.c_double), ip, ip, C.c_int64]
    for n in EXPORTS:
        if n not in ("pv_last_error", "pv_status_string", "pv_stretch_last_error"):
            getattr(L, n).restype = C.c_int
    L.pv_onsets_from_strength.restype = L.pv_transient_plan.restype = C.c_int64
    L.pv_resample_design.restype = L.pv_resample_count.restype = C.c_int64
    L.pv_resample_last_error.restype = L.pv_pitch_last_error.restype = C.c_char_p
    L.pv_pitch_stretch.restype = L.pv_pitch_resampler.restype = vp
    L.pv_vari_prototype.restype = C.c_int64
    L.pv_vari_half_width.restype = C.c_int32
    L.pv_vari_last_error.restype = L.pv_glide_last_error.restype = C.c_char_p
    L.pv_glide_stretch.restype = L.pv_glide_resampler.restype = vp
    L.pv_f0_last_error.restype = C.c_char_p
    L.pv_f0_period.restype = C.c_double
    L.pv_tune_plan.restype = C.c_int64
    L.pv_psola_last_error.restype = C.c_char_p
    L.pv_psola_window.restype = L.pv_psola_ratios.restype = L.pv_psola_plan.restype = C.c_int64
    L.pv_epoch_last_error.restype = C.c_char_p
    L.pv_epoch_periods.restype = L.pv_epoch_plan.restype = C.c_int64
    L.pv_tsm_create.argtypes = [C.POINTER(_TsmConfig), C.POINTER(vp)]
    L.pv_tsm_destroy.argtypes = [vp]
    L.pv_tsm_last_error.argtypes = [vp]
    L.pv_tsm_set_stream.argtypes = [vp, vp]
    L.pv_tsm_synchronize.argtypes = [vp]
    L.pv_tsm_process.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, fp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_tsm_process_device.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_tsm_plan.argtypes = [C.POINTER(_PsolaParams), C.POINTER(_EpochParams), ip, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), ip, ip, C.c_int64,
                              C.POINTER(C.c_int64)]
    L.pv_tsm_last_error.restype = C.c_char_p
    L.pv_tsm_plan.restype = C.c_int64
    L.pv_harmony_create.argtypes = [C.POINTER(_HarmonyConfig), C.POINTER(vp)]
    L.pv_harmony_destroy.argtypes = [vp]
    L.pv_harmony_last_error.argtypes = [vp]
    L.pv_harmony_set_stream.argtypes = [vp, vp]
    L.pv_harmony_synchronize.argtypes = [vp]
    L.pv_harmony_process.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int32, ip, C.POINTER(C.c_int64), C.c_int32, fp, fp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_harmony_process_device.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32, ip, C.POINTER(C.c_int64), C.c_int32, fp, vp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_harmony_ratios.argtypes = [C.POINTER(_TuneParams), ip, C.c_int64, ip, C.c_int32, C.POINTER(C.c_double), C.c_int64]
    L.pv_harmony_last_error.restype = C.c_char_p
    L.pv_harmony_ratios.restype = C.c_int64
    L.pv_takes_create.argtypes = [C.POINTER(_TakesConfig), C.POINTER(vp)]
    L.pv_takes_destroy.argtypes = [vp]
    L.pv_takes_last_error.argtypes = [vp]
    L.pv_takes_set_stream.argtypes = [vp, vp]
    L.pv_takes_synchronize.argtypes = [vp]
    L.pv_takes_process.argtypes = [vp, C.POINTER(_Take), C.c_int32, C.c_int32]
    L.pv_takes_process_device.argtypes = [vp, C.POINTER(_Take), C.c_int32, C.c_int32]
    L.pv_takes_tiles.argtypes = [C.POINTER(_TakesConfig), C.POINTER(_Take), C.c_int32, ip, C.c_int64]
    L.pv_takes_last_error.restype = C.c_char_p
    L.pv_takes_tiles.restype = C.c_int64
    L.pv_mirror_create.argtypes = [C.POINTER(_MirrorConfig), C.POINTER(vp)]
    L.pv_mirror_destroy.argtypes = [vp]
    L.pv_mirror_last_error.argtypes = [vp]
    L.pv_mirror_set_stream.argtypes = [vp, vp]
    L.pv_mirror_synchronize.argtypes = [vp]
    L.pv_mirror_process.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, fp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_mirror_process_device.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_mirror_plan.argtypes = [C.POINTER(_PsolaParams), C.POINTER(_EpochParams), ip, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), ip, C.c_int32, ip,
                                 C.c_int64, C.POINTER(C.c_int64)]
    L.pv_mirror_last_error.restype = C.c_char_p
    L.pv_mirror_plan.restype = C.c_int64
    L.pv_formant_create.argtypes = [C.POINTER(_FormantConfig), C.POINTER(vp)]
    L.pv_formant_destroy.argtypes = [vp]
    L.pv_formant_last_error.argtypes = [vp]
    L.pv_formant_set_stream.argtypes = [vp, vp]
    L.pv_formant_synchronize.argtypes = [vp]
    L.pv_formant_process.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, fp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_formant_process_device.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_formant_plan.argtypes = [C.POINTER(_PsolaParams), C.POINTER(_EpochParams), ip, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  ip, ip, C.c_int64, C.POINTER(C.c_int64)]
    L.pv_formant_last_error.restype = C.c_char_p
    L.pv_formant_plan.restype = C.c_int64
    L.pv_contour_create.argtypes = [C.POINTER(_ContourConfig), C.POINTER(vp)]
    L.pv_contour_destroy.argtypes = [vp]
    L.pv_contour_last_error.argtypes = [vp]
    L.pv_contour_set_stream.argtypes = [vp, vp]
    L.pv_contour_synchronize.argtypes = [vp]
    L.pv_contour_track.argtypes = [vp, fp, C.c_int32, C.c_int64, C.c_int64, C.c_int32, ip, C.c_int64]
    L.pv_contour_track_device.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, C.c_int32, vp, C.c_int64]
    L.pv_contour_path.argtypes = [C.POINTER(_ContourParams), ip, C.c_int64, ip, ip]
    L.pv_contour_last_error.restype = C.c_char_p
    L.pv_choir_create.argtypes = [C.POINTER(_ChoirConfig), C.POINTER(vp)]
    L.pv_choir_destroy.argtypes = [vp]
    L.pv_choir_last_error.argtypes = [vp]
    L.pv_choir_set_stream.argtypes = [vp, vp]
    L.pv_choir_synchronize.argtypes = [vp]
    L.pv_choir_process.argtypes = [vp, fp, C.c_int64, C.c_int64, C.c_int32, ip, C.POINTER(C.c_int64), C.c_int32, fp, fp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_choir_process_device.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32, ip, C.POINTER(C.c_int64), C.c_int32, fp, vp, C.c_int64, C.c_int64, C.c_int64]
    L.pv_choir_plan.argtypes = [C.POINTER(_PsolaParams), C.POINTER(_EpochParams), ip, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                ip, C.c_int32, ip, C.c_int64, C.POINTER(C.c_int64)]
    L.pv_choir_last_error.restype = C.c_char_p
    L.pv_choir_plan.restype = C.c_int64
    L.pv_process_begin.argtypes = [vp, C.POINTER(fp), C.c_int32, C.c_int32, C.c_float]
    L.pv_process_end.argtypes = [vp, C.POINTER(fp)]
    L.pv_device_count.argtypes = [C.POINTER(C.c_int32)]
    L.pv_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.pv_host_free.argtypes = [vp]
    L.pv_forward_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int32]
    L.pv_abi_version.argtypes = []
    if L.pv_abi_version() != ABI_VERSION:
        raise PvError(PV_ERR_ARGUMENT, f"{_LIB_PATH} has PV_ABI_VERSION {L.pv_abi_version()}, this binding expects {ABI_VERSION}: rebuild the library")
    _lib = L
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class _PinnedBlock:
    """Owner of one pv_host_alloc block: frees it when the last numpy view is gone."""

    def __init__(self, nbytes):
        self._L = load_library()
        self.ptr = C.c_void_p()
        rc = self._L.pv_host_alloc(max(int(nbytes), 1), C.byref(self.ptr))
        if rc != PV_OK:
            raise PvError(rc, self._L.pv_last_error(None).decode())
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.ptr and self.ptr.value:
                self._L.pv_host_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float32):
    """numpy array in page-locked host memory (pv_host_alloc): process_batch() pipelines batches that live in such arrays (DMA both ways at
    once).  The memory is released when the array and every view of it are gone."""
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if shape else 1
    blk = _PinnedBlock(n * dt.itemsize)
    buf = (C.c_char * max(n * dt.itemsize, 1)).from_address(blk.ptr.value)
    buf._pv_owner = blk                              # the ctypes object keeps the block alive; numpy keeps the ctypes object alive (base)
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


class _Handle:
    """What the handle classes share: create-and-raise, close, the status check and reset / set_stream / synchronize.  `_prefix` is the C
    prefix of the handle type's entry points (<prefix>_create, _destroy, _last_error, _reset, _set_stream, _synchronize)."""

    _prefix = None
    _fft_size_is_value_error = True     # PV_ERR_FFT_SIZE from create raises ValueError: the reference throws Error('FFT size must be ...') (bundle:6-7)
    _owned = True                       # close() destroys the handle (False: borrowed from the handle that owns it)

    def _bind(self, handle=None):
        self._L = load_library()
        self._h = C.c_void_p(handle)
        self._destroy, self._last_error, self._reset, self._set_stream, self._synchronize = (
            getattr(self._L, f"{self._prefix}_{n}", None) for n in ("destroy", "last_error", "reset", "set_stream", "synchronize"))   # a stateless handle has no reset

    def _create(self, cfg):
        self._bind()
        rc = getattr(self._L, self._prefix + "_create")(C.byref(cfg), C.byref(self._h))
        if rc != PV_OK:
            msg = self._last_error(None).decode()
            self._h = C.c_void_p()
            if rc == PV_ERR_FFT_SIZE and self._fft_size_is_value_error:
                raise ValueError(msg)
            raise PvError(rc, msg)

    def close(self):
        if getattr(self, "_h", None) and self._h.value and self._owned:
            self._destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != PV_OK:
            raise PvError(rc, self._last_error(self._h).decode())

    def reset(self):
        self._check(self._reset(self._h))

    def set_stream(self, hip_stream):
        self._check(self._set_stream(self._h, C.c_void_p(hip_stream)))

    def synchronize(self):
        self._check(self._synchronize(self._h))


class PhaseVocoder(_Handle):
    """One processor instance = one `new PhaseVocoderProcessor(options)` (phase-vocoder.js:24-43)."""

    _prefix = "pv"
    parameter_descriptors = [{"name": "pitchFactor", "defaultValue": 1.0}]   # phase-vocoder.js:17-22

    def __init__(self, fft_size=2048, hop_size=128, max_channels=2, max_hops=1, device_id=0, frames_per_chunk=0, flags=0):
        self._create(make_config(fft_size, hop_size, max_channels, max_hops, device_id, frames_per_chunk, flags))
        self.fft_size, self.hop_size = fft_size, hop_size
        self.max_channels, self.max_hops = max_channels, max_hops
        self._host_channels = bool(flags & FLAG_HOST_CHANNEL_BOOKKEEPING)
        self._nin = self._nout = 1                          # "default to 1 channel per input / output until we know more" (ola-processor.js:24-33)
        # host bookkeeping only: what it takes to reproduce an output channel that lost its input while outputs[0].length stayed (see _stale_frame)
        self._device_id, self._flags = device_id, flags
        self._window = np.zeros((max_channels, fft_size), np.float32) if self._host_channels else None   # inputBuffers as the reference holds them (ola-processor.js:59,121-127)
        self._stale = {}                                    # channel -> [frame / nbOverlaps as the last real quantum added it, quanta it has been re-added since]
        self._last_pitch = None
        self._scratch = None

    # -- lifetime --
    def close(self):
        if getattr(self, "_scratch", None) is not None:
            self._scratch.close()
            self._scratch = None
        super().close()

    # -- state --
    def reset_channels(self, first, count, parts=STATE_HISTORY | STATE_ACCUMULATOR):
        self._check(self._L.pv_reset_channels_part(self._h, first, count, parts))

    @property
    def time_cursor(self):
        v = C.c_int64()
        self._check(self._L.pv_get_time_cursor(self._h, C.byref(v)))
        return v.value

    @time_cursor.setter
    def time_cursor(self, value):
        self._check(self._L.pv_set_time_cursor(self._h, int(value)))

    def export_state(self, ch):
        """(hist[N-hop], acc[N-hop], time_cursor) of channel slot `ch`: ola-processor.js:59,77 + phase-vocoder.js:31."""
        L = self.fft_size - self.hop_size
        hist, acc, tc = np.zeros(max(L, 1), np.float32), np.zeros(max(L, 1), np.float32), C.c_int64()
        self._check(self._L.pv_export_state(self._h, ch, _fp(hist), _fp(acc), C.byref(tc)))
        return hist[:L], acc[:L], tc.value

    def import_state(self, ch, hist=None, acc=None, time_cursor=-1):
        L = self.fft_size - self.hop_size
        def chk(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.size != L:
                raise ValueError(f"state arrays hold N - hop = {L} floats")
            return a
        hist, acc = chk(hist), chk(acc)
        self._check(self._L.pv_import_state(self._h, ch, _fp(hist) if hist is not None and L else None,
                                            _fp(acc) if acc is not None and L else None, C.c_int64(int(time_cursor))))

    def info(self):
        i = _Info()
        self._check(self._L.pv_get_info(self._h, C.byref(i)))
        d = {n: getattr(i, n) for n, _ in _Info._fields_}
        d["device_name"] = i.device_name.decode()
        d["kernel_name"] = i.kernel_name.decode()
        return d

    # -- the hot call, AudioWorklet form --
    def process(self, inputs, outputs, parameters):
        """inputs[0][c]: float32[hop] (or length 0 when paused); outputs[0][c]: float32[hop], filled.
        parameters['pitchFactor']: float32 array, last element used (phase-vocoder.js:47).  Returns True."""
        chans = inputs[0]
        nch = len(chans)
        if self._host_channels:
            # the reference's reallocateChannelsIfNeeded (ola-processor.js:38-52): inputs and outputs are two separate events
            if len(outputs[0]) < nch:
                raise TypeError("outputs[0] has fewer channels than inputs[0]: the reference's processOLA dereferences outputs[i][j] (phase-vocoder.js:51) and throws")
            out_changed = len(outputs[0]) != self._nout
            if nch != self._nin:
                if not out_changed:
                    # One corner of ola-processor.js (149-157): `outputBuffersToRetrieve` is only reallocated with the OUTPUT channels, so an output channel whose input
                    # disappears keeps its last frame there, and handleOutputBuffersToRetrieve goes on adding that stale frame (and shifting) every quantum.  Nobody
                    # hears it (writeOutputs walks the input channels) -- unless the input returns before the output count changes: then the channel's pending sums
                    # are those of the stale frame.  Lost channels: remember the frame; regained channels: their accumulator becomes what the reference's has become.
                    for c in range(nch, min(self._nin, self._nout, self.max_channels)):
                        self._stale[c] = [self._stale_frame(c), 0]
                    regained = {c: self._stale_accumulator(c) for c in range(self._nin, min(nch, self.max_channels)) if c in self._stale}
                else:
                    regained = {}
                self.reset_channels(0, self.max_channels, STATE_HISTORY)
                self._window[:] = 0.0
                for c, acc in regained.items():
                    self.import_state(c, acc=acc)
                    del self._stale[c]
                self._nin = nch
            if out_changed:
                self._stale.clear()                                              # allocateOutputChannels: fresh (zeroed) outputBuffersToRetrieve (ola-processor.js:74-85)
                self.reset_channels(0, self.max_channels, STATE_ACCUMULATOR)
                self._nout = len(outputs[0])
        pf = np.asarray(parameters["pitchFactor"], dtype=np.float32)
        pitch = float(pf[-1])
        paused = nch > 0 and len(chans[0]) == 0                                 # ola-processor.js:93
        outs = outputs[0]
        fpt = C.POINTER(C.c_float)
        keep = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
        ip = (fpt * max(nch, 1))(*[_fp(a) if a.size else None for a in keep])
        tmp = [np.zeros(self.hop_size, dtype=np.float32) for _ in range(nch)]
        op = (fpt * max(nch, 1))(*[_fp(a) for a in tmp])
        self._check(self._L.pv_process(self._h, ip, op, nch, 0 if paused else self.hop_size, C.c_float(pitch)))
        for c in range(min(nch, len(outs))):
            outs[c][:] = tmp[c]
        if self._host_channels:
            h = self.hop_size
            for c in range(min(nch, self.max_channels)):                           # readInputs + shiftInputBuffers (ola-processor.js:89-127)
                w = self._window[c]
                if h < self.fft_size:
                    w[:-h] = w[h:].copy()
                w[-h:] = 0.0 if paused else keep[c]
            self._last_pitch = pitch
            for rec in self._stale.values():
                rec[1] += 1
        return True

    def _stale_frame(self, ch):
        """The windowed frame / nbOverlaps that the last quantum added for channel `ch`, recomputed on a one-channel scratch handle from the window the reference's
        inputBuffers held (zero accumulator in: the hop that comes out and the accumulator left behind ARE the frame, 0 + x being exact)."""
        N, h = self.fft_size, self.hop_size
        t = self.time_cursor
        if self._last_pitch is None or t < h:
            return np.zeros(N, np.float32)                                        # no frame yet: outputBuffersToRetrieve still holds its zeros
        if self._scratch is None:
            self._scratch = PhaseVocoder(N, h, 1, 1, self._device_id, 0, self._flags & FLAG_FP64_FORWARD)
        sc = self._scratch
        sc.import_state(0, hist=self._window[ch, :N - h], acc=np.zeros(N - h, np.float32), time_cursor=t - h)
        out = [[np.zeros(h, np.float32)]]
        sc.process([[self._window[ch, N - h:].copy()]], out, {"pitchFactor": np.array([self._last_pitch], np.float32)})
        return np.concatenate([out[0][0], sc.export_state(0)[1]]).astype(np.float32)

    def _stale_accumulator(self, ch):
        """outputBuffers of a channel whose stale frame has been re-added for q quanta (f32 adds in the reference's order, ola-processor.js:130-157)."""
        N, h = self.fft_size, self.hop_size
        frame, q = self._stale[ch]
        a = np.concatenate([self.export_state(ch)[1], np.zeros(h, np.float32)]).astype(np.float32)
        for _ in range(min(q, N // h + 1)):                                       # (after N / hop quanta the sums no longer change)
            a = a + frame
            a = np.concatenate([a[h:], np.zeros(h, np.float32)])
        return a[:N - h]

    # -- the hot call, batch forms --
    def process_batch(self, x, pitch, channels_per_stream=0, out=None):
        """x: float32[nch, nhops*hop] (host); pitch: float32[nhops] or [nstreams, nhops]. Returns y like x (written into `out` when given:
        with x and out in page-locked memory -- pinned_empty() -- the call is pipelined, see pv_process_batch)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        nch, n = x.shape
        nhops = n // self.hop_size
        assert nhops * self.hop_size == n
        pitch = np.ascontiguousarray(pitch, dtype=np.float32)
        stride = 0
        if pitch.ndim == 2:
            stride = pitch.shape[1]
        if out is not None:
            assert out.shape == x.shape and out.dtype == np.float32 and out.flags.c_contiguous
            y = out
        else:
            y = np.empty_like(x)
        self._check(self._L.pv_process_batch(self._h, _fp(x), _fp(y), nch, nhops, n, _fp(pitch), stride, channels_per_stream or 1))
        return y

    def process_batch_device(self, d_in, d_out, nch, nhops, ch_stride, d_pitch, pitch_stride=0, channels_per_stream=1):
        """Raw device pointers (ints).  Asynchronous on the handle's stream."""
        self._check(self._L.pv_process_batch_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), nch, nhops, ch_stride,
                                                    C.c_void_p(d_pitch), pitch_stride, channels_per_stream))

    def forward_stats(self, reset=False):
        """(frames whose forward transform an fp32-first instance computed, frames of those that re-ran it in fp64) since creation / the last reset."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pv_forward_stats(self._h, C.byref(a), C.byref(b), 1 if reset else 0))
        return int(a.value), int(b.value)

    # -- test tap --
    def debug_frame(self, ch, block, pitch):
        N = self.fft_size
        H = N // 2 + 1
        block = np.ascontiguousarray(block, dtype=np.float32)
        X = np.zeros(2 * N, dtype=np.float64)
        mag = np.zeros(H, dtype=np.float32)
        flags = np.zeros(H, dtype=np.int32)
        Y = np.zeros(2 * H, dtype=np.float32)
        self._check(self._L.pv_debug_frame(self._h, ch, _fp(block), C.c_float(float(pitch)), X.ctypes.data_as(C.POINTER(C.c_double)),
                                           _fp(mag), flags.ctypes.data_as(C.POINTER(C.c_int32)), _fp(Y)))
        return {"X": X, "mag": mag, "flags": flags, "Y": Y}


def tempo_hops(tempo, synthesis_hop, min_hop, max_hop, carry=0.0):
    """Integer analysis hops for a per-frame tempo (input samples per output sample: 1.25 plays 25 % faster), by error diffusion:
    hop_m = round(carry + tempo_m * synthesis_hop), the remainder carried on.  After every frame the input consumed, sum(hops), is within half a
    sample of carry + sum(tempo * synthesis_hop).  Every tempo_m * synthesis_hop must lie in [min_hop, max_hop] (a TimeStretch's analysis_hop and
    fft_size).  Returns (int32[nframes] hops, carry); continuing with the returned carry gives the hops of one call over the whole tempo track."""
    t = np.atleast_1d(np.asarray(tempo, np.float64))
    if t.ndim != 1:
        raise ValueError("tempo must be a scalar or one value per frame")
    want = t * synthesis_hop
    if not (min_hop <= max_hop) or np.any(~np.isfinite(want)) or np.any(want < min_hop) or np.any(want > max_hop):
        raise ValueError(f"tempo * synthesis_hop must lie in [{min_hop}, {max_hop}]")
    hops = np.empty(t.size, np.int32)
    e = float(carry)
    for m, w in enumerate(want.tolist()):
        x = e + w
        h = min(max(int(np.floor(x + 0.5)), min_hop), max_hop)
        hops[m] = h
        e = x - h
    return hops, e


def onsets_from_strength(counts, fft_size, analysis_hop, tau=0.4):
    """pv_onsets_from_strength: int64 onset positions (input samples) from one row of onset counts (TimeStretch.onset_strength).  Frame m is an onset
    when counts[m] >= tau (fft_size / 2 - 1) and counts[m - 1] is below it; its position is m * analysis_hop."""
    L = load_library()
    c = np.ascontiguousarray(counts, dtype=np.int32)
    if c.ndim != 1:
        raise ValueError("counts must be one row, int[nframes]")
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    n = L.pv_onsets_from_strength(c.ctypes.data_as(ip), c.size, fft_size, analysis_hop, float(tau), None, 0)
    if n < 0:
        raise ValueError("onsets_from_strength: bad argument (tau must be > 0, fft_size >= 4, analysis_hop >= 1)")
    out = np.zeros(n, np.int64)
    if n:
        L.pv_onsets_from_strength(c.ctypes.data_as(ip), c.size, fft_size, analysis_hop, float(tau), out.ctypes.data_as(lp), n)
    return out


def transient_plan(onsets, input_len, fft_size, nominal_hop, floor_hop, synthesis_hop, lead=None, release=None):
    """pv_transient_plan: (hops int32[T], resets uint8[T]) for TimeStretch.process_hops(x[:, :hops.sum()], hops, resets).  onsets: sorted positions in
    input samples; nominal_hop: the hop outside holds (tempo synthesis_hop / nominal_hop); floor_hop: the handle's analysis_hop; lead: 0 .. fft_size/2,
    default fft_size / 8; release: how many samples behind its position an attack is taken to last, 0 .. fft_size, default fft_size / 2 (a frame is
    held while [lead, N - lead) of its window meets [onset, onset + release]).  Raises ValueError when synthesis_hop < floor_hop (a hold runs at hop == synthesis_hop) or an argument is out of range."""
    L = load_library()
    o = np.ascontiguousarray(onsets, dtype=np.int64).ravel()
    ip, lp, bp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    args = (o.ctypes.data_as(lp), o.size, int(input_len), fft_size, nominal_hop, floor_hop, synthesis_hop, -1 if lead is None else int(lead),
            -1 if release is None else int(release))
    if (lead is not None and lead < 0) or (release is not None and release < 0):
        raise ValueError("lead must be within 0 .. fft_size / 2 and release within 0 .. fft_size")
    n = L.pv_transient_plan(*args, None, None, 0)
    if n < 0:
        raise ValueError("transient_plan: bad argument (synthesis_hop >= floor_hop, floor_hop <= nominal_hop <= fft_size, lead <= fft_size / 2, release <= fft_size, sorted onsets)")
    hops, resets = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    if n:
        L.pv_transient_plan(*args, hops.ctypes.data_as(ip), resets.ctypes.data_as(bp), n)
    return hops, resets


class TimeStretch(_Handle):
    """Phase-locked time stretch (pv_stretch_*): tempo change at constant pitch.  Each frame consumes `analysis_hop` input samples and emits
    `synthesis_hop` output samples, so the output lasts synthesis_hop / analysis_hop times as long; it lags the input by fft_size - synthesis_hop
    samples.  State carries across calls: any split of a stream into calls gives the same bits.  channels_per_group > 1 links consecutive channel
    slots into groups with one phase track each (pv_link_channels, link_channels): the stereo image survives the stretch."""

    _prefix = "pv_stretch"

    def __init__(self, fft_size, analysis_hop, synthesis_hop, max_channels=1, max_frames=1, device_id=0, channels_per_group=1):
        self._create(make_stretch_config(fft_size, analysis_hop, synthesis_hop, max_channels, max_frames, device_id, 0))
        self.fft_size, self.analysis_hop, self.synthesis_hop = fft_size, analysis_hop, synthesis_hop
        self.max_channels, self.max_frames = max_channels, max_frames
        self.channels_per_group = 1
        if channels_per_group != 1:
            try:
                self.link_channels(channels_per_group)
            except Exception:
                self.close()
                raise

    def reset(self):
        """Zero every slot's state; the channel linking stays."""
        super().reset()

    def link_channels(self, channels_per_group):
        """pv_link_channels: slots [g G, (g + 1) G) become one group with one phase track (G = 1: every slot on its own).  Resets every slot."""
        self._check(self._L.pv_link_channels(self._h, int(channels_per_group)))
        self.channels_per_group = int(channels_per_group)

    def _check_groups(self, nch):
        if nch % self.channels_per_group:
            raise ValueError(f"{nch} channels are not a whole number of linked groups of {self.channels_per_group}")

    def process(self, x):
        """x: float32[nch, nframes * analysis_hop] (host) -> float32[nch, nframes * synthesis_hop] for channel slots 0 .. nch-1."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, n = x.shape
        nframes = n // self.analysis_hop
        if nframes * self.analysis_hop != n:
            raise ValueError("the input length must be a whole number of analysis hops")
        self._check_groups(nch)
        y = np.empty((nch, nframes * self.synthesis_hop), np.float32)
        if nch and nframes:
            self._check(self._L.pv_stretch_process(self._h, _fp(x), _fp(y), nch, nframes, n, nframes * self.synthesis_hop))
        return y

    def process_device(self, d_in, d_out, nch, nframes, in_stride, out_stride):
        """Raw device pointers (ints).  Asynchronous on the handle's stream."""
        self._check_groups(nch)
        self._check(self._L.pv_stretch_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), nch, nframes, in_stride, out_stride))

    @staticmethod
    def _hop_rows(hops):
        """(int32 array, nframes, hop_stride): a 1-D schedule is one row for every channel, a 2-D one [nch, nframes] a row per channel."""
        hops = np.ascontiguousarray(hops, dtype=np.int32)
        if hops.ndim == 1:
            return hops, hops.size, 0
        if hops.ndim != 2:
            raise ValueError("hops must be int[nframes] or int[nch, nframes]")
        return hops, hops.shape[1], hops.shape[1]

    @staticmethod
    def _reset_rows(resets, nframes):
        """(uint8 array, reset_stride): a 1-D row of nframes flags is shared by every channel, a 2-D one [nch, >= nframes] holds a row per channel."""
        r = np.ascontiguousarray(resets, dtype=np.uint8)
        if r.ndim == 1 and r.size == nframes:
            return r, 0
        if r.ndim == 2 and r.shape[1] >= nframes:
            return r, r.shape[1]
        raise ValueError(f"resets must be [nframes] or [nch, >= nframes] with nframes = {nframes}")

    def process_hops(self, x, hops, resets=None):
        """Variable tempo (pv_tempo_process): frame m of channel c consumes hops[m] (1-D) or hops[c, m] (2-D) input samples, each in
        [analysis_hop, fft_size], and emits synthesis_hop samples.  x: float32[nch, n] (host), n == hops.sum() for a 1-D schedule, n >= the largest
        row sum for a 2-D one (each row reads its own prefix) -> float32[nch, nframes * synthesis_hop].
        resets (pv_transient_process): 0 / 1 per frame, [nframes] or [nch, nframes]; a flagged frame sets psi := q (its output is the windowed input
        frame), and the frames after it at hop == synthesis_hop stay the input sample for sample.  hops=None: every hop is analysis_hop."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, n = x.shape
        if hops is None:
            if resets is None:
                return self.process(x)
            hops = np.full(n // self.analysis_hop, self.analysis_hop, np.int32)
        h, nframes, stride = self._hop_rows(hops)
        if h.ndim == 1 and int(h.astype(np.int64).sum()) != n:
            raise ValueError(f"the input holds {n} samples per channel, the schedule consumes {int(h.astype(np.int64).sum())}")
        if h.ndim == 2:
            if h.shape[0] != nch:
                raise ValueError(f"{h.shape[0]} schedule rows for {nch} channels")
            if nframes and int(h.astype(np.int64).sum(axis=1).max()) > n:
                raise ValueError("the input is shorter than a row of the schedule consumes")
        self._check_groups(nch)
        y = np.empty((nch, nframes * self.synthesis_hop), np.float32)
        if nch and nframes and resets is None:
            self._check(self._L.pv_tempo_process(self._h, _fp(x), _fp(y), nch, nframes, h.ctypes.data_as(C.POINTER(C.c_int32)), stride, n,
                                                 nframes * self.synthesis_hop))
        elif nch and nframes:
            r, rstride = self._reset_rows(resets, nframes)
            if r.ndim == 2 and r.shape[0] != nch:
                raise ValueError(f"{r.shape[0]} reset rows for {nch} channels")
            self._check(self._L.pv_transient_process(self._h, _fp(x), _fp(y), nch, nframes, h.ctypes.data_as(C.POINTER(C.c_int32)), stride,
                                                     r.ctypes.data_as(C.POINTER(C.c_uint8)), rstride, n, nframes * self.synthesis_hop))
        return y

    def process_hops_device(self, d_in, d_out, nch, nframes, hops, in_stride, out_stride, resets=None):
        """pv_tempo_process_device on raw device pointers (ints), asynchronous on the handle's stream.  hops: host int[nframes] (shared) or int[nch, >= nframes];
        the library has read it when this returns."""
        h, _, stride = self._hop_rows(hops)
        if h.ndim == 1 and h.size != nframes:
            raise ValueError(f"{h.size} hops for {nframes} frames")
        if h.ndim == 2 and h.shape[0] < nch:
            raise ValueError(f"{h.shape[0]} schedule rows for {nch} channels")
        self._check_groups(nch)
        if resets is not None:
            r, rstride = self._reset_rows(resets, nframes)
            if r.ndim == 2 and r.shape[0] < nch:
                raise ValueError(f"{r.shape[0]} reset rows for {nch} channels")
            self._check(self._L.pv_transient_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), nch, nframes, h.ctypes.data_as(C.POINTER(C.c_int32)),
                                                            stride, r.ctypes.data_as(C.POINTER(C.c_uint8)), rstride, in_stride, out_stride))
            return
        self._check(self._L.pv_tempo_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), nch, nframes, h.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    stride, in_stride, out_stride))

    def onset_strength(self, x):
        """pv_onset_strength: x float32[nch, n] (host) -> int32[nch / channels_per_group, n // analysis_hop], per group and frame the number of bins
        whose power rose more than fourfold over the previous frame and lies above 2^-20 of the frame's largest.  Frame m's window ends at
        (m + 1) analysis_hop; zeros before x.  Stateless: the handle's carried state is neither read nor written."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, n = x.shape
        self._check_groups(nch)
        nframes = n // self.analysis_hop
        counts = np.zeros((nch // self.channels_per_group, nframes), np.int32)
        if nch and nframes:
            self._check(self._L.pv_onset_strength(self._h, _fp(x), nch, nframes, n, counts.ctypes.data_as(C.POINTER(C.c_int32)), nframes))
        return counts

    def onset_strength_device(self, d_in, nch, nframes, in_stride, d_counts, count_stride):
        """pv_onset_strength_device on raw device pointers (ints), asynchronous on the handle's stream."""
        self._check_groups(nch)
        self._check(self._L.pv_onset_strength_device(self._h, C.c_void_p(d_in), nch, nframes, in_stride, C.c_void_p(d_counts), count_stride))

    def chain_layout(self, nch, nframes):
        """(frames per chain, halo) of a call of nch channels and nframes frames on this chip (pv_transient_chain_layout, a test hook)."""
        F, halo = C.c_int32(), C.c_int32()
        self._check(self._L.pv_transient_chain_layout(self._h, nch, nframes, C.byref(F), C.byref(halo)))
        return F.value, halo.value

    def onset_chain_layout(self, nch, nframes):
        """Frames per chain of an onset_strength call of nch channels and nframes frames on this chip (pv_onset_chain_layout, a test hook)."""
        F = C.c_int32()
        self._check(self._L.pv_onset_chain_layout(self._h, nch, nframes, C.byref(F)))
        return F.value

    def process_transients(self, x, tau=0.4, lead=None, hop=None, release=None):
        """Offline stretch that carries attacks through unstretched: onset_strength -> onsets_from_strength(tau) -> transient_plan(lead, release) ->
        process_hops(hops, resets).  x: float32[nch, n] (host).  hop: the nominal analysis hop outside holds (tempo synthesis_hop / hop), default
        analysis_hop; for a speed-up create the handle with analysis_hop <= synthesis_hop and pass the nominal hop here.  Every channel follows ONE
        schedule, planned from the onsets of all groups together, so channels stay aligned with each other.  Returns (y float32[nch, T *
        synthesis_hop], hops, resets); the schedule consumes x[:, :hops.sum()]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        hop = self.analysis_hop if hop is None else int(hop)
        counts = self.onset_strength(x)
        onsets = np.unique(np.concatenate([onsets_from_strength(row, self.fft_size, self.analysis_hop, tau) for row in counts] + [np.zeros(0, np.int64)]))
        hops, resets = transient_plan(onsets, x.shape[1], self.fft_size, hop, self.analysis_hop, self.synthesis_hop, lead, release)
        y = self.process_hops(x[:, :int(hops.astype(np.int64).sum())], hops, resets)
        return y, hops, resets

    def export_state(self, ch):
        """(hist[N - ha], acc[N - hs], phi[N/2 + 1] u32, psi[N/2 + 1] u32) of channel slot `ch`."""
        N, H = self.fft_size, self.fft_size // 2 + 1
        hist = np.zeros(max(N - self.analysis_hop, 1), np.float32)
        acc = np.zeros(N - self.synthesis_hop, np.float32)
        phi, psi = np.zeros(H, np.uint32), np.zeros(H, np.uint32)
        up = C.POINTER(C.c_uint32)
        self._check(self._L.pv_stretch_export_state(self._h, ch, _fp(hist), _fp(acc), phi.ctypes.data_as(up), psi.ctypes.data_as(up)))
        return hist[:N - self.analysis_hop], acc, phi, psi

    def import_state(self, ch, hist=None, acc=None, phi=None, psi=None):
        N, H = self.fft_size, self.fft_size // 2 + 1
        up = C.POINTER(C.c_uint32)

        def chk(a, n, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != n:
                raise ValueError(f"state array of {a.size} values, {n} expected")
            return a
        hist, acc = chk(hist, N - self.analysis_hop, np.float32), chk(acc, N - self.synthesis_hop, np.float32)
        phi, psi = chk(phi, H, np.uint32), chk(psi, H, np.uint32)
        self._check(self._L.pv_stretch_import_state(self._h, ch, _fp(hist) if hist is not None and hist.size else None, _fp(acc) if acc is not None else None,
                                                    phi.ctypes.data_as(up) if phi is not None else None, psi.ctypes.data_as(up) if psi is not None else None))


def resample_design(up, down):
    """pv_resample_design: (taps float32[L, T], L, M, W) of the ratio up / down -- the table the kernels use (T = 2 W taps per phase)."""
    L_ = load_library()
    l, m, w = C.c_int32(), C.c_int32(), C.c_int32()
    n = L_.pv_resample_design(int(up), int(down), None, 0, C.byref(l), C.byref(m), C.byref(w))
    if n < 0:
        raise ValueError("resample_design: up and down must be positive, up / down within [1/8, 8], both terms <= 8192 once reduced")
    taps = np.zeros(n, np.float32)
    L_.pv_resample_design(int(up), int(down), _fp(taps), n, None, None, None)
    return taps.reshape(l.value, 2 * w.value), l.value, m.value, w.value


def resample_count(up, down, total_in):
    """pv_resample_count: J(I) = max(0, ceil((I - W) L / M)), the outputs that exist after total_in input samples."""
    n = load_library().pv_resample_count(int(up), int(down), int(total_in))
    if n < 0:
        raise ValueError("resample_count: bad ratio or a negative total")
    return int(n)


class Resampler(_Handle):
    """Band-limited rational resampler (pv_resample_*): `up` output samples per `down` input samples, Kaiser-windowed sinc.  Output j of the stream
    sits at input position j down / up; the output lags by `latency` input samples (feed that many zeros to drain).  State carries across calls: any
    split of a stream into calls gives the same bits."""

    _prefix = "pv_resample"
    _fft_size_is_value_error = False

    def __init__(self, up, down, max_channels=1, max_samples=1 << 16, device_id=0, _borrowed=None):
        self._owned = _borrowed is None
        if _borrowed is not None:
            self._bind(_borrowed)
        else:
            self._create(make_resample_config(up, down, max_channels, max_samples, device_id, 0))
        l, m, w = C.c_int32(), C.c_int32(), C.c_int32()
        self._L.pv_resample_design(int(up), int(down), None, 0, C.byref(l), C.byref(m), C.byref(w))
        self.up, self.down, self.half_width, self.taps_per_phase = l.value, m.value, w.value, 2 * w.value
        self.max_channels = max_channels

    @property
    def latency(self):
        """The output's lag in input samples (the half width W)."""
        return self.half_width

    def out_count(self, nin):
        """What the next call of nin samples writes per channel."""
        n = C.c_int64()
        self._check(self._L.pv_resample_out_count(self._h, int(nin), C.byref(n)))
        return n.value

    def process(self, x):
        """x: float32[nch, nin] (host) -> float32[nch, out_count(nin)] for channel slots 0 .. nch-1."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, nin = x.shape
        cap = self.out_count(nin)
        y = np.empty((nch, cap), np.float32)
        n = C.c_int64()
        self._check(self._L.pv_resample_process(self._h, _fp(x), nch, nin, nin, _fp(y), cap, cap, C.byref(n)))
        assert n.value == cap
        return y

    def process_device(self, d_in, nch, nin, in_stride, d_out, out_stride, out_capacity):
        """Raw device pointers (ints).  Asynchronous on the handle's stream; returns the samples written per channel."""
        n = C.c_int64()
        self._check(self._L.pv_resample_process_device(self._h, C.c_void_p(d_in), nch, nin, in_stride, C.c_void_p(d_out), out_stride, out_capacity, C.byref(n)))
        return n.value

    def export_state(self, ch):
        """(hist float32[T - 1], total_in, total_out) of channel slot `ch`."""
        hist = np.zeros(self.taps_per_phase - 1, np.float32)
        i, j = C.c_int64(), C.c_int64()
        self._check(self._L.pv_resample_export_state(self._h, ch, _fp(hist), C.byref(i), C.byref(j)))
        return hist, i.value, j.value

    def import_state(self, ch, hist=None, total_in=-1, total_out=-1):
        if hist is not None:
            hist = np.ascontiguousarray(hist, dtype=np.float32)
            if hist.size != self.taps_per_phase - 1:
                raise ValueError(f"state array of {hist.size} values, {self.taps_per_phase - 1} expected")
        self._check(self._L.pv_resample_import_state(self._h, ch, _fp(hist) if hist is not None else None, int(total_in), int(total_out)))


class _BorrowedStretch(TimeStretch):
    """The stretch handle a PitchStretch owns, seen through the TimeStretch methods (link_channels, export_state / import_state, chain_layout)."""

    def __init__(self, handle, fft_size, analysis_hop, synthesis_hop, max_channels):
        self._bind(handle)
        self.fft_size, self.analysis_hop, self.synthesis_hop = fft_size, analysis_hop, synthesis_hop
        self.max_channels, self.max_frames = max_channels, 1
        self.channels_per_group = 1

    def close(self):
        self._h = C.c_void_p()                          # owned by the pitch handle


class PitchStretch(_Handle):
    """Pitch shifting through the time stretch (pv_pitch_*): a TimeStretch followed by a Resampler at up / down on one stream, the stretched signal
    staying on the device.  Pitch factor down / up, duration factor (synthesis_hop / analysis_hop) (up / down); up = down = 0 means analysis_hop /
    synthesis_hop: constant duration, pitch x synthesis_hop / analysis_hop.  `.stretch` and `.resampler` are the inner handles."""

    _prefix = "pv_pitch"

    def __init__(self, fft_size, analysis_hop, synthesis_hop, up=0, down=0, max_channels=1, max_frames=1, channels_per_group=1, device_id=0):
        self._create(make_pitch_config(fft_size, analysis_hop, synthesis_hop, up, down, max_channels, max_frames, device_id, 0))
        self.fft_size, self.analysis_hop, self.synthesis_hop = fft_size, analysis_hop, synthesis_hop
        self.max_channels = max_channels
        if up == 0 and down == 0:
            up, down = analysis_hop, synthesis_hop
        self.stretch = _BorrowedStretch(self._L.pv_pitch_stretch(self._h), fft_size, analysis_hop, synthesis_hop, max_channels)
        self.resampler = Resampler(up, down, max_channels, _borrowed=self._L.pv_pitch_resampler(self._h))
        if channels_per_group != 1:
            try:
                self.stretch.link_channels(channels_per_group)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.stretch.close()
            self.resampler.close()
        super().close()

    @property
    def latency(self):
        """The output's lag in output samples: ((N - hs) + W) L / M."""
        return ((self.fft_size - self.synthesis_hop) + self.resampler.half_width) * self.resampler.up / self.resampler.down

    def process(self, x):
        """x: float32[nch, nframes * analysis_hop] (host) -> float32[nch, resampler.out_count(nframes * synthesis_hop)]."""
        return self.process_hops(x, None)

    def process_hops(self, x, hops, resets=None):
        """TimeStretch.process_hops (a 1-D or 2-D hop schedule, optional reset flags; hops=None: every hop is analysis_hop), resampled."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, n = x.shape
        ipt, bpt = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        hp, stride = None, 0
        if hops is None:
            nframes = n // self.analysis_hop
            if nframes * self.analysis_hop != n:
                raise ValueError("the input length must be a whole number of analysis hops")
        else:
            h, nframes, stride = TimeStretch._hop_rows(hops)
            if h.ndim == 1 and int(h.astype(np.int64).sum()) != n:
                raise ValueError(f"the input holds {n} samples per channel, the schedule consumes {int(h.astype(np.int64).sum())}")
            if h.ndim == 2 and (h.shape[0] != nch or (nframes and int(h.astype(np.int64).sum(axis=1).max()) > n)):
                raise ValueError("the schedule needs one row per channel, none longer than the input")
            hp = h.ctypes.data_as(ipt)
        rp, rstride = None, 0
        if resets is not None:
            r, rstride = TimeStretch._reset_rows(resets, nframes)
            if r.ndim == 2 and r.shape[0] != nch:
                raise ValueError(f"{r.shape[0]} reset rows for {nch} channels")
            rp = r.ctypes.data_as(bpt)
        cap = self.resampler.out_count(nframes * self.synthesis_hop)
        y = np.empty((nch, cap), np.float32)
        got = C.c_int64()
        if nch and nframes:
            self._check(self._L.pv_pitch_process(self._h, _fp(x), _fp(y), nch, nframes, hp, stride, rp, rstride, n, cap, cap, C.byref(got)))
            assert got.value == cap
        return y

    def process_device(self, d_in, d_out, nch, nframes, in_stride, out_stride, out_capacity, hops=None, resets=None):
        """pv_pitch_process_device on raw device pointers (ints), asynchronous on the handle's stream; hops / resets are host rows as in
        TimeStretch.process_hops_device.  Returns the samples written per channel."""
        hp, stride, rp, rstride = None, 0, None, 0
        if hops is not None:
            h, _, stride = TimeStretch._hop_rows(hops)
            hp = h.ctypes.data_as(C.POINTER(C.c_int32))
        if resets is not None:
            r, rstride = TimeStretch._reset_rows(resets, nframes)
            rp = r.ctypes.data_as(C.POINTER(C.c_uint8))
        got = C.c_int64()
        self._check(self._L.pv_pitch_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), nch, nframes, hp, stride, rp, rstride, in_stride, out_stride,
                                                    out_capacity, C.byref(got)))
        return got.value


def vari_prototype():
    """pv_vari_prototype: the table P float32[8194] the variable-ratio kernel interpolates its weights from (P[q] = h0(q / 256), 0 from q = 8192 on)."""
    L_ = load_library()
    n = L_.pv_vari_prototype(None, 0)
    table = np.zeros(n, np.float32)
    L_.pv_vari_prototype(_fp(table), n)
    return table


def vari_half_width(block, min_count, max_count):
    """pv_vari_half_width: W = ceil(32 max(1, block / min_count)) of a VariResampler config; ValueError for a config pv_vari_create refuses."""
    L_ = load_library()
    w = L_.pv_vari_half_width(int(block), int(min_count), int(max_count))
    if w < 0:
        raise ValueError(L_.pv_vari_last_error(None).decode())
    return int(w)


class VariResampler(_Handle):
    """Variable-ratio band-limited resampler (pv_vari_*): block b of `block` input samples emits counts[b] output samples, min_count <= counts[b] <=
    max_count, so the step block / counts[b] (the pitch factor) changes from block to block.  The output lags by `latency` input samples.  State
    carries across calls: any split of a stream into calls gives the same bits."""

    _prefix = "pv_vari"
    _fft_size_is_value_error = False

    def __init__(self, block, min_count, max_count, max_channels=1, max_blocks=0, device_id=0, _borrowed=None):
        self._owned = _borrowed is None
        if _borrowed is not None:
            self._bind(_borrowed)
        else:
            self._create(make_vari_config(block, min_count, max_count, max_channels, max_blocks, device_id, 0))
        self.block, self.min_count, self.max_count, self.max_channels = block, min_count, max_count, max_channels
        self.half_width = vari_half_width(block, min_count, max_count)
        self.taps = 2 * self.half_width

    @property
    def latency(self):
        """The output's lag in input samples (the half width W)."""
        return self.half_width

    @staticmethod
    def _counts(counts):
        c = np.ascontiguousarray(counts, dtype=np.int32)
        if c.ndim != 1:
            raise ValueError("counts must be int[nblocks]")
        return c

    def process(self, x, counts):
        """x: float32[nch, nblocks * block] (host), counts: int[nblocks] -> float32[nch, counts.sum()] for channel slots 0 .. nch-1."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        c = self._counts(counts)
        nch, nin = x.shape
        if nin != c.size * self.block:
            raise ValueError(f"the input holds {nin} samples per channel, {c.size} blocks of {self.block} consume {c.size * self.block}")
        cap = int(c.astype(np.int64).sum())
        y = np.empty((nch, cap), np.float32)
        n = C.c_int64()
        self._check(self._L.pv_vari_process(self._h, _fp(x), nch, c.size, c.ctypes.data_as(C.POINTER(C.c_int32)), nin, _fp(y), cap, cap, C.byref(n)))
        assert n.value == cap
        return y

    def process_device(self, d_in, nch, counts, in_stride, d_out, out_stride, out_capacity):
        """Raw device pointers (ints), counts a host row.  Asynchronous on the handle's stream; returns the samples written per channel."""
        c = self._counts(counts)
        n = C.c_int64()
        self._check(self._L.pv_vari_process_device(self._h, C.c_void_p(d_in), nch, c.size, c.ctypes.data_as(C.POINTER(C.c_int32)), in_stride, C.c_void_p(d_out),
                                                   out_stride, out_capacity, C.byref(n)))
        return n.value

    def export_state(self, ch):
        """(hist float32[T - 1], blocks, outputs) of channel slot `ch`."""
        hist = np.zeros(self.taps - 1, np.float32)
        i, j = C.c_int64(), C.c_int64()
        self._check(self._L.pv_vari_export_state(self._h, ch, _fp(hist), C.byref(i), C.byref(j)))
        return hist, i.value, j.value

    def import_state(self, ch, hist=None, blocks=-1, outputs=0):
        if hist is not None:
            hist = np.ascontiguousarray(hist, dtype=np.float32)
            if hist.size != self.taps - 1:
                raise ValueError(f"state array of {hist.size} values, {self.taps - 1} expected")
        self._check(self._L.pv_vari_import_state(self._h, ch, _fp(hist) if hist is not None else None, int(blocks), int(outputs)))


class PitchGlide(_Handle):
    """Pitch curves through the time stretch (pv_glide_*): frame m consumes hops[m] input samples and emits hops[m] output samples, shifted in pitch
    by synthesis_hop / hops[m]; min_hop <= hops[m] <= max_hop.  Duration is kept sample for sample.  tempo_hops(1 / pitch, synthesis_hop, min_hop,
    max_hop) turns a per-frame pitch curve into the hop row; the curve acts at output time, `latency` stretched samples behind the content.
    `.stretch` and `.resampler` are the inner handles."""

    _prefix = "pv_glide"

    def __init__(self, fft_size, synthesis_hop, min_hop, max_hop, max_channels=1, max_frames=1, channels_per_group=1, device_id=0):
        self._create(make_glide_config(fft_size, synthesis_hop, min_hop, max_hop, max_channels, max_frames, device_id, 0))
        self.fft_size, self.synthesis_hop, self.min_hop, self.max_hop = fft_size, synthesis_hop, min_hop, max_hop
        self.max_channels = max_channels
        self.stretch = _BorrowedStretch(self._L.pv_glide_stretch(self._h), fft_size, min_hop, synthesis_hop, max_channels)
        self.resampler = VariResampler(synthesis_hop, min_hop, max_hop, max_channels, _borrowed=self._L.pv_glide_resampler(self._h))
        if channels_per_group != 1:
            try:
                self.stretch.link_channels(channels_per_group)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.stretch.close()
            self.resampler.close()
        super().close()

    @property
    def latency(self):
        """The content's lag in samples of the stretched signal: (N - hs) + W."""
        return (self.fft_size - self.synthesis_hop) + self.resampler.half_width

    def _rows(self, hops, resets):
        h = np.ascontiguousarray(hops, dtype=np.int32)
        if h.ndim != 1:
            raise ValueError("hops must be int[nframes]: one row for all channels")
        r, rstride = None, 0
        if resets is not None:
            r, rstride = TimeStretch._reset_rows(resets, h.size)
        return h, r, rstride

    def process(self, x, hops, resets=None):
        """x: float32[nch, hops.sum()] (host), hops: int[nframes], resets: 0 / 1 per frame as TimeStretch.process_hops -> float32 of the shape of x."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nch, n = x.shape
        h, r, rstride = self._rows(hops, resets)
        rp = r.ctypes.data_as(C.POINTER(C.c_uint8)) if r is not None else None
        if int(h.astype(np.int64).sum()) != n:
            raise ValueError(f"the input holds {n} samples per channel, the schedule consumes {int(h.astype(np.int64).sum())}")
        y = np.empty((nch, n), np.float32)
        if nch and h.size:
            self._check(self._L.pv_glide_process(self._h, _fp(x), _fp(y), nch, h.size, h.ctypes.data_as(C.POINTER(C.c_int32)), rp, rstride, n, n))
        return y[0] if one else y

    def process_device(self, d_in, d_out, nch, hops, in_stride, out_stride, resets=None):
        """pv_glide_process_device on raw device pointers (ints), asynchronous on the handle's stream; hops / resets are host rows."""
        h, r, rstride = self._rows(hops, resets)
        rp = r.ctypes.data_as(C.POINTER(C.c_uint8)) if r is not None else None
        self._check(self._L.pv_glide_process_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), nch, h.size, h.ctypes.data_as(C.POINTER(C.c_int32)), rp, rstride,
                                                    in_stride, out_stride))

    def process_tuned(self, x, sample_rate, scale_mask=0xFFF, strength=1.0, retune=1.0, tracker=None, threshold=2458, a4=440.0, shift=0):
        """Offline pitch correction onto a scale, the counterpart of TimeStretch.process_transients: F0Tracker.track (channel 0: the glide has one row
        for all channels) -> tune_plan -> process.  x: float32[nch, n] (host).  tracker: an F0Tracker, default window = max_lag = fft_size, hop =
        synthesis_hop, min_lag = 32.  shift: the caller's compensation for the content lag, in input samples.  Returns (y of the shape of
        x[:, :hops.sum()], hops)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        own = tracker is None
        if own:
            tracker = F0Tracker(min(self.fft_size, 4096), self.synthesis_hop, 32, min(self.fft_size, 4096))
        try:
            records = tracker.track(x[0], threshold)[0]
        finally:
            if own:
                tracker.close()
        hops = tune_plan(records, tracker.hop, sample_rate, self.synthesis_hop, self.min_hop, self.max_hop, x.shape[1], scale_mask=scale_mask, strength=strength,
                         retune=retune, a4=a4, shift=shift, f0_center=(tracker.window + tracker.max_lag) // 2)
        y = self.process(x[:, :int(hops.astype(np.int64).sum())], hops)
        return (y[0] if one else y), hops


def f0_period(records):
    """pv_f0_period: float64 periods in samples of int32[..., 4] records (F0Tracker.track); 0 for an unvoiced or empty record."""
    L = load_library()
    r = np.ascontiguousarray(records, dtype=np.int32)
    if r.ndim < 1 or r.shape[-1] != 4:
        raise ValueError("records must be int32[..., 4]")
    flat = r.reshape(-1, 4)
    out = np.empty(flat.shape[0], np.float64)
    ip = C.POINTER(C.c_int32)
    for i in range(flat.shape[0]):
        out[i] = L.pv_f0_period(flat[i].ctypes.data_as(ip))
    return out.reshape(r.shape[:-1])


def tune_plan(records, f0_hop, sample_rate, synthesis_hop, min_hop, max_hop, input_len, scale_mask=0xFFF, strength=1.0, retune=1.0, a4=440.0, shift=0,
              f0_center=0, curve=False):
    """pv_tune_plan: the int32 hop row of PitchGlide.process that moves every frame onto the nearest allowed note.  records: int32[nrec, 4] of ONE
    channel; scale_mask: bit k = pitch class k (C = 0); strength 0 .. 1; retune (0, 1], the one-pole speed per frame; f0_center: where in its span a
    record sits, normally (window + max_lag) // 2.  curve=True returns (hops, float64 shift per frame in octaves)."""
    L = load_library()
    r = np.ascontiguousarray(records, dtype=np.int32)
    if r.size and (r.ndim != 2 or r.shape[1] != 4):
        raise ValueError("records must be int32[nrec, 4]: one channel")
    nrec = r.shape[0] if r.size else 0
    p = make_tune_params(f0_hop, f0_center, float(sample_rate), synthesis_hop, min_hop, max_hop, int(input_len), scale_mask, float(strength), float(retune), float(a4),
                         int(shift))
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rp = r.ctypes.data_as(ip) if nrec else None
    n = L.pv_tune_plan(C.byref(p), rp, nrec, None, None, 0)
    if n < 0:
        raise ValueError("tune_plan: bad argument (scale_mask 1 .. 0xFFF, strength 0 .. 1, retune (0, 1], 1 <= min_hop <= max_hop, positive rates)")
    hops, r_row = np.zeros(n, np.int32), np.zeros(n, np.float64)
    if n:
        L.pv_tune_plan(C.byref(p), rp, nrec, hops.ctypes.data_as(ip), r_row.ctypes.data_as(dp), n)
    return (hops, r_row) if curve else hops


class F0Tracker(_Handle):
    """The fundamental-frequency tracker (pv_f0_*): YIN on block-scaled integers.  Frame m of a channel reads x[m hop, m hop + window + max_lag) and
    gives one record int32[4] = {lag, c(lag - 1), c(lag), c(lag + 1)}, lag < 0 for an unvoiced frame and all zeros for silence or a non-finite sample;
    f0_period turns records into periods.  Stateless: a stream analysed in pieces overlaps them by window + max_lag - hop samples."""

    _prefix = "pv_f0"

    def __init__(self, window, hop, min_lag, max_lag, max_channels=1, max_frames=0, device_id=0):
        self._create(make_f0_config(window, hop, min_lag, max_lag, max_channels, max_frames, device_id, 0))
        self.window, self.hop, self.min_lag, self.max_lag, self.max_channels = window, hop, min_lag, max_lag, max_channels

    def reset(self):
        """Nothing to reset: the tracker carries no state."""

    def frames(self, n):
        """How many frames fit n samples per channel."""
        return max((n - self.window - self.max_lag) // self.hop + 1, 0)

    def track(self, x, threshold=2458):
        """x: float32[nch, n] (host) -> int32[nch, frames(n), 4]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, n = x.shape
        nframes = self.frames(n)
        rec = np.zeros((nch, nframes, 4), np.int32)
        self._check(self._L.pv_f0_track(self._h, _fp(x), nch, nframes, n, int(threshold), rec.ctypes.data_as(C.POINTER(C.c_int32)), nframes))
        return rec

    def track_device(self, d_in, nch, nframes, in_stride, d_records, rec_stride, threshold=2458):
        """pv_f0_track_device on raw device pointers (ints), asynchronous on the handle's stream; rec_stride counts records."""
        self._check(self._L.pv_f0_track_device(self._h, C.c_void_p(d_in), nch, nframes, in_stride, int(threshold), C.c_void_p(d_records), rec_stride))


def contour_path(candidates, max_lag, bias=1024, unvoiced_cost=2458, voicing_cost=2458, jump_cost=16384, states=False):
    """pv_contour_path: the f0 records int32[nrec, 4] of the cheapest path through the candidate table int32[nrec, K, 4] of ONE channel
    (ContourTracker.candidates): per frame the states are its occupied slots and the unvoiced state K; unvoiced_cost is what a frame pays for being
    called unvoiced while it has a candidate, voicing_cost what a change of voicing costs and jump_cost what a relative change of the period of 1 costs
    (an octave: two thirds of it).  states=True returns (records, int32[nrec] state per frame)."""
    L = load_library()
    c = np.ascontiguousarray(candidates, dtype=np.int32)
    if c.ndim != 3 or c.shape[2] != 4 or not 1 <= c.shape[1] <= 8:
        raise ValueError("candidates must be int32[nrec, K, 4] with K in 1 .. 8: one channel")
    nrec, K = c.shape[0], c.shape[1]
    p = make_contour_params(K, int(max_lag), int(bias), int(unvoiced_cost), int(voicing_cost), int(jump_cost))
    ip = C.POINTER(C.c_int32)
    rec, st = np.zeros((nrec, 4), np.int32), np.zeros(nrec, np.int32)
    rc = L.pv_contour_path(C.byref(p), c.ctypes.data_as(ip) if nrec else None, nrec, rec.ctypes.data_as(ip) if nrec else None,
                           st.ctypes.data_as(ip) if states and nrec else None)
    if rc == PV_ERR_DEVICE:
        raise MemoryError("contour_path: out of host memory")
    if rc != PV_OK:
        raise ValueError("contour_path: bad argument (max_lag 3 .. 4096, bias 0 .. 16384, unvoiced_cost 1 .. 16384, voicing_cost and jump_cost 0 .. 2^20, "
                         "0 <= tau <= 65535 and c values >= 0 in the table)")
    return (rec, st) if states else rec


class ContourTracker(_Handle):
    """The pitch contour tracker (pv_contour_*): per frame the K best dips of YIN's c curve on block-scaled integers (candidates), and contour_path
    through them (track).  track gives F0Tracker.track's records, so a ContourTracker goes wherever a tracker is taken:
    Psola(...).process_tuned(x, rate, tracker=ContourTracker(...)).  Frame m of a channel reads x[m hop, m hop + window + max_lag).  Stateless: the
    candidates of a stream analysed in pieces overlap by window + max_lag - hop samples; the path is per call."""

    _prefix = "pv_contour"

    def __init__(self, window, hop, min_lag, max_lag, candidates=8, max_channels=1, max_frames=0, device_id=0, bias=1024, voicing_cost=2458, jump_cost=16384):
        self._create(make_contour_config(window, hop, min_lag, max_lag, candidates, max_channels, max_frames, device_id, 0))
        self.window, self.hop, self.min_lag, self.max_lag, self.max_channels = window, hop, min_lag, max_lag, max_channels
        self.K = candidates if candidates else 8
        self.bias, self.voicing_cost, self.jump_cost = bias, voicing_cost, jump_cost

    def reset(self):
        """Nothing to reset: the tracker carries no state."""

    def frames(self, n):
        """How many frames fit n samples per channel."""
        return max((n - self.window - self.max_lag) // self.hop + 1, 0)

    def candidates(self, x, bias=None):
        """x: float32[nch, n] (host) -> int32[nch, frames(n), K, 4]: slot k = {lag, c(lag - 1), c(lag), c(lag + 1)} of the dip with the k-th smallest key,
        zeros beyond the number of dips."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, n = x.shape
        nframes = self.frames(n)
        cand = np.zeros((nch, nframes, self.K, 4), np.int32)
        self._check(self._L.pv_contour_track(self._h, _fp(x), nch, nframes, n, int(self.bias if bias is None else bias),
                                             cand.ctypes.data_as(C.POINTER(C.c_int32)), nframes))
        return cand

    def track(self, x, threshold=2458):
        """x: float32[nch, n] (host) -> int32[nch, frames(n), 4], F0Tracker.track's records: the candidates, then one path per channel with `threshold` as
        the unvoiced cost."""
        cand = self.candidates(x)
        return np.stack([contour_path(c, self.max_lag, self.bias, threshold, self.voicing_cost, self.jump_cost) for c in cand]).reshape(cand.shape[0], -1, 4)

    def track_device(self, d_in, nch, nframes, in_stride, d_candidates, cand_stride, bias=None):
        """pv_contour_track_device on raw device pointers (ints), asynchronous on the handle's stream; cand_stride counts frames."""
        self._check(self._L.pv_contour_track_device(self._h, C.c_void_p(d_in), nch, nframes, in_stride, int(self.bias if bias is None else bias),
                                                    C.c_void_p(d_candidates), cand_stride))


def psola_window():
    """pv_psola_window: the window table Hn float32[1026] of the overlap-add kernel, Hn[q] = (1 + cos(pi q / 1024)) / 2 for q < 1024 and two zeros."""
    L_ = load_library()
    n = L_.pv_psola_window(None, 0)
    table = np.zeros(n, np.float32)
    L_.pv_psola_window(_fp(table), n)
    return table


def _one_channel_records(records):
    r = np.ascontiguousarray(records, dtype=np.int32)
    if r.size and (r.ndim != 2 or r.shape[1] != 4):
        raise ValueError("records must be int32[nrec, 4]: one channel")
    return r, (r.shape[0] if r.size else 0)


def tune_ratios(records, sample_rate, scale_mask=0xFFF, strength=1.0, retune=1.0, a4=440.0):
    """pv_psola_ratios: one pitch ratio (float64, within [1/2, 2]) per f0 record of ONE channel: the target rule of tune_plan with the one-pole running
    per record; 1 where a record is unvoiced and the pole has settled."""
    L = load_library()
    r, nrec = _one_channel_records(records)
    p = make_tune_params(0, 0, float(sample_rate), 0, 0, 0, 0, scale_mask, float(strength), float(retune), float(a4), 0)
    out = np.zeros(nrec, np.float64)
    n = L.pv_psola_ratios(C.byref(p), r.ctypes.data_as(C.POINTER(C.c_int32)) if nrec else None, nrec, out.ctypes.data_as(C.POINTER(C.c_double)) if nrec else None, nrec)
    if n < 0:
        raise ValueError("tune_ratios: bad argument (scale_mask 1 .. 0xFFF, strength 0 .. 1, retune (0, 1], positive rates)")
    return out


def psola_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None):
    """pv_psola_plan: the grain table int32[ngrains, 4] = {t, tf, dq, L} of Psola.process that moves every voiced stretch of ONE channel's records by
    its ratio (float64[nrec] within [1/2, 2]; None: 1 everywhere) and passes unvoiced stretches unshifted."""
    L = load_library()
    r, nrec = _one_channel_records(records)
    rho = None
    if ratios is not None:
        rho = np.ascontiguousarray(ratios, dtype=np.float64)
        if rho.shape != (nrec,):
            raise ValueError("ratios must be float64[nrec]")
    p = make_psola_params(int(f0_hop), int(f0_center), int(input_len), float(unvoiced_period), int(min_period), int(max_period))
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rp = r.ctypes.data_as(ip) if nrec else None
    qp = rho.ctypes.data_as(dp) if rho is not None and nrec else None
    n = L.pv_psola_plan(C.byref(p), rp, nrec, qp, None, 0)
    if n < 0:
        raise ValueError("psola_plan: bad argument (2 <= min_period <= unvoiced_period <= max_period <= 4096, ratios within [1/2, 2], 0 <= input_len < 2^30)")
    grains = np.zeros((n, 4), np.int32)
    if n:
        L.pv_psola_plan(C.byref(p), rp, nrec, qp, grains.ctypes.data_as(ip), n)
    return grains


class Psola(_Handle):
    """Pitch-synchronous overlap-add (pv_psola_*): formant-preserving pitch correction of a monophonic voice.  A grain int32[4] = {t, tf, dq, L} is a
    Hann window of half length L centred at output position t + tf / 256 over the input shifted by dq / 256 samples; one table serves every channel.
    Stateless: outputs [out_first, out_first + nout) are a pure function of (x, grains), and any partition of the range gives the same bits."""

    _prefix = "pv_psola"
    _fft_size_is_value_error = False

    def __init__(self, max_period, max_channels=1, max_outputs=0, device_id=0):
        self._create(make_psola_config(max_period, max_channels, max_outputs, device_id, 0))
        self.max_period, self.max_channels = max_period, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no signal state."""

    @staticmethod
    def _grains(grains):
        g = np.ascontiguousarray(grains, dtype=np.int32)
        if g.size and (g.ndim != 2 or g.shape[1] != 4):
            raise ValueError("grains must be int32[ngrains, 4]")
        return g, (g.shape[0] if g.size else 0)

    def process(self, x, grains, out_first=0, nout=None):
        """x: float32[nch, n] (host), grains: int32[ngrains, 4] -> float32[nch, nout], outputs out_first .. out_first + nout - 1 (default: all n)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nch, n = x.shape
        g, ng = self._grains(grains)
        nout = n - out_first if nout is None else int(nout)
        y = np.zeros((nch, max(nout, 0)), np.float32)
        self._check(self._L.pv_psola_process(self._h, _fp(x), n, n, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng, _fp(y), int(out_first), nout,
                                             max(nout, 0)))
        return y[0] if one else y

    def process_device(self, d_in, nin, in_stride, nch, grains, d_out, out_first, nout, out_stride):
        """pv_psola_process_device on raw device pointers (ints), asynchronous on the handle's stream; grains is a host table."""
        g, ng = self._grains(grains)
        self._check(self._L.pv_psola_process_device(self._h, C.c_void_p(d_in), nin, in_stride, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng,
                                                    C.c_void_p(d_out), out_first, nout, out_stride))

    def process_tuned(self, x, sample_rate, scale_mask=0xFFF, strength=1.0, retune=1.0, tracker=None, threshold=2458, a4=440.0, epochs=False):
        """Offline formant-preserving pitch correction onto a scale: F0Tracker.track (channel 0: one plan for all channels) -> tune_ratios -> psola_plan
        -> process.  x: float32[nch, n] (host).  tracker: an F0Tracker, default window 1024, hop 256, min_lag 32 and max_lag = max_period.  epochs=True
        puts the analysis marks on the pitch pulses: an EpochTracker at the tracker's hop (longest period min(max_lag, 2048, span // 2), window twice
        that, span = the tracker's window + max_lag) -> epoch_plan in place of psola_plan.  Returns (y of the shape of x, grains)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        own = tracker is None
        if own:
            max_lag = max(self.max_period, 3)
            tracker = F0Tracker(1024, 256, max(2, min(32, max_lag // 2)), max_lag)
        try:
            records = tracker.track(x[0], threshold)[0]
        finally:
            if own:
                tracker.close()
        ratios = tune_ratios(records, sample_rate, scale_mask=scale_mask, strength=strength, retune=retune, a4=a4)
        min_period = tracker.min_lag
        plan_args = (records, tracker.hop, (tracker.window + tracker.max_lag) // 2, x.shape[1], float(min(max(256, min_period), self.max_period)), min_period,
                     self.max_period, ratios)
        if epochs:
            longest = min(tracker.max_lag, 2048, (tracker.window + tracker.max_lag) // 2)
            marks = EpochTracker(2 * longest, tracker.hop, longest)
            try:
                found = marks.track(x[0], epoch_periods(records))[0]
            finally:
                marks.close()
            grains = epoch_plan(*plan_args, epochs=found)
        else:
            grains = psola_plan(*plan_args)
        y = self.process(x, grains)
        return (y[0] if one else y), grains


def epoch_periods(records):
    """pv_epoch_periods: the int32 period row of EpochTracker.track from the f0 records int32[nrec, 4] of ONE channel: floor(256 period + 1/2), 0 where
    a record is unvoiced or empty."""
    L = load_library()
    r, nrec = _one_channel_records(records)
    out = np.zeros(nrec, np.int32)
    ip = C.POINTER(C.c_int32)
    if L.pv_epoch_periods(r.ctypes.data_as(ip) if nrec else None, nrec, out.ctypes.data_as(ip) if nrec else None, nrec) != nrec:
        raise ValueError("epoch_periods: bad argument")
    return out


def epoch_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, epochs=None, min_strength=0, lock=0.125):
    """pv_epoch_plan: psola_plan with the analysis marks on the pitch pulses.  epochs: int32[nrec, 4] of EpochTracker.track run at the tracker's hop on the
    same buffer (record j belongs to f0 record j), or None: then the grains are psola_plan's.  min_strength 0 .. 16384: weaker records leave their marks
    alone; lock (0, 1]: how much of a small correction one mark takes."""
    L = load_library()
    r, nrec = _one_channel_records(records)
    rho = None
    if ratios is not None:
        rho = np.ascontiguousarray(ratios, dtype=np.float64)
        if rho.shape != (nrec,):
            raise ValueError("ratios must be float64[nrec]")
    ep = None
    if epochs is not None:
        ep = np.ascontiguousarray(epochs, dtype=np.int32)
        if ep.shape != (nrec, 4) and not (nrec == 0 and ep.size == 0):
            raise ValueError("epochs must be int32[nrec, 4]: one record per f0 record")
    p = make_psola_params(int(f0_hop), int(f0_center), int(input_len), float(unvoiced_period), int(min_period), int(max_period))
    e = make_epoch_params(int(min_strength), float(lock))
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rp = r.ctypes.data_as(ip) if nrec else None
    qp = rho.ctypes.data_as(dp) if rho is not None and nrec else None
    ep_ = ep.ctypes.data_as(ip) if ep is not None and nrec else None
    n = L.pv_epoch_plan(C.byref(p), C.byref(e), rp, nrec, qp, ep_, None, 0)
    if n < 0:
        raise ValueError("epoch_plan: bad argument (psola_plan's ranges, 0 <= min_strength <= 16384, 0 < lock <= 1)")
    grains = np.zeros((n, 4), np.int32)
    if n:
        L.pv_epoch_plan(C.byref(p), C.byref(e), rp, nrec, qp, ep_, grains.ctypes.data_as(ip), n)
    return grains


class EpochTracker(_Handle):
    """The epoch records (pv_epoch_*): where in a frame the pitch pulses sit.  Frame m of a channel reads x[m hop, m hop + window) and the period
    periods256[m] in 1/256 sample (one row for all channels; epoch_periods makes it from f0 records) and gives one record int32[4] =
    {position of the first pulse found, teeth summed, quarter period, strength 0 .. 16384}; all zeros for silence, a non-finite sample or a period outside
    [8, max_period].  Stateless: a stream analysed in pieces overlaps them by window - hop samples."""

    _prefix = "pv_epoch"
    _fft_size_is_value_error = False

    def __init__(self, window, hop, max_period, max_channels=1, max_frames=256, device_id=0):
        self._create(make_epoch_config(window, hop, max_period, max_channels, max_frames, device_id, 0))
        self.window, self.hop, self.max_period, self.max_channels = window, hop, max_period, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no state."""

    def frames(self, n):
        """How many frames fit n samples per channel."""
        return max((n - self.window) // self.hop + 1, 0)

    def track(self, x, periods256):
        """x: float32[nch, n] (host), periods256: int32[nframes] with nframes <= frames(n) -> int32[nch, nframes, 4]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        nch, n = x.shape
        per = np.ascontiguousarray(periods256, dtype=np.int32)
        if per.ndim != 1 or per.size > self.frames(n):
            raise ValueError("periods256 must be int32[nframes] with nframes <= frames(n)")
        nframes = per.size
        rec = np.zeros((nch, nframes, 4), np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self._L.pv_epoch_track(self._h, _fp(x), nch, nframes, n, per.ctypes.data_as(ip), rec.ctypes.data_as(ip), nframes))
        return rec

    def track_device(self, d_in, nch, nframes, in_stride, d_periods256, d_records, rec_stride):
        """pv_epoch_track_device on raw device pointers (ints), asynchronous on the handle's stream; rec_stride counts records."""
        self._check(self._L.pv_epoch_track_device(self._h, C.c_void_p(d_in), nch, nframes, in_stride, C.c_void_p(d_periods256), C.c_void_p(d_records), rec_stride))


def tsm_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, epochs=None, min_strength=0, lock=0.125):
    """pv_tsm_plan: (far grains int32[ngrains, 4] = {t, tf + 256 phi, D, L} of Tsm.process, output_len).  epoch_plan with a read position beside the
    synthesis position: rates float64[nrec], the input samples consumed per output sample while the read position lies on record j (2: twice as fast,
    1/2: half speed; finite and positive, held within [1/4, 4]; None: 1, and then the grains are epoch_plan's in the far notation)."""
    return _far_plan(None, records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios, rates, epochs, min_strength, lock)


def mirror_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, epochs=None, min_strength=0, lock=0.125,
                mirror=True):
    """pv_mirror_plan: (grains int32[ngrains, 4] = {t, tf + 256 phi + 65536 m, D, L} of Mirror.process, output_len).  tsm_plan with the time direction of
    every grain: with mirror=True every second use of an unvoiced analysis mark reads the input backwards about that mark (m = 1), which takes the buzz
    out of noise repeated at rates below 1; voiced grains are never mirrored.  mirror=False: tsm_plan's grains bit for bit."""
    return _far_plan(bool(mirror), records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios, rates, epochs, min_strength, lock)


def formant_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, warps=None, epochs=None, min_strength=0,
                 lock=0.125):
    """pv_formant_plan: (grains int32[ngrains, 4] = {t, tf + 256 phi + 131072 z, D, L} of Formant.process, output_len).  tsm_plan with one more row:
    warps float64[nrec], the step of the grains of record j within [1/2, 2] (above 1 the formants move up); z is the step in 1/256, 0 where it is 256, and a
    grain's half length starts from period / step.  warps=None: tsm_plan's grains bit for bit."""
    return _far_plan(None, records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios, rates, epochs, min_strength, lock, warps, True)


def choir_plan(records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios=None, rates=None, warps=None, epochs=None, min_strength=0,
               lock=0.125, mirror=True):
    """pv_choir_plan: (grains int32[ngrains, 4] = {t, tf + 256 phi + 65536 m + 131072 z, D, L} of one voice of Choir.process, output_len).  mirror_plan with
    formant_plan's row warps: warps=None gives mirror_plan's grains bit for bit, mirror=False formant_plan's.  With both, every grain takes its step and its
    half length from formant_plan's rule and a reuse of an unvoiced mark its direction, D and phi from mirror_plan's, so a mirrored warped grain reads
    about its own mark."""
    return _far_plan(bool(mirror), records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios, rates, epochs, min_strength, lock, warps,
                     choir=True)


def _far_plan(mirror, records, f0_hop, f0_center, input_len, unvoiced_period, min_period, max_period, ratios, rates, epochs, min_strength, lock, warps=None,
              formant=False, choir=False):
    """The body of tsm_plan (mirror is None: pv_tsm_plan), of mirror_plan (pv_mirror_plan with that mirror argument), of formant_plan (formant: pv_formant_plan
    with the row warps) and of choir_plan (choir: pv_choir_plan with both)."""
    L = load_library()
    r, nrec = _one_channel_records(records)
    rows = []
    for name, row in (("ratios", ratios), ("rates", rates), ("warps", warps)):
        if row is not None:
            row = np.ascontiguousarray(row, dtype=np.float64)
            if row.shape != (nrec,):
                raise ValueError(f"{name} must be float64[nrec]")
        rows.append(row)
    rho, spd, wrp = rows
    ep = None
    if epochs is not None:
        ep = np.ascontiguousarray(epochs, dtype=np.int32)
        if ep.shape != (nrec, 4) and not (nrec == 0 and ep.size == 0):
            raise ValueError("epochs must be int32[nrec, 4]: one record per f0 record")
    p = make_psola_params(int(f0_hop), int(f0_center), int(input_len), float(unvoiced_period), int(min_period), int(max_period))
    e = make_epoch_params(int(min_strength), float(lock))
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rp = r.ctypes.data_as(ip) if nrec else None
    qp = rho.ctypes.data_as(dp) if rho is not None and nrec else None
    sp = spd.ctypes.data_as(dp) if spd is not None and nrec else None
    ep_ = ep.ctypes.data_as(ip) if ep is not None and nrec else None
    out_len = C.c_int64(0)
    if choir:
        wp = wrp.ctypes.data_as(dp) if wrp is not None and nrec else None
        name, plan = "choir_plan", lambda out, cap: L.pv_choir_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, int(mirror), out, cap, C.byref(out_len))
    elif formant:
        wp = wrp.ctypes.data_as(dp) if wrp is not None and nrec else None
        name, plan = "formant_plan", lambda out, cap: L.pv_formant_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, wp, ep_, out, cap, C.byref(out_len))
    elif mirror is None:
        name, plan = "tsm_plan", lambda out, cap: L.pv_tsm_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, ep_, out, cap, C.byref(out_len))
    else:
        name, plan = "mirror_plan", lambda out, cap: L.pv_mirror_plan(C.byref(p), C.byref(e), rp, nrec, qp, sp, ep_, int(mirror), out, cap, C.byref(out_len))
    n = plan(None, 0)
    if n < 0:
        raise ValueError(f"{name}: bad argument (epoch_plan's ranges, rates finite and positive, and the output must end below 2^30)")
    grains = np.zeros((n, 4), np.int32)
    if n:
        plan(grains.ctypes.data_as(ip), n)
    return grains, int(out_len.value)


class Tsm(_Handle):
    """Time-scale modification by pitch-synchronous overlap-add (pv_tsm_*): the tempo of a monophonic voice changes, pitch and formants stay (and the pitch
    may be corrected in the same pass).  A far grain int32[4] = {t, tf + 256 phi, D, L} is a Hann window of half length L centred at output position
    t + tf / 256 that reads the input at n - D - phi / 256, anywhere; one table serves every channel.  A tile of 1024 outputs may read
    max_rate (1024 + 2 max_period) + 4 max_period + 64 input samples: tsm_plan's tables at rates within [1 / max_rate, max_rate] keep to that.  Stateless:
    outputs [out_first, out_first + nout) are a pure function of (x, grains), and any partition of the range gives the same bits; on a table that reads near
    where it writes they are Psola.process's bits."""

    _prefix = "pv_tsm"
    _fft_size_is_value_error = False

    def __init__(self, max_period, max_rate=2, max_channels=1, max_outputs=0, device_id=0):
        self._create(make_tsm_config(max_period, max_rate, max_channels, max_outputs, device_id, 0))
        self.max_period, self.max_rate, self.max_channels = max_period, max_rate, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no signal state."""

    _grains = staticmethod(Psola._grains)

    def process(self, x, grains, out_first=0, nout=None):
        """x: float32[nch, n] (host), grains: int32[ngrains, 4] -> float32[nch, nout], outputs out_first .. out_first + nout - 1 (default: n - out_first; pass
        tsm_plan's output_len for a whole stretched signal)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nch, n = x.shape
        g, ng = self._grains(grains)
        nout = n - out_first if nout is None else int(nout)
        y = np.zeros((nch, max(nout, 0)), np.float32)
        self._check(self._L.pv_tsm_process(self._h, _fp(x), n, n, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng, _fp(y), int(out_first), nout,
                                           max(nout, 0)))
        return y[0] if one else y

    def process_device(self, d_in, nin, in_stride, nch, grains, d_out, out_first, nout, out_stride):
        """pv_tsm_process_device on raw device pointers (ints), asynchronous on the handle's stream; grains is a host table."""
        g, ng = self._grains(grains)
        self._check(self._L.pv_tsm_process_device(self._h, C.c_void_p(d_in), nin, in_stride, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng,
                                                  C.c_void_p(d_out), out_first, nout, out_stride))

    def process_tuned(self, x, sample_rate, rate=1.0, scale_mask=0xFFF, strength=1.0, retune=1.0, tracker=None, threshold=2458, a4=440.0, epochs=False):
        """Offline tempo change of a monophonic voice: F0Tracker.track (channel 0: one plan for all channels) -> tune_ratios -> tsm_plan -> process.
        rate: the input samples consumed per output sample, one number or one per f0 record (float64[nrec]: a tempo curve); 1/2 is half speed.
        The voice is corrected onto the scale in the same pass, as Psola.process_tuned does; strength = 0 leaves the pitch alone.  tracker and epochs as
        there.  x: float32[nch, n] (host).  Returns (y float32[nch, output_len], grains)."""
        return _process_tuned(self, tsm_plan, x, sample_rate, rate, scale_mask, strength, retune, tracker, threshold, a4, epochs)


def _process_tuned(self, plan, x, sample_rate, rate, scale_mask, strength, retune, tracker, threshold, a4, epochs):
    """Tsm.process_tuned and Mirror.process_tuned: track, tune_ratios, `plan` (tsm_plan's arguments), process."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    one = x.ndim == 1
    if one:
        x = x[None, :]
    own = tracker is None
    if own:
        max_lag = max(self.max_period, 3)
        tracker = F0Tracker(1024, 256, max(2, min(32, max_lag // 2)), max_lag)
    try:
        records = tracker.track(x[0], threshold)[0]
    finally:
        if own:
            tracker.close()
    nrec = records.shape[0]
    ratios = tune_ratios(records, sample_rate, scale_mask=scale_mask, strength=strength, retune=retune, a4=a4)
    rates = np.full(nrec, float(rate)) if np.ndim(rate) == 0 else np.ascontiguousarray(rate, dtype=np.float64)
    if rates.shape != (nrec,):
        raise ValueError(f"rate must be one number or one per f0 record ({nrec})")
    min_period = tracker.min_lag
    found = None
    if epochs:
        longest = min(tracker.max_lag, 2048, (tracker.window + tracker.max_lag) // 2)
        marks = EpochTracker(2 * longest, tracker.hop, longest)
        try:
            found = marks.track(x[0], epoch_periods(records))[0]
        finally:
            marks.close()
    grains, output_len = plan(records, tracker.hop, (tracker.window + tracker.max_lag) // 2, x.shape[1], float(min(max(256, min_period), self.max_period)), min_period,
                              self.max_period, ratios=ratios, rates=rates, epochs=found)
    y = self.process(x, grains, 0, output_len)
    return (y[0] if one else y), grains


class Mirror(_Handle):
    """Overlap-add of grains that read the input in either time direction (pv_mirror_*): Tsm with one more bit per grain.  A grain int32[4] =
    {t, tf + 256 phi + 65536 m, D, L}; with m = 0 it is Tsm's far grain (and a table without mirrored grains gives Tsm.process's bits), with m = 1 it
    reads the input at D - n - phi / 256: backwards.  mirror_plan mirrors every second use of an unvoiced analysis mark, which takes the buzz out of
    noise repeated at rates below 1.  The span, the LDS rule and the partition invariance are Tsm's."""

    _prefix = "pv_mirror"
    _fft_size_is_value_error = False

    def __init__(self, max_period, max_rate=2, max_channels=1, max_outputs=0, device_id=0):
        self._create(make_mirror_config(max_period, max_rate, max_channels, max_outputs, device_id, 0))
        self.max_period, self.max_rate, self.max_channels = max_period, max_rate, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no signal state."""

    _grains = staticmethod(Psola._grains)

    def process(self, x, grains, out_first=0, nout=None):
        """x: float32[nch, n] (host), grains: int32[ngrains, 4] -> float32[nch, nout], outputs out_first .. out_first + nout - 1 (default: n - out_first; pass
        mirror_plan's output_len for a whole stretched signal)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nch, n = x.shape
        g, ng = self._grains(grains)
        nout = n - out_first if nout is None else int(nout)
        y = np.zeros((nch, max(nout, 0)), np.float32)
        self._check(self._L.pv_mirror_process(self._h, _fp(x), n, n, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng, _fp(y), int(out_first), nout,
                                              max(nout, 0)))
        return y[0] if one else y

    def process_device(self, d_in, nin, in_stride, nch, grains, d_out, out_first, nout, out_stride):
        """pv_mirror_process_device on raw device pointers (ints), asynchronous on the handle's stream; grains is a host table."""
        g, ng = self._grains(grains)
        self._check(self._L.pv_mirror_process_device(self._h, C.c_void_p(d_in), nin, in_stride, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng,
                                                     C.c_void_p(d_out), out_first, nout, out_stride))

    def process_tuned(self, x, sample_rate, rate=1.0, mirror=True, scale_mask=0xFFF, strength=1.0, retune=1.0, tracker=None, threshold=2458, a4=440.0, epochs=False):
        """Tsm.process_tuned with mirror_plan in place of tsm_plan: at rates below 1 the repeated unvoiced grains alternate their time direction.
        mirror=False plans as Tsm.process_tuned does.  Returns (y float32[nch, output_len], grains)."""
        def plan(*args, **kw):
            return mirror_plan(*args, mirror=mirror, **kw)
        return _process_tuned(self, plan, x, sample_rate, rate, scale_mask, strength, retune, tracker, threshold, a4, epochs)


class Formant(_Handle):
    """Formant shifting on the overlap-add path (pv_formant_*): Tsm with a step per grain.  A grain int32[4] = {t, tf + 256 phi + 131072 z, D, L}; z is the
    step s in 1/256 (0: 256; else 128 .. 512).  With s = 256 it is Tsm's far grain (and a table without warped grains gives Tsm.process's bits); otherwise
    the grain reads s / 256 input samples per output sample about its centre, which moves its spectral envelope by s / 256 while the grain spacing still
    sets the pitch.  formant_plan writes the steps from one warp per f0 record.  The span is wider than Tsm's (max_rate (1024 + 2 max_period) +
    6 max_period + 192), so fewer (max_period, max_rate) pairs fit the LDS; the partition invariance is Tsm's."""

    _prefix = "pv_formant"
    _fft_size_is_value_error = False

    def __init__(self, max_period, max_rate=2, max_channels=1, max_outputs=0, device_id=0):
        self._create(make_formant_config(max_period, max_rate, max_channels, max_outputs, device_id, 0))
        self.max_period, self.max_rate, self.max_channels = max_period, max_rate, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no signal state."""

    _grains = staticmethod(Psola._grains)

    def process(self, x, grains, out_first=0, nout=None):
        """x: float32[nch, n] (host), grains: int32[ngrains, 4] -> float32[nch, nout], outputs out_first .. out_first + nout - 1 (default: n - out_first; pass
        formant_plan's output_len for a whole signal)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nch, n = x.shape
        g, ng = self._grains(grains)
        nout = n - out_first if nout is None else int(nout)
        y = np.zeros((nch, max(nout, 0)), np.float32)
        self._check(self._L.pv_formant_process(self._h, _fp(x), n, n, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng, _fp(y), int(out_first), nout,
                                               max(nout, 0)))
        return y[0] if one else y

    def process_device(self, d_in, nin, in_stride, nch, grains, d_out, out_first, nout, out_stride):
        """pv_formant_process_device on raw device pointers (ints), asynchronous on the handle's stream; grains is a host table."""
        g, ng = self._grains(grains)
        self._check(self._L.pv_formant_process_device(self._h, C.c_void_p(d_in), nin, in_stride, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng,
                                                      C.c_void_p(d_out), out_first, nout, out_stride))

    def process_tuned(self, x, sample_rate, warp=1.0, rate=1.0, scale_mask=0xFFF, strength=1.0, retune=1.0, tracker=None, threshold=2458, a4=440.0, epochs=False):
        """Tsm.process_tuned with formant_plan in place of tsm_plan.  warp: the factor the formants move by, within [1/2, 2], one number or one per f0 record
        (float64[nrec]); warp=1.0 plans as Tsm.process_tuned does and gives its bits.  Returns (y float32[nch, output_len], grains)."""
        def plan(records, *args, **kw):
            nrec = np.asarray(records).reshape(-1, 4).shape[0]
            warps = np.full(nrec, float(warp)) if np.ndim(warp) == 0 else np.ascontiguousarray(warp, dtype=np.float64)
            if warps.shape != (nrec,):
                raise ValueError(f"warp must be one number or one per f0 record ({nrec})")
            return formant_plan(records, *args, warps=warps, **kw)
        return _process_tuned(self, plan, x, sample_rate, rate, scale_mask, strength, retune, tracker, threshold, a4, epochs)


def harmony_ratios(records, sample_rate, degrees, scale_mask=0xFFF, strength=1.0, retune=1.0, a4=440.0):
    """pv_harmony_ratios: float64[nvoices, nrec], one pitch ratio within [1/2, 2] per (voice, f0 record of ONE channel).  Voice v lies degrees[v] ALLOWED
    notes of scale_mask above (below, when negative) the note the lead is corrected onto: on the chromatic mask a degree is a semitone, on a seven-note
    mask degree 2 is a diatonic third.  The row of degree 0 is tune_ratios's bit for bit; unvoiced records give every voice the lead's ratio.  1 to 8
    voices, |degree| <= 24; a full octave on top of a correction in the same direction saturates at the clamp."""
    L = load_library()
    r, nrec = _one_channel_records(records)
    deg = np.ascontiguousarray(degrees, dtype=np.int32)
    if deg.ndim != 1:
        raise ValueError("degrees must be int32[nvoices]")
    p = make_tune_params(0, 0, float(sample_rate), 0, 0, 0, 0, scale_mask, float(strength), float(retune), float(a4), 0)
    out = np.zeros((deg.size, nrec), np.float64)
    ip = C.POINTER(C.c_int32)
    n = L.pv_harmony_ratios(C.byref(p), r.ctypes.data_as(ip) if nrec else None, nrec, deg.ctypes.data_as(ip) if deg.size else None, deg.size,
                            out.ctypes.data_as(C.POINTER(C.c_double)) if out.size else None, nrec)
    if n < 0:
        raise ValueError("harmony_ratios: bad argument (tune_ratios's ranges, 1 to 8 voices, degrees within [-24, 24])")
    return out


class Harmony(_Handle):
    """Harmony voices on the overlap-add path (pv_harmony_*): several differently shifted copies of a monophonic voice summed into one output by one
    kernel.  Every voice is a far-grain table of Tsm.process and gives exactly Tsm.process's output for that table; out[c] is the float32 sum over the
    voices, in order, of gains[v, c] * y_v (the product rounded on its own), skipping a voice where its gain is 0 or no grain of it covers the output.  A
    tile of 1024 outputs stages its input once for all voices: the hull of what the voices read there must fit Tsm's span of (max_period, max_rate).
    Stateless; any partition of the output range gives the same bits.  Limits: a monophonic voice; one row of rates for all voices; in unvoiced
    stretches every voice is the same unshifted copy, so consonants add up V-fold (the gains are the remedy)."""

    _prefix = "pv_harmony"
    _fft_size_is_value_error = False

    def __init__(self, max_period, max_rate=2, max_voices=8, max_channels=1, max_outputs=0, device_id=0):
        self._create(make_harmony_config(max_period, max_rate, max_voices, max_channels, max_outputs, device_id, 0))
        self.max_period, self.max_rate, self.max_voices, self.max_channels = max_period, max_rate, max_voices, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no signal state."""

    @staticmethod
    def _tables(tables, gains, nch):
        """(concatenated grains int32[ngrains, 4], voice_first int64[V + 1], gains float32[V, nch]) of a list of far-grain arrays and gains [V] or [V, nch]."""
        parts = [Psola._grains(t)[0].reshape(-1, 4) for t in tables]
        nv = len(parts)
        first = np.zeros(nv + 1, np.int64)
        if nv:
            first[1:] = np.cumsum([q.shape[0] for q in parts])
        g = np.ascontiguousarray(np.concatenate(parts, axis=0) if nv else np.zeros((0, 4)), dtype=np.int32)
        w = np.asarray(gains, dtype=np.float32)
        if w.ndim == 1:
            w = np.repeat(w[:, None], nch, axis=1)
        if w.shape != (nv, nch):
            raise ValueError("gains must have the shape [V] or [V, nch]")
        return g, first, np.ascontiguousarray(w)

    def process(self, x, tables, gains, out_first=0, nout=None):
        """x: float32[nch, n] (host), tables: a list of far-grain arrays int32[., 4], one per voice, gains: [V] or [V, nch] -> float32[nch, nout], outputs
        out_first .. out_first + nout - 1 (default: n - out_first; pass tsm_plan's output_len for a whole stretched signal)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nch, n = x.shape
        g, first, w = self._tables(tables, gains, nch)
        nout = n - out_first if nout is None else int(nout)
        y = np.zeros((nch, max(nout, 0)), np.float32)
        self._check(self._L.pv_harmony_process(self._h, _fp(x), n, n, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if g.size else None,
                                               first.ctypes.data_as(C.POINTER(C.c_int64)), len(first) - 1, _fp(w), _fp(y), int(out_first), nout, max(nout, 0)))
        return y[0] if one else y

    def process_device(self, d_in, nin, in_stride, nch, tables, gains, d_out, out_first, nout, out_stride):
        """pv_harmony_process_device on raw device pointers (ints), asynchronous on the handle's stream; tables and gains are host tables."""
        g, first, w = self._tables(tables, gains, nch)
        self._check(self._L.pv_harmony_process_device(self._h, C.c_void_p(d_in), nin, in_stride, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if g.size else None,
                                                      first.ctypes.data_as(C.POINTER(C.c_int64)), len(first) - 1, _fp(w), C.c_void_p(d_out), out_first, nout,
                                                      out_stride))

    def process_tuned(self, x, sample_rate, degrees=(0, 2, 4), gains=None, rate=1.0, scale_mask=0xFFF, strength=1.0, retune=1.0, tracker=None, threshold=2458,
                      a4=440.0, epochs=False):
        """Offline harmonizer of a monophonic voice: one F0Tracker.track (channel 0: one plan for all channels), optionally one epoch track,
        harmony_ratios, one tsm_plan per voice, all on the same row of rates, and one kernel call.  degrees: one per voice, see harmony_ratios; gains: [V]
        or [V, nch], default 1 / V each; rate, tracker and epochs as Tsm.process_tuned.  x: float32[nch, n] (host).  Returns (y float32[nch,
        output_len], tables): output_len is voice 0's."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nv = len(degrees)
        own = tracker is None
        if own:
            max_lag = max(self.max_period, 3)
            tracker = F0Tracker(1024, 256, max(2, min(32, max_lag // 2)), max_lag)
        try:
            records = tracker.track(x[0], threshold)[0]
        finally:
            if own:
                tracker.close()
        nrec = records.shape[0]
        ratios = harmony_ratios(records, sample_rate, degrees, scale_mask=scale_mask, strength=strength, retune=retune, a4=a4)
        rates = np.full(nrec, float(rate)) if np.ndim(rate) == 0 else np.ascontiguousarray(rate, dtype=np.float64)
        if rates.shape != (nrec,):
            raise ValueError(f"rate must be one number or one per f0 record ({nrec})")
        min_period = tracker.min_lag
        found = None
        if epochs:
            longest = min(tracker.max_lag, 2048, (tracker.window + tracker.max_lag) // 2)
            marks = EpochTracker(2 * longest, tracker.hop, longest)
            try:
                found = marks.track(x[0], epoch_periods(records))[0]
            finally:
                marks.close()
        plans = [tsm_plan(records, tracker.hop, (tracker.window + tracker.max_lag) // 2, x.shape[1], float(min(max(256, min_period), self.max_period)), min_period,
                          self.max_period, ratios=ratios[v], rates=rates, epochs=found) for v in range(nv)]
        tables = [g for g, _ in plans]
        y = self.process(x, tables, np.full(nv, 1.0 / nv, np.float32) if gains is None else gains, 0, plans[0][1])
        return (y[0] if one else y), tables


class Choir(_Handle):
    """Full-grain harmony voices on the overlap-add path (pv_choir_*): Harmony whose voices carry the full grain word.  A grain int32[4] =
    {t, tf + 256 phi + 65536 m + 131072 z, D, L}: m is Mirror's direction bit and z Formant's step, and a grain may have both, in which case it reads
    s / 256 input samples per output sample DOWNWARDS from D - t - tf / 256 - phi / 256 at its centre.  On plain far-grain tables the output is
    Harmony.process's bit for bit; one voice at gain 1 gives Mirror.process's or Formant.process's values.  The mix, the hull staged once per tile and the
    partition invariance are Harmony's; the span and the (max_period, max_rate) pairs that fit the LDS are Formant's.  choir_plan writes one voice's
    table."""

    _prefix = "pv_choir"
    _fft_size_is_value_error = False

    def __init__(self, max_period, max_rate=2, max_voices=8, max_channels=1, max_outputs=0, device_id=0):
        self._create(make_choir_config(max_period, max_rate, max_voices, max_channels, max_outputs, device_id, 0))
        self.max_period, self.max_rate, self.max_voices, self.max_channels = max_period, max_rate, max_voices, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no signal state."""

    _tables = staticmethod(Harmony._tables)

    def process(self, x, tables, gains, out_first=0, nout=None):
        """x: float32[nch, n] (host), tables: a list of grain arrays int32[., 4], one per voice, gains: [V] or [V, nch] -> float32[nch, nout], outputs
        out_first .. out_first + nout - 1 (default: n - out_first; pass choir_plan's output_len for a whole stretched signal)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nch, n = x.shape
        g, first, w = self._tables(tables, gains, nch)
        nout = n - out_first if nout is None else int(nout)
        y = np.zeros((nch, max(nout, 0)), np.float32)
        self._check(self._L.pv_choir_process(self._h, _fp(x), n, n, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if g.size else None,
                                             first.ctypes.data_as(C.POINTER(C.c_int64)), len(first) - 1, _fp(w), _fp(y), int(out_first), nout, max(nout, 0)))
        return y[0] if one else y

    def process_device(self, d_in, nin, in_stride, nch, tables, gains, d_out, out_first, nout, out_stride):
        """pv_choir_process_device on raw device pointers (ints), asynchronous on the handle's stream; tables and gains are host tables."""
        g, first, w = self._tables(tables, gains, nch)
        self._check(self._L.pv_choir_process_device(self._h, C.c_void_p(d_in), nin, in_stride, nch, g.ctypes.data_as(C.POINTER(C.c_int32)) if g.size else None,
                                                    first.ctypes.data_as(C.POINTER(C.c_int64)), len(first) - 1, _fp(w), C.c_void_p(d_out), out_first, nout,
                                                    out_stride))

    def process_tuned(self, x, sample_rate, degrees=(0, 2, 4), warps=None, gains=None, rate=1.0, mirror=False, scale_mask=0xFFF, strength=1.0, retune=1.0,
                      tracker=None, threshold=2458, a4=440.0, epochs=False):
        """Harmony.process_tuned with choir_plan in place of tsm_plan: one f0 track, optionally one epoch track, harmony_ratios, one choir_plan per voice on
        the same row of rates, and one kernel call.  warps: None (no voice is warped), or one entry per voice, each one number or one per f0 record
        (float64[nrec]) within [1/2, 2]: the factor the formants of that voice move by.  mirror: at rates below 1 the repeated unvoiced grains of every
        voice alternate their time direction.  warps=None, mirror=False plans as Harmony.process_tuned does and gives its bits.  Returns
        (y float32[nch, output_len], tables): output_len is voice 0's."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        nv = len(degrees)
        if warps is not None and len(warps) != nv:
            raise ValueError(f"warps must be None or have one entry per voice ({nv})")
        own = tracker is None
        if own:
            max_lag = max(self.max_period, 3)
            tracker = F0Tracker(1024, 256, max(2, min(32, max_lag // 2)), max_lag)
        try:
            records = tracker.track(x[0], threshold)[0]
        finally:
            if own:
                tracker.close()
        nrec = records.shape[0]
        ratios = harmony_ratios(records, sample_rate, degrees, scale_mask=scale_mask, strength=strength, retune=retune, a4=a4)
        rates = np.full(nrec, float(rate)) if np.ndim(rate) == 0 else np.ascontiguousarray(rate, dtype=np.float64)
        if rates.shape != (nrec,):
            raise ValueError(f"rate must be one number or one per f0 record ({nrec})")
        rows = []
        for v in range(nv):
            row = None
            if warps is not None:
                row = np.full(nrec, float(warps[v])) if np.ndim(warps[v]) == 0 else np.ascontiguousarray(warps[v], dtype=np.float64)
                if row.shape != (nrec,):
                    raise ValueError(f"warps[{v}] must be one number or one per f0 record ({nrec})")
            rows.append(row)
        min_period = tracker.min_lag
        found = None
        if epochs:
            longest = min(tracker.max_lag, 2048, (tracker.window + tracker.max_lag) // 2)
            marks = EpochTracker(2 * longest, tracker.hop, longest)
            try:
                found = marks.track(x[0], epoch_periods(records))[0]
            finally:
                marks.close()
        plans = [choir_plan(records, tracker.hop, (tracker.window + tracker.max_lag) // 2, x.shape[1], float(min(max(256, min_period), self.max_period)), min_period,
                            self.max_period, ratios=ratios[v], rates=rates, warps=rows[v], epochs=found, mirror=mirror) for v in range(nv)]
        tables = [g for g, _ in plans]
        y = self.process(x, tables, np.full(nv, 1.0 / nv, np.float32) if gains is None else gains, 0, plans[0][1])
        return (y[0] if one else y), tables


def _take_array(entries):
    """(pv_take array, the arrays it points into) of entries (in address, nin, in_stride, grains, out address, out_first, nout, out_stride)."""
    arr = (_Take * max(len(entries), 1))()
    keep = []
    for k, (d_in, nin, in_stride, grains, d_out, out_first, nout, out_stride) in enumerate(entries):
        g, ng = Psola._grains(grains)
        keep.append(g)
        arr[k] = _Take(d_in or None, int(nin), int(in_stride), g.ctypes.data_as(C.POINTER(C.c_int32)) if ng else None, ng, d_out or None, int(out_first), int(nout),
                       int(out_stride))
    return arr, keep


def takes_tiles(max_period, max_rate, tables, out_firsts, nouts):
    """pv_takes_tiles: int32[ntiles, 8] = {take, first, g_first, g_end, src0, src_count, cls, 0} per tile of 1024 outputs of a Takes call, in (take, tile)
    order: the host's tile walk, pure host code.  tables: one far-grain array per take; out_firsts, nouts: one number per take.  Raises PvError for
    whatever Takes.process refuses in the config, the tables and the ranges."""
    L = load_library()
    if not len(tables) == len(out_firsts) == len(nouts):
        raise ValueError("tables, out_firsts and nouts must have one entry per take")
    arr, keep = _take_array([(0, 0, 0, g, 0, f, n, 0) for g, f, n in zip(tables, out_firsts, nouts)])
    cfg = make_takes_config(int(max_period), int(max_rate))
    n = L.pv_takes_tiles(C.byref(cfg), arr, len(tables), None, 0)
    if n < 0:
        raise PvError(int(-n), L.pv_takes_last_error(None).decode())
    out = np.zeros((n, 8), np.int32)
    if n:
        L.pv_takes_tiles(C.byref(cfg), arr, len(tables), out.ctypes.data_as(C.POINTER(C.c_int32)), n)
    return out


class Takes(_Handle):
    """Per-take plans on the overlap-add path (pv_takes_*): one call plays K independently planned takes of different lengths.  A take is one monophonic
    recording with its own input, far-grain table, length and output range; take k's output is exactly Tsm.process on take k alone, bit for bit, on a
    Tsm of the same (max_period, max_rate).  Takes may share an input; no two output rows may overlap; the channel count is common to the call.  The
    tiles of all takes go out in at most four launches, grouped by occupancy class (takes_tiles).  Stateless."""

    _prefix = "pv_takes"
    _fft_size_is_value_error = False

    def __init__(self, max_period, max_rate=2, max_channels=1, max_outputs=0, device_id=0):
        self._create(make_takes_config(max_period, max_rate, max_channels, max_outputs, device_id, 0))
        self.max_period, self.max_rate, self.max_channels = max_period, max_rate, max_channels

    def reset(self):
        """Nothing to reset: the handle carries no signal state."""

    def process(self, xs, tables, out_first=None, nouts=None):
        """xs: a list of float32[n_k] or float32[nch, n_k] (host), the same nch for all; tables: one far-grain array int32[., 4] per take; out_first, nouts: one
        number per take (default: 0, and n_k - out_first_k) -> a list of float32 arrays, [nout_k] for a one-dimensional take, else [nch, nout_k]."""
        K = len(xs)
        if len(tables) != K or (out_first is not None and len(out_first) != K) or (nouts is not None and len(nouts) != K):
            raise ValueError("xs, tables, out_first and nouts must have one entry per take")
        xs = [np.ascontiguousarray(x, dtype=np.float32) for x in xs]
        one = [x.ndim == 1 for x in xs]
        rows = [x[None, :] if x.ndim == 1 else x for x in xs]
        if any(x.ndim != 2 for x in rows) or len({x.shape[0] for x in rows}) > 1:
            raise ValueError("every take must be float32[n] or float32[nch, n] with the same nch")
        nch = rows[0].shape[0] if K else 0
        firsts = [0] * K if out_first is None else [int(v) for v in out_first]
        counts = [x.shape[1] - f for x, f in zip(rows, firsts)] if nouts is None else [int(v) for v in nouts]
        ys = [np.zeros((nch, max(n, 0)), np.float32) for n in counts]
        arr, keep = _take_array([(x.ctypes.data, x.shape[1], x.shape[1], g, y.ctypes.data, f, n, max(n, 0)) for x, g, y, f, n in zip(rows, tables, ys, firsts, counts)])
        self._check(self._L.pv_takes_process(self._h, arr, K, nch))
        return [y[0] if o else y for y, o in zip(ys, one)]

    def process_device(self, takes, nch):
        """pv_takes_process_device: takes is a list of (d_in, nin, in_stride, grains, d_out, out_first, nout, out_stride) with raw device pointers (ints) and a
        host far-grain array each; asynchronous on the handle's stream."""
        arr, keep = _take_array(takes)
        self._check(self._L.pv_takes_process_device(self._h, arr, len(takes), int(nch)))

    def process_tuned(self, xs, sample_rate, rate=1.0, scale_mask=0xFFF, strength=1.0, retune=1.0, threshold=2458, a4=440.0, epochs=False):
        """Offline tempo change and pitch correction of K takes in one overlap-add call: what Tsm.process_tuned does for one.  Channel 0 of every take is
        zero-padded to the longest take and all are tracked in ONE F0Tracker.track call of K channels (in chunks, if K is more than the tracker takes);
        take k keeps the first frames(n_k) records of its row, which are the records of tracking take k alone, a record being an exact integer function
        of its own frame.  Then tune_ratios and tsm_plan per take on the host, and one Takes.process.  rate: one number, or one entry per take, each a
        number or a row float64[nrec_k].  epochs=True: the epoch tracker runs once PER TAKE, since it takes one row of periods for all its channels.
        The tracker is Tsm.process_tuned's default one (window 1024, hop 256, lags up to max_period) with K channels, so there is no tracker argument.
        A take shorter than window + max_lag samples has no whole f0 frame: it gets no records and tsm_plan's unvoiced grains, exactly as
        Tsm.process_tuned treats it alone.  xs: a list of float32[n_k] or float32[nch, n_k] (host).  Returns (ys, tables): ys[k] has tsm_plan's
        output_len of take k."""
        K = len(xs)
        xs = [np.ascontiguousarray(x, dtype=np.float32) for x in xs]
        leads = [x if x.ndim == 1 else x[0] for x in xs]
        rate_of = [rate] * K if isinstance(rate, (int, float, np.integer, np.floating)) else list(rate)       # (a list may mix numbers and rows)
        if len(rate_of) != K:
            raise ValueError(f"rate must be one number or one entry per take ({K})")
        if K == 0:
            return [], []
        max_lag = max(self.max_period, 3)
        window, hop, min_lag = 1024, 256, max(2, min(32, max_lag // 2))
        longest = max(v.shape[0] for v in leads)
        chunk = 1024
        records = []
        tracker = F0Tracker(window, hop, min_lag, max_lag, max_channels=min(K, chunk))           # one tracker for all chunks
        try:
            for k0 in range(0, K, chunk):
                part = leads[k0:k0 + chunk]
                padded = np.zeros((len(part), longest), np.float32)
                for j, v in enumerate(part):
                    padded[j, :v.shape[0]] = v
                rows = tracker.track(padded, threshold)
                records += [np.ascontiguousarray(rows[j, :tracker.frames(v.shape[0])]) for j, v in enumerate(part)]
        finally:
            tracker.close()
        marks = None
        if epochs:
            reach = min(max_lag, 2048, (window + max_lag) // 2)
            marks = EpochTracker(2 * reach, hop, reach)                                          # one handle, one track call per take
        tables, lengths = [], []
        try:
            for k in range(K):
                rec, n = records[k], leads[k].shape[0]
                nrec = rec.shape[0]
                ratios = tune_ratios(rec, sample_rate, scale_mask=scale_mask, strength=strength, retune=retune, a4=a4)
                rates = np.full(nrec, float(rate_of[k])) if np.ndim(rate_of[k]) == 0 else np.ascontiguousarray(rate_of[k], dtype=np.float64)
                if rates.shape != (nrec,):
                    raise ValueError(f"take {k}: rate must be one number or one per f0 record ({nrec})")
                found = marks.track(leads[k], epoch_periods(rec))[0] if marks is not None else None
                grains, output_len = tsm_plan(rec, hop, (window + max_lag) // 2, n, float(min(max(256, min_lag), self.max_period)), min_lag, self.max_period,
                                              ratios=ratios, rates=rates, epochs=found)
                tables.append(grains)
                lengths.append(output_len)
        finally:
            if marks is not None:
                marks.close()
        return self.process(xs, tables, [0] * K, lengths), tables
