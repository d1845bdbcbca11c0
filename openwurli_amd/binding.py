"""ctypes binding of include/openwurli_hip.h (the C-ABI of the HIP library)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class OwError(RuntimeError):
    pass


class OwDiag(C.Structure):
    _fields_ = [
        ("active_voices", C.c_uint32), ("held_voices", C.c_uint32), ("sustained_voices", C.c_uint32),
        ("releasing_voices", C.c_uint32), ("steal_voices", C.c_uint32), ("sustain_held", C.c_uint32),
        ("nan_guard_fires", C.c_uint64), ("tremolo_be_fallbacks", C.c_uint64),
        ("preamp_nan_resets", C.c_uint64), ("output_nan_resets", C.c_uint64),
    ]


class OwPowerAmpDiag(C.Structure):
    _fields_ = [("clamp_count", C.c_uint64), ("nr_max_iter_count", C.c_uint64), ("peak_output_volts", C.c_double),
                ("nan_resets", C.c_uint64), ("guard_resets", C.c_uint64), ("rail_pos_volts", C.c_double), ("rail_neg_volts", C.c_double)]


class OwJob(C.Structure):
    _fields_ = [("note", C.c_uint8), ("velocity", C.c_uint8), ("mlp", C.c_uint8), ("poweramp", C.c_uint8),
                ("no_preamp", C.c_uint8), ("no_attack_noise", C.c_uint8), ("has_displacement_scale", C.c_uint8), ("reserved", C.c_uint8),
                ("volume", C.c_double), ("speaker", C.c_double), ("r_ldr", C.c_double),
                ("tremolo_depth", C.c_double), ("displacement_scale", C.c_double)]


MLP_HIDDEN, MLP_OUTPUTS = 16, 11      # include/openwurli_hip.h OW_MLP_HIDDEN / OW_MLP_OUTPUTS


class OwMlpWeights(C.Structure):
    """mlp_weights.rs, same shapes and order."""
    _fields_ = [("w1", C.c_double * 2 * 16), ("b1", C.c_double * 16), ("w2", C.c_double * 16 * 16), ("b2", C.c_double * 16),
                ("w3", C.c_double * 16 * 11), ("b3", C.c_double * 11), ("target_means", C.c_double * 11), ("target_stds", C.c_double * 11)]


class OwMlpCorrections(C.Structure):
    _fields_ = [("freq_offsets_cents", C.c_double * 5), ("decay_offsets", C.c_double * 5), ("ds_correction", C.c_double)]


class OwMlpTrainModel(C.Structure):
    """One model's hyper-parameters (ml/train_mlp.py's flags); target_mask bit i = target i is trained on."""
    _fields_ = [("lr", C.c_double), ("min_lr", C.c_double), ("weight_decay", C.c_double), ("huber_delta", C.c_double), ("sched_factor", C.c_double),
                ("epochs", C.c_uint32), ("patience", C.c_uint32), ("sched_patience", C.c_uint32), ("target_mask", C.c_uint32)]


MLP_TRAIN_MODEL_DTYPE = np.dtype(OwMlpTrainModel)
MLP_TRAIN_MAX_ROW_EPOCHS = 1 << 26      # include/openwurli_hip.h OW_MLP_TRAIN_MAX_ROW_EPOCHS


class OwMlpTrainCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("model_size", C.c_uint32), ("device", C.c_int), ("n_rows", C.c_uint32),
                ("history_epochs", C.c_uint32), ("reserved", C.c_uint32), ("kernel_ms_out", C.POINTER(C.c_double))]

    def __init__(self, n_rows=0, history_epochs=0, device=0, kernel_ms_out=None):
        super().__init__(C.sizeof(OwMlpTrainCfg), C.sizeof(OwMlpTrainModel), device, n_rows, history_epochs, 0, kernel_ms_out)


class OwMlpTrainResult(C.Structure):
    _fields_ = [("best_val_loss", C.c_double), ("last_train_loss", C.c_double), ("last_val_loss", C.c_double), ("last_lr", C.c_double),
                ("best_epoch", C.c_uint32), ("epochs_run", C.c_uint32), ("lr_reductions", C.c_uint32), ("status", C.c_uint32)]


MLP_TRAIN_RESULT_DTYPE = np.dtype(OwMlpTrainResult)


class OwMidiEvent(C.Structure):
    _fields_ = [("engine", C.c_uint32), ("type", C.c_uint8), ("note", C.c_uint8), ("reserved", C.c_uint16), ("value", C.c_float)]


MIDI_DTYPE = np.dtype(OwMidiEvent)


ABI_VERSION = 8      # include/openwurli_hip.h OW_ABI_VERSION; load_library() checks it against ow_abi_version()


class OwBatchCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("job_size", C.c_uint32),
                ("sample_rate", C.c_double), ("duration_s", C.c_double), ("device", C.c_int), ("preamp_kind", C.c_int),
                ("power_amp_kind", C.c_int), ("no_rail_sag", C.c_int)]

    def __init__(self, sample_rate=44100.0, duration_s=2.0, device=0, preamp_kind=0, power_amp_kind=0, no_rail_sag=0):
        super().__init__(C.sizeof(OwBatchCfg), C.sizeof(OwJob), sample_rate, duration_s, device, preamp_kind, power_amp_kind, no_rail_sag)


AUDIT_HARMONICS = 12      # include/openwurli_hip.h OW_AUDIT_HARMONICS


class OwAliasAuditResult(C.Structure):
    _fields_ = [("f0_hz", C.c_double), ("h1_dbfs", C.c_double), ("harmonic_db", C.c_double * AUDIT_HARMONICS), ("harmonic_dbc", C.c_double * AUDIT_HARMONICS),
                ("max_step_up_db", C.c_double), ("max_step_up_from_harmonic", C.c_uint32), ("reserved", C.c_uint32),
                ("hf_band_dbc", C.c_double)]


class OwTimedEvent(C.Structure):
    _fields_ = [("time_s", C.c_double), ("type", C.c_uint8), ("note", C.c_uint8), ("value", C.c_uint8), ("reserved", C.c_uint8 * 5)]


TIMED_EVENT_DTYPE = np.dtype(OwTimedEvent)


class OwMidiRenderCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
                ("volume", C.c_double), ("speaker", C.c_double), ("tail_s", C.c_double), ("no_poweramp", C.c_int), ("device", C.c_int),
                ("preamp_kind", C.c_int), ("power_amp_kind", C.c_int), ("no_rail_sag", C.c_int), ("reserved", C.c_int)]

    def __init__(self, volume=0.6, speaker=1.0, tail_s=2.0, no_poweramp=0, device=0, preamp_kind=0, power_amp_kind=0, no_rail_sag=0, reserved=0):
        super().__init__(C.sizeof(OwMidiRenderCfg), 0, volume, speaker, tail_s, no_poweramp, device, preamp_kind, power_amp_kind, no_rail_sag, reserved)


class OwMidiRenderStats(C.Structure):
    _fields_ = [("n_samples", C.c_uint64), ("note_ons", C.c_uint64), ("peak_polyphony", C.c_uint64)]


class OwCalibPoint(C.Structure):
    _fields_ = [("note", C.c_uint8), ("velocity", C.c_uint8), ("zero_trim", C.c_uint8), ("reserved", C.c_uint8 * 5),
                ("ds_at_c4", C.c_double), ("ds_exponent", C.c_double), ("ds_clamp_lo", C.c_double), ("ds_clamp_hi", C.c_double),
                ("target_db", C.c_double), ("voicing_slope", C.c_double)]


class OwCalibrateCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("point_size", C.c_uint32), ("volume", C.c_double), ("speaker", C.c_double),
                ("device", C.c_int), ("preamp_kind", C.c_int), ("power_amp_kind", C.c_int), ("reserved", C.c_int)]

    def __init__(self, volume=0.40, speaker=1.0, device=0, preamp_kind=0, power_amp_kind=0):
        super().__init__(C.sizeof(OwCalibrateCfg), C.sizeof(OwCalibPoint), volume, speaker, device, preamp_kind, power_amp_kind, 0)


CALIBRATE_ROW_FIELDS = ("ds_at_c4", "ds_actual", "y_peak", "t2_peak_db", "t2_rms_db", "t2_h2_h1_db", "t3_peak_db", "t3_rms_db",
                        "t4_peak_db", "t4_rms_db", "t4_h2_h1_db", "t5_peak_db", "t5_rms_db", "t5_h2_h1_db", "proxy_db", "trim_db",
                        "proxy_error_db", "tanh_compression_db")


class OwCalibrateRow(C.Structure):
    _fields_ = [("midi", C.c_uint8), ("velocity", C.c_uint8), ("reserved", C.c_uint8 * 6)] + [(f, C.c_double) for f in CALIBRATE_ROW_FIELDS]


CALIB_SAMPLES = 22050   # include/openwurli_hip.h OW_CALIB_SAMPLES


class OwPreampPoint(C.Structure):
    _fields_ = [("freq_hz", C.c_double), ("amplitude", C.c_double), ("r_ldr", C.c_double), ("r_reset", C.c_double)]


class OwPreampMeasureCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("point_size", C.c_uint32), ("device", C.c_int), ("preamp_kind", C.c_int),
                ("reserved", C.c_int * 4)]

    def __init__(self, device=0, preamp_kind=0):
        super().__init__(C.sizeof(OwPreampMeasureCfg), C.sizeof(OwPreampPoint), device, preamp_kind)


class OwPreampMeasureRow(C.Structure):
    _fields_ = [("freq_hz", C.c_double), ("amplitude", C.c_double), ("r_ldr", C.c_double), ("gain", C.c_double), ("gain_db", C.c_double),
                ("h", C.c_double * 5), ("thd_pct", C.c_double), ("h2_h3_db", C.c_double)]


PBENCH_SAMPLES = 22050   # include/openwurli_hip.h OW_PBENCH_SAMPLES
PBENCH_GAIN_LO = 13230   # OW_PBENCH_GAIN_LO
PBENCH_HARM_LO = 16537   # OW_PBENCH_HARM_LO


POLY_MAX_NOTES = 31      # include/openwurli_hip.h OW_POLY_MAX_NOTES


class OwPolyChord(C.Structure):
    _fields_ = [("n_notes", C.c_uint8), ("no_poweramp", C.c_uint8), ("reserved", C.c_uint8 * 6), ("notes", C.c_uint8 * 32),
                ("velocities", C.c_uint8 * 32), ("volume", C.c_double), ("speaker", C.c_double), ("r_ldr", C.c_double)]


class OwPolyCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("chord_size", C.c_uint32), ("duration_s", C.c_double), ("device", C.c_int),
                ("preamp_kind", C.c_int), ("power_amp_kind", C.c_int), ("reserved", C.c_int)]

    def __init__(self, duration_s=3.0, device=0, preamp_kind=0, power_amp_kind=0):
        super().__init__(C.sizeof(OwPolyCfg), C.sizeof(OwPolyChord), duration_s, device, preamp_kind, power_amp_kind, 0)


class OwPolyRow(C.Structure):
    _fields_ = [("peak", C.c_double), ("residual_peak", C.c_double), ("win_peak", C.c_double * 3), ("win_mean_sq", C.c_double * 3),
                ("peak_db", C.c_double * 3), ("rms_db", C.c_double * 3), ("intermod_ratio_db", C.c_double)]


CENTROID_MAX_WINDOW = 4096                                  # include/openwurli_hip.h OW_CENTROID_MAX_WINDOW
CENTROID_NO_DATA, CENTROID_OK, CENTROID_MISS = 0, 1, 2      # the status bytes of ow_centroid_row


class OwCentroidJob(C.Structure):
    _fields_ = [("note", C.c_uint8), ("velocity", C.c_uint8), ("no_preamp", C.c_uint8), ("no_poweramp", C.c_uint8),
                ("has_displacement_scale", C.c_uint8), ("reserved", C.c_uint8 * 3), ("displacement_scale", C.c_double),
                ("volume", C.c_double), ("speaker", C.c_double), ("r_ldr", C.c_double)]


class OwCentroidCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("job_size", C.c_uint32), ("duration_s", C.c_double), ("window_ms", C.c_double),
                ("hop_ms", C.c_double), ("end_ms", C.c_double), ("device", C.c_int), ("preamp_kind", C.c_int), ("power_amp_kind", C.c_int),
                ("reserved", C.c_int)]

    def __init__(self, duration_s=1.0, window_ms=5.0, hop_ms=2.5, end_ms=500.0, device=0, preamp_kind=0, power_amp_kind=0):
        super().__init__(C.sizeof(OwCentroidCfg), C.sizeof(OwCentroidJob), duration_s, window_ms, hop_ms, end_ms, device, preamp_kind, power_amp_kind, 0)


class OwCentroidRow(C.Structure):
    _fields_ = [("c10", C.c_double), ("c300", C.c_double), ("drift", C.c_double), ("attack_lo", C.c_double), ("attack_hi", C.c_double),
                ("sustain_lo", C.c_double), ("sustain_hi", C.c_double), ("drift_lo", C.c_double), ("drift_hi", C.c_double),
                ("frame10", C.c_int32), ("frame300", C.c_int32), ("has_c10", C.c_uint8), ("has_c300", C.c_uint8),
                ("attack_status", C.c_uint8), ("sustain_status", C.c_uint8), ("drift_status", C.c_uint8), ("reserved", C.c_uint8 * 3)]


INTERMOD_MAX_PROBES = 75                                    # include/openwurli_hip.h OW_INTERMOD_MAX_PROBES
INTERMOD_DIRTY, INTERMOD_MARGINAL, INTERMOD_OK, INTERMOD_CLEAN = 0, 1, 2, 3      # ow_intermod_row.verdict


class OwNoteJob(C.Structure):
    _fields_ = [("note", C.c_uint8), ("velocity", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class OwIntermodProduct(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("nearest_integer", C.c_uint32), ("mode_ratio", C.c_double), ("fractional_offset", C.c_double),
                ("beat_hz", C.c_double), ("effective_amplitude", C.c_double), ("perceptual_weight", C.c_double), ("risk_score", C.c_double)]


class OwIntermodReport(C.Structure):
    _fields_ = [("midi", C.c_uint8), ("reserved", C.c_uint8 * 7), ("fundamental_hz", C.c_double), ("mu", C.c_double),
                ("products", OwIntermodProduct * 6), ("max_risk", C.c_double), ("total_risk", C.c_double)]


class OwIntermodCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("job_size", C.c_uint32), ("duration_s", C.c_double), ("device", C.c_int), ("reserved", C.c_int)]

    def __init__(self, duration_s=3.0, device=0):
        super().__init__(C.sizeof(OwIntermodCfg), C.sizeof(OwNoteJob), duration_s, device, 0)


class OwIntermodDetail(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("nearest_integer", C.c_uint32), ("intermod_freq", C.c_double), ("nearest_freq", C.c_double),
                ("intermod_mag", C.c_double), ("nearest_mag", C.c_double), ("ratio_db", C.c_double), ("risk_score", C.c_double),
                ("listed", C.c_uint8), ("reserved", C.c_uint8 * 7)]


class OwIntermodRow(C.Structure):
    _fields_ = [("midi", C.c_uint8), ("velocity", C.c_uint8), ("too_short", C.c_uint8), ("verdict", C.c_uint8), ("n_harmonics", C.c_uint32),
                ("n_midpoints", C.c_uint32), ("window_start", C.c_uint32), ("window_end", C.c_uint32), ("reserved", C.c_uint32), ("fundamental_hz", C.c_double),
                ("harmonic_energy", C.c_double), ("midpoint_energy", C.c_double), ("h_db", C.c_double), ("m_db", C.c_double),
                ("ratio_db", C.c_double), ("products", OwIntermodDetail * 6)]


class OwOvershootCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("job_size", C.c_uint32), ("duration_s", C.c_double), ("device", C.c_int), ("reserved", C.c_int)]

    def __init__(self, duration_s=2.0, device=0):
        super().__init__(C.sizeof(OwOvershootCfg), C.sizeof(OwNoteJob), duration_s, device, 0)


OVERSHOOT_ROW_FIELDS = ("peak_0_10", "peak_0_50", "rms_100_200", "rms_1000_1500", "overshoot_db", "bark_decay_db", "pk_dbfs", "rms1_dbfs",
                        "rms2_dbfs")


class OwOvershootRow(C.Structure):
    _fields_ = [("note", C.c_uint8), ("velocity", C.c_uint8), ("reserved", C.c_uint8 * 6)] + [(f, C.c_double) for f in OVERSHOOT_ROW_FIELDS]


class OwBarkCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("job_size", C.c_uint32), ("duration_s", C.c_double), ("measure_start_s", C.c_double),
                ("device", C.c_int), ("preamp_kind", C.c_int)]

    def __init__(self, duration_s=0.5, measure_start_s=0.25, device=0, preamp_kind=0):
        super().__init__(C.sizeof(OwBarkCfg), C.sizeof(OwNoteJob), duration_s, measure_start_s, device, preamp_kind)


BARK_ROW_FIELDS = ("fundamental_hz", "displacement_scale", "reed_peak", "y_peak", "pu_peak", "pu_h1", "pu_h2", "pu_h2_h1", "pre_h1", "pre_h2",
                   "pre_h2_h1")


class OwBarkRow(C.Structure):
    _fields_ = [("note", C.c_uint8), ("velocity", C.c_uint8), ("reserved", C.c_uint8 * 6), ("window_start", C.c_uint32),
                ("window_end", C.c_uint32)] + [(f, C.c_double) for f in BARK_ROW_FIELDS]


PUMP_STATIC, PUMP_STEP, PUMP_RAMP, PUMP_LOGCOS = 0, 1, 2, 3                     # include/openwurli_hip.h OW_PUMP_*


class OwPumpPoint(C.Structure):
    _fields_ = [("sample_rate", C.c_double), ("r_settle", C.c_double), ("settle", C.c_uint64), ("capture", C.c_uint64), ("in_amp", C.c_double),
                ("in_freq", C.c_double), ("extra_sample", C.c_uint32), ("schedule", C.c_uint32), ("r_to", C.c_double), ("ln_mid", C.c_double),
                ("ln_amp", C.c_double), ("sched_freq", C.c_double)]


class OwPumpCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("point_size", C.c_uint32), ("device", C.c_int), ("reserved", C.c_int * 5)]

    def __init__(self, device=0):
        super().__init__(C.sizeof(OwPumpCfg), C.sizeof(OwPumpPoint), device)


class OwPumpRow(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("sum", "sum_sq", "mean", "std", "min", "max", "pair_mean", "pair_std", "raw_std", "extra", "max_step")] + \
               [(f, C.c_uint64) for f in ("nr_exhausted", "be_fallbacks", "voltage_damps", "nan_resets")]


PUMP_FIT_MAX_LUT = 1024                                                           # include/openwurli_hip.h: ow_pump_fit's table limit
PUMP_FIT_CONVERGED, PUMP_FIT_MAXITER, PUMP_FIT_START_INVALID = 0, 1, 2            # its status codes


class OwSegment(C.Structure):
    _fields_ = [("row", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("n_harmonics", C.c_uint32), ("f0", C.c_double)]


SEGMENT_DTYPE = np.dtype(OwSegment)
MAX_HARMONICS = 8
WAV_NONE, WAV_ROUND, WAV_TRUNCATE = -1, 0, 1
GOERTZEL_OFFSETS = 11            # include/openwurli_hip.h OW_GOERTZEL_OFFSETS
NOISE_MAX_BAND_BINS = 4096       # include/openwurli_hip.h OW_NOISE_MAX_BAND_BINS


class OwHarmonicsCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("segment_size", C.c_uint32), ("sample_rate", C.c_double), ("search_pct", C.c_double),
                ("wav24_mode", C.c_int), ("device", C.c_int), ("audio_is_device", C.c_int), ("reserved", C.c_int)]

    def __init__(self, sample_rate=44100.0, search_pct=0.01, wav24_mode=WAV_NONE, device=0, audio_is_device=0):
        super().__init__(C.sizeof(OwHarmonicsCfg), C.sizeof(OwSegment), sample_rate, search_pct, wav24_mode, device, audio_is_device, 0)


class OwIsoNote(C.Structure):
    _fields_ = [("onset_s", C.c_double), ("offset_s", C.c_double), ("amplitude", C.c_double), ("window_start", C.c_double),
                ("window_end", C.c_double), ("id_key", C.c_int64), ("midi_note", C.c_int32), ("score", C.c_int32)]


ISO_NOTE_DTYPE = np.dtype(OwIsoNote)


class OwIsoCfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("note_size", C.c_uint32), ("device", C.c_int), ("reserved", C.c_int),
                ("collision_ratio", C.c_double), ("decay_rate", C.POINTER(C.c_double)), ("midi_freq", C.POINTER(C.c_double)),
                ("kernel_ms_out", C.POINTER(C.c_double))]

    def __init__(self, collision_ratio=0.0, decay_rate=None, midi_freq=None, device=0, kernel_ms_out=None):
        super().__init__(C.sizeof(OwIsoCfg), C.sizeof(OwIsoNote), device, 0, collision_ratio, decay_rate, midi_freq, kernel_ms_out)


# every symbol include/openwurli_hip.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
SYMBOLS = {
    "ow_abi_version": (C.c_int, []),
    "ow_last_error": (C.c_char_p, []),
    "ow_clear_error": (None, []),
    "ow_pool_new": (_VP, [C.c_double, C.c_size_t, C.c_int, C.c_int]),
    "ow_pool_new_with": (_VP, [C.c_double, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "ow_pool_new_kinds": (_VP, [C.c_double, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ow_pool_free": (None, [_VP]),
    "ow_pool_size": (C.c_size_t, [_VP]),
    "ow_pool_engine": (_VP, [_VP, C.c_size_t]),
    "ow_engine_pool": (_VP, [_VP]),
    "ow_pool_set_sample_rate": (C.c_int, [_VP, C.c_double]),
    "ow_pool_reset": (None, [_VP]),
    "ow_pool_ensure_buffer_capacity": (None, [_VP, C.c_size_t]),
    "ow_pool_render": (None, [_VP, _VP, C.c_size_t, C.c_size_t]),
    "ow_pool_midi": (None, [_VP, _VP, C.c_size_t]),
    "ow_pool_device_output": (_VP, [_VP, C.POINTER(C.c_size_t)]),
    "ow_pool_read_voice_sum": (C.c_int, [_VP, _VP, C.c_size_t, C.c_size_t]),
    "ow_pool_read_preamp_out": (C.c_int, [_VP, _VP, C.c_size_t, C.c_size_t]),
    "ow_pool_read_tremolo_r": (C.c_int, [_VP, _VP, C.c_size_t, C.c_size_t]),
    "ow_tremolo_prefetch": (C.c_longlong, [C.c_double, C.c_int, C.c_double]),
    "ow_tremolo_export": (C.c_longlong, [C.c_double, C.c_int, C.c_char_p]),
    "ow_tremolo_import": (C.c_longlong, [C.c_double, C.c_int, C.c_char_p]),
    "ow_tremolo_configure": (C.c_int, [C.c_int, C.c_double, C.c_double]),
    "ow_pool_stream": (_VP, [_VP]),
    "ow_pool_set_profiling": (None, [_VP, C.c_int]),
    "ow_pool_last_kernel_ms": (None, [_VP, C.POINTER(C.c_float)]),
    "ow_engine_new": (_VP, [C.c_double, C.c_int, C.c_int]),
    "ow_engine_new_with": (_VP, [C.c_double, C.c_int, C.c_int, C.c_int]),
    "ow_engine_new_kinds": (_VP, [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ow_engine_set_rail_sag": (None, [_VP, C.c_int]),
    "ow_engine_rail_sag_enabled": (C.c_int, [_VP]),
    "ow_engine_power_amp_diag": (None, [_VP, C.POINTER(OwPowerAmpDiag)]),
    "ow_engine_free": (None, [_VP]),
    "ow_engine_set_sample_rate": (None, [_VP, C.c_double]),
    "ow_engine_reset": (None, [_VP]),
    "ow_engine_warm_up": (None, [_VP]),
    "ow_engine_ensure_buffer_capacity": (None, [_VP, C.c_size_t]),
    "ow_engine_note_on": (None, [_VP, C.c_uint8, C.c_float]),
    "ow_engine_note_off": (None, [_VP, C.c_uint8]),
    "ow_engine_set_sustain": (None, [_VP, C.c_int]),
    "ow_engine_set_volume": (None, [_VP, C.c_double]),
    "ow_engine_set_tremolo_depth": (None, [_VP, C.c_double]),
    "ow_engine_set_speaker_character": (None, [_VP, C.c_double]),
    "ow_engine_set_mlp_enabled": (None, [_VP, C.c_int]),
    "ow_engine_set_noise_enabled": (None, [_VP, C.c_int]),
    "ow_engine_set_noise_gain": (None, [_VP, C.c_double]),
    "ow_engine_set_noise_seed": (None, [_VP, C.c_uint64]),
    "ow_engine_render": (None, [_VP, _VP, C.c_size_t]),
    "ow_engine_get_diag": (None, [_VP, C.POINTER(OwDiag)]),
    "ow_engine_slot_state": (C.c_int, [_VP, C.c_int]),
    "ow_engine_slot_note": (C.c_int, [_VP, C.c_int]),
    "ow_engine_has_steal_voice_for": (C.c_int, [_VP, C.c_uint8]),
    "ow_render_note": (C.c_longlong, [C.c_uint8, C.c_double, C.c_double, C.c_double, C.c_int, _VP, C.c_size_t]),
    "ow_render_note_with_scale": (C.c_longlong, [C.c_uint8, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, _VP, C.c_size_t]),
    "ow_normalize_scale": (C.c_double, [_VP, C.c_size_t]),
    "ow_batch_render": (C.c_longlong, [C.POINTER(OwJob), C.c_size_t, C.POINTER(OwBatchCfg), _VP, C.c_size_t, C.c_int]),
    "ow_mlp_default_weights": (C.c_int, [_VP]),
    "ow_mlp_infer": (C.c_int, [_VP, C.c_size_t, _VP, _VP, C.c_size_t, C.c_int, _VP, _VP]),
    "ow_batch_render_corrected": (C.c_longlong, [C.POINTER(OwJob), C.c_size_t, C.POINTER(OwBatchCfg), _VP, _VP, C.c_size_t, C.c_int]),
    "ow_batch_render_mlp": (C.c_longlong, [C.POINTER(OwJob), C.c_size_t, C.POINTER(OwBatchCfg), _VP, C.c_size_t, _VP, _VP, C.c_size_t, C.c_int]),
    "ow_mlp_train": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, C.POINTER(OwMlpTrainCfg), _VP, _VP, _VP]),
    "ow_device_alloc": (_VP, [C.c_size_t, C.c_int]),
    "ow_device_free": (None, [_VP, C.c_int]),
    "ow_host_alloc": (_VP, [C.c_size_t, C.c_int]),
    "ow_host_free": (None, [_VP, C.c_int]),
    "ow_wav24_quantize": (C.c_int, [_VP, C.c_size_t, C.c_double, C.c_int, _VP]),
    "ow_wav24_write": (C.c_int, [C.c_char_p, _VP, C.c_size_t, C.c_uint32, C.c_double, C.c_int]),
    "ow_extract_harmonics": (C.c_int, [_VP, C.c_size_t, C.c_size_t, C.c_double, _VP, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int,
                                       _VP, _VP, _VP]),
    "ow_goertzel_harmonics": (C.c_int, [_VP, C.c_size_t, C.c_size_t, _VP, C.c_size_t, C.POINTER(OwHarmonicsCfg), _VP, _VP, _VP]),
    "ow_interharmonic_noise": (C.c_int, [_VP, C.c_size_t, C.c_size_t, _VP, C.c_size_t, C.POINTER(OwHarmonicsCfg), _VP]),
    "ow_isolation_collision_table": (C.c_int, [_VP, C.c_double, _VP]),
    "ow_isolation_score": (C.c_int, [_VP, C.c_size_t, _VP, C.c_size_t, C.POINTER(OwIsoCfg), _VP, _VP, _VP, _VP]),
    "ow_clip_bounds": (C.c_int, [_VP, C.c_size_t, C.c_size_t, _VP, C.c_double, C.c_double, C.c_int, _VP, _VP, _VP]),
    "ow_alias_audit_analyze": (C.c_int, [_VP, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, _VP, C.c_int, C.c_int, _VP]),
    "ow_alias_audit_run": (C.c_int, [_VP, _VP, C.c_size_t, C.c_int, C.c_int, _VP, _VP, C.c_size_t]),
    "ow_smf_parse": (C.c_longlong, [_VP, C.c_size_t, C.c_int, _VP, C.c_size_t]),
    "ow_render_midi": (C.c_longlong, [_VP, _VP, C.c_size_t, _VP, _VP, C.c_size_t, _VP]),
    "ow_calibrate": (C.c_int, [_VP, C.c_size_t, C.POINTER(OwCalibrateCfg), _VP, _VP, C.c_size_t]),
    "ow_preamp_measure": (C.c_int, [_VP, C.c_size_t, C.POINTER(OwPreampMeasureCfg), _VP, _VP, C.c_size_t]),
    "ow_render_poly": (C.c_longlong, [_VP, C.c_size_t, C.POINTER(OwPolyCfg), _VP, _VP, _VP, _VP, C.c_size_t]),
    "ow_centroid_frame_count": (C.c_longlong, [C.POINTER(OwCentroidCfg)]),
    "ow_centroid_track": (C.c_longlong, [_VP, C.c_size_t, C.POINTER(OwCentroidCfg), _VP, _VP, C.c_size_t, _VP, C.c_size_t]),
    "ow_centroid_analyze": (C.c_longlong, [_VP, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _VP, C.c_size_t]),
    "ow_intermod_risk": (C.c_int, [C.c_uint8, C.POINTER(OwIntermodReport)]),
    "ow_dft_magnitudes": (C.c_int, [_VP, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, _VP, C.c_size_t, C.c_int, C.c_int, _VP]),
    "ow_intermod_probes": (C.c_int, [C.c_uint8, _VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ow_intermod_audit": (C.c_longlong, [_VP, C.c_size_t, C.POINTER(OwIntermodCfg), _VP, _VP, C.c_size_t]),
    "ow_overshoot": (C.c_longlong, [_VP, C.c_size_t, C.POINTER(OwOvershootCfg), _VP, _VP, C.c_size_t]),
    "ow_bark_audit": (C.c_longlong, [_VP, C.c_size_t, C.POINTER(OwBarkCfg), _VP, _VP, C.c_size_t]),
    "ow_pump_measure": (C.c_int, [_VP, C.c_size_t, C.POINTER(OwPumpCfg), _VP, _VP, C.c_size_t]),
    "ow_pump_fit_eval": (C.c_int, [_VP, _VP, _VP, _VP, C.c_size_t, _VP, _VP, C.c_size_t, _VP, _VP, _VP, C.c_size_t, C.c_uint32, C.c_int, _VP, _VP, C.c_size_t]),
    "ow_pump_fit": (C.c_int, [_VP, _VP, _VP, _VP, C.c_size_t, _VP, _VP, C.c_size_t, _VP, _VP, _VP, C.c_size_t, C.c_uint32, C.c_double, C.c_double,
                              C.c_uint32, C.c_int, _VP, _VP, _VP, _VP, _VP]),
    "ow_pickup_law": (C.c_int, [_VP, C.c_size_t, _VP, _VP, C.c_size_t, C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double,
                                C.c_int, _VP, _VP]),
    "ow_stft_profile": (C.c_int, [_VP, C.c_size_t, C.c_size_t, _VP, _VP, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, _VP, _VP]),
    "ow_frame_rms": (C.c_int, [_VP, C.c_size_t, C.c_size_t, _VP, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, _VP, C.c_size_t, _VP, _VP]),
}


VOICE_RECORD_FIELDS = 103     # OW_TEST_VF_COUNT: doubles of one voice record (ow_test_engine_read_voice_record / _write_voice_record)

# include/openwurli_hip_test.h: test and debug hooks (not part of the drop-in boundary; bound for tests/ only)
TEST_SYMBOLS = {
    "ow_test_engine_new": (_VP, [C.c_double]),
    "ow_test_engine_free": (None, [_VP]),
    "ow_test_engine_take_ops": (C.c_size_t, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t]),
    "ow_test_engine_after_render": (None, [_VP, C.c_size_t, C.c_uint64]),
    "ow_test_engine_masks": (C.c_uint64, [_VP, C.c_int]),
    "ow_debug_mlp_raw": (C.c_int, [_VP, _VP, C.c_size_t, _VP, C.c_int, C.c_int]),
    "ow_debug_div": (C.c_int, [_VP, _VP, C.c_size_t, _VP, _VP, C.c_int]),
    "ow_debug_div_const": (C.c_int, [C.c_int, _VP, C.c_size_t, _VP, _VP, _VP, C.c_int]),
    "ow_debug_div_forms": (C.c_int, [C.c_int, _VP, _VP, _VP, C.c_size_t, _VP, _VP, C.c_int]),
    "ow_debug_unary": (C.c_int, [C.c_int, _VP, C.c_size_t, _VP, _VP, C.c_int]),
    "ow_debug_dk_step": (C.c_int, [C.c_int, C.c_double, _VP, _VP, _VP, _VP, C.c_size_t, _VP, _VP, C.c_int]),
    "ow_debug_trem_step": (C.c_int, [C.c_int, C.c_double, _VP, C.c_size_t, _VP, _VP, _VP, C.c_int]),
    "ow_debug_mel_step": (C.c_int, [C.c_int, C.c_double, _VP, _VP, _VP, C.c_size_t, _VP, _VP, _VP, C.c_int]),
    "ow_test_inject_render_faults": (None, [_VP, C.c_int]),
    "ow_test_fail_acquire_after": (None, [C.c_int]),
    "ow_test_live_resources": (C.c_uint64, []),
    "ow_debug_power_amp": (C.c_int, [C.c_double, _VP, C.c_size_t, C.c_size_t, C.c_int, _VP, _VP, _VP, _VP, _VP, C.c_int]),
    "ow_test_pool_enable_power_amp_tap": (C.c_int, [_VP]),
    "ow_test_pool_power_amp_passes": (C.c_int, [_VP, _VP, C.c_size_t]),
    "ow_test_pool_read_power_amp_out": (C.c_int, [_VP, _VP, C.c_size_t, C.c_size_t]),
    "ow_test_engine_poke_power_amp_node": (C.c_int, [_VP, C.c_int, C.c_double]),
    "ow_test_pool_stagger_tremolo": (C.c_int, [_VP, C.c_size_t]),
    "ow_test_pool_tremolo_groups": (C.c_size_t, [_VP]),
    "ow_test_clear_settle_caches": (C.c_int, []),
    "ow_test_pool_set_switch": (C.c_int, [_VP, C.c_char_p, C.c_int]),
    "ow_test_pool_get_switch": (C.c_int, [_VP, C.c_char_p]),
    "ow_test_block_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t]),
    "ow_test_pool_trajectory_info": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "ow_test_pool_trajectory_state": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "ow_test_host_melange_paths": (C.c_int, [C.c_double]),
    "ow_test_device_read": (C.c_int, [_VP, _VP, C.c_size_t, C.c_int]),
    "ow_test_device_write": (C.c_int, [_VP, _VP, C.c_size_t, C.c_int]),
    "ow_debug_window_stats": (C.c_int, [_VP, C.c_size_t, C.c_size_t, _VP, _VP, _VP, C.c_size_t, C.c_int, _VP]),
    "ow_debug_note_table": (C.c_int, [_VP, C.c_int]),
    "ow_test_engine_poke_voice": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.c_double]),
    "ow_test_engine_poke_preamp_node": (C.c_int, [_VP, C.c_int, C.c_int, C.c_double]),
    "ow_test_engine_read_preamp_state": (C.c_int, [_VP, C.c_int, _VP]),
    "ow_test_engine_read_chain_rows": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "ow_test_engine_write_chain_rows": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "ow_test_engine_read_voice_record": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "ow_test_engine_write_voice_record": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "ow_test_host_matrices": (C.c_int, [C.c_int, C.c_double, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ow_debug_trem_trajectory": (C.c_int, [C.c_double, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, _VP, _VP, _VP, _VP, _VP, C.c_int, _VP, _VP]),
}


def library_path():
    return os.environ.get("OPENWURLI_HIP_LIB", os.path.join(_HERE, "lib", "libopenwurli_hip.so"))


def load_library():
    """Load the HIP library.  Fails loudly when it has not been built -- there is no fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise OwError(f"{path} not found: build it with ./build.sh (hipcc --offload-arch=gfx950); "
                      "openwurli-hip has no CPU fallback")
    lib = C.CDLL(path)

    def bind(name, res, args):
        fn = getattr(lib, name, None)
        if fn is None:
            raise OwError(f"{path} does not export {name}: rebuild with ./build.sh")
        fn.restype, fn.argtypes = res, args
        return fn

    built = bind("ow_abi_version", *SYMBOLS["ow_abi_version"])()      # before anything else: a stale library is named as such
    if built != ABI_VERSION:
        raise OwError(f"{path} was built against OW_ABI_VERSION {built}, this binding against {ABI_VERSION}: rebuild with ./build.sh")
    for name, (res, args) in list(SYMBOLS.items()) + list(TEST_SYMBOLS.items()):
        bind(name, res, args)
    _LIB = lib
    return lib


def last_error(lib=None):
    lib = lib or load_library()
    msg = lib.ow_last_error()
    return msg.decode() if msg else ""


def take_error(lib=None):
    """The recorded error message, cleared (so that a later raise_if_error does not report it again)."""
    lib = lib or load_library()
    msg = last_error(lib)
    lib.ow_clear_error()
    return msg


def check(lib, rc):
    """rc of an entry point that reports failure by a negative return: raises the recorded reason, else returns rc."""
    if rc < 0:
        raise OwError(take_error(lib))
    return rc


def raise_if_error(lib=None):
    """The realtime C entry points return void and degrade to silence; the Python mirror turns the recorded reason into an exception
    (the block it returns alongside is the silence the C contract promises)."""
    lib = lib or load_library()
    msg = last_error(lib)
    if msg:
        lib.ow_clear_error()
        raise OwError(msg)
