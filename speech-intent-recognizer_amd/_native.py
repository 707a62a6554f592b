"""ctypes binding of libsir_hip.so (C ABI: include/sir_hip.h).

There is no fallback: ``lib()`` raises if the library is missing (build it with
``python __graft_entry__.py`` or ``make -C speech-intent-recognizer_amd/csrc``), and every op that
computes raises if its tensors are not on a HIP device.
"""
import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsir_hip.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

SIR_OK = 0
SIR_EINVAL = -1
SIR_EUNSUPPORTED = -4
SIR_ETIMEOUT = -5
SIR_ENOMEM = -2
WAVE_F32, WAVE_I16 = 0, 1
WAVE_ULAW, WAVE_ALAW = 2, 3     # G.711, one byte per sample: accepted only by sir_stream_input_*
BWD_ALL, BWD_HEAD_GRU, BWD_CNN = 0, 1, 2
STREAM_FORCED, STREAM_FLUSHED = 1, 2     # flags column of a sir_stream_push table row
PROFILE_EXTRA_IDS = 1           # SIR_PROFILE_EXTRA_IDS: profile ids behind sir_profile_kernel_count() (include/sir_hip.h)


class FeatureConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int), ("n_fft", C.c_int), ("hop_length", C.c_int), ("n_mels", C.c_int),
                ("f_min", C.c_float), ("f_max", C.c_float), ("window", C.c_void_p), ("mel_fb", C.c_void_p)]


class Augment(C.Structure):
    _fields_ = [("shift", C.c_void_p), ("noise_sigma", C.c_void_p), ("noise_seed", C.c_uint64),
                ("time_mask", C.c_void_p), ("freq_mask", C.c_void_p)]


class ModelWeights(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * 3), ("bn_w", C.c_void_p * 3), ("bn_b", C.c_void_p * 3),
                ("bn_mean", C.c_void_p * 3), ("bn_var", C.c_void_p * 3),
                ("gru_w_ih", C.c_void_p * 4), ("gru_w_hh", C.c_void_p * 4),
                ("gru_b_ih", C.c_void_p * 4), ("gru_b_hh", C.c_void_p * 4),
                ("attn_w", C.c_void_p), ("attn_b", C.c_void_p), ("fc_w", C.c_void_p), ("fc_b", C.c_void_p),
                ("num_classes", C.c_int)]


class ModelGrads(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * 3), ("bn_w", C.c_void_p * 3), ("bn_b", C.c_void_p * 3),
                ("gru_w_ih", C.c_void_p * 4), ("gru_w_hh", C.c_void_p * 4),
                ("gru_b_ih", C.c_void_p * 4), ("gru_b_hh", C.c_void_p * 4),
                ("attn_w", C.c_void_p), ("attn_b", C.c_void_p), ("fc_w", C.c_void_p), ("fc_b", C.c_void_p)]


class TrainConfig(C.Structure):
    _fields_ = [("bn_frozen", C.c_int * 3)]


class AdamConfig(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("decoupled", C.c_int), ("max_norm", C.c_float), ("ema_decay", C.c_float)]


class VadConfig(C.Structure):
    _fields_ = [("chunk_size", C.c_int), ("threshold", C.c_float), ("silence_chunks", C.c_int), ("prior_chunks", C.c_int),
                ("flush_tail", C.c_int)]


class StreamConfig(C.Structure):
    _fields_ = [("vad", VadConfig), ("n_streams", C.c_int), ("wave_dtype", C.c_int), ("max_in", C.c_int), ("max_utt_chunks", C.c_int),
                ("ring_chunks", C.c_int)]


class StreamInputConfig(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("in_dtype", C.c_int), ("in_rate", C.c_int), ("out_rate", C.c_int), ("max_in", C.c_int)]


class AdvConfig(C.Structure):
    _fields_ = [("eps", C.c_float), ("alpha", C.c_float), ("keep_zero_columns", C.c_int)]


# name -> (restype, argtypes); must list every function declared in include/sir_hip.h
SIGNATURES = {
    "sir_abi_version": (C.c_int, []),
    "sir_last_error": (C.c_char_p, []),
    "sir_create": (C.c_int, [C.POINTER(FeatureConfig), C.POINTER(C.c_void_p)]),
    "sir_create_ex": (C.c_int, [C.POINTER(FeatureConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "sir_destroy": (C.c_int, [C.c_void_p]),
    "sir_features_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "sir_features_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Augment),
                                   C.c_void_p]),
    "sir_features_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Augment), C.c_void_p, C.c_int64, C.c_void_p]),
    "sir_mix_to_mono": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_int64, C.c_void_p]),
    "sir_resample_out_len": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "sir_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "sir_perturb_out_len": (C.c_int, [C.c_int, C.c_float]),
    "sir_perturb_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "sir_wave_perturb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_reverb_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "sir_wave_reverb_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_vad_stop_chunks": (C.c_int, [C.c_int, C.c_int, C.c_double]),
    "sir_vad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "sir_vad_segment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.POINTER(VadConfig),
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_vad_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "sir_stream_min_ring_chunks": (C.c_int, [C.POINTER(StreamConfig)]),
    "sir_stream_max_rows": (C.c_int, [C.POINTER(StreamConfig)]),
    "sir_stream_state_bytes": (C.c_size_t, [C.c_void_p, C.POINTER(StreamConfig)]),
    "sir_stream_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(StreamConfig), C.c_void_p, C.c_void_p]),
    "sir_stream_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(StreamConfig), C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "sir_stream_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(StreamConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "sir_stream_input_max_out": (C.c_int, [C.POINTER(StreamInputConfig)]),
    "sir_stream_input_state_bytes": (C.c_size_t, [C.c_void_p, C.POINTER(StreamInputConfig)]),
    "sir_stream_input_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(StreamInputConfig), C.c_void_p, C.c_void_p]),
    "sir_stream_input_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(StreamInputConfig), C.c_void_p, C.c_int64, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sir_gather_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "sir_mix_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "sir_adv_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                               C.POINTER(AdvConfig), C.c_uint64, C.c_void_p, C.c_void_p]),
    "sir_model_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "sir_model_workspace_offsets": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.c_int]),
    "sir_model_infer_table_offsets": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.c_int]),
    "sir_model_set_weights_version": (C.c_int, [C.c_void_p, C.c_uint64]),
    "sir_model_infer": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_model_infer_ragged": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_model_embed": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_proto_state_bytes": (C.c_size_t, [C.c_int]),
    "sir_proto_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "sir_proto_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "sir_proto_finalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sir_proto_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sir_check_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sir_pipeline_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "sir_pipeline_destroy": (C.c_int, [C.c_void_p]),
    "sir_pipeline_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "sir_pipeline_end": (C.c_int, [C.c_void_p, C.c_int]),
    "sir_pipeline_join": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sir_model_train_fwd": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                      C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint64, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_ce_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                              C.c_void_p]),
    "sir_ce_loss_soft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "sir_model_train_bwd": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_float, C.c_uint64, C.POINTER(ModelGrads), C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_model_train_bwd_part": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_float, C.c_uint64, C.POINTER(ModelGrads), C.c_void_p, C.c_size_t, C.c_int,
                                           C.c_void_p]),
    "sir_model_train_workspace_offsets": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.c_int]),
    "sir_model_train_fwd_cfg": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint64, C.POINTER(TrainConfig),
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_model_train_bwd_cfg": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_float, C.c_uint64, C.POINTER(TrainConfig), C.POINTER(ModelGrads), C.c_void_p,
                                          C.c_size_t, C.c_int, C.c_void_p]),
    "sir_model_train_bwd_x": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_float, C.c_uint64, C.POINTER(TrainConfig), C.POINTER(ModelGrads), C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "sir_model_train_fwd_ragged": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.POINTER(TrainConfig),
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_model_train_bwd_ragged": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_float, C.c_uint64, C.POINTER(TrainConfig), C.POINTER(ModelGrads), C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "sir_model_train_bwd_emb": (C.c_int, [C.c_void_p, C.POINTER(ModelWeights), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int, C.c_float, C.c_uint64, C.POINTER(TrainConfig), C.POINTER(ModelGrads), C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "sir_proxy_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sir_proxy_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_adam_step": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_float, C.c_float, C.c_float,
                                C.c_float, C.c_float, C.c_void_p]),
    "sir_grad_norm_partials": (C.c_int, [C.c_int, C.POINTER(C.c_int64)]),
    "sir_grad_norm": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_float, C.c_void_p,
                                C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "sir_adam_step_clipped": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "sir_adam_step_ex": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.POINTER(AdamConfig),
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "sir_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "sir_eval_state_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sir_eval_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "sir_temperature_fit_workspace_bytes": (C.c_size_t, [C.c_int]),
    "sir_temperature_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "sir_ce_loss_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_void_p]),
    "sir_classify_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sir_eval_slots_state_bytes": (C.c_size_t, [C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "sir_eval_accumulate_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sir_decode_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "sir_profile_kernel_count": (C.c_int, []),
    "sir_profile_kernel_name": (C.c_char_p, [C.c_int]),
    "sir_profile_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "sir_profile_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
}

_lib = None
_lock = threading.Lock()


class SirError(RuntimeError):
    pass


def build(verbose=False):
    """Compile every HIP source for gfx950 into lib/libsir_hip.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, "-j4"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-8000:])
    if res.returncode != 0:
        raise SirError("building libsir_hip.so failed")
    return LIB_PATH


def lib():
    """The loaded library; raises SirError if it has not been built (no CPU fallback exists)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise SirError(f"{LIB_PATH} is missing: the HIP extension is required, there is no CPU "
                               "fallback (run `python __graft_entry__.py` to build it)")
            # torch ships its own libamdhip64; import it FIRST so that libsir_hip.so binds to the
            # HIP runtime torch uses (two runtimes in one process do not share devices/streams)
            import torch  # noqa: F401
            handle = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def check(rc, what=""):
    if rc != SIR_OK:
        msg = lib().sir_last_error().decode(errors="replace")
        raise SirError(f"{what} failed with code {rc}: {msg}")


def require_hip(*tensors):
    import torch
    if not torch.cuda.is_available():
        raise SirError("no HIP device visible: this path runs on MI355X only (no CPU fallback)")
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise SirError("tensor is not on a HIP device: this path runs on MI355X only (no CPU fallback)")


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
