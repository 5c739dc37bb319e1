"""ctypes binding over the C ABI of libq3tts.so (include/q3tts.h).

Python here is harness plumbing for tests / bench only; the product is the shared library.  There is no
fallback: if the library is missing or no HIP device is visible, compute entry points raise.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))
LIB_PATH = os.path.join(PKG_ROOT, "libq3tts.so")
_lib = None


class Q3Error(RuntimeError):
    pass


class SamplerConfig(C.Structure):  # engine.rs:13-45
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("has_seed", C.c_int32),
                ("seed", C.c_uint64)]


class GenOptions(C.Structure):  # q3tts_gen_options [EXT]: upstream's generation controls; the defaults reproduce the reference
    _fields_ = [("repetition_penalty", C.c_float), ("predictor_temperature", C.c_float), ("predictor_top_k", C.c_int32),
                ("predictor_top_p", C.c_float)]


GEN_DEFAULTS = {"repetition_penalty": 1.0, "predictor_temperature": 0.0, "predictor_top_k": 0, "predictor_top_p": 1.0}


class EngineParams(C.Structure):
    _fields_ = [("model_dir", C.c_char_p), ("quant", C.c_char_p), ("device", C.c_int32), ("max_batch", C.c_int32),
                ("max_prompt", C.c_int32), ("max_steps", C.c_int32), ("load_codec", C.c_int32), ("use_graph", C.c_int32)]


class Request(C.Structure):
    _fields_ = [("prompt", C.c_void_p), ("n_prompt", C.c_int32), ("sampler", SamplerConfig), ("max_steps", C.c_int32),
                ("mask_eos", C.c_int32), ("codes_out", C.c_void_p), ("pcm_out", C.c_void_p), ("pcm_capacity", C.c_int64),
                ("n_frames", C.c_int32), ("n_pcm", C.c_int64), ("prefill_ms", C.c_double), ("first_chunk_ms", C.c_double),
                ("total_ms", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("frame_loop_ms", C.c_double), ("frames", C.c_int64), ("prefill_ms", C.c_double), ("gemv_ms", C.c_double),
                ("gemv_launches", C.c_int64), ("gemv_bytes", C.c_double), ("codec_ms", C.c_double), ("codec_calls", C.c_int64),
                ("talker_weight_bytes", C.c_double), ("predictor_weight_bytes", C.c_double), ("kv_bytes_per_token", C.c_double),
                ("gu_ms", C.c_double), ("gu_launches", C.c_int64), ("gu_bytes", C.c_double),
                ("sched_steps", C.c_int64), ("slot_frames", C.c_double), ("graph_frames", C.c_int64)]


class ReqStatus(C.Structure):
    _fields_ = [("state", C.c_int32), ("n_frames", C.c_int32), ("n_pcm", C.c_int64), ("queue_ms", C.c_double),
                ("prefill_ms", C.c_double), ("first_chunk_ms", C.c_double), ("total_ms", C.c_double)]


REQ_QUEUED, REQ_RUNNING, REQ_DRAINING, REQ_DONE, REQ_CANCELLED, REQ_FAILED = 0, 1, 2, 3, 4, -1


DECODE_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32)

# every symbol include/q3tts.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "q3tts_last_error", "q3tts_version", "q3tts_device_count", "q3tts_sampler_config_default", "q3tts_engine_params_default",
    "q3tts_engine_create", "q3tts_engine_destroy", "q3tts_generate_batch", "q3tts_engine_stats", "q3tts_engine_reset_stats",
    "q3tts_engine_set_instrument", "q3tts_engine_bytes_per_step", "q3tts_assets_open", "q3tts_assets_close", "q3tts_engine_assets",
    "q3tts_assets_codec_embedding", "q3tts_assets_text_embedding", "q3tts_assets_tts_pad", "q3tts_prompt_build_core",
    "q3tts_prompt_build_clone", "q3tts_sampler_new", "q3tts_sampler_free", "q3tts_sampler_sample", "q3tts_chunker_new",
    "q3tts_chunker_free", "q3tts_chunker_push", "q3tts_decoder_create", "q3tts_decoder_destroy", "q3tts_decoder_samples_per_frame",
    "q3tts_decoder_reset", "q3tts_decoder_decode", "q3tts_mel_frames", "q3tts_mel", "q3tts_tf_open", "q3tts_tf_close",
    "q3tts_tf_dims", "q3tts_tf_clear", "q3tts_tf_eval", "q3tts_op_gemv_q8", "q3tts_op_gateup_q8", "q3tts_op_matmul_float", "q3tts_op_rmsnorm_quant", "q3tts_op_swiglu_quant",
    "q3tts_op_argmax", "q3tts_op_project", "q3tts_op_sample", "q3tts_submit", "q3tts_poll", "q3tts_fetch", "q3tts_wait",
    "q3tts_release", "q3tts_decoder_create_ex", "q3tts_decoder_decode_group", "q3tts_sched_start", "q3tts_sched_stop", "q3tts_sched_step", "q3tts_voice_register", "q3tts_submit_text",
    "q3tts_group_create", "q3tts_group_destroy", "q3tts_group_size", "q3tts_group_engine", "q3tts_group_uses_rccl", "q3tts_group_voice_register",
    "q3tts_group_submit", "q3tts_group_submit_text", "q3tts_group_device_of", "q3tts_group_poll", "q3tts_group_fetch", "q3tts_group_wait",
    "q3tts_group_release", "q3tts_group_start", "q3tts_group_stop", "q3tts_comm_available", "q3tts_comm_unique_id", "q3tts_comm_create",
    "q3tts_comm_destroy", "q3tts_comm_voice_register", "q3tts_engine_device",
    "q3tts_onnx_open", "q3tts_onnx_close", "q3tts_onnx_counts", "q3tts_onnx_summary", "q3tts_onnx_node", "q3tts_onnx_node_input", "q3tts_onnx_node_output",
    "q3tts_onnx_node_attr_ints", "q3tts_onnx_node_attr_float", "q3tts_onnx_initializer", "q3tts_onnx_op_kernel", "q3tts_onnx_decoder_contract",
    "q3tts_onnx_session_open", "q3tts_onnx_session_close", "q3tts_onnx_session_unsupported", "q3tts_onnx_session_set_input", "q3tts_onnx_session_run",
    "q3tts_onnx_session_output_info", "q3tts_onnx_session_output", "q3tts_onnx_session_launches", "q3tts_onnx_op_executable",
    "q3tts_text_nfc", "q3tts_op_gemv_kq", "q3tts_op_gateup_kq", "q3tts_onnx_decoder_open", "q3tts_onnx_decoder_close", "q3tts_onnx_decoder_reset", "q3tts_onnx_decoder_fetch", "q3tts_group_info", "q3tts_onnx_decoder_decode",
    "q3tts_decoder_state_floats", "q3tts_decoder_state_export", "q3tts_decoder_state_import", "q3tts_decoder_state_entry",
    "q3tts_tokenizer_open", "q3tts_tokenizer_close", "q3tts_tokenizer_encode", "q3tts_tokenizer_decode", "q3tts_tokenizer_vocab_size",
    "q3tts_gen_options_default", "q3tts_submit_ex", "q3tts_submit_text_ex", "q3tts_generate_batch_ex", "q3tts_group_submit_ex",
    "q3tts_group_submit_text_ex", "q3tts_op_sample_rows",
    "q3tts_prompt_build_streaming", "q3tts_submit_trailing", "q3tts_submit_text_streaming", "q3tts_generate_batch_trailing",
    "q3tts_group_submit_text_streaming", "q3tts_op_codec_gemm", "q3tts_codec_gemm_plan", "q3tts_codec_gemm_tap_reuse", "q3tts_op_codec_kernel", "q3tts_op_attention", "q3tts_attention_plan",
    "q3tts_op_linear", "q3tts_linear_plan", "q3tts_argmax_key",
    "q3tts_submit_trailing_open", "q3tts_trail_append", "q3tts_trail_progress", "q3tts_submit_text_streaming_open", "q3tts_text_append",
    "q3tts_group_submit_text_streaming_open", "q3tts_group_text_append", "q3tts_group_trail_append", "q3tts_group_trail_progress",
    "q3tts_cancel", "q3tts_group_cancel",
    "q3tts_submit_resume", "q3tts_group_submit_resume", "q3tts_op_feedback_rows", "q3tts_engine_prefill_width",
    "q3tts_engine_set_logprobs", "q3tts_fetch_logprobs", "q3tts_group_set_logprobs", "q3tts_group_fetch_logprobs", "q3tts_op_logprob_rows",
    "q3tts_submit_score", "q3tts_group_submit_score", "q3tts_engine_score_width", "q3tts_op_score_rows", "q3tts_op_score_inputs",
    "q3tts_pred_table_bytes", "q3tts_op_attention_keyed", "q3tts_op_select_rows", "q3tts_op_frame_glue", "q3tts_op_ggml",
    "q3tts_submit_candidates", "q3tts_group_submit_candidates", "q3tts_engine_candidate_stats", "q3tts_op_kv_fork",
    "q3tts_submit_decode", "q3tts_group_submit_decode", "q3tts_engine_decode_width", "q3tts_engine_decode_stats",
    "q3tts_engine_set_output_format", "q3tts_request_format", "q3tts_fetch_pcm16", "q3tts_engine_pcm_out_stats",
    "q3tts_group_set_output_format", "q3tts_group_fetch_pcm16", "q3tts_group_request_format",
    "q3tts_pcm_out_plan", "q3tts_pcm_out_filter", "q3tts_pcm_out_samples", "q3tts_pcm_format_check", "q3tts_op_pcm_convert",
    "q3tts_decoder_snapshot_create", "q3tts_decoder_snapshot_restore", "q3tts_decoder_snapshot_free", "q3tts_decoder_snapshot_bytes",
    "q3tts_preamble_create", "q3tts_preamble_poll", "q3tts_preamble_wait", "q3tts_preamble_release", "q3tts_voice_set_preamble",
    "q3tts_engine_set_preamble", "q3tts_request_preamble", "q3tts_engine_preamble_stats",
    "q3tts_group_preamble_create", "q3tts_group_preamble_wait", "q3tts_group_preamble_release", "q3tts_group_voice_set_preamble",
    "q3tts_group_set_preamble", "q3tts_group_request_preamble",
    "q3tts_stem_create", "q3tts_voice_stem_create", "q3tts_stem_poll", "q3tts_stem_wait", "q3tts_stem_release", "q3tts_voice_set_stem",
    "q3tts_engine_set_stem", "q3tts_request_stem", "q3tts_engine_stem_stats", "q3tts_op_kv_stem",
    "q3tts_group_stem_create", "q3tts_group_voice_stem_create", "q3tts_group_stem_wait", "q3tts_group_stem_release",
    "q3tts_group_voice_set_stem", "q3tts_group_set_stem", "q3tts_group_request_stem", "q3tts_group_stem_stats",
    "q3tts_engine_set_speech_rate", "q3tts_request_speech_rate", "q3tts_engine_tsm_stats", "q3tts_group_set_speech_rate",
    "q3tts_group_request_speech_rate", "q3tts_tsm_samples", "q3tts_tsm_windows", "q3tts_op_tsm", "q3tts_mel_tables",
    "q3tts_engine_set_pitch", "q3tts_request_pitch", "q3tts_engine_pitch_stats", "q3tts_group_set_pitch", "q3tts_group_request_pitch",
    "q3tts_pitch_samples", "q3tts_pitch_plan", "q3tts_pitch_filter", "q3tts_op_pitch",
    "q3tts_engine_set_volume", "q3tts_request_volume", "q3tts_engine_volume_stats", "q3tts_group_set_volume", "q3tts_group_request_volume",
    "q3tts_volume_gain", "q3tts_op_volume",
    "q3tts_engine_set_loudness", "q3tts_fetch_loudness", "q3tts_request_loudness", "q3tts_request_metered", "q3tts_engine_loudness_stats",
    "q3tts_group_set_loudness", "q3tts_group_fetch_loudness", "q3tts_group_request_loudness", "q3tts_group_request_metered",
    "q3tts_loudness_tables", "q3tts_loudness_gate", "q3tts_loudness_gain_db10", "q3tts_op_loudness",
    "q3tts_intake_plan", "q3tts_intake_filter", "q3tts_intake_samples", "q3tts_intake_tile", "q3tts_intake_check", "q3tts_wav_probe",
    "q3tts_intake", "q3tts_wav_intake",
]


class IntakeClip(C.Structure):  # q3tts_intake_clip
    _fields_ = [("data", C.c_void_p), ("n_frames", C.c_int64), ("sample_rate", C.c_int32), ("channels", C.c_int32),
                ("sample_format", C.c_int32), ("downmix", C.c_int32)]


class WavInfo(C.Structure):  # q3tts_wav_info
    _fields_ = [("sample_format", C.c_int32), ("channels", C.c_int32), ("sample_rate", C.c_int32), ("bits", C.c_int32),
                ("data_offset", C.c_int64), ("n_frames", C.c_int64)]


class PcmFormat(C.Structure):  # q3tts_pcm_format
    _fields_ = [("sample_rate", C.c_int32), ("encoding", C.c_int32)]


class Loudness(C.Structure):  # q3tts_loudness
    _fields_ = [("integrated_lufs", C.c_double), ("momentary_max_lufs", C.c_double), ("peak_dbfs", C.c_double), ("n_blocks", C.c_int32),
                ("n_gated", C.c_int32)]


class StemStats(C.Structure):  # q3tts_stem_stats
    _fields_ = [("built", C.c_int64), ("restores", C.c_int64), ("rows_not_prefilled", C.c_int64), ("pages_copied", C.c_int64),
                ("mismatches", C.c_int64), ("device_bytes", C.c_int64)]


PCM_F32, PCM_S16 = 0, 1                                                  # q3tts_pcm_format.encoding
PCM_RATES = (8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000)      # q3tts_spec.h "output formats"
PCM_NATIVE_RATE, PCM_FRAME, PCM_HIST = 24000, 1920, 96
TSM_HOP, TSM_WIN, TSM_SEARCH, TSM_LOOK, TSM_HIST, TSM_MIN, TSM_MAX = 480, 960, 240, 1200, 1920, 50, 200   # q3tts_spec.h "speaking rate"
PITCH_MIN, PITCH_MAX, PITCH_HIST = 50, 200, 64                           # q3tts_spec.h "pitch"
VOL_MIN, VOL_MAX, VOL_LOOK, VOL_HOLD, VOL_DELAY, VOL_HIST = -400, 200, 128, 512, 127, 638   # q3tts_spec.h "volume"
LOUD_SEG, LOUD_BLOCK, LOUD_STATE = 96, 2400, 6                           # q3tts_spec.h "loudness"
INTAKE_U8, INTAKE_S16, INTAKE_S24, INTAKE_S32, INTAKE_F32 = 0, 1, 2, 3, 4   # q3tts_spec.h "reference audio intake"
INTAKE_FIRST, INTAKE_MEAN = 0, 1
INTAKE_SAMPLE_BYTES = (1, 2, 3, 4, 4)
INTAKE_MAX_CLIPS, INTAKE_MAX_OUT = 64, 2880000
MAX_PREAMBLES = 64                                                       # Q3TTS_MAX_PREAMBLES (q3tts_spec.h "codec preambles")
PREAMBLE_BUILDING, PREAMBLE_READY, PREAMBLE_FAILED = 0, 1, -1            # Q3TTS_PREAMBLE_*
MAX_STEMS = 64                                                           # Q3TTS_MAX_STEMS (q3tts_spec.h "prompt stems")
STEM_BUILDING, STEM_READY, STEM_FAILED = 0, 1, -1                        # Q3TTS_STEM_*
LOGPROB_COLS = 17     # Q3TTS_LOGPROB_COLS: code_0, the 15 predictor codes, EOS in code_0's talker row
LOGPROB_NONE = 1.0    # Q3TTS_LOGPROB_NONE: not computed (a real value is never positive)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Q3Error("libq3tts.so not built (run qwen3-tts-rust_amd/build.sh); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.q3tts_last_error.restype = C.c_char_p
        L.q3tts_engine_create.argtypes = [C.POINTER(EngineParams), C.POINTER(C.c_void_p)]
        L.q3tts_engine_destroy.argtypes = [C.c_void_p]
        L.q3tts_generate_batch.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.c_int32]
        L.q3tts_engine_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.q3tts_submit.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.POINTER(C.c_int64)]
        L.q3tts_poll.argtypes = [C.c_void_p, C.c_int64, C.POINTER(ReqStatus)]
        L.q3tts_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.q3tts_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
        L.q3tts_release.argtypes = [C.c_void_p, C.c_int64]
        L.q3tts_sched_start.argtypes = [C.c_void_p]
        L.q3tts_sched_stop.argtypes = [C.c_void_p]
        L.q3tts_sched_step.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.q3tts_voice_register.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.q3tts_submit_text.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                        C.POINTER(SamplerConfig), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.q3tts_engine_reset_stats.argtypes = [C.c_void_p]
        L.q3tts_engine_set_instrument.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_engine_bytes_per_step.restype = C.c_double
        L.q3tts_engine_bytes_per_step.argtypes = [C.c_void_p, C.c_int32, C.c_double]
        L.q3tts_assets_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.q3tts_assets_close.argtypes = [C.c_void_p]
        L.q3tts_engine_assets.restype = C.c_void_p
        L.q3tts_engine_assets.argtypes = [C.c_void_p]
        L.q3tts_assets_codec_embedding.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.q3tts_assets_text_embedding.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.q3tts_assets_tts_pad.argtypes = [C.c_void_p, C.c_void_p]
        L.q3tts_prompt_build_core.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.q3tts_prompt_build_clone.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                               C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.q3tts_sampler_new.restype = C.c_void_p
        L.q3tts_sampler_new.argtypes = [C.c_float, C.c_int32, C.c_float, C.c_uint64]
        L.q3tts_sampler_free.argtypes = [C.c_void_p]
        L.q3tts_sampler_sample.restype = C.c_int32
        L.q3tts_sampler_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.q3tts_chunker_new.restype = C.c_void_p
        L.q3tts_chunker_new.argtypes = [DECODE_CB, C.c_void_p]
        L.q3tts_chunker_free.argtypes = [C.c_void_p]
        L.q3tts_chunker_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_decoder_create.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_void_p)]
        L.q3tts_decoder_destroy.argtypes = [C.c_void_p]
        L.q3tts_decoder_create_ex.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.q3tts_decoder_decode_group.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.q3tts_decoder_samples_per_frame.argtypes = [C.c_void_p]
        L.q3tts_decoder_reset.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_decoder_decode.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]
        L.q3tts_mel_frames.argtypes = [C.c_int32]
        L.q3tts_mel.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.q3tts_mel_tables.argtypes = [C.c_void_p, C.c_void_p]
        L.q3tts_tf_open.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.q3tts_tf_close.argtypes = [C.c_void_p]
        L.q3tts_tf_dims.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
        L.q3tts_tf_clear.argtypes = [C.c_void_p]
        L.q3tts_tf_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_op_gemv_q8.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.q3tts_op_gateup_q8.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.q3tts_op_matmul_float.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.q3tts_op_rmsnorm_quant.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.q3tts_op_swiglu_quant.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.q3tts_op_argmax.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.q3tts_op_sample.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p]
        L.q3tts_op_project.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.q3tts_gen_options_default.argtypes = [C.POINTER(GenOptions)]
        L.q3tts_submit_ex.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.POINTER(GenOptions), C.POINTER(C.c_int64)]
        L.q3tts_submit_text_ex.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                           C.POINTER(SamplerConfig), C.c_int32, C.c_int32, C.c_int32, C.POINTER(GenOptions),
                                           C.POINTER(C.c_int64)]
        L.q3tts_generate_batch_ex.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.c_int32, C.POINTER(GenOptions)]
        L.q3tts_group_submit_ex.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.POINTER(GenOptions), C.POINTER(C.c_int64)]
        L.q3tts_group_submit_text_ex.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                                 C.POINTER(SamplerConfig), C.c_int32, C.c_int32, C.c_int32, C.POINTER(GenOptions),
                                                 C.POINTER(C.c_int64)]
        L.q3tts_op_sample_rows.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.q3tts_prompt_build_streaming.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                   C.POINTER(C.c_int32)]
        L.q3tts_submit_trailing.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.POINTER(GenOptions), C.c_void_p, C.c_int32,
                                            C.POINTER(C.c_int64)]
        L.q3tts_submit_text_streaming.argtypes = L.q3tts_submit_text_ex.argtypes
        L.q3tts_generate_batch_trailing.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.c_int32, C.POINTER(GenOptions),
                                                    C.POINTER(C.c_void_p), C.c_void_p]
        L.q3tts_group_submit_text_streaming.argtypes = L.q3tts_group_submit_text_ex.argtypes
        L.q3tts_submit_trailing_open.argtypes = L.q3tts_submit_trailing.argtypes
        L.q3tts_trail_append.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_trail_progress.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.q3tts_submit_text_streaming_open.argtypes = L.q3tts_submit_text_ex.argtypes
        L.q3tts_text_append.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_group_submit_text_streaming_open.argtypes = L.q3tts_group_submit_text_ex.argtypes
        L.q3tts_group_text_append.argtypes = L.q3tts_text_append.argtypes
        L.q3tts_group_trail_append.argtypes = L.q3tts_trail_append.argtypes
        L.q3tts_group_trail_progress.argtypes = L.q3tts_trail_progress.argtypes
        L.q3tts_cancel.argtypes = [C.c_void_p, C.c_int64]
        L.q3tts_group_cancel.argtypes = [C.c_void_p, C.c_int64]
        L.q3tts_submit_resume.argtypes = [C.c_void_p, C.POINTER(Request), C.c_int32, C.POINTER(GenOptions), C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
        L.q3tts_group_submit_resume.argtypes = [C.c_void_p, C.c_int32] + L.q3tts_submit_resume.argtypes[1:]
        L.q3tts_op_feedback_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.q3tts_engine_prefill_width.argtypes = [C.c_void_p]
        L.q3tts_engine_set_logprobs.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_fetch_logprobs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
        L.q3tts_group_set_logprobs.argtypes = L.q3tts_engine_set_logprobs.argtypes
        L.q3tts_group_fetch_logprobs.argtypes = L.q3tts_fetch_logprobs.argtypes
        L.q3tts_submit_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
        L.q3tts_group_submit_score.argtypes = [C.c_void_p, C.c_int32] + L.q3tts_submit_score.argtypes[1:]
        L.q3tts_engine_score_width.argtypes = [C.c_void_p]
        L.q3tts_submit_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.q3tts_group_submit_candidates.argtypes = [C.c_void_p, C.c_int32] + L.q3tts_submit_candidates.argtypes[1:]
        L.q3tts_engine_candidate_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.q3tts_op_kv_fork.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_int32, C.c_int32]
        L.q3tts_engine_score_width.restype = C.c_int32
        L.q3tts_submit_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
        L.q3tts_group_submit_decode.argtypes = [C.c_void_p, C.c_int32] + L.q3tts_submit_decode.argtypes[1:]
        L.q3tts_engine_decode_width.argtypes = [C.c_void_p]
        L.q3tts_engine_decode_width.restype = C.c_int32
        L.q3tts_engine_decode_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.q3tts_op_score_rows.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.q3tts_op_score_inputs.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.q3tts_op_logprob_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.q3tts_op_frame_glue.argtypes = [C.c_void_p]
        L.q3tts_engine_set_output_format.argtypes = [C.c_void_p, C.POINTER(PcmFormat)]
        L.q3tts_request_format.argtypes = [C.c_void_p, C.c_int64, C.POINTER(PcmFormat)]
        L.q3tts_fetch_pcm16.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.q3tts_engine_pcm_out_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.q3tts_group_set_output_format.argtypes = L.q3tts_engine_set_output_format.argtypes
        L.q3tts_group_fetch_pcm16.argtypes = L.q3tts_fetch_pcm16.argtypes
        L.q3tts_group_request_format.argtypes = L.q3tts_request_format.argtypes
        L.q3tts_decoder_snapshot_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.q3tts_decoder_snapshot_restore.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_decoder_snapshot_free.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_decoder_snapshot_bytes.argtypes = [C.c_void_p]
        L.q3tts_decoder_snapshot_bytes.restype = C.c_int64
        L.q3tts_preamble_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.q3tts_preamble_poll.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.q3tts_preamble_wait.argtypes = [C.c_void_p, C.c_int32, C.c_double]
        L.q3tts_preamble_release.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_voice_set_preamble.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_engine_set_preamble.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_request_preamble.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.q3tts_engine_preamble_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.q3tts_group_preamble_create.argtypes = L.q3tts_preamble_create.argtypes
        L.q3tts_group_preamble_wait.argtypes = L.q3tts_preamble_wait.argtypes
        L.q3tts_group_preamble_release.argtypes = L.q3tts_preamble_release.argtypes
        L.q3tts_group_voice_set_preamble.argtypes = L.q3tts_voice_set_preamble.argtypes
        L.q3tts_group_set_preamble.argtypes = L.q3tts_engine_set_preamble.argtypes
        L.q3tts_group_request_preamble.argtypes = L.q3tts_request_preamble.argtypes
        L.q3tts_stem_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.q3tts_voice_stem_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.q3tts_stem_poll.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.q3tts_stem_wait.argtypes = [C.c_void_p, C.c_int32, C.c_double]
        L.q3tts_stem_release.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_voice_set_stem.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_engine_set_stem.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_request_stem.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.q3tts_engine_stem_stats.argtypes = [C.c_void_p, C.POINTER(StemStats)]
        L.q3tts_group_stem_create.argtypes = L.q3tts_stem_create.argtypes
        L.q3tts_group_voice_stem_create.argtypes = L.q3tts_voice_stem_create.argtypes
        L.q3tts_group_stem_wait.argtypes = L.q3tts_stem_wait.argtypes
        L.q3tts_group_stem_release.argtypes = L.q3tts_stem_release.argtypes
        L.q3tts_group_voice_set_stem.argtypes = L.q3tts_voice_set_stem.argtypes
        L.q3tts_group_set_stem.argtypes = L.q3tts_engine_set_stem.argtypes
        L.q3tts_group_request_stem.argtypes = L.q3tts_request_stem.argtypes
        L.q3tts_group_stem_stats.argtypes = L.q3tts_engine_stem_stats.argtypes
        L.q3tts_op_kv_stem.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_pcm_out_plan.argtypes = [C.c_int32] + [C.POINTER(C.c_int32)] * 4
        L.q3tts_pcm_out_filter.argtypes = [C.c_int32, C.c_void_p, C.c_int64]
        L.q3tts_pcm_out_filter.restype = C.c_int64
        L.q3tts_pcm_out_samples.argtypes = [C.c_int32, C.c_int64]
        L.q3tts_pcm_out_samples.restype = C.c_int64
        L.q3tts_pcm_format_check.argtypes = [C.POINTER(PcmFormat)]
        L.q3tts_op_pcm_convert.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
        L.q3tts_engine_set_speech_rate.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_request_speech_rate.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.q3tts_engine_tsm_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3
        L.q3tts_group_set_speech_rate.argtypes = L.q3tts_engine_set_speech_rate.argtypes
        L.q3tts_group_request_speech_rate.argtypes = L.q3tts_request_speech_rate.argtypes
        L.q3tts_tsm_samples.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        L.q3tts_tsm_samples.restype = C.c_int64
        L.q3tts_tsm_windows.argtypes = [C.c_void_p, C.c_void_p]
        L.q3tts_op_tsm.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
        L.q3tts_engine_set_pitch.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_request_pitch.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.q3tts_engine_pitch_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 4
        L.q3tts_group_set_pitch.argtypes = L.q3tts_engine_set_pitch.argtypes
        L.q3tts_group_request_pitch.argtypes = L.q3tts_request_pitch.argtypes
        L.q3tts_engine_set_volume.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_request_volume.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.q3tts_engine_volume_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 2
        L.q3tts_group_set_volume.argtypes = L.q3tts_engine_set_volume.argtypes
        L.q3tts_group_request_volume.argtypes = L.q3tts_request_volume.argtypes
        L.q3tts_volume_gain.argtypes = [C.c_int32]
        L.q3tts_volume_gain.restype = C.c_float
        L.q3tts_op_volume.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.q3tts_engine_set_loudness.argtypes = [C.c_void_p, C.c_int32]
        L.q3tts_fetch_loudness.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.q3tts_request_loudness.argtypes = [C.c_void_p, C.c_int64, C.POINTER(Loudness)]
        L.q3tts_request_metered.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.q3tts_engine_loudness_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 2
        L.q3tts_group_set_loudness.argtypes = L.q3tts_engine_set_loudness.argtypes
        L.q3tts_group_fetch_loudness.argtypes = L.q3tts_fetch_loudness.argtypes
        L.q3tts_group_request_loudness.argtypes = L.q3tts_request_loudness.argtypes
        L.q3tts_group_request_metered.argtypes = L.q3tts_request_metered.argtypes
        L.q3tts_loudness_tables.argtypes = [C.c_void_p, C.c_void_p]
        L.q3tts_loudness_gate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Loudness)]
        L.q3tts_loudness_gain_db10.argtypes = [C.c_double, C.c_double]
        L.q3tts_loudness_gain_db10.restype = C.c_int32
        L.q3tts_op_loudness.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
        L.q3tts_intake_plan.argtypes = [C.c_int32] + [C.POINTER(C.c_int32)] * 4
        L.q3tts_intake_filter.argtypes = [C.c_int32, C.c_void_p, C.c_int64]
        L.q3tts_intake_filter.restype = C.c_int64
        L.q3tts_intake_samples.argtypes = [C.c_int32, C.c_int64]
        L.q3tts_intake_samples.restype = C.c_int64
        L.q3tts_intake_tile.argtypes = [C.c_int32]
        L.q3tts_intake_tile.restype = C.c_int32
        L.q3tts_intake_check.argtypes = [C.POINTER(IntakeClip)]
        L.q3tts_wav_probe.argtypes = [C.c_void_p, C.c_int64, C.POINTER(WavInfo)]
        L.q3tts_intake.argtypes = [C.c_int32, C.POINTER(IntakeClip), C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
        L.q3tts_wav_intake.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(WavInfo)]
        L.q3tts_pitch_samples.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
        L.q3tts_pitch_samples.restype = C.c_int64
        L.q3tts_pitch_plan.argtypes = [C.c_int32] + [C.POINTER(C.c_int32)] * 4
        L.q3tts_pitch_filter.argtypes = [C.c_int32, C.c_void_p, C.c_int64]
        L.q3tts_pitch_filter.restype = C.c_int64
        L.q3tts_op_pitch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                     C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _chk(rc):
    if rc != 0:
        raise Q3Error(lib().q3tts_last_error().decode())


def device_count():
    return lib().q3tts_device_count()


class Assets:
    def __init__(self, path=None, handle=None):
        self._own = handle is None
        if handle is None:
            h = C.c_void_p()
            _chk(lib().q3tts_assets_open(path.encode(), C.byref(h)))
            handle = h.value
        self.h = handle

    def close(self):
        if self._own and self.h:
            lib().q3tts_assets_close(self.h)
        self.h = None

    def codec_embedding(self, q, code):
        out = np.zeros(2048, np.float32)
        _chk(lib().q3tts_assets_codec_embedding(self.h, q, code, _p(out)))
        return out

    def text_embedding(self, tok):
        out = np.zeros(2048, np.float32)
        _chk(lib().q3tts_assets_text_embedding(self.h, tok, _p(out)))
        return out

    def tts_pad(self):
        out = np.zeros(2048, np.float32)
        _chk(lib().q3tts_assets_tts_pad(self.h, _p(out)))
        return out

    def build_core(self, text_ids, lang_id=2055, spk_id=None, spk_emb=None, instr_ids=None, mid=None, max_rows=4096):
        t = np.ascontiguousarray(text_ids, np.int32)
        ins = np.ascontiguousarray(instr_ids, np.int32) if instr_ids is not None else None
        se = np.ascontiguousarray(spk_emb, np.float32) if spk_emb is not None else None
        md = np.ascontiguousarray(mid, np.float32) if mid is not None else None
        out = np.zeros((max_rows, 2048), np.float32)
        n = lib().q3tts_prompt_build_core(self.h, _p(t), t.size, -1 if lang_id is None else lang_id,
                                          -1 if spk_id is None else spk_id, _p(se), _p(ins), ins.size if ins is not None else 0,
                                          _p(md), md.shape[0] if md is not None else 0, _p(out), max_rows)
        if n < 0:
            raise Q3Error(lib().q3tts_last_error().decode())
        return out[:n].copy()

    def build_clone(self, text_ids, ref_codes, ref_text_ids, spk_emb, lang_id=2055, instr_ids=None, max_rows=4096):
        t = np.ascontiguousarray(text_ids, np.int32)
        rc = np.ascontiguousarray(ref_codes, np.int32)
        rt = np.ascontiguousarray(ref_text_ids, np.int32)
        se = np.ascontiguousarray(spk_emb, np.float32)
        ins = np.ascontiguousarray(instr_ids, np.int32) if instr_ids is not None else None
        out = np.zeros((max_rows, 2048), np.float32)
        n = lib().q3tts_prompt_build_clone(self.h, _p(t), t.size, _p(rc), rc.size, _p(rt), rt.size, _p(se), lang_id, _p(ins),
                                           ins.size if ins is not None else 0, _p(out), max_rows)
        if n < 0:
            raise Q3Error(lib().q3tts_last_error().decode())
        return out[:n].copy()


    def prompt_build_streaming(self, text_ids, lang_id=2055, spk_id=None, spk_emb=None, instr_ids=None, ref_codes=None, ref_text_ids=None,
                               max_rows=4096):
        """[EXT] streaming-text layout: (prompt rows, trailing ids t_1 .. t_{n-1}, TEXT_EOS); ref_codes given = clone voice"""
        t = np.ascontiguousarray(text_ids, np.int32)
        ins = np.ascontiguousarray(instr_ids, np.int32) if instr_ids is not None else None
        se = np.ascontiguousarray(spk_emb, np.float32) if spk_emb is not None else None
        rc = np.ascontiguousarray(ref_codes, np.int32).reshape(-1) if ref_codes is not None else None
        rt = np.ascontiguousarray(ref_text_ids, np.int32) if ref_text_ids is not None else None
        out = np.zeros((max_rows, 2048), np.float32)
        trail = np.zeros(max(t.size, 1), np.int32)
        nt = C.c_int32()
        n = lib().q3tts_prompt_build_streaming(self.h, _p(t), t.size, -1 if lang_id is None else lang_id, -1 if spk_id is None else spk_id,
                                               _p(se), _p(ins), ins.size if ins is not None else 0, _p(rc), rc.size if rc is not None else 0,
                                               _p(rt), rt.size if rt is not None else 0, _p(out), max_rows, _p(trail), trail.size, C.byref(nt))
        if n < 0:
            raise Q3Error(lib().q3tts_last_error().decode())
        return out[:n].copy(), trail[: nt.value].copy()


def op_feedback_rows(assets, codes, trailing_ids=None):
    """[EXT] resume: the feedback rows [n][2048] of codes [n][16] as k_feedback_codes writes them (row f adds text(trailing_ids[f]) while
    f < len(trailing_ids), tts_pad after)"""
    c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
    t = np.ascontiguousarray(trailing_ids, np.int32) if trailing_ids is not None else None
    rows = np.zeros((c.shape[0], 2048), np.float32)
    _chk(lib().q3tts_op_feedback_rows(assets.h, _p(c), c.shape[0], _p(t) if t is not None and t.size else None,
                                      t.size if t is not None else 0, _p(rows)))
    return rows


def op_logprob_rows(logits, chosen, n=None, extra_idx=-1):
    """[EXT] k_logprob_rows over host rows: logits [B][stride] f32 (the first n columns of a row count, default all), chosen [B] ->
    log softmax(row)[chosen] [B]; with extra_idx >= 0 also log softmax(row)[extra_idx] [B]"""
    lg = np.ascontiguousarray(logits, np.float32)
    lg = lg.reshape(-1, lg.shape[-1])
    c = np.ascontiguousarray(chosen, np.int32).reshape(-1)
    B, stride = lg.shape
    out, extra = np.zeros(B, np.float32), np.zeros(B, np.float32)
    _chk(lib().q3tts_op_logprob_rows(_p(lg), B, stride if n is None else n, stride, _p(c), extra_idx, _p(out), _p(extra) if extra_idx >= 0 else None))
    return (out, extra) if extra_idx >= 0 else out


def op_score_rows(tlogits, plogits, codes):
    """[EXT] k_score_rows over host buffers: tlogits [F][t_stride >= 2160] f32, plogits [15][F][2048], codes [F][16] -> float32 [F][17]"""
    tl = np.ascontiguousarray(tlogits, np.float32)
    pl = np.ascontiguousarray(plogits, np.float32)
    c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
    F = c.shape[0]
    if tl.ndim != 2 or tl.shape[0] != F or pl.shape != (15, F, 2048):
        raise Q3Error("op_score_rows: tlogits [F][stride], plogits [15][F][2048], codes [F][16]")
    out = np.zeros((F, LOGPROB_COLS), np.float32)
    _chk(lib().q3tts_op_score_rows(_p(tl), tl.shape[1], _p(pl), _p(c), F, _p(out)))
    return out


def op_score_inputs(hidden_proj, tabs, codes):
    """[EXT] k_score_inputs over host buffers: hidden_proj [F][dP], tabs = 15 tables [rows_q][dP], codes [F][16] -> float32 [16 F][dP],
    row p * F + f = position p of frame f"""
    hp = np.ascontiguousarray(hidden_proj, np.float32)
    c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
    F, dP = hp.shape
    tb = [np.ascontiguousarray(t, np.float32) for t in tabs]
    if len(tb) != 15 or c.shape[0] != F or any(t.ndim != 2 or t.shape[1] != dP for t in tb):
        raise Q3Error("op_score_inputs: hidden_proj [F][dP], 15 tables [rows][dP], codes [F][16]")
    ptrs = (C.c_void_p * 15)(*[t.ctypes.data for t in tb])
    rows = np.array([t.shape[0] for t in tb], np.int64)
    out = np.zeros((16 * F, dP), np.float32)
    _chk(lib().q3tts_op_score_inputs(_p(hp), ptrs, _p(rows), dP, _p(c), F, _p(out)))
    return out


def op_kv_fork(k_cache, v_cache, page_table, src_seq, dst_seqs, n_positions):
    """[EXT] k_kv_fork over host buffers (q3tts_op_kv_fork): k_cache / v_cache uint16 [n_pages][n_layer][n_kv][8192], page_table int32
    [n_seq][max_pages]; returns the two caches after the copy (the arguments are not changed)"""
    k = np.array(k_cache, np.uint16, order="C")
    v = np.array(v_cache, np.uint16, order="C")
    pt = np.ascontiguousarray(page_table, np.int32)
    ds = np.ascontiguousarray(dst_seqs, np.int32).reshape(-1)
    if k.ndim != 4 or k.shape != v.shape or k.shape[3] != 8192 or pt.ndim != 2:
        raise Q3Error("op_kv_fork: caches [n_pages][n_layer][n_kv][8192] of one shape, page_table [n_seq][max_pages]")
    _chk(lib().q3tts_op_kv_fork(_p(k), _p(v), k.shape[0], k.shape[1], k.shape[2], _p(pt), pt.shape[0], pt.shape[1], src_seq,
                                _p(ds) if ds.size else None, ds.size, n_positions))
    return k, v


def op_kv_stem(k_cache, v_cache, page_table, store_k, store_v, jobs, save):
    """[EXT] k_kv_stem over host buffers (q3tts_op_kv_stem): k_cache / v_cache uint16 [n_pages][n_layer][n_kv][8192], page_table int32
    [n_seq][max_pages], store_k / store_v uint16 [n_store_pages][n_layer][n_kv][8192]; jobs = [(first store page, n_pages, [slots])], all in
    one launch; save False restores store pages into the slots' pages, True saves the one slot's pages into the store.  Returns
    (k_cache, v_cache, store_k, store_v) after the launch (the arguments are not changed)"""
    k = np.array(k_cache, np.uint16, order="C")
    v = np.array(v_cache, np.uint16, order="C")
    sk = np.array(store_k, np.uint16, order="C")
    sv = np.array(store_v, np.uint16, order="C")
    pt = np.ascontiguousarray(page_table, np.int32)
    if k.ndim != 4 or k.shape != v.shape or k.shape[3] != 8192 or pt.ndim != 2 or sk.ndim != 4 or sk.shape != sv.shape or sk.shape[1:] != k.shape[1:]:
        raise Q3Error("op_kv_stem: caches and stores [pages][n_layer][n_kv][8192], page_table [n_seq][max_pages]")
    page0 = np.array([j[0] for j in jobs], np.int32)
    npg = np.array([j[1] for j in jobs], np.int32)
    ndst = np.array([len(j[2]) for j in jobs], np.int32)
    first = np.array([sum(len(j[2]) for j in jobs[:i]) for i in range(len(jobs))], np.int32)
    slots = np.array([b for j in jobs for b in j[2]], np.int32)
    if slots.size == 0:
        slots = np.zeros(1, np.int32)   # a job without slots is refused for its n_dst, not for the empty list
    _chk(lib().q3tts_op_kv_stem(_p(k), _p(v), k.shape[0], k.shape[1], k.shape[2], _p(pt), pt.shape[0], pt.shape[1], _p(sk), _p(sv), sk.shape[0],
                                len(jobs), _p(page0) if len(jobs) else None, _p(npg) if len(jobs) else None, _p(first) if len(jobs) else None,
                                _p(ndst) if len(jobs) else None, _p(slots), slots.size, 1 if save else 0))
    return k, v, sk, sv


def group_submit_candidates(group, engine_index, prompt, seeds, max_steps=8, temperature=0.0, top_k=40, top_p=0.9, mask_eos=True, want_pcm=False,
                            repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0, trailing_ids=None):
    """[EXT] q3tts_group_submit_candidates on a q3tts_group handle (engine_index -1 = round robin): the group request ids, all on one engine"""
    return _submit_candidates(lib().q3tts_group_submit_candidates, (group, engine_index), prompt, seeds, max_steps, temperature, top_k, top_p,
                              mask_eos, want_pcm, GenOptions(repetition_penalty, predictor_temperature, predictor_top_k, predictor_top_p), trailing_ids)


def _submit_candidates(fn, head, prompt, seeds, max_steps, temperature, top_k, top_p, mask_eos, want_pcm, opts, trailing_ids):
    pr = np.ascontiguousarray(prompt, np.float32)
    sd = np.ascontiguousarray(seeds, np.uint64).reshape(-1)
    tr = np.ascontiguousarray(trailing_ids if trailing_ids is not None else [], np.int32)
    r = Request()
    r.prompt = pr.ctypes.data
    r.n_prompt = pr.shape[0]
    r.sampler.temperature, r.sampler.top_k, r.sampler.top_p = temperature, top_k, top_p
    r.max_steps = max_steps
    r.mask_eos = 1 if mask_eos else 0
    o = None if all(getattr(opts, k) == v for k, v in GEN_DEFAULTS.items()) else opts
    ids = np.zeros(max(sd.size, 1), np.int64)
    _chk(fn(*head, C.byref(r), 1 if want_pcm else 0, C.byref(o) if o is not None else None, _p(tr) if tr.size else None, tr.size,
            _p(sd) if sd.size else None, sd.size, _p(ids)))
    return [int(i) for i in ids[: sd.size]]


def group_submit_score(group, engine_index, prompt, codes, trailing_ids=None):
    """[EXT] q3tts_group_submit_score on a q3tts_group handle (engine_index -1 = round robin): the group request id"""
    pr = np.ascontiguousarray(prompt, np.float32)
    c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
    tr = np.ascontiguousarray(trailing_ids if trailing_ids is not None else [], np.int32)
    rid = C.c_int64()
    _chk(lib().q3tts_group_submit_score(group, engine_index, _p(pr), pr.shape[0], _p(tr) if tr.size else None, tr.size,
                                        _p(c) if c.size else None, c.shape[0], C.byref(rid)))
    return rid.value


def group_submit_decode(group, engine_index, codes):
    """[EXT] q3tts_group_submit_decode on a q3tts_group handle (engine_index -1 = round robin): the group request id"""
    c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
    rid = C.c_int64()
    _chk(lib().q3tts_group_submit_decode(group, engine_index, _p(c) if c.size else None, c.shape[0], C.byref(rid)))
    return rid.value


def _fetch_logprobs(fn, h, rid, frame_off, max_frames):
    out = np.zeros((max(max_frames, 1), LOGPROB_COLS), np.float32)
    gf = C.c_int32()
    _chk(fn(h, rid, _p(out), frame_off, max_frames, C.byref(gf)))
    return out[: gf.value].copy()


def group_set_logprobs(group, on):
    """[EXT] q3tts_group_set_logprobs on a q3tts_group handle: every engine of the group records from now on (or stops)"""
    _chk(lib().q3tts_group_set_logprobs(group, 1 if on else 0))


def group_fetch_logprobs(group, rid, frame_off=0, max_frames=4096):
    """[EXT] q3tts_group_fetch_logprobs: float32 [n][17] of a group request id"""
    return _fetch_logprobs(lib().q3tts_group_fetch_logprobs, group, rid, frame_off, max_frames)


def _set_output_format(fn, h, rate, encoding):
    _chk(fn(h, None if rate is None else C.byref(PcmFormat(int(rate), int(encoding)))))


def _request_format(fn, h, rid):
    f = PcmFormat()
    _chk(fn(h, rid, C.byref(f)))
    return f.sample_rate, f.encoding


def _fetch_pcm16(fn, h, rid, off, cap):
    out = np.zeros(max(cap, 1), np.int16)
    got = C.c_int64()
    _chk(fn(h, rid, _p(out), off, cap, C.byref(got)))
    return out[: got.value].copy()


def group_set_output_format(group, rate=None, encoding=PCM_F32):
    """[EXT] q3tts_group_set_output_format on a q3tts_group handle: every engine of the group (rate None = native)"""
    _set_output_format(lib().q3tts_group_set_output_format, group, rate, encoding)


def group_request_format(group, rid):
    """[EXT] q3tts_group_request_format: (sample_rate, encoding) of a group request id"""
    return _request_format(lib().q3tts_group_request_format, group, rid)


def group_fetch_pcm16(group, rid, off=0, cap=0):
    """[EXT] q3tts_group_fetch_pcm16: int16 samples [off, off + cap) available now of a group request id"""
    return _fetch_pcm16(lib().q3tts_group_fetch_pcm16, group, rid, off, cap)


def _request_speech_rate(fn, h, rid):
    v = C.c_int32()
    _chk(fn(h, rid, C.byref(v)))
    return v.value


def group_set_speech_rate(group, rate_pct=100):
    """[EXT] q3tts_group_set_speech_rate on a q3tts_group handle: every engine of the group (100 = off)"""
    _chk(lib().q3tts_group_set_speech_rate(group, int(rate_pct)))


def group_request_speech_rate(group, rid):
    """[EXT] q3tts_group_request_speech_rate: the percent a group request id is spoken at"""
    return _request_speech_rate(lib().q3tts_group_request_speech_rate, group, rid)


def group_set_pitch(group, pitch_pct=100):
    """[EXT] q3tts_group_set_pitch on a q3tts_group handle: every engine of the group (100 = off)"""
    _chk(lib().q3tts_group_set_pitch(group, int(pitch_pct)))


def group_request_pitch(group, rid):
    """[EXT] q3tts_group_request_pitch: the percent a group request id's pitch is shifted to"""
    return _request_speech_rate(lib().q3tts_group_request_pitch, group, rid)


def group_set_volume(group, db10=0):
    """[EXT] q3tts_group_set_volume on a q3tts_group handle: every engine of the group (tenths of a dB, 0 = off)"""
    _chk(lib().q3tts_group_set_volume(group, int(db10)))


def group_request_volume(group, rid):
    """[EXT] q3tts_group_request_volume: the volume of a group request id in tenths of a dB"""
    return _request_speech_rate(lib().q3tts_group_request_volume, group, rid)


def _loudness_dict(o):
    return dict(integrated_lufs=o.integrated_lufs, momentary_max_lufs=o.momentary_max_lufs, peak_dbfs=o.peak_dbfs, n_blocks=o.n_blocks,
                n_gated=o.n_gated)


def _fetch_loudness(fn, h, rid, off=0, cap=None):
    """rows [got][2] float64 = {energy, peak} of the 100 ms blocks [off, off + cap) of a metered request that are available now"""
    cap = 1 << 14 if cap is None else int(cap)
    out, got = np.zeros((max(cap, 1), 2), np.float64), C.c_int64(-1)
    _chk(fn(h, rid, _p(out), int(off), cap, C.byref(got)))
    return out[: got.value].copy()


def _request_loudness(fn, h, rid):
    o = Loudness()
    _chk(fn(h, rid, C.byref(o)))
    return _loudness_dict(o)


def group_set_loudness(group, on=True):
    """[EXT] q3tts_group_set_loudness on a q3tts_group handle: every engine of the group"""
    _chk(lib().q3tts_group_set_loudness(group, 1 if on else 0))


def group_fetch_loudness(group, rid, off=0, cap=None):
    """[EXT] q3tts_group_fetch_loudness: the rows of a group request id"""
    return _fetch_loudness(lib().q3tts_group_fetch_loudness, group, rid, off, cap)


def group_request_loudness(group, rid):
    """[EXT] q3tts_group_request_loudness: the gate over the rows of a group request id so far"""
    return _request_loudness(lib().q3tts_group_request_loudness, group, rid)


def group_request_metered(group, rid):
    """[EXT] q3tts_group_request_metered: whether a group request id is metered"""
    return bool(_request_speech_rate(lib().q3tts_group_request_metered, group, rid))


def _preamble_create(fn, h, codes):
    c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
    pid = C.c_int32()
    _chk(fn(h, _p(c) if c.size else None, c.shape[0], C.byref(pid)))
    return pid.value


def _preamble_wait(fn, h, pid, timeout_ms):
    rc = fn(h, pid, timeout_ms)
    if rc < 0:
        _chk(rc)
    return rc == 0


def _request_preamble(fn, h, rid):
    pid = C.c_int32()
    _chk(fn(h, rid, C.byref(pid)))
    return pid.value


def group_preamble_create(group, codes):
    """[EXT] q3tts_group_preamble_create on a q3tts_group handle: the preamble of codes [n][16] on every engine, under one id"""
    return _preamble_create(lib().q3tts_group_preamble_create, group, codes)


def group_preamble_wait(group, pid, timeout_ms=-1.0):
    """[EXT] q3tts_group_preamble_wait: True once every engine's copy is READY or FAILED"""
    return _preamble_wait(lib().q3tts_group_preamble_wait, group, pid, timeout_ms)


def group_preamble_release(group, pid):
    _chk(lib().q3tts_group_preamble_release(group, pid))


def group_voice_set_preamble(group, voice_id, pid):
    """[EXT] q3tts_group_voice_set_preamble (pid None or -1: none)"""
    _chk(lib().q3tts_group_voice_set_preamble(group, voice_id, -1 if pid is None else pid))


def group_set_preamble(group, pid):
    """[EXT] q3tts_group_set_preamble on every engine (pid None or -1: none)"""
    _chk(lib().q3tts_group_set_preamble(group, -1 if pid is None else pid))


def group_request_preamble(group, rid):
    """[EXT] q3tts_group_request_preamble: the preamble a group request was primed with, -1 when none"""
    return _request_preamble(lib().q3tts_group_request_preamble, group, rid)


def _stem_create(fn, h, rows):
    r = np.ascontiguousarray(rows, np.float32).reshape(-1, 2048) if rows is not None else None
    sid = C.c_int32()
    _chk(fn(h, _p(r) if r is not None and r.size else None, r.shape[0] if r is not None else 0, C.byref(sid)))
    return sid.value


def _voice_stem_create(fn, h, voice_id, lang_id, instr_ids):
    ins = np.ascontiguousarray(instr_ids, np.int32) if instr_ids is not None else None
    sid = C.c_int32()
    _chk(fn(h, voice_id, lang_id, _p(ins), ins.size if ins is not None else 0, C.byref(sid)))
    return sid.value


def _request_stem(fn, h, rid):
    sid, n = C.c_int32(), C.c_int32()
    _chk(fn(h, rid, C.byref(sid), C.byref(n)))
    return sid.value, n.value


def _stem_stats(fn, h):
    s = StemStats()
    _chk(fn(h, C.byref(s)))
    return {k: getattr(s, k) for k, _ in StemStats._fields_}


def group_stem_create(group, rows):
    """[EXT] q3tts_group_stem_create on a q3tts_group handle: the stem of rows [n][2048] on every engine, under one id"""
    return _stem_create(lib().q3tts_group_stem_create, group, rows)


def group_voice_stem_create(group, voice_id, lang_id=2055, instr_ids=None):
    """[EXT] q3tts_group_voice_stem_create: the head the text forms build for this voice, language and instruction, on every engine"""
    return _voice_stem_create(lib().q3tts_group_voice_stem_create, group, voice_id, lang_id, instr_ids)


def group_stem_wait(group, sid, timeout_ms=-1.0):
    """[EXT] q3tts_group_stem_wait: True once every engine's copy is READY or FAILED"""
    return _preamble_wait(lib().q3tts_group_stem_wait, group, sid, timeout_ms)


def group_stem_release(group, sid):
    _chk(lib().q3tts_group_stem_release(group, sid))


def group_voice_set_stem(group, voice_id, sid):
    """[EXT] q3tts_group_voice_set_stem (sid None or -1: none)"""
    _chk(lib().q3tts_group_voice_set_stem(group, voice_id, -1 if sid is None else sid))


def group_set_stem(group, sid):
    """[EXT] q3tts_group_set_stem on every engine (sid None or -1: none)"""
    _chk(lib().q3tts_group_set_stem(group, -1 if sid is None else sid))


def group_request_stem(group, rid):
    """[EXT] q3tts_group_request_stem: (stem id, rows not prefilled) of a group request; (-1, 0) when it took none"""
    return _request_stem(lib().q3tts_group_request_stem, group, rid)


def group_stem_stats(group):
    """[EXT] q3tts_group_stem_stats: the engines' counters added up"""
    return _stem_stats(lib().q3tts_group_stem_stats, group)


class Sampler:  # LlamaSampler (llama/mod.rs:627-776)
    def __init__(self, temperature=0.0, top_k=0, top_p=1.0, seed=42):
        self.h = lib().q3tts_sampler_new(temperature, top_k, top_p, seed)

    def sample(self, logits, start=0, end=None):
        logits = np.ascontiguousarray(logits, np.float32)
        return lib().q3tts_sampler_sample(self.h, _p(logits), logits.size, start, logits.size if end is None else end)

    def close(self):
        if self.h:
            lib().q3tts_sampler_free(self.h)
        self.h = None


class Chunker:  # engine.rs:495-543
    def __init__(self):
        self.calls = []

        def cb(user, codes, n, fin):
            self.calls.append(([codes[i] for i in range(n)], bool(fin)))

        self._cb = DECODE_CB(cb)
        self.h = lib().q3tts_chunker_new(self._cb, None)

    def push(self, codes, is_final=False):
        a = np.ascontiguousarray(codes, np.int64)
        _chk(lib().q3tts_chunker_push(self.h, _p(a) if a.size else None, a.size, 1 if is_final else 0))

    def close(self):
        if self.h:
            lib().q3tts_chunker_free(self.h)
        self.h = None


class Engine:  # TtsEngine (engine.rs:53-169) at the embedding level
    def __init__(self, model_dir, quant="q8_0", max_batch=1, max_prompt=1024, max_steps=512, load_codec=True, use_graph=True, device=0):
        p = EngineParams()
        lib().q3tts_engine_params_default(C.byref(p))
        self._md = model_dir.encode()
        self._q = quant.encode()
        p.model_dir = self._md
        p.quant = self._q
        p.device = device
        p.max_batch = max_batch
        p.max_prompt = max_prompt
        p.max_steps = max_steps
        p.load_codec = 1 if load_codec else 0
        p.use_graph = 1 if use_graph else 0
        h = C.c_void_p()
        _chk(lib().q3tts_engine_create(C.byref(p), C.byref(h)))
        self.h = h.value
        self.max_steps = max_steps
        self._voice_ref = {}   # voice id -> its reference codes [n][16] (prime_voice)
        self.assets = Assets(handle=lib().q3tts_engine_assets(self.h))

    def close(self):
        if self.h:
            lib().q3tts_engine_destroy(self.h)
        self.h = None

    @staticmethod
    def _per(v, i):
        return v[i] if isinstance(v, (list, tuple, np.ndarray)) else v

    @classmethod
    def _opts(cls, i, repetition_penalty, predictor_temperature, predictor_top_k, predictor_top_p):
        """q3tts_gen_options of request i; None when every value is the default (the plain entry points' path)"""
        o = GenOptions(cls._per(repetition_penalty, i), cls._per(predictor_temperature, i), cls._per(predictor_top_k, i),
                       cls._per(predictor_top_p, i))
        return None if all(getattr(o, k) == v for k, v in GEN_DEFAULTS.items()) else o

    def _fill(self, r, pr, i, max_steps, temperature, top_k, top_p, seed, mask_eos):
        r.prompt = pr.ctypes.data
        r.n_prompt = pr.shape[0]
        r.sampler.temperature = self._per(temperature, i)
        r.sampler.top_k = self._per(top_k, i)
        r.sampler.top_p = self._per(top_p, i)
        r.sampler.has_seed = 1
        r.sampler.seed = self._per(seed, i)
        r.max_steps = self._per(max_steps, i)
        r.mask_eos = 1 if self._per(mask_eos, i) else 0

    # ---- continuous-batching scheduler (q3tts_submit / poll / fetch / wait) ----
    def submit(self, prompt, max_steps=8, temperature=0.0, top_k=40, top_p=0.9, seed=42, mask_eos=True, want_pcm=False,
               repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0, trailing_ids=None,
               open_trail=False, prefix_codes=None):
        """trailing_ids: [EXT] streaming-text input, one text id added to the feedback per frame (None = the reference's feedback);
        open_trail: [EXT] live text append -- the trail stays open (trailing_ids may be None / empty), frames past it wait for trail_append;
        prefix_codes: [EXT] resume (q3tts_submit_resume) -- [k][16] frames the request already emitted: it goes on behind them, with every
        other argument (the seed too) as the original submission had it"""
        pr = np.ascontiguousarray(prompt, np.float32)
        r = Request()
        self._fill(r, pr, 0, max_steps, temperature, top_k, top_p, seed, mask_eos)
        o = self._opts(0, repetition_penalty, predictor_temperature, predictor_top_k, predictor_top_p)
        rid = C.c_int64()
        if prefix_codes is not None:
            pc = np.ascontiguousarray(prefix_codes, np.int32).reshape(-1, 16)
            tr = np.ascontiguousarray(trailing_ids if trailing_ids is not None else [], np.int32)
            _chk(lib().q3tts_submit_resume(self.h, C.byref(r), 1 if want_pcm else 0, C.byref(o) if o is not None else None,
                                           _p(tr) if tr.size else None, tr.size, 1 if open_trail else 0, _p(pc) if pc.size else None,
                                           pc.shape[0], C.byref(rid)))
        elif trailing_ids is not None or open_trail:
            tr = np.ascontiguousarray(trailing_ids if trailing_ids is not None else [], np.int32)
            fn = lib().q3tts_submit_trailing_open if open_trail else lib().q3tts_submit_trailing
            _chk(fn(self.h, C.byref(r), 1 if want_pcm else 0, C.byref(o) if o is not None else None, _p(tr), tr.size,
                                             C.byref(rid)))
        elif o is None:
            _chk(lib().q3tts_submit(self.h, C.byref(r), 1 if want_pcm else 0, C.byref(rid)))
        else:
            _chk(lib().q3tts_submit_ex(self.h, C.byref(r), 1 if want_pcm else 0, C.byref(o), C.byref(rid)))
        return rid.value

    def submit_score(self, prompt, codes, trailing_ids=None):
        """[EXT] scoring given frames (q3tts_submit_score): queues the teacher-forced scoring of codes [n][16] behind prompt [rows][2048]
        (and closed trailing ids); when the request is DONE, fetch_logprobs gives float32 [n][17] and fetch the given codes"""
        pr = np.ascontiguousarray(prompt, np.float32)
        c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
        tr = np.ascontiguousarray(trailing_ids if trailing_ids is not None else [], np.int32)
        rid = C.c_int64()
        _chk(lib().q3tts_submit_score(self.h, _p(pr), pr.shape[0], _p(tr) if tr.size else None, tr.size, _p(c) if c.size else None,
                                      c.shape[0], C.byref(rid)))
        return rid.value

    def submit_candidates(self, prompt, seeds, max_steps=8, temperature=0.0, top_k=40, top_p=0.9, mask_eos=True, want_pcm=False,
                          repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0, trailing_ids=None):
        """[EXT] candidate sets (q3tts_submit_candidates): len(seeds) takes of one prompt behind one prefill; candidate i is exactly
        submit(prompt, seed=seeds[i], ...) with the same arguments (a closed trail only).  Returns the request ids, in seed order"""
        return _submit_candidates(lib().q3tts_submit_candidates, (self.h,), prompt, seeds, max_steps, temperature, top_k, top_p, mask_eos, want_pcm,
                                  GenOptions(repetition_penalty, predictor_temperature, predictor_top_k, predictor_top_p), trailing_ids)

    def submit_decode(self, codes):
        """[EXT] decoding given frames (q3tts_submit_decode): queues the decoding of codes [n][16] to PCM on the engine's codec.  The request
        takes no talker slot; poll / fetch / wait / cancel / result(rid, want_pcm=True) serve it like any other"""
        c = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
        rid = C.c_int64()
        _chk(lib().q3tts_submit_decode(self.h, _p(c) if c.size else None, c.shape[0], C.byref(rid)))
        return rid.value

    def decode_width(self):
        """[EXT] decode-only requests that may hold a codec stream at once (q3tts_engine_decode_width)"""
        return lib().q3tts_engine_decode_width(self.h)

    def decode_stats(self):
        """[EXT] q3tts_engine_decode_stats: dict(requests, chunks, chunks_shared)"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_decode_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(requests=a.value, chunks=b.value, chunks_shared=c.value)

    def candidate_stats(self):
        """[EXT] q3tts_engine_candidate_stats: dict(sets, prefill_rows_saved, pages_copied)"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_candidate_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(sets=a.value, prefill_rows_saved=b.value, pages_copied=c.value)

    def score_width(self):
        """[EXT] frames per predictor scoring pass (q3tts_engine_score_width)"""
        return lib().q3tts_engine_score_width(self.h)

    def register_voice(self, spk_emb, ref_codes=None, ref_text_ids=None):
        spk = np.ascontiguousarray(spk_emb, np.float32)
        rc = np.ascontiguousarray(ref_codes, np.int32).reshape(-1) if ref_codes is not None else None
        rt = np.ascontiguousarray(ref_text_ids, np.int32) if ref_text_ids is not None else None
        vid = C.c_int32()
        _chk(lib().q3tts_voice_register(self.h, _p(spk), _p(rc), rc.size if rc is not None else 0, _p(rt), rt.size if rt is not None else 0,
                                        C.byref(vid)))
        if rc is not None and rc.size:
            self._voice_ref[vid.value] = rc.reshape(-1, 16).copy()
        return vid.value

    # ---- [EXT] codec preambles (q3tts_spec.h "codec preambles") ----
    def preamble_create(self, codes):
        """q3tts_preamble_create: queues the build of the codec state behind codes [n][16]; returns the preamble id (BUILDING)"""
        return _preamble_create(lib().q3tts_preamble_create, self.h, codes)

    def preamble_poll(self, pid):
        """(state, n_frames): PREAMBLE_BUILDING / _READY / _FAILED"""
        st, n = C.c_int32(), C.c_int32()
        _chk(lib().q3tts_preamble_poll(self.h, pid, C.byref(st), C.byref(n)))
        return st.value, n.value

    def preamble_wait(self, pid, timeout_ms=-1.0):
        """True once the preamble is READY or FAILED; drives the scheduler itself when no driver thread runs"""
        return _preamble_wait(lib().q3tts_preamble_wait, self.h, pid, timeout_ms)

    def preamble_release(self, pid):
        """the creator's reference goes; voices, the engine-level setting and submitted requests hold their own"""
        _chk(lib().q3tts_preamble_release(self.h, pid))

    def voice_set_preamble(self, voice_id, pid):
        """requests of the text forms with this voice and want_pcm are primed with READY preamble pid (None or -1: none)"""
        _chk(lib().q3tts_voice_set_preamble(self.h, voice_id, -1 if pid is None else pid))

    def set_preamble(self, pid):
        """requests of the raw-prompt forms (submit, candidates, decode) submitted from now on with want_pcm are primed (None or -1: none)"""
        _chk(lib().q3tts_engine_set_preamble(self.h, -1 if pid is None else pid))

    def request_preamble(self, rid):
        """the preamble the request was primed with, -1 when none"""
        return _request_preamble(lib().q3tts_request_preamble, self.h, rid)

    def preamble_stats(self):
        """q3tts_engine_preamble_stats: dict(built, restores, bytes_per_snapshot)"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_preamble_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(built=a.value, restores=b.value, bytes_per_snapshot=c.value)

    # ---- [EXT] prompt stems (q3tts_spec.h "prompt stems") ----
    def stem_create(self, rows):
        """q3tts_stem_create: queues the build of the talker K/V behind rows [n][2048]; returns the stem id (BUILDING)"""
        return _stem_create(lib().q3tts_stem_create, self.h, rows)

    def voice_stem_create(self, voice_id, lang_id=2055, instr_ids=None):
        """q3tts_voice_stem_create: the stem of the rows the text forms build in front of the task text for this voice, language and
        instruction"""
        return _voice_stem_create(lib().q3tts_voice_stem_create, self.h, voice_id, lang_id, instr_ids)

    def stem_poll(self, sid):
        """(state, n_rows): STEM_BUILDING / _READY / _FAILED"""
        st, n = C.c_int32(), C.c_int32()
        _chk(lib().q3tts_stem_poll(self.h, sid, C.byref(st), C.byref(n)))
        return st.value, n.value

    def stem_wait(self, sid, timeout_ms=-1.0):
        """True once the stem is READY or FAILED; drives the scheduler itself when no driver thread runs"""
        return _preamble_wait(lib().q3tts_stem_wait, self.h, sid, timeout_ms)

    def stem_release(self, sid):
        """the creator's reference goes; voices, the engine-level setting and the requests that took the stem hold their own"""
        _chk(lib().q3tts_stem_release(self.h, sid))

    def voice_set_stem(self, voice_id, sid):
        """the READY stem sid applies to requests of the text forms with this voice (None or -1: none)"""
        _chk(lib().q3tts_voice_set_stem(self.h, voice_id, -1 if sid is None else sid))

    def set_stem(self, sid):
        """the READY stem sid applies to requests of the raw-prompt forms (submit, candidates) submitted from now on (None or -1: none)"""
        _chk(lib().q3tts_engine_set_stem(self.h, -1 if sid is None else sid))

    def request_stem(self, rid):
        """(stem id, prompt rows not prefilled) of a request; (-1, 0) when it took none"""
        return _request_stem(lib().q3tts_request_stem, self.h, rid)

    def stem_stats(self):
        """q3tts_engine_stem_stats: dict(built, restores, rows_not_prefilled, pages_copied, mismatches, device_bytes)"""
        return _stem_stats(lib().q3tts_engine_stem_stats, self.h)

    def stem_voice(self, voice_id, lang_id=2055, instr_ids=None, timeout_ms=-1.0):
        """create -> wait -> set for the head of this voice's prompts; the voice then holds the stem (the creator's reference is released).
        Returns the stem id"""
        sid = self.voice_stem_create(voice_id, lang_id, instr_ids)
        try:
            if not self.stem_wait(sid, timeout_ms) or self.stem_poll(sid)[0] != STEM_READY:
                raise Q3Error("the stem of voice %d did not become ready" % voice_id)
            self.voice_set_stem(voice_id, sid)
        finally:
            self.stem_release(sid)
        return sid

    def prime_voice(self, voice_id, timeout_ms=-1.0):
        """create -> wait -> set from the clone voice's own reference codes; the voice then holds the preamble (the creator's reference is
        released).  Returns the preamble id"""
        if voice_id not in self._voice_ref:
            raise Q3Error("voice %d has no reference codes to prime from (a preset voice)" % voice_id)
        pid = self.preamble_create(self._voice_ref[voice_id])
        try:
            if not self.preamble_wait(pid, timeout_ms) or self.preamble_poll(pid)[0] != PREAMBLE_READY:
                raise Q3Error("the preamble of voice %d did not become ready" % voice_id)
            self.voice_set_preamble(voice_id, pid)
        finally:
            self.preamble_release(pid)
        return pid

    def submit_text(self, voice_id, text_ids, lang_id=2055, instr_ids=None, max_steps=8, temperature=0.0, top_k=40, top_p=0.9, seed=42,
                    mask_eos=True, want_pcm=False, repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0,
                    streaming_text=False, open_text=False):
        """streaming_text: [EXT] upstream's streaming-text layout (q3tts_submit_text_streaming); open_text (with streaming_text): the text
        known so far, the rest follows through text_append (q3tts_submit_text_streaming_open)"""
        if open_text and not streaming_text:
            raise Q3Error("open_text needs streaming_text=True")
        t = np.ascontiguousarray(text_ids, np.int32)
        ins = np.ascontiguousarray(instr_ids, np.int32) if instr_ids is not None else None
        sc = SamplerConfig(temperature, top_k, top_p, 1, seed)
        o = self._opts(0, repetition_penalty, predictor_temperature, predictor_top_k, predictor_top_p)
        rid = C.c_int64()
        fn = (lib().q3tts_submit_text_streaming_open if open_text else lib().q3tts_submit_text_streaming) if streaming_text \
            else lib().q3tts_submit_text_ex
        _chk(fn(self.h, voice_id, _p(t), t.size, lang_id, _p(ins), ins.size if ins is not None else 0, C.byref(sc),
                                        max_steps, 1 if mask_eos else 0, 1 if want_pcm else 0, C.byref(o) if o is not None else None,
                                        C.byref(rid)))
        return rid.value

    def trail_append(self, rid, ids, close=False):
        """[EXT] appends raw trailing ids to an open request: 0 appended, 1 the request no longer takes text (raises on errors)"""
        a = np.ascontiguousarray(ids if ids is not None else [], np.int32)
        rc = lib().q3tts_trail_append(self.h, rid, _p(a) if a.size else None, a.size, 1 if close else 0)
        if rc < 0:
            _chk(rc)
        return rc

    def text_append(self, rid, ids, is_last=False):
        """[EXT] appends text ids to an open text-level request; is_last also appends TEXT_EOS and closes.  Returns as trail_append"""
        a = np.ascontiguousarray(ids if ids is not None else [], np.int32)
        rc = lib().q3tts_text_append(self.h, rid, _p(a) if a.size else None, a.size, 1 if is_last else 0)
        if rc < 0:
            _chk(rc)
        return rc

    def trail_progress(self, rid):
        """[EXT] (ids appended, ids consumed by the feedback so far, closed)"""
        na, nc, cl = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(lib().q3tts_trail_progress(self.h, rid, C.byref(na), C.byref(nc), C.byref(cl)))
        return na.value, nc.value, bool(cl.value)

    def poll(self, rid):
        s = ReqStatus()
        _chk(lib().q3tts_poll(self.h, rid, C.byref(s)))
        return {k: getattr(s, k) for k, _ in ReqStatus._fields_}

    def fetch(self, rid, frame_off=0, max_frames=4096, pcm_off=0, pcm_cap=0):
        codes = np.zeros(max(max_frames, 1) * 16, np.int32)
        pcm = np.zeros(max(pcm_cap, 1), np.float32)
        gf, gp = C.c_int32(), C.c_int64()
        _chk(lib().q3tts_fetch(self.h, rid, _p(codes), frame_off, max_frames, _p(pcm) if pcm_cap > 0 else None, pcm_off, pcm_cap,
                               C.byref(gf), C.byref(gp)))
        return codes[: gf.value * 16].reshape(gf.value, 16).copy(), pcm[: gp.value].copy()

    def set_output_format(self, rate=None, encoding=PCM_F32):
        """[EXT] output formats (q3tts_engine_set_output_format): requests submitted from now on with want_pcm deliver `rate` Hz (one of
        PCM_RATES) as PCM_F32 (up to 24000) or PCM_S16; rate None = native.  The converted stream lags the native one by 16 F / L native
        samples (2 ms at 8000 Hz) and its last such samples do not come out"""
        _set_output_format(lib().q3tts_engine_set_output_format, self.h, rate, encoding)

    def request_format(self, rid):
        """[EXT] (sample_rate, encoding) the request delivers"""
        return _request_format(lib().q3tts_request_format, self.h, rid)

    def fetch_pcm16(self, rid, off=0, cap=0):
        """[EXT] int16 samples [off, off + cap) available now of an s16 request (raises on an f32 one)"""
        return _fetch_pcm16(lib().q3tts_fetch_pcm16, self.h, rid, off, cap)

    def pcm_out_stats(self):
        """[EXT] q3tts_engine_pcm_out_stats: dict(chunks_converted, samples_out)"""
        a, b = C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_pcm_out_stats(self.h, C.byref(a), C.byref(b)))
        return dict(chunks_converted=a.value, samples_out=b.value)

    def set_speech_rate(self, rate_pct=100):
        """[EXT] speaking rate (q3tts_engine_set_speech_rate): requests submitted from now on with want_pcm are spoken at rate_pct percent of
        the native tempo, TSM_MIN .. TSM_MAX, pitch preserved; 100 = off.  Such a request delivers 24000 Hz (f32 or s16) and
        tsm_samples(rate_pct, n * 1920, True) samples for n frames"""
        _chk(lib().q3tts_engine_set_speech_rate(self.h, int(rate_pct)))

    def request_speech_rate(self, rid):
        """[EXT] the percent the request is spoken at (100: not stretched)"""
        return _request_speech_rate(lib().q3tts_request_speech_rate, self.h, rid)

    def tsm_stats(self):
        """[EXT] q3tts_engine_tsm_stats: dict(chunks, frames_out, flushes)"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_tsm_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(chunks=a.value, frames_out=b.value, flushes=c.value)

    def set_pitch(self, pitch_pct=100):
        """[EXT] pitch (q3tts_engine_set_pitch): requests submitted from now on with want_pcm have their fundamental multiplied by
        pitch_pct / 100, PITCH_MIN .. PITCH_MAX, with or without a speech rate; 100 = off.  Such a request delivers 24000 Hz (f32 or s16) and
        pitch_samples(rate_pct, pitch_pct, n * 1920, True) samples for n frames; rate / pitch must lie in [1/2, 2] when it is submitted"""
        _chk(lib().q3tts_engine_set_pitch(self.h, int(pitch_pct)))

    def request_pitch(self, rid):
        """[EXT] the percent the request's pitch is shifted to (100: not shifted)"""
        return _request_speech_rate(lib().q3tts_request_pitch, self.h, rid)

    def pitch_stats(self):
        """[EXT] q3tts_engine_pitch_stats: dict(chunks, samples_out, flushes, table_bytes)"""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_pitch_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(chunks=a.value, samples_out=b.value, flushes=c.value, table_bytes=d.value)

    def set_volume(self, db10=0):
        """[EXT] volume (q3tts_engine_set_volume): requests submitted from now on with want_pcm get a gain of db10 tenths of a dB, VOL_MIN ..
        VOL_MAX, behind a look-ahead peak limiter, in front of whatever format, rate or pitch they have; 0 = off.  No count changes; the
        stream is delayed by VOL_DELAY native samples, which are not flushed"""
        _chk(lib().q3tts_engine_set_volume(self.h, int(db10)))

    def request_volume(self, rid):
        """[EXT] the request's volume in tenths of a dB (0: none)"""
        return _request_speech_rate(lib().q3tts_request_volume, self.h, rid)

    def volume_stats(self):
        """[EXT] q3tts_engine_volume_stats: dict(chunks, samples)"""
        a, b = C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_volume_stats(self.h, C.byref(a), C.byref(b)))
        return dict(chunks=a.value, samples=b.value)

    def set_loudness(self, on=True):
        """[EXT] loudness (q3tts_engine_set_loudness): requests submitted from now on with want_pcm are metered: the K-weighted energy and
        the sample peak of every 100 ms block of their native stream, whatever format, rate, pitch or volume they are delivered with"""
        _chk(lib().q3tts_engine_set_loudness(self.h, 1 if on else 0))

    def request_metered(self, rid):
        """[EXT] whether the request was submitted metered"""
        return bool(_request_speech_rate(lib().q3tts_request_metered, self.h, rid))

    def fetch_loudness(self, rid, off=0, cap=None):
        """[EXT] q3tts_fetch_loudness: rows [got][2] float64 = {energy, peak} of the blocks [off, off + cap) available now; they grow with
        poll()'s n_pcm, and n frames give (4 * n) // 5 at the end.  Raises Q3Error for a request that is not metered"""
        return _fetch_loudness(lib().q3tts_fetch_loudness, self.h, rid, off, cap)

    def request_loudness(self, rid):
        """[EXT] q3tts_request_loudness: loudness_gate over the request's rows so far"""
        return _request_loudness(lib().q3tts_request_loudness, self.h, rid)

    def loudness_stats(self):
        """[EXT] q3tts_engine_loudness_stats: dict(chunks, blocks)"""
        a, b = C.c_int64(), C.c_int64()
        _chk(lib().q3tts_engine_loudness_stats(self.h, C.byref(a), C.byref(b)))
        return dict(chunks=a.value, blocks=b.value)

    def wait(self, rid, timeout_ms=-1.0):
        rc = lib().q3tts_wait(self.h, rid, timeout_ms)
        if rc < 0:
            _chk(rc)
        return rc == 0

    def release(self, rid):
        _chk(lib().q3tts_release(self.h, rid))

    def cancel(self, rid):
        """[EXT] stops a request wherever it is (any thread): True when the cancellation was requested -- the request reaches REQ_CANCELLED
        within the scheduler's next steps and keeps what it produced until release --, False when it had already ended (raises on errors)"""
        rc = lib().q3tts_cancel(self.h, rid)
        if rc < 0:
            _chk(rc)
        return rc == 0

    def set_logprobs(self, on):
        """[EXT] token log-probabilities (q3tts_engine_set_logprobs): requests submitted from now on record 17 floats per frame"""
        _chk(lib().q3tts_engine_set_logprobs(self.h, 1 if on else 0))

    def fetch_logprobs(self, rid, frame_off=0, max_frames=4096):
        """[EXT] float32 [n][17] available now -- log softmax of the raw logits at code_0, the 15 predictor codes and (column 16) EOS;
        LOGPROB_NONE where nothing was computed.  Raises for a request that does not record"""
        return _fetch_logprobs(lib().q3tts_fetch_logprobs, self.h, rid, frame_off, max_frames)

    def records(self, rid):
        """whether the request records log-probabilities"""
        return lib().q3tts_fetch_logprobs(self.h, rid, None, 0, 0, None) == 0

    def prefill_width(self):
        """rows of one talker prefill launch (q3tts_engine_prefill_width)"""
        return lib().q3tts_engine_prefill_width(self.h)

    def sched_start(self):
        _chk(lib().q3tts_sched_start(self.h))

    def sched_stop(self):
        _chk(lib().q3tts_sched_stop(self.h))

    def sched_step(self):
        b = C.c_int32()
        _chk(lib().q3tts_sched_step(self.h, C.byref(b)))
        return bool(b.value)

    def result(self, rid, want_pcm=False):
        """collects a finished request (codes [n][16], pcm) and releases it.  pcm is float32 or, for an s16 request ([EXT] output formats),
        int16, at sample_rate Hz"""
        st = self.poll(rid)
        rate, enc = self.request_format(rid)
        s16 = want_pcm and enc == PCM_S16
        codes, pcm = self.fetch(rid, 0, max(st["n_frames"], 1), 0, st["n_pcm"] if want_pcm and not s16 else 0)
        if s16:
            pcm = self.fetch_pcm16(rid, 0, st["n_pcm"])
        out = {"codes": codes, "pcm": pcm if want_pcm else None, "sample_rate": rate, **st}
        if self.records(rid):
            out["logprobs"] = self.fetch_logprobs(rid, 0, max(st["n_frames"], 1))
        self.release(rid)
        return out

    def generate_batch(self, prompts, max_steps=8, temperature=0.0, top_k=40, top_p=0.9, seed=42, mask_eos=True, want_pcm=False,
                       pcm_per_frame=1920, repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0,
                       trailing_ids=None):
        """per-request values may be given as lists (max_steps, temperature, top_k, top_p, seed, mask_eos and the GenOptions fields);
        trailing_ids: None, or a list with one entry per request (None or a sequence of text ids, [EXT] streaming-text input)"""
        n = len(prompts)
        reqs = (Request * n)()
        opts = [self._opts(i, repetition_penalty, predictor_temperature, predictor_top_k, predictor_top_p) for i in range(n)]
        keep = []
        for i, pr in enumerate(prompts):
            pr = np.ascontiguousarray(pr, np.float32)
            ms = self._per(max_steps, i)
            codes = np.zeros(max(ms, 1) * 16, np.int32)
            pcm = np.zeros(max(ms * pcm_per_frame, 1), np.float32) if want_pcm else None
            keep.append((pr, codes, pcm))
            r = reqs[i]
            self._fill(r, pr, i, max_steps, temperature, top_k, top_p, seed, mask_eos)
            r.codes_out = codes.ctypes.data
            r.pcm_out = pcm.ctypes.data if pcm is not None else None
            r.pcm_capacity = pcm.size if pcm is not None else 0
        if trailing_ids is not None:
            if len(trailing_ids) != n:
                raise Q3Error("trailing_ids needs one entry per request")
            trs = [np.ascontiguousarray(t if t is not None else [], np.int32) for t in trailing_ids]
            ptrs = (C.c_void_p * n)(*[t.ctypes.data if t.size else None for t in trs])
            cnt = np.array([t.size for t in trs], np.int32)
            arr = (GenOptions * n)(*[o if o is not None else GenOptions(**GEN_DEFAULTS) for o in opts])
            _chk(lib().q3tts_generate_batch_trailing(self.h, reqs, n, 1 if want_pcm else 0, arr, ptrs, _p(cnt)))
        elif all(o is None for o in opts):
            _chk(lib().q3tts_generate_batch(self.h, reqs, n, 1 if want_pcm else 0))
        else:
            arr = (GenOptions * n)(*[o if o is not None else GenOptions(**GEN_DEFAULTS) for o in opts])
            _chk(lib().q3tts_generate_batch_ex(self.h, reqs, n, 1 if want_pcm else 0, arr))
        out = []
        for i in range(n):
            nf = reqs[i].n_frames
            out.append({"codes": keep[i][1][: nf * 16].reshape(nf, 16).copy(),
                        "pcm": keep[i][2][: reqs[i].n_pcm].copy() if want_pcm else None,
                        "prefill_ms": reqs[i].prefill_ms, "first_chunk_ms": reqs[i].first_chunk_ms, "total_ms": reqs[i].total_ms})
        return out

    def stats(self):
        s = Stats()
        _chk(lib().q3tts_engine_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def reset_stats(self):
        lib().q3tts_engine_reset_stats(self.h)

    def set_instrument(self, on):
        lib().q3tts_engine_set_instrument(self.h, 1 if on else 0)

    def bytes_per_step(self, batch, mean_ctx):
        return lib().q3tts_engine_bytes_per_step(self.h, batch, mean_ctx)

    def pred_table_bytes(self):
        """device bytes of the predictor's layer-0 q/k/v table (q3tts_pred_table_bytes; 0 = off)"""
        L = lib()
        L.q3tts_pred_table_bytes.restype = C.c_int64
        L.q3tts_pred_table_bytes.argtypes = [C.c_void_p]
        return int(L.q3tts_pred_table_bytes(self.h))


class TfContext:  # LlamaModel + LlamaContext at the embedding level (llama/mod.rs:326-513)
    def __init__(self, path, n_ctx=4096, max_tok=64):
        h = C.c_void_p()
        _chk(lib().q3tts_tf_open(path.encode(), n_ctx, max_tok, C.byref(h)))
        self.h = h.value
        d = [C.c_int32() for _ in range(4)]
        lib().q3tts_tf_dims(self.h, *[C.byref(x) for x in d])
        self.n_embd, self.n_layer, self.n_head, self.n_vocab = [x.value for x in d]

    def close(self):
        if self.h:
            lib().q3tts_tf_close(self.h)
        self.h = None

    def clear(self):
        lib().q3tts_tf_clear(self.h)

    def eval(self, x, pos4, row0=0, row1=0):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.n_embd)
        pos4 = np.ascontiguousarray(pos4, np.int32).reshape(-1, 4)
        n = x.shape[0]
        hid = np.zeros((n, self.n_embd), np.float32)
        logits = np.zeros((n, max(row1 - row0, 1)), np.float32)
        _chk(lib().q3tts_tf_eval(self.h, _p(x), _p(pos4), n, _p(hid), _p(logits) if row1 > row0 else None, row0, row1))
        return hid, logits[:, : max(row1 - row0, 0)]


class Decoder:  # AudioDecoder (onnx.rs:324-496)
    def __init__(self, path, n_streams=1, max_frames=64, max_group=1):
        h = C.c_void_p()
        if max_group > 1 or max_frames != 64:
            _chk(lib().q3tts_decoder_create_ex(path.encode(), n_streams, max_frames, max_group, C.byref(h)))
        else:
            _chk(lib().q3tts_decoder_create(path.encode(), n_streams, C.byref(h)))
        self.h = h.value
        self.spf = lib().q3tts_decoder_samples_per_frame(self.h)

    def close(self):
        if self.h:
            lib().q3tts_decoder_destroy(self.h)
        self.h = None

    def reset(self, stream=0):
        _chk(lib().q3tts_decoder_reset(self.h, stream))

    def decode(self, codes, is_last=False, stream=0):
        codes = np.ascontiguousarray(codes, np.int64).reshape(-1, 16)
        wav = np.zeros(codes.shape[0] * self.spf, np.float32)
        valid = C.c_int64(0)
        _chk(lib().q3tts_decoder_decode(self.h, stream, _p(codes), codes.shape[0], 1 if is_last else 0, _p(wav), C.byref(valid)))
        return wav[: valid.value]


    # ---- [EXT] codec preambles: device-side snapshots of a stream's state (q3tts_decoder_snapshot_*) ----
    def snapshot_create(self, stream=0):
        s = C.c_int32()
        _chk(lib().q3tts_decoder_snapshot_create(self.h, stream, C.byref(s)))
        return s.value

    def snapshot_restore(self, snapshot, stream=0):
        _chk(lib().q3tts_decoder_snapshot_restore(self.h, snapshot, stream))

    def snapshot_free(self, snapshot):
        _chk(lib().q3tts_decoder_snapshot_free(self.h, snapshot))

    def snapshot_bytes(self):
        return int(lib().q3tts_decoder_snapshot_bytes(self.h))

    def state_export(self, stream=0):
        L = lib()
        L.q3tts_decoder_state_floats.restype = C.c_int64
        L.q3tts_decoder_state_floats.argtypes = [C.c_void_p]
        L.q3tts_decoder_state_export.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        buf = np.zeros(L.q3tts_decoder_state_floats(self.h), np.float32)
        _chk(L.q3tts_decoder_state_export(self.h, stream, _p(buf), buf.size))
        return buf

    def state_import(self, blob, stream=0):
        lib().q3tts_decoder_state_import.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        blob = np.ascontiguousarray(blob, np.float32)
        _chk(lib().q3tts_decoder_state_import(self.h, stream, _p(blob), blob.size))

    def state_layout(self):
        L = lib()
        L.q3tts_decoder_state_entry.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        n = L.q3tts_decoder_state_entry(self.h, -1, None, None, None, None)
        out = []
        for i in range(n):
            nm, off, r, c = C.c_char_p(), C.c_int64(), C.c_int32(), C.c_int32()
            L.q3tts_decoder_state_entry(self.h, i, C.byref(nm), C.byref(off), C.byref(r), C.byref(c))
            out.append((nm.value.decode(), off.value, r.value, c.value))
        return out

    def decode_group(self, streams, codes):
        """codes [G][n_frames][16] for G distinct streams -> wav [G][n_frames*spf] (one decode pass for the whole group)"""
        st = np.ascontiguousarray(streams, np.int32)
        codes = np.ascontiguousarray(codes, np.int64).reshape(st.size, -1, 16)
        wav = np.zeros((st.size, codes.shape[1] * self.spf), np.float32)
        _chk(lib().q3tts_decoder_decode_group(self.h, st.size, _p(st), _p(codes), codes.shape[1], _p(wav)))
        return wav


def op_gemv_q8(w_raw, n, k, xq, xd, lpr=0):
    xq = np.ascontiguousarray(xq, np.int8).reshape(-1, k)
    xd = np.ascontiguousarray(xd, np.uint16).reshape(-1, k // 32)
    w_raw = np.ascontiguousarray(w_raw, np.uint8)
    y = np.zeros((xq.shape[0], n), np.float32)
    _chk(lib().q3tts_op_gemv_q8(_p(w_raw), n, k, _p(xq), _p(xd), xq.shape[0], _p(y), lpr))
    return y


def op_gateup_q8(w_raw, ff, k, xq, xd):
    """fused gate/up + SwiGLU + quant of the batched layer path: w_raw = Q8_0 rows [2*ff][k/32][34] (gate first)"""
    xq = np.ascontiguousarray(xq, np.int8).reshape(-1, k)
    xd = np.ascontiguousarray(xd, np.uint16).reshape(-1, k // 32)
    w_raw = np.ascontiguousarray(w_raw, np.uint8)
    aq = np.zeros((xq.shape[0], ff), np.int8)
    ad = np.zeros((xq.shape[0], ff // 32), np.uint16)
    _chk(lib().q3tts_op_gateup_q8(_p(w_raw), ff, k, _p(xq), _p(xd), xq.shape[0], _p(aq), _p(ad)))
    return aq, ad


def op_matmul_float(w_raw, ggml_type, n, k, x, row0=0, nrows=None):
    """w_raw: the row-major weight bytes (f32 / f16 / bf16 per ggml_type); x [ntok][k] f32 -> y [ntok][nrows] f32"""
    nrows = n - row0 if nrows is None else nrows
    w_raw = np.ascontiguousarray(w_raw)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros((x.shape[0], nrows), np.float32)
    _chk(lib().q3tts_op_matmul_float(_p(w_raw), ggml_type, n, k, row0, nrows, _p(x), x.shape[0], _p(y)))
    return y


def op_rmsnorm_quant(x, g, eps=1e-6):
    x = np.ascontiguousarray(x, np.float32)
    x2 = x.reshape(-1, x.shape[-1])
    d = x2.shape[1]
    g = np.ascontiguousarray(g, np.float32)
    xq = np.zeros(x2.shape, np.int8)
    xd = np.zeros((x2.shape[0], d // 32), np.uint16)
    xn = np.zeros(x2.shape, np.float32)
    _chk(lib().q3tts_op_rmsnorm_quant(_p(x2), _p(g), d, x2.shape[0], eps, _p(xq), _p(xd), _p(xn)))
    return xq, xd, xn


def op_swiglu_quant(gu, ff):
    gu = np.ascontiguousarray(gu, np.float32).reshape(-1, 2 * ff)
    aq = np.zeros((gu.shape[0], ff), np.int8)
    ad = np.zeros((gu.shape[0], ff // 32), np.uint16)
    _chk(lib().q3tts_op_swiglu_quant(_p(gu), ff, gu.shape[0], _p(aq), _p(ad)))
    return aq, ad


def op_argmax(logits, start, end, mask_idx=-1):
    logits = np.ascontiguousarray(logits, np.float32)
    out = np.zeros(1, np.int32)
    _chk(lib().q3tts_op_argmax(_p(logits), logits.size, start, end, mask_idx, _p(out)))
    return int(out[0])


def op_sample(logits, temperature, top_k, top_p, seed, n_draws=1, mask_idx=-1):
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    out = np.zeros(n_draws, dtype=np.int32)
    _chk(lib().q3tts_op_sample(_p(logits), logits.size, temperature, top_k, top_p, seed, mask_idx, n_draws, _p(out)))
    return out


def op_sample_rows(logits, temperature, top_k, top_p, seed, n_draws=1, kernel=0, penalty=None, history=None):
    """[EXT] the frame graph's sampler kernels over B rows: kernel 0 = k_sample (talker, optional penalty + per-row history lists of code_0),
    kernel 1 = k_sample_pred (code predictor).  Per-row parameters are arrays of length B.  Returns [n_draws][B] codes."""
    lg = np.ascontiguousarray(logits, np.float32)
    B, n = lg.shape
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, np.float32), (B,)))
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(top_k, np.int32), (B,)))
    p = np.ascontiguousarray(np.broadcast_to(np.asarray(top_p, np.float32), (B,)))
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, np.uint64), (B,)))
    pen = hist = hlen = None
    cap = 1
    if penalty is not None:
        pen = np.ascontiguousarray(np.broadcast_to(np.asarray(penalty, np.float32), (B,)))
        history = history if history is not None else [[] for _ in range(B)]
        cap = max(1, max(len(h) for h in history))
        hist = np.full((B, cap), -1, np.int32)
        hlen = np.array([len(h) for h in history], np.int32)
        for b, h in enumerate(history):
            hist[b, : len(h)] = h
    out = np.zeros((n_draws, B), np.int32)
    _chk(lib().q3tts_op_sample_rows(kernel, _p(lg), B, n, _p(t), _p(k), _p(p), _p(pen), _p(s), _p(hist), _p(hlen), cap, n_draws, _p(out)))
    return out


def op_project(x, w, b):
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    y = np.zeros(b.size, np.float32)
    _chk(lib().q3tts_op_project(_p(x), _p(w), _p(b), x.size, b.size, _p(y)))
    return y


# codec GEMM forms (include/q3tts.h Q3TTS_GEMM_*) and epilogues (Q3TTS_EPI_*)
GEMM_FORMS = {"AUTO": 0, "SKINNY4": 1, "SKINNY8": 2, "SKINNY16": 3, "F32_1": 4, "F32_2": 5, "H1": 6, "H1_EPL": 7, "H2": 8, "H2_EPL": 9,
              "H3": 10, "H3_EPL": 11}
GEMM_FORM_NAMES = {v: k for k, v in GEMM_FORMS.items()}
EPI_NONE, EPI_GELU, EPI_RES_SCALE, EPI_RES, EPI_SNAKE = range(5)


class CodecGemmDesc(C.Structure):  # q3tts_codec_gemm_desc
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("cin", C.c_int32), ("taps", C.c_int32), ("dil", C.c_int32),
                ("A", C.c_void_p), ("a_rows", C.c_int64), ("lda", C.c_int32), ("a_segT", C.c_int32), ("a_skip", C.c_int32),
                ("a_split", C.c_int32), ("o_split", C.c_int32),
                ("W", C.c_void_p), ("bias", C.c_void_p),
                ("epi", C.c_int32), ("res", C.c_void_p), ("res_floats", C.c_int64), ("ldr", C.c_int32), ("r_segT", C.c_int32), ("r_skip", C.c_int64),
                ("scale", C.c_void_p), ("snake_ea", C.c_void_p), ("snake_ib", C.c_void_p),
                ("out", C.c_void_p), ("out_floats", C.c_int64), ("out_off", C.c_int64), ("ldo", C.c_int32), ("o_segT", C.c_int32), ("o_skip", C.c_int64),
                ("ws_floats", C.c_int64),
                ("form", C.c_int32), ("ksplit", C.c_int32), ("reducer", C.c_int32),
                ("form_ran", C.c_int32), ("ksplit_ran", C.c_int32), ("reducer_ran", C.c_int32)]


def _codec_gemm_desc(M, N, cin, taps, dil, lda, a_rows, a_segT, a_skip, epi, ldr, res_floats, r_segT, r_skip, ldo, out_floats, out_off,
                     o_segT, o_skip, a_split, o_split, ws_floats, form, ksplit, reducer):
    d = CodecGemmDesc()
    d.M, d.N, d.cin, d.taps, d.dil = M, N, cin, taps, dil
    d.lda, d.a_rows, d.a_segT, d.a_skip = lda, a_rows, a_segT, a_skip
    d.epi, d.ldr, d.res_floats, d.r_segT, d.r_skip = epi, ldr, res_floats, r_segT, r_skip
    d.ldo, d.out_floats, d.out_off, d.o_segT, d.o_skip = ldo, out_floats, out_off, o_segT, o_skip
    d.a_split, d.o_split, d.ws_floats = int(bool(a_split)), int(bool(o_split)), ws_floats
    d.form = GEMM_FORMS[form] if isinstance(form, str) else form
    d.ksplit, d.reducer = ksplit, reducer
    return d


def op_codec_gemm(A, W, M, cin, taps=1, dil=1, out=None, ldo=None, out_off=0, o_segT=0, o_skip=0, a_segT=0, a_skip=0, bias=None,
                  epi=EPI_NONE, res=None, ldr=0, r_segT=0, r_skip=0, scale=None, ea=None, ib=None, a_split=False, o_split=False,
                  ws_floats=1 << 22, form="AUTO", ksplit=1, reducer=-1):
    """one codec-decoder GEMM on the device (q3tts_op_codec_gemm).  A: [a_rows][lda] (float32, or the bit pattern of split rows);
    W: [N][cin*taps] float32; out: the whole output buffer (1-D float32 / uint32; uploaded, then returned written back whole).
    Returns (out buffer, (form name, ksplit, reducer)) of what ran."""
    A = np.ascontiguousarray(A)
    assert A.ndim == 2 and A.dtype.itemsize == 4
    W = np.ascontiguousarray(W, np.float32)
    N = W.shape[0]
    ldo = N if ldo is None else ldo
    if out is None:
        out = np.zeros(out_off + M * ldo, np.float32)
    out = np.array(out, copy=True).reshape(-1)
    assert out.dtype.itemsize == 4
    vecs = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (bias, scale, ea, ib)]
    for v in vecs:
        assert v is None or v.size == N
    res = None if res is None else np.ascontiguousarray(res, np.float32).reshape(-1)
    d = _codec_gemm_desc(M, N, cin, taps, dil, A.shape[1], A.shape[0], a_segT, a_skip, epi, ldr, 0 if res is None else res.size, r_segT, r_skip,
                         ldo, out.size, out_off, o_segT, o_skip, a_split, o_split, ws_floats, form, ksplit, reducer)
    d.A, d.W, d.out, d.res = _p(A), _p(W), _p(out), _p(res)
    d.bias, d.scale, d.snake_ea, d.snake_ib = (_p(v) for v in vecs)
    lib().q3tts_op_codec_gemm.argtypes = [C.POINTER(CodecGemmDesc)]
    _chk(lib().q3tts_op_codec_gemm(C.byref(d)))
    return out, (GEMM_FORM_NAMES[d.form_ran], d.ksplit_ran, d.reducer_ran)


def codec_gemm_plan(M, N, cin, taps=1, dil=1, lda=None, ldo=None, out_off=0, o_segT=0, o_skip=0, a_segT=0, a_skip=0, epi=EPI_NONE, ldr=0,
                    r_segT=0, r_skip=0, a_split=False, o_split=False, ws_floats=1 << 22):
    """the decoder's dispatch for one GEMM shape (host only; every buffer taken as 16-byte aligned, out shifted by out_off floats)"""
    d = _codec_gemm_desc(M, N, cin, taps, dil, cin if lda is None else lda, 0, a_segT, a_skip, epi, ldr, 0, r_segT, r_skip,
                         N if ldo is None else ldo, 0, out_off, o_segT, o_skip, a_split, o_split, ws_floats, 0, 1, -1)
    lib().q3tts_codec_gemm_plan.argtypes = [C.POINTER(CodecGemmDesc)]
    _chk(lib().q3tts_codec_gemm_plan(C.byref(d)))
    return GEMM_FORM_NAMES[d.form_ran], d.ksplit_ran, d.reducer_ran


def codec_gemm_tap_reuse(M, N, cin, taps=1, dil=1, lda=None, ldo=None, out_off=0, o_segT=0, o_skip=0, a_segT=0, a_skip=0, epi=EPI_NONE, ldr=0,
                         r_segT=0, r_skip=0, a_split=False, o_split=False, ws_floats=1 << 22, form="AUTO", ksplit=1, reducer=-1):
    """does this GEMM run k_conv_gemm_h3's tap-reusing main loop?  (host only; form AUTO: as the decoder dispatches it, else the forced form)"""
    d = _codec_gemm_desc(M, N, cin, taps, dil, cin if lda is None else lda, 0, a_segT, a_skip, epi, ldr, 0, r_segT, r_skip,
                         N if ldo is None else ldo, 0, out_off, o_segT, o_skip, a_split, o_split, ws_floats, form, ksplit, reducer)
    lib().q3tts_codec_gemm_tap_reuse.argtypes = [C.POINTER(CodecGemmDesc)]
    r = lib().q3tts_codec_gemm_tap_reuse(C.byref(d))
    if r < 0:
        _chk(r)
    return bool(r)


# codec non-GEMM kernels (include/q3tts.h Q3TTS_CK_*) and the per-stream frame limit
CODEC_KERNELS = {"RVQ_SUM": 0, "RMSNORM_ROWS": 1, "LAYERNORM_ROWS": 2, "ROPE_APPEND": 3, "WINDOW_ATTN": 4, "SWIGLU_ROWS": 5, "DWCONV7": 6,
                 "SNAKE": 7, "SNAKE_SPLIT": 8, "CONV_OUT_WAVE": 9, "CONV_OUT_WIN": 10, "HIST_LOAD": 11, "HIST_SAVE": 12, "HIST_ZERO": 13}
CODEC_MAX_FRAMES = 65536


class CodecKernelDesc(C.Structure):  # q3tts_codec_kernel_desc
    _fields_ = [("kernel", C.c_int32), ("G", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("H", C.c_int32),
                ("n_heads", C.c_int32), ("head_dim", C.c_int32), ("window", C.c_int32), ("rope_base", C.c_float), ("eps", C.c_float),
                ("bias", C.c_float), ("meta", C.c_void_p), ("codes", C.c_void_p), ("n_q", C.c_int32), ("cb_size", C.c_int32),
                ("n_streams", C.c_int32), ("stream", C.c_int32), ("inp", C.c_void_p * 3), ("in_floats", C.c_int64 * 3),
                ("p0", C.c_void_p), ("p1", C.c_void_p), ("p0_floats", C.c_int64), ("p1_floats", C.c_int64),
                ("out", C.c_void_p * 3), ("out_floats", C.c_int64 * 3)]


def op_codec_kernel(kernel, G, T, C_, H=0, ins=(), outs=(), p0=None, p1=None, meta=None, codes=None, n_q=0, cb_size=0, n_heads=0,
                    head_dim=0, window=0, rope_base=10000.0, eps=1e-5, bias=0.0, n_streams=0, stream=0):
    """one codec-decoder kernel on the device (q3tts_op_codec_kernel).  ins / outs: up to 3 float32 (or 4-byte) arrays each, None allowed;
    the outputs are uploaded and returned written back whole (copies).  meta: [3G] int64 (slot, kv_len, frames seen)."""
    d = CodecKernelDesc()
    d.kernel = CODEC_KERNELS[kernel] if isinstance(kernel, str) else kernel
    d.G, d.T, d.C, d.H = G, T, C_, H
    d.n_heads, d.head_dim, d.window, d.rope_base, d.eps, d.bias = n_heads, head_dim, window, rope_base, eps, bias
    d.n_q, d.cb_size, d.n_streams, d.stream = n_q, cb_size, n_streams, stream
    keep = []
    if meta is not None:
        meta = np.ascontiguousarray(meta, np.int64).reshape(-1)
        assert meta.size == 3 * G
        d.meta = meta.ctypes.data; keep.append(meta)
    if codes is not None:
        codes = np.ascontiguousarray(codes, np.int64).reshape(-1)
        assert codes.size == G * T * n_q
        d.codes = codes.ctypes.data; keep.append(codes)
    for i, a in enumerate(ins):
        if a is not None:
            a = np.ascontiguousarray(a).reshape(-1)
            assert a.dtype.itemsize == 4
            d.inp[i], d.in_floats[i] = a.ctypes.data, a.size; keep.append(a)
    res = []
    for i, a in enumerate(outs):
        a = None if a is None else np.array(a, copy=True).reshape(-1)
        if a is not None:
            assert a.dtype.itemsize == 4
            d.out[i], d.out_floats[i] = a.ctypes.data, a.size
        res.append(a)
    for nm, a in (("p0", p0), ("p1", p1)):
        if a is not None:
            a = np.ascontiguousarray(a, np.float32).reshape(-1)
            setattr(d, nm, a.ctypes.data); setattr(d, nm + "_floats", a.size); keep.append(a)
    lib().q3tts_op_codec_kernel.argtypes = [C.POINTER(CodecKernelDesc)]
    _chk(lib().q3tts_op_codec_kernel(C.byref(d)))
    return res


def mel(audio):
    audio = np.ascontiguousarray(audio, np.float32)
    n = lib().q3tts_mel_frames(audio.size)
    out = np.zeros((max(n, 1), 128), np.float32)   # never an empty buffer: a null pointer is an error of the C entry
    src = audio if audio.size else np.zeros(1, np.float32)
    _chk(lib().q3tts_mel(_p(src), audio.size, _p(out)))
    return out[:n]


def mel_frames(n):
    return int(lib().q3tts_mel_frames(int(n)))


def mel_tables():
    """the f32 tables the mel kernel reads: periodic Hann [1024], Slaney filterbank [128, 513] (host only)"""
    hann, fb = np.zeros(1024, np.float32), np.zeros((128, 513), np.float32)
    _chk(lib().q3tts_mel_tables(_p(hann), _p(fb)))
    return hann, fb


class OnnxSession:
    """ONNX graph executed on the GPU through the C ABI (q3tts_onnx_session_*): the role `ort::Session` has in the reference's encoders"""

    def __init__(self, path, device=0):
        L = lib()
        L.q3tts_onnx_session_open.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_void_p)]
        L.q3tts_onnx_session_close.argtypes = [C.c_void_p]
        L.q3tts_onnx_session_unsupported.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.q3tts_onnx_session_set_input.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        L.q3tts_onnx_session_run.argtypes = [C.c_void_p]
        L.q3tts_onnx_session_output_info.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        L.q3tts_onnx_session_output.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]
        L.q3tts_onnx_session_launches.restype = C.c_int64
        L.q3tts_onnx_session_launches.argtypes = [C.c_void_p]
        h = C.c_void_p()
        _chk(L.q3tts_onnx_session_open(path.encode(), device, C.byref(h)))
        self.h = h.value

    def close(self):
        if self.h:
            lib().q3tts_onnx_session_close(self.h)
        self.h = None

    def unsupported(self):
        buf = C.create_string_buffer(4096)
        n = lib().q3tts_onnx_session_unsupported(self.h, buf, 4096)
        return [x for x in buf.value.decode().split(",") if x] if n else []

    def run(self, feeds, outputs):
        """feeds: {name: ndarray (float32 or int64)}; returns {name: ndarray} for the requested graph outputs"""
        keep = []
        for name, arr in feeds.items():
            a = np.ascontiguousarray(arr, dtype=np.int64 if np.issubdtype(np.asarray(arr).dtype, np.integer) else np.float32)
            keep.append(a)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            _chk(lib().q3tts_onnx_session_set_input(self.h, name.encode(), 7 if a.dtype == np.int64 else 1, a.ctypes.data, shape, a.ndim))
        _chk(lib().q3tts_onnx_session_run(self.h))
        res = {}
        for name in outputs:
            dt, rk = C.c_int32(), C.c_int32()
            shape = (C.c_int64 * 8)()
            _chk(lib().q3tts_onnx_session_output_info(self.h, name.encode(), C.byref(dt), C.byref(rk), shape))
            shp = tuple(shape[i] for i in range(rk.value))
            out = np.empty(shp, dtype=np.int64 if dt.value == 7 else np.float32)
            _chk(lib().q3tts_onnx_session_output(self.h, name.encode(), out.ctypes.data, out.nbytes))
            res[name] = out.astype(bool) if dt.value == 9 else out
        return res

    def launches(self):
        return lib().q3tts_onnx_session_launches(self.h)


class OnnxDecoder:
    """The exported streaming decoder graph run through the executor with its state on the device (AudioDecoder, onnx.rs:322-458)"""

    def __init__(self, path, device=0):
        L = lib()
        L.q3tts_onnx_decoder_open.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_void_p)]
        L.q3tts_onnx_decoder_close.argtypes = [C.c_void_p]
        L.q3tts_onnx_decoder_reset.argtypes = [C.c_void_p]
        L.q3tts_onnx_decoder_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        h = C.c_void_p()
        _chk(L.q3tts_onnx_decoder_open(path.encode(), device, C.byref(h)))
        self.h = h.value

    def close(self):
        if self.h:
            lib().q3tts_onnx_decoder_close(self.h)
        self.h = None

    def reset(self):
        _chk(lib().q3tts_onnx_decoder_reset(self.h))

    def decode(self, codes, is_final=False, max_samples_per_frame=1920):
        codes = np.ascontiguousarray(codes, np.int64).reshape(-1, 16)
        out = np.zeros(max(codes.shape[0], 1) * max_samples_per_frame, np.float32)
        n = C.c_int64()
        rc = lib().q3tts_onnx_decoder_decode(self.h, codes.ctypes.data, codes.shape[0], 1 if is_final else 0, out.ctypes.data, out.size, C.byref(n))
        if rc == 2:  # buffer too small: the chunk is kept in the handle, fetch it again into one that fits
            out = np.zeros(n.value, np.float32)
            lib().q3tts_onnx_decoder_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            rc = lib().q3tts_onnx_decoder_fetch(self.h, out.ctypes.data, out.size, C.byref(n))
        _chk(rc)
        return out[: n.value].copy()


ATTN_FORMS = {"AUTO": 0, "UNFUSED": 1, "FUSED": 2, "SHORT1": 3, "SHORT2": 4, "GGML": 5}
ATTN_FORM_NAMES = {v: k for k, v in ATTN_FORMS.items()}


class AttentionDesc(C.Structure):  # q3tts_attention_desc
    _fields_ = [("n_head", C.c_int32), ("n_kv", C.c_int32), ("n_layer", C.c_int32), ("layer", C.c_int32), ("ntok", C.c_int32),
                ("qkv", C.c_void_p), ("qkv_stride", C.c_int32), ("q_norm", C.c_void_p), ("k_norm", C.c_void_p),
                ("eps", C.c_float), ("rope_base", C.c_float), ("n_ctx", C.c_int32), ("mrope_sec", C.c_int32 * 4),
                ("seq", C.c_void_p), ("slot", C.c_void_p), ("pos", C.c_void_p), ("uniform_pos", C.c_int32),
                ("page_table", C.c_void_p), ("n_seq", C.c_int32), ("max_pages", C.c_int32),
                ("k_cache", C.c_void_p), ("v_cache", C.c_void_p), ("n_pages", C.c_int32),
                ("fused", C.c_int32), ("fused_max_tok", C.c_int32), ("same_seq", C.c_int32), ("short_attn_min", C.c_int32),
                ("hpw1_max", C.c_int32), ("float_mode", C.c_int32), ("ggml_mode", C.c_int32),
                ("form", C.c_int32), ("att", C.c_void_p), ("aq", C.c_void_p), ("ad", C.c_void_p), ("form_ran", C.c_int32)]


def _attn_flags(d, fused, fused_max_tok, same_seq, short_attn_min, hpw1_max, float_mode, ggml_mode):
    d.fused, d.fused_max_tok, d.same_seq, d.short_attn_min = int(fused), fused_max_tok, int(same_seq), short_attn_min
    d.hpw1_max, d.float_mode, d.ggml_mode = hpw1_max, int(float_mode), int(ggml_mode)


def attention_plan(ntok, n_head=16, n_kv=8, fused=True, fused_max_tok=8, same_seq=False, short_attn_min=0, hpw1_max=0, float_mode=False,
                   ggml_mode=False):
    """the attention form Transformer::forward runs for one step with these flags (host only; hpw1_max 0 = the engine's threshold)"""
    d = AttentionDesc()
    d.ntok, d.n_head, d.n_kv = ntok, n_head, n_kv
    _attn_flags(d, fused, fused_max_tok, same_seq, short_attn_min, hpw1_max, float_mode, ggml_mode)
    lib().q3tts_attention_plan.argtypes = [C.POINTER(AttentionDesc)]
    _chk(lib().q3tts_attention_plan(C.byref(d)))
    return ATTN_FORM_NAMES[d.form_ran]


def op_attention(qkv, q_norm, k_norm, k_cache, v_cache, n_head, n_kv, n_layer, layer, eps=1e-6, rope_base=1e6, n_ctx=4096,
                 mrope_sec=(0, 0, 0, 0), seq=None, slot=None, pos=None, uniform_pos=-1, page_table=None, form="AUTO", fused=True,
                 fused_max_tok=8, same_seq=False, short_attn_min=0, hpw1_max=0, float_mode=False, ggml_mode=False, keys=None):
    """one layer's attention step on the device (q3tts_op_attention).  qkv [ntok][>= (n_head + 2 n_kv) * 128] f32; k_cache / v_cache: the
    paged f16 caches as uint16 [n_pages][n_layer][n_kv][8192] (copied; the written-back caches are returned); seq / slot [ntok] and
    pos [ntok][4], or uniform_pos >= 0; page_table [n_seq][max_pages] or None (identity).
    keys (q3tts_op_attention_keyed): uint64 [ntok][key_stride] argmax keys; qkv is then a table and token t reads the row keys[t][0] selects.
    Returns dict(att=[ntok][n_head*128] f32 or None, aq, ad (None for GGML), k_cache, v_cache, form=name of what ran; keyed: qkv = the
    table as written back)."""
    if keys is not None:
        keys = np.ascontiguousarray(keys, np.uint64)
        keys = keys.reshape(keys.shape[0], -1)
        qkv = np.array(qkv, np.float32, copy=True, order="C")
        ntok = keys.shape[0]
    else:
        qkv = np.ascontiguousarray(qkv, np.float32)
        ntok = qkv.shape[0]
    q_norm = np.ascontiguousarray(q_norm, np.float32)
    k_norm = np.ascontiguousarray(k_norm, np.float32)
    kc = np.array(k_cache, np.uint16, copy=True, order="C")
    vc = np.array(v_cache, np.uint16, copy=True, order="C")
    assert kc.shape == vc.shape and kc.size % (n_layer * n_kv * 8192) == 0
    d = AttentionDesc()
    d.n_head, d.n_kv, d.n_layer, d.layer, d.ntok = n_head, n_kv, n_layer, layer, ntok
    d.qkv, d.qkv_stride, d.q_norm, d.k_norm = _p(qkv), qkv.shape[1], _p(q_norm), _p(k_norm)
    d.eps, d.rope_base, d.n_ctx = eps, rope_base, n_ctx
    for i in range(4):
        d.mrope_sec[i] = int(mrope_sec[i])
    keep = []
    if uniform_pos < 0:
        seq = np.ascontiguousarray(seq, np.int32)
        slot = np.ascontiguousarray(slot, np.int32)
        pos = np.ascontiguousarray(pos, np.int32).reshape(ntok, 4)
        keep += [seq, slot, pos]
        d.seq, d.slot, d.pos = _p(seq), _p(slot), _p(pos)
    d.uniform_pos = uniform_pos
    if page_table is not None:
        page_table = np.ascontiguousarray(page_table, np.int32)
        keep.append(page_table)
        d.page_table, d.n_seq, d.max_pages = _p(page_table), page_table.shape[0], page_table.shape[1]
    d.k_cache, d.v_cache, d.n_pages = _p(kc), _p(vc), kc.size // (n_layer * n_kv * 8192)
    _attn_flags(d, fused, fused_max_tok, same_seq, short_attn_min, hpw1_max, float_mode, ggml_mode)
    d.form = ATTN_FORMS[form]
    att = np.full((ntok, n_head * 128), np.nan, np.float32)
    aq = np.zeros((ntok, n_head * 128), np.int8)
    ad = np.zeros((ntok, n_head * 4), np.uint16)
    d.att, d.aq, d.ad = _p(att), _p(aq), _p(ad)
    if keys is not None:
        lib().q3tts_op_attention_keyed.argtypes = [C.POINTER(AttentionDesc), C.c_void_p, C.c_int32, C.c_int32]
        _chk(lib().q3tts_op_attention_keyed(C.byref(d), _p(keys), keys.shape[1], qkv.shape[0]))
    else:
        lib().q3tts_op_attention.argtypes = [C.POINTER(AttentionDesc)]
        _chk(lib().q3tts_op_attention(C.byref(d)))
    ran = ATTN_FORM_NAMES[d.form_ran]
    r = dict(att=None if ran == "FUSED" else att, aq=None if ran == "GGML" else aq, ad=None if ran == "GGML" else ad,
             k_cache=kc, v_cache=vc, form=ran)
    if keys is not None:
        r["qkv"] = qkv
    return r


def op_gemv_kq(parts, k, xq, xd, lpr=0):
    """parts: [(raw bytes ndarray, ggml type, rows)] -> y [ntok, sum rows] through the K-quant GEMV / matrix-core GEMM"""
    L = lib()
    L.q3tts_op_gemv_kq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    raws = [np.ascontiguousarray(p[0]) for p in parts]
    ptrs = (C.c_void_p * len(parts))(*[r.ctypes.data for r in raws])
    types = np.asarray([p[1] for p in parts], np.int32); rows = np.asarray([p[2] for p in parts], np.int32)
    xq = np.ascontiguousarray(xq, np.int8); xd = np.ascontiguousarray(xd, np.uint16)
    ntok = xq.shape[0]
    y = np.zeros((ntok, int(rows.sum())), np.float32)
    _chk(L.q3tts_op_gemv_kq(ptrs, types.ctypes.data, rows.ctypes.data, len(parts), k, xq.ctypes.data, xd.ctypes.data, ntok, y.ctypes.data, lpr))
    return y


def op_gateup_kq(gate_raw, up_raw, qtype, ff, k, xq, xd):
    L = lib()
    L.q3tts_op_gateup_kq.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    g = np.ascontiguousarray(gate_raw); u = np.ascontiguousarray(up_raw)
    xq = np.ascontiguousarray(xq, np.int8); xd = np.ascontiguousarray(xd, np.uint16)
    ntok = xq.shape[0]
    aq = np.zeros((ntok, ff), np.int8); ad = np.zeros((ntok, ff // 32), np.uint16)
    _chk(L.q3tts_op_gateup_kq(g.ctypes.data, u.ctypes.data, qtype, ff, k, xq.ctypes.data, xd.ctypes.data, ntok, aq.ctypes.data, ad.ctypes.data))
    return aq, ad


def text_nfc(text):
    """NFC as the tokenizer's normaliser applies it (q3tts_text_nfc)"""
    L = lib()
    L.q3tts_text_nfc.restype = C.c_int64
    L.q3tts_text_nfc.argtypes = [C.c_char_p, C.c_char_p, C.c_int64]
    raw = text.encode("utf-8", "surrogatepass")
    n = L.q3tts_text_nfc(raw, None, 0)
    buf = C.create_string_buffer(int(n))
    L.q3tts_text_nfc(raw, buf, n)
    return buf.raw[: n - 1].decode("utf-8", "surrogatepass")


def onnx_op_executable(op_type):
    L = lib()
    L.q3tts_onnx_op_executable.argtypes = [C.c_char_p]
    return bool(L.q3tts_onnx_op_executable(op_type.encode()))


class OnnxModel:
    """ONNX ModelProto through the C ABI's reader (q3tts_onnx_*): nodes, attributes, initialisers, I/O contract"""

    def __init__(self, path):
        L = lib()
        L.q3tts_onnx_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.q3tts_onnx_close.argtypes = [C.c_void_p]
        L.q3tts_onnx_counts.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
        L.q3tts_onnx_summary.restype = C.c_int64
        L.q3tts_onnx_summary.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.q3tts_onnx_node.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)] + [C.POINTER(C.c_int32)] * 3
        L.q3tts_onnx_node_input.restype = C.c_char_p
        L.q3tts_onnx_node_input.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_onnx_node_output.restype = C.c_char_p
        L.q3tts_onnx_node_output.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.q3tts_onnx_node_attr_ints.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_int32]
        L.q3tts_onnx_node_attr_float.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.POINTER(C.c_float)]
        L.q3tts_onnx_initializer.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.q3tts_onnx_op_kernel.restype = C.c_char_p
        L.q3tts_onnx_op_kernel.argtypes = [C.c_char_p]
        L.q3tts_onnx_decoder_contract.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        h = C.c_void_p()
        _chk(L.q3tts_onnx_open(path.encode(), C.byref(h)))
        self.h = h.value
        c = [C.c_int32() for _ in range(4)]
        L.q3tts_onnx_counts(self.h, *[C.byref(x) for x in c])
        self.n_nodes, self.n_initializers, self.n_inputs, self.n_outputs = [x.value for x in c]

    def close(self):
        if self.h:
            lib().q3tts_onnx_close(self.h)
        self.h = None

    def summary(self):
        n = lib().q3tts_onnx_summary(self.h, None, 0)
        buf = C.create_string_buffer(n)
        lib().q3tts_onnx_summary(self.h, buf, n)
        return buf.value.decode()

    def node(self, i):
        op, nm = C.c_char_p(), C.c_char_p()
        c = [C.c_int32() for _ in range(3)]
        _chk(lib().q3tts_onnx_node(self.h, i, C.byref(op), C.byref(nm), *[C.byref(x) for x in c]))
        return {"op_type": op.value.decode(), "name": nm.value.decode(),
                "inputs": [lib().q3tts_onnx_node_input(self.h, i, j).decode() for j in range(c[0].value)],
                "outputs": [lib().q3tts_onnx_node_output(self.h, i, j).decode() for j in range(c[1].value)], "n_attr": c[2].value}

    def attr_ints(self, i, name):
        buf = (C.c_int64 * 16)()
        n = lib().q3tts_onnx_node_attr_ints(self.h, i, name.encode(), buf, 16)
        return None if n < 0 else [buf[k] for k in range(min(n, 16))]

    def attr_float(self, i, name):
        f = C.c_float()
        return f.value if lib().q3tts_onnx_node_attr_float(self.h, i, name.encode(), C.byref(f)) == 1 else None

    def initializer(self, i):
        nm, dt, nd, data, nb = C.c_char_p(), C.c_int32(), C.c_int32(), C.c_void_p(), C.c_int64()
        dims = (C.c_int64 * 8)()
        _chk(lib().q3tts_onnx_initializer(self.h, i, C.byref(nm), C.byref(dt), dims, C.byref(nd), C.byref(data), C.byref(nb)))
        raw = C.string_at(data.value, nb.value) if data.value and nb.value else b""
        return {"name": nm.value.decode(), "dtype": dt.value, "dims": [dims[k] for k in range(nd.value)], "raw": raw}

    def decoder_contract(self):
        buf = C.create_string_buffer(4096)
        rc = lib().q3tts_onnx_decoder_contract(self.h, buf, 4096)
        return rc == 0, buf.value.decode()


def onnx_op_kernel(op_type):
    lib().q3tts_onnx_op_kernel.restype = C.c_char_p
    lib().q3tts_onnx_op_kernel.argtypes = [C.c_char_p]
    r = lib().q3tts_onnx_op_kernel(op_type.encode())
    return r.decode() if r else None


class Tokenizer:  # utils/tokenizer.rs:4-38
    def __init__(self, tokenizer_json):
        L = lib()
        L.q3tts_tokenizer_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.q3tts_tokenizer_close.argtypes = [C.c_void_p]
        L.q3tts_tokenizer_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32]
        L.q3tts_tokenizer_decode.restype = C.c_int64
        L.q3tts_tokenizer_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_int64]
        L.q3tts_tokenizer_vocab_size.argtypes = [C.c_void_p]
        h = C.c_void_p()
        _chk(L.q3tts_tokenizer_open(tokenizer_json.encode(), C.byref(h)))
        self.h = h.value

    def close(self):
        if self.h:
            lib().q3tts_tokenizer_close(self.h)
        self.h = None

    def encode(self, text):
        raw = text.encode("utf-8")
        cap = max(16, 2 * len(raw) + 8)
        ids = np.zeros(cap, np.int32)
        n = lib().q3tts_tokenizer_encode(self.h, raw, _p(ids), cap)
        if n < 0:
            raise Q3Error(lib().q3tts_last_error().decode())
        return ids[:n].tolist()

    def decode(self, ids):
        a = np.ascontiguousarray(ids, np.int32)
        n = lib().q3tts_tokenizer_decode(self.h, _p(a), a.size, None, 0)
        if n < 0:
            raise Q3Error(lib().q3tts_last_error().decode())
        buf = C.create_string_buffer(n + 1)
        lib().q3tts_tokenizer_decode(self.h, _p(a), a.size, buf, n + 1)
        return buf.raw[:n].decode("utf-8", errors="replace")


# ---- one linear-layer operation (q3tts_op_linear / q3tts_linear_plan) ----
LOP_GEMV, LOP_GATEUP, LOP_NORM, LOP_NORM_GEMV, LOP_NORM_ARGMAX, LOP_NORM_GATEUP, LOP_F_GEMV, LOP_F_GATEUP = range(8)
LIN_FORMS = ["AUTO", "GEMV_Q8", "GEMM_Q8_TOK", "GEMM_Q8_MFMA", "GEMM_Q8_TILE1", "GEMV_KQ", "GEMM_KQ_MFMA", "GU_Q8_TILE1", "GU_Q8_MFMA", "GU_KQ_MFMA",
             "GU_UNFUSED", "NORM", "NORM_WG", "GEMV_NORM", "GEMV_NORM_ARGMAX", "GU_SWIGLU_NORM", "F_GEMV", "F_MFMA16", "F_MFMA", "F_GU_MFMA16",
             "F_GU_UNFUSED", "GEMM_Q8_WIDE", "GU_Q8_WIDE"]
LIN = {n: i for i, n in enumerate(LIN_FORMS)}


class LinearDesc(C.Structure):  # q3tts_linear_desc
    _fields_ = [("op", C.c_int32), ("form", C.c_int32),
                ("nw", C.c_int32), ("raw", C.c_void_p * 3), ("type", C.c_int32 * 3), ("rows", C.c_int32 * 3), ("kq_layout", C.c_int32),
                ("K", C.c_int32), ("row0", C.c_int32), ("nrows", C.c_int32), ("nrows_valid", C.c_int32), ("ntok", C.c_int32), ("ff", C.c_int32),
                ("lpr", C.c_int32), ("mt", C.c_int32), ("ztiles", C.c_int32), ("fused", C.c_int32),
                ("xq", C.c_void_p), ("xd", C.c_void_p), ("a_rows", C.c_int32),
                ("x", C.c_void_p), ("x_floats", C.c_int64), ("x_off", C.c_int32), ("x_stride", C.c_int32),
                ("h_in", C.c_void_p), ("h_floats", C.c_int64), ("h_stride", C.c_int32),
                ("idx_keys", C.c_void_p), ("idx", C.c_void_p), ("idx_stride", C.c_int32),
                ("parts", C.c_void_p), ("parts_floats", C.c_int64), ("nparts", C.c_int32), ("parts_stride", C.c_int32), ("parts_slab", C.c_int64),
                ("g", C.c_void_p), ("eps", C.c_float),
                ("h_out", C.c_void_p), ("xn_out", C.c_void_p), ("xq_out", C.c_void_p), ("xd_out", C.c_void_p),
                ("keys", C.c_void_p), ("n_keys", C.c_int64), ("key_stride", C.c_int32), ("mask_per_tok", C.c_void_p), ("idx_add", C.c_int32),
                ("out", C.c_void_p), ("out_floats", C.c_int64), ("out_off", C.c_int64), ("out_stride", C.c_int32),
                ("aq", C.c_void_p), ("ad", C.c_void_p),
                ("form_ran", C.c_int32), ("lpr_ran", C.c_int32), ("mt_ran", C.c_int32), ("z_ran", C.c_int32)]


_LIN_SIZES = {"x": "x_floats", "h_in": "h_floats", "parts": "parts_floats", "out": "out_floats", "keys": "n_keys"}


def _linear_desc(op, form, weights, fields):
    """weights: [(raw ndarray, type, rows)]; fields: LinearDesc fields, ndarrays for the buffers (passed by address: outputs are written in place)"""
    d = LinearDesc()
    d.op = op; d.form = LIN[form] if isinstance(form, str) else form; d.fused = 1
    keep = []
    d.nw = len(weights)
    for i, (raw, t, rows) in enumerate(weights):
        raw = np.ascontiguousarray(raw); keep.append(raw)
        d.raw[i] = raw.ctypes.data if raw.size else None; d.type[i] = t; d.rows[i] = rows
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            assert v.flags.c_contiguous, k
            keep.append(v)
            setattr(d, k, v.ctypes.data)
            if k in _LIN_SIZES and k + "_n" not in fields:
                setattr(d, _LIN_SIZES[k], v.size)
        elif v is not None:
            setattr(d, k, v)
    return d, keep


def op_linear(op, form="AUTO", weights=(), **fields):
    """runs one linear-layer op on the device; output ndarrays in fields are overwritten whole.  Returns (form_ran name, lpr, mt, z)"""
    d, keep = _linear_desc(op, form, list(weights), fields)
    lib().q3tts_op_linear.argtypes = [C.POINTER(LinearDesc)]
    _chk(lib().q3tts_op_linear(C.byref(d)))
    return LIN_FORMS[d.form_ran], d.lpr_ran, d.mt_ran, d.z_ran


def linear_plan(op, weights=(), **fields):
    """host only: the engine's dispatch for the op / shape -> (form name, lpr, mt, z)"""
    d, keep = _linear_desc(op, 0, list(weights), fields)
    lib().q3tts_linear_plan.argtypes = [C.POINTER(LinearDesc)]
    _chk(lib().q3tts_linear_plan(C.byref(d)))
    return LIN_FORMS[d.form_ran], d.lpr_ran, d.mt_ran, d.z_ran


def argmax_key(v, idx):
    """host only: kdev.h's pack_key(v, idx) as the library computes it"""
    L = lib()
    L.q3tts_argmax_key.restype = C.c_uint64
    L.q3tts_argmax_key.argtypes = [C.c_float, C.c_int32]
    return int(L.q3tts_argmax_key(v, idx))


# ---- the four token-selection kernels (q3tts_op_select_rows) ----
SEL_SAMPLE, SEL_SAMPLE_PRED, SEL_ARGMAX, SEL_ARGMAX_KEYS = range(4)
SELECT_SENTINEL = 0xA5C3F00D5A3C0FF1   # Q3TTS_SELECT_SENTINEL


class SelectDesc(C.Structure):  # q3tts_select_desc
    _fields_ = [("kernel", C.c_int32), ("B", C.c_int32), ("n", C.c_int32), ("stride", C.c_int32), ("row_off", C.c_int32),
                ("logits", C.c_void_p), ("temperature", C.c_void_p), ("top_k", C.c_void_p), ("top_p", C.c_void_p), ("mask_idx", C.c_void_p),
                ("seed", C.c_void_p), ("draw0", C.c_void_p), ("n_draws", C.c_int32),
                ("penalty", C.c_void_p), ("hist", C.c_void_p), ("hist_len", C.c_void_p), ("hist_cap", C.c_int32), ("cur_code", C.c_void_p),
                ("out_stride", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("add", C.c_int32),
                ("tokens", C.c_void_p), ("out_raw", C.c_void_p), ("draws_out", C.c_void_p)]


def select_outputs(B, n_draws=1, out_stride=1):
    """the output arrays of op_select_rows, every element a sentinel: (tokens [n_draws][B] = -1, raw [n_draws][B*out_stride], draws [B])"""
    return (np.full((n_draws, B), -1, np.int32), np.full((n_draws, B * out_stride), SELECT_SENTINEL, np.uint64),
            np.full(B, 0xFFFFFFFF, np.uint32))


def op_select_rows(kernel, logits, stride=None, row_off=0, temperature=0.0, top_k=0, top_p=1.0, mask_idx=None, seed=0, draw0=None, n_draws=1,
                   penalty=None, history=None, cur_code=None, out_stride=1, start=0, end=None, add=0, outputs=None):
    """one of k_sample / k_sample_pred / k_argmax / k_argmax_keys over the rows logits [B][n] (q3tts_op_select_rows).  Per-row parameters are
    scalars or arrays of length B; history = per-row lists of codes, passed on as they are.  Returns (tokens, raw, draws); `outputs` (from
    select_outputs) is written in place, so that a caller still holds it when the call raises."""
    lg = np.ascontiguousarray(logits, np.float32)
    B, n = lg.shape
    row = lambda v, t: None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, t), (B,)))
    sampler = kernel in (SEL_SAMPLE, SEL_SAMPLE_PRED)
    nl = n_draws if sampler else 1
    keep = [lg, row(temperature, np.float32), row(top_k, np.int32), row(top_p, np.float32), row(mask_idx, np.int32), row(seed, np.uint64),
            row(draw0, np.uint32), row(penalty, np.float32), row(cur_code, np.int32)]
    d = SelectDesc()
    d.kernel, d.B, d.n, d.stride, d.row_off, d.n_draws = kernel, B, n, n if stride is None else stride, row_off, n_draws
    d.logits, d.temperature, d.top_k, d.top_p, d.mask_idx, d.seed, d.draw0, d.penalty, d.cur_code = [_p(a) for a in keep]
    if penalty is not None:
        history = history if history is not None else [[] for _ in range(B)]
        d.hist_cap = max(1, max(len(h) for h in history))
        hist = np.full((B, d.hist_cap), -1, np.int32)
        hlen = np.array([len(h) for h in history], np.int32)
        for b, h in enumerate(history):
            hist[b, : len(h)] = h
        keep += [hist, hlen]
        d.hist, d.hist_len = _p(hist), _p(hlen)
    d.out_stride, d.start, d.end, d.add = out_stride, start, n if end is None else end, add
    tokens, raw, draws = outputs if outputs is not None else select_outputs(B, nl, out_stride)
    assert tokens.shape == (nl, B) and raw.shape == (nl, B * out_stride) and draws.shape == (B,)
    d.tokens, d.out_raw, d.draws_out = _p(tokens), _p(raw), _p(draws)
    lib().q3tts_op_select_rows.argtypes = [C.POINTER(SelectDesc)]
    _chk(lib().q3tts_op_select_rows(C.byref(d)))
    return tokens, raw, draws


# ---- the frame-loop glue kernels (q3tts_op_frame_glue) ----
(GLUE_PROJECT_MT, GLUE_PROJECT_TABLE, GLUE_FEEDBACK_KEYS, GLUE_GATHER_ROWS_KEYS, GLUE_ADVANCE_KEYS, GLUE_STALL_SAVE,
 GLUE_ADVANCE_KEYS_GATED) = range(7)
GLUE_GUARD = 64   # Q3TTS_GLUE_GUARD


class Guarded(C.Structure):  # q3tts_guarded
    _fields_ = [("p", C.c_void_p), ("n", C.c_int64)]


_GLUE_GUARDED = {"out": np.float32, "keys": np.uint64, "next_key0": np.uint64, "finished": np.int32, "n_frames": np.int32, "t_slot": np.int32,
                 "t_pos": np.int32, "hist": np.int32, "hidden": np.float32, "save_hidden": np.float32, "draws": np.uint32, "pdraws": np.uint32,
                 "save_draws": np.uint32}
_GLUE_ARRAYS = {"x": np.float32, "w": np.float32, "b": np.float32, "tts_pad": np.float32, "trail_ids": np.int32, "text_table": np.float32,
                "n_trail": np.int32, "open": np.int32, "max_frames": np.int32}


_GLUE_INTS = ("ntok", "n_in", "n_out", "x_stride", "x_off", "out_stride", "row_len", "key_stride", "trail", "ids_stride", "hist_stride")


class FrameGlueDesc(C.Structure):  # q3tts_frame_glue_desc
    _fields_ = [("kernel", C.c_int32), ("ntok", C.c_int32),
                ("n_in", C.c_int32), ("n_out", C.c_int32), ("x_stride", C.c_int32), ("x_off", C.c_int32), ("out_stride", C.c_int32),
                ("x", C.c_void_p), ("x_floats", C.c_int64), ("w", C.c_void_p), ("b", C.c_void_p),
                ("tables", C.c_void_p), ("table_rows", C.c_void_p), ("row_len", C.c_int32), ("key_stride", C.c_int32), ("tts_pad", C.c_void_p),
                ("trail", C.c_int32), ("trail_ids", C.c_void_p), ("ids_stride", C.c_int32), ("text_table", C.c_void_p), ("text_rows", C.c_int64),
                ("n_trail", C.c_void_p), ("open", C.c_void_p), ("max_frames", C.c_void_p), ("hist_stride", C.c_int32)] + \
               [(k, Guarded) for k in ("out", "keys", "next_key0", "finished", "n_frames", "t_slot", "t_pos", "hist", "hidden", "save_hidden",
                                       "draws", "pdraws", "save_draws")]


def glue_guarded(core, sentinel, dtype=None):
    """a whole q3tts_guarded buffer: GLUE_GUARD sentinels, the core (any shape, flattened), GLUE_GUARD sentinels"""
    core = np.ascontiguousarray(core, dtype).reshape(-1)
    whole = np.full(core.size + 2 * GLUE_GUARD, sentinel, core.dtype)
    whole[GLUE_GUARD: GLUE_GUARD + core.size] = core
    return whole


def glue_core(whole, shape=None):
    """the core of a whole guarded buffer (a view)"""
    c = whole[GLUE_GUARD: whole.size - GLUE_GUARD]
    return c if shape is None else c.reshape(shape)


def op_frame_glue(kernel, tables=None, **fields):
    """one launch of one frame-loop glue kernel (q3tts_op_frame_glue).  Guarded buffers (out, keys, next_key0, finished, n_frames, t_slot, t_pos,
    hist, hidden, save_hidden, draws, pdraws, save_draws) are whole arrays from glue_guarded and are rewritten in place after the launch ran; a
    refused call leaves them as they were.  tables = a list of float32 arrays [rows][row length]; every other field is an int or an array."""
    d = FrameGlueDesc()
    d.kernel = kernel
    keep = []
    for k, v in fields.items():
        if k in _GLUE_GUARDED:
            assert isinstance(v, np.ndarray) and v.dtype == _GLUE_GUARDED[k] and v.ndim == 1 and v.flags["C_CONTIGUOUS"], k
            setattr(d, k, Guarded(v.ctypes.data, v.size))
        elif k in _GLUE_ARRAYS:
            a = np.ascontiguousarray(v, _GLUE_ARRAYS[k])
            keep.append(a)
            setattr(d, k, a.ctypes.data)
            if k == "x":
                d.x_floats = a.size
            if k == "text_table":
                d.text_rows = a.shape[0]
        elif k in _GLUE_INTS:
            setattr(d, k, int(v))
        else:
            raise TypeError("op_frame_glue: q3tts_frame_glue_desc has no field %r for the caller to set" % k)
    if tables is not None:
        tabs = [np.ascontiguousarray(t, np.float32) for t in tables]
        ptrs = (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
        rows = np.array([t.shape[0] for t in tabs], np.int64)
        keep += [tabs, ptrs, rows]
        d.tables, d.table_rows = C.cast(ptrs, C.c_void_p), rows.ctypes.data
    _chk(lib().q3tts_op_frame_glue(C.byref(d)))


# ---- the ggml-mode kernels (q3tts_op_ggml) ----
GG_LOAD_ROWS, GG_ADD, GG_RMSNORM, GG_QUANT, GG_MATVEC, GG_LINEAR, GG_SWIGLU = range(7)
_GG_GUARDED = {"out": np.float32, "q8": np.int8, "d8": np.uint16, "qk": np.int8, "dk": np.float32, "bs": np.int16}
_GG_ARRAYS = {"x": np.float32, "u": np.float32, "idx": np.int32, "idx_keys": np.uint64, "w": np.uint8}
_GG_INTS = ("ntok", "k", "n", "x_stride", "x_rows", "idx_stride", "type", "rows", "row0", "nrows", "out_stride")


class GgmlDesc(C.Structure):  # q3tts_ggml_desc
    _fields_ = [("op", C.c_int32), ("ntok", C.c_int32), ("k", C.c_int32), ("n", C.c_int64),
                ("x", C.c_void_p), ("x_floats", C.c_int64), ("x_stride", C.c_int32), ("x_rows", C.c_int32),
                ("u", C.c_void_p), ("eps", C.c_float),
                ("idx", C.c_void_p), ("idx_keys", C.c_void_p), ("idx_stride", C.c_int32), ("idx_n", C.c_int64),
                ("w", C.c_void_p), ("type", C.c_int32), ("rows", C.c_int32), ("row0", C.c_int32), ("nrows", C.c_int32), ("out_stride", C.c_int32)] + \
               [(k, Guarded) for k in ("out", "q8", "d8", "qk", "dk", "bs")]


def op_ggml(op, **fields):
    """one launcher of csrc/ggml_mode.h on caller buffers (q3tts_op_ggml; GG_LINEAR = gg_quant then gg_matvec).  out, q8, d8, qk, dk, bs are
    whole arrays from glue_guarded and are rewritten in place after the launch ran; a refused call and a no-op leave them as they were."""
    d = GgmlDesc()
    d.op = op
    keep = []
    for k, v in fields.items():
        if k in _GG_GUARDED:
            assert isinstance(v, np.ndarray) and v.dtype == _GG_GUARDED[k] and v.ndim == 1 and v.flags["C_CONTIGUOUS"], k
            setattr(d, k, Guarded(v.ctypes.data, v.size))
        elif k in _GG_ARRAYS:
            a = np.ascontiguousarray(v, _GG_ARRAYS[k]).reshape(-1)
            keep.append(a)
            setattr(d, k, a.ctypes.data if a.size else None)
            if k == "x":
                d.x_floats = a.size
            if k in ("idx", "idx_keys"):
                d.idx_n = a.size
        elif k in _GG_INTS:
            setattr(d, k, int(v))
        elif k == "eps":
            d.eps = float(v)
        else:
            raise TypeError("op_ggml: q3tts_ggml_desc has no field %r for the caller to set" % k)
    lib().q3tts_op_ggml.argtypes = [C.POINTER(GgmlDesc)]
    _chk(lib().q3tts_op_ggml(C.byref(d)))


# ---- output formats: the host-only half and the convert kernel (q3tts_op_pcm_convert) ----
def pcm_out_plan(rate):
    """(L, M, n_taps, taps_per_phase) of one of PCM_RATES"""
    v = [C.c_int32() for _ in range(4)]
    _chk(lib().q3tts_pcm_out_plan(rate, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def pcm_out_filter(rate):
    """the f32 prototype filter the converter uploads for this rate (empty at 24000)"""
    h = np.zeros(pcm_out_plan(rate)[2], np.float32)
    n = lib().q3tts_pcm_out_filter(rate, _p(h), h.size)
    if n != h.size:
        raise Q3Error(lib().q3tts_last_error().decode())
    return h


def pcm_out_samples(rate, n_native):
    return int(lib().q3tts_pcm_out_samples(rate, n_native))


def pcm_format_ok(rate, encoding):
    return lib().q3tts_pcm_format_check(C.byref(PcmFormat(rate, encoding))) == 0


def pcm_dtype(encoding):
    return np.int16 if encoding == PCM_S16 else np.float32


# ---- reference audio intake: the host-only half, the WAV header reader and the intake itself (q3tts_intake, q3tts_wav_intake) ----
def intake_plan(rate):
    """(L, M, n_taps, taps_per_output): 24000 / rate = L / M"""
    v = [C.c_int32() for _ in range(4)]
    _chk(lib().q3tts_intake_plan(rate, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def intake_filter(rate):
    """the f32 prototype filter of this rate (empty at 24000)"""
    h = np.zeros(intake_plan(rate)[2], np.float32)
    n = lib().q3tts_intake_filter(rate, _p(h), h.size)
    if n != h.size:
        raise Q3Error(lib().q3tts_last_error().decode())
    return h


def intake_samples(rate, n_frames):
    """ceil(n_frames L / M); < 0 for a rate the intake does not take"""
    return int(lib().q3tts_intake_samples(rate, n_frames))


def intake_tile(rate):
    """output samples one block of the kernel computes at this rate"""
    t = int(lib().q3tts_intake_tile(rate))
    if t < 0:
        raise Q3Error(lib().q3tts_last_error().decode())
    return t


def _intake_clip(clip):
    """(the C struct, the array that keeps its bytes alive) of (data, sample_rate, channels, sample_format, downmix[, n_frames]); data is
    the clip's raw interleaved samples as an array of any dtype or as bytes"""
    data, rate, ch, fmt, mix = clip[:5]
    raw = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    row = ch * INTAKE_SAMPLE_BYTES[fmt] if 0 <= fmt < 5 and ch > 0 else 0
    n = int(clip[5]) if len(clip) > 5 else (raw.size // row if row else 0)
    if row and n * row > raw.size:
        raise ValueError("clip holds fewer than n_frames frames")
    return IntakeClip(raw.ctypes.data if raw.size else None, n, rate, ch, fmt, mix), raw


def intake_why_not(clip):
    """None if q3tts_intake_check lets the clip run, else its reason"""
    c, _keep = _intake_clip(clip)
    return None if lib().q3tts_intake_check(C.byref(c)) == 0 else lib().q3tts_last_error().decode()


def wav_probe(data):
    """q3tts_wav_probe over the bytes of a WAV file: dict(sample_format, channels, sample_rate, bits, data_offset, n_frames)"""
    raw = np.frombuffer(bytes(data), np.uint8)
    w = WavInfo()
    _chk(lib().q3tts_wav_probe(raw.ctypes.data if raw.size else None, raw.size, C.byref(w)))
    return {k: int(getattr(w, k)) for k, _ in WavInfo._fields_}


def intake(clips, device=0, slack=0, fill=0x5A, caps=None):
    """q3tts_intake: a list of clips (see _intake_clip) -> a list of f32 arrays, mono at 24000 Hz.  slack > 0 over-allocates every output by
    that many floats of `fill` bytes and returns (outs, wholes, n_out) for a test to look behind the samples; a refused call raises Q3Error
    with .wholes and .n_out as the call left them.  caps: the capacities to declare instead of the buffers' own (never more than those)"""
    cs = [_intake_clip(c) for c in clips]
    arr = (IntakeClip * max(len(cs), 1))(*[c for c, _ in cs])
    want = [max(intake_samples(c.sample_rate, c.n_frames), 0) for c, _ in cs]
    wholes = [np.full((n + slack) * 4, fill, np.uint8).view(np.float32) for n in want]
    ptrs = (C.c_void_p * max(len(cs), 1))(*[w.ctypes.data for w in wholes])
    if caps is not None and any(c > w.size for c, w in zip(caps, wholes)):
        raise ValueError("a declared capacity exceeds its buffer")
    caps = np.array([w.size for w in wholes] + [0] if caps is None else list(caps) + [0], np.int64)
    n_out = np.full(len(cs) + 1, -1, np.int64)
    if lib().q3tts_intake(device, arr, len(cs), ptrs, _p(caps), _p(n_out)) != 0:
        ex = Q3Error(lib().q3tts_last_error().decode())
        ex.wholes, ex.n_out = wholes, n_out[: len(cs)]
        raise ex
    outs = [w[:n].copy() for w, n in zip(wholes, n_out[: len(cs)])]
    return (outs, wholes, n_out[: len(cs)]) if slack else outs


def wav_intake(path, downmix=INTAKE_FIRST, device=0):
    """q3tts_wav_intake: (samples, info) of a WAV file at any accepted rate, sample format and channel count"""
    n, w = C.c_int64(), WavInfo()
    _chk(lib().q3tts_wav_intake(path.encode(), downmix, device, None, 0, C.byref(n), C.byref(w)))   # the size query
    out = np.zeros(n.value, np.float32)
    _chk(lib().q3tts_wav_intake(path.encode(), downmix, device, _p(out), out.size, C.byref(n), C.byref(w)))
    return out[: n.value], {k: int(getattr(w, k)) for k, _ in WavInfo._fields_}


# ---- what the four output-stage entry points (op_pcm_convert, op_tsm, op_volume, op_pitch) share in front of their call and behind it ----
def _stage_inputs(x, chunk_samples, streams, reset_before, pad_empty=True):
    """(G, chunk lengths, slots [n_chunks][G], resets or None, the chunks flattened [n_chunks concatenated][G][T_c]); pad_empty: chunks that hold
    nothing still hand the call one float"""
    x = np.ascontiguousarray(x, np.float32)
    G = x.shape[0] if x.ndim == 2 else 0
    cs = np.ascontiguousarray(chunk_samples, np.int32)
    sl = np.ascontiguousarray(streams, np.int32).reshape(cs.size, -1)
    rb = None if reset_before is None else np.ascontiguousarray(reset_before, np.int32).reshape(cs.size, -1)
    parts, at = [], 0
    for t in cs:
        parts.append(x[:, at: at + max(int(t), 0)].reshape(-1))
        at += max(int(t), 0)
    some = parts and G and (not pad_empty or sum(p.size for p in parts))
    return G, cs, sl, rb, np.ascontiguousarray(np.concatenate(parts)) if some else np.zeros(1, np.float32)


def _stage_store(h, n_streams, width):
    """a whole guarded state store: the caller's, or a zero store between guards of -3e38"""
    if h is None:
        h = np.zeros(n_streams * width + 2 * GLUE_GUARD, np.float32)
        h[:GLUE_GUARD] = h[-GLUE_GUARD:] = -3e38
    assert h.dtype == np.float32 and h.size == n_streams * width + 2 * GLUE_GUARD and h.flags["C_CONTIGUOUS"]
    return h


def _stage_bufs(bufs, per=1):
    """(pointer array, lengths in units of `per` elements) of a list of whole buffers; an empty list still hands the call one entry of each"""
    return (C.c_void_p * max(len(bufs), 1))(*[w.ctypes.data for w in bufs]), np.array([w.size // per for w in bufs] or [0], np.int64)


def _pz(a):
    return _p(a if a.size else np.zeros(1, np.int32))   # an empty list still hands the call a pointer


def _stage_call(fn, *args, n_out, **carried):
    """the call; returns a copy of n_out, the counts it reported.  A refused call raises Q3Error carrying n_out and `carried` as they are
    then: the caller can see that nothing was written"""
    try:
        _chk(fn(*args))
    except Q3Error as ex:
        ex.n_out = n_out.copy()
        for k, v in carried.items():
            setattr(ex, k, v)
        raise
    return n_out.copy()


def op_pcm_convert(x, chunk_samples, streams, n_streams, fmts, reset_before=None, hist=None, slack=0, fill=0x5A):
    """the convert kernel over host buffers, one launch of the engine's launcher per chunk.  x [G][sum(chunk_samples)] f32: the native signal of
    each position; streams [n_chunks][G] history slots; fmts [G] (rate, encoding).  hist: a whole guarded store (GLUE_GUARD floats,
    [n_streams][2][96], GLUE_GUARD floats) or None for a zero store between guards of -3e38.  Every output buffer is made exactly as large as
    the result plus `slack` elements, every byte `fill`.  Returns (outs, wholes, n_out, hist): the converted samples per position, the whole
    buffers as they came back, the counts the call reported, the whole store.  A refused call raises Q3Error carrying wholes / n_out / hist as they are then."""
    G, cs, sl, rb, flat = _stage_inputs(x, chunk_samples, streams, reset_before, pad_empty=False)
    fm = (PcmFormat * max(len(fmts), 1))(*[PcmFormat(int(r), int(e)) for r, e in fmts])
    wholes, want = [], []
    for r, e in fmts:
        n = sum(max(pcm_out_samples(r, int(t)), 0) for t in cs)
        want.append(n)
        wholes.append(np.full((n + slack + 2 * GLUE_GUARD) * np.dtype(pcm_dtype(e)).itemsize, fill, np.uint8))
    hist = _stage_store(hist, n_streams, 2 * PCM_HIST)
    (ptrs, nbytes), n_out = _stage_bufs(wholes), np.full(max(len(wholes), 1), -1, np.int64)
    n_out = _stage_call(lib().q3tts_op_pcm_convert, _p(flat), G, _p(cs), cs.size, _p(sl), n_streams, C.cast(fm, C.c_void_p), _p(rb), ptrs, _p(nbytes),
                        _p(n_out), _p(hist), n_out=n_out[: len(wholes)], wholes=wholes, hist=hist)
    outs = [w.view(pcm_dtype(e))[GLUE_GUARD: GLUE_GUARD + n].copy() for w, (r, e), n in zip(wholes, fmts, want)]
    return outs, wholes, n_out, hist


# ---- speaking rate: the host-only half and the stretch kernel (q3tts_op_tsm) ----
def tsm_samples(rate_pct, n_native, final=False):
    """samples delivered for n_native native samples at rate_pct: while streaming, or (final) once flushed; < 0 for a rate out of range"""
    return int(lib().q3tts_tsm_samples(int(rate_pct), int(n_native), 1 if final else 0))


def tsm_windows():
    """the two normative 480-entry f32 tables (w, w2)"""
    w, w2 = np.zeros(TSM_HOP, np.float32), np.zeros(TSM_HOP, np.float32)
    _chk(lib().q3tts_tsm_windows(_p(w), _p(w2)))
    return w, w2


def op_tsm(x, chunk_samples, streams, n_streams, rates, encodings, reset_before=None, flush=False, hist=None, slack=0, fill=0x5A):
    """the stretch kernel over host buffers, one launch of the engine's launcher per chunk and one more for the flush.  x [G][sum(chunk_samples)]
    f32: the native signal of each position; streams [n_chunks][G] state slots; rates [G] percent; encodings [G].  hist: a whole guarded store
    (GLUE_GUARD floats, [n_streams][1920], GLUE_GUARD floats) or None for a zero store between guards of -3e38.  Every output and trace buffer
    is made exactly as large as the result plus `slack` elements, every byte `fill`.  A position whose slot is reset starts a new utterance: its
    counts start over.  Returns (outs, traces, wholes, twholes, n_out, hist).  A refused call raises Q3Error carrying wholes / twholes / n_out /
    hist as they are then."""
    G, cs, sl, rb, flat = _stage_inputs(x, chunk_samples, streams, reset_before)
    rt = np.ascontiguousarray(rates, np.int32)
    en = np.ascontiguousarray(encodings, np.int32)
    wholes, twholes, want, dts = [], [], [], []
    seen, done, ns, frs = {}, {}, [0] * len(rt), [0] * len(rt)   # the plan, as the call works it out: counters per slot, starting over at a reset
    for c in range(cs.size + (1 if flush else 0)):
        T = max(int(cs[c]), 0) if c < cs.size else 0
        for g in range(len(rt)):
            s = int(sl[min(c, cs.size - 1), g]) if sl.size else 0
            if c < cs.size and rb is not None and rb[c, g]:
                seen[s] = done[s] = 0
            if rt[g] == 100:
                ns[g] += T
                continue
            tot = max(tsm_samples(rt[g], seen.get(s, 0) + T, c == cs.size), 0) // TSM_HOP
            nf = max(tot - done.get(s, 0), 0)
            seen[s] = seen.get(s, 0) + T
            done[s] = done.get(s, 0) + nf
            ns[g] += nf * TSM_HOP
            frs[g] += nf
    for g in range(len(rt)):
        dt = np.int16 if (en[g] == PCM_S16 and rt[g] != 100) else np.float32
        want.append((ns[g], frs[g])); dts.append(dt)
        wholes.append(np.full((ns[g] + slack + 2 * GLUE_GUARD) * np.dtype(dt).itemsize, fill, np.uint8))
        twholes.append(np.full(frs[g] + slack + 2 * GLUE_GUARD, 0x5A5A5A5A, np.int32))
    hist = _stage_store(hist, n_streams, TSM_HIST)
    (ptrs, nbytes), (tptrs, tlen), n_out = _stage_bufs(wholes), _stage_bufs(twholes), np.full(max(len(wholes), 1), -1, np.int64)
    n_out = _stage_call(lib().q3tts_op_tsm, _p(flat), G, _p(cs), cs.size, _pz(sl), n_streams, _pz(rt), _pz(en), _p(rb), 1 if flush else 0, ptrs,
                        _p(nbytes), _p(n_out), tptrs, _p(tlen), _p(hist), n_out=n_out[: len(wholes)], wholes=wholes, twholes=twholes, hist=hist)
    outs = [w.view(dt)[GLUE_GUARD: GLUE_GUARD + n].copy() for w, dt, (n, fr) in zip(wholes, dts, want)]
    traces = [t[GLUE_GUARD: GLUE_GUARD + fr].copy() for t, (n, fr) in zip(twholes, want)]
    return outs, traces, wholes, twholes, n_out, hist


# ---- volume: the host-only half and the volume kernel (q3tts_op_volume) ----
def volume_gain(db10):
    """G = (float) pow(10.0, db10 / 200.0) as np.float32; NaN for a volume outside [VOL_MIN, VOL_MAX]"""
    return np.float32(lib().q3tts_volume_gain(int(db10)))


def op_volume(x, chunk_samples, streams, n_streams, volumes, reset_before=None, hist=None, trace=True, slack=0, fill=0x5A):
    """the volume kernel over host buffers, one launch of the engine's launcher per chunk.  x [G][sum(chunk_samples)] f32: the native signal of
    each position; streams [n_chunks][G] state slots; volumes [G] tenths of a dB.  hist: a whole guarded store (GLUE_GUARD floats,
    [n_streams][VOL_HIST], GLUE_GUARD floats) or None for a zero store between guards of -3e38.  Every output and trace buffer is made exactly
    as large as the result plus `slack` elements, every byte `fill`; trace=False passes no traces.  Returns (outs, traces, wholes, twholes,
    n_out, hist).  A refused call raises Q3Error carrying wholes / twholes / n_out / hist as they are then."""
    G, cs, sl, rb, flat = _stage_inputs(x, chunk_samples, streams, reset_before)
    vo = np.ascontiguousarray(volumes, np.int32)
    n = int(sum(max(int(t), 0) for t in cs))
    wholes = [np.full((n + slack + 2 * GLUE_GUARD) * 4, fill, np.uint8) for _ in range(len(vo))]
    twholes = [np.full((n + slack + 2 * GLUE_GUARD) * 4, fill, np.uint8) for _ in range(len(vo))] if trace else []
    hist = _stage_store(hist, n_streams, VOL_HIST)
    (ptrs, nbytes), (tptrs, tlen), n_out = _stage_bufs(wholes), _stage_bufs(twholes, 4), np.full(max(len(wholes), 1), -1, np.int64)
    n_out = _stage_call(lib().q3tts_op_volume, _p(flat), G, _p(cs), cs.size, _pz(sl), n_streams, _pz(vo), _p(rb), ptrs, _p(nbytes), _p(n_out),
                        tptrs if trace else None, _p(tlen), _p(hist), n_out=n_out[: len(wholes)], wholes=wholes, twholes=twholes, hist=hist)
    outs = [w.view(np.float32)[GLUE_GUARD: GLUE_GUARD + n].copy() for w in wholes]
    traces = [t.view(np.float32)[GLUE_GUARD: GLUE_GUARD + n].copy() for t in twholes]
    return outs, traces, wholes, twholes, n_out, hist


# ---- loudness: the host-only half and the loudness kernel (q3tts_op_loudness) ----
def loudness_tables():
    """(coef [10], m [4][4]) float64: the two K-weighting stages at 24000 Hz (b0 b1 b2 a1 a2 each) and A^LOUD_SEG"""
    coef, m = np.zeros(10, np.float64), np.zeros((4, 4), np.float64)
    _chk(lib().q3tts_loudness_tables(_p(coef), _p(m)))
    return coef, m


def loudness_gate(rows):
    """the BS.1770 gate over rows [n][2] = {energy, peak}: dict(integrated_lufs, momentary_max_lufs, peak_dbfs, n_blocks, n_gated)"""
    r = np.ascontiguousarray(rows, np.float64).reshape(-1, 2)
    o = Loudness()
    _chk(lib().q3tts_loudness_gate(_p(r if r.size else np.zeros((1, 2), np.float64)), r.shape[0], C.byref(o)))
    return _loudness_dict(o)


def loudness_gain_db10(measured_lufs, target_lufs):
    """the volume in tenths of a dB that takes measured_lufs to target_lufs, rounded and clamped to [VOL_MIN, VOL_MAX]; 0 for a non-finite input"""
    return int(lib().q3tts_loudness_gain_db10(float(measured_lufs), float(target_lufs)))


def op_loudness(x, chunk_samples, streams, n_streams, metered, reset_before=None, state=None, slack=0, fill=0x5A):
    """the loudness kernel over host buffers, one launch of the engine's launcher per chunk.  x [G][sum(chunk_samples)] f32: the native signal
    of each position; streams [n_chunks][G] state slots; metered [G].  state: a whole guarded store (GLUE_GUARD doubles, [n_streams][LOUD_STATE],
    GLUE_GUARD doubles) or None for a zero store between guards of -3e300.  Every row buffer is made exactly as large as the result plus `slack`
    rows, every byte `fill`.  Returns (rows, wholes, n_rows, state): the rows [n][2] per position, the whole buffers as they came back, the
    counts the call reported, the whole store.  A refused call raises Q3Error carrying wholes / n_out / state as they are then."""
    G, cs, sl, rb, flat = _stage_inputs(x, chunk_samples, streams, reset_before)
    me = np.ascontiguousarray(metered, np.int32)
    pos, want = {}, [0] * len(me)   # the plan, as the call works it out: a position per slot, starting over at a reset
    for c in range(cs.size):
        T = max(int(cs[c]), 0)
        for g in range(len(me)):
            s = int(sl[c, g]) if sl.size else 0
            if rb is not None and rb[c, g]:
                pos[s] = 0
            if me[g]:
                want[g] += (pos.get(s, 0) + T) // LOUD_BLOCK - pos.get(s, 0) // LOUD_BLOCK
            pos[s] = pos.get(s, 0) + T
    wholes = [np.full((n + slack + 2 * GLUE_GUARD) * 16, fill, np.uint8) for n in want]
    if state is None:
        state = np.zeros(n_streams * LOUD_STATE + 2 * GLUE_GUARD, np.float64)
        state[:GLUE_GUARD] = state[-GLUE_GUARD:] = -3e300
    assert state.dtype == np.float64 and state.size == n_streams * LOUD_STATE + 2 * GLUE_GUARD and state.flags["C_CONTIGUOUS"]
    (ptrs, nbytes), n_out = _stage_bufs(wholes), np.full(max(len(wholes), 1), -1, np.int64)
    n_out = _stage_call(lib().q3tts_op_loudness, _p(flat), G, _p(cs), cs.size, _pz(sl), n_streams, _pz(me), _p(rb), ptrs, _p(nbytes), _p(n_out),
                        _p(state), n_out=n_out[: len(wholes)], wholes=wholes, state=state)
    rows = [w.view(np.float64).reshape(-1, 2)[GLUE_GUARD: GLUE_GUARD + n].copy() for w, n in zip(wholes, want)]
    return rows, wholes, n_out, state


# ---- pitch: the host-only half and the pitch kernel (q3tts_op_pitch) ----
def pitch_samples(rate_pct, pitch_pct, n_native, final=False):
    """samples delivered for n_native native samples at the pair (rate_pct, pitch_pct): while streaming, or (final) once flushed; < 0 for a
    value or the pair out of range"""
    return int(lib().q3tts_pitch_samples(int(rate_pct), int(pitch_pct), int(n_native), 1 if final else 0))


def pitch_plan(pitch_pct):
    """dict(L, M, n_taps, taps_per_output) of a pitch's resampler; raises Q3Error for a pitch out of range"""
    v = [C.c_int32() for _ in range(4)]
    _chk(lib().q3tts_pitch_plan(int(pitch_pct), *[C.byref(t) for t in v]))
    return dict(L=v[0].value, M=v[1].value, n_taps=v[2].value, taps_per_output=v[3].value)


def pitch_filter(pitch_pct):
    """the normative f32 prototype h32 of a pitch's resampler"""
    h = np.zeros(pitch_plan(pitch_pct)["n_taps"], np.float32)
    if int(lib().q3tts_pitch_filter(int(pitch_pct), _p(h), h.size)) != h.size:
        raise Q3Error(lib().q3tts_last_error().decode())
    return h


def pitch_frames(rate_pct, pitch_pct, n_native, final=False):
    """stage-1 frames behind pitch_samples (q3tts_spec.h "pitch", available / flush), for sizing a trace; 0 for anything out of range"""
    R, P, N = int(rate_pct), int(pitch_pct), int(n_native)
    if not (TSM_MIN <= R <= TSM_MAX and PITCH_MIN <= P <= PITCH_MAX and 2 * R >= P and R <= 2 * P) or N < 0:
        return 0
    if final:
        return -(-P * N // (TSM_HOP * R))
    return 0 if N < TSM_LOOK else (P * (N - TSM_LOOK + 1) - 1) // (TSM_HOP * R) + 1


def op_pitch(x, chunk_samples, streams, n_streams, rates, pitches, encodings, reset_before=None, flush=False, hist=None, zhist=None, slack=0,
             fill=0x5A):
    """the pitch kernel over host buffers, one launch of the engine's launcher per chunk and one more for the flush: op_tsm plus pitches [G]
    and a second state store.  A position with pitch 100 and a rate goes through the stretcher beside it; one with neither is copied through.
    hist / zhist: whole guarded stores ([n_streams][1920] and [n_streams][64] between GLUE_GUARD floats) or None for zero stores between
    guards of -3e38.  Every output and trace buffer is made exactly as large as the result plus `slack` elements, every byte `fill`.
    Returns (outs, traces, wholes, twholes, n_out, hist, zhist).  A refused call raises Q3Error carrying wholes / twholes / n_out / hist /
    zhist as they are then."""
    G, cs, sl, rb, flat = _stage_inputs(x, chunk_samples, streams, reset_before)
    rt = np.ascontiguousarray(rates, np.int32)
    pt = np.ascontiguousarray(pitches, np.int32)
    en = np.ascontiguousarray(encodings, np.int32)
    wholes, twholes, want, dts = [], [], [], []
    seen, ns, frs = {}, [0] * len(rt), [0] * len(rt)   # the plan, as the call works it out: native samples per slot, starting over at a reset

    def made(g, n, final):   # (stage-1 frames, delivered samples) of position g after n native samples of an utterance
        if pt[g] == 100:
            v = max(tsm_samples(rt[g], n, final), 0)
            return v // TSM_HOP, v
        return pitch_frames(rt[g], pt[g], n, final), max(pitch_samples(rt[g], pt[g], n, final), 0)

    for c in range(cs.size + (1 if flush else 0)):
        T = max(int(cs[c]), 0) if c < cs.size else 0
        for g in range(len(rt)):
            s = int(sl[min(c, cs.size - 1), g]) if sl.size else 0
            if c < cs.size and rb is not None and rb[c, g]:
                seen[s] = 0
            if rt[g] == 100 and pt[g] == 100:
                ns[g] += T
                continue
            (f0, v0), (f1, v1) = made(g, seen.get(s, 0), False), made(g, seen.get(s, 0) + T, c == cs.size)
            seen[s] = seen.get(s, 0) + T
            ns[g] += max(v1 - v0, 0)
            frs[g] += max(f1 - f0, 0)
    for g in range(len(rt)):
        dt = np.int16 if (en[g] == PCM_S16 and (rt[g] != 100 or pt[g] != 100)) else np.float32
        want.append((ns[g], frs[g])); dts.append(dt)
        wholes.append(np.full((ns[g] + slack + 2 * GLUE_GUARD) * np.dtype(dt).itemsize, fill, np.uint8))
        twholes.append(np.full(frs[g] + slack + 2 * GLUE_GUARD, 0x5A5A5A5A, np.int32))
    hist, zhist = _stage_store(hist, n_streams, TSM_HIST), _stage_store(zhist, n_streams, PITCH_HIST)
    (ptrs, nbytes), (tptrs, tlen), n_out = _stage_bufs(wholes), _stage_bufs(twholes), np.full(max(len(wholes), 1), -1, np.int64)
    n_out = _stage_call(lib().q3tts_op_pitch, _p(flat), G, _p(cs), cs.size, _pz(sl), n_streams, _pz(rt), _pz(pt), _pz(en), _p(rb), 1 if flush else 0,
                        ptrs, _p(nbytes), _p(n_out), tptrs, _p(tlen), _p(hist), _p(zhist), n_out=n_out[: len(wholes)], wholes=wholes, twholes=twholes,
                        hist=hist, zhist=zhist)
    outs = [w.view(dt)[GLUE_GUARD: GLUE_GUARD + n].copy() for w, dt, (n, fr) in zip(wholes, dts, want)]
    traces = [t[GLUE_GUARD: GLUE_GUARD + fr].copy() for t, (n, fr) in zip(twholes, want)]
    return outs, traces, wholes, twholes, n_out, hist, zhist
