"""Python restatement of oracle/q3o_engine.c::q3o_engine_generate (the loop at :305-381) with the [EXT] generation controls of
include/q3tts_spec.h: the talker repetition penalty (numpy f32) and the sampled code predictor (a second q3oracle.sample state seeded with
seed ^ Q3_PRED_SEED_XOR).  TEST INFRASTRUCTURE ONLY: built from q3oracle.Model.eval, Assets.project / codec_embedding and q3oracle.sample;
the reference PCM comes from the oracle engine replaying the codes teacher-forced, so the oracle's own chunker and codec produce it."""
import ctypes as C

import numpy as np

import q3oracle

CODEC_EOS, TEXT_EOS, SAMPLE_END, CODEBOOK = 2150, 151673, 2160, 2048
PRED_SEED_XOR = 0x9E3779B97F4A7C15


def penalise(logits, history, p):
    """transformers' RepetitionPenaltyLogitsProcessor on f32: every distinct history token once, l < 0 ? l * p : l / p"""
    out = np.array(logits, np.float32, copy=True)
    if history:
        idx = np.array(sorted(set(int(h) for h in history)), np.int64)
        v = out[idx]
        out[idx] = np.where(v < 0, v * np.float32(p), v / np.float32(p)).astype(np.float32)
    return out


def _model(handle):
    m = q3oracle.Model.__new__(q3oracle.Model)
    m.h = handle
    return m


def _dims(handle):  # q3o_model: q3o_gguf* g; char arch[64]; int n_embd, n_layer, n_head, n_head_kv, head_dim, n_ff, n_vocab
    return C.c_int.from_address(handle + 72).value, C.c_int.from_address(handle + 96).value


def generate(oe, tts_pad, prompt, max_steps, temperature=0.0, top_k=40, top_p=0.9, seed=42, mask_eos=True, repetition_penalty=1.0,
             predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0):
    """codes [n][16] of one request on the oracle engine `oe` (q3oracle.Engine); tts_pad = the assets' tts_pad row"""
    T, P, A = _model(oe.s.talker), _model(oe.s.predictor), oe.assets
    dT, t_vocab = _dims(oe.s.talker)
    dP, _ = _dims(oe.s.predictor)
    t_end = min(t_vocab, SAMPLE_END)
    prompt = np.ascontiguousarray(prompt, np.float32)
    T.clear()
    for t in range(prompt.shape[0]):                                    # prefill, positions (t, t, t, 0)
        last = t == prompt.shape[0] - 1
        hid, lg = T.eval(prompt[t], [t, t, t, 0], dT, 0, t_end if last else 0)
    ts = ps = None
    hist, codes, cur_pos = set(), [], prompt.shape[0]
    for _ in range(max_steps):
        lg = np.array(lg, np.float32, copy=True)
        if mask_eos:
            lg[CODEC_EOS] = -np.inf
        if repetition_penalty != 1.0:
            lg = penalise(lg, hist, repetition_penalty)
        code0, ts = q3oracle.sample(lg, 0, SAMPLE_END, temperature, top_k, top_p, seed, state=ts)
        if code0 in (CODEC_EOS, TEXT_EOS):
            break
        fc = [code0]
        P.clear()
        P.eval(A.project(hid)[:dP], [0, 0, 0, 0], dP)
        emb = [A.codec_embedding(0, code0)]
        _, pl = P.eval(A.project(emb[0])[:dP], [1, 1, 1, 1], dP, 0, CODEBOOK)
        for q in range(1, 16):
            if predictor_temperature > 0:
                mi, ps = q3oracle.sample(pl, 0, CODEBOOK, predictor_temperature, predictor_top_k, predictor_top_p,
                                         (seed ^ PRED_SEED_XOR) & (2 ** 64 - 1), state=ps)
            else:
                mi = int(np.argmax(pl))                                 # first max (strict >)
            fc.append(mi)
            emb.append(A.codec_embedding(q, mi))
            if q < 15:
                _, pl = P.eval(A.project(emb[q])[:dP], [q + 1] * 4, dP, q * CODEBOOK, (q + 1) * CODEBOOK)
        codes.append(fc)
        hist.add(code0)
        fb = np.zeros(2048, np.float32)                                 # feedback: codebook rows in q order, then tts_pad
        for q in range(16):
            fb = fb + emb[q]
        fb = fb + tts_pad
        hid, lg = T.eval(fb, [cur_pos, cur_pos, cur_pos, 0], dT, 0, t_end)
        cur_pos += 1
    return np.array(codes, np.int32).reshape(-1, 16)


def replay_pcm(oe, prompt, codes):
    """PCM of `codes` through the oracle engine's own loop, chunker and codec (teacher-forced replay)"""
    codes = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
    if codes.shape[0] == 0:
        return np.zeros(0, np.float32)
    oe.s.forced, oe.s.forced_frames = codes.ctypes.data, codes.shape[0]
    try:
        got, pcm = oe.generate(prompt, max_steps=codes.shape[0], temperature=0.0, mask_eos=True, want_pcm=True)
    finally:
        oe.s.forced, oe.s.forced_frames = None, 0
    assert np.array_equal(got, codes)
    return pcm
