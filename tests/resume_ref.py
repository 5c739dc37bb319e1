"""Python restatement of the [EXT] resume definition (include/q3tts_spec.h "resume"): the feedback row of a frame in numpy f32, and
resume(R, c[0..k)) composed from the helpers of gen_loop_ref / text_stream_ref -- the prompt and the k feedback rows are teacher-forced
through the talker, the history, both RNG streams and the frame counter start where frame k finds them, and the loop of
text_stream_ref.generate goes on from there.  TEST INFRASTRUCTURE ONLY; neither imported module is changed."""
import numpy as np

import q3oracle
from gen_loop_ref import CODEBOOK, CODEC_EOS, PRED_SEED_XOR, SAMPLE_END, TEXT_EOS, _dims, _model, penalise

SYNTH_TEXT_ROWS = 4096   # text table rows of the synthetic models (q3tts_spec.h "streaming-text talker input")


def fallback_row(tok):
    """HostAssets::text_embedding for an id outside the table: fmod((float)((u64)id * 17 + i), 2) - 1, i = 0..2047"""
    v = ((int(tok) % (1 << 64)) * 17 + np.arange(2048, dtype=np.uint64).astype(object)) % (1 << 64)
    x = np.array([float(np.float32(int(t))) for t in v], np.float64)      # (float): round to nearest even
    return (np.fmod(x, 2.0) - 1.0).astype(np.float32)


def text_row(assets, tok, text_rows=SYNTH_TEXT_ROWS):
    return assets.text_embedding(int(tok)) if 0 <= int(tok) < text_rows else fallback_row(tok)


def feedback_row(assets, tts_pad, codes16, trail_id=None, text_rows=SYNTH_TEXT_ROWS):
    """sum_q E_q[code_q], q = 0..15 in order, then + text(trail_id) or + tts_pad: np.float32 adds, left to right from 0.
    A negative code reads row 0 and a code past its table the zero row (Assets.codec_embedding does both, as k_feedback_keys)"""
    acc = np.zeros(2048, np.float32)
    for q in range(16):
        acc = (acc + np.asarray(assets.codec_embedding(q, int(codes16[q])), np.float32)).astype(np.float32)
    last = np.asarray(tts_pad, np.float32) if trail_id is None else text_row(assets, trail_id, text_rows)
    return (acc + last).astype(np.float32)


def feedback_rows(assets, tts_pad, codes, trail=(), text_rows=SYNTH_TEXT_ROWS):
    codes = np.asarray(codes, np.int32).reshape(-1, 16)
    return np.stack([feedback_row(assets, tts_pad, codes[f], trail[f] if f < len(trail) else None, text_rows) for f in range(codes.shape[0])])


def resume(oe, tts_pad, prompt, max_steps, prefix, trail=(), temperature=0.0, top_k=40, top_p=0.9, seed=42, mask_eos=True,
           repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0, text_rows=SYNTH_TEXT_ROWS):
    """codes [n][16] of resume(R, prefix) on the oracle engine `oe`: rows 0..k-1 are the prefix, the rest is generated"""
    T, P, A = _model(oe.s.talker), _model(oe.s.predictor), oe.assets
    dT, t_vocab = _dims(oe.s.talker)
    dP, _ = _dims(oe.s.predictor)
    t_end = min(t_vocab, SAMPLE_END)
    trail = [int(t) for t in trail]
    prefix = np.asarray(prefix, np.int32).reshape(-1, 16)
    k = prefix.shape[0]
    assert 0 <= k < max_steps or k == 0
    prompt = np.ascontiguousarray(prompt, np.float32)
    rows = prompt if k == 0 else np.concatenate([prompt, feedback_rows(A, tts_pad, prefix, trail[:k], text_rows)])
    T.clear()
    for t in range(rows.shape[0]):                                      # prefill over n_prompt + k rows, positions (t, t, t, 0)
        last = t == rows.shape[0] - 1
        hid, lg = T.eval(rows[t], [t, t, t, 0], dT, 0, t_end if last else 0)
    ts = ps = None
    dummy = np.zeros(8, np.float32)
    if temperature > 0:                                                 # frame k's code_0 is talker draw k (a sampled pick takes one draw)
        for _ in range(k):
            _, ts = q3oracle.sample(dummy, 0, 8, temperature, top_k, top_p, seed, state=ts)
    if predictor_temperature > 0:                                       # the predictor stream stands at draw 15 k
        for _ in range(15 * k):
            _, ps = q3oracle.sample(dummy, 0, 8, predictor_temperature, predictor_top_k, predictor_top_p,
                                    (seed ^ PRED_SEED_XOR) & (2 ** 64 - 1), state=ps)
    hist = set(int(c) for c in prefix[:, 0])                            # distinct code_0 of frames 0..k-1
    codes, cur_pos = [list(map(int, r)) for r in prefix], rows.shape[0]
    for f in range(k, max_steps):
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
        _, pl = P.eval(A.project(A.codec_embedding(0, code0))[:dP], [1, 1, 1, 1], dP, 0, CODEBOOK)
        for q in range(1, 16):
            if predictor_temperature > 0:
                mi, ps = q3oracle.sample(pl, 0, CODEBOOK, predictor_temperature, predictor_top_k, predictor_top_p,
                                         (seed ^ PRED_SEED_XOR) & (2 ** 64 - 1), state=ps)
            else:
                mi = int(np.argmax(pl))
            fc.append(mi)
            if q < 15:
                _, pl = P.eval(A.project(A.codec_embedding(q, mi))[:dP], [q + 1] * 4, dP, q * CODEBOOK, (q + 1) * CODEBOOK)
        codes.append(fc)
        hist.add(code0)
        fb = feedback_row(A, tts_pad, fc, trail[f] if f < len(trail) else None, text_rows)
        hid, lg = T.eval(fb, [cur_pos, cur_pos, cur_pos, 0], dT, 0, t_end)
        cur_pos += 1
    return np.array(codes, np.int32).reshape(-1, 16)
