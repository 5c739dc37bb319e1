"""Reference for [EXT] scoring given frames (include/q3tts_spec.h "scoring"): tests/logprob_ref.py::generate restated with FORCED codes on the
oracle engine.  Nothing is sampled: frame f's talker logits are those of prefill row n_prompt - 1 + f (the last prompt row, then the feedback
rows of the given frames, with text(trail[f]) as the last addend while f < len(trail), as tests/text_stream_ref.py has it), the predictor
runs its 16 positions on the given codes, every head's raw f32 logits are kept and the log-softmax is numpy float64.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import gen_loop_ref as G
from logprob_ref import COLS, NONE, log_softmax64


def score(oe, tts_pad, prompt, codes, trail=()):
    """float64 [n][17]: the rows a recording request shows that emitted exactly codes [n][16] behind prompt"""
    T, P, A = G._model(oe.s.talker), G._model(oe.s.predictor), oe.assets
    dT, t_vocab = G._dims(oe.s.talker)
    dP, _ = G._dims(oe.s.predictor)
    t_end = min(t_vocab, G.SAMPLE_END)
    assert t_end == G.SAMPLE_END
    prompt = np.ascontiguousarray(prompt, np.float32)
    codes = np.asarray(codes, np.int32).reshape(-1, 16)
    trail = [int(t) for t in trail]
    T.clear()
    for t in range(prompt.shape[0]):
        last = t == prompt.shape[0] - 1
        hid, lg = T.eval(prompt[t], [t, t, t, 0], dT, 0, t_end if last else 0)
    rows, cur_pos = [], prompt.shape[0]
    for f in range(codes.shape[0]):
        raw = np.array(lg, np.float32, copy=True)
        fc = [int(c) for c in codes[f]]
        row = np.full(COLS, NONE, np.float64)
        row[0], row[16] = log_softmax64(raw, fc[0]), log_softmax64(raw, G.CODEC_EOS)
        P.clear()
        P.eval(A.project(hid)[:dP], [0, 0, 0, 0], dP)
        emb = [A.codec_embedding(0, fc[0])]
        _, pl = P.eval(A.project(emb[0])[:dP], [1, 1, 1, 1], dP, 0, G.CODEBOOK)
        for q in range(1, 16):
            row[q] = log_softmax64(pl, fc[q])
            emb.append(A.codec_embedding(q, fc[q]))
            if q < 15:
                _, pl = P.eval(A.project(emb[q])[:dP], [q + 1] * 4, dP, q * G.CODEBOOK, (q + 1) * G.CODEBOOK)
        rows.append(row)
        if f + 1 == codes.shape[0]:
            break                                                       # the last frame's feedback row would only serve a frame n
        fb = np.zeros(2048, np.float32)
        for q in range(16):
            fb = fb + emb[q]
        fb = fb + (A.text_embedding(trail[f]) if f < len(trail) else tts_pad)
        hid, lg = T.eval(fb, [cur_pos, cur_pos, cur_pos, 0], dT, 0, t_end)
        cur_pos += 1
    return np.array(rows, np.float64).reshape(-1, COLS)
