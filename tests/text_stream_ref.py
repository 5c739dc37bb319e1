"""Python restatement of the [EXT] streaming-text talker input (include/q3tts_spec.h "streaming-text talker input"): the loop of
gen_loop_ref.generate with the feedback's last addend taken from the trailing text ids -- text(trail[f]) at frame f while f < n_trail,
tts_pad after.  TEST INFRASTRUCTURE ONLY: built from gen_loop_ref's helpers and q3oracle (Model.eval, Assets.project / codec_embedding /
text_embedding, sample); gen_loop_ref itself is not changed."""
import numpy as np

import q3oracle
from gen_loop_ref import CODEBOOK, CODEC_EOS, PRED_SEED_XOR, SAMPLE_END, TEXT_EOS, _dims, _model, penalise


def generate(oe, tts_pad, prompt, max_steps, trail=(), temperature=0.0, top_k=40, top_p=0.9, seed=42, mask_eos=True,
             repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0):
    """codes [n][16] of one request with trailing text ids `trail` on the oracle engine `oe`; trail = () is gen_loop_ref.generate"""
    T, P, A = _model(oe.s.talker), _model(oe.s.predictor), oe.assets
    dT, t_vocab = _dims(oe.s.talker)
    dP, _ = _dims(oe.s.predictor)
    t_end = min(t_vocab, SAMPLE_END)
    trail = [int(t) for t in trail]
    prompt = np.ascontiguousarray(prompt, np.float32)
    T.clear()
    for t in range(prompt.shape[0]):                                    # prefill, positions (t, t, t, 0)
        last = t == prompt.shape[0] - 1
        hid, lg = T.eval(prompt[t], [t, t, t, 0], dT, 0, t_end if last else 0)
    ts = ps = None
    hist, codes, cur_pos = set(), [], prompt.shape[0]
    for f in range(max_steps):
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
        fb = np.zeros(2048, np.float32)                                 # feedback: codebook rows in q order, then the text row of frame f
        for q in range(16):
            fb = fb + emb[q]
        fb = fb + (A.text_embedding(trail[f]) if f < len(trail) else tts_pad)
        hid, lg = T.eval(fb, [cur_pos, cur_pos, cur_pos, 0], dT, 0, t_end)
        cur_pos += 1
    return np.array(codes, np.int32).reshape(-1, 16)
