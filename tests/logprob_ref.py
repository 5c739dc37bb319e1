"""Reference for the [EXT] token log-probabilities (include/q3tts_spec.h): the loop of tests/gen_loop_ref.py::generate on the oracle engine,
restated so that every head's raw f32 logits are kept, and the log-softmax of those logits in numpy float64.  TEST INFRASTRUCTURE ONLY.

Row f of the result: column 0 = log softmax(L_T)[code_0] and column 16 = log softmax(L_T)[CODEC_EOS] over the talker logits [0, 2160) that
produced frame f's code_0 (raw: before the EOS mask, the repetition penalty and the sampler), columns 1..15 = log softmax(L_q)[code_q] over
the 2048 predictor logits of step q."""
import numpy as np

import gen_loop_ref as G
import q3oracle

COLS, NONE = 17, 1.0
TOL = 1e-5   # |lp - lp64| <= TOL * max(1, |lp64|), the issue's bound (q3tts_spec.h derives it)


def log_softmax64(x, idx):
    """float64 log softmax(x)[idx] of f32 logits; -inf entries allowed (an -inf at idx gives -inf)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    if x[idx] == -np.inf:
        return -np.inf
    m = np.max(x)
    return float((x[idx] - m) - np.log(np.sum(np.exp(x - m))))


def generate(oe, tts_pad, prompt, max_steps, temperature=0.0, top_k=40, top_p=0.9, seed=42, mask_eos=True, repetition_penalty=1.0,
             predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0):
    """(codes [n][16] int32, logprobs [n][17] float64) of one request on the oracle engine `oe`"""
    T, P, A = G._model(oe.s.talker), G._model(oe.s.predictor), oe.assets
    dT, t_vocab = G._dims(oe.s.talker)
    dP, _ = G._dims(oe.s.predictor)
    t_end = min(t_vocab, G.SAMPLE_END)
    assert t_end == G.SAMPLE_END
    prompt = np.ascontiguousarray(prompt, np.float32)
    T.clear()
    for t in range(prompt.shape[0]):
        last = t == prompt.shape[0] - 1
        hid, lg = T.eval(prompt[t], [t, t, t, 0], dT, 0, t_end if last else 0)
    ts = ps = None
    hist, codes, lps, cur_pos = set(), [], [], prompt.shape[0]
    for _ in range(max_steps):
        raw = np.array(lg, np.float32, copy=True)                       # what the log-probabilities are taken from
        lg = raw.copy()
        if mask_eos:
            lg[G.CODEC_EOS] = -np.inf
        if repetition_penalty != 1.0:
            lg = G.penalise(lg, hist, repetition_penalty)
        code0, ts = q3oracle.sample(lg, 0, G.SAMPLE_END, temperature, top_k, top_p, seed, state=ts)
        if code0 in (G.CODEC_EOS, G.TEXT_EOS):
            break
        row = np.full(COLS, NONE, np.float64)
        row[0], row[16] = log_softmax64(raw, code0), log_softmax64(raw, G.CODEC_EOS)
        fc = [code0]
        P.clear()
        P.eval(A.project(hid)[:dP], [0, 0, 0, 0], dP)
        emb = [A.codec_embedding(0, code0)]
        _, pl = P.eval(A.project(emb[0])[:dP], [1, 1, 1, 1], dP, 0, G.CODEBOOK)
        for q in range(1, 16):
            if predictor_temperature > 0:
                mi, ps = q3oracle.sample(pl, 0, G.CODEBOOK, predictor_temperature, predictor_top_k, predictor_top_p,
                                         (seed ^ G.PRED_SEED_XOR) & (2 ** 64 - 1), state=ps)
            else:
                mi = int(np.argmax(pl))
            row[q] = log_softmax64(pl, mi)
            fc.append(mi)
            emb.append(A.codec_embedding(q, mi))
            if q < 15:
                _, pl = P.eval(A.project(emb[q])[:dP], [q + 1] * 4, dP, q * G.CODEBOOK, (q + 1) * G.CODEBOOK)
        codes.append(fc)
        lps.append(row)
        hist.add(code0)
        fb = np.zeros(2048, np.float32)
        for q in range(16):
            fb = fb + emb[q]
        fb = fb + tts_pad
        hid, lg = T.eval(fb, [cur_pos, cur_pos, cur_pos, 0], dT, 0, t_end)
        cur_pos += 1
    return np.array(codes, np.int32).reshape(-1, 16), np.array(lps, np.float64).reshape(-1, COLS)


def close(got, want, tol=TOL):
    """elementwise |got - want| <= tol * max(1, |want|), -inf matching -inf; returns (ok, worst ratio to the bound)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    inf = np.isneginf(want)
    if not np.array_equal(inf, np.isneginf(got)):
        return False, np.inf
    fin = ~inf
    if not fin.any():
        return True, 0.0
    ratio = np.abs(got[fin] - want[fin]) / (tol * np.maximum(1.0, np.abs(want[fin])))
    worst = float(np.max(ratio))
    return bool(np.isfinite(worst) and worst <= 1.0), worst
