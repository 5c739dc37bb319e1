"""The case table of the engine step-width sweep (tests/test_gpu_engine_widths.py) and the rules it rests on, restated without the
library: which step widths a max_batch = B engine can run (Engine::run_group's pick_width, csrc/engine.cpp), frame counts per slot that
make one run replay every one of them, and the requests themselves.  tests/test_engine_widths_cpu.py checks the restatements and which
kernel forms the table reaches.  No GPU needed to import this."""
import numpy as np

GROUP = 4          # frames per scheduler step (run_group: min(4, remaining))
MAX_FRAMES = 36    # the engines' max_steps: 4 * (1 + log2(256))
NARROW = 8         # max_batch of the reference engine: the fused 5-launch layer path


def _ceil_pow2(n):
    w = 1
    while w < n:
        w <<= 1
    return w


def pick_width(hi, B):
    """csrc/engine.cpp pick_width: the next power of two at or above the highest live slot + 1, capped at max_batch"""
    return min(_ceil_pow2(hi), B)


def graph_widths(B):
    """every step width a max_batch = B engine can run: the powers of two below B, and B itself"""
    return {pick_width(hi, B) for hi in range(1, B + 1)}


def lengths(B):
    """frames per slot: slot b runs 4 * (1 + floor(log2(B_ceil / (b + 1)))), at most MAX_FRAMES.  Slot 0 is longest, the upper half retires
    after one group, the live set then halves with every group: one run steps B, B_ceil / 2, B_ceil / 4, ..., 1 slots wide"""
    bc = _ceil_pow2(B)
    return [min(MAX_FRAMES, GROUP * (1 + ((bc // (b + 1)).bit_length() - 1))) for b in range(B)]


def holes(B):
    """slots 0 and B - 1 run three groups, every slot between one: after the first group the graph stays B wide with B - 2 dead slots"""
    return [3 * GROUP if b in (0, B - 1) else GROUP for b in range(B)]


PATTERNS = {"lengths": lengths, "holes": holes}


def simulate(frames):
    """the step widths of a run whose slot b makes frames[b] frames, all slots admitted in one wave: [width of group 0, of group 1, ...]"""
    B, out, done = len(frames), [], 0
    while True:
        live = [b for b in range(B) if frames[b] > done]
        if not live:
            return out
        out.append(pick_width(live[-1] + 1, B))
        done += GROUP


# (quant, B, pattern, codec, flavour).  B sits on every dispatch boundary itself: a width that is no power of two runs only as max_batch
_Q8 = [9, 15, 16, 17, 33, 64, 65, 96, 97, 128, 129, 193, 256]
_Q5 = [15, 16, 17, 33, 129, 256]
_BF = [8, 95, 96, 129, 256]
CASES = ([("q8_0", B, "lengths", B in (33, 256), "plain") for B in _Q8] +
         [("q5_k_m", B, "lengths", False, "plain") for B in _Q5] +
         [("bf16", B, "lengths", B == 96, "plain") for B in _BF] +
         [("q8_0", 129, "holes", False, "plain"), ("q8_0", 256, "holes", False, "plain"), ("q5_k_m", 129, "holes", False, "plain")] +
         [("q8_0", 129, "lengths", False, "all_variants"), ("q8_0", 256, "lengths", False, "all_variants"),
          ("q5_k_m", 129, "lengths", False, "all_variants")])
CHILD_CASES = [("q8_0", 256), ("q5_k_m", 256)]   # plain, lengths, no codec, under Q3_MFMA_WGS=16 in a process of their own


def case_id(c):
    return "%s-%d-%s-%s%s" % (c[0], c[1], c[2], c[4], "-pcm" if c[3] else "")


def text_ids(i):
    """the 3 + (7 i) % 23 random text ids of request i"""
    return np.random.default_rng(1000 + i).integers(0, 4000, 3 + (7 * i) % 23).astype(np.int32)


def prompt(assets, i, spk_emb):
    """request i's prompt rows [n][2048]: build_core of its text ids, every ninth a clone prompt; the same for every B and quantisation"""
    ids = text_ids(i)
    if i % 9 == 8:
        rng = np.random.default_rng(5000 + i)
        return assets.build_clone(ids, rng.integers(0, 2048, (2 + i % 3) * 16), rng.integers(0, 4000, 2 + i % 4).astype(np.int32), spk_emb, max_rows=256)
    return assets.build_core(ids, lang_id=2055, spk_emb=spk_emb, max_rows=256)


def options(i, flavour):
    """the submit() keywords of request i (prompt and max_steps apart).
    plain: greedy, every fifth slot (2, 7, 12, ...) sampled with its own seed -- slots 0 and 1 stay greedy, so the narrowest steps run the
    talker head's argmax epilogue and every wider one the device sampler.
    all_variants: on top of that, repetition penalty 1.1 and a sampled predictor on every third slot (0, 3, ...: at every width), trailing
    text ids on every fourth; the engine records log-probabilities (set_logprobs, the caller's job)"""
    o = dict(temperature=0.9 if i % 5 == 2 else 0.0, top_k=20, top_p=0.9, seed=7 + i, mask_eos=True)
    if flavour == "all_variants":
        if i % 3 == 0:
            o.update(repetition_penalty=1.1, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
        if i % 4 == 0:
            o["trailing_ids"] = np.random.default_rng(9000 + i).integers(0, 4000, 2 + i % 7).astype(np.int32)
    elif flavour != "plain":
        raise ValueError(flavour)
    return o


def oracle_slots(B):
    return sorted({0, B // 2, B - 1})


def pcm_oracle_streams(B):
    """streams held to the oracle codec: both sides of the 16-stream group edge, the ends and two in the middle"""
    return sorted({0, 15, 16, B // 3, B // 2, B - 1} & set(range(B)))
