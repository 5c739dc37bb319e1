"""The yardstick of tests/test_gpu_frame_glue.py checked without a GPU: tests/frame_glue_ref.py against independent things the project
already has (the C oracle's project / codec_embedding / text_embedding on the tiny model's assets, tests/resume_ref.py, q3tts_argmax_key),
the slot state machine against hand-written before / after states, the case builders against the situations they claim to hold, and the
declaration of q3tts_op_frame_glue.  Every projection case the GPU test runs must tell mul-then-add from fma here."""
import os
import re

import numpy as np
import pytest

import frame_glue_cases as K
import frame_glue_ref as R
import resume_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tiny_assets(oracle, tiny_model):
    import ggml_ref as G
    path = os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf")
    _, t = G.read_gguf(path)
    ten = lambda n: np.array(t[n][2]).view(np.float32).reshape(-1, 2048)
    oa = oracle.Assets(path)
    yield oa, ten, np.array(t["proj.bias"][2]).view(np.float32)
    oa.close()


def test_entry_point_is_declared_exported_and_listed(q3):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "q3tts.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+q3tts_op_frame_glue\s*\(\s*q3tts_frame_glue_desc\s*\*\s*\w+\s*\)\s*;", txt)
    assert "q3tts_op_frame_glue" in q3.SYMBOLS and hasattr(q3.lib(), "q3tts_op_frame_glue") and q3.lib().q3tts_op_frame_glue.argtypes
    kinds = re.search(r"enum\s*\{\s*(Q3TTS_GLUE_PROJECT_MT[^}]*)\}", txt).group(1)
    names = [k.split("=")[0].strip() for k in kinds.split(",")]
    assert names == ["Q3TTS_GLUE_" + n for n in ("PROJECT_MT", "PROJECT_TABLE", "FEEDBACK_KEYS", "GATHER_ROWS_KEYS", "ADVANCE_KEYS", "STALL_SAVE",
                                                  "ADVANCE_KEYS_GATED")]
    assert [int(k.split("=")[1]) for k in kinds.split(",")] == [q3.GLUE_PROJECT_MT, q3.GLUE_PROJECT_TABLE, q3.GLUE_FEEDBACK_KEYS,
                                                                q3.GLUE_GATHER_ROWS_KEYS, q3.GLUE_ADVANCE_KEYS, q3.GLUE_STALL_SAVE,
                                                                q3.GLUE_ADVANCE_KEYS_GATED]
    assert int(re.search(r"#define\s+Q3TTS_GLUE_GUARD\s+(\d+)", txt).group(1)) == q3.GLUE_GUARD
    # the Python mirror of the descriptor has the header's fields in the header's order
    body = re.search(r"typedef\s+struct\s+q3tts_frame_glue_desc\s*\{(.*?)\}\s*q3tts_frame_glue_desc\s*;", txt, flags=re.S).group(1)
    fields = [re.sub(r"[\s\*]", "", n) for decl in body.split(";") if decl.strip()
              for n in re.sub(r"^\s*(const\s+)?\w+(\s+const)?[\s\*]*(const\s*\*)?", "", decl.strip(), count=1).split(",")]
    assert fields == [f for f, _ in q3.FrameGlueDesc._fields_]
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    assert re.search(r"#define\s+Q3_CODEC_EOS\s+%d\b" % R.CODEC_EOS, spec) and re.search(r"#define\s+Q3_TEXT_EOS\s+%d\b" % R.TEXT_EOS, spec)


def test_fails_cleanly_without_a_descriptor(q3):
    L = q3.lib()
    assert L.q3tts_op_frame_glue(None) < 0 and L.q3tts_last_error()


def test_wrapper_rejects_a_field_the_descriptor_does_not_have(q3):
    out = q3.glue_guarded(np.full(16, K.F32), K.F32)
    for kw in (dict(xstride=512), dict(x_floats=4), dict(text_rows=1), dict(nonsense=np.zeros(3))):
        with pytest.raises(TypeError, match="no field"):
            q3.op_frame_glue(q3.GLUE_PROJECT_MT, ntok=1, n_in=512, n_out=16, out=out, **kw)
    names = [f for f, _ in q3.FrameGlueDesc._fields_]
    settable = set(q3._GLUE_INTS) | set(q3._GLUE_ARRAYS) | set(q3._GLUE_GUARDED)
    assert settable <= set(names) and set(names) - settable == {"kernel", "x_floats", "tables", "table_rows", "text_rows"}   # set by the wrapper


def test_fails_cleanly_without_a_device(q3):
    if q3.device_count() > 0:
        return   # with a device present the no-device path cannot be observed (the suite's convention, as test_compute_fails_loudly_without_gpu)
    out = q3.glue_guarded(np.full(16, K.F32), K.F32)
    with pytest.raises(q3.Q3Error, match="no HIP device"):
        q3.op_frame_glue(q3.GLUE_PROJECT_MT, ntok=1, n_in=512, n_out=16, x_stride=512, out_stride=16, x=np.zeros(512), w=np.zeros((16, 512)),
                         b=np.zeros(16), out=out)
    assert np.all(out == K.F32)


def test_guarded_buffers_round_trip(q3):
    core = np.arange(10, dtype=np.int32).reshape(2, 5)
    whole = q3.glue_guarded(core, K.I32)
    assert whole.size == 10 + 2 * q3.GLUE_GUARD and np.all(whole[: q3.GLUE_GUARD] == K.I32) and np.all(whole[-q3.GLUE_GUARD:] == K.I32)
    assert np.array_equal(q3.glue_core(whole, (2, 5)), core)
    q3.glue_core(whole)[0] = 77          # a view: what the device wrote is what the caller reads
    assert whole[q3.GLUE_GUARD] == 77


# ------------------------------------------------------------ keys ------------------------------------------------------------
def test_key_layout_against_the_library(q3):
    vals = [0.0, -0.0, 1.5, -3.25, np.inf, -np.inf, 1e-40, -1e-40, 3e38, -3e38]
    for v in vals:
        for idx in (0, 1, 2047, 2150, R.TEXT_EOS, K.INT32_MAX, -1, -5, -2 ** 31):
            k = q3.argmax_key(v, idx)
            assert R.pack_key(v, idx) == k and R.make_key(v, idx) == k
            assert R.key_code(k) == idx
            assert R.raw_key(k >> 32, idx) == k
    assert R.ARMED == q3.argmax_key(-np.inf, 0) and R.key_code(R.ARMED) == 0
    for hi in K.HI_WORDS:
        assert R.key_code(R.raw_key(hi, -7)) == -7 and R.raw_key(hi, 3) >> 32 == hi
    assert K.HI_WORDS[0] == R.ARMED >> 32


# ------------------------------------------------------------ projection ------------------------------------------------------------
def test_project_against_the_oracle(tiny_assets, vivian):
    oa, ten, b = tiny_assets
    W = ten("proj.weight")
    rng = np.random.default_rng(11)
    x = np.stack([vivian, (rng.standard_normal(2048) * 3).astype(np.float32), np.zeros(2048, np.float32)])
    got = R.project(x, W, b)
    for t in range(3):
        assert np.array_equal(_bits(got[t]), _bits(oa.project(x[t])[: b.size]))
    assert not np.array_equal(_bits(got), _bits(R.project_fma(x, W, b)))   # the oracle's chain is the unfused one


@pytest.mark.parametrize("shape", sorted(set(c[:2] for c in K.PROJECTION_CASES)))
def test_projection_cases_tell_fma_from_mul_add(shape):
    n_in, n_out = shape
    ref, fma, d, mag = K.projection_ref(n_in, n_out)
    for case in K.PROJECTION_CASES:
        if case[:2] == shape:
            ntok = case[2]
            assert np.any(_bits(ref[:ntok]) != _bits(fma[:ntok])), case
            # and a chunk lost, repeated or taken in another order shows: both chains stay inside the bound, far from each other's bits
            assert np.all(np.abs(ref[:ntok].astype(np.float64) - d[:ntok]) <= R.gamma(n_in + 1) * mag[:ntok])
    explicit = np.float32(K.projection_inputs(n_in, n_out)[2][3])
    x, W, _ = K.projection_inputs(n_in, n_out)
    for i in range(n_in):   # one output by an explicit scalar loop: the vectorised chain is the chain
        explicit = np.float32(explicit + np.float32(x[2, i] * W[3, i]))
    assert _bits(explicit) == _bits(ref[2, 3])


def test_projection_cases_cover_every_axis():
    cs = K.PROJECTION_CASES
    assert {c[0] for c in cs} == {512, 1024, 2048} and {c[1] for c in cs} == {16, 48, 1024} and {c[2] for c in cs} == {1, 15, 16, 17, 33}
    assert {(c[0], c[2]) for c in cs} == {(a, b) for a in (512, 1024, 2048) for b in (1, 15, 16, 17, 33)}
    for n_in in (512, 1024, 2048):
        assert {c[3] for c in cs if c[0] == n_in} == {0, 4} and {c[4] for c in cs if c[0] == n_in} == {0, 3}
    ts = K.TABLE_CASES
    assert {c[0] for c in ts} == {1, 3, 4, 5, 9} and {c[1] for c in ts} == {16, 256, 272, 1024} and {c[2] for c in ts} == {64, 2048}


# ------------------------------------------------------------ code consumers ------------------------------------------------------------
def test_fallback_row_against_the_host_assets(tiny_assets):
    oa, _, _ = tiny_assets
    for tok in (4096, 4097, 151671, R.TEXT_EOS, 986800, 986801, K.INT32_MAX, -1, -2, -2 ** 31):
        want = oa.text_embedding(tok)
        assert np.array_equal(_bits(R.fallback_row(tok)), _bits(want)), tok
        assert np.array_equal(_bits(resume_ref.fallback_row(tok)), _bits(want)), tok
    row = R.fallback_row(986800)   # 986800*17 + 1616 = 2^24: exact and alternating below, even (so -1) from there on
    assert row[1614] == -1.0 and row[1615] == 0.0 and np.all(row[1616:] == -1.0) and set(row[:1616]) == {-1.0, 0.0}
    assert np.array_equal(R.fallback_row(-1)[17:21], [-1.0, 0.0, -1.0, 0.0])   # (u64)(-1)*17 + 17 wraps to 0


def test_feedback_against_the_resume_restatement(tiny_assets):
    oa, ten, _ = tiny_assets
    tables = [ten("codec_embd.%d" % q) for q in range(16)]
    rows = [t.shape[0] for t in tables]
    text = ten("text_embd")
    pad = oa.text_embedding(151671)
    rng = np.random.default_rng(12)
    codes = rng.integers(0, 2048, (6, 16)).astype(np.int32)
    codes[0] = 0
    codes[1] = [r - 1 for r in rows]
    codes[2] = rows
    codes[3, ::2] = -3
    codes[4, 1::2] = 100000
    want = resume_ref.feedback_rows(oa, pad, codes)
    got, d, mag = R.feedback(tables, rows, codes, pad)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.all(np.abs(got.astype(np.float64) - d) <= R.gamma(17) * mag)
    trail = [5, 4095, 4096, R.TEXT_EOS, -1, 986800]
    want = resume_ref.feedback_rows(oa, pad, codes, trail)
    n_frames = np.arange(6)
    last = R.last_rows(pad, 6, n_frames, np.full(6, 6), np.tile(trail, (6, 1)), text)
    assert np.array_equal(_bits(R.feedback(tables, rows, codes, pad, last)[0]), _bits(want))
    last = R.last_rows(pad, 6, n_frames, np.full(6, 3), np.tile(trail, (6, 1)), text)     # f >= n_trail: tts_pad
    want = resume_ref.feedback_rows(oa, pad, codes, trail[:3])
    assert np.array_equal(_bits(R.feedback(tables, rows, codes, pad, last)[0]), _bits(want))
    for q in (0, 7):
        g = R.gather(tables[q][:, :260], rows[q], [0, rows[q] - 1, rows[q], -1, K.INT32_MAX], 260)
        for j, c in enumerate([0, rows[q] - 1, rows[q], -1, K.INT32_MAX]):
            assert np.array_equal(_bits(g[j]), _bits(oa.codec_embedding(q, c)[:260]))


def test_code_and_trail_cases_hold_their_situations():
    for ntok in (1, 3, 65):
        c = K.feedback_codes(ntok)
        assert c.shape == (ntok, 16) and c.dtype == np.int32
        for q, r in enumerate(K.CODEC_ROWS):
            if ntok == 65:
                assert set(K.code_edges(r)) <= set(c[:, q].tolist()), q
        assert set(int(v) for v in K.code_edges(24)) | set(int(v) for v in K.code_edges(40)) >= set(c[c < 0].tolist())
        have = set()
        for q, r in enumerate(K.CODEC_ROWS):
            have |= {K.code_edges(r).index(v) for v in c[:, q].tolist() if v in K.code_edges(r)}
        assert have == set(range(9)), (ntok, have)           # even one token meets every edge somewhere
        k = K.keys_of(c, 17)
        assert np.all(k[:, 16] == K.U64) and [[R.key_code(v) for v in row[:16]] for row in k] == c.tolist()
        assert len({int(v) >> 32 for v in k[:, :16].ravel()}) > 1 or ntok == 0
    assert R.ARMED in K.keys_of(K.feedback_codes(65), 16)
    nf, nt, ids = K.trail_case(65)
    assert K.IDS_STRIDE > nt.max() - 1 and np.all(nt <= K.IDS_STRIDE)
    shapes = set(zip(nf.tolist(), nt.tolist()))
    assert any(f < n - 1 for f, n in shapes) and any(f == n - 1 for f, n in shapes) and any(f == n > 0 for f, n in shapes)
    assert any(n == 0 and f == 0 for f, n in shapes) and any(n == 0 and f > 0 for f, n in shapes)
    read = {int(ids[t, nf[t]]) for t in range(65) if nf[t] < nt[t]}
    assert read >= set(K.TRAIL_IDS)
    for ntok in (1, 3):
        nf, nt, _ = K.trail_case(ntok)
        assert np.any(nf < nt)


# ------------------------------------------------------------ slot state machine ------------------------------------------------------------
def _one_slot(finished, n_frames, code0, next_code=9):
    s = dict(finished=np.array([finished], np.int32), n_frames=np.array([n_frames], np.int32), max_frames=np.array([4], np.int32),
             t_slot=np.array([50], np.int32), t_pos=np.array([[7, 8, 9, 3]], np.int32),
             keys=np.array([[R.raw_key(0x3F800000 + q, code0 if q == 0 else 100 + q) for q in range(16)]], np.uint64),
             next_key0=np.array([R.raw_key(0x40000000, next_code)], np.uint64), hist=np.full((1, 4 * 16 + 4), -9, np.int32))
    return s


ADVANCE_TABLE = [   # (finished, n_frames, code_0) -> (finished, n_frames, history row written or None, counters stepped)
    ((0, 0, 5), (0, 1, 0, True)),                    # ordinary, first row
    ((0, 3, 5), (0, 4, 3, True)),                    # n_frames == max - 1: the last history row
    ((0, 4, 5), (0, 4, None, False)),                # n_frames == max: not live
    ((1, 1, 5), (1, 1, None, False)),                # finished
    ((0, 1, R.CODEC_EOS), (1, 1, None, False)),      # either EOS id finishes and appends nothing
    ((0, 1, R.TEXT_EOS), (1, 1, None, False)),
    ((1, 1, R.CODEC_EOS), (1, 1, None, False)),
    ((0, 2, 2149), (0, 3, 2, True)),                 # the ids next to the EOS ids are ordinary codes
    ((0, 2, R.TEXT_EOS + 1), (0, 3, 2, True)),
    ((0, 2, -1), (0, 3, 2, True)),                   # the history takes the code as it is
]


@pytest.mark.parametrize("before, after", ADVANCE_TABLE)
def test_advance_against_hand_written_states(before, after):
    s = _one_slot(*before)
    got = R.advance(s)
    fin, nf, row, stepped = after
    want_hist = np.full((1, 68), -9, np.int32)
    if row is not None:
        want_hist[0, row * 16: row * 16 + 16] = [before[2]] + [100 + q for q in range(1, 16)]
    assert got["finished"][0] == fin and got["n_frames"][0] == nf and np.array_equal(got["hist"], want_hist)
    assert got["t_slot"][0] == 50 + stepped and got["t_pos"].tolist() == [[7 + stepped, 8 + stepped, 9 + stepped, 3]]
    assert got["keys"][0].tolist() == [R.raw_key(0x40000000, 9)] + [R.ARMED] * 15 and got["next_key0"][0] == R.ARMED
    assert s["n_frames"][0] == before[1] and s["keys"][0, 1] != R.ARMED      # the input state is not changed


def test_gate_against_hand_written_states():
    # waits = !finished && f < max && open && f >= n_trail (max = 4)
    for fin, f, opn, ntrail, want in [(0, 1, 1, 1, True), (0, 1, 1, 0, True), (0, 1, 1, 2, False), (0, 1, 0, 1, False), (1, 1, 1, 1, False),
                                      (0, 4, 1, 1, False), (0, 3, 1, 3, True)]:
        s = _one_slot(fin, f, 5)
        s.update(open=np.array([opn], np.int32), n_trail=np.array([ntrail], np.int32), hidden=np.full((1, 2048), 1.0, np.float32),
                 save_hidden=np.full((1, 2048), 2.0, np.float32), draws=np.array([10], np.uint32), pdraws=np.array([20], np.uint32),
                 save_draws=np.array([[30, 40]], np.uint32))
        assert R.waits(s, 0) == want
        saved = R.stall_save(s)
        assert saved["save_hidden"][0, 0] == (1.0 if want else 2.0) and saved["save_draws"].tolist() == ([[10, 20]] if want else [[30, 40]])
        for k in ("hidden", "draws", "pdraws", "keys", "next_key0", "finished", "n_frames", "hist", "t_slot", "t_pos"):
            assert np.array_equal(saved[k], s[k]), k
        saved["hidden"][:] = 3.0; saved["draws"][:] = 11; saved["pdraws"][:] = 21     # the discarded frame ran
        got = R.advance_gated(saved)
        if want:
            assert got["hidden"][0, 0] == 1.0 and got["draws"][0] == 10 and got["pdraws"][0] == 20
            assert got["keys"][0].tolist() == [s["keys"][0, 0]] + [R.ARMED] * 15 and got["next_key0"][0] == R.ARMED
            for k in ("finished", "n_frames", "hist", "t_slot", "t_pos", "save_hidden", "save_draws"):
                assert np.array_equal(got[k], saved[k]), k
        else:
            plain = R.advance(saved)
            for k in got:
                assert np.array_equal(got[k], plain[k]), k
            assert got["hidden"][0, 0] == 3.0 and got["draws"][0] == 11


def test_slot_cases_hold_their_situations():
    for B in (1, 63, 64, 65, 130):
        s, eos = K.slot_state(B)
        assert s["hist"].shape == (B, K.HIST_STRIDE) and K.HIST_STRIDE > K.MAX_FRAMES * 16
        if B >= 6:
            assert np.any(s["finished"] == 1) and np.any(s["n_frames"] == K.MAX_FRAMES) and np.any(s["n_frames"] == K.MAX_FRAMES - 1)
            assert set(eos.values()) == {R.CODEC_EOS, R.TEXT_EOS}
    assert {K.SLOT_KINDS[k % 6] for k in range(6)} == set(K.SLOT_KINDS)
    s = K.gate_state()
    combos = {(int(s["finished"][b]), bool(s["n_frames"][b] < s["max_frames"][b]), int(s["open"][b]), bool(s["n_frames"][b] >= s["n_trail"][b]))
              for b in range(16)}
    assert len(combos) == 16
    assert [b for b in range(17) if R.waits(s, b)] == [7]
