"""The engine at every step width up to 256 slots (tests/engine_width_cases.py): each case fills a max_batch = B engine, drives the scheduler
by hand, reads every step's width from the stats() deltas and holds every slot's codes (log-probability rows, PCM) to the same requests on a
max_batch = 8 engine -- the fused 5-launch path the parity tests hold to the oracle -- and three slots to the oracle itself.
tests/test_engine_widths_cpu.py shows which kernel forms these widths reach.  Run with -s for the per-case times and errors
(profiles/engine_widths.md)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import engine_width_cases as W
import text_stream_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCM_RMS_TOL = 1e-4       # engine PCM against the oracle codec (the suite's constant, tests/test_gpu_parity.py)
PCM_BATCH_TOL = 1e-5     # wide against narrow engine PCM (the batch-invariance bound of tests/test_gpu_fullsize.py)
SPF = 1920


def _need(quant, flavour, i):
    """the most frames any case of (quant, flavour) asks of request i.  A request's frames do not depend on its max_steps (each frame follows
    from the prompt, the seed and the frames before it; EOS is masked), so one reference run of that length serves every case as a prefix"""
    n = [W.PATTERNS[p](B)[i] for q, B, p, _, f in W.CASES if (q, f) == (quant, flavour) and i < B]
    n += [W.lengths(B)[i] for q, B in W.CHILD_CASES if (q, "plain") == (quant, flavour) and i < B]
    return max(n)


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2))) if a.size else 0.0


def drive(ge, prompts, frames, opts, want_pcm):
    """submits every request, steps the scheduler by hand -> (results in request order, [width of each step that ran a frame group])"""
    rids = [ge.submit(p, max_steps=n, want_pcm=want_pcm, **o) for p, n, o in zip(prompts, frames, opts)]
    widths, s0 = [], ge.stats()
    for _ in range(100000):
        more = ge.sched_step()
        s1 = ge.stats()
        dg = s1["graph_frames"] - s0["graph_frames"]
        if dg:
            w = (s1["slot_frames"] - s0["slot_frames"]) / dg
            assert w == int(w) and s1["sched_steps"] == s0["sched_steps"] + 1, (w, dg)
            widths.append(int(w))
        s0 = s1
        if not more:
            break
    else:
        pytest.fail("the scheduler did not run dry")
    return [ge.result(r, want_pcm) for r in rids], widths


class Refs:
    """the shared references of the module: prompts, narrow engines and their results, oracle engines and theirs -- each computed once"""

    def __init__(self, gpu, oracle, model, spk):
        self.gpu, self.oracle, self.model, self.spk = gpu, oracle, model, spk
        self.assets = gpu.Assets(os.path.join(model, "gguf_q8_0", "qwen3_assets.gguf"))     # the assets file is the same F32 file in every directory
        self.pad = self.assets.tts_pad()
        self._prompts, self._narrow, self._oracle, self._done, self._odone = {}, {}, {}, {}, {}
        self.times = {"narrow": 0.0, "oracle": 0.0}

    def close(self):
        for e in list(self._narrow.values()) + list(self._oracle.values()):
            e.close()
        self.assets.close()

    def prompt(self, i):
        if i not in self._prompts:
            self._prompts[i] = W.prompt(self.assets, i, self.spk)
            self._prompts[i].setflags(write=False)
        return self._prompts[i]

    def narrow(self, quant, flavour, codec, wanted):
        """wanted [(i, frames)] -> {i: result} from the max_batch = 8 engine, eight requests a round (longest first, so a round's requests end
        together).  Without PCM request i runs _need frames once for all cases; with PCM it runs exactly `frames`."""
        t0 = time.time()
        key = (quant, codec)
        if key not in self._narrow:
            self._narrow[key] = self.gpu.Engine(self.model, quant, max_batch=W.NARROW, max_steps=W.MAX_FRAMES, load_codec=codec)
        ge = self._narrow[key]
        todo = []
        for i, n in wanted:
            n = n if codec else _need(quant, flavour, i)
            assert n >= dict(wanted)[i]
            if (quant, flavour, codec, i, n) not in self._done:
                todo.append((n, i))
        todo.sort(reverse=True)
        ge.set_logprobs(flavour == "all_variants")
        for k in range(0, len(todo), W.NARROW):
            part = todo[k:k + W.NARROW]
            ps, ns, os_ = [self.prompt(i) for _, i in part], [n for n, _ in part], [W.options(i, flavour) for _, i in part]
            if flavour == "plain":
                res = ge.generate_batch(ps, max_steps=ns, want_pcm=codec, **{k2: [o[k2] for o in os_] for k2 in os_[0]})
            else:                       # log-probability rows come through fetch_logprobs: the same scheduler, stepped here
                res, _ = drive(ge, ps, ns, os_, codec)
            for (n, i), r in zip(part, res):
                assert r["codes"].shape == (n, 16), (i, r["codes"].shape)
                self._done[(quant, flavour, codec, i, n)] = r
        self.times["narrow"] += time.time() - t0
        return {i: self._done[(quant, flavour, codec, i, n if codec else _need(quant, flavour, i))] for i, n in wanted}

    def oracle_codes(self, quant, flavour, i, frames):
        t0 = time.time()
        if quant not in self._oracle:
            self._oracle[quant] = self.oracle.Engine(os.path.join(self.model, "gguf_" + quant), None, 4)
        oe = self._oracle[quant]
        if (quant, flavour, i) not in self._odone:
            n, o = _need(quant, flavour, i), dict(W.options(i, flavour))
            if flavour == "plain":      # q3o_engine_generate itself
                c, _ = oe.generate(self.prompt(i), max_steps=n, **o)
            else:                       # the oracle has no surface for these options: the restatement of its loop over its model and sampler
                trail = o.pop("trailing_ids", ())
                c = text_stream_ref.generate(oe, self.pad, self.prompt(i), n, trail=trail, **o)
            assert c.shape == (n, 16)
            self._odone[(quant, flavour, i)] = c
        self.times["oracle"] += time.time() - t0
        return self._odone[(quant, flavour, i)][:frames]


@pytest.fixture(scope="module")
def refs(gpu, oracle, tiny_model, vivian):
    r = Refs(gpu, oracle, tiny_model, vivian)
    yield r
    r.close()


def _first_diff(a, b):
    if a.shape != b.shape:
        return "%d frames against %d" % (a.shape[0], b.shape[0])
    d = np.nonzero((a != b).any(axis=1))[0]
    return None if d.size == 0 else "first differing frame %d" % d[0]


def check_codes(quant, B, flavour, frames, res, nar, refs):
    for b in range(B):
        want = nar[b]["codes"][:frames[b]]
        d = _first_diff(res[b]["codes"], want)
        assert d is None, "slot %d of %d differs from the narrow engine: %s" % (b, B, d)
        if flavour == "all_variants":
            lp, wl = res[b]["logprobs"], nar[b]["logprobs"][:frames[b]]
            assert lp.shape == (frames[b], 17) and wl.shape == lp.shape, (b, lp.shape, wl.shape)
            d = _first_diff(lp.view(np.uint32), wl.view(np.uint32))
            assert d is None, "log-probability rows of slot %d of %d differ from the narrow engine: %s" % (b, B, d)
    for b in W.oracle_slots(B):
        d = _first_diff(res[b]["codes"], refs.oracle_codes(quant, flavour, b, frames[b]))
        assert d is None, "slot %d of %d differs from the oracle: %s" % (b, B, d)


@pytest.mark.parametrize("case", W.CASES, ids=[W.case_id(c) for c in W.CASES])
def test_engine_width(gpu, oracle, tiny_model, refs, case):
    quant, B, pattern, codec, flavour = case
    frames = W.PATTERNS[pattern](B)
    t0 = time.time()
    refs.times = {"narrow": 0.0, "oracle": 0.0}
    ge = gpu.Engine(tiny_model, quant, max_batch=B, max_steps=W.MAX_FRAMES, load_codec=codec)
    t_build = time.time() - t0
    try:
        if flavour == "all_variants":
            ge.set_logprobs(True)
        t1 = time.time()
        res, widths = drive(ge, [refs.prompt(i) for i in range(B)], frames, [W.options(i, flavour) for i in range(B)], codec)
        t_wide = time.time() - t1
    finally:
        ge.close()
    nar = refs.narrow(quant, flavour, codec, list(enumerate(frames)))
    worst_batch = worst_oracle = 0.0
    try:
        # every width the length pattern is built to replay ran (an admission wave that came up narrower only adds members of the same set)
        if pattern == "lengths":
            assert set(widths) == W.graph_widths(B), widths
        else:
            assert set(widths) == {B} and len(widths) >= 3, widths
        check_codes(quant, B, flavour, frames, res, nar, refs)
        if codec:
            for b in range(B):
                pcm = res[b]["pcm"]
                assert pcm.size == frames[b] * SPF and np.isfinite(pcm).all(), b
                assert nar[b]["pcm"].size == pcm.size, b
                worst_batch = max(worst_batch, _rms(pcm, nar[b]["pcm"]))
            t2 = time.time()
            oc = oracle.Codec(os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"))
            for b in W.pcm_oracle_streams(B):
                oc.reset()
                worst_oracle = max(worst_oracle, _rms(res[b]["pcm"], oc.decode(np.clip(res[b]["codes"], 0, 2047))))
            oc.close()
            refs.times["oracle"] += time.time() - t2
    finally:
        print("\nengine_widths %s: widths %s; build %.2f s, wide run %.2f s, narrow rounds %.2f s, oracle %.2f s, total %.2f s; pcm rms wide-narrow "
              "%.2e, oracle codec %.2e" % (W.case_id(case), widths, t_build, t_wide, refs.times["narrow"], refs.times["oracle"], time.time() - t0,
                                           worst_batch, worst_oracle))
    if codec:
        assert worst_batch < PCM_BATCH_TOL and worst_oracle < PCM_RMS_TOL, (worst_batch, worst_oracle)


CHILD = (
    "import sys, json, numpy as np\n"
    "sys.path[:0] = %r\n"
    "import q3tts as Q\n"
    "import engine_width_cases as W\n"
    "from test_gpu_engine_widths import drive\n"
    "model, quant, B, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]\n"
    "spk = np.array(json.load(open(%r))['spk_emb'], np.float32)\n"
    "ge = Q.Engine(model, quant, max_batch=B, max_steps=W.MAX_FRAMES, load_codec=False)\n"
    "frames = W.lengths(B)\n"
    "res, widths = drive(ge, [W.prompt(ge.assets, i, spk) for i in range(B)], frames, [W.options(i, 'plain') for i in range(B)], False)\n"
    "ge.close()\n"
    "codes = np.full((B, W.MAX_FRAMES, 16), -1, np.int32)\n"
    "for b, r in enumerate(res):\n"
    "    codes[b, :r['codes'].shape[0]] = r['codes']\n"
    "np.savez(out, codes=codes, n=np.array([r['codes'].shape[0] for r in res]), widths=np.array(widths))\n"
)


def test_engine_width_256_one_workgroup_per_token_walk(gpu, tiny_model, refs, tmp_path):
    """Decode steps whose int8 GEMM workgroups loop over several token tiles.  mfma_ztiles gives every tiny matrix one tile per workgroup;
    under Q3_MFMA_WGS=16 (read once, so in a process of its own) a 256-slot step's workgroups walk all eight tiles (four in the gate/up GEMMs
    and the predictor's 256-row matrices), as full-size matrices do in decode above 96 or 192 slots.  The codes equal the narrow reference."""
    import test_engine_widths_cpu as T
    plans = T.z1_plans()                                   # the plan under the child's environment, from a host-only child
    for key, (form, _, _, z) in plans.items():
        quant, model, name = key.split()
        if form != "GU_UNFUSED":
            assert form in ("GEMM_Q8_MFMA", "GEMM_KQ_MFMA", "GU_Q8_MFMA", "GU_KQ_MFMA") and z < 8, key
        if model == "talker" and name != "gate_up" or name == "qkv":
            assert z == 1, key
    path = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "qwen3-tts-rust_amd", "python")]
    child = CHILD % (path, os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json"))
    for quant, B in W.CHILD_CASES:
        t0 = time.time()
        out = os.path.join(str(tmp_path), quant + ".npz")
        r = subprocess.run([sys.executable, "-c", child, tiny_model, quant, str(B), out], env=dict(os.environ, Q3_MFMA_WGS="16"),
                           capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr[-2000:]
        t_child = time.time() - t0
        got = np.load(out)
        frames = W.lengths(B)
        assert set(got["widths"].tolist()) == W.graph_widths(B) and got["n"].tolist() == frames
        nar = refs.narrow(quant, "plain", False, list(enumerate(frames)))
        for b in range(B):
            d = _first_diff(got["codes"][b, :frames[b]], nar[b]["codes"][:frames[b]])
            assert d is None, "%s slot %d of %d differs from the narrow engine: %s" % (quant, b, B, d)
        print("\nengine_widths child %s-%d: widths %s; child %.2f s, total %.2f s" % (quant, B, got["widths"].tolist(), t_child, time.time() - t0))
