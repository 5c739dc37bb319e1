#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X-native Qwen3-TTS hot path (contract in the task prompt, part 4).

Default workload = BASELINE.json configs[2] ("C3", the largest single-GPU configuration): 64 concurrent utterances through
64 sequence slots per GPU, "Q3TTS-1.7B-synth" Q8_0 weights (seeded random, written on the box by tools/q3synth), speaker = vivian,
preset prompts with 16/32/64 synthetic text ids round-robin (27/43/75 prompt rows), greedy (temperature 0, seed 42), EOS masked so
every utterance emits exactly 4*K frames; continuous-batching scheduler + paged KV, codec decoding inside the timed region.
One "step" = one 4-frame streaming step of every slot (4 hipGraph replays of the batched frame + the codec chunks they complete).
The timed region is the whole job: prompt upload (PCIe, ~20 MB) + batched prefill + K steps + codec tail.
value = audio seconds generated per wall second, summed over ranks (weak scaling: the same 64 utterances per GPU; BASELINE
configs[3] = 512 utterances over 8 GPUs is exactly `--gpus 8`).

A config-C2 leg (single utterance, one slot, hipGraph-captured 4-frame streaming) runs after the timed region on rank 0 and supplies
`rtf`, `first_chunk_ms_p50` and `decode_ms_per_frame` -- the latency half of BASELINE.json's metric.
`--config c2` makes C2 the timed workload instead; `--config c5` = bf16 weights, 32 slots, voice-clone prompts.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment re-launches itself under torch.distributed.run (one rank per GPU) BEFORE
torch or HIP is touched; under a launcher, --gpus must equal WORLD_SIZE.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth_models  # noqa: E402  (seeded synthetic weights, cached per user outside the checkout)

FRAME_SEC = 1920.0 / 24000.0  # 12.5 Hz codec frames [EXT]
HBM_PEAK_GBS = 8000.0         # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
I8_MFMA_PEAK_TOPS = 5000.0    # dense int8 matrix-core peak (same guide: ~5 PFLOP/s fp8/int8 dense, sparsity excluded)
F32_MFMA_PEAK_TFLOPS = 157.3

_T0 = time.time()


def log(msg):
    print("[bench %.1fs] %s" % (time.time() - _T0, msg), file=sys.stderr, flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--config", default="c3", choices=["c2", "c3", "c5"], help="timed workload (BASELINE.json configs[1] / [2] / [4])")
    ap.add_argument("--quant", default=None, help="weights: q8_0 (default), q5_k_m, bf16 (default for c5)")
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"), help="default: the seeded full-size model in this user's cache")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-codec", action="store_true")
    ap.add_argument("--no-c2-leg", action="store_true", help="skip the single-utterance latency leg that rides along with c3 / c5")
    ap.add_argument("--batch", type=int, default=0, help="sequence slots per GPU (default: 1 for c2, 64 for c3, 32 for c5)")
    ap.add_argument("--requests", type=int, default=0, help="utterances per GPU (default = --batch); more than --batch queue up and are "
                                                            "admitted by the continuous-batching scheduler as slots retire")
    ap.add_argument("--clone", action="store_true", help="voice-clone prompt layout (implied by --config c5)")
    ap.add_argument("--ragged", action="store_true", help="utterance lengths 50..100 %% of 4*steps frames (slots retire at different times)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed region, write what it computed (codec tokens, PCM) "
                                                                           "as DIR/<name>.npy, float32 / float64, at most 64 MB in all (over all ranks)")
    ap.add_argument("--stub-engine", action="store_true", help=argparse.SUPPRESS)  # CPU rehearsal of the rank logic (tests/test_dist_cpu.py)
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.config == "c5":
        args.clone = True
    if args.quant is None:
        args.quant = "bf16" if args.config == "c5" else "q8_0"
    if args.batch <= 0:
        args.batch = {"c2": 1, "c3": 64, "c5": 32}[args.config]
    if args.dump_outputs:   # the codec tokens are always written whole: refuse before any work when they alone break the budget
        n_req, n_fr = max(args.requests, args.batch), 4 * args.steps
        if dump_fixed_bytes(n_req, n_fr) > DUMP_BYTES // args.gpus:
            ap.error("--dump-outputs: the codec tokens of %d requests x %d frames on each of %d rank(s) exceed the %d MB budget"
                     % (n_req, n_fr, args.gpus, DUMP_BYTES >> 20))
    if args.model_dir is None:
        args.model_dir = synth_models.model_dir("full")
    return args


def launch_ranks(n, argv):
    """--gpus N without a launcher: start N ranks (one per GPU) as a CHILD process tree and return its exit code.  Runs before torch /
    HIP is initialised in this process (a process that has touched the GPU must not exec or fork GPU work)."""
    port = 29400 + (os.getpid() % 500)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def reduce_over_ranks(dist, torch, dev, audio_s, elapsed):
    """whole-job aggregate: SUM of the audio seconds every rank generated, MAX of the elapsed times (ranks may hold different work)"""
    if dist is None:
        return audio_s, elapsed
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    a = torch.tensor([audio_s], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(a, op=dist.ReduceOp.SUM)
    return float(a.item()), float(t.item())


def describe_ranks(dist, torch, dev, audio_s, elapsed, device_name):
    """What a multi-GPU line must say about itself (nobody can launch N > 1 on this pool but the driver): per-rank audio seconds and elapsed
    times (all_gather), the world size the COLLECTIVE saw (an all_reduce of ones -- not the launcher's environment), the backend, and every
    rank's device name.  Single process: the same keys with one entry."""
    if dist is None:
        return {"per_rank_audio_s": [audio_s], "per_rank_elapsed_s": [elapsed], "rccl_world": 1, "backend": None, "devices": [device_name]}
    world = dist.get_world_size()
    mine = torch.tensor([audio_s, elapsed], dtype=torch.float64, device=dev)
    allv = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(world)]
    dist.all_gather(allv, mine)
    ones = torch.ones(1, dtype=torch.float64, device=dev)
    dist.all_reduce(ones, op=dist.ReduceOp.SUM)
    names = [None] * world
    dist.all_gather_object(names, device_name)
    return {"per_rank_audio_s": [float(v[0].item()) for v in allv], "per_rank_elapsed_s": [float(v[1].item()) for v in allv],
            "rccl_world": int(round(float(ones.item()))), "backend": dist.get_backend(), "devices": names}


def ensure_model(model_dir, quant):
    synth_models.full(quant, model_dir)


DUMP_BYTES = 64 << 20      # --dump-outputs, all ranks together
DUMP_HEADERS = 4096        # room left for the .npy headers


def dump_fixed_bytes(n_req, max_frames):
    """bytes of the arrays dump_outputs never samples: codes, frames, pcm_samples"""
    return n_req * max_frames * 16 * 4 + 2 * n_req * 8 + DUMP_HEADERS


def dump_outputs(out_dir, results, prefix="", budget=DUMP_BYTES):
    """What the timed generate_batch call handed back to its caller, for output-for-output comparison of two builds:
    codes.npy   [requests, max frames, 16] codec tokens (float32, exact below 2^24; -1 past a request's last frame)
    frames.npy  [requests] frames per request (float64)
    pcm.npy     the requests' PCM concatenated in request order (float32); when that exceeds what the budget leaves, a fixed
                seeded sample of it, sorted, with pcm_index.npy (float64) = the sample's positions in the concatenation
    pcm_samples.npy  [requests] PCM samples per request (float64)
    Everything stays within `budget` bytes; the caller refuses shapes whose codes alone would not fit (dump_fixed_bytes)."""
    os.makedirs(out_dir, exist_ok=True)
    frames = np.array([r["codes"].shape[0] for r in results], np.float64)
    codes = np.full((len(results), int(frames.max()), 16), -1.0, np.float32)
    for i, r in enumerate(results):
        codes[i, : r["codes"].shape[0]] = r["codes"]
    arrays = {"codes": codes, "frames": frames}
    if dump_fixed_bytes(len(results), codes.shape[1]) > budget:
        raise ValueError("dump_outputs: %d requests x %d frames of codes exceed the %d-byte budget" % (len(results), codes.shape[1], budget))
    if all(r["pcm"] is not None for r in results):
        pcm = np.concatenate([r["pcm"] for r in results]).astype(np.float32)
        arrays["pcm_samples"] = np.array([r["pcm"].size for r in results], np.float64)
        room = budget - sum(a.nbytes for a in arrays.values()) - DUMP_HEADERS
        if pcm.nbytes > room:
            n = room // (4 + 8)                                             # float32 value + float64 position per sampled sample
            idx = np.sort(np.random.default_rng(0).choice(pcm.size, size=n, replace=False))
            arrays["pcm_index"] = idx.astype(np.float64)
            pcm = pcm[idx]
        arrays["pcm"] = pcm
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, prefix + name + ".npy"), a)
    return sorted(arrays)


def build_prompt(assets, spk_emb, n_text=32, seed=42):
    rng = np.random.default_rng(seed)
    text = rng.integers(0, 4000, n_text).astype(np.int32)
    return assets.build_core(text, lang_id=2055, spk_emb=spk_emb)


def host_cpu_info():
    model, phys, logical = "unknown", None, os.cpu_count()
    try:
        cores = set()
        phys_id = core_id = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys_id = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core_id = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys_id is not None and core_id is not None:
                    cores.add((phys_id, core_id))
                phys_id = core_id = None
        phys = len(cores) or None
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = logical
    return {"model": model, "physical_cores": phys, "logical_cpus": logical, "usable_cpus": usable}


def cpu_baseline(model_dir, quant_dir, prompt, codec_path):
    """The CPU restatement (oracle/, kind "port") of the same single-utterance loop, timed on this box's host cores the way the reference
    threads it: talker + predictor on 4 threads (llama.cpp thread cap, /root/reference/src/models/llama/mod.rs:420-428), the codec decoder
    on its own thread (engine.rs:495) with a team of its own -- so the AR loop and the decoder overlap and the utterance takes
    max(AR, codec).  Headline = 4 + 4 threads; `all_cores` = every usable core for the AR loop and then for the codec (no overlap assumed:
    both want all of them).  The codec is threaded over (channel, time) pairs, so it scales with the cores it is given and the figures are
    AR-bound like the reference's own (README.md:31-32).  BOUNDED sample (a few prefill tokens + frames), extrapolated to the 43-row /
    128-frame utterance of C2."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import q3oracle as O
    info = host_cpu_info()
    n_pre, n_fr, frames = 8, 8, 128
    out = {"unit": "audio_s/s", "kind": "port", "host": info}

    def ar_rate(threads):
        eng = O.Engine(os.path.join(model_dir, quant_dir), None, threads)
        eng.generate(prompt[-2:], max_steps=0)  # page the mmapped weights in (untimed)
        t0 = time.time()
        eng.generate(prompt[-n_pre:], max_steps=0)
        t_pre = (time.time() - t0) / n_pre
        t0 = time.time()
        eng.generate(prompt[-n_pre:], max_steps=n_fr)
        t_frame = max((time.time() - t0 - t_pre * n_pre) / n_fr, 1e-9)
        eng.close()
        return t_pre, t_frame

    def codec_rate(threads):
        if not (codec_path and os.path.exists(codec_path)):
            return None
        O.set_threads(threads)
        oc = O.Codec(codec_path)
        oc.reset()
        rng = np.random.default_rng(3)
        oc.decode(rng.integers(0, 2048, (1, 16)))          # warm
        t0 = time.time()
        oc.decode(rng.integers(0, 2048, (4, 16)))          # one 4-frame chunk, as the chunker hands it over
        t = (time.time() - t0) / 4
        oc.close()
        return t

    t_pre4, t_frame4 = ar_rate(4)
    t_codec4 = codec_rate(4)
    ar_total = t_pre4 * prompt.shape[0] + t_frame4 * frames
    codec_total = (t_codec4 or 0.0) * frames
    total4 = max(ar_total, codec_total) + (4 * (t_codec4 or 0.0))   # overlapped threads + the last chunk's decode after the loop
    out.update({"value": frames * FRAME_SEC / total4, "cores": 4 + (4 if t_codec4 else 0), "rtf": total4 / (frames * FRAME_SEC),
                "s_per_prefill_token": t_pre4, "s_per_frame_ar": t_frame4, "s_per_frame_codec": t_codec4,
                "bound_by": "codec thread" if codec_total > ar_total else "AR loop"})
    allc = max(1, min(int(info["usable_cpus"] or 4), 16))   # 16 = a one-GPU box's CPU share on this pool
    extra = ""
    if allc > 4:
        t_preA, t_frameA = ar_rate(allc)
        t_codecA = codec_rate(allc)
        totalA = t_preA * prompt.shape[0] + (t_frameA + (t_codecA or 0.0)) * frames
        out["all_cores"] = {"value": frames * FRAME_SEC / totalA, "cores": allc, "rtf": totalA / (frames * FRAME_SEC),
                            "s_per_prefill_token": t_preA, "s_per_frame_ar": t_frameA, "s_per_frame_codec": t_codecA,
                            "note": "AR loop and codec both on every core, one after the other (no overlap assumed)"}
        extra = "; all-cores run: %d threads" % allc
    out["reference_published"] = {"rtf_cpu_q8_0": 1.866, "rtf_cpu_q5_k_m": 1.677, "hardware": "Intel i9-13980HX, llama.cpp b8123 + onnxruntime 1.24.2, real weights",
                                  "source": "reference README.md:31-32 (context only: different CPU, weights and utterance)"}
    out["sample"] = ("oracle single-utterance loop, config-C2 shape: %d prefill tokens + %d AR frames timed on 4 threads (%.3f s/token, "
                     "%.3f s/frame)%s; utterance = max(AR, codec thread) extrapolated to %d prompt rows + %d frames%s"
                     % (n_pre, n_fr, t_pre4, t_frame4,
                        ", codec absent" if t_codec4 is None else " + one 4-frame codec chunk on a 4-thread team of its own (%.3f s/frame)" % t_codec4,
                        prompt.shape[0], frames, extra))
    return out


def load_traffic(kernel_key):
    """HBM bytes per launch of the roofline kernel from the tracked PMC summary (profiles/hbm_traffic_latest.json, written by
    scripts/make_hbm_traffic_md.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes); None when no entry matches."""
    path = os.path.join(ROOT, "profiles", "hbm_traffic_latest.json")
    try:
        tab = json.load(open(path))
    except (OSError, ValueError):
        return None
    ent = tab.get(kernel_key) or next((v for k, v in tab.items() if k != "_meta" and k.startswith(kernel_key.rstrip(">"))), None)  # template arguments may follow
    return float(ent["read_bytes"] + ent.get("write_bytes", 0.0)) if ent else None


def traffic_source(kernel_key):
    """`roofline.traffic` is NOT measured by this run (PMC counters need separate rocprofv3 --pmc passes): it is read from the tracked summary of the
    builder's last PMC pass; say so, and say which commit's kernel it belongs to, so a stale figure is visible as stale"""
    path = os.path.join(ROOT, "profiles", "hbm_traffic_latest.json")
    try:
        tab = json.load(open(path))
    except (OSError, ValueError):
        return None
    meta = tab.get("_meta", {})
    return "tracked file profiles/hbm_traffic_latest.json (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, %s); not collected by this run" % (
        meta.get("collected", "round 2, kernel k_gemm_q8_mfma<true> before the round-3 one-tile kernel"))


class StubEngine:
    """CPU stand-in used only by tests/test_dist_cpu.py to rehearse the launcher + rank aggregation (no GPU, no library)."""

    class _Assets:
        def build_core(self, text, lang_id=2055, spk_emb=None):
            return np.zeros((11 + len(text), 2048), np.float32)

        def build_clone(self, text, rc, rt, se):
            return np.zeros((133, 2048), np.float32)

    def __init__(self, rank):
        self.assets = StubEngine._Assets()
        self.rank = rank

    def generate_batch(self, prompts, max_steps=8, **kw):
        ms = max_steps if isinstance(max_steps, (list, tuple)) else [max_steps] * len(prompts)
        time.sleep(0.02 * (1 + self.rank))
        return [{"codes": np.zeros((m, 16), np.int32), "pcm": None, "prefill_ms": 1.0, "first_chunk_ms": 2.0, "total_ms": 3.0} for m in ms]

    def stats(self):
        return {"frame_loop_ms": 1.0, "graph_frames": 1, "slot_frames": 1.0, "prefill_ms": 0.0, "codec_ms": 0.0, "codec_calls": 0,
                "gemv_bytes": 0.0, "gemv_ms": 0.0, "gemv_launches": 0, "gu_bytes": 0.0, "gu_ms": 0.0, "gu_launches": 0}

    def reset_stats(self):
        pass

    def set_instrument(self, on):
        pass

    def bytes_per_step(self, batch, ctx):
        return 0.0

    def close(self):
        pass


def main(argv=None):
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:] if argv is None else argv))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d does not match WORLD_SIZE %d (launch one rank per GPU, or drop the launcher and let "
                         "--gpus start the ranks)" % (args.gpus, world))
    import torch
    stub = args.stub_engine
    dist = None
    if world > 1 or os.environ.get("Q3_BENCH_FORCE_DIST") == "1":  # the knob rehearses the RCCL path with a single rank
        import torch.distributed as dist
        if stub:
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cpu") if stub else torch.device("cuda", local_rank)

    def sync():
        if not stub:
            torch.cuda.synchronize()

    log("torch imported")
    if local_rank == 0 and not stub:
        ensure_model(args.model_dir, args.quant)
    log("model ready")
    if dist:
        dist.barrier()

    quant_dir = {"q8_0": "gguf_q8_0", "q5_k_m": "gguf_q5_k_m", "bf16": "gguf_bf16"}.get(args.quant, "gguf")
    codec_path = os.path.join(args.model_dir, "onnx", "q3tts_codec.gguf")
    have_codec = (not args.no_codec) and (stub or os.path.exists(codec_path))
    max_frames = 4 * max(args.steps, args.warmup, 2)
    if stub:
        eng = StubEngine(rank)
        Q = None
    else:
        import q3tts as Q
        eng = Q.Engine(args.model_dir, args.quant, max_batch=args.batch, max_prompt=1024, max_steps=max_frames, load_codec=have_codec,
                       device=local_rank)

    # speaker embedding: rank 0 owns the voice file; the ONE collective of the path is its broadcast over RCCL/xGMI
    spk = torch.zeros(2048, dtype=torch.float32, device=dev)
    if rank == 0:
        v = json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))
        spk.copy_(torch.tensor(v["spk_emb"], dtype=torch.float32))
    if dist:
        dist.broadcast(spk, src=0)
    spk_emb = spk.cpu().numpy()
    prompt = build_prompt(eng.assets, spk_emb)
    log("engine up, prompt rows %d" % prompt.shape[0])

    n_req = max(args.requests, args.batch)
    clone_info = None
    if args.clone:  # clone prompts, 4 voices (the speaker embeddings are perturbations of the broadcast one; codes are seeded)
        voices = []
        for v in range(4):
            vr = np.random.default_rng(1000 + v)
            voices.append(((spk_emb * (1.0 - 0.1 * v) + 0.01 * vr.standard_normal(2048)).astype(np.float32), vr.integers(0, 2048, 62 * 16).astype(np.int32),
                           vr.integers(0, 4000, 24).astype(np.int32)))
        if not stub:
            # reference-audio front end (row a16, onnx.rs:167-320): log-mel of a seeded 5 s chirp + noise per voice on the device.  The codec /
            # speaker encoder graphs that would consume it are not in the container (SURVEY 8a row a17 -> next row f-2), so the reference
            # codes and speaker embeddings above stay synthetic; the mel time is reported, not hidden.
            tt = np.arange(5 * 24000) / 24000.0
            ref_audio = [(0.4 * np.sin(2 * np.pi * (200 + 600 * v + 2500 * tt) * tt) + 0.02 * np.random.default_rng(7 + v).standard_normal(tt.size)).astype(np.float32)
                         for v in range(4)]
            Q.mel(ref_audio[0])  # warm-up (filter bank + twiddles are built on first use)
            t0 = time.perf_counter()
            mels = [Q.mel(a) for a in ref_audio]
            clone_info = {"ref_audio_s_per_voice": 5.0, "voices": 4, "mel_frames_per_voice": int(mels[0].shape[0]),
                          "mel_ms_per_voice_incl_pcie": 1e3 * (time.perf_counter() - t0) / 4,
                          "encoders": "absent from the container (SURVEY 8a a17 / 8f f-2): reference codes and speaker embeddings are seeded synthetic"}
        prompts = []
        for i in range(n_req):
            se, rc, rt = voices[i % 4]
            prompts.append(eng.assets.build_clone(np.random.default_rng(42 + i).integers(0, 4000, 32).astype(np.int32), rc, rt, se))
        prompt = prompts[0]
    else:
        prompts = [prompt] if n_req == 1 else [build_prompt(eng.assets, spk_emb, n_text=(16, 32, 64)[i % 3], seed=42 + i) for i in range(n_req)]
    last_run = {}

    def run(engine, plist, steps, pcm):
        ms = [4 * steps] * len(plist)
        if args.ragged and len(plist) > 1:
            ms = [max(1, int(4 * steps * (0.5 + 0.5 * ((i * 7) % 11) / 10.0))) for i in range(len(plist))]
        res = engine.generate_batch(plist, max_steps=ms, temperature=0.0, seed=42, mask_eos=True, want_pcm=pcm)
        last_run["results"] = res
        last_run["frames"] = sum(r["codes"].shape[0] for r in res)
        last_run["first_chunk"] = [r["first_chunk_ms"] for r in res]
        assert all(r["codes"].shape[0] == m for r, m in zip(res, ms)), "EOS-masked runs must emit exactly max_steps frames"
        return res[0]

    if args.warmup > 0:
        run(eng, prompts, args.warmup, have_codec)
    log("warmup done")
    eng.reset_stats()
    if dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    res = run(eng, prompts, args.steps, have_codec)
    sync()
    if dist:
        dist.barrier()
    elapsed_local = time.perf_counter() - t0
    audio_local = last_run["frames"] * FRAME_SEC
    audio_s, elapsed = reduce_over_ranks(dist, torch, dev, audio_local, elapsed_local)
    ranks_info = describe_ranks(dist, torch, dev, audio_local, elapsed_local,
                                "cpu (stub engine)" if stub else torch.cuda.get_device_name(local_rank))
    st = eng.stats()
    log("timed region done: %.3f s (this rank %.3f s, %.1f audio-s)" % (elapsed, elapsed_local, audio_local))
    n_frames = res["codes"].shape[0]
    timed_first_chunk = list(last_run["first_chunk"])
    if args.dump_outputs:
        # every rank writes its own results under its own prefix, in an equal share of the budget
        names = dump_outputs(args.dump_outputs, last_run["results"], "" if world == 1 else "rank%d_" % rank, DUMP_BYTES // world)
        log("timed outputs written to %s: %s" % (args.dump_outputs, ", ".join(names)))

    if rank == 0:
        frame_ms = st["frame_loop_ms"] / max(st["graph_frames"], 1)   # one graph replay advances every active slot by a frame
        is_float = args.quant in ("bf16", "f16", "f32")
        workload = {"c2": "C2: single utterance per GPU, hipGraph-captured 4-frame streaming",
                    "c3": "C3: %d concurrent utterances through %d slots per GPU, continuous-batching scheduler + paged KV" % (n_req, args.batch),
                    "c5": "C5: voice-clone prompts (133 rows, 4 voices), %d utterances through %d slots per GPU" % (n_req, args.batch)}[args.config]
        if args.config == "c2" and args.batch > 1:
            workload = "custom: %d utterances through %d slots per GPU" % (n_req, args.batch)
        out = {
            "metric": "audio-seconds generated per second (aggregate over GPUs) = concurrent real-time streams; RTF and first-chunk latency from the single-utterance leg",
            "value": audio_s / elapsed, "unit": "audio_s/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"bf16": "f32 x bf16 weights", "f16": "f32 x f16 weights"}.get(args.quant, "i8"), "data": "synthetic",
            "config": {"workload": workload + ", Q3TTS-1.7B-synth %s, greedy, EOS masked" % args.quant.upper(),
                       "quant": args.quant, "n_prompt": int(prompt.shape[0]), "frames_per_utterance": int(n_frames), "batch_per_gpu": args.batch,
                       "requests_per_gpu": n_req, "ragged": bool(args.ragged),
                       "mean_graph_width": st["slot_frames"] / max(st["graph_frames"], 1),
                       "codec_in_timed_region": bool(have_codec), "parallelism": "request-sharded x%d" % world},
            "audio_s_total": audio_s, "elapsed_s": elapsed,
            "ranks": ranks_info,   # per-rank audio / elapsed, the world size the collective saw, backend, device names
            "batch_rtf": elapsed / audio_s,
            "batch_first_chunk_ms_p50": statistics.median([v for v in timed_first_chunk if v > 0] or [0.0]),
            "batch_decode_ms_per_step_frame": frame_ms,
            "prefill_ms": st["prefill_ms"],
        }
        if clone_info:
            out["config"]["ref_audio_front_end"] = clone_info
        if stub:
            print(json.dumps(out))
            eng.close()
            if dist:
                dist.barrier()
                dist.destroy_process_group()
            return
        # ---- instrumented leg: the same K steps, eager launches with a HIP-event pair (on the engine's stream) around every weight-streaming launch
        eng.reset_stats()
        eng.set_instrument(True)
        run(eng, prompts, args.steps, False)
        eng.set_instrument(False)
        si = eng.stats()
        mean_ctx = float(np.mean([p.shape[0] for p in prompts])) + 4 * args.steps / 2.0
        step_bytes = eng.bytes_per_step(args.batch, mean_ctx)
        out["frame_hbm_frac"] = (step_bytes / (frame_ms * 1e-3) / 1e9) / HBM_PEAK_GBS if frame_ms > 0 else None
        fam_bytes, fam_ms, fam_n = si["gemv_bytes"] + si["gu_bytes"], si["gemv_ms"] + si["gu_ms"], si["gemv_launches"] + si["gu_launches"]
        fam_gbs = fam_bytes / (fam_ms * 1e-3) / 1e9 if fam_ms > 0 else 0.0
        gu_gbs = si["gu_bytes"] / (si["gu_ms"] * 1e-3) / 1e9 if si["gu_ms"] > 0 else 0.0
        gu_us = 1e3 * si["gu_ms"] / max(si["gu_launches"], 1)
        gu_bpl = si["gu_bytes"] / max(si["gu_launches"], 1)
        ntok = args.batch
        if args.batch == 1:
            kq = args.quant == "q5_k_m"
            kname = "q3::k_gateup_swiglu<1, 8, %s> (talker: norm + gate/up GEMV + SwiGLU + quant%s)" % ("true" if kq else "false", ", packed K-quant planes" if kq else "")
            kkey = "k_gateup_swiglu<1, 8, true>" if kq else "k_gateup_swiglu<1, 8>"
        elif is_float:
            kname, kkey = "q3::k_gateup_float_mfma16 / k_gemm_float_mfma (talker gate/up, K = 1 f32 MFMA chains)", "k_gateup_float"
        else:
            if args.quant == "q5_k_m":
                kname, kkey = "q3::k_gemm_kq_mfma<GU, Q5_K> (talker gate/up GEMM on packed K-quant planes + SwiGLU + quant, %d tokens per launch)" % ntok, "k_gemm_kq_mfma<true"
            else:
                one_tile = ntok <= 128   # every workgroup owns one 32-token tile: the latency-tuned kernel (csrc/kernels.hip launch_gateup_mfma)
                kname = "q3::%s<GU> (talker gate/up GEMM + SwiGLU + quant, %d tokens per launch)" % ("k_gemm_q8_tile1" if one_tile else "k_gemm_q8_mfma", ntok)
                kkey = "k_gemm_q8_tile1<true>" if one_tile else "k_gemm_q8_mfma<true>"
        # dominant kernel by algorithmic bytes AND by share of the batched step: the talker's gate/up launch (12288 rows x 2048 x 1.0625 B
        # = 26.7 MB of Q8_0 weights per launch, 28 launches per frame step)
        roof = {"bound": "hbm", "kernel": "%s; %d launches" % (kname, si["gu_launches"]),
                "achieved": gu_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gu_gbs / HBM_PEAK_GBS,
                "avg_launch_us": gu_us, "bytes_per_launch": gu_bpl, "traffic": load_traffic(kkey), "traffic_source": traffic_source(kkey),
                "method": "HIP-event pair on the engine's stream around every launch in an eager replay of the same K steps (adds ~2 us over rocprofv3's kernel time)",
                "family_all_weight_streaming_launches": {"achieved": fam_gbs, "frac": fam_gbs / HBM_PEAK_GBS, "launches": fam_n,
                                                         "avg_launch_us": 1e3 * fam_ms / max(fam_n, 1), "bytes_per_launch": fam_bytes / max(fam_n, 1)}}
        if args.batch > 1 and si["gu_ms"] > 0:
            if is_float:
                esz = 4 if args.quant == "f32" else 2
                tfl = 2.0 * (si["gu_bytes"] / esz) * ntok / (si["gu_ms"] * 1e-3) / 1e12
                roof.update({"bound": "mfma", "achieved": tfl, "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tfl / F32_MFMA_PEAK_TFLOPS,
                             "hbm_view": {"achieved_gbs": gu_gbs, "frac": gu_gbs / HBM_PEAK_GBS}})
            else:
                # int8 view: 2 ops per weight element per token on the int8 matrix cores; at <= 256 tokens per launch HBM is the nearer roof
                tops = 2.0 * (si["gu_bytes"] / 1.0625) * ntok / (si["gu_ms"] * 1e-3) / 1e12
                roof["mfma_view"] = {"achieved_tops": tops, "peak_tops": I8_MFMA_PEAK_TOPS, "frac": tops / I8_MFMA_PEAK_TOPS, "tokens_per_launch": ntok}
        out["roofline"] = roof
        log("instrumented leg done")
        # ---- config-C2 leg: the latency half of the metric (single utterance, one slot) ----
        c2_prompt = prompt if (n_req == 1 or args.clone) else build_prompt(eng.assets, spk_emb)
        if args.batch == 1:
            e1, own = eng, False
        elif not args.no_c2_leg:
            e1, own = Q.Engine(args.model_dir, args.quant, max_batch=1, max_prompt=1024, max_steps=max_frames, load_codec=have_codec, device=local_rank), True
        else:
            e1, own = None, False
        if e1 is not None:
            if own:
                run(e1, [c2_prompt], max(args.warmup, 1), have_codec)
            e1.reset_stats()
            sync()
            t1 = time.perf_counter()
            run(e1, [c2_prompt], args.steps, have_codec)
            sync()
            c2_elapsed = time.perf_counter() - t1
            s1 = e1.stats()
            lat = []
            for _ in range(5):
                r = run(e1, [c2_prompt], 2, have_codec)
                lat.append(r["first_chunk_ms"] if have_codec else r["prefill_ms"] + (r["total_ms"] - r["prefill_ms"]) / 2.0)
            c2_audio = 4 * args.steps * FRAME_SEC
            out["rtf"] = c2_elapsed / c2_audio
            out["first_chunk_ms_p50"] = statistics.median(lat)
            out["decode_ms_per_frame"] = s1["frame_loop_ms"] / max(s1["graph_frames"], 1)
            out["c2_leg"] = {"workload": "C2: single utterance, 1 slot, %d frames, hipGraph 4-frame steps, codec included" % (4 * args.steps),
                             "audio_s_per_s": c2_audio / c2_elapsed, "prefill_ms": s1["prefill_ms"], "n_prompt": int(c2_prompt.shape[0]),
                             "frame_hbm_frac": (e1.bytes_per_step(1, c2_prompt.shape[0] + 2.0 * args.steps) / (out["decode_ms_per_frame"] * 1e-3) / 1e9) / HBM_PEAK_GBS}
            if own:
                e1.close()
            log("C2 leg done")
        if world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args.model_dir, quant_dir, build_prompt(eng.assets, spk_emb), codec_path if have_codec else None)
            except Exception as ex:  # the oracle is optional test infrastructure; report, do not hide
                out["cpu_baseline"] = {"value": None, "unit": "audio_s/s", "cores": 4, "kind": "port", "sample": "failed: %s" % ex}
            log("cpu baseline done")
        print(json.dumps(out))
    eng.close()
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
