"""The scheduler's pure bookkeeping (qwen3-tts-rust_amd/csrc/sched_logic.h: frame variant, slot table, stall predicate, prefill chunk packer, staging cursor),
built with plain g++ -- no HIP header, no GPU -- and compared with the few lines of Python that restate each rule here."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2150  # Q3_CODEC_EOS


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("sched_logic") / "sched_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "sched_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_header_is_hip_free():
    src = open(os.path.join(ROOT, "qwen3-tts-rust_amd", "csrc", "sched_logic.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)', src)
    assert includes and all(i == "../../include/q3tts_spec.h" or "/" not in i and "." not in i for i in includes)  # the spec header + std only


def test_variant_key(driver):
    combos = [(w,) + f for w in (1, 2, 4, 512) for f in itertools.product((0, 1), repeat=5)]
    out = driver("".join("key %d %d %d %d %d %d\n" % c for c in combos))
    keys = [int(x) for x in out]
    assert keys == [w * 32 + gate * 16 + trail * 8 + pred * 4 + pen * 2 + sampled for (w, sampled, pen, pred, trail, gate) in combos]
    assert len(set(keys)) == len(combos) == 128


# one slot: has_request live temperature penalty pred_temperature n_trail open_request host_open finished n_frames max_frames
def slot(has=1, live=1, temp=0.0, pen=1.0, ptemp=0.0, n_trail=0, open_req=0, host_open=0, fin=0, nf=0, maxf=16):
    return (has, live, temp, pen, ptemp, n_trail, open_req, host_open, fin, nf, maxf)


def slots_text(cmd, slots):
    return "%s %d\n" % (cmd, len(slots)) + "".join("%d %d %r %r %r %d %d %d %d %d %d\n" % s for s in slots)


def variant_ref(slots):
    v = [0, 0, 0, 0, 0]
    for (has, live, temp, pen, ptemp, n_trail, open_req, host_open, fin, nf, maxf) in slots:
        if not live:
            continue
        v[0] |= temp > 0
        v[1] |= pen != 1.0
        v[2] |= ptemp > 0
        v[3] |= n_trail > 0 or bool(open_req) or bool(host_open)
        v[4] |= bool(host_open)
    return [int(x) for x in v]


IDLE = slot(has=0, live=0)
# a reserved slot that is not live (prefilling) and a retired one whose stale flags would set every bit: neither may contribute
LOUD = slot(live=0, temp=0.9, pen=1.3, ptemp=0.5, n_trail=3, open_req=1, host_open=1)
VARIANT_CASES = {
    "no live slot": ([IDLE, LOUD, IDLE, LOUD], [0, 0, 0, 0, 0]),
    "one greedy slot": ([slot(), IDLE, LOUD, IDLE], [0, 0, 0, 0, 0]),
    "sampled next to greedy": ([slot(), slot(temp=0.7), slot(), LOUD], [1, 0, 0, 0, 0]),
    "penalty and sampled predictor": ([slot(pen=1.2), slot(ptemp=0.4), LOUD, IDLE], [0, 1, 1, 0, 0]),
    "closed trail": ([slot(), slot(n_trail=5), IDLE, LOUD], [0, 0, 0, 1, 0]),
    "open trail": ([LOUD, slot(open_req=1, host_open=1), slot(), IDLE], [0, 0, 0, 1, 1]),
    "open trail, no ids yet, next to sampled": ([slot(temp=0.7), IDLE, LOUD, slot(open_req=1, host_open=1, n_trail=0)], [1, 0, 0, 1, 1]),
    "open request that has been closed": ([slot(open_req=1, host_open=0, n_trail=0), IDLE, LOUD, slot()], [0, 0, 0, 1, 0]),
}


def test_variant_derivation(driver):
    names = list(VARIANT_CASES)
    out = driver("".join(slots_text("variant", VARIANT_CASES[n][0]) for n in names))
    for n, line in zip(names, out):
        got = [int(x) for x in line.split()]
        assert got == VARIANT_CASES[n][1] == variant_ref(VARIANT_CASES[n][0]), n
        assert not got[4] or got[3], n  # gate => trail


def stall_ref(slots):
    live = [s for s in slots if s[1]]
    return int(bool(live) and all(host_open and not fin and nf < maxf and nf >= n_trail
                                  for (_, _, _, _, _, n_trail, _, host_open, fin, nf, maxf) in live))


def waiting(**kw):
    return slot(**dict(dict(open_req=1, host_open=1, n_trail=4, nf=4, maxf=16), **kw))


STALL_CASES = {
    "no live slot": ([IDLE, waiting(live=0), IDLE], 0),
    "one waiting at n_frames == n_trail": ([waiting(), IDLE, IDLE], 1),
    "one id short of the boundary": ([waiting(nf=3), IDLE, IDLE], 0),
    "past the boundary": ([waiting(nf=6), waiting(), IDLE], 1),
    "a closed-trail slot keeps the batch running": ([waiting(), slot(n_trail=4, nf=4), IDLE], 0),
    "a plain slot keeps the batch running": ([waiting(), waiting(), slot(nf=2)], 0),
    "a finished open slot does not wait": ([waiting(fin=1), IDLE, IDLE], 0),
    "an open slot at max_frames does not wait": ([waiting(nf=16, n_trail=16), waiting(), IDLE], 0),
    "closed after the last id": ([waiting(host_open=0), IDLE, IDLE], 0),
    "a non-live slot that would run does not count": ([waiting(), slot(live=0, nf=1), waiting(n_trail=0, nf=0)], 1),
}


def test_stall_predicate(driver):
    names = list(STALL_CASES)
    out = driver("".join(slots_text("stall", STALL_CASES[n][0]) for n in names))
    for n, line in zip(names, out):
        assert int(line) == STALL_CASES[n][1] == stall_ref(STALL_CASES[n][0]), n


# dump order of the driver: the int fields, t_pos[4], the float fields
INT_NAMES = ["tseq", "tslot", "finished", "max_frames", "n_frames", "n_prompt", "mask", "top_k", "ptop_k", "n_trail", "open"]
FLT_NAMES = ["temp", "top_p", "pen", "ptemp", "ptop_p"]


def parse_row(line):
    w = line.split()
    assert w[0] == "row" and len(w) == 1 + 11 + 4 + 5
    d = dict(zip(INT_NAMES, (int(x) for x in w[1:12])))
    d["tpos"] = [int(x) for x in w[12:16]]
    d.update(zip(FLT_NAMES, (float(x) for x in w[16:])))
    return d


def idle_row(B):
    return dict(finished=1, max_frames=0, n_frames=0, n_prompt=0, mask=-1, temp=0.0, top_k=0, top_p=1.0, pen=1.0, ptemp=0.0, ptop_k=0, ptop_p=1.0,
                n_trail=0, open=0, tseq=B, tslot=0, tpos=[0, 0, 0, 0])


@pytest.mark.parametrize("B,b", [(4, 2), (1, 0), (19, 18)])
def test_slot_table_reset_load_route(driver, B, b):
    out = driver("table %d %d 3\n" % (B, b))
    fresh, loaded = parse_row(out[0]), parse_row(out[2])
    assert fresh == idle_row(B)
    assert out[1] == "req 1"
    # the request the driver loads: n_prompt 5, max_steps 77, mask_eos, sampler 0.625 / 13 / 0.75, options 1.5 / 0.25 / 9 / 0.5, n_trail 6, open
    assert loaded == dict(idle_row(B), finished=0, max_frames=77, n_frames=0, n_prompt=5, mask=EOS, temp=0.625, top_k=13, top_p=0.75, pen=1.5,
                          ptemp=0.25, ptop_k=9, ptop_p=0.5, n_trail=6, open=0)  # open: the host flag is the scheduler's, load() leaves it clear
    routed = [parse_row(x) for x in out[3:3 + B]]
    for s, r in enumerate(routed):
        if s == b:  # live, n_prompt 5 + n_frames 3
            assert (r["tseq"], r["tslot"], r["tpos"]) == (b, 8, [8, 8, 8, 0])
        else:       # idle: the scratch sequence
            assert r == idle_row(B)
    assert out[3 + B] == "req 1"  # reset() drops the request
    assert parse_row(out[4 + B]) == fresh


@pytest.mark.parametrize("B", [1, 4, 16, 17, 512])
def test_slot_table_layout(driver, B):
    w = [int(x) for x in driver("layout %d\n" % B)[0].split()]
    off, size = w[:-1], w[-1]
    assert len(off) == 18 and off[0] == 0 and off[-1] == size
    pad = lambda n: (n + 15) & ~15                              # words: every row is a multiple of 64 bytes
    assert sorted(b - a for a, b in zip(off, off[1:])) == sorted([pad(4 * B)] + [pad(B)] * 16)  # t_pos is [B][4], the other sixteen [B]
    assert size * 4 <= 40960 or B > 512                         # one upload: 40 KB at 512 slots


def test_prefill_packer(driver):
    lens, slots, n_max = [1, 4, 2, 5], [3, 0, 2, 1], 4
    out = driver("pack %d %d\n" % (n_max, len(lens)) + "".join("%d %d\n" % p for p in zip(lens, slots)))
    # restatement: the token stream of the wave, cut every n_max tokens
    stream = [(i, t) for i, n in enumerate(lens) for t in range(n)]
    chunks = [stream[k:k + n_max] for k in range(0, len(stream), n_max)]
    assert len(chunks) == 3 and out[-1] == "cursor %d 0" % len(lens)
    assert len(out) == 6 * len(chunks) + 1
    for c, toks in enumerate(chunks):
        head, seq, slot_, pos, lasts, stage = (out[6 * c + k].split() for k in range(6))
        assert head == ["chunk", str(len(toks))]
        assert seq == ["seq"] + [str(slots[i]) for i, t in toks]
        assert slot_ == ["slot"] + [str(t) for i, t in toks]
        assert pos == ["pos"] + [str(x) for i, t in toks for x in (t, t, t, 0)]
        assert lasts == ["lasts"] + ["%d:%d" % (i, k) for k, (i, t) in enumerate(toks) if t == lens[i] - 1]
        assert stage == ["stage"] + ["%g" % (100 * i + t) for i, t in toks] + ["-1"] * (n_max - len(toks))  # rows past n stay untouched
    # what this batch is for: a one-token prompt, prompts that straddle a chunk edge, the last one ending exactly on one
    assert chunks[0][0] == (0, 0) and chunks[1][0] == (1, 3) and chunks[1][-1][0] == 3 and chunks[2][0][0] == 3


def stage_ref(cap, sizes):
    """The staging cursor restated: 64-byte pieces handed out in order, nothing moves when a piece does not fit."""
    used, out = 0, []
    for b in sizes:
        if b < 0:
            used = 0
            out.append(("reset", 0))
            continue
        need = (b + 63) // 64 * 64
        if b > cap or used + need > cap:
            out.append((-1, used))
        else:
            out.append((used, used + need))
            used += need
    return out


def stage_run(driver, cap, sizes):
    out = driver("stage %d %d\n%s\n" % (cap, len(sizes), " ".join(str(b) for b in sizes)))
    assert len(out) == len(sizes)
    return [("reset", int(l.split()[1])) if l.startswith("reset") else tuple(int(x) for x in l.split()) for l in out]


def test_stage_cursor_offsets_are_aligned(driver):
    cap = 4096
    sizes = [1, 63, 64, 65, 0, 100, 128, 1000, 7, 640, 1, 1, 2000, 5, -1, 4000, 96, 1, -1, 33, 4033, 31]
    got = stage_run(driver, cap, sizes)
    assert got == stage_ref(cap, sizes)
    offsets = [at for at, _ in got if at not in ("reset", -1)]
    assert len(offsets) >= 15 and all(at % 64 == 0 for at in offsets)
    assert any(at == -1 for at, _ in got)                       # the sequence fills the arena at least once
    assert all(used % 64 == 0 and used <= cap for _, used in got)


def test_stage_cursor_exact_fit_and_one_byte_more(driver):
    # 256 bytes: 192 in use, then exactly the 64 that are left / one byte more than what is left
    assert stage_run(driver, 256, [192, 64]) == [(0, 192), (192, 256)]
    assert stage_run(driver, 256, [192, 65]) == [(0, 192), (-1, 192)]          # does not fit: the cursor stays
    assert stage_run(driver, 256, [192, 65, 64]) == [(0, 192), (-1, 192), (192, 256)]  # and still serves what does
    assert stage_run(driver, 256, [256, 1, 0]) == [(0, 256), (-1, 256), (256, 256)]    # a full arena: the whole of it, then nothing but nothing
    # a capacity that is no multiple of 64: the piece is rounded up, so the last 36 bytes serve nobody
    assert stage_run(driver, 100, [64, 1]) == [(0, 64), (-1, 64)]


def test_stage_cursor_refuses_what_no_arena_holds(driver):
    for before in ([], [64], [64, 64, 64, 64]):                 # whatever is in use: empty, partly, full
        got = stage_run(driver, 256, before + [257, 1 << 40])
        used = 64 * len(before)
        assert got[len(before):] == [(-1, used), (-1, used)]


def test_stage_cursor_reset(driver):
    got = stage_run(driver, 256, [100, 100, 100, -1, 10, -1, 256])
    assert got == [(0, 128), (128, 256), (-1, 256), ("reset", 0), (0, 64), ("reset", 0), (0, 256)]
