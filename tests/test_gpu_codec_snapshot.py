"""[EXT] codec preambles, the codec half (q3tts_decoder_snapshot_create / _restore / _free; include/q3tts_spec.h "codec preambles", P4): a
snapshot is a device-side copy of one stream's whole state -- the history slots of every state tensor and the two counters -- made and put
back by k_hist_copy on the decoder's own HIP stream.  Everything here is bit for bit: a restored stream runs the same launches on the same
bytes as the snapshotted one, so a mismatch is a finding, not a tolerance.  Tiny codec (window 8: kv_len saturates at 7), four streams.

m in {1, 3, 4, 7, 8, 9, 13}: below, at and past the window, on and off the 4-frame chunk grid."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
A, B, C_, SCRATCH = 0, 1, 2, 3
MS = (1, 3, 4, 7, 8, 9, 13)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _feed(dec, stream, codes):
    """4-frame chunks, then the tail, as a Chunker cuts them; the PCM of all of them"""
    out = [dec.decode(codes[i: i + 4], stream=stream) for i in range(0, len(codes), 4)]
    return np.concatenate(out) if out else np.zeros(0, np.float32)


@pytest.fixture(scope="module")
def dec(gpu, tiny_model):
    d = gpu.Decoder(tiny_model + "/onnx/q3tts_codec.gguf", n_streams=4)
    yield d
    d.close()


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(7)
    f = dict(p=rng.integers(0, 2048, (13, 16)).astype(np.int64), c=rng.integers(0, 2048, (9, 16)).astype(np.int64),
             dirt=rng.integers(0, 2048, (5, 16)).astype(np.int64), other=rng.integers(0, 2048, (6, 16)).astype(np.int64))
    for v in f.values():
        v.setflags(write=False)
    return f


@pytest.mark.parametrize("m", MS)
def test_restored_stream_continues_the_snapshotted_one_bit_for_bit(gpu, dec, frames, m):
    p, c = frames["p"][:m], frames["c"]
    dec.reset(C_)
    _feed(dec, C_, frames["other"][:3])                   # the bystander has a state of its own
    blob_c = dec.state_export(C_)
    dec.reset(A)
    _feed(dec, A, p)
    snap = dec.snapshot_create(A)
    blob_a = dec.state_export(A)
    assert blob_a[-2] == min(m, 7) and blob_a[-1] == m    # counters: cached positions saturate at window - 1, frames seen
    pcm_a = _feed(dec, A, c)                              # 4, 4, 1
    _feed(dec, B, frames["dirt"])                         # B is left dirty by an unrelated decode (no reset)
    dec.snapshot_restore(snap, B)
    blob_b = dec.state_export(B)
    assert _same(blob_b, blob_a), "state after the restore differs from the state at the snapshot (m = %d)" % m
    pcm_b = _feed(dec, B, c)
    assert pcm_a.size == pcm_b.size == 9 * dec.spf and np.abs(pcm_a).max() > 0
    assert _same(pcm_a, pcm_b), "the restored stream's PCM differs (m = %d): %d samples" % (m, int((_bits(pcm_a) != _bits(pcm_b)).sum()))
    assert _same(dec.state_export(A), dec.state_export(B))                # and they stay together
    assert _same(dec.state_export(C_), blob_c), "snapshot / restore touched another stream"
    # the snapshot survives the reset (and the further decodes) of its source stream
    dec.reset(A)
    assert not _same(dec.state_export(A), blob_a)
    dec.snapshot_restore(snap, SCRATCH)
    assert _same(dec.state_export(SCRATCH), blob_a)
    dec.snapshot_free(snap)


def test_a_second_snapshot_is_unchanged_by_restores_of_the_first(gpu, dec, frames):
    dec.reset(A)
    _feed(dec, A, frames["p"][:5])
    s1, blob1 = dec.snapshot_create(A), dec.state_export(A)
    _feed(dec, A, frames["other"])
    s2, blob2 = dec.snapshot_create(A), dec.state_export(A)
    assert s1 != s2 and not _same(blob1, blob2)
    for stream in (B, C_, B):
        dec.snapshot_restore(s1, stream)
        assert _same(dec.state_export(stream), blob1)
    dec.snapshot_restore(s2, SCRATCH)
    assert _same(dec.state_export(SCRATCH), blob2)
    dec.snapshot_restore(s1, SCRATCH)                                     # and the other way round
    assert _same(dec.state_export(SCRATCH), blob1)
    # a freed slot is taken again by the next snapshot, which is as good as the first
    dec.snapshot_free(s1)
    s3 = dec.snapshot_create(SCRATCH)
    assert s3 == s1
    dec.reset(B)
    dec.snapshot_restore(s3, B)
    assert _same(dec.state_export(B), blob1)
    dec.snapshot_restore(s2, B)
    assert _same(dec.state_export(B), blob2)
    dec.snapshot_free(s2)
    dec.snapshot_free(s3)
    assert dec.snapshot_bytes() == (blob1.size - 2) * 4                   # the blob without its two counters


def test_every_refusal_leaves_the_state_alone(gpu, dec, frames):
    dec.reset(A)
    _feed(dec, A, frames["p"][:3])
    before = [dec.state_export(s) for s in range(4)]
    snap = dec.snapshot_create(A)
    for bad in (-1, 4, 1000):
        with pytest.raises(gpu.Q3Error, match="stream out of range"):
            dec.snapshot_create(bad)
        with pytest.raises(gpu.Q3Error, match="stream out of range"):
            dec.snapshot_restore(snap, bad)
    for bad in (-1, 64, 100000):
        with pytest.raises(gpu.Q3Error, match="snapshot out of range"):
            dec.snapshot_restore(bad, B)
        with pytest.raises(gpu.Q3Error, match="snapshot out of range"):
            dec.snapshot_free(bad)
    dec.snapshot_free(snap)
    with pytest.raises(gpu.Q3Error, match="freed"):
        dec.snapshot_restore(snap, B)
    with pytest.raises(gpu.Q3Error, match="freed"):
        dec.snapshot_free(snap)
    for s in range(4):
        assert _same(dec.state_export(s), before[s]), s
