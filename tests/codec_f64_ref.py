"""The whole codec decoder restated with torch.nn.functional (conv1d / conv_transpose1d / layer_norm / gelu / softmax), independent of the C
oracle and of the product: codes [T][16] -> PCM [T * 1920].  In float32 it is the restatement test_codec_mel_oracle.py has always compared
the oracle with; in float64 (weights .double(), the cos / sin tables left in double) it is the reference the assembled GPU decoder is held
to frame by frame (test_gpu_codec_pcm_f64.py).  No oracle and no GPU in this file."""
import numpy as np
import torch

import ggml_ref as G

F = torch.nn.functional
SPF = 1920          # samples per frame

# The per-frame bounds of test_gpu_codec_pcm_f64.py, in units of the C oracle's own worst frame against float64 (the float32 floor):
# twice the worst ratio measured on the MI355X over all of that file's cases, rounded up (profiles/codec_pcm_f64.md).  Neither may
# pass K_CAP; a decoder that needs more is a finding, not a reason to move the cap.
K_CAP = 16
K_RMS = 12         # worst measured 5.67 (full-size group of 16)
K_MAX = 13         # worst measured 6.36 (the same case)

_model = {}         # path -> (kv, tensors): the last file read (the full-size codec is large; one at a time)
_weights = {}       # (path, dtype, name) -> tensor, for the file in _model


def _load(path):
    if path not in _model:
        _model.clear(), _weights.clear()
        _model[path] = G.read_gguf(path)
    return _model[path]


def _decode(path, codes, dtype):
    """codes: int64 tensor [B][T][16] -> tensor [B][T * 1920] of dtype.  One stream (B = 1) in float32 computes what torch_codec has
    computed since it was written: the same calls on the same shapes, in the same order."""
    kv, t = _load(path)

    def _w(name):
        key = (path, dtype, name)
        if key not in _weights:
            ty, ne, raw = t[name]
            _weights[key] = torch.from_numpy(np.array(raw).view(np.float32).reshape(list(reversed(ne))).copy()).to(dtype)
        return _weights[key]
    H, nh, hd, W = kv["codec.hidden"], kv["codec.n_heads"], kv["codec.head_dim"], kv["codec.window"]
    B, T = codes.shape[0], codes.shape[1]
    z = sum(_w("codec.codebook.%d" % q)[codes[:, :, q]] for q in range(16)).transpose(1, 2)          # [B,512,T]
    causal = lambda x, w, b, dil=1, groups=1: F.conv1d(F.pad(x, ((w.shape[-1] - 1) * dil, 0)), w, b, dilation=dil, groups=groups)
    h = causal(z, _w("codec.pre_conv.weight"), _w("codec.pre_conv.bias")).transpose(1, 2)            # [B,T,H]
    rms = lambda x, g: x * torch.rsqrt((x * x).mean(-1, keepdim=True) + kv["codec.eps"]) * g
    pos = torch.arange(T, dtype=torch.float64)
    inv = torch.tensor(kv["codec.rope_base"], dtype=torch.float64) ** (-torch.arange(hd // 2, dtype=torch.float64) / (hd // 2))
    ang = pos[:, None] * inv[None]
    cs, sn = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)

    def rope(x):  # [B, T, nh, hd]
        a, b = x[..., : hd // 2], x[..., hd // 2:]
        return torch.cat([a * cs[:, None] - b * sn[:, None], b * cs[:, None] + a * sn[:, None]], -1)
    idx = torch.arange(T)
    mask = (idx[None] <= idx[:, None]) & (idx[:, None] - idx[None] < W)
    for l in range(kv["codec.n_layers"]):
        p = "codec.tf.%d." % l
        xn = rms(h, _w(p + "attn_norm"))
        q = rope((xn @ _w(p + "wq").T).view(B, T, nh, hd)); k = rope((xn @ _w(p + "wk").T).view(B, T, nh, hd))
        v = (xn @ _w(p + "wv").T).view(B, T, nh, hd)
        s = torch.einsum("bthd,bshd->bhts", q, k) / hd ** 0.5
        s = s.masked_fill(~mask[None, None], float("-inf"))
        a = torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), v).reshape(B, T, nh * hd)
        h = h + _w(p + "ls_attn") * (a @ _w(p + "wo").T)
        xn = rms(h, _w(p + "ffn_norm"))
        h = h + _w(p + "ls_ffn") * ((F.silu(xn @ _w(p + "w_gate").T) * (xn @ _w(p + "w_up").T)) @ _w(p + "w_down").T)
    x = rms(h, _w("codec.tf.norm")).transpose(1, 2)                                                  # [B,H,T]

    def convt(x, w, b, s):  # keep the first T*s outputs (right trim k-s): the streamable causal form
        y = F.conv_transpose1d(x, w, b, stride=s)
        return y[..., : x.shape[-1] * s]
    for i in range(kv["codec.n_up"]):
        p = "codec.up.%d." % i
        x = convt(x, _w(p + "convt.weight"), _w(p + "convt.bias"), kv["codec.up_ratio.%d" % i])
        d = causal(x, _w(p + "dw.weight").unsqueeze(1), _w(p + "dw.bias"), groups=H)
        d = F.layer_norm(d.transpose(1, 2), (H,), _w(p + "ln.weight"), _w(p + "ln.bias"), 1e-6)
        d = F.gelu(d @ _w(p + "pw1.weight").T + _w(p + "pw1.bias")) @ _w(p + "pw2.weight").T + _w(p + "pw2.bias")
        x = x + (_w(p + "gamma") * d).transpose(1, 2)
    snake = lambda x, a, b: x + (1.0 / (torch.exp(b) + 1e-9))[None, :, None] * torch.sin(x * torch.exp(a)[None, :, None]) ** 2
    x = causal(x, _w("codec.dec.conv_in.weight"), _w("codec.dec.conv_in.bias"))
    for b in range(kv["codec.n_dec"]):
        p = "codec.dec.%d." % b
        r = kv["codec.dec_rate.%d" % b]
        x = convt(snake(x, _w(p + "snake.alpha"), _w(p + "snake.beta")), _w(p + "convt.weight"), _w(p + "convt.bias"), r)
        for u, dil in enumerate((1, 3, 9)):
            q = p + "ru.%d." % u
            y = causal(snake(x, _w(q + "snake1.alpha"), _w(q + "snake1.beta")), _w(q + "conv1.weight"), _w(q + "conv1.bias"), dil)
            y = causal(snake(y, _w(q + "snake2.alpha"), _w(q + "snake2.beta")), _w(q + "conv2.weight"), _w(q + "conv2.bias"))
            x = x + y
    x = causal(snake(x, _w("codec.dec.snake_out.alpha"), _w("codec.dec.snake_out.beta")), _w("codec.dec.conv_out.weight").reshape(1, -1, 7),
               _w("codec.dec.conv_out.bias").reshape(1))
    return x.clamp(-1, 1)[:, 0]


def _codes(c):
    c = c if torch.is_tensor(c) else torch.from_numpy(np.array(c))
    return c.to(torch.int64).reshape(-1, 16)


def torch_codec(path, codes, dtype=torch.float32, prime=None):
    """codes: one [T][16] array (or tensor) of codes in 0..2047, or a list of them (streams; the lengths may differ).
    prime: for a stream that starts behind k earlier frames, their codes [k][16] (one array for one stream, a list with None or an array per
    stream for a list): the concatenation is decoded and its first k * 1920 samples are dropped.
    Returns a numpy array [T * 1920] of dtype, or a list of them.  Streams whose concatenations are equally long go through torch as one
    batch."""
    single = not isinstance(codes, (list, tuple))
    streams = [_codes(codes)] if single else [_codes(c) for c in codes]
    primes = [prime] if single else (list(prime) if prime is not None else [None] * len(streams))
    assert len(primes) == len(streams)
    whole, cut = [], []
    for c, p in zip(streams, primes):
        p = _codes(p) if p is not None else c[:0]
        whole.append(torch.cat([p, c]))
        cut.append(p.shape[0] * SPF)
    out = [None] * len(streams)
    with torch.no_grad():
        for n in sorted(set(w.shape[0] for w in whole)):
            ids = [i for i, w in enumerate(whole) if w.shape[0] == n]
            pcm = _decode(path, torch.stack([whole[i] for i in ids]), dtype).numpy()
            for j, i in enumerate(ids):
                out[i] = pcm[j, cut[i]:].copy()
    return out[0] if single else out


def frame_errors(got, ref):
    """(per-frame RMS, per-frame max abs) of got - ref, float64 arrays of one entry per 1920-sample frame"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape and got.size % SPF == 0, (got.shape, ref.shape)
    d = (got - ref).reshape(-1, SPF)
    return np.sqrt(np.mean(d * d, axis=1)), np.abs(d).max(axis=1)
