"""[EXT] KV cache type Q8_0, host side: the entry points exist, q3tts_kv_layout gives the byte counts of both cache types, plane pages are
whole 16-KiB tiles, unknown types and bad descriptors are refused, and without a device the op says so.  No GPU needed."""
import numpy as np
import pytest

import q3tts


def test_declared():
    new = ("q3tts_op_attention_q8kv", "q3tts_kv_layout", "q3tts_engine_create_kv", "q3tts_tf_open_kv")
    assert set(new) <= set(q3tts.SYMBOLS) and all(hasattr(q3tts.lib(), s) for s in new)
    assert q3tts.KV_TYPES == {"f16": 1, "q8_0": 8}   # ggml's type ids


@pytest.mark.parametrize("n_layer,n_kv,kv_type,per_token", [(28, 8, "f16", 114688), (28, 8, "q8_0", 60928), (2, 2, "f16", 2048), (2, 2, "q8_0", 1536)])
def test_layout(n_layer, n_kv, kv_type, per_token):
    """full size: 28 x 8 units of 16384 / 8704 bytes per plane page (1 949 696 = 119 x 16 KiB at Q8_0); the tiny model's 2 x 2 units of
    8704 bytes pad from 34 816 to 49 152"""
    bpt, page = q3tts.kv_layout(n_layer, n_kv, kv_type)
    assert bpt == per_token and page % 16384 == 0 and 2 * page == 64 * bpt
    assert page >= n_layer * n_kv * (16384 if kv_type == "f16" else 8704) > page - 16384


@pytest.mark.parametrize("kv_type", [0, 2, 9, -1])
def test_unknown_type(kv_type):
    with pytest.raises(q3tts.Q3Error, match="unknown KV cache type"):
        q3tts.kv_layout(28, 8, kv_type)


def _call(n_head=4, slot=5):
    z = np.zeros
    return q3tts.op_attention_q8kv(z((1, (n_head + 4) * 128), np.float32), z(128, np.float32), z(128, np.float32), z((1, 1, 2, 8192), np.int8),
                                   z((1, 1, 2, 256), np.uint16), z((1, 1, 2, 8192), np.int8), z((1, 1, 2, 256), np.uint16), n_head, 2, 1, 0,
                                   [0], [slot], z((1, 4), np.int32))


def test_refused_on_the_host():
    with pytest.raises(q3tts.Q3Error, match="1, 2, 4 or 8 query heads"):
        _call(n_head=6)
    with pytest.raises(q3tts.Q3Error, match="identity paging"):
        _call(slot=64)
    if q3tts.device_count() < 1:
        with pytest.raises(q3tts.Q3Error, match="no HIP device"):
            _call()
