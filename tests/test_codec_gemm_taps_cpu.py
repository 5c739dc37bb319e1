"""Host-only: which launches of the full-size decoder take k_conv_gemm_h3's tap-reusing main loop (q3tts_codec_gemm_tap_reuse, csrc/codec.hip).
No GPU needed."""
import pytest

from test_codec_gemm_plan_cpu import decoder_gemms

CONV1 = ["dec%d.ru%d.conv1" % (b, u) for b in range(4) for u in range(3)]


@pytest.mark.parametrize("G", (16, 32))
def test_every_k7_residual_conv_reuses_its_taps(q3, G):
    gemms = decoder_gemms(G)
    left_out = []   # launches the dispatcher does not give to the 128 x 96 tile: not part of the claim
    for name in CONV1:
        form, ks, red = q3.codec_gemm_plan(**gemms[name])
        if form not in ("H3", "H3_EPL"):
            left_out.append((name, form))
            continue
        assert (ks, red) == (1, -1), name
        assert q3.codec_gemm_tap_reuse(**gemms[name]) is True, name
    print("G = %d: not planned as H3 / H3_EPL: %s" % (G, left_out or "none"))
    if G == 16:
        assert not left_out   # tests/test_codec_gemm_plan_cpu.py::PLANS[16] pins all twelve to H3_EPL


@pytest.mark.parametrize("G", (1, 4, 16, 32))
def test_single_tap_launches_never_do(q3, G):
    for name, a in decoder_gemms(G).items():
        if a["taps"] == 1:
            assert q3.codec_gemm_tap_reuse(**a) is False, name


def test_split_k_and_other_forms_keep_the_tap_major_loop(q3):
    shape = dict(M=2048, N=768, cin=768, taps=7, dil=3, a_segT=128, a_skip=18)
    assert q3.codec_gemm_plan(**shape) == ("H3_EPL", 1, -1) and q3.codec_gemm_tap_reuse(**shape) is True
    for form in ("H3", "H3_EPL"):
        assert q3.codec_gemm_tap_reuse(form=form, **shape) is True
        for ks in (2, 3, 7):
            assert q3.codec_gemm_tap_reuse(form=form, ksplit=ks, reducer=1, **shape) is False, (form, ks)
    for form in ("H1", "H1_EPL", "H2", "H2_EPL", "F32_2"):
        assert q3.codec_gemm_tap_reuse(form=form, **shape) is False, form
    assert q3.codec_gemm_tap_reuse(form="H3", **dict(shape, taps=1)) is False
    # the halo of a tile: 128 rows + a_skip per segment boundary inside it + (taps - 1) * dil, at most 240 rows
    assert q3.codec_gemm_tap_reuse(form="H3", **dict(shape, dil=9, a_segT=64, a_skip=58)) is True     # 128 + 58 + 54 = 240
    assert q3.codec_gemm_tap_reuse(form="H3", **dict(shape, dil=9, a_segT=64, a_skip=59)) is False
    assert q3.codec_gemm_tap_reuse(form="H3", **dict(shape, dil=9, a_segT=128, a_skip=500)) is True   # tiles aligned to the segments: no boundary inside
    assert q3.codec_gemm_tap_reuse(form="H3", **dict(shape, M=100, dil=9, a_segT=64, a_skip=500)) is False
    assert q3.codec_gemm_tap_reuse(form="H3", **dict(shape, M=64, dil=9, a_segT=64, a_skip=500)) is True   # one short tile, one segment


def test_query_rejects_a_bad_descriptor(q3):
    with pytest.raises(q3.Q3Error):
        q3.codec_gemm_tap_reuse(0, 96, 96, 7)
